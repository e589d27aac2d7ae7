"""Fused SGD with Nesterov momentum (and `FusedAdam`, below) over the model's flat arenas.

Counterpart of `optim.SGD(model.parameters(), lr, momentum, nesterov=True,
weight_decay)` as configured in Our_UNet/src/train.py:445-451.  When every
parameter and gradient is a view into the `UNet` arenas the whole step is ONE
kernel launch over 19.66 M floats; otherwise each parameter gets its own launch
of the same kernel.  `state_dict()` keeps torch's SGD layout
(`state[i]['momentum_buffer']`, `param_groups`) so checkpoints interchange.
"""
import torch

from . import ops


class FusedSGD(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0,
                 nesterov=False, model=None):
        if dampening != 0.0:
            raise NotImplementedError("FusedSGD implements dampening == 0 (the reference setting)")
        if nesterov and momentum <= 0:
            raise ValueError("Nesterov momentum requires a momentum")
        if not nesterov:
            raise NotImplementedError("FusedSGD implements the Nesterov form used by the reference")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                        nesterov=nesterov)
        super().__init__(params, defaults)
        self._model = model
        self._flat_buf = None
        self._steps = 0
        self.grad_scale = 1.0
        # graph-captured steps (train.GraphedTrainStep): lr / momentum / weight decay / grad_scale
        # are read by the kernel from this device tensor, refreshed by sync_device_hyper()
        self._hyper = None
        self._hyper_host = None

    def use_device_hyper(self, on=True):
        """Make the flat-arena step read its hyper-parameters from device memory, so that a step
        captured in a HIP graph follows later changes of `param_groups[0]['lr']` (LR schedule).
        The device tensor is created once and kept: a graph captured earlier keeps reading the
        same address when a second GraphedTrainStep is built on this optimizer."""
        if not on:
            self._hyper = self._hyper_host = None
            return
        if self._hyper is None:
            arena, _ = self._model.flat_parameters()
            self._hyper = torch.zeros(4, dtype=torch.float32, device=arena.device)
            self._hyper_host = None
        self.sync_device_hyper()

    def sync_device_hyper(self):
        """Copy {lr, momentum, weight_decay, grad_scale} to the device tensor if they changed."""
        if self._hyper is None:
            return
        g = self.param_groups[0]
        vals = (float(g["lr"]), float(g["momentum"]), float(g["weight_decay"]),
                float(self.grad_scale))
        if vals != self._hyper_host:
            self._hyper.copy_(torch.tensor(vals, dtype=torch.float32))
            self._hyper_host = vals

    def _flat_ready(self):
        """True when one launch over the arenas is equivalent to the per-parameter update."""
        m = self._model
        if m is None or len(self.param_groups) != 1:
            return False
        arena, garena = m.flat_parameters()
        params = self.param_groups[0]["params"]
        if len(params) != len(m._offsets):
            return False
        base, gbase = arena.data_ptr(), garena.data_ptr()
        for p, off in zip(params, m._offsets):
            if p.grad is None or p.data_ptr() != base + 4 * off or \
                    p.grad.data_ptr() != gbase + 4 * off:
                return False
        return True

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._flat_buf = None      # adopt the loaded momentum buffers on the next step

    @torch.no_grad()
    def adopt_flat_momentum(self):
        """Build the flat momentum arena (one buffer aliased by every state[p]['momentum_buffer'])
        without taking a step.  Buffers that already exist - a checkpoint loaded through
        load_state_dict - are copied in.  Returns True when none existed (zero momentum: the next
        step is torch SGD's "first step", buf <- g).  No-op (returns None) once the arena exists."""
        if self._flat_buf is not None:
            return None
        m = self._model
        g = self.param_groups[0]
        arena, _ = m.flat_parameters()
        if len(self.param_groups) != 1 or len(g["params"]) != len(m._offsets):
            raise RuntimeError("the flat momentum arena needs one parameter group holding every "
                               "parameter of the model")
        self._flat_buf = torch.zeros_like(arena)
        fresh = True
        for p, off in zip(g["params"], m._offsets):
            st = self.state[p]
            if "momentum_buffer" in st and st["momentum_buffer"] is not None:
                # resumed from a checkpoint: adopt the loaded buffers
                self._flat_buf[off:off + p.numel()].view_as(p).copy_(st["momentum_buffer"])
                fresh = False
            st["momentum_buffer"] = self._flat_buf[off:off + p.numel()].view_as(p)
        return fresh

    # graph capture (train.GraphedTrainStep): what a throw-away warm-up step changes
    def _snapshot(self):
        self.adopt_flat_momentum()
        return self._flat_buf.detach().clone(), self._steps

    def _restore(self, snap):
        self._flat_buf.copy_(snap[0])
        self._steps = snap[1]

    def _advanced(self):
        self._steps += 1

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        flat = self._flat_ready()
        if not flat and self.grad_scale != 1.0 and self._model is not None:
            # grad_scale is set by the data-parallel wrapper, which all-reduces the ARENA: a
            # gradient that left the arena was not reduced
            m = self._model
            _, garena = m.flat_parameters()
            for (name, p), off in zip(m.named_parameters(), m._offsets):
                if p.grad is not None and p.grad.data_ptr() != garena.data_ptr() + 4 * off:
                    raise RuntimeError(f"{name}.grad does not alias the gradient arena the "
                                       "all-reduce operates on")
        if flat:
            g = self.param_groups[0]
            arena, garena = self._model.flat_parameters()
            first = bool(self.adopt_flat_momentum())
            if self._hyper is not None:
                # (an eager step after a GraphedTrainStep was built - a last batch of another
                # shape, a data-parallel path that sets grad_scale - must not run on stale
                # values; no-op when nothing changed, so also inside a capture)
                self.sync_device_hyper()
                ops.sgd_nesterov_step_dev(arena, garena, self._flat_buf, self._hyper, first)
            else:
                ops.sgd_nesterov_step(arena, garena, self._flat_buf, g["lr"], g["momentum"],
                                      g["weight_decay"], first, self.grad_scale)
        else:
            if self._hyper is not None:
                raise RuntimeError("device-side hyper-parameters need the flat-arena step (every "
                                   "parameter and gradient a view of the UNet arenas)")
            for g in self.param_groups:
                for p in g["params"]:
                    if p.grad is None:
                        continue
                    st = self.state[p]
                    first = "momentum_buffer" not in st or st["momentum_buffer"] is None
                    if first:
                        st["momentum_buffer"] = torch.zeros_like(p)
                    if p.data_ptr() % 16 or p.grad.data_ptr() % 16 or not p.is_contiguous() \
                            or not p.grad.is_contiguous():
                        raise RuntimeError("FusedSGD needs contiguous, 16-byte aligned tensors")
                    ops.sgd_nesterov_step(p.data.view(-1), p.grad.view(-1),
                                          st["momentum_buffer"].view(-1), g["lr"], g["momentum"],
                                          g["weight_decay"], first, self.grad_scale)
        self._steps += 1
        return loss


def _torch_adam_defaults():
    """param_groups keys of the installed torch's Adam (so state_dicts interchange)."""
    probe = torch.optim.Adam([torch.zeros(1, requires_grad=True)])
    return dict(probe.defaults)


class FusedAdam(torch.optim.Optimizer):
    """`optim.Adam(params, lr, betas, eps, weight_decay)` (AE_pretrained/reconstruction/src/
    train.py:377-397: amsgrad = maximize = False, coupled L2 weight decay) on the HIP path.

    When every parameter and gradient is a view into the model's arenas the step is ONE launch
    over the flat arena (`exp_avg` / `exp_avg_sq` are views of two flat moment arenas); otherwise
    each parameter gets its own launch of the same kernel.  lr, betas, eps, weight_decay,
    grad_scale and the step count are ALWAYS read from one fp64 device tensor, refreshed by
    `sync_device_hyper()` when they change on the host and advanced by the step itself on the
    device, so a step captured in a HIP graph (GraphedTrainStep) follows an LR schedule and the bias
    correction without re-capture.  That tensor is created once and never dropped.

    One step count is kept for the whole optimizer (torch keeps one per parameter; they agree
    whenever every parameter has a gradient at every step, the training loop's case).
    `state_dict()` has torch's Adam layout (`state[i] = {step, exp_avg, exp_avg_sq}`, the installed
    torch's `param_groups` keys): checkpoints load into torch.optim.Adam and back.
    """

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0,
                 amsgrad=False, *, maximize=False, decoupled_weight_decay=False, model=None,
                 **kwargs):
        if amsgrad:
            raise NotImplementedError("FusedAdam implements amsgrad=False (the reference setting)")
        if maximize:
            raise NotImplementedError("FusedAdam implements maximize=False")
        if decoupled_weight_decay:
            raise NotImplementedError("FusedAdam implements coupled (L2) weight decay; "
                                      "decoupled_weight_decay (AdamW) is not on the HIP path")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        for k in ("foreach", "fused", "capturable", "differentiable"):
            if kwargs.get(k):
                raise NotImplementedError(f"FusedAdam has no '{k}' variant (it is one HIP kernel)")
        defaults = _torch_adam_defaults()
        defaults.update(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise NotImplementedError("FusedAdam takes one parameter group")
        self._model = model
        self._flat_m = self._flat_v = None
        self._steps = 0            # completed steps (the device step count after them)
        self.grad_scale = 1.0
        self._hyper = None         # fp64 [8] {lr, beta1, beta2, eps, wd, grad_scale, step, -}
        self._hyper_host = None    # what the device tensor holds

    # -- device hyper-parameters ---------------------------------------------------------------
    def _device(self):
        return self.param_groups[0]["params"][0].device

    def use_device_hyper(self, on=True):
        """Kept for FusedSGD's interface: FusedAdam always reads its hyper-parameters from the
        device tensor.  `on=False` changes nothing - the tensor stays alive, so a graph captured
        earlier never reads freed memory."""
        self.sync_device_hyper()

    def sync_device_hyper(self):
        """Copy {lr, betas, eps, weight_decay, grad_scale, step} to the device tensor if they
        changed (no-op otherwise, so also inside a graph capture)."""
        if self._hyper is None:
            self._hyper = torch.zeros(8, dtype=torch.float64, device=self._device())
        g = self.param_groups[0]
        vals = (float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                float(g["weight_decay"]), float(self.grad_scale), float(self._steps), 0.0)
        if vals != self._hyper_host:
            self._hyper.copy_(torch.tensor(vals, dtype=torch.float64))
            self._hyper_host = vals

    def _advanced(self):
        """The device advanced its step count: follow it on the host."""
        self._steps += 1
        if self._hyper_host is not None:
            h = list(self._hyper_host)
            h[6] += 1.0
            self._hyper_host = tuple(h)

    # -- flat moment arenas --------------------------------------------------------------------
    def _flat_ready(self):
        m = self._model
        if m is None:
            return False
        arena, garena = m.flat_parameters()
        params = self.param_groups[0]["params"]
        if len(params) != len(m._offsets):
            return False
        base, gbase = arena.data_ptr(), garena.data_ptr()
        for p, off in zip(params, m._offsets):
            if p.grad is None or p.data_ptr() != base + 4 * off or \
                    p.grad.data_ptr() != gbase + 4 * off:
                return False
        return True

    @torch.no_grad()
    def adopt_flat_moments(self):
        """Build the two flat moment arenas (aliased by every state[p]['exp_avg'] /
        ['exp_avg_sq']) without taking a step; moments that already exist (a checkpoint) are
        copied in.  No-op once the arenas exist."""
        if self._flat_m is not None:
            return
        m = self._model
        g = self.param_groups[0]
        arena, _ = m.flat_parameters()
        if len(g["params"]) != len(m._offsets):
            raise RuntimeError("the flat moment arenas need one parameter group holding every "
                               "parameter of the model")
        self._flat_m, self._flat_v = torch.zeros_like(arena), torch.zeros_like(arena)
        for p, off in zip(g["params"], m._offsets):
            st = self.state[p]
            for key, flat in (("exp_avg", self._flat_m), ("exp_avg_sq", self._flat_v)):
                view = flat[off:off + p.numel()].view_as(p)
                if st.get(key) is not None:
                    view.copy_(st[key])
                st[key] = view

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._flat_m = self._flat_v = None     # adopt the loaded moments on the next step
        steps = [float(st["step"]) for st in self.state.values() if "step" in st]
        self._steps = int(max(steps)) if steps else 0

    def state_dict(self):
        for p in self.param_groups[0]["params"]:
            st = self.state.get(p)
            if st:
                st["step"] = torch.tensor(float(self._steps), dtype=torch.float32)
        return super().state_dict()

    # graph capture (train.GraphedTrainStep): what a throw-away warm-up step changes
    def _snapshot(self):
        self.adopt_flat_moments()
        self.sync_device_hyper()
        return (self._flat_m.clone(), self._flat_v.clone(), self._hyper.clone(), self._steps,
                self._hyper_host)

    def _restore(self, snap):
        m, v, hyper, steps, host = snap
        self._flat_m.copy_(m)
        self._flat_v.copy_(v)
        self._hyper.copy_(hyper)
        self._steps, self._hyper_host = steps, host

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        flat = self._flat_ready()
        if not flat and self.grad_scale != 1.0 and self._model is not None:
            m = self._model
            _, garena = m.flat_parameters()
            for (name, p), off in zip(m.named_parameters(), m._offsets):
                if p.grad is not None and p.grad.data_ptr() != garena.data_ptr() + 4 * off:
                    raise RuntimeError(f"{name}.grad does not alias the gradient arena the "
                                       "all-reduce operates on")
        self.sync_device_hyper()
        if flat:
            arena, garena = self._model.flat_parameters()
            self.adopt_flat_moments()
            ops.adam_step(arena, garena, self._flat_m, self._flat_v, self._hyper, True)
        else:
            first = True
            for p in self.param_groups[0]["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("FusedAdam does not support sparse gradients")
                st = self.state[p]
                if st.get("exp_avg") is None:
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                if not (p.is_contiguous() and p.grad.is_contiguous() and
                        st["exp_avg"].is_contiguous() and st["exp_avg_sq"].is_contiguous()):
                    raise RuntimeError("FusedAdam needs contiguous tensors")
                ops.adam_step(p.data.view(-1), p.grad.view(-1), st["exp_avg"].view(-1),
                              st["exp_avg_sq"].view(-1), self._hyper, first)
                first = False
            if first:          # no gradient at all: nothing stepped
                return loss
        self._advanced()
        return loss
