"""Drop-in `SimpleLoss` (reference: Our_UNet/models/losses.py:5-121).

Dice + cross-entropy with per-batch inverse-frequency class weights and
ignore_index handling.  `forward(logits[N,3,H,W] fp32, target[N,H,W] int64)`
returns a 0-dim fp32 tensor supporting `.backward()` / `.item()`; with
`target_layout="u8"` the target is the dataset's uint8 mask itself.  One fused
kernel sequence computes the loss AND dL/dlogits in the forward call; autograd's
backward only scales that stored gradient.
"""
import torch
import torch.nn as nn

from . import ops


class _LossFunction(torch.autograd.Function):
    """Forward: the loss value and, in the workspace, the class weights / Dice coefficients the
    gradient needs.  Backward: ONE launch of the gradient kernel with autograd's upstream scalar
    applied inside it (`unet_dice_wce_loss_grad`) - no stock-torch scaling pass over dlogits."""

    @staticmethod
    def forward(ctx, logits, target, mod, class_weights):
        want_grad = ctx.needs_input_grad[0]
        world = mod._world()
        if world > 1:      # (K != 3 was refused in SimpleLoss.forward)
            import torch.distributed as dist
            stats, ws = ops.dice_wce_loss_shard_stats(logits, target, mod.smooth, mod.ignore_index)
            dist.all_reduce(stats, op=dist.ReduceOp.SUM, group=mod.process_group)
            out, _ = ops.dice_wce_loss_shard_apply(
                logits, target, stats, logits.shape[0] * world, ws, mod.smooth, mod.weight_dice,
                mod.weight_ce, mod.ignore_index, mod.dynamic_weights, class_weights=class_weights,
                grad_scale=mod.grad_scale, want_grad=False)
        else:
            ws = ops.dice_wce_loss_workspace(logits)
            out, _ = ops.dice_wce_loss_fwd_bwd(
                logits, target, mod.smooth, mod.weight_dice, mod.weight_ce, mod.ignore_index,
                mod.dynamic_weights, class_weights=class_weights, grad_scale=mod.grad_scale,
                want_grad=False, ws=ws)
        if want_grad:
            ctx.held = (logits, target, ws, mod.ignore_index)
        # [total, ce, dice, w0, w1, w2, -, -] on device (no sync); K != 3: [total, ce, dice, w[K]]
        mod.last_terms = out
        return out[0].clone()

    @staticmethod
    def backward(ctx, g):
        logits, target, ws, ignore_index = ctx.held
        ctx.held = None
        # g is the 0-dim upstream gradient (1 for loss.backward()), read on the device
        return ops.dice_wce_loss_grad(logits, target, ws, g, ignore_index), None, None, None


class SimpleLoss(nn.Module):
    def __init__(self, weight_dice=1.0, weight_ce=1.0, ignore_index=255, smooth=1e-5,
                 class_weights=None, dynamic_weights=True, batch_sync="local", process_group=None,
                 target_layout="int64"):
        """`target_layout="u8"`: the target is the dataset's uint8 [N,H,W] mask on the device,
        handed to the kernels untouched (1 byte a pixel instead of 8; a raw mask is cleaned on
        load with the dataset's rule v > 2 and v != 255 -> 0).  The loss, `last_terms` and the
        gradient equal those of the default layout on the cleaned mask bit for bit.

        `batch_sync="global"` (data parallel only; not in the reference, which is
        single-process): every rank evaluates the loss of the CONCATENATED batch - class weights,
        CE denominator and the Dice batch mean taken over all ranks' images (equal per-rank batch
        sizes) - so that N ranks x batch b reproduce one process at batch N*b.  Gradients must
        then be summed, not averaged: `ddp.GradBucketAllReduce(..., average=False)`."""
        super().__init__()
        if batch_sync not in ("local", "global"):
            raise ValueError("batch_sync must be 'local' or 'global'")
        if target_layout not in ("int64", "u8"):
            raise ValueError("target_layout must be 'int64' or 'u8'")
        self.target_layout = target_layout
        self.batch_sync = batch_sync
        self.process_group = process_group
        self.weight_dice = weight_dice
        self.weight_ce = weight_ce
        self.ignore_index = ignore_index
        self.smooth = smooth
        self.class_weights = class_weights
        self.dynamic_weights = dynamic_weights
        self.grad_scale = 1.0  # data-parallel training pre-scales the gradient by 1/world
        self.last_terms = None

    def _world(self):
        if self.batch_sync != "global":
            return 1
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return 1
        return dist.get_world_size(self.process_group)

    def forward(self, input, target):
        # (what this class count does not cover is refused first, before the device is touched)
        K = input.shape[1]
        ops._check_classes(K, "SimpleLoss")
        if K != 3 and self.batch_sync == "global":
            raise NotImplementedError("SimpleLoss(batch_sync='global'), the sharded loss, "
                                      f"covers exactly 3 classes (got {K})")
        if not bool(self.dynamic_weights) and self.class_weights is not None and \
                len(self.class_weights) != K:
            raise ValueError(f"class_weights holds {len(self.class_weights)} values for {K} "
                             "classes")
        if not input.is_cuda:
            raise RuntimeError("unet-implementations_amd.SimpleLoss runs on MI355X only "
                               "(no CPU fallback exists)")
        if input.shape[-2:] != target.shape[-2:]:
            # the reference resizes the logits to the target (Our_UNet/models/losses.py:66-68)
            input = ops.resize_bilinear(input, target.shape[-2:])
        if self.target_layout == "u8":
            if target.dtype != torch.uint8 or not target.is_cuda or not target.is_contiguous():
                raise TypeError("target_layout='u8' takes a contiguous uint8 device tensor")
        elif target.dtype != torch.int64:
            target = target.long()
        cw = None
        dynamic = bool(self.dynamic_weights) and target.size(0) > 0
        if not dynamic and self.class_weights is not None:
            cw = torch.as_tensor(self.class_weights, dtype=torch.float32,
                                 device=input.device).contiguous()
        mod = self
        if dynamic != bool(self.dynamic_weights):
            raise NotImplementedError("empty batch")
        return _LossFunction.apply(input.contiguous().float(), target.contiguous(), mod, cw)


class _MSEFunction(torch.autograd.Function):
    """Forward: the loss and the per-image sums of squares (unet_mse_loss_fwd).  Backward: ONE
    launch of the gradient kernel with autograd's upstream scalar applied inside it."""

    @staticmethod
    def forward(ctx, output, target, mod, target_u8):
        loss, per_image = ops.mse_loss_fwd(output, target, target_u8)
        mod.last_per_image = per_image      # fp64 [N] on the device (no sync)
        if ctx.needs_input_grad[0]:
            ctx.held = (output, target, target_u8)
        return loss[0].clone()

    @staticmethod
    def backward(ctx, g):
        output, target, target_u8 = ctx.held
        ctx.held = None
        return ops.mse_loss_grad(output, target, g, target_u8), None, None, None


class MSELoss(nn.Module):
    """`nn.MSELoss()` (reduction "mean") on the HIP path: the autoencoder's loss
    (AE_pretrained/reconstruction/src/train.py:420-437).  `forward(output[N,C,H,W] fp32, target)`
    returns a 0-dim fp32 tensor supporting `.backward()`.  The target is the NCHW fp32 tensor, or -
    with `target_layout="nhwc_u8"` - the dataset's uint8 [N,H,W,3] image itself, read as
    v / 255 rounded once to fp32 (what the reference's CPU dataset computes for
    `image.float() / 255.0`: the two forms give the same loss bit for bit).  `last_per_image` keeps the per-image sums of squared differences (fp64,
    on the device) of the last call."""

    def __init__(self, size_average=None, reduce=None, reduction="mean", target_layout="nchw"):
        super().__init__()
        if size_average is not None or reduce is not None or reduction != "mean":
            raise NotImplementedError("MSELoss on the HIP path implements reduction='mean' "
                                      "(the reference setting)")
        if target_layout not in ("nchw", "nhwc_u8"):
            raise ValueError("target_layout must be 'nchw' or 'nhwc_u8'")
        self.reduction = reduction
        self.target_layout = target_layout
        self.last_per_image = None

    def forward(self, input, target):
        if not input.is_cuda:
            raise RuntimeError("unet-implementations_amd.MSELoss runs on MI355X only "
                               "(no CPU fallback exists)")
        if input.dim() != 4:
            raise ValueError("expected an NCHW output")
        u8 = self.target_layout == "nhwc_u8"
        if not u8 and target.dtype != torch.float32:
            target = target.float()
        return _MSEFunction.apply(input.contiguous().float(), target.contiguous(), self, u8)


class _SSIMFunction(torch.autograd.Function):
    """Forward: one fused pass for w_ssim * (1 - SSIM) + w_mse * MSE and the per-image SSIM and
    sums of squares (unet_ssim_fwd).  Backward: ONE launch of the gradient kernel with both weights
    and autograd's upstream (a scalar, or one value per image) applied inside it."""

    @staticmethod
    def forward(ctx, output, target, mod, target_u8, w_ssim, w_mse, per_image):
        loss, ssim, sq = ops.ssim_fwd(output, target, target_u8, w_ssim=w_ssim, w_mse=w_mse,
                                      want_loss=not per_image)
        mod.last_ssim_per_image = ssim      # fp64 [N] on the device (no sync)
        mod.last_per_image = sq
        if ctx.needs_input_grad[0]:
            ctx.held = (output, target, target_u8, w_ssim, w_mse, per_image)
        if per_image:
            return (1.0 - ssim).float()
        return loss[0].clone()

    @staticmethod
    def backward(ctx, g):
        output, target, target_u8, w_ssim, w_mse, per_image = ctx.held
        ctx.held = None
        d = ops.ssim_grad(output, target, g, per_image, target_u8, w_ssim=w_ssim, w_mse=w_mse)
        return d, None, None, None, None, None, None


def _check_input(name, input, target_layout):
    if not input.is_cuda:
        raise RuntimeError(f"unet-implementations_amd.{name} runs on MI355X only "
                           "(no CPU fallback exists)")
    if input.dim() != 4:
        raise ValueError("expected an NCHW output")
    return input.contiguous().float()


class SSIMLoss(nn.Module):
    """`SSIMLoss` (AE_pretrained/reconstruction/models/losses.py:178-245) on the HIP path:
    1 - SSIM with the 11-tap Gaussian window (sigma 1.5), C1 = 0.01^2, C2 = 0.03^2, zero padding.
    `size_average=True` returns a 0-dim fp32 tensor (1 - the mean SSIM over N*C*H*W);
    `size_average=False` one value per image [N].  The reference's constructor raises (its window
    builder calls torch.exp on a Python float); this implements the window it evidently intends,
    which equals utils/metrics.py's gaussian_kernel(11, 1.5).  `target_layout` as `MSELoss`.
    `last_ssim_per_image` / `last_per_image` keep the per-image SSIM and sums of squared
    differences (fp64, on the device) of the last call."""

    def __init__(self, window_size=11, size_average=True, target_layout="nchw"):
        super().__init__()
        if window_size != 11:
            raise NotImplementedError("the HIP SSIM kernels implement window_size=11")
        if target_layout not in ("nchw", "nhwc_u8"):
            raise ValueError("target_layout must be 'nchw' or 'nhwc_u8'")
        self.window_size = window_size
        self.size_average = size_average
        self.channel = 3
        self.target_layout = target_layout
        self.last_ssim_per_image = None
        self.last_per_image = None

    def forward(self, output, target):
        output = _check_input("SSIMLoss", output, self.target_layout)
        u8 = self.target_layout == "nhwc_u8"
        if not u8 and target.dtype != torch.float32:
            target = target.float()
        return _SSIMFunction.apply(output, target.contiguous(), self, u8, 1.0, 0.0,
                                   not self.size_average)


# torchvision's VGG configuration "D" (vgg16): channels of the 3x3 convolutions, "M" = MaxPool2d(2, 2)
_VGG16_CFG = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M")
# index of each named ReLU inside vgg16().features (models/losses.py:103-109)
_VGG16_LAYER_MAP = {
    "relu1_1": 1, "relu1_2": 3,
    "relu2_1": 6, "relu2_2": 8,
    "relu3_1": 11, "relu3_2": 13, "relu3_3": 15,
    "relu4_1": 18, "relu4_2": 20, "relu4_3": 22,
    "relu5_1": 25, "relu5_2": 27, "relu5_3": 29,
}


def _vgg16_features(depth):
    """The 31 stock modules of torchvision's vgg16().features with its initialisation
    (kaiming_normal_(fan_out, relu), bias 0) drawn in layer order from torch's global generator
    for the convolutions among the first `depth` modules only."""
    mods, cin = [], 3
    for v in _VGG16_CFG:
        if v == "M":
            mods.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            mods += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    for m in mods[:depth]:
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            nn.init.constant_(m.bias, 0)
    return mods


class _PerceptualFunction(torch.autograd.Function):
    """Forward: the loss and - when the output needs a gradient - the trunk's backward, chunk by
    chunk, leaving only the unscaled dL/doutput.  Backward: that gradient times autograd's
    upstream scalar, on the device."""

    @staticmethod
    def forward(ctx, output, target, mod, target_u8, want_grad):
        # want_grad is decided by the caller: grad mode is always off in here, and
        # ctx.needs_input_grad mirrors output.requires_grad even under torch.no_grad()
        loss, dout = mod._run(output, target, target_u8, want_grad)
        ctx.dout = dout
        return loss

    @staticmethod
    def backward(ctx, g):
        # (dout is kept: a second backward through a retained graph scales it again)
        if ctx.dout is None:
            raise RuntimeError("PerceptualLoss: the forward call formed no gradient (it ran with "
                               "autograd disabled)")
        return ctx.dout * g, None, None, None, None


class PerceptualLoss(nn.Module):
    """`PerceptualLoss` (AE_pretrained/reconstruction/models/losses.py:82-168) on the HIP path:
    the mean over the tapped layers of the MSE between VGG16 features of the normalised output and
    target, a 0-dim fp32 tensor.  The reference builds `models.vgg16(weights=None)`: a randomly
    initialised, frozen network used as a fixed random feature extractor, so the term is fully
    defined by code (a user with pretrained weights can `load_state_dict` them).

    The module tree is the reference's - a ModuleDict of nn.Sequential prefixes sharing one set of
    stock Conv2d / ReLU / MaxPool2d modules - so `state_dict()` has its keys and a reference
    checkpoint loads; the modules are never called.  The trunk runs ONCE over the stacked
    [output; target] batch on the fused pipeline's fp32 convolution kernels (Winograd where they
    tile) with taps, in chunks of at most `chunk` images; the trunk is frozen, so the only gradient
    is d/d output, formed inside the forward call and scaled by autograd's upstream in backward.
    `target_layout` as `MSELoss`.  `last_layer_mse` keeps the per-layer MSEs (fp64 [L], on the
    device, in the order of `features`) of the last call."""

    def __init__(self, layers=None, target_layout="nchw", chunk=8, precision="fp32"):
        super().__init__()
        if ops._prec(precision) != 0:
            raise NotImplementedError("the perceptual trunk runs on fp32 layer tensors only "
                                      "(no bf16 / bf16x3 form)")
        if target_layout not in ("nchw", "nhwc_u8"):
            raise ValueError("target_layout must be 'nchw' or 'nhwc_u8'")
        if int(chunk) < 1:
            raise ValueError("chunk must be >= 1")
        if layers is None:
            layers = ["relu1_2", "relu2_2", "relu3_3", "relu4_3"]
        names = [n for n in layers if n in _VGG16_LAYER_MAP]      # unknown names are skipped
        if not names:
            raise ValueError("no valid VGG16 layer name among " + repr(list(layers)))
        self.target_layout = target_layout
        self.chunk = int(chunk)
        depth = max(_VGG16_LAYER_MAP[n] for n in names) + 1
        mods = _vgg16_features(depth)
        self.features = nn.ModuleDict()
        for n in names:
            self.features[n] = nn.Sequential(*mods[:_VGG16_LAYER_MAP[n] + 1])
        for param in self.parameters():
            param.requires_grad = False
        self.eval()
        self.register_buffer("mean", torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1))
        self.register_buffer("std", torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1))
        # the trunk as the kernels walk it: one record per convolution up to the deepest tap
        row = {_VGG16_LAYER_MAP[n]: i for i, n in enumerate(self.features)}   # relu index -> row
        self._trunk = []    # (conv module, row of the tap or None, pooled before this conv)
        pooled = False
        for idx, m in enumerate(mods[:depth]):
            if isinstance(m, nn.MaxPool2d):
                pooled = True
            elif isinstance(m, nn.Conv2d):
                self._trunk.append((m, row.get(idx + 1), pooled))
                pooled = False
        self._pools = sum(1 for _, _, p in self._trunk if p)
        self._packed = None
        self._norm = None
        self._ones = {}
        self.last_layer_mse = None

    # ---- packed weights: once per device placement / load_state_dict (the trunk is frozen) ----
    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._packed = None
        self._ones = {}
        return out

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self._packed = None
        return out

    def _pack(self):
        if self._packed is None:
            packed = []
            for i, (m, _, _) in enumerate(self._trunk):
                w = m.weight.detach().contiguous()
                cout, cin = w.shape[:2]
                wf, wd = ops.pack_conv3x3_weights(w, want_wd=i > 0)
                uf = ud = None
                # the Winograd forms where the channel counts admit them (the stem has none);
                # whether a launch takes them is a question of its shape, asked per call
                want_f, want_d = i > 0 and cout % 64 == 0, i > 0 and cin % 64 == 0
                if want_f or want_d:
                    uf, ud = ops.pack_wino_weights(w, want_f=want_f, want_d=want_d)
                packed.append((w, m.bias.detach().contiguous(), wf, wd, uf, ud))
            self._packed = packed
            self._norm = (tuple(self.mean.flatten().tolist()), tuple(self.std.flatten().tolist()))
        return self._packed

    def _relu_coeffs(self, n, c, like):
        key = (n, c)
        if key not in self._ones:
            self._ones[key] = (torch.ones((n, c), dtype=torch.float32, device=like.device),
                               torch.zeros((n, c), dtype=torch.float32, device=like.device))
        return self._ones[key]

    def _raw(self, y):
        """The raw convolution output y as an operand activated on load: relu(y * 1 + 0)."""
        return ops.Act(y, *self._relu_coeffs(y.shape[0], y.shape[3], y))

    def _run(self, output, target, target_u8, want_grad):
        N, _, H, W = output.shape
        packed = self._pack()
        mean, std = self._norm
        L = len(self.features)
        last = len(self._trunk) - 1
        sums = torch.empty((L, N), dtype=torch.float64, device=output.device)
        dout = torch.empty_like(output) if want_grad else None
        for c0 in range(0, N, self.chunk):
            n = min(self.chunk, N - c0)
            src = ops.Act(ops.perceptual_prep(output[c0:c0 + n], target[c0:c0 + n], target_u8,
                                              mean, std))
            ys = []
            for i, (_, tap, pooled) in enumerate(self._trunk):
                _, bias, wf, _, uf, _ = packed[i]
                if pooled:
                    src = ops.Act(ops.relu_maxpool2x2_fwd(src.x))
                elif i > 0:
                    src = self._raw(src.x)
                M, h, w, cin = src.shape
                wino = uf is not None and ops.conv_wino_supported(M, h, w, cin, 0, wf.shape[1])
                if wino and src.alpha is None:   # the Winograd loader activates: relu(p) == p
                    src = self._raw(src.x)
                y = ops.conv_fwd_raw(src, 0.0, wf, bias, wu=uf if wino else None)
                if tap is not None:
                    ops.feature_mse_fwd(y, sums[tap, c0:c0 + n])
                ys.append(y if want_grad else None)
                src = ops.Act(y)
            if not want_grad:
                continue
            g = gp = None       # dL/d relu(y_i): at y_i's resolution, or behind the pool after it
            for i in range(last, -1, -1):
                _, tap, pooled = self._trunk[i]
                w, _, _, wd, _, ud = packed[i]
                y = ys[i]
                ys[i] = None
                _, h, w_px, c = y.shape
                coef = 2.0 / (float(L) * N * c * h * w_px) if tap is not None else 0.0
                dz = ops.perceptual_relu_bwd(y[:n], y[n:] if tap is not None else None, coef,
                                             g=g, gp=gp)
                del y
                if i == 0:
                    ops.perceptual_stem_bwd_data(dz, w, std, out=dout[c0:c0 + n])
                    break
                # the data gradient of conv i on the n output images: dL/d(its source), which is
                # relu(y_{i-1}) or - `pooled` - the pool's output in front of it
                cin = w.shape[1]
                wino = ud is not None and ops.conv_wino_supported(n, h, w_px, c, 0, cin)
                gin = ops.conv3x3_bwd_data(dz, wd, 0, cin, h, w_px, 1, ud=ud if wino else None)
                g, gp = (None, gin) if pooled else (gin, None)
        # loss = (1/L) sum_l [sum_n sums[l][n]] / (N C_l H_l W_l): images, then layers, in index
        # order (a handful of tiny launches on [L] doubles; no host value is read)
        acc = sums[:, 0]
        for k in range(1, N):
            acc = acc + sums[:, k]
        counts = [0.0] * L
        h, w = H, W
        for m, tap, pooled in self._trunk:
            if pooled:
                h, w = h // 2, w // 2
            if tap is not None:
                counts[tap] = float(N) * m.out_channels * h * w
        mses = [acc[l] / counts[l] for l in range(L)]
        total = mses[0]
        for l in range(1, L):
            total = total + mses[l]
        self.last_layer_mse = torch.stack(mses)
        return (total / L).float(), dout

    def forward(self, output, target):
        if output.dim() != 4 or output.shape[1] != 3:
            raise ValueError("expected an NCHW RGB output")
        if min(output.shape[2:]) < (1 << self._pools):
            raise ValueError(f"a {output.shape[2]}x{output.shape[3]} image does not survive the "
                             f"{self._pools} poolings in front of the deepest requested layer")
        output = _check_input("PerceptualLoss", output, self.target_layout)
        u8 = self.target_layout == "nhwc_u8"
        if not u8 and target.dtype != torch.float32:
            target = target.float()
        want_grad = torch.is_grad_enabled() and output.requires_grad
        return _PerceptualFunction.apply(output, target.contiguous(), self, u8, want_grad)


class ReconstructionLoss(nn.Module):
    """`ReconstructionLoss` (AE_pretrained/reconstruction/models/losses.py:12-79) on the HIP path:
    mse_weight * MSE + ssim_weight * (1 - SSIM), a 0-dim fp32 tensor.  With ssim_weight > 0 the
    loss is one fused forward (two launches) and one gradient launch; with ssim_weight == 0 it runs
    exactly `MSELoss`'s launches (the same bits).  `target_layout` as `MSELoss`; `last_per_image`
    keeps the per-image sums of squared differences (fp64, on the device) of the last call.

    The perceptual term (perceptual_weight > 0) takes its network from the caller:
    `perceptual=PerceptualLoss(...)`.  The reference builds `models.vgg16(weights=None)` inside the
    loss - a randomly initialised, frozen VGG16, a fixed random feature extractor silently drawn
    from the global generator; here the caller owns that draw (and may `load_state_dict` other
    weights), so a positive weight without a module raises NotImplementedError.  The MSE(+SSIM)
    part keeps its launches and bits; the perceptual gradient is added into dL/doutput by
    autograd's accumulation."""

    def __init__(self, mse_weight=1.0, perceptual_weight=0.0, ssim_weight=0.0,
                 perceptual_layers=None, target_layout="nchw", perceptual=None):
        super().__init__()
        if perceptual_weight > 0:
            if perceptual is None:
                raise NotImplementedError(
                    "the perceptual term needs its feature network from the caller: pass "
                    "perceptual=ua.PerceptualLoss(...) (the reference silently draws a random "
                    "VGG16 inside the loss; here the caller owns that draw)")
            if not isinstance(perceptual, PerceptualLoss):
                raise TypeError("perceptual must be a PerceptualLoss")
            if perceptual.target_layout != target_layout:
                raise ValueError("perceptual.target_layout differs from target_layout")
        self.mse_weight = mse_weight
        self.perceptual_weight = perceptual_weight
        self.ssim_weight = ssim_weight
        self.target_layout = target_layout
        self.mse_loss = MSELoss(target_layout=target_layout)
        self.perceptual_loss = perceptual if perceptual_weight > 0 else None
        self.ssim_loss = SSIMLoss(target_layout=target_layout) if ssim_weight > 0 else None
        self.last_per_image = None

    def forward(self, output, target):
        if self.perceptual_loss is not None:
            base = self._base(output, target)
            return base + self.perceptual_weight * self.perceptual_loss(output, target)
        return self._base(output, target)

    def _base(self, output, target):
        if self.ssim_loss is None:
            mse = self.mse_loss(output, target)
            self.last_per_image = self.mse_loss.last_per_image
            return mse if self.mse_weight == 1.0 else self.mse_weight * mse
        output = _check_input("ReconstructionLoss", output, self.target_layout)
        u8 = self.target_layout == "nhwc_u8"
        if not u8 and target.dtype != torch.float32:
            target = target.float()
        loss = _SSIMFunction.apply(output, target.contiguous(), self.ssim_loss, u8,
                                   float(self.ssim_weight), float(self.mse_weight), False)
        self.last_per_image = self.ssim_loss.last_per_image
        return loss
