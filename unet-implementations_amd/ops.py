"""Thin torch-tensor wrappers over the C ABI: one Python function per operation.

Tensors are plumbing only: device memory, the current HIP stream and nothing
else.  Activations are NHWC (`[N, H, W, C]` contiguous), fp32 or - on the
mixed-precision pipeline - bf16; statistics, weights and gradients of weights are
fp32.  Every function launches asynchronously on torch's current stream.

An operation whose C entry point comes in several forms (storage type of the
tensors, matrix-core operand mode, Winograd form, with or without the
InstanceNorm-backward epilogue) has a `_sel_<operation>` function that names the
entry point (resolved once per combination), says which optional arguments it
takes and gives the KernelTimer tag; the wrapper then allocates, calls and
brackets once.  The accounting rules of the timer records live in `_end_conv`
(Winograd 16/36), `_end_lowres` (1/4) and `_sel_conv3x3_bwd_data` (stride-2
launches).
"""
import ctypes
import functools
import threading

import torch

from ._lib import ActSrc, BwdStats, PackEntry, WinoPackEntry, check, lib


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """hipStream_t of torch's current stream on the current device.  Every entry-point call needs
    it (~330 per train step): the raw accessors cost ~0.3 us, `torch.cuda.current_stream()`
    builds a Stream object for ~10 us (3 ms of host time per step)."""
    if _raw_stream is not None and _raw_device is not None:
        return _raw_stream(_raw_device())
    return torch.cuda.current_stream().cuda_stream


class KernelTimer:
    """HIP-event timing of kernel launches, recorded on the stream the kernels are launched on
    (torch's current stream).  bench.py installs one over its timed region to report
    `roofline.achieved` = algorithmic FLOPs / measured kernel time, the MFMA FLOPs actually
    issued (`executed`: lower where a gradient is reassociated onto the low-resolution grid) and
    the HBM rates of the streaming kernels (`nbytes` = algorithmic bytes)."""

    def __init__(self, only=None):
        # only: set of call-site classes ("conv" = 3x3 forward / data gradient, "wgrad") to
        # bracket; None = every entry point.  An event pair costs ~2.5 us of stream time (the
        # marker packets serialise the command processor), 0.8 ms per step over all ~330
        # calls - so bench.py brackets only the roofline group inside its timed region.
        self.only = only
        self.records = []  # (tag, flops, launches, start_event, end_event, executed, nbytes)

    def begin(self, kind=None):
        if self.only is not None and kind not in self.only:
            return None
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev

    def end(self, tag, flops, launches, start, executed=None, nbytes=0.0):
        if start is None:
            return
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        self.records.append((tag, flops, launches, start, ev,
                             flops if executed is None else executed, nbytes))

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for tag, flops, launches, e0, e1, executed, nbytes in self.records:
            d = out.setdefault(tag, dict(flops=0.0, executed=0.0, bytes=0.0, ms=0.0, launches=0,
                                         calls=0))
            d["flops"] += flops
            d["executed"] += executed
            d["bytes"] += nbytes
            d["ms"] += e0.elapsed_time(e1)
            d["launches"] += launches
            d["calls"] += 1
        return out


_timer = None
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def set_timer(timer):
    global _timer
    _timer = timer


def _begin(kind=None):
    """Opening half of the timer bracket: the start event, or None when no timer is installed or
    it does not take call sites of `kind`.  The closing half stays at the call site as
    `if t0 is not None: _timer.end(...)`, so that the FLOP and byte arithmetic of a record runs
    only when the record is kept."""
    return _timer.begin(kind) if _timer is not None else None


def _end_conv(t0, tag, alg, launches, wino):
    """Record of a 3x3 matrix-core launch: a Winograd form F(2x2, 3x3) issues 16/36 of the
    algorithmic MFMA FLOPs."""
    _timer.end(tag, alg, launches, t0, executed=alg * 16.0 / 36.0 if wino else None)


def _end_lowres(t0, tag, N, h, w, Cin, Cout, launches):
    """Record of a gradient of conv3x3(upsample2x(.)) reassociated onto the low-resolution grid
    (from the taps D): algorithmic FLOPs are those on the up-sampled grid, 1/4 of them execute."""
    alg = 2.0 * N * 4 * h * w * 9 * Cin * Cout
    _timer.end(tag, alg, launches, t0, executed=alg / 4)


def _ptr(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("unet-implementations_amd: the HIP path needs CUDA/ROCm tensors "
                           "(no CPU fallback exists)")
    if t.dtype not in (torch.float32, torch.int64, torch.uint8, torch.bfloat16):
        raise TypeError(f"unsupported dtype {t.dtype}")
    if not t.is_contiguous():
        raise ValueError("tensor must be contiguous")
    return t.data_ptr()


def _f32(shape, like):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


def _b16(shape, like):
    return torch.empty(shape, dtype=torch.bfloat16, device=like.device)


def _is_b16(t):
    return t is not None and t.dtype == torch.bfloat16


def _ws(nbytes, like):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=like.device)


@functools.lru_cache(maxsize=None)
def _export(name):
    """The entry point `name`, resolved once (the selectors below build names from parts)."""
    return getattr(lib(), name)


@functools.lru_cache(maxsize=None)
def _twin(name, b16):
    """The export `name`, or its twin for bf16 tensors (`name_b16`)."""
    return getattr(lib(), name + "_b16" if b16 else name)


def _call_nxt(fn, args, nxt):
    """fn(*args, unet_bwd_stats* of the NextNorm `nxt` or NULL, stream); afterwards `nxt.tiles`
    says whether the launch left that layer's InstanceNorm-backward reductions."""
    if nxt is None:
        check(fn(*args, None, _stream()))
        return
    bs = nxt.c_struct()
    check(fn(*args, ctypes.byref(bs), _stream()))
    nxt.tiles = bs.tiles_out


# ---- deferred weight-gradient reductions (unet_wgrad_defer_*) -----------------------------------
_defer = threading.local()


def _wgrad_ws(nbytes, like):
    """Workspace of a weight-gradient call: while its reduction is only queued (wgrad_deferral)
    it must outlive the flush."""
    ws = _ws(nbytes, like)
    held = getattr(_defer, "held", None)
    if held is not None:
        held.append(ws)
    return ws


class wgrad_deferral:
    """`with wgrad_deferral() as d:` - the weight-gradient entry points called inside only queue
    the reductions of their slabs; `d.flush()` (and the end of the block) launches everything
    queued so far as 2-3 batched launches instead of 2-3 per layer.  A weight gradient is valid
    only after the flush that follows its call.  Per thread and nestable: an inner scope (a
    nested backward on the same thread) joins the outer one - its flush and its exit launch
    what is queued and leave the queue on; only the outermost exit turns deferral off."""

    def __enter__(self):
        depth = getattr(_defer, "depth", 0)
        if depth == 0:
            check(lib().unet_wgrad_defer_begin())
            _defer.held = []
        _defer.depth = depth + 1
        return self

    def flush(self):
        n = lib().unet_wgrad_defer_pending()
        if n:
            t0 = _begin("wgrad")
            check(lib().unet_wgrad_defer_flush(_stream()))
            if t0 is not None:
                _timer.end("conv_wgrad_reduce", 0.0, 2, t0)
        # (stream order: the allocator hands the blocks out again only behind the flush)
        _defer.held.clear()
        return n

    def __exit__(self, *exc):
        _defer.depth -= 1
        if _defer.depth:
            self.flush()
            return False
        try:
            check(lib().unet_wgrad_defer_end(_stream()))
        finally:
            _defer.held = None
        return False


# ---- launch record (unet_debug_record_launches) ------------------------------------------------
class record_launches:
    """`with record_launches() as rec: ...` - afterwards `rec.names` lists the kernels the library
    launched inside the block (demangled names, launch order, launches from every thread).  A
    test hook: the record is process-wide, so two blocks must not overlap."""

    def __init__(self):
        self.names = None

    def __enter__(self):
        check(lib().unet_debug_record_launches(1))
        return self

    def __exit__(self, *exc):
        n = lib().unet_debug_recorded_launches(None, 0)
        buf = ctypes.create_string_buffer(n + 1)
        lib().unet_debug_recorded_launches(buf, n + 1)
        check(lib().unet_debug_record_launches(0))
        self.names = buf.value.decode().splitlines()
        return False


# ---- layout -------------------------------------------------------------------
def nchw_to_nhwc(x):
    N, C, H, W = x.shape
    y = _f32((N, H, W, C), x)
    check(lib().unet_nchw_to_nhwc(_ptr(x), _ptr(y), N, C, H, W, _stream()))
    return y


def nhwc_to_nchw(x):
    N, H, W, C = x.shape
    y = _f32((N, C, H, W), x)
    check(lib().unet_nhwc_to_nchw(_ptr(x), _ptr(y), N, C, H, W, _stream()))
    return y


def pack_conv3x3_weights(w_oihw, wf=None, wd=None, want_wd=True):
    Cout, Cin, kh, kw = w_oihw.shape
    assert kh == 3 and kw == 3
    if wf is None:
        wf = _f32((9, Cout, Cin), w_oihw)   # forward: reduction axis (ci) contiguous
    if wd is None and want_wd:
        wd = _f32((9, Cin, Cout), w_oihw)   # data gradient: reduction axis (co) contiguous
    check(lib().unet_pack_conv3x3_weights(_ptr(w_oihw), _ptr(wf), _ptr(wd), Cout, Cin, _stream()))
    return wf, wd


def pack_conv3x3_weights_bf16x3(w_oihw, want_wd=True, want_wf=True):
    """The two packed layouts as three bf16 planes each (the split-bf16 operand mode):
    wf3 [3, 9, Cout, Cin], wd3 [3, 9, Cin, Cout]."""
    Cout, Cin, kh, kw = w_oihw.shape
    assert kh == 3 and kw == 3
    wf3 = torch.empty((3, 9, Cout, Cin), dtype=torch.bfloat16, device=w_oihw.device) \
        if want_wf else None
    wd3 = torch.empty((3, 9, Cin, Cout), dtype=torch.bfloat16, device=w_oihw.device) \
        if want_wd else None
    check(lib().unet_pack_conv3x3_weights_bf16x3(_ptr(w_oihw), _ptr(wf3), _ptr(wd3), Cout, Cin,
                                                 _stream()))
    return wf3, wd3


class PackTable:
    """Device table for `unet_pack_conv3x3_weights_batched`: one entry per 3x3 layer with
    persistent destination buffers (fp32 layouts always, bf16x3 planes on request)."""

    def __init__(self, weights, planes, wino=None):
        """wino: per weight a pair (forward, data gradient) of flags - also keep the Winograd
        forms U = G g G^T of that layer (csrc/conv_wino.hip), refreshed by run()."""
        self.wf, self.wd, self.wf3, self.wd3 = [], [], [], []
        self.src_ptrs = [w.data_ptr() for w in weights]
        self.planes = planes
        self.wino = tuple(wino) if wino is not None else tuple((False, False) for _ in weights)
        self.uf, self.ud, self._wino_jobs = [], [], []
        for w, (ff, fd) in zip(weights, self.wino):
            cout, cin = w.shape[0], w.shape[1]
            uf = _f32((16 * cout * cin,), w) if ff else None
            ud = _f32((16 * cout * cin,), w) if fd else None
            self.uf.append(uf)
            self.ud.append(ud)
            if uf is not None or ud is not None:
                self._wino_jobs.append((w, uf, ud, cout, cin))
        # device table of unet_pack_wino_weights_batched: one launch for every Winograd form
        self._wino_table, self._wino_blocks = None, 0
        if self._wino_jobs:
            rawu = b""
            for w, uf, ud, cout, cin in self._wino_jobs:
                rawu += bytes(WinoPackEntry(w.data_ptr(), 0 if uf is None else uf.data_ptr(),
                                            0 if ud is None else ud.data_ptr(), cout, cin,
                                            self._wino_blocks, 0))
                self._wino_blocks += (cout * cin // 8 + 255) // 256
            self._wino_table = torch.frombuffer(bytearray(rawu), dtype=torch.uint8).to(
                weights[0].device)
        raw = b""
        tiles = 0
        for w in weights:
            cout, cin = w.shape[0], w.shape[1]
            if cout % 32:
                raise ValueError("batched packing needs Cout to be a multiple of 32")
            wf = _f32((9, cout, cin), w)
            wd = _f32((9, cin, cout), w)
            wf3 = wd3 = None
            if planes and cin != 3:
                # planes: True / 3 = the three split planes, 1 = the bf16-rounded weight alone
                npl = 1 if planes == 1 and planes is not True else 3
                wf3 = torch.empty((npl, 9, cout, cin), dtype=torch.bfloat16, device=w.device)
                wd3 = torch.empty((npl, 9, cin, cout), dtype=torch.bfloat16, device=w.device)
            self.wf.append(wf); self.wd.append(wd); self.wf3.append(wf3); self.wd3.append(wd3)
            # the last member, `reserved`, carries the planes flag
            raw += bytes(PackEntry(w.data_ptr(), wf.data_ptr(), wd.data_ptr(),
                                   0 if wf3 is None else wf3.data_ptr(),
                                   0 if wd3 is None else wd3.data_ptr(), cout, cin, tiles,
                                   1 if (wf3 is not None and wf3.shape[0] == 1) else 0))
            tiles += (cout // 32) * ((cin + 31) // 32)
        self.n, self.tiles = len(weights), tiles
        self.table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(weights[0].device)

    def matches(self, weights, planes, wino=None):
        wino = tuple(wino) if wino is not None else tuple((False, False) for _ in weights)
        return planes == self.planes and len(weights) == self.n and wino == self.wino and \
            all(w.data_ptr() == p for w, p in zip(weights, self.src_ptrs))

    def run(self):
        check(lib().unet_pack_conv3x3_weights_batched(self.table.data_ptr(), self.n, self.tiles,
                                                      _stream()))
        if self._wino_table is not None:
            check(lib().unet_pack_wino_weights_batched(self._wino_table.data_ptr(),
                                                       len(self._wino_jobs), self._wino_blocks,
                                                       _stream()))


# ---- convolution ---------------------------------------------------------------
_PREC = {False: 0, True: 1, 0: 0, 1: 1, 3: 3, "fp32": 0, "bf16": 1, "bf16x3": 3}
_SUFFIX = {0: "", 1: "_bf16", 3: "_bf16x3"}   # of an operand mode: in export names and timer tags


def _prec(bf16):
    """Matrix-core operand mode of a conv call: fp32 MFMA (default), bf16 operands, or the
    split-bf16 emulation of fp32 ("bf16x3": 3 bf16 terms per operand, 6 products)."""
    try:
        return _PREC[bf16]
    except (KeyError, TypeError):
        raise ValueError("precision must be 'fp32', 'bf16' or 'bf16x3'") from None


@functools.lru_cache(maxsize=None)
def _sel_conv3x3_fwd(pr, C0):
    """-> (entry point, takes the weight planes wf3, timer tag)"""
    if pr == 3 and C0 == 3:
        pr = 0                      # the RGB stem has no split form (K = 27, HBM-bound)
    return (_export("unet_conv3x3_fwd" + _SUFFIX[pr]), pr == 3,
            "conv_stem_fwd" if C0 == 3 else "conv_igemm" + _SUFFIX[pr])


def conv3x3_fwd(x0, x1, wf, bias, stride, out=None, bf16=False, wf3=None):
    N, H, W, C0 = x0.shape
    C1 = 0 if x1 is None else x1.shape[3]
    if x1 is not None:
        assert x1.shape[:3] == x0.shape[:3]
    Cout = wf.shape[1]
    assert wf.shape[0] == 9 and wf.shape[2] == C0 + C1
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    y = out if out is not None else _f32((N, Ho, Wo, Cout), x0)
    fn, planes, tag = _sel_conv3x3_fwd(_prec(bf16), C0)
    if planes and wf3 is None:
        raise ValueError("bf16x3 needs wf3 from pack_conv3x3_weights_bf16x3")
    w3 = (_ptr(wf3),) if planes else ()
    t0 = _begin("conv")
    check(fn(_ptr(x0), C0, _ptr(x1), C1, _ptr(wf), *w3, _ptr(bias), _ptr(y), N, H, W, Cout, stride,
             _stream()))
    if t0 is not None:
        _timer.end(tag, 2.0 * N * Ho * Wo * 9 * (C0 + C1) * Cout, 1, t0)
    return y


class NextNorm:
    """Layer l as seen by the producer of g = dL/da_l: raw output y, statistics, affine
    parameters, dropout mask.  A data gradient whose output is FINAL for layer l takes one and
    leaves the per-tile reductions of l's InstanceNorm backward in `.partial` / `.tiles`
    (tiles == 0: that launch had no such epilogue)."""

    __slots__ = ("y", "st", "gamma", "beta", "mask", "slope", "partial", "tiles", "applied")

    def __init__(self, y, st, gamma, beta, mask, slope):
        self.y, self.st, self.gamma, self.beta, self.mask, self.slope = y, st, gamma, beta, mask, slope
        self.partial, self.tiles = None, 0
        # the producer went on to l's whole InstanceNorm backward (head1x1_in_bwd_fold): what it
        # returned is dL/dz and l's parameter gradients are written
        self.applied = False

    def c_struct(self):
        N, H, W, C = self.y.shape
        nbytes = N * ((H * W + 63) // 64) * C * 8
        self.partial = torch.empty(nbytes, dtype=torch.uint8, device=self.y.device)
        return BwdStats(_ptr(self.y), _ptr(self.st[0]), _ptr(self.st[1]), _ptr(self.gamma),
                        _ptr(self.beta), _ptr(self.mask), self.slope, _ptr(self.partial), nbytes, 0)


def _c32_winograd(N, H, W, Cin, Cout, stride):
    """True when the fp32 32 -> 32 channel kernel of this shape runs in its Winograd form
    (csrc/conv_c32.hip; `set_c32_winograd`): 16/36 of the direct kernel's MFMA FLOPs."""
    return bool(lib().unet_conv_c32_is_winograd(N, H, W, Cin, Cout, stride))


_c32_override = None


def c32_winograd_override():
    """The setting a direct `set_c32_winograd(...)` call left behind (tests, benchmarks), or None."""
    return _c32_override


class c32_winograd_scope:
    """`with c32_winograd_scope(mode):` - the calling thread's switch set to `mode` (True /
    False / "always") for the block and put back afterwards: how UNet.forward / backward pass
    their model's choice to the entry points they call without leaving it behind."""

    def __init__(self, mode):
        self.code = 2 if mode == "always" else (1 if mode else 0)

    def __enter__(self):
        self.prev = lib().unet_set_c32_winograd(self.code)
        return self

    def __exit__(self, *exc):
        lib().unet_set_c32_winograd(self.prev)
        return False


def set_c32_winograd(on, override=True):
    """Choice for the 32 -> 32 channel stride-1 layers on the fused fp32 pipeline: True (default)
    = the Winograd kernel for launches that fill the chip (>= 512 tiles of 8 x 32 pixels),
    "always" = for every shape it tiles, False = the direct kernel.  Returns the previous setting
    of the calling thread in the same terms.  The library keeps the switch PER THREAD;
    `UNet.forward` applies `model.winograd` to its own calls only (`c32_winograd_scope`) and
    hands the decision to its backward.  A direct call (override=True) is a test / benchmark
    override for kernel-level calls: "always" then also wins over `model.winograd`."""
    global _c32_override
    code = 2 if on == "always" else (1 if on else 0)
    prev = lib().unet_set_c32_winograd(code)
    if override:
        _c32_override = on if on == "always" else None
    return "always" if prev == 2 else bool(prev)


@functools.lru_cache(maxsize=None)
def _sel_conv3x3_bwd_data(b16, pr, has_wd3, has_nxt, wino):
    """-> (entry point, takes the weight planes wd3, takes unet_bwd_stats, timer tag, launches at
    stride 2: 4 = one per output parity class, 1 = one kernel covers them, 0 = the plain fp32
    kernel: 1 when it has >= 512 tiles, else 4)"""
    if wino:
        return _export("unet_conv3x3_bwd_data_bs_wino"), False, True, "conv_igemm", 1
    if b16:     # mixed-precision pipeline: bf16 tensors, bf16 matrix cores
        if has_nxt or has_wd3:
            # (wd3: the weights also pre-rounded to bf16 - plane 0 of the pack's planes)
            return _export("unet_conv3x3_bwd_data_bs_b16_wb"), True, True, "conv_igemm_bf16", 4
        return _export("unet_conv3x3_bwd_data_b16"), False, False, "conv_igemm_bf16", 4
    bs = has_nxt and pr != 1
    return (_export("unet_conv3x3_bwd_data" + ("_bs" if bs else "") + _SUFFIX[pr]), pr == 3, bs,
            "conv_igemm" + _SUFFIX[pr], 1 if bs else (0 if pr == 0 else 4))


def conv3x3_bwd_data(dy, wd, ci_offset, ccols, H, W, stride, out=None, accumulate=False,
                     bf16=False, wd3=None, nxt=None, ud=None):
    """dx[N,H,W,ccols] (+)= transpose-conv of dy for input channels [ci_offset, ci_offset+ccols).
    nxt (NextNorm): dx is final for that layer - also emit its backward reductions.
    ud: the Winograd data-gradient form of the weight (fp32 tensors, stride 1, no accumulate,
    shape checked by the caller with conv_wino_supported)."""
    N, Ho, Wo, Cout = dy.shape
    cin_total = wd.shape[1]
    assert wd.shape[0] == 9 and wd.shape[2] == Cout
    b16 = _is_b16(dy)
    pr = 1 if b16 else _prec(bf16)
    wino = ud is not None and not b16 and stride == 1 and not accumulate and pr == 0
    fn, planes, takes_bs, tag, stride2 = _sel_conv3x3_bwd_data(b16, pr, wd3 is not None,
                                                               nxt is not None, wino)
    dx = out if out is not None else (_b16 if b16 else _f32)((N, H, W, ccols), dy)
    assert dx.shape == (N, H, W, ccols) and (not b16 or _is_b16(dx))
    if planes and wd3 is None and not takes_bs:
        raise ValueError("bf16x3 needs wd3 from pack_conv3x3_weights_bf16x3")
    w3 = (_ptr(wd3),) if planes else ()
    form = () if wino else (stride, 1 if accumulate else 0)
    args = (_ptr(dy), _ptr(ud if wino else wd), *w3, cin_total, ci_offset, _ptr(dx), N, H, W, Cout,
            ccols, *form)
    t0 = _begin("conv")
    if takes_bs:
        _call_nxt(fn, args, nxt)
    else:
        check(fn(*args, _stream()))
    if t0 is not None:
        launches = 1 if stride == 1 else stride2 or \
            (1 if -(-(N * Ho * Wo) // 128) * (ccols // 32) >= 512 else 4)
        _end_conv(t0, tag, 2.0 * N * Ho * Wo * 9 * ccols * Cout, launches,
                  wino or (not b16 and pr == 0 and _c32_winograd(N, H, W, ccols, Cout, stride)))
    return dx


def conv3x3_bwd_weight(x, dy, dw_oihw, ci_offset, stride, db=None, bf16=False):
    N, H, W, Cx = x.shape
    Cout = dy.shape[3]
    cin_total = dw_oihw.shape[1]
    assert dw_oihw.shape[0] == Cout and dw_oihw.is_contiguous()
    nbytes = lib().unet_conv3x3_bwd_weight_workspace_bytes(N, H, W, Cx, Cout, stride)
    ws = _wgrad_ws(nbytes, x)
    sfx = _SUFFIX[_prec(bf16)]
    t0 = _begin("wgrad")
    check(_export("unet_conv3x3_bwd_weight" + sfx)(
        _ptr(x), Cx, _ptr(dy), _ptr(dw_oihw), ci_offset, cin_total, _ptr(db), _ptr(ws), ws.numel(),
        N, H, W, Cout, stride, _stream()))
    if t0 is not None:  # wgrad kernel + slab reduce
        _timer.end("conv_stem_wgrad" if Cx == 3 else "conv_wgrad" + sfx,
                   2.0 * N * dy.shape[1] * dy.shape[2] * 9 * Cx * Cout, 2, t0)
    return dw_oihw


# ---- 1x1 convolution (CLIP fusion layer) ------------------------------------------------
def conv1x1_fwd(x0, x1, w2d, bias):
    """y = conv1x1(cat(x0, x1)) + bias; w2d is [Cout, C0+C1]."""
    N, H, W, C0 = x0.shape
    C1 = 0 if x1 is None else x1.shape[3]
    Cout = w2d.shape[0]
    assert w2d.shape[1] == C0 + C1 and w2d.is_contiguous()
    y = _f32((N, H, W, Cout), x0)
    check(lib().unet_conv1x1_fwd(_ptr(x0), C0, _ptr(x1), C1, _ptr(w2d), _ptr(bias), _ptr(y), N, H,
                                 W, Cout, _stream()))
    return y


def transpose2d(w2d):
    R, C = w2d.shape
    out = _f32((C, R), w2d)
    check(lib().unet_transpose2d(_ptr(w2d), _ptr(out), R, C, _stream()))
    return out


def conv1x1_bwd_data(dy, wT, ci_offset, ccols, accumulate=False, out=None):
    N, H, W, Cout = dy.shape
    cin_total = wT.shape[0]
    assert wT.shape[1] == Cout
    dx = out if out is not None else _f32((N, H, W, ccols), dy)
    check(lib().unet_conv1x1_bwd_data(_ptr(dy), _ptr(wT), cin_total, ci_offset, _ptr(dx), N, H, W,
                                      Cout, ccols, 1 if accumulate else 0, _stream()))
    return dx


def conv1x1_bwd_weight(x, dy, dw2d, ci_offset):
    N, H, W, Cx = x.shape
    Cout = dy.shape[3]
    assert dw2d.shape[0] == Cout and dw2d.is_contiguous()
    ws = _wgrad_ws(lib().unet_conv3x3_bwd_weight_workspace_bytes(N, H, W, Cx, Cout, 1), x)
    check(lib().unet_conv1x1_bwd_weight(_ptr(x), Cx, _ptr(dy), _ptr(dw2d), ci_offset,
                                        dw2d.shape[1], _ptr(ws), ws.numel(), N, H, W, Cout,
                                        _stream()))
    return dw2d


# ---- InstanceNorm + LeakyReLU + channel dropout -----------------------------------
def instnorm_stats(y, gamma, beta, eps):
    N, H, W, C = y.shape
    st = _f32((4, N, C), y)  # mean, rstd, alpha, beta2
    ws = _ws(lib().unet_instnorm_workspace_bytes(N, H * W, C), y)
    check(lib().unet_instnorm_stats(_ptr(y), _ptr(gamma), _ptr(beta), eps, _ptr(st[0]),
                                    _ptr(st[1]), _ptr(st[2]), _ptr(st[3]), _ptr(ws), ws.numel(), N,
                                    H * W, C, _stream()))
    return st


def instnorm_lrelu_drop_fwd(y, alpha, beta2, mask, slope, out=None):
    N, H, W, C = y.shape
    a = out if out is not None else torch.empty_like(y)
    check(lib().unet_instnorm_lrelu_drop_fwd(_ptr(y), _ptr(alpha), _ptr(beta2), _ptr(mask), slope,
                                             _ptr(a), N, H * W, C, _stream()))
    return a


def instnorm_lrelu_drop_bwd(ga, y, mean, rstd, gamma, beta, mask, slope, dgamma, dbeta, dbias,
                            out=None, partials=None):
    """Returns dy (in place over `ga` unless `out` is given).  partials = (buffer, tiles): the
    reductions were already summarised per tile by the producer of ga (NextNorm)."""
    N, H, W, C = y.shape
    dy = ga if out is None else out
    ws = _ws(lib().unet_instnorm_workspace_bytes(N, H * W, C), y)
    if partials is not None:    # apply pass only: ga + y in, dy out
        name, part, launches, passes = "unet_instnorm_lrelu_drop_bwd_partials", \
            (_ptr(partials[0]), partials[1]), 2, 3.0
    else:       # reduce pass: ga + y; apply pass: ga + y in, dy out (+ tiny finalizers)
        name, part, launches, passes = "unet_instnorm_lrelu_drop_bwd", (), 5, 5
        if _is_b16(y) != _is_b16(ga):
            raise TypeError("ga and y must share their storage type")
    t0 = _begin()
    check(_twin(name, _is_b16(y))(
        _ptr(ga), _ptr(y), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), _ptr(mask), slope,
        _ptr(dy), _ptr(dgamma), _ptr(dbeta), _ptr(dbias), *part, _ptr(ws), ws.numel(), N, H * W, C,
        _stream()))
    if t0 is not None:
        _timer.end("instnorm_bwd", 0.0, launches, t0, nbytes=y.element_size() * passes * y.numel())
    return dy


def instnorm_bwd_merge_partials(partial, tiles, N, HW, C):
    """Per-tile reductions partial[N, tiles, C, 2] = (S1, S2) -> (coef, sums), [N, C, 2] each:
    sums = the tiles summed (in double, fixed order), coef = sums / HW."""
    coef, sums = _f32((N, C, 2), partial), _f32((N, C, 2), partial)
    check(lib().unet_instnorm_bwd_merge_partials(_ptr(partial), tiles, _ptr(coef), _ptr(sums), N,
                                                 HW, C, _stream()))
    return coef, sums


class _ResizeBilinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, H, W):
        n, c, h, w = x.shape
        x = x.contiguous().float()
        y = _f32((n, c, H, W), x)
        check(lib().unet_resize_bilinear_fwd(_ptr(x), _ptr(y), n * c, h, w, H, W, _stream()))
        ctx.hw = (h, w)
        return y

    @staticmethod
    def backward(ctx, gy):
        n, c, H, W = gy.shape
        h, w = ctx.hw
        gy = gy.contiguous().float()
        gx = _f32((n, c, h, w), gy)
        check(lib().unet_resize_bilinear_bwd(_ptr(gy), _ptr(gx), n * c, h, w, H, W, _stream()))
        return gx, None, None


def resize_bilinear(x, size):
    """F.interpolate(x, size=size, mode="bilinear", align_corners=False) of an NCHW fp32 tensor
    on the HIP kernels (differentiable; the backward is the deterministic gather-form adjoint)."""
    return _ResizeBilinear.apply(x, int(size[0]), int(size[1]))


# ---- fused layer pipeline (include/unet_hip.h) ---------------------------------------------
class Act:
    """An operand that is activated on load: `x` is the RAW output of a convolution (NHWC)
    and the consumer applies `lrelu(x * alpha[n, c] + beta[n, c])` while staging it, or a
    plain tensor (`alpha is None`).  alpha / beta are rows 2 and 3 of the statistics tensor
    `conv_in_fwd` returns (InstanceNorm scale / shift with the dropout mask folded in)."""

    __slots__ = ("x", "alpha", "beta")

    def __init__(self, x, alpha=None, beta=None):
        self.x, self.alpha, self.beta = x, alpha, beta

    @property
    def shape(self):
        return self.x.shape

    def c_struct(self):
        return ActSrc(_ptr(self.x), self.x.shape[3], _ptr(self.alpha), _ptr(self.beta))


class U8Image:
    """The dataset's uint8 HWC batch [N, H, W, 3] as the operand of the RGB stem: normalised
    ((v / 255) - mean) / std inside the loaders of the first convolution and of its weight
    gradient (unet_stem_u8_fwd / _bwd_weight and their `_b16` twins for bf16 layer tensors), never
    materialised as fp32."""

    __slots__ = ("x", "mean", "std")

    def __init__(self, x, mean=None, std=None):
        if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3 or not x.is_contiguous():
            raise TypeError("U8Image takes a contiguous uint8 [N,H,W,3] tensor")
        if x.shape[2] % 128:
            raise ValueError("the fused uint8 stem needs W % 128 == 0 (use preprocess_u8 otherwise)")
        self.x = x
        self.mean = tuple(IMAGENET_MEAN if mean is None else mean)
        self.std = tuple(IMAGENET_STD if std is None else std)

    @property
    def shape(self):
        return self.x.shape

    def c_mean_std(self):
        return (ctypes.c_float * 3)(*self.mean), (ctypes.c_float * 3)(*self.std)


def _act(a):
    if a is None:
        return None, None
    if not isinstance(a, Act):
        a = Act(a)
    st = a.c_struct()
    return a, ctypes.byref(st)


def conv_wino_supported(N, H, W, C0, C1, Cout):
    """Does the Winograd kernel tile conv3x3(stride 1) of [N,H,W,C0+C1] -> Cout (forward), or the
    data gradient with K = C0 reduction channels and Cout columns?"""
    return bool(lib().unet_conv_wino_supported(N, H, W, C0, C1, Cout))


def pack_wino_weights(w_oihw, want_f=True, want_d=True):
    """(uf, ud): the Winograd forms of a 3x3 weight (flat fp32 tensors of 16*Cout*Cin floats)."""
    cout, cin = w_oihw.shape[0], w_oihw.shape[1]
    uf = _f32((16 * cout * cin,), w_oihw) if want_f else None
    ud = _f32((16 * cout * cin,), w_oihw) if want_d else None
    check(lib().unet_pack_wino_weights(_ptr(w_oihw), _ptr(uf), _ptr(ud), cout, cin, _stream()))
    return uf, ud


def _conv_stats_launch(fn, head, b16, like, N, H, W, Cout, stride):
    """First half of the tail shared by the fused forwards "convolution + InstanceNorm statistics":
    allocates y, the statistics and the workspace and launches `fn(*head, y, workspace, &px, N, H,
    W, Cout, stream)` behind the opened timer bracket.  -> (y, st, ws, px, t0)"""
    y = (_b16 if b16 else _f32)((N, (H - 1) // stride + 1, (W - 1) // stride + 1, Cout), like)
    st = _f32((4, N, Cout), like)
    ws = _ws(lib().unet_conv_in_fwd_workspace_bytes(N, H, W, Cout, stride), like)
    px = ctypes.c_int(0)
    t0 = _begin("conv")
    check(fn(*head, _ptr(y), _ptr(ws), ws.numel(), ctypes.byref(px), N, H, W, Cout, _stream()))
    return y, st, ws, px, t0


def _conv_stats_finalize(b16, y, st, ws, px, gamma, beta, eps, mask):
    """Second half: the statistics of y from the partial sums the convolution left in ws."""
    N, Ho, Wo, Cout = y.shape
    check(_twin("unet_conv_in_stats_finalize", b16)(
        _ptr(y), _ptr(ws), ws.numel(), px.value, _ptr(gamma), _ptr(beta), eps, _ptr(mask),
        _ptr(st[0]), _ptr(st[1]), _ptr(st[2]), _ptr(st[3]), N, Ho * Wo, Cout, _stream()))
    return y, st


@functools.lru_cache(maxsize=None)
def _sel_conv_in_bwd_weight(u8, b16, x3):
    """-> entry point of a fused layer's weight gradient: the normalising RGB stem (U8Image) or a
    layer source, for fp32 / bf16 dy; x3: the split-bf16 operand mode (fp32 tensors)"""
    if u8:
        return _twin("unet_stem_u8_bwd_weight", b16)
    return _export("unet_conv_in_bwd_weight" + ("_b16" if b16 else ("_bf16x3" if x3 else "")))


@functools.lru_cache(maxsize=None)
def _sel_conv_in_fwd(b16, u8, wino, has_w3, ksize, C0):
    """-> (entry point, form: "u8" (normalising RGB stem) / "wino" (takes wu, no ksize / stride) /
    "planes" (takes w3) / "plain", timer tag)"""
    tag = "conv_stem_fwd" if C0 == 3 else \
        "conv_igemm" + _SUFFIX[1 if b16 else (3 if has_w3 else 0)]
    if u8:
        return _twin("unet_stem_u8_fwd", b16), "u8", tag
    if wino:    # Winograd F(2x2, 3x3) form (the caller checked conv_wino_supported)
        return _export("unet_conv_in_fwd_wino"), "wino", tag
    # planes on bf16 tensors: the weights also pre-rounded to bf16 (plane 0 of the planes)
    planes = has_w3 and C0 != 3 and (ksize == 3 or not b16)
    mark = ("_b16_wb" if b16 else "_bf16x3") if planes else ("_b16" if b16 else "")
    return _export("unet_conv_in_fwd" + mark), "planes" if planes else "plain", tag


def conv_in_fwd(s0, s1, slope, w, bias, ksize, stride, gamma, beta, eps, mask, b16=False,
                w3=None, wu=None):
    """Fused layer forward: y = conv(cat(act(s0), act(s1))) + bias and the InstanceNorm
    statistics of y.  Returns (y, st) with st = [mean, rstd, alpha, beta] as [4, N, Cout];
    alpha / beta carry the dropout `mask` [N, Cout] (or None) folded in.
    b16: the mixed-precision pipeline - y (and the sources other than the RGB image, fp32 or a
    U8Image) are bf16 tensors, bf16 matrix cores, fp32 statistics.
    w3 (pre-split weight planes): the split-bf16 operand mode on fp32 tensors."""
    u8 = s0 if isinstance(s0, U8Image) else None
    if u8 is None:
        s0, r0 = _act(s0)
    s1, r1 = _act(s1)
    N, H, W, C0 = s0.shape
    C1 = 0 if s1 is None else s1.shape[3]
    if s1 is not None:
        assert s1.shape[:3] == s0.shape[:3]
    Cout = w.shape[1] if ksize == 3 else w.shape[0]
    assert (w.shape[0] == 9 and w.shape[2] == C0 + C1) if ksize == 3 else w.shape[1] == C0 + C1
    if b16:
        for src in (s0, s1):
            if src is not None and src.shape[3] != 3 and not _is_b16(src.x):
                raise TypeError("the bf16 pipeline takes bf16 layer tensors")
    wino = wu is not None and not b16 and ksize == 3 and stride == 1
    fn, form, tag = _sel_conv_in_fwd(b16, u8 is not None, wino, w3 is not None, ksize, C0)
    if form == "u8":
        assert s1 is None and ksize == 3 and stride == 1
        head = (_ptr(u8.x), *u8.c_mean_std(), _ptr(w), _ptr(bias))
    elif form == "wino":
        head = (r0, r1, slope, _ptr(wu), _ptr(bias))
    elif form == "planes":
        head = (r0, r1, slope, _ptr(w), _ptr(w3), _ptr(bias), ksize, stride)
    else:
        head = (r0, r1, slope, _ptr(w), _ptr(bias), ksize, stride)
    y, st, ws, px, t0 = _conv_stats_launch(fn, head, b16, s0.x, N, H, W, Cout, stride)
    if t0 is not None:   # the convolution launch alone (its epilogue includes the statistics)
        # (a U8Image handed wu as well is recorded as a Winograd launch, which it is not: kept
        # as it always was, the network never makes that call)
        if form == "plain" and not b16 and w3 is None and ksize == 3 and s1 is None:
            wino = _c32_winograd(N, H, W, C0, Cout, stride)
        _end_conv(t0, tag, 2.0 * N * y.shape[1] * y.shape[2] * ksize * ksize * (C0 + C1) * Cout, 1,
                  wino)
    return _conv_stats_finalize(b16, y, st, ws, px, gamma, beta, eps, mask)


def conv_up_in_fwd_supported(low, skip, Cout):
    N, H, W, C1 = skip.shape
    if _is_b16(skip.x):     # mixed-precision pipeline: both sources activated bf16 tensors
        return low.alpha is not None and skip.alpha is not None and _is_b16(low.x) and \
            bool(lib().unet_conv_up_in_fwd_b16_supported(N, H, W, low.shape[3], C1, Cout))
    return bool(lib().unet_conv_up_in_fwd_supported(N, H, W, low.shape[3], C1, Cout))


def conv_up_wino_supported(N, H, W, C0, C1, Cout):
    """Winograd form of conv_up_in_fwd for output [N,H,W,Cout], low-res source C0, skip C1?"""
    return bool(lib().unet_conv_up_wino_supported(N, H, W, C0, C1, Cout))


def conv_up_in_fwd(low, skip, slope, wf, bias, gamma, beta, eps, mask, wu=None, w3=None):
    """y = conv3x3(cat(upsample2x(act(low)), act(skip))) + bias with the up-sampling in the
    loader, plus the InstanceNorm statistics of y (as conv_in_fwd).  wu: the Winograd forward
    form of the weight (shape checked by the caller with conv_up_wino_supported).  bf16 sources
    (the mixed-precision pipeline): y is bf16, w3 = the bf16-rounded weight plane or None."""
    low, rl = _act(low)
    skip, rs = _act(skip)
    N, H, W, C1 = skip.shape
    C0 = low.shape[3]
    assert low.shape[1] * 2 == H and low.shape[2] * 2 == W and low.shape[0] == N
    Cout = wf.shape[1]
    assert wf.shape[0] == 9 and wf.shape[2] == C0 + C1
    b16 = _is_b16(skip.x)
    if b16:     # takes the bf16-rounded weight plane (or NULL), has no Winograd form
        fn, head = lib().unet_conv_up_in_fwd_b16, (rl, rs, slope, _ptr(wf), _ptr(w3), _ptr(bias))
    elif wu is not None:
        fn, head = lib().unet_conv_up_in_fwd_wino, (rl, rs, slope, _ptr(wu), _ptr(bias))
    else:
        fn, head = lib().unet_conv_up_in_fwd, (rl, rs, slope, _ptr(wf), _ptr(bias))
    y, st, ws, px, t0 = _conv_stats_launch(fn, head, b16, skip.x, N, H, W, Cout, 1)
    if t0 is not None:
        wino = not b16 and (wu is not None or (
            low.alpha is not None and skip.alpha is not None and
            bool(lib().unet_conv_up_c32_is_winograd(N, H, W, C0, C1, Cout))))
        _end_conv(t0, "conv_igemm_bf16" if b16 else "conv_igemm",
                  2.0 * N * H * W * 9 * (C0 + C1) * Cout, 1, wino)
    return _conv_stats_finalize(b16, y, st, ws, px, gamma, beta, eps, mask)


def conv_in_bwd_weight(x, slope, dy, dw_oihw, ci_offset, ksize, stride, x3=False):
    """Weight gradient of a fused layer: dw[:, ci_offset : ci_offset + Cx] = act(x) (x) dy.
    x3: the split-bf16 operand mode (fp32 tensors).  x a U8Image: the whole weight gradient of
    the normalising RGB stem (3x3, stride 1), for an fp32 or a bf16 dy."""
    u8 = isinstance(x, U8Image)
    if not u8:
        x, rx = _act(x)
    N, H, W, Cx = x.shape
    Cout = dy.shape[3]
    b16 = _is_b16(dy)
    sfx = "_bf16" if b16 else ("_bf16x3" if x3 else "")     # of the timer tag
    fn = _sel_conv_in_bwd_weight(u8, b16, bool(x3))
    if u8:
        ksize, stride = 3, 1
        head = (_ptr(x.x), *x.c_mean_std(), _ptr(dy), _ptr(dw_oihw))
    else:
        assert dw_oihw.shape[0] == Cout and dw_oihw.is_contiguous()
        head = (rx, slope, _ptr(dy), _ptr(dw_oihw), ci_offset, dw_oihw.shape[1], ksize, stride)
    ws = _wgrad_ws(lib().unet_conv3x3_bwd_weight_workspace_bytes(N, H, W, Cx, Cout, stride), dy)
    t0 = _begin("wgrad")
    check(fn(*head, _ptr(ws), ws.numel(), N, H, W, Cout, _stream()))
    if t0 is not None:
        wino = not u8 and not b16 and not x3 and ksize == 3 and \
            bool(lib().unet_conv3x3_bwd_weight_is_winograd(N, H, W, Cx, Cout, stride))
        Ho, Wo = (H, W) if u8 else dy.shape[1:3]
        _end_conv(t0, "conv_stem_wgrad" if Cx == 3 else "conv_wgrad" + sfx,
                  2.0 * N * Ho * Wo * ksize * ksize * Cx * Cout, 2, wino)
    return dw_oihw


def stem_in_bwd_weight_fold_supported(x, g):
    """Can stem_in_bwd_weight_fold take the stem's operand `x` (Act of the fp32 image, or a
    U8Image) and the gradient g of its output?  (fp32 tensors in the raw-row kernel's widths)"""
    xt = x.x if isinstance(x, (Act, U8Image)) else x
    return g.dtype == torch.float32 and xt.shape[3] == 3 and xt.shape[2] % 128 == 0 and \
        xt.dtype in (torch.float32, torch.uint8) and getattr(x, "alpha", None) is None


def stem_in_bwd_weight_fold(x, g, y, mean, rstd, gamma, beta, mask, slope, partials, dw_oihw,
                            dgamma, dbeta, dbias):
    """instnorm_lrelu_drop_bwd(g, ..., partials=partials) and conv_in_bwd_weight(x, ...) of the RGB
    stem as one call that never stores the layer's dL/dz (nothing else reads it when no gradient
    is taken with respect to the image): the weight gradient's loader forms it from g and y."""
    u8 = isinstance(x, U8Image)
    if not u8 and not isinstance(x, Act):
        x = Act(x)
    N, H, W, _ = x.shape
    Cout = g.shape[3]
    if u8:
        img = (None, _ptr(x.x), *x.c_mean_std())
    else:
        if x.alpha is not None:
            raise ValueError("the RGB image is a plain operand")
        img = (_ptr(x.x), None, None, None)
    ws = _wgrad_ws(lib().unet_stem_in_bwd_weight_fold_workspace_bytes(N, H, W, Cout), g)
    t0 = _begin("wgrad")
    check(lib().unet_stem_in_bwd_weight_fold(
        *img, _ptr(g), _ptr(y), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), _ptr(mask), slope,
        _ptr(partials[0]), partials[1], _ptr(dw_oihw), _ptr(dgamma), _ptr(dbeta), _ptr(dbias),
        _ptr(ws), ws.numel(), N, H, W, Cout, _stream()))
    if t0 is not None:
        _end_conv(t0, "conv_stem_wgrad", 2.0 * N * H * W * 27 * Cout, 3, False)
    return dw_oihw


def conv_in_bwd_weight_fold32_supported(x, g):
    """Can conv_in_bwd_weight_fold32 take the operand `x` and the gradient g of the layer's output?
    (fp32 tensors of a shape conv_in_bwd_weight runs on the 32-channel Winograd kernel under the
    calling thread's c32 switch)"""
    xt = x.x if isinstance(x, Act) else x
    if isinstance(x, U8Image) or xt.dtype != torch.float32 or g.dtype != torch.float32 or \
            xt.shape[:3] != g.shape[:3]:
        return False
    N, H, W, Cx = xt.shape
    return bool(lib().unet_conv_in_bwd_weight_fold32_supported(N, H, W, Cx, g.shape[3]))


def conv_in_bwd_weight_fold32(x, slope_x, g, y, mean, rstd, gamma, beta, mask, slope, partials,
                              dw_oihw, ci_offset, dgamma, dbeta, dbias):
    """instnorm_lrelu_drop_bwd(g, ..., partials=partials) and conv_in_bwd_weight(x, slope_x, dz,
    dw_oihw, ci_offset, 3, 1) of a 32 -> 32 channel layer as one call: the weight gradient forms
    the layer's dL/dz from g and y and stores it over g in place (the separate pass over the
    tensor is gone).  Returns g, which now holds dL/dz."""
    x, rx = _act(x)
    N, H, W, _ = x.shape
    assert dw_oihw.shape[0] == 32 and dw_oihw.is_contiguous() and g.is_contiguous()
    ws = _wgrad_ws(lib().unet_conv_in_bwd_weight_fold32_workspace_bytes(N, H, W), g)
    t0 = _begin("wgrad")
    check(lib().unet_conv_in_bwd_weight_fold32(
        rx, slope_x, _ptr(g), _ptr(y), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), _ptr(mask),
        slope, _ptr(partials[0]), partials[1], _ptr(dw_oihw), ci_offset, dw_oihw.shape[1],
        _ptr(dgamma), _ptr(dbeta), _ptr(dbias), _ptr(ws), ws.numel(), N, H, W, _stream()))
    if t0 is not None:
        _end_conv(t0, "conv_wgrad", 2.0 * N * H * W * 9 * 32 * 32, 3, True)
    return g


def upsample2x_in_fwd(x, slope):
    x, rx = _act(x)
    N, h, w, C = x.shape
    b16 = _is_b16(x.x)
    up = (_b16 if b16 else _f32)((N, 2 * h, 2 * w, C), x.x)
    t0 = _begin()
    check(_twin("unet_upsample2x_in_fwd", b16)(rx, slope, _ptr(up), N, h, w, _stream()))
    if t0 is not None:
        _timer.end("upsample2x_fwd", 0.0, 1, t0,
                   nbytes=x.x.element_size() * (x.x.numel() + up.numel()))
    return up


def upsample2x_bwd_taps(dy):
    """D[N, h, w, 9*C] = the nine transposed-upsampled shifts of dy[N, 2h, 2w, C] (tap-major)."""
    N, H2, W2, C = dy.shape
    b16 = _is_b16(dy)
    D = (_b16 if b16 else _f32)((N, H2 // 2, W2 // 2, 9 * C), dy)
    t0 = _begin()
    check(_twin("unet_upsample2x_bwd_taps", b16)(_ptr(dy), _ptr(D), N, H2 // 2, W2 // 2, C,
                                                 _stream()))
    if t0 is not None:   # reads dy once, writes 9/4 of it
        _timer.end("upsample2x_bwd_taps", 0.0, 1, t0,
                   nbytes=dy.element_size() * dy.numel() * (1 + 9 / 4))
    return D


def conv3x3_up_bwd_weight(x, slope, D, dw_oihw, ci_offset):
    """dw[:, ci_offset : ci_offset + Cx] of conv3x3(upsample2x(act(x))) from D (low-res GEMM)."""
    x, rx = _act(x)
    N, h, w, Cx = x.shape
    Cout = D.shape[3] // 9
    assert D.shape[:3] == x.shape[:3] and dw_oihw.shape[0] == Cout and dw_oihw.is_contiguous()
    ws = _wgrad_ws(lib().unet_conv3x3_up_bwd_weight_workspace_bytes(N, h, w, Cx, Cout), D)
    b16 = _is_b16(D)
    t0 = _begin("wgrad")
    check(_twin("unet_conv3x3_up_bwd_weight", b16)(
        rx, slope, _ptr(D), _ptr(dw_oihw), ci_offset, dw_oihw.shape[1], _ptr(ws), ws.numel(), N, h,
        w, Cout, _stream()))
    if t0 is not None:
        _end_lowres(t0, "conv_wgrad_bf16" if b16 else "conv_wgrad", N, h, w, Cx, Cout, 2)
    return dw_oihw


@functools.lru_cache(maxsize=None)
def _sel_conv3x3_up_bwd_data(b16, has_wd3, has_nxt):
    """-> (entry point, takes the bf16-rounded weights wd3, takes unet_bwd_stats, timer tag)"""
    wb = b16 and has_wd3
    bs = wb or has_nxt
    return (_export("unet_conv3x3_up_bwd_data" + ("_bs" if bs else "") + ("_b16" if b16 else "") +
                    ("_wb" if wb else "")), wb, bs, "conv_igemm_bf16" if b16 else "conv_igemm")


def conv3x3_up_bwd_data(D, wd, ci_offset, ccols, out=None, accumulate=False, nxt=None, wd3=None):
    """g[N, h, w, ccols] (+)= dL/d(low-res operand) of conv3x3(upsample2x(.)) from D.
    nxt (NextNorm): g is final for that layer - also emit its backward reductions.
    wd3 (bf16 tensors only): the data-gradient weights pre-rounded to bf16 (plain-GEMM form)."""
    N, h, w, C9 = D.shape
    Cout = C9 // 9
    cin_total = wd.shape[1]
    assert wd.shape[0] == 9 and wd.shape[2] == Cout
    b16 = _is_b16(D)
    g = out if out is not None else (_b16 if b16 else _f32)((N, h, w, ccols), D)
    fn, planes, takes_bs, tag = _sel_conv3x3_up_bwd_data(b16, wd3 is not None, nxt is not None)
    w3 = (_ptr(wd3),) if planes else ()
    args = (_ptr(D), _ptr(wd), *w3, cin_total, ci_offset, _ptr(g), N, h, w, Cout, ccols,
            1 if accumulate else 0)
    t0 = _begin("conv")
    if takes_bs:
        _call_nxt(fn, args, nxt)
    else:
        check(fn(*args, _stream()))
    if t0 is not None:
        _end_lowres(t0, tag, N, h, w, ccols, Cout, 1)
    return g


def head1x1_in_fwd(x, slope, w, b):
    x, rx = _act(x)
    N, H, W, C = x.shape
    K = w.shape[0]
    logits = _f32((N, K, H, W), x.x)
    t0 = _begin()
    check(_twin("unet_head1x1_in_fwd", _is_b16(x.x))(rx, slope, _ptr(w), _ptr(b), _ptr(logits), N,
                                                     H * W, K, _stream()))
    if t0 is not None:
        _timer.end("head_fwd", 0.0, 1, t0,
                   nbytes=x.x.element_size() * x.x.numel() + 4.0 * logits.numel())
    return logits


def head1x1_in_bwd(x, slope, dlogits, w, dw, db, nxt=None):
    """nxt (NextNorm of the layer whose raw output x.x is): also leave the reductions of that
    layer's InstanceNorm backward (nxt.tiles == 0: this shape has no such epilogue)."""
    x, rx = _act(x)
    N, H, W, C = x.shape
    K = w.shape[0]
    da = torch.empty_like(x.x)
    ws = _ws(lib().unet_head1x1_bwd_workspace_bytes(N, H * W, C, K), x.x)
    args = (rx, slope, _ptr(dlogits), _ptr(w), _ptr(da), _ptr(dw), _ptr(db), _ptr(ws), ws.numel(),
            N, H * W, K)
    fn = _twin("unet_head1x1_in_bwd" + ("_bs" if nxt is not None else ""), _is_b16(x.x))
    t0 = _begin()
    if nxt is not None:
        _call_nxt(fn, args, nxt)
    else:
        check(fn(*args, _stream()))
    if t0 is not None:
        _timer.end("head_bwd", 0.0, 2, t0,
                   nbytes=da.element_size() * 2 * da.numel() + 4.0 * dlogits.numel())
    return da


def head1x1_in_bwd_fold(x, slope, dlogits, w, dw, db, nxt, dgamma, dbeta, dbias):
    """head1x1_in_bwd(..., nxt) and the InstanceNorm + LeakyReLU + dropout backward of nxt's
    layer in one call (fp32 tensors): with `nxt.applied` set on return the result is that layer's
    dL/dz - da was never stored - and dgamma / dbeta / dbias hold its parameter gradients;
    otherwise (this shape has no such form) the result is da, as head1x1_in_bwd left it."""
    x, rx = _act(x)
    N, H, W, C = x.shape
    K = w.shape[0]
    dz = torch.empty_like(x.x)
    ws = _ws(lib().unet_head1x1_in_bwd_fold_workspace_bytes(N, H * W, K), x.x)
    t0 = _begin()
    _call_nxt(lib().unet_head1x1_in_bwd_fold,
              (rx, slope, _ptr(dlogits), _ptr(w), _ptr(dz), _ptr(dw), _ptr(db), _ptr(dgamma),
               _ptr(dbeta), _ptr(dbias), _ptr(ws), ws.numel(), N, H * W, K), nxt)
    nxt.applied = nxt.tiles > 0
    if t0 is not None:      # folded: y + dlogits in, twice; dz out
        _timer.end("head_bwd", 0.0, 4 if nxt.applied else 2, t0,
                   nbytes=4.0 * ((3 if nxt.applied else 2) * dz.numel() +
                                 (2 if nxt.applied else 1) * dlogits.numel()))
    return dz


# ---- bilinear 2x ---------------------------------------------------------------------
def upsample2x_fwd(x):
    N, h, w, C = x.shape
    y = _f32((N, 2 * h, 2 * w, C), x)
    check(lib().unet_upsample2x_fwd(_ptr(x), _ptr(y), N, h, w, C, _stream()))
    return y


def upsample2x_bwd(gy, out=None, accumulate=False):
    N, H2, W2, C = gy.shape
    h, w = H2 // 2, W2 // 2
    gx = out if out is not None else _f32((N, h, w, C), gy)
    check(lib().unet_upsample2x_bwd(_ptr(gy), _ptr(gx), N, h, w, C, 1 if accumulate else 0,
                                    _stream()))
    return gx


# ---- head + loss ---------------------------------------------------------------------
def head1x1_fwd(a, w, b):
    N, H, W, C = a.shape
    K = w.shape[0]
    logits = _f32((N, K, H, W), a)
    check(lib().unet_head1x1_fwd(_ptr(a), _ptr(w), _ptr(b), _ptr(logits), N, H * W, C, K,
                                 _stream()))
    return logits


def head1x1_bwd(a, dlogits, w, dw, db):
    N, H, W, C = a.shape
    K = w.shape[0]
    da = torch.empty_like(a)
    ws = _ws(lib().unet_head1x1_bwd_workspace_bytes(N, H * W, C, K), a)
    check(lib().unet_head1x1_bwd(_ptr(a), _ptr(dlogits), _ptr(w), _ptr(da), _ptr(dw), _ptr(db),
                                 _ptr(ws), ws.numel(), N, H * W, C, K, _stream()))
    return da


MAX_CLASSES = 32     # UNET_MAX_CLASSES: one 32-column matrix-core tile, per-class sums in registers


def _check_classes(K, what):
    """2..MAX_CLASSES classes, refused on the host before any launch."""
    if not 2 <= K <= MAX_CLASSES:
        raise ValueError(f"{what}: {K} classes; the HIP tail (head, loss, counts) covers 2 to "
                         f"{MAX_CLASSES} classes (the cap is one 32-column matrix-core tile)")


def _target_twin(name, target):
    """The export `name` for an int64 target, its `_u8` twin for the dataset's uint8 mask."""
    if target.dtype == torch.uint8:
        return _export(name + "_u8")
    if target.dtype != torch.int64:
        raise TypeError(f"{name}: the target is int64 or uint8 (got {target.dtype})")
    return _export(name)


def dice_wce_loss_fwd_bwd(logits, target, smooth, w_dice, w_ce, ignore_index, dynamic_weights,
                          class_weights=None, grad_scale=1.0, want_grad=True, ws=None):
    """ws: a caller-kept workspace (dice_wce_loss_workspace) - needed when the gradient is taken
    later with dice_wce_loss_grad (want_grad=False here).  target: int64 labels, or (here and in
    the four functions below) the dataset's uint8 mask as it is - raw or cleaned, 1 byte a pixel."""
    N, K, H, W = logits.shape
    _check_classes(K, "dice_wce_loss_fwd_bwd")
    if class_weights is not None and class_weights.numel() != K:
        raise ValueError(f"class_weights holds {class_weights.numel()} values for {K} classes")
    # out = {loss, ce, dice, w[0..K-1]}; 8 floats at 3 classes, as ever (the last two unused)
    out = _f32((8 if K == 3 else 3 + K,), logits)
    dl = torch.empty_like(logits) if want_grad else None
    if ws is None:
        ws = dice_wce_loss_workspace(logits)
    check(_target_twin("unet_dice_wce_lossk_fwd_bwd", target)(
        _ptr(logits), _ptr(target), _ptr(out), _ptr(dl), _ptr(ws), ws.numel(), N, K, H, W,
        smooth, w_dice, w_ce, ignore_index, 1 if dynamic_weights else 0, _ptr(class_weights),
        grad_scale, _stream()))
    return out, dl


def dice_wce_loss_workspace(logits):
    N, K, H, W = logits.shape
    _check_classes(K, "dice_wce_loss_workspace")
    nbytes = lib().unet_dice_wce_lossk_workspace_bytes(N, K, H, W)
    # (at 3 classes a batch outside the limit has always been refused by the call that follows)
    if nbytes == 0 and K != 3:
        raise ValueError(f"dice_wce_loss: a batch of {N} images is outside the 1..1024 the "
                         "loss kernels take per call")
    return _ws(nbytes, logits)


def dice_wce_loss_grad(logits, target, ws, upstream, ignore_index):
    """dL/dlogits of a loss whose forward ran with want_grad=False on the workspace `ws`
    (dice_wce_loss_fwd_bwd(..., ws=ws) or dice_wce_loss_shard_apply): upstream (a device float,
    dL/dloss from autograd, or None = 1) is applied inside the gradient kernel."""
    N, K, H, W = logits.shape
    dl = torch.empty_like(logits)
    if upstream is not None:
        upstream = upstream.reshape(1).float().contiguous()
    _check_classes(K, "dice_wce_loss_grad")
    check(_target_twin("unet_dice_wce_lossk_grad", target)(
        _ptr(logits), _ptr(target), _ptr(ws), ws.numel(), _ptr(upstream), _ptr(dl), N, K, H, W,
        ignore_index, _stream()))
    return dl


def dice_wce_loss_shard_stats(logits, target, smooth, ignore_index):
    """Phase 1 of the sharded-batch loss: (stats float64[10] on the device, workspace)."""
    N, K, H, W = logits.shape
    if K != 3:
        raise NotImplementedError("the sharded (batch_sync='global') loss covers exactly 3 "
                                  f"classes (got {K}); use batch_sync='local'")
    stats = torch.empty((10,), dtype=torch.float64, device=logits.device)
    ws = _ws(lib().unet_dice_wce_loss_workspace_bytes(N, H, W), logits)
    check(_target_twin("unet_dice_wce_loss_shard_stats", target)(
        _ptr(logits), _ptr(target), stats.data_ptr(), _ptr(ws), ws.numel(), N, H, W, smooth,
        ignore_index, _stream()))
    return stats, ws


def dice_wce_loss_shard_apply(logits, target, global_stats, n_global, ws, smooth, w_dice, w_ce,
                              ignore_index, dynamic_weights, class_weights=None, grad_scale=1.0,
                              want_grad=True):
    """Phase 2: loss of the concatenated batch (out[0]) and this shard's dL/dlogits."""
    N, K, H, W = logits.shape
    out = _f32((8,), logits)
    dl = torch.empty_like(logits) if want_grad else None
    check(_target_twin("unet_dice_wce_loss_shard_apply", target)(
        _ptr(logits), _ptr(target), global_stats.data_ptr(), int(n_global), _ptr(out), _ptr(dl),
        _ptr(ws), ws.numel(), N, H, W, smooth, w_dice, w_ce, ignore_index,
        1 if dynamic_weights else 0, _ptr(class_weights), grad_scale, _stream()))
    return out, dl


# ---- validation metrics / input pipeline ---------------------------------------------------
def argmax_dice_counts(logits, target, ignore_index=255, want_preds=True):
    """Returns (preds uint8 [N,H,W] or None, counts int64 [K,3] = per class
    {intersection, predicted, labelled}); everything stays on the device.  target: int64 labels
    or the dataset's uint8 mask."""
    N, K, H, W = logits.shape
    _check_classes(K, "argmax_dice_counts")
    logits, target = logits.contiguous(), target.contiguous()
    if logits.dtype != torch.float32 or target.dtype not in (torch.int64, torch.uint8):
        raise TypeError("argmax_dice_counts takes fp32 logits and int64 (or uint8) targets")
    preds = torch.empty((N, H, W), dtype=torch.uint8, device=logits.device) if want_preds else None
    counts = torch.empty((K, 3), dtype=torch.int64, device=logits.device)
    check(_target_twin("unet_argmax_countsk", target)(
        _ptr(logits), _ptr(target), _ptr(preds), counts.data_ptr(), N, K, H, W, ignore_index,
        _stream()))
    return preds, counts


def argmax_classes(logits):
    """uint8 [N,H,W] class map of fp32 logits [N,K,H,W] (first maximum wins, like torch.argmax)."""
    N, K, H, W = logits.shape
    if logits.dtype != torch.float32:
        raise TypeError("argmax_classes takes fp32 logits")
    _check_classes(K, "argmax_classes")
    logits = logits.contiguous()
    preds = torch.empty((N, H, W), dtype=torch.uint8, device=logits.device)
    check(lib().unet_argmax_countsk(_ptr(logits), None, _ptr(preds), None, N, K, H, W, 255,
                                    _stream()))
    return preds


def _eval_operands(name, logits, target, any_k=False):
    """any_k: the caller has a K-class form; otherwise K != 3 is refused (NotImplementedError,
    before the device is touched)."""
    if torch.is_tensor(logits) and logits.dim() == 4 and logits.shape[1] != 3:
        if not any_k:
            raise NotImplementedError(f"{name} covers exactly 3 classes (the three-colour maps "
                                      f"of the pet trimap); got {logits.shape[1]}")
        _check_classes(logits.shape[1], name)
    if not torch.is_tensor(logits) or not logits.is_cuda:
        raise RuntimeError(f"unet-implementations_amd.{name} runs on MI355X only "
                           "(no CPU fallback exists)")
    if logits.dim() != 4:
        raise ValueError("logits [B, K, H, W] expected")
    if logits.dtype != torch.float32:
        raise TypeError(f"{name} takes fp32 logits")
    if target is not None:
        if target.dtype != torch.int64:
            raise TypeError(f"{name} takes int64 targets")
        if tuple(target.shape) != (logits.shape[0],) + tuple(logits.shape[2:]):
            raise ValueError("target must be [B, H, W] of the logits' size")
        target = target.contiguous()
    return logits.contiguous(), target


def eval_confusion(logits, target, dims=None, ignore_index=255):
    """Per-image confusion matrices int64 [B, K, K] = [target class][predicted class] of the
    argmax map and the mask, both nearest-resized to dims[b] = (orig_h, orig_w): the counting of
    evaluate_model (src/evaluate.py:189-211) in one launch.  dims: int64 [B, 2] on the device
    (never read on the host), or None for "at network size".  A size outside 1..16384 gives that
    image zero counts."""
    logits, target = _eval_operands("eval_confusion", logits, target, any_k=True)
    if target is None:
        raise TypeError("eval_confusion needs the target")
    B, K, H, W = logits.shape
    if dims is not None:
        if not torch.is_tensor(dims) or dims.dtype != torch.int64 or tuple(dims.shape) != (B, 2):
            raise TypeError("dims must be an int64 [B, 2] tensor of (orig_h, orig_w)")
        dims = dims.contiguous()
    cm = torch.empty((B, K, K), dtype=torch.int64, device=logits.device)
    check(lib().unet_eval_confusionk(_ptr(logits), _ptr(target), _ptr(dims), cm.data_ptr(), B, K,
                                     H, W, int(ignore_index), _stream()))
    return cm


def eval_maps(logits, target=None, want_probs=True, want_classes=True, want_errors=None):
    """(probs fp32 [B,3,H,W], classes uint8 [B,H,W], errors uint8 [B,H,W]) from one read of the
    logits; an output that was not asked for is None.  errors (default: when a target is given)
    holds the categories of create_error_visualization (utils/visualize.py:205-222): 0 none,
    1 true positive, 2 false positive, 3 false negative, 4 wrong class, 255 read as background."""
    logits, target = _eval_operands("eval_maps", logits, target)
    if want_errors is None:
        want_errors = target is not None
    if want_errors and target is None:
        raise TypeError("eval_maps: the error map needs the target")
    B, _, H, W = logits.shape
    probs = torch.empty_like(logits) if want_probs else None
    classes = torch.empty((B, H, W), dtype=torch.uint8, device=logits.device) \
        if want_classes else None
    errors = torch.empty((B, H, W), dtype=torch.uint8, device=logits.device) \
        if want_errors else None
    check(lib().unet_eval_maps(_ptr(logits), _ptr(target) if want_errors else None, _ptr(probs),
                               _ptr(classes), _ptr(errors), B, H, W, _stream()))
    return probs, classes, errors


# ---- mask post-processing (postprocess.hip; definitions: include/unet_hip.h) ------------------
CC_MODES = {"foreground": 0, "class": 1, "background": 2}      # UNET_CC_*
CLEANUP_VOTES = {None: 0, "image": 1, "component": 2}          # UNET_VOTE_*
_rc = check     # (cc_label and mask_cleanup have a `check` argument of their own)


def _class_map(name, classes, num_classes):
    """A uint8 [B, H, W] class map on the device; what is wrong with the tensor itself is said
    before the device is asked for anything."""
    if not torch.is_tensor(classes):
        raise TypeError(f"{name} takes a uint8 [B, H, W] tensor (got {type(classes).__name__})")
    if classes.dtype != torch.uint8:
        raise TypeError(f"{name} takes a uint8 class map (got {classes.dtype})")
    if classes.dim() != 3 or 0 in classes.shape:
        raise ValueError(f"{name}: class map [B, H, W] expected (got {tuple(classes.shape)})")
    _check_classes(int(num_classes), name)
    if not classes.is_cuda:
        raise RuntimeError(f"unet-implementations_amd.{name} runs on MI355X only "
                           "(no CPU fallback exists)")
    return classes.contiguous()


def postprocess_status(workspace):
    """The status word of a cc_label / mask_cleanup workspace (one device-to-host read): 0 when
    every bounded loop of the kernels ended by itself."""
    return int(workspace[:4].view(torch.int32).item())


def _check_status(name, workspace):
    status = postprocess_status(workspace)
    if status:
        raise RuntimeError(f"{name}: a bounded loop of the labelling kernels ran into its limit "
                           f"(status {status:#x}); the result is not valid")


def cc_label(classes, connectivity=8, mode="foreground", num_classes=32, check=False,
             workspace=None):
    """(labels, areas), both uint32 [B, H, W]: the connected components of a uint8 class map.
    labels = 0 on unselected pixels, otherwise 1 + the raster index (within the image) of the
    component's first pixel; areas = the component's pixel count at that pixel, 0 elsewhere.
    check=True reads the workspace's status word afterwards (a host sync) and raises if a kernel
    loop ran into its bound."""
    if mode not in CC_MODES:
        raise ValueError(f"cc_label: mode is one of {sorted(CC_MODES)} (got {mode!r})")
    if connectivity not in (4, 8):
        raise ValueError(f"cc_label: connectivity is 4 or 8 (got {connectivity!r})")
    classes = _class_map("cc_label", classes, num_classes)
    B, H, W = classes.shape
    need = lib().unet_cc_workspace_bytes(B, H, W)
    if need == 0:
        raise ValueError(f"cc_label: shape {tuple(classes.shape)} is outside B <= 65535, "
                         "H, W <= 16384, H * W <= 2^30")
    ws = workspace if workspace is not None else _ws(need, classes)
    labels = torch.empty((B, H, W), dtype=torch.uint32, device=classes.device)
    areas = torch.empty((B, H, W), dtype=torch.uint32, device=classes.device)
    _rc(lib().unet_cc_label_u8(_ptr(classes), labels.data_ptr(), areas.data_ptr(), _ptr(ws),
                               ws.numel(), B, int(num_classes), H, W, connectivity, CC_MODES[mode],
                               _stream()))
    if check:
        _check_status("cc_label", ws)
    return labels, areas


def mask_cleanup_workspace(classes, num_classes):
    """A workspace for mask_cleanup of maps of this shape (16 bytes a pixel)."""
    B, H, W = classes.shape
    need = lib().unet_mask_cleanup_workspace_bytes(B, int(num_classes), H, W)
    if need == 0:
        raise ValueError(f"mask_cleanup: shape {tuple(classes.shape)} is outside B <= 65535, "
                         "H, W <= 16384, H * W <= 2^30")
    return _ws(need, classes)


def mask_cleanup(classes, num_classes, vote=None, keep_largest=False, min_area=0,
                 fill_holes=False, max_hole_area=0, connectivity=8, out=None, check=False,
                 workspace=None):
    """The cleaned uint8 [B, H, W] map: component removal, class vote and hole filling in the
    order and with the definitions of include/unet_hip.h.  out: the destination (may be `classes`
    itself); check=True reads the status word afterwards (a host sync)."""
    if vote not in CLEANUP_VOTES:
        raise ValueError(f"mask_cleanup: vote is None, 'image' or 'component' (got {vote!r})")
    if connectivity not in (4, 8):
        raise ValueError(f"mask_cleanup: connectivity is 4 or 8 (got {connectivity!r})")
    if int(min_area) < 0 or int(max_hole_area) < 0:
        raise ValueError("mask_cleanup: min_area and max_hole_area are >= 0")
    classes = _class_map("mask_cleanup", classes, num_classes)
    B, H, W = classes.shape
    if out is None:
        out = torch.empty_like(classes)
    elif out.dtype != torch.uint8 or out.shape != classes.shape or not out.is_contiguous() or \
            out.device != classes.device:
        raise ValueError("mask_cleanup: out must be a contiguous uint8 tensor of the map's shape "
                         "on its device")
    ws = workspace if workspace is not None else mask_cleanup_workspace(classes, num_classes)
    _rc(lib().unet_mask_cleanup_u8(_ptr(classes), _ptr(out), _ptr(ws), ws.numel(), B,
                                   int(num_classes), H, W, connectivity, CLEANUP_VOTES[vote],
                                   1 if keep_largest else 0, int(min_area),
                                   1 if fill_holes else 0, int(max_hole_area), _stream()))
    if check:
        _check_status("mask_cleanup", ws)
    return out


def eval_confusion_classes(preds, target, dims=None, num_classes=3, ignore_index=255):
    """eval_confusion with the uint8 class map `preds` [B, H, W] in place of the logits' argmax (a
    byte >= num_classes reads as 0): int64 [B, K, K] = [target class][predicted class], both maps
    nearest-resized to dims[b] (int64 [B, 2] on the device, never read on the host; None = at
    network size)."""
    if torch.is_tensor(target) and target.dtype != torch.int64:
        raise TypeError("eval_confusion_classes takes int64 targets")
    preds = _class_map("eval_confusion_classes", preds, num_classes)
    B, H, W = preds.shape
    K = int(num_classes)
    if not torch.is_tensor(target) or tuple(target.shape) != (B, H, W):
        raise ValueError("target must be [B, H, W] of the class map's size")
    target = target.contiguous()
    if dims is not None:
        if not torch.is_tensor(dims) or dims.dtype != torch.int64 or tuple(dims.shape) != (B, 2):
            raise TypeError("dims must be an int64 [B, 2] tensor of (orig_h, orig_w)")
        dims = dims.contiguous()
    cm = torch.empty((B, K, K), dtype=torch.int64, device=preds.device)
    check(lib().unet_eval_confusion_classes(_ptr(preds), _ptr(target), _ptr(dims), cm.data_ptr(),
                                            B, K, H, W, int(ignore_index), _stream()))
    return cm


# ---- ragged uint8 batches to network size (letterbox.hip) ------------------------------------
LETTERBOX_FIELDS = 8    # UNET_LETTERBOX_FIELDS: image offset, mask offset, h, w, out_h, out_w,
#                         pad_y, pad_x


def _ragged_operands(name, arena, table):
    if not torch.is_tensor(arena) or not arena.is_cuda:
        raise RuntimeError(f"unet-implementations_amd.{name} runs on MI355X only "
                           "(no CPU fallback exists)")
    if arena.dtype != torch.uint8 or arena.dim() != 1:
        raise TypeError(f"{name}: the arena is a flat uint8 tensor")
    if not torch.is_tensor(table) or table.dtype != torch.int64 or table.dim() != 2 or \
            table.shape[1] != LETTERBOX_FIELDS or table.shape[0] < 1:
        raise TypeError(f"{name}: the table is int64 [B, {LETTERBOX_FIELDS}]")
    if table.device != arena.device:
        raise ValueError(f"{name}: the table lives on the arena's device (it is never read on "
                         "the host)")
    return arena.contiguous(), table.contiguous()


def letterbox_u8(arena, table, size, want_mask=True, lut=None, out=None):
    """(images uint8 [B, S_h, S_w, 3], masks uint8 [B, S_h, S_w] or None): every sample of a
    ragged batch resized and placed in its tile in one launch (`unet_letterbox_u8`; cv2.resize's
    fixed-point INTER_LINEAR for the image, INTER_NEAREST for the mask, zero padding).
    arena: flat uint8 device tensor holding the samples; table: int64 [B, 8] device tensor of
    (image offset, mask offset or -1, h, w, out_h, out_w, pad_y, pad_x) - `dataprep` builds both.
    size: S or (S_h, S_w).  lut: uint8 [B, 256], applied to the mask bytes.  out: (images, masks)
    to write into."""
    arena, table = _ragged_operands("letterbox_u8", arena, table)
    S_h, S_w = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    B = table.shape[0]
    if lut is not None:
        if not want_mask:
            raise ValueError("letterbox_u8: a lut needs the mask output")
        if lut.dtype != torch.uint8 or tuple(lut.shape) != (B, 256) or lut.device != arena.device:
            raise TypeError("letterbox_u8: lut is uint8 [B, 256] on the arena's device")
        lut = lut.contiguous()
    images, masks = out if out is not None else (None, None)
    if images is None:
        images = torch.empty((B, max(S_h, 0), max(S_w, 0), 3), dtype=torch.uint8,
                             device=arena.device)
    if want_mask and masks is None:
        masks = torch.empty((B, max(S_h, 0), max(S_w, 0)), dtype=torch.uint8, device=arena.device)
    if tuple(images.shape) != (B, S_h, S_w, 3) or images.dtype != torch.uint8 or \
            (want_mask and (tuple(masks.shape) != (B, S_h, S_w) or masks.dtype != torch.uint8)):
        raise ValueError("letterbox_u8: out must be uint8 [B, S_h, S_w, 3] and [B, S_h, S_w]")
    check(lib().unet_letterbox_u8(_ptr(arena), arena.numel(), _ptr(table), B, S_h, S_w,
                                  _ptr(images), _ptr(masks) if want_mask else None, _ptr(lut),
                                  _stream()))
    return images, (masks if want_mask else None)


def byte_histogram_u8(arena, table=None):
    """int64 [B, 256]: how often every byte value occurs in each sample's mask at its original
    size (`unet_byte_histogram_u8`, one launch).  arena / table as for `letterbox_u8`; with
    table=None, `arena` is a contiguous uint8 [B, H, W] mask batch."""
    if table is None:
        if not torch.is_tensor(arena) or arena.dim() != 3 or arena.dtype != torch.uint8:
            raise TypeError("byte_histogram_u8: without a table, a uint8 [B, H, W] mask batch")
        B, H, W = arena.shape
        rows = [[-1, b * H * W, H, W, 0, 0, 0, 0] for b in range(B)]
        table = torch.tensor(rows, dtype=torch.int64).to(arena.device, non_blocking=True)
        arena = arena.contiguous().view(-1)
    arena, table = _ragged_operands("byte_histogram_u8", arena, table)
    hist = torch.empty((table.shape[0], 256), dtype=torch.int64, device=arena.device)
    check(lib().unet_byte_histogram_u8(_ptr(arena), arena.numel(), _ptr(table), table.shape[0],
                                       hist.data_ptr(), _stream()))
    return hist


# ---- evaluation pictures (render.hip) --------------------------------------------------------
RENDER_PANELS = ("image", "gt", "pred", "error", "conf0", "conf1", "conf2", "target", "heat")
_RENDER_NEEDS_MASK = ("gt", "error", "target")
_RENDER_NEEDS_LOGITS = ("pred", "error", "conf0", "conf1", "conf2")
_jet_tables = {}


def _jet_table(device):
    """The jet colour table uint8 [256, 3] on `device` (uploaded once per device)."""
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    table = _jet_tables.get(key)
    if table is None:
        from .render import jet_lut
        table = _jet_tables[key] = torch.from_numpy(jet_lut()).to(device)
    return table


def _render_image(name, what, image):
    """(contiguous image, is_u8, B, H, W): fp32 [B,3,H,W] or uint8 [B,H,W,3] on the device."""
    if not torch.is_tensor(image) or image.dim() != 4 or not (
            (image.dtype == torch.uint8 and image.shape[3] == 3) or
            (image.dtype == torch.float32 and image.shape[1] == 3)):
        raise TypeError(f"{name}: {what} must be fp32 [B,3,H,W] or uint8 [B,H,W,3]")
    if not image.is_cuda:
        raise RuntimeError(f"unet-implementations_amd.{name} runs on MI355X only "
                           "(no CPU fallback exists)")
    if image.dtype == torch.uint8:
        B, H, W, _ = image.shape
        return image.contiguous(), 1, B, H, W
    B, _, H, W = image.shape
    return image.contiguous(), 0, B, H, W


def _render_out(name, out, shape, like):
    if out is None:
        return torch.empty(shape, dtype=torch.uint8, device=like.device)
    if not torch.is_tensor(out) or out.dtype != torch.uint8 or tuple(out.shape) != shape or \
            not out.is_contiguous() or out.device != like.device:
        raise TypeError(f"{name}: out must be a contiguous uint8 {list(shape)} tensor on the "
                        "image's device")
    return out


def render_seg_panels(image, logits, mask=None, heat=None, panels=("image", "gt", "pred"),
                      target_class=1, out=None):
    """uint8 [B, H, P, W, 3] on the device: the requested panels of every image side by side, one
    launch of `unet_render_seg_panels` (`.view(B * H, P * W, 3)` is the picture of the batch).
    image: fp32 [B,3,H,W] normalised with the ImageNet mean / std, or the uint8 [B,H,W,3] bytes
    (taken from the dtype).  logits: fp32 [B,3,H,W], or None when no panel needs them.  mask:
    int64 or uint8 [B,H,W]; heat: fp32 [B,H,W].  panels: 1 to 9 names of RENDER_PANELS, in order."""
    name = "render_seg_panels"
    panels = tuple(panels)
    if not 1 <= len(panels) <= 9:
        raise ValueError(f"{name}: 1 to 9 panels")
    for p in panels:
        if p not in RENDER_PANELS:
            raise ValueError(f"{name}: unknown panel {p!r} (one of {', '.join(RENDER_PANELS)})")
    if mask is None and any(p in _RENDER_NEEDS_MASK for p in panels):
        raise TypeError(f"{name}: the panels gt, error and target need the mask")
    if logits is None and any(p in _RENDER_NEEDS_LOGITS for p in panels):
        raise TypeError(f"{name}: the panels pred, error and conf0..2 need the logits")
    if heat is None and "heat" in panels:
        raise TypeError(f"{name}: the heat panel needs the heat map")
    image, image_u8, B, H, W = _render_image(name, "image", image)
    if logits is not None:
        logits, _ = _eval_operands(name, logits, None)
        if tuple(logits.shape) != (B, 3, H, W) or logits.device != image.device:
            raise ValueError(f"{name}: logits must be [B, 3, H, W] of the image's size and device")
    mask_u8 = 0
    if mask is not None:
        if not torch.is_tensor(mask) or mask.dtype not in (torch.int64, torch.uint8):
            raise TypeError(f"{name} takes int64 or uint8 masks")
        if tuple(mask.shape) != (B, H, W) or mask.device != image.device:
            raise ValueError(f"{name}: mask must be [B, H, W] of the image's size and device")
        mask, mask_u8 = mask.contiguous(), int(mask.dtype == torch.uint8)
    if heat is not None:
        if not torch.is_tensor(heat) or heat.dtype != torch.float32:
            raise TypeError(f"{name} takes an fp32 heat map")
        if tuple(heat.shape) != (B, H, W) or heat.device != image.device:
            raise ValueError(f"{name}: heat must be [B, H, W] of the image's size and device")
        heat = heat.contiguous()
    out = _render_out(name, out, (B, H, len(panels), W, 3), image)
    word = 0
    for k, p in enumerate(panels):
        word |= (RENDER_PANELS.index(p) + 1) << (4 * k)
    check(lib().unet_render_seg_panels(_ptr(image), image_u8, _ptr(logits), _ptr(mask), mask_u8,
                                       _ptr(heat), _ptr(_jet_table(image.device)),
                                       int(target_class), word, _ptr(out), B, H, W, _stream()))
    return out


def render_recon_panels(original, recon, out=None):
    """uint8 [B, H, 3, W, 3] on the device: original | reconstruction | error map per image
    (create_comparison_image of the autoencoder's visualize.py), `unet_render_recon_panels`.
    original: fp32 [B,3,H,W] in [0, 1] or the uint8 [B,H,W,3] bytes; recon: fp32 [B,3,H,W].  The
    error map is scaled by each image's own maximum difference."""
    name = "render_recon_panels"
    original, original_u8, B, H, W = _render_image(name, "original", original)
    if not torch.is_tensor(recon) or not recon.is_cuda:
        raise RuntimeError(f"unet-implementations_amd.{name} runs on MI355X only "
                           "(no CPU fallback exists)")
    if recon.dtype != torch.float32:
        raise TypeError(f"{name} takes an fp32 reconstruction")
    if tuple(recon.shape) != (B, 3, H, W) or recon.device != original.device:
        raise ValueError(f"{name}: recon must be [B, 3, H, W] of the original's size and device")
    recon = recon.contiguous()
    out = _render_out(name, out, (B, H, 3, W, 3), original)
    maxima = torch.empty(B, dtype=torch.int32, device=original.device)
    check(lib().unet_render_recon_panels(_ptr(original), original_u8, _ptr(recon),
                                         _ptr(_jet_table(original.device)), maxima.data_ptr(),
                                         _ptr(out), B, H, W, _stream()))
    return out


# ---- Grad-CAM (gradcam.hip) ------------------------------------------------------------------
def gradcam_workspace(N, HW, C, like):
    """The workspace the three Grad-CAM calls of one heatmap share."""
    return _ws(lib().unet_gradcam_workspace_bytes(N, HW, C), like)


def gradcam_weights(g, ws=None):
    """w fp32 [N, C] = mean over the pixels of g [N, h, w, C] (NHWC, fp32 or bf16)."""
    N, h, w_, C = g.shape
    ws = gradcam_workspace(N, h * w_, C, g) if ws is None else ws
    w = _f32((N, C), g)
    t0 = _begin()
    check(lib().unet_gradcam_weights(_ptr(g), 1 if _is_b16(g) else 0, _ptr(w), _ptr(ws),
                                     ws.numel(), N, h * w_, C, _stream()))
    if t0 is not None:
        _timer.end("gradcam_weights", 0.0, 2, t0, nbytes=float(g.element_size() * g.numel()))
    return w


def gradcam_map(a, slope, w, ws=None):
    """cam fp32 [N, h, w] = relu(sum_c w[n, c] * act(a)[n, :, :, c]); a: ops.Act (activated on
    load) or a plain NHWC tensor.  The per-workgroup minima / maxima stay in `ws` for
    gradcam_heatmap."""
    a, ra = _act(a)
    N, h, w_, C = a.shape
    if tuple(w.shape) != (N, C) or w.dtype != torch.float32:
        raise ValueError("w must be an fp32 [N, C] tensor")
    ws = gradcam_workspace(N, h * w_, C, a.x) if ws is None else ws
    cam = _f32((N, h, w_), a.x)
    t0 = _begin()
    check(lib().unet_gradcam_map(ra, 1 if _is_b16(a.x) else 0, slope, _ptr(w), _ptr(cam), _ptr(ws),
                                 ws.numel(), N, h * w_, _stream()))
    if t0 is not None:
        _timer.end("gradcam_map", 0.0, 1, t0,
                   nbytes=float(a.x.element_size() * a.x.numel() + 4 * cam.numel()))
    return cam, ws


def gradcam_heatmap(cam, ws, size):
    """fp32 [N, H, W]: cam [N, h, w] normalised per image (minus its minimum, over its range unless
    that is 0: then all zero) and resized bilinearly (align_corners=False) to size = (H, W).
    ws: what gradcam_map returned for this cam."""
    N, h, w_ = cam.shape
    H, W = int(size[0]), int(size[1])
    out = _f32((N, H, W), cam)
    check(lib().unet_gradcam_heatmap(_ptr(cam), _ptr(ws), ws.numel(), _ptr(out), N, h, w_, H, W,
                                     _stream()))
    return out


# ---- latent-space analysis (latent.hip) ------------------------------------------------------
TSNE_MAX_N = 8192


def _latent_matrix(name, x):
    """`name` takes a contiguous fp32 [N, D] matrix on the device, D a multiple of 4 -> (N, D)"""
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError(f"unet-implementations_amd.{name} runs on MI355X only "
                           "(no CPU fallback exists)")
    if x.dtype != torch.float32 or x.dim() != 2 or not x.is_contiguous():
        raise TypeError(f"{name} takes a contiguous fp32 [N, D] matrix")
    N, D = x.shape
    if not 2 <= N <= 65536 or D < 4 or D % 4:
        raise ValueError(f"{name}: N must lie in 2..65536 and D be a multiple of 4, got {N} x {D}")
    return N, D


def latent_col_mean(x):
    """mean fp32 [D] of x [N, D] over N, in a fixed order."""
    N, D = _latent_matrix("latent_col_mean", x)
    ws = _ws(lib().unet_latent_colsum_workspace_bytes(N, D), x)
    mean = _f32((D,), x)
    check(lib().unet_latent_col_mean(_ptr(x), _ptr(mean), _ptr(ws), ws.numel(), N, D, _stream()))
    return mean


def latent_gram_splitk(N, D):
    """How many slabs of D `latent_gram` sums for an [N, D] matrix."""
    return lib().unet_latent_gram_splitk(N, D)


def latent_gram(x, mean):
    """G fp32 [N, N] = (x - mean)(x - mean)^T on the fp32 matrix cores; bitwise symmetric."""
    N, D = _latent_matrix("latent_gram", x)
    if tuple(mean.shape) != (D,) or mean.dtype != torch.float32 or mean.device != x.device:
        raise ValueError("latent_gram: mean must be an fp32 [D] tensor on x's device")
    ws = _ws(lib().unet_latent_gram_workspace_bytes(N, D), x)
    g = _f32((N, N), x)
    t0 = _begin()
    check(lib().unet_latent_gram(_ptr(x), _ptr(mean), _ptr(g), _ptr(ws), ws.numel(), N, D,
                                 _stream()))
    if t0 is not None:
        _timer.end("latent_gram", 2.0 * N * N * D, 2, t0, executed=1.0 * N * (N + 128) * D)
    return g


def latent_gram_apply(g, q, out=None):
    """z fp32 [N, 8] = g @ q for the 8-column block q of the subspace iteration."""
    N = g.shape[0]
    if tuple(g.shape) != (N, N) or tuple(q.shape) != (N, 8) or g.dtype != torch.float32 or \
            q.dtype != torch.float32:
        raise ValueError("latent_gram_apply takes an fp32 [N, N] matrix and an fp32 [N, 8] block")
    z = _f32((N, 8), g) if out is None else out
    check(lib().unet_latent_gram_apply(_ptr(g), _ptr(q), _ptr(z), N, _stream()))
    return z


def latent_project(x, mean, w):
    """fp32 [2, D] = w^T (x - mean) for w [N, 2]: one pass over x."""
    N, D = _latent_matrix("latent_project", x)
    if tuple(w.shape) != (N, 2) or w.dtype != torch.float32 or tuple(mean.shape) != (D,):
        raise ValueError("latent_project takes an fp32 [D] mean and fp32 [N, 2] weights")
    ws = _ws(lib().unet_latent_colsum_workspace_bytes(N, D), x)
    out = _f32((2, D), x)
    check(lib().unet_latent_project(_ptr(x), _ptr(mean), _ptr(w), _ptr(out), _ptr(ws), ws.numel(),
                                    N, D, _stream()))
    return out


def tsne_joint_p(g, perplexity):
    """The joint probabilities P fp32 [N, N] of the exact t-SNE from the Gram matrix g (the squared
    distances are formed on load) -> (P, the conditional probabilities)."""
    N = g.shape[0]
    if tuple(g.shape) != (N, N) or g.dtype != torch.float32 or not g.is_cuda:
        raise ValueError("tsne_joint_p takes an fp32 [N, N] Gram matrix on the device")
    diag = g.diagonal().contiguous()
    pc, p = _f32((N, N), g), _f32((N, N), g)
    rowsum = torch.empty(N + 1, dtype=torch.float64, device=g.device)
    check(lib().unet_tsne_cond_p(_ptr(g), _ptr(diag), float(perplexity), _ptr(pc),
                                 rowsum.data_ptr(), N, _stream()))
    check(lib().unet_tsne_joint_p(_ptr(pc), rowsum.data_ptr(), _ptr(p), N, _stream()))
    return p, pc


def tsne_step(p, state_in, state_out, rows, exaggeration, momentum, lr, stats=None):
    """One descent iteration: state [N, 6] = (y, update, gains) from state_in to state_out; `stats`
    (a 2-element fp64 view, or None) receives the KL divergence and |gains grad| at state_in."""
    N = p.shape[0]
    check(lib().unet_tsne_step(_ptr(p), _ptr(state_in), _ptr(state_out), _ptr(rows),
                               None if stats is None else stats.data_ptr(), float(exaggeration),
                               float(momentum), float(lr), 0 if stats is None else 1, N,
                               _stream()))


def latent_scatter(centres, labels, palette, size, radius):
    """uint8 [H, W, 3]: the scatter picture of int32 [N, 2] pixel centres (x, y), uint8 [N] labels
    and a uint8 [K, 3] palette on a white ground."""
    H, W = int(size[0]), int(size[1])
    N, K = centres.shape[0], palette.shape[0]
    if not (centres.is_cuda and labels.is_cuda and palette.is_cuda):
        raise RuntimeError("unet-implementations_amd.latent_scatter runs on MI355X only "
                           "(no CPU fallback exists)")
    if centres.dtype != torch.int32 or tuple(centres.shape) != (N, 2) or \
            labels.dtype != torch.uint8 or tuple(labels.shape) != (N,) or \
            palette.dtype != torch.uint8 or tuple(palette.shape) != (K, 3):
        raise ValueError("latent_scatter takes int32 [N, 2] centres, uint8 [N] labels and a uint8 "
                         "[K, 3] palette")
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=centres.device)
    check(lib().unet_latent_scatter(centres.contiguous().data_ptr(), _ptr(labels.contiguous()),
                                    _ptr(palette.contiguous()), K, _ptr(out), N, H, W, int(radius),
                                    _stream()))
    return out


# ---- online batch augmentation (augment.hip) -------------------------------------------------
def _check_u8_image(what, image):
    """`what` (the caller) takes a contiguous uint8 [N,H,W,3] image on the device -> (N, H, W)"""
    if not torch.is_tensor(image) or not image.is_cuda:
        raise RuntimeError(f"unet-implementations_amd.{what} runs on MI355X only "
                           "(no CPU fallback exists)")
    if image.dim() != 4 or image.shape[3] != 3 or image.dtype != torch.uint8 or \
            not image.is_contiguous():
        raise TypeError(f"{what} takes a contiguous uint8 [N,H,W,3] image")
    return image.shape[:3]


def _check_record(kind, rec, N, k, device):
    """the record named `kind` ("params", "warp", "post", "light") is a contiguous fp32 [N, k]
    tensor on `device`"""
    if not torch.is_tensor(rec) or rec.dtype != torch.float32 or tuple(rec.shape) != (N, k) or \
            not rec.is_contiguous() or rec.device != device:
        raise TypeError(f"{kind} must be a contiguous fp32 [N, {k}] tensor on the image's device")


def _check_rng(rng, N, device):
    if rng is not None and (rng.element_size() != 4 or rng.is_floating_point() or
                            tuple(rng.shape) != (N, 4) or not rng.is_contiguous() or
                            rng.device != device):
        raise TypeError("rng must be a contiguous int32 / uint32 [N, 4] tensor on the image's "
                        "device")


def _check_u8_out(out, like, name="out", whose="the image's"):
    """`out` is a contiguous uint8 tensor of the shape and on the device of `like` -> out"""
    if out is None or out.dtype != torch.uint8 or out.shape != like.shape or \
            not out.is_contiguous() or out.device != like.device:
        raise TypeError(f"{name} must be a contiguous uint8 tensor of {whose} shape")
    return out


def _stage_workspace(workspace, need, device):
    """a stage's workspace: a fresh uint8 tensor of `need` bytes, or the caller's, checked"""
    if workspace is None:
        return torch.empty(need, dtype=torch.uint8, device=device)
    if workspace.dtype != torch.uint8 or not workspace.is_contiguous() or \
            workspace.device != device:
        raise TypeError("workspace must be a contiguous uint8 tensor on the image's device")
    return workspace


def _augment_args(what, image, mask, params, rng, out):
    """The argument checks `augment_u8` and `augment_warp_u8` share -> (image_out, mask_out)."""
    N, H, W = _check_u8_image(what, image)
    if mask is not None and (mask.dtype != torch.uint8 or tuple(mask.shape) != (N, H, W) or
                             not mask.is_contiguous() or mask.device != image.device):
        raise TypeError("mask must be a contiguous uint8 [N,H,W] tensor on the image's device")
    _check_record("params", params, N, lib().unet_augment_params_per_sample(), image.device)
    _check_rng(rng, N, image.device)
    if out is None:
        return torch.empty_like(image), torch.empty_like(mask) if mask is not None else None
    image_out, mask_out = out
    _check_u8_out(image_out, image, "image_out", "its input's")
    if mask is None:
        return image_out, None
    return image_out, _check_u8_out(mask_out, mask, "mask_out", "its input's")


def augment_u8(image, mask, params, rng=None, out=None):
    """(image_out, mask_out): uint8 [N,H,W,3] / [N,H,W] augmented by one launch of
    `unet_augment_u8` on the current stream.  params: fp32 [N, 24] and rng: int32 / uint32
    [N, 4] (or None: all noise off) are DEVICE tensors the kernel reads, so a captured launch
    follows records written into them later.  mask may be None (mask_out is then None).
    out=(image_out, mask_out) names the tensors to write; they must not overlap the inputs."""
    image_out, mask_out = _augment_args("augment_u8", image, mask, params, rng, out)
    N, H, W, _ = image.shape
    check(lib().unet_augment_u8(_ptr(image), _ptr(mask), _ptr(image_out), _ptr(mask_out),
                                _ptr(params), rng.data_ptr() if rng is not None else None,
                                N, H, W, _stream()))
    return image_out, mask_out


def elastic_field(warp, rng, size, out=None):
    """fp32 [N, H, W, 2]: the displacement field (dx, dy in pixels) of the samples whose warp
    record (fp32 [N, 64], DEVICE) says "elastic", by one launch of `unet_elastic_field`; the
    slices of all other samples are NOT written (a fresh tensor starts as zeros).  rng as for
    `augment_u8` (None: the field is 0).  size = (H, W); out names the tensor to write."""
    if not torch.is_tensor(warp) or not warp.is_cuda:
        raise RuntimeError("unet-implementations_amd.elastic_field runs on MI355X only "
                           "(no CPU fallback exists)")
    N, H, W = warp.shape[0], int(size[0]), int(size[1])
    _check_record("warp", warp, N, lib().unet_augment_warp_params_per_sample(), warp.device)
    _check_rng(rng, N, warp.device)
    if out is None:
        out = torch.zeros((N, H, W, 2), dtype=torch.float32, device=warp.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (N, H, W, 2) or \
            not out.is_contiguous() or out.device != warp.device:
        raise TypeError("out must be a contiguous fp32 [N, H, W, 2] tensor on warp's device")
    check(lib().unet_elastic_field(_ptr(out), _ptr(warp),
                                   rng.data_ptr() if rng is not None else None, N, H, W,
                                   _stream()))
    return out


def augment_warp_u8(image, mask, params, rng, warp, field=None, out=None):
    """`augment_u8` behind the per-pixel warp of `unet_augment_warp_u8`: warp is the fp32 [N, 64]
    DEVICE record of elastic / grid / optical distortion, field the fp32 [N, H, W, 2] tensor
    `elastic_field` wrote (None: elastic samples get a zero displacement)."""
    image_out, mask_out = _augment_args("augment_warp_u8", image, mask, params, rng, out)
    N, H, W, _ = image.shape
    _check_record("warp", warp, N, lib().unet_augment_warp_params_per_sample(), image.device)
    if field is not None and (field.dtype != torch.float32 or
                              tuple(field.shape) != (N, H, W, 2) or not field.is_contiguous() or
                              field.device != image.device):
        raise TypeError("field must be a contiguous fp32 [N, H, W, 2] tensor on the image's device")
    check(lib().unet_augment_warp_u8(_ptr(image), _ptr(mask), _ptr(image_out), _ptr(mask_out),
                                     _ptr(params), rng.data_ptr() if rng is not None else None,
                                     _ptr(warp), _ptr(field), N, H, W, _stream()))
    return image_out, mask_out


def augment_post_u8(image, post, rng=None, out=None, workspace=None):
    """uint8 [N,H,W,3]: `image` behind the second augmentation stage of `unet_augment_post_u8`
    (HSV shift, equalize / CLAHE, Gaussian / motion blur, salt / pepper) on the current stream.
    post: fp32 [N, 64] and rng: int32 / uint32 [N, 4] (or None: no salt / pepper) are DEVICE
    tensors the kernels read.  out names the tensor to write (it must not overlap image);
    workspace is a uint8 tensor of at least `unet_augment_post_workspace_bytes(N)` bytes that a
    caller may keep between calls (None: one is allocated)."""
    N, H, W = _check_u8_image("augment_post_u8", image)
    _check_record("post", post, N, lib().unet_augment_post_params_per_sample(), image.device)
    _check_rng(rng, N, image.device)
    out = torch.empty_like(image) if out is None else _check_u8_out(out, image)
    workspace = _stage_workspace(workspace, lib().unet_augment_post_workspace_bytes(N),
                                 image.device)
    check(lib().unet_augment_post_u8(_ptr(image), _ptr(out), _ptr(post),
                                     rng.data_ptr() if rng is not None else None,
                                     _ptr(workspace), workspace.numel(), N, H, W, _stream()))
    return out


def _light_args(name, image, light, rng, out, workspace, need_out):
    """The argument checks of `augment_light_u8` and its two halves -> (out, workspace)."""
    N, _, _ = _check_u8_image(name, image)
    _check_record("light", light, N, lib().unet_augment_light_params_per_sample(), image.device)
    _check_rng(rng, N, image.device)
    if need_out:
        out = torch.empty_like(image) if out is None else _check_u8_out(out, image)
    return out, _stage_workspace(workspace, lib().unet_augment_light_workspace_bytes(N),
                                 image.device)


def augment_light_u8(image, light, rng=None, out=None, workspace=None):
    """uint8 [N,H,W,3]: `image` behind the third augmentation stage of `unet_augment_light_u8`
    (ISO noise, then one of shadow / sun flare / fog) on the current stream.  light: fp32
    [N, 272] and rng: int32 / uint32 [N, 4] (or None: no ISO noise) are DEVICE tensors the kernels
    read.  out names the tensor to write (it must not overlap image); workspace is a uint8 tensor
    of at least `unet_augment_light_workspace_bytes(N)` bytes that a caller may keep between calls
    (None: one is allocated)."""
    out, workspace = _light_args("augment_light_u8", image, light, rng, out, workspace, True)
    N, H, W, _ = image.shape
    check(lib().unet_augment_light_u8(_ptr(image), _ptr(out), _ptr(light),
                                      rng.data_ptr() if rng is not None else None,
                                      _ptr(workspace), workspace.numel(), N, H, W, _stream()))
    return out


def augment_light_stats(image, light, workspace):
    """The statistics half of `augment_light_u8` (the memset of the sums and the statistics
    kernel) into `workspace`, which `augment_light_apply` reads."""
    _, workspace = _light_args("augment_light_stats", image, light, None, None, workspace, False)
    N, H, W, _ = image.shape
    check(lib().unet_augment_light_stats(_ptr(image), _ptr(light), _ptr(workspace),
                                         workspace.numel(), N, H, W, _stream()))
    return workspace


def augment_light_apply(image, light, rng, workspace, out=None):
    """The apply half of `augment_light_u8`, on a workspace `augment_light_stats` filled."""
    out, workspace = _light_args("augment_light_apply", image, light, rng, out, workspace, True)
    N, H, W, _ = image.shape
    check(lib().unet_augment_light_apply(_ptr(image), _ptr(out), _ptr(light),
                                         rng.data_ptr() if rng is not None else None,
                                         _ptr(workspace), workspace.numel(), N, H, W, _stream()))
    return out


def preprocess_u8(image_hwc_u8, mask_u8=None, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """uint8 [N,H,W,3] (+ uint8 [N,H,W]) on the device -> (fp32 NHWC image, int64 target)."""
    N, H, W, C = image_hwc_u8.shape
    if C != 3 or image_hwc_u8.dtype != torch.uint8 or not image_hwc_u8.is_contiguous():
        raise TypeError("preprocess_u8 takes a contiguous uint8 [N,H,W,3] tensor")
    out = _f32((N, H, W, 3), image_hwc_u8)
    tgt = None
    if mask_u8 is not None:
        if mask_u8.dtype != torch.uint8 or tuple(mask_u8.shape) != (N, H, W) or \
                not mask_u8.is_contiguous():
            raise TypeError("mask must be a contiguous uint8 [N,H,W] tensor")
        tgt = torch.empty((N, H, W), dtype=torch.int64, device=image_hwc_u8.device)
    m3 = (ctypes.c_float * 3)(*mean)
    s3 = (ctypes.c_float * 3)(*std)
    check(lib().unet_preprocess_u8(_ptr(image_hwc_u8), _ptr(mask_u8), _ptr(out), _ptr(tgt), N, H,
                                   W, m3, s3, _stream()))
    return out, tgt


# ---- optimizer -------------------------------------------------------------------------
def sgd_nesterov_step(params, grads, momentum, lr, mu, weight_decay, first_step, grad_scale=1.0):
    n = params.numel()
    t0 = _begin()
    check(lib().unet_sgd_nesterov_step(_ptr(params), _ptr(grads), _ptr(momentum), n, lr, mu,
                                       weight_decay, 1 if first_step else 0, grad_scale,
                                       _stream()))
    if t0 is not None:   # p, g, buf in; p, buf out
        _timer.end("sgd_nesterov", 0.0, 1, t0, nbytes=4.0 * (5 if not first_step else 4) * n)


def sgd_nesterov_step_dev(params, grads, momentum, hyper, first_step):
    """As sgd_nesterov_step with {lr, mu, weight_decay, grad_scale} read from the device tensor
    `hyper` (fp32 [4]): what a graph-captured train step launches."""
    n = params.numel()
    check(lib().unet_sgd_nesterov_step_dev(_ptr(params), _ptr(grads), _ptr(momentum), n,
                                           _ptr(hyper), 1 if first_step else 0, _stream()))


# ---- autoencoder pretraining step (recon.hip) ------------------------------------------------
def recon3x3_fwd(x, slope, w, b):
    """sigmoid(conv3x3(act(x)) + b) of the autoencoder's reconstruction head: NCHW fp32 [N,3,H,W].
    x: the last decoder layer's output (ops.Act or a plain NHWC tensor, fp32 or bf16)."""
    x, rx = _act(x)
    N, H, W, C = x.shape
    K = w.shape[0]
    out = _f32((N, K, H, W), x.x)
    t0 = _begin()
    check(lib().unet_recon3x3_fwd(rx, 1 if _is_b16(x.x) else 0, slope, _ptr(w), _ptr(b),
                                  _ptr(out), N, H, W, K, _stream()))
    if t0 is not None:
        _timer.end("recon_fwd", 2.0 * N * H * W * K * C * 9, 1, t0,
                   nbytes=x.x.element_size() * x.x.numel() + 4.0 * out.numel())
    return out


_recon_ws = {}


def recon3x3_bwd(x, slope, dout, out, w, dw, db, nxt=None):
    """dL/d act(x) (NHWC, x's storage type) of the reconstruction head; dw / db are written.
    nxt (NextNorm of the layer whose raw output x.x is): also leave the reductions of that layer's
    InstanceNorm backward (nxt.tiles == 0: not emitted for this call)."""
    x, rx = _act(x)
    N, H, W, C = x.shape
    K = w.shape[0]
    da = torch.empty_like(x.x)
    key = (N, H, W, x.x.device)
    ws = _recon_ws.get(key)
    if ws is None:
        ws = _recon_ws[key] = _ws(lib().unet_recon3x3_bwd_workspace_bytes(N, H, W), x.x)
    t0 = _begin()
    _call_nxt(lib().unet_recon3x3_bwd,
              (rx, 1 if _is_b16(x.x) else 0, slope, _ptr(dout), _ptr(out), _ptr(w), _ptr(da),
               _ptr(dw), _ptr(db), _ptr(ws), ws.numel(), N, H, W, K), nxt)
    if t0 is not None:   # x in, da out, dout + out in
        _timer.end("recon_bwd", 4.0 * N * H * W * K * C * 9, 2, t0,
                   nbytes=da.element_size() * 2.0 * da.numel() + 8.0 * dout.numel())
    return da


def _mse_target(out, target, target_u8):
    N, C, H, W = out.shape
    if target_u8:
        if target.dtype != torch.uint8 or tuple(target.shape) != (N, H, W, C):
            raise TypeError("a uint8 target is the [N,H,W,3] image of the output's size")
    elif target.dtype != torch.float32 or target.shape != out.shape:
        raise TypeError("the target must be an fp32 tensor of the output's shape")
    return target.contiguous()


def mse_loss_fwd(out, target, target_u8=False):
    """(loss fp32 [1], per-image sums of squares fp64 [N]) of nn.MSELoss() on the device."""
    N, C, H, W = out.shape
    target = _mse_target(out, target, target_u8)
    loss = _f32((1,), out)
    per_image = torch.empty((N,), dtype=torch.float64, device=out.device)
    ws = _ws(lib().unet_mse_loss_workspace_bytes(N, C, H, W), out)
    t0 = _begin()
    check(lib().unet_mse_loss_fwd(_ptr(out), _ptr(target), 1 if target_u8 else 0, _ptr(loss),
                                  per_image.data_ptr(), _ptr(ws), ws.numel(), N, C, H, W,
                                  _stream()))
    if t0 is not None:
        _timer.end("mse_loss", 0.0, 2, t0, nbytes=4.0 * out.numel() + target.element_size() *
                   target.numel())
    return loss, per_image


def mse_loss_grad(out, target, upstream=None, target_u8=False):
    """dL/dout = upstream * 2 (out - t) / numel; upstream: a device scalar (autograd's) or None."""
    N, C, H, W = out.shape
    target = _mse_target(out, target, target_u8)
    dout = torch.empty_like(out)
    if upstream is not None:
        upstream = upstream.reshape(1).float().contiguous()
    t0 = _begin()
    check(lib().unet_mse_loss_grad(_ptr(out), _ptr(target), 1 if target_u8 else 0, _ptr(upstream),
                                   _ptr(dout), N, C, H, W, _stream()))
    if t0 is not None:
        _timer.end("mse_grad", 0.0, 1, t0, nbytes=8.0 * out.numel() + target.element_size() *
                   target.numel())
    return dout


def adam_step(params, grads, exp_avg, exp_avg_sq, hyper, advance_step):
    """torch.optim.Adam's update over flat fp32 tensors; hyper: the fp64 [8] device tensor
    {lr, beta1, beta2, eps, weight_decay, grad_scale, step, -} (advance_step: step += 1 first)."""
    n = params.numel()
    if hyper.dtype != torch.float64 or not hyper.is_cuda or hyper.numel() < 8:
        raise TypeError("hyper must be an fp64 [8] device tensor")
    t0 = _begin()
    check(lib().unet_adam_step(_ptr(params), _ptr(grads), _ptr(exp_avg), _ptr(exp_avg_sq), n,
                               hyper.data_ptr(), 1 if advance_step else 0, _stream()))
    if t0 is not None:   # p, g, m, v in; p, m, v out
        _timer.end("adam", 0.0, 2 if advance_step else 1, t0, nbytes=4.0 * 7 * n)


# ---- SSIM (unet_ssim_*) -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gaussian_window(size=11, sigma=1.5):
    """The 1-D window of the reference's gaussian_kernel (utils/metrics.py:44-73): fp32 exp of the
    centred coordinates, normalised by its sum (the 2-D window is its outer product)."""
    coords = torch.arange(size).float() - (size - 1) / 2
    g = torch.exp(-(coords ** 2) / (2 * sigma ** 2))
    return tuple((g / g.sum()).tolist())


def _gauss11(window):
    w = [float(v) for v in window]
    if len(w) != 11:
        raise ValueError("the SSIM kernels take an 11-tap window")
    return (ctypes.c_float * 11)(*w)


def ssim_fwd(pred, target, target_u8=False, window=None, c1=1e-4, c2=9e-4, w_ssim=1.0,
             w_mse=0.0, want_loss=True):
    """(loss fp32 [1] or None, per-image mean SSIM fp64 [N], per-image sums of squares fp64 [N])
    from one read of both images; loss = w_ssim * (1 - mean SSIM) + w_mse * mean sq."""
    N, C, H, W = pred.shape
    target = _mse_target(pred, target, target_u8)
    g = _gauss11(window if window is not None else gaussian_window())
    loss = _f32((1,), pred) if want_loss else None
    ssim = torch.empty((N,), dtype=torch.float64, device=pred.device)
    sq = torch.empty((N,), dtype=torch.float64, device=pred.device)
    ws = _ws(lib().unet_ssim_workspace_bytes(N, C, H, W), pred)
    t0 = _begin()
    check(lib().unet_ssim_fwd(_ptr(pred), _ptr(target), 1 if target_u8 else 0, g, c1, c2,
                              ssim.data_ptr(), sq.data_ptr(), _ptr(loss), w_ssim, w_mse, _ptr(ws),
                              ws.numel(), N, C, H, W, _stream()))
    if t0 is not None:
        _timer.end("ssim_fwd", 0.0, 2, t0, nbytes=4.0 * pred.numel() + target.element_size() *
                   target.numel())
    return loss, ssim, sq


def ssim_grad(pred, target, upstream=None, upstream_per_image=False, target_u8=False, window=None,
              c1=1e-4, c2=9e-4, w_ssim=1.0, w_mse=0.0):
    """dL/dpred of L = up * [w_ssim * (1 - mean SSIM) + w_mse * mean (pred - t)^2]; upstream: a
    device scalar (means over the batch) or, with upstream_per_image, a device [N] (means per
    image), or None (= 1)."""
    N, C, H, W = pred.shape
    target = _mse_target(pred, target, target_u8)
    g = _gauss11(window if window is not None else gaussian_window())
    dpred = torch.empty_like(pred)
    if upstream is not None:
        upstream = upstream.reshape(-1).float().contiguous()
        if upstream.numel() != (N if upstream_per_image else 1):
            raise ValueError("upstream must hold one value (or one per image)")
    elif upstream_per_image:
        raise ValueError("a per-image upstream needs upstream")
    t0 = _begin()
    check(lib().unet_ssim_grad(_ptr(pred), _ptr(target), 1 if target_u8 else 0, g, c1, c2,
                               _ptr(upstream), 1 if upstream_per_image else 0, w_ssim, w_mse,
                               _ptr(dpred), N, C, H, W, _stream()))
    if t0 is not None:
        _timer.end("ssim_grad", 0.0, 1, t0, nbytes=8.0 * pred.numel() + target.element_size() *
                   target.numel())
    return dpred


# ---- perceptual (VGG16 feature) loss (perceptual.hip) -------------------------------------------
def conv_fwd_raw(s0, slope, w, bias, wu=None):
    """y = conv3x3(act(s0)) + bias (stride 1) on the fused layer's kernels WITHOUT the statistics
    finalize: the launch of `conv_in_fwd`, its per-tile summaries ignored (a layer with no
    InstanceNorm behind it: the perceptual loss's trunk).  wu: the Winograd forward form - the
    caller checked `conv_wino_supported` and s0 carries alpha / beta."""
    s0, r0 = _act(s0)
    N, H, W, C0 = s0.shape
    Cout = w.shape[1]
    assert w.shape[0] == 9 and w.shape[2] == C0
    wino = wu is not None
    fn, form, tag = _sel_conv_in_fwd(False, False, wino, False, 3, C0)
    head = (r0, None, slope, _ptr(wu), _ptr(bias)) if wino else \
        (r0, None, slope, _ptr(w), _ptr(bias), 3, 1)
    y, _, _, _, t0 = _conv_stats_launch(fn, head, False, s0.x, N, H, W, Cout, 1)
    if t0 is not None:
        if not wino and C0 != 3:
            wino = _c32_winograd(N, H, W, C0, Cout, 1)
        _end_conv(t0, tag, 2.0 * N * H * W * 9 * C0 * Cout, 1, wino)
    return y


def _mean_std3(mean, std):
    return (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)


def perceptual_prep(out, target, target_u8=False, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """The stacked, normalised NHWC tensor [2N,H,W,3] of PerceptualLoss: (x - mean) / std of the
    output (images 0..N-1) and of the target (N..2N-1; NCHW fp32 or the uint8 NHWC image)."""
    N, C, H, W = out.shape
    if C != 3:
        raise ValueError("the perceptual loss takes RGB images")
    target = _mse_target(out, target, target_u8)
    xn = _f32((2 * N, H, W, 3), out)
    m, s = _mean_std3(mean, std)
    t0 = _begin()
    check(lib().unet_perceptual_prep(_ptr(out), _ptr(target), 1 if target_u8 else 0, m, s,
                                     _ptr(xn), N, H, W, _stream()))
    if t0 is not None:
        _timer.end("perceptual_prep", 0.0, 1, t0, nbytes=4.0 * out.numel() + 4.0 * xn.numel() +
                   target.element_size() * target.numel())
    return xn


def relu_maxpool2x2_fwd(y):
    """max_pool2d(relu(y), 2) of a raw NHWC tensor (floor semantics) as a plain tensor."""
    M, H, W, C = y.shape
    p = _f32((M, H // 2, W // 2, C), y)
    t0 = _begin()
    check(lib().unet_relu_maxpool2x2_fwd(_ptr(y), _ptr(p), M, H, W, C, _stream()))
    if t0 is not None:
        _timer.end("relu_maxpool", 0.0, 1, t0, nbytes=4.0 * (4 * p.numel() + p.numel()))
    return p


def feature_mse_fwd(y, sums):
    """sums[n] (fp64 [N]) = sum (relu(y[n]) - relu(y[n + N]))^2 over the raw stacked [2N,H,W,C]."""
    M, H, W, C = y.shape
    N = M // 2
    if M != 2 * N or sums.dtype != torch.float64 or sums.numel() != N or not sums.is_contiguous():
        raise ValueError("feature_mse_fwd takes a stacked [2N,H,W,C] tensor and fp64 sums [N]")
    ws = _ws(lib().unet_feature_mse_workspace_bytes(N, H, W, C), y)
    t0 = _begin()
    check(lib().unet_feature_mse_fwd(_ptr(y), sums.data_ptr(), _ptr(ws), ws.numel(), N, H, W, C,
                                     _stream()))
    if t0 is not None:
        _timer.end("feature_mse", 0.0, 2, t0, nbytes=4.0 * y.numel())
    return sums


def perceptual_relu_bwd(y_o, y_t=None, coef=0.0, g=None, gp=None):
    """dz = y_o > 0 ? g_in + coef * (relu(y_o) - relu(y_t)) : 0 of one trunk layer; g_in = g (same
    resolution), gp (the following pool's output gradient, routed to the first maximum) or none."""
    N, H, W, C = y_o.shape
    for t, shape in ((y_t, y_o.shape), (g, y_o.shape), (gp, (N, H // 2, W // 2, C))):
        if t is not None and tuple(t.shape) != tuple(shape):
            raise ValueError("perceptual_relu_bwd: operand shape mismatch")
    dz = torch.empty_like(y_o)
    t0 = _begin()
    check(lib().unet_perceptual_relu_bwd(_ptr(y_o), _ptr(y_t), coef, _ptr(g), _ptr(gp), _ptr(dz),
                                         N, H, W, C, _stream()))
    if t0 is not None:
        nb = 2 + (y_t is not None) + (g is not None) + 0.25 * (gp is not None)
        _timer.end("perceptual_relu_bwd", 0.0, 1, t0, nbytes=4.0 * nb * y_o.numel())
    return dz


def perceptual_stem_bwd_data(dz, w_oihw, std=IMAGENET_STD, out=None):
    """dL/doutput (NCHW fp32 [N,3,H,W]) from dz of conv1_1: its data gradient divided by std."""
    N, H, W, Cout = dz.shape
    assert tuple(w_oihw.shape) == (Cout, 3, 3, 3)
    dout = out if out is not None else _f32((N, 3, H, W), dz)
    assert tuple(dout.shape) == (N, 3, H, W) and dout.dtype == torch.float32
    _, s = _mean_std3(std, std)
    t0 = _begin()
    check(lib().unet_perceptual_stem_bwd_data(_ptr(dz), _ptr(w_oihw), s, _ptr(dout), N, H, W, Cout,
                                              _stream()))
    if t0 is not None:
        _timer.end("perceptual_stem_bwd_data", 2.0 * N * H * W * 27 * Cout, 1, t0,
                   nbytes=4.0 * (dz.numel() + dout.numel()))
    return dout


# ---- CLIP ViT image tower (vit.hip) ------------------------------------------------------------
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
VIT_PLAIN, VIT_BIAS, VIT_BIAS_GELU, VIT_BIAS_RESIDUAL = 0, 1, 2, 3


def vit_k_padded(patch_size, step=16):
    """Columns of the patch matrix: 3 P^2 rounded up to the GEMM's K step."""
    k = 3 * patch_size * patch_size
    return (k + step - 1) // step * step


def vit_patchify(images, resolution, patch_size, input_layout="nchw", mean=CLIP_MEAN,
                 std=CLIP_STD):
    """bf16 patch matrix [N G^2, Kp] of fp32 NCHW images (taken as they are) or uint8 NHWC images
    ("nhwc_u8": (v / 255 - mean) / std folded in), resized to resolution^2 while gathering."""
    u8 = input_layout == "nhwc_u8"
    if u8:
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3:
            raise ValueError('input_layout="nhwc_u8" takes a uint8 [N,H,W,3] batch')
        N, H, W, _ = images.shape
    elif input_layout == "nchw":
        if images.dtype != torch.float32 or images.dim() != 4 or images.shape[1] != 3:
            raise ValueError('input_layout="nchw" takes an fp32 [N,3,H,W] batch')
        N, _, H, W = images.shape
    else:
        raise ValueError(f"unknown input_layout {input_layout!r}")
    G = resolution // patch_size
    Kp = vit_k_padded(patch_size)
    a = _b16((N * G * G, Kp), images)
    m, s = _mean_std3(mean, std)
    t0 = _begin()
    check(lib().unet_vit_patchify(_ptr(images), 1 if u8 else 0, m, s, _ptr(a), N, H, W, resolution,
                                  patch_size, Kp, _stream()))
    if t0 is not None:
        _timer.end("vit_patchify", 0.0, 1, t0, nbytes=2.0 * a.numel())
    return a


def vit_gemm(a, w, bias=None, epilogue=VIT_PLAIN, out=None):
    """a [M,K] @ w [Nout,K]^T (bf16 operands, fp32 accumulation) with the epilogue of
    unet_vit_gemm_bf16; VIT_BIAS_RESIDUAL adds into `out` (the fp32 stream) in place."""
    M, K = a.shape
    Nout = w.shape[0]
    if a.dtype != torch.bfloat16 or w.dtype != torch.bfloat16 or w.shape[1] != K:
        raise ValueError("vit_gemm takes bf16 a [M,K] and w [Nout,K]")
    if epilogue == VIT_BIAS_RESIDUAL:
        if out is None or out.dtype != torch.float32 or out.shape[0] < M or out.shape[1] != Nout:
            raise ValueError("the residual epilogue adds into an fp32 out [>= M, Nout]")
    elif out is None:
        out = _f32((M, Nout), a) if epilogue == VIT_PLAIN else _b16((M, Nout), a)
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != Nout):
        raise ValueError("vit_gemm: bias must be fp32 [Nout]")
    t0 = _begin()
    check(lib().unet_vit_gemm_bf16(_ptr(a), _ptr(w), _ptr(bias), _ptr(out), epilogue, M, Nout, K,
                                   _stream()))
    if t0 is not None:
        _timer.end("vit_gemm", 2.0 * M * Nout * K, 1, t0)
    return out


def vit_tokens_ln(patches, cls, pos, gamma, beta, N, eps=1e-5):
    """The fp32 stream [N T, D]: ln_pre of [cls + pos[0]; patches + pos[1:]]."""
    T, D = pos.shape
    out = _f32((N * T, D), patches)
    t0 = _begin()
    check(lib().unet_vit_tokens_ln(_ptr(patches), _ptr(cls), _ptr(pos), _ptr(gamma), _ptr(beta),
                                   eps, _ptr(out), N, T, D, _stream()))
    if t0 is not None:
        _timer.end("vit_ln", 0.0, 1, t0, nbytes=8.0 * out.numel())
    return out


def vit_layernorm(x, gamma, beta, eps=1e-5, rows=None):
    """bf16 LayerNorm of the first `rows` rows of the fp32 x [R, D]."""
    R, D = x.shape
    rows = R if rows is None else rows
    if x.dtype != torch.float32 or rows > R:
        raise ValueError("vit_layernorm takes an fp32 [rows, D] tensor")
    out = _b16((rows, D), x)
    t0 = _begin()
    check(lib().unet_vit_layernorm(_ptr(x), _ptr(gamma), _ptr(beta), eps, _ptr(out), rows, D,
                                   _stream()))
    if t0 is not None:
        _timer.end("vit_ln", 0.0, 1, t0, nbytes=6.0 * out.numel())
    return out


def vit_attention(qkv, N, T, heads):
    """softmax(q k^T / 8) v of the packed bf16 projection [N T, 3 D], every head in one launch."""
    D = qkv.shape[1] // 3
    if qkv.dtype != torch.bfloat16 or qkv.shape[0] != N * T or qkv.shape[1] != 3 * D:
        raise ValueError("vit_attention takes the bf16 [N T, 3 D] projection")
    out = _b16((N * T, D), qkv)
    t0 = _begin()
    check(lib().unet_vit_attention(_ptr(qkv), _ptr(out), N, T, D, heads, _stream()))
    if t0 is not None:
        _timer.end("vit_attention", 4.0 * N * heads * T * T * 64, 1, t0)
    return out


def vit_head(x, gamma, beta, proj, N, T, grid, eps=1e-5):
    """ln_post(class rows) @ proj broadcast to fp32 NCHW [N, E, grid, grid]."""
    D, E = proj.shape
    out = _f32((N, E, grid, grid), x)
    t0 = _begin()
    check(lib().unet_vit_head(_ptr(x), _ptr(gamma), _ptr(beta), eps, _ptr(proj), _ptr(out), N, T,
                              D, E, grid, _stream()))
    if t0 is not None:
        _timer.end("vit_head", 2.0 * N * D * E, 1, t0, nbytes=4.0 * out.numel())
    return out
