"""Deferred weight-gradient reductions (-m gpu): `ops.wgrad_deferral` / `unet_wgrad_defer_*`.

Every `*_bwd_weight*` entry point leaves one partial gradient per workgroup (a slab) and sums the
slabs in a fixed order: chunks of 16 while more than 16 remain (1 or 2 SLAB stages), then a final
sum + scatter whose kind depends on the layer (TAP, WIDE8, WIDE16, GENERIC, CENTER, STEM).  Inside
a deferral scope the entry points only queue those jobs, and a flush runs the queued jobs of every
layer stage by stage through one batched kernel that finds its job in a table of <= 56 entries.
That is claimed to be bit-identical to the per-call form.  Here every entry point and reduction
kind runs both ways on the same inputs (`torch.equal`), the per-call result is held to an fp64
CPU reference, and the number of queued stages (`unet_wgrad_defer_pending` after one call) is
asserted, so each case provably reaches the 1, 2 or 3 stages it was chosen for.  Then the batched
table itself: mixed kinds and stage counts in one flush, more than 56 jobs in a stage, a flush in
the middle of a scope, the workspaces held until the flush, disjoint column slices of one
gradient, nested scopes, a refused call, and the whole network with and without deferral."""
import re
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as F

from oracle import unet_ref as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
SLOPE = 0.01
BF = torch.bfloat16
SENTINEL = 7.0


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def coeffs(n, c, seed):
    """Folded InstanceNorm / dropout coefficients: mostly alpha > 0, some channels dropped."""
    al = rnd(n, c, seed=seed) * 0.5 + 1.0
    be = rnd(n, c, seed=seed + 1) * 0.7
    drop = torch.rand(n, c, generator=torch.Generator().manual_seed(seed + 2)) < 0.15
    return torch.where(drop, torch.zeros_like(al), al), torch.where(drop, torch.zeros_like(be), be)


def r16(t):
    return t.to(BF).float()


def act_ref(x, al, be, b16=False):
    """lrelu(x * alpha + beta) per (n, c) of an NCHW tensor: in fp64, or in fp32 and then rounded
    to bf16 as the bf16-storage loaders stage it."""
    if b16:
        z = x.float() * al[:, :, None, None] + be[:, :, None, None]
        return r16(F.leaky_relu(z, SLOPE)).double()
    z = x.double() * al.double()[:, :, None, None] + be.double()[:, :, None, None]
    return F.leaky_relu(z, SLOPE)


def to_nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().to(DEV)


def to_nhwc_b16(t):
    return t.permute(0, 2, 3, 1).contiguous().to(DEV).to(BF)


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def pending(ua):
    return ua._lib.lib().unet_wgrad_defer_pending()


# entry: conv3x3 (ops.conv3x3_bwd_weight, plain operand), in (ops.conv_in_bwd_weight, activated on
# load), 1x1 (ops.conv1x1_bwd_weight), stem (Cx = 3 through conv_in_bwd_weight), u8 (the stem from
# a U8Image), up (ops.conv3x3_up_bwd_weight; H, W = the low-resolution size).
# mode: fp32, bf16 (bf16 matrix cores on fp32 tensors whose values are bf16 numbers, conv3x3
# only), x3 (split bf16 on fp32 tensors), b16 (bf16 tensors).  dw has off + Cx + extra
# input channels, the layer writes [off, off + Cx).  stages / kind: what the plan of the shape
# queues (emit_wgrad_reduction in csrc/conv_wgrad.hip).  chunk: images per launch, forced with
# the debug chunk limit (0: the whole batch).  kernel: the compute launches of the call, in
# order, as short_name() writes them: the instantiation wgrad_select / launch_wgrad_plan of
# csrc/conv_wgrad.hip pick for the shape (one name per launch, so one per chunk).
Spec = namedtuple("Spec", "entry mode N H W Cx Cout stride ks off extra stages kind c32 chunk "
                          "kernel", defaults=(1, 3, 0, 0, 1, "TAP", None, 0, None))


def wg(targs, nw=4):
    """conv_wgrad_kernel<CI_T, CO_T, S, STRIDE, ACT, TX, TD, NW> on fp32 tensors"""
    return (f"conv_wgrad_kernel<{targs}, float, float, {nw}>",)


def wg_bf16(targs, act="true"):
    """conv_wgrad_bf16_kernel<CI_T, CO_T, S, NPL, SB, TX, TD, ACT, STRIDE> on fp32 tensors"""
    return (f"conv_wgrad_bf16_kernel<{targs}, float, float, {act}, 1>",)


def wg_b16(S, stride):
    """conv_wgrad_bf16_kernel<64, 64, S, 1, false, __bf16, __bf16, true, stride> (mangled: the
    demangler gives up on __bf16 template arguments)"""
    return (f"_ZN12_GLOBAL__N_122conv_wgrad_bf16_kernelILi64ELi64ELi{S}ELi1ELb0EDF16bDF16bLb1ELi"
            f"{stride}EEEvNS_11WgradParamsE",)


def ring(targs):
    """conv_wgrad_b16_ring_kernel<CI_T, CO_T, S, ACT, DEPTH, RG, STRIDE>"""
    return (f"conv_wgrad_b16_ring_kernel<{targs}>",)


def taps(targs, nw=4):
    """conv_wgrad_taps_kernel<CI_T, CO_T, S, ACT, TX, TD, NW> on fp32 tensors"""
    return (f"conv_wgrad_taps_kernel<{targs}, true, float, float, {nw}>",)


def taps_b16(targs):
    return (f"conv_wgrad_taps_b16_kernel<{targs}, true>",)


CASES = {
    # conv3x3_bwd_weight, fp32
    "conv3x3-4wave": Spec("conv3x3", "fp32", 2, 24, 40, 32, 32, stages=2,           # 24 slabs
                          kernel=wg("32, 32, 32, 1, false")),
    "conv3x3-8wave": Spec("conv3x3", "fp32", 2, 16, 24, 128, 128,                    # wide, 8 slabs
                          kernel=wg("64, 64, 32, 1, false", nw=8)),
    "conv3x3-winograd": Spec("conv3x3", "fp32", 2, 64, 64, 64, 64, stages=2,        # 32 slabs
                             kernel=("conv_wgrad_wino_kernel<false>",)),
    "conv3x3-wino32": Spec("conv3x3", "fp32", 2, 64, 64, 32, 32, stages=2, c32="always",
                           kernel=("conv_wgrad_wino32_kernel<false>",)),
    "conv3x3-stride2": Spec("conv3x3", "fp32", 2, 64, 64, 32, 64, stride=2,          # 16 slabs
                            kernel=wg("32, 64, 32, 2, false")),
    "conv3x3-slice": Spec("conv3x3", "fp32", 2, 32, 48, 64, 32, off=32, extra=32, stages=2,
                          kernel=wg("32, 32, 32, 1, false")),
    # conv_in_bwd_weight (activation on load)
    "in-fp32": Spec("in", "fp32", 2, 24, 40, 32, 64, off=32, stages=2,               # 24 slabs
                    kernel=wg("32, 64, 32, 1, true")),
    "in-bf16x3": Spec("in", "x3", 2, 24, 40, 32, 64, off=32, stages=2,               # 24 slabs
                      kernel=wg_bf16("32, 64, 32, 3, false")),
    "in-bf16x3-3stages": Spec("in", "x3", 2, 256, 256, 32, 32, stages=3,             # 512 slabs
                              kernel=wg_bf16("32, 32, 64, 3, true")),
    "in-b16-ring": Spec("in", "b16", 2, 64, 64, 64, 64, off=32, stages=2,            # 64 slabs
                        kernel=ring("64, 64, 32, true, 2, 2, 1")),
    "in-b16-stride2": Spec("in", "b16", 2, 64, 64, 64, 128, stride=2, stages=2,      # 32 slabs
                           kernel=ring("64, 64, 16, true, 2, 2, 2")),
    "generic": Spec("in", "fp32", 2, 16, 16, 256, 96, kind="GENERIC",                # 8 slabs
                    kernel=wg("32, 32, 16, 1, true", nw=8)),
    "generic-bf16x3": Spec("in", "x3", 2, 48, 32, 256, 96, stages=2, kind="GENERIC",  # 20 slabs
                           kernel=wg("32, 32, 32, 1, true")),
    "wide8": Spec("in", "fp32", 2, 8, 16, 256, 128, kind="WIDE8",                    # 4 slabs
                  kernel=wg("64, 64, 16, 1, true", nw=8)),
    "wide16": Spec("in", "fp32", 1, 8, 8, 512, 512, kind="WIDE16",                   # 2 slabs
                   kernel=wg("64, 64, 16, 1, true", nw=8)),
    "center-ksize1": Spec("in", "fp32", 2, 4, 4, 256, 64, ks=1, off=64, kind="CENTER",  # 2 slabs
                          kernel=wg("64, 64, 16, 1, true", nw=8)),
    "conv1x1": Spec("1x1", "fp32", 2, 16, 16, 64, 64, ks=1, off=64, extra=32, kind="CENTER",
                    kernel=wg("64, 64, 16, 1, false")),
    # the RGB stem: 1 x 256 x 256 = 512 blocks, 1 x 256 x 192 = 384: three stages
    "stem-rows": Spec("stem", "fp32", 1, 256, 256, 3, 32, stages=3, kind="STEM",     # W % 128 == 0
                      kernel=("conv_stem_wgrad_rows_kernel<float, float>",)),
    "stem-generic": Spec("stem", "fp32", 1, 256, 192, 3, 32, stages=3, kind="STEM",
                         kernel=("conv_stem_wgrad_kernel<float>",)),
    "stem-u8": Spec("u8", "fp32", 1, 256, 256, 3, 32, stages=3, kind="STEM",
                    kernel=("conv_stem_wgrad_rows_kernel<unsigned char, float>",)),
    # conv3x3(upsample2x(.)) at low resolution
    "up-fp32": Spec("up", "fp32", 2, 8, 16, 64, 64, extra=32,                        # 4 slabs
                    kernel=taps("64, 64, 16")),
    "up-fp32-8wave": Spec("up", "fp32", 2, 16, 16, 128, 128,                         # wide, 4 slabs
                          kernel=taps("64, 64, 32", nw=8)),
    "up-b16": Spec("up", "b16", 2, 32, 32, 64, 64, off=32, stages=2,                 # 32 slabs
                   kernel=taps_b16("64, 64, 16")),
    # bf16 tensors with an odd number of output rows: no whole ring rounds, so the segment
    # kernels of the bf16 matrix cores
    "in-b16-segments": Spec("in", "b16", 2, 25, 40, 64, 64, stages=2,                # 25 slabs
                            kernel=wg_b16(32, 1)),
    "in-b16-stride2-segments": Spec("in", "b16", 2, 50, 40, 64, 128, stride=2, stages=2,
                                    kernel=wg_b16(16, 2)),
    # unet_conv3x3_bwd_weight_bf16 (fp32 tensors), bf16x3 on the 64x64 and the single-buffered
    # 32x32 tile, the bf16 tap kernel on the 32x32 tile
    "conv3x3-bf16": Spec("conv3x3", "bf16", 2, 16, 24, 32, 64,                       # 8 slabs
                         kernel=wg_bf16("32, 64, 32, 1, false", act="false")),
    "in-bf16x3-64x64": Spec("in", "x3", 2, 16, 24, 64, 64,                           # 16 slabs
                            kernel=wg_bf16("64, 64, 16, 3, false")),
    "in-bf16x3-32x32": Spec("in", "x3", 2, 16, 64, 32, 32,                           # 8 slabs
                            kernel=wg_bf16("32, 32, 64, 3, true")),
    "up-b16-32x32": Spec("up", "b16", 2, 16, 16, 32, 32,                             # 2 slabs
                         kernel=taps_b16("32, 32, 64")),
    # batches split by the chunk limit: 2 + 1 images, a launch each
    "conv3x3-chunked": Spec("conv3x3", "fp32", 3, 24, 40, 32, 32, stages=2, chunk=2,  # 24 + 12
                            kernel=wg("32, 32, 32, 1, false") * 2),
    "up-chunked": Spec("up", "fp32", 3, 8, 16, 64, 64, chunk=2,                      # 4 + 2 slabs
                       kernel=taps("64, 64, 16") * 2),
}


class Layer:
    """One weight-gradient call on seeded inputs (already on the device): `layer(dw)` launches it,
    `new_dw()` is a sentinel-filled gradient, `ref()` the fp64 CPU gradient of its slice."""

    def __init__(self, ua, spec, seed=1):
        self.ua, self.s = ua, spec
        s = spec
        self.total = s.off + s.Cx + s.extra
        self.Ho, self.Wo = (s.H - 1) // s.stride + 1, (s.W - 1) // s.stride + 1
        b16 = s.mode == "b16"
        rounded = b16 or s.mode == "bf16"      # operand values are bf16 numbers
        if s.entry == "u8":
            self.u8 = torch.randint(0, 256, (s.N, s.H, s.W, 3), dtype=torch.uint8,
                                    generator=torch.Generator().manual_seed(seed))
            self.src = ua.ops.U8Image(self.u8.to(DEV))
        else:
            self.x = rnd(s.N, s.Cx, s.H, s.W, seed=seed)
            if rounded:
                self.x = r16(self.x)
            self.coef = coeffs(s.N, s.Cx, seed + 10) if s.entry in ("in", "up") else None
            xd = to_nhwc_b16(self.x) if b16 else to_nhwc(self.x)
            if self.coef is None:
                self.src = xd
            else:
                self.src = ua.ops.Act(xd, self.coef[0].to(DEV).contiguous(),
                                      self.coef[1].to(DEV).contiguous())
        if s.entry == "up":
            self.dy = rnd(s.N, s.Cout, 2 * s.H, 2 * s.W, seed=seed + 1)
            if b16:
                self.dy = r16(self.dy)
            self.dyd = ua.ops.upsample2x_bwd_taps(to_nhwc_b16(self.dy) if b16 else to_nhwc(self.dy))
        else:
            self.dy = rnd(s.N, s.Cout, self.Ho, self.Wo, seed=seed + 1)
            if rounded:
                self.dy = r16(self.dy)
            self.dyd = to_nhwc_b16(self.dy) if b16 else to_nhwc(self.dy)

    def new_dw(self):
        s = self.s
        shape = (s.Cout, self.total) if s.entry == "1x1" else (s.Cout, self.total, s.ks, s.ks)
        return torch.full(shape, SENTINEL, device=DEV)

    def workspace_bytes(self):
        s, lib = self.s, self.ua._lib.lib()
        if s.entry == "up":
            return lib.unet_conv3x3_up_bwd_weight_workspace_bytes(s.N, s.H, s.W, s.Cx, s.Cout)
        return lib.unet_conv3x3_bwd_weight_workspace_bytes(s.N, s.H, s.W, s.Cx, s.Cout, s.stride)

    def chunk_limit_bytes(self):
        """The debug chunk limit under which the call takes s.chunk images a launch; a tensor's
        image is counted at four bytes an element."""
        s = self.s
        dy_image = s.H * s.W * 9 * s.Cout if s.entry == "up" else self.Ho * self.Wo * s.Cout
        return int((s.chunk + 0.5) * 4 * max(s.H * s.W * s.Cx, dy_image))

    def __call__(self, dw):
        if not self.s.chunk:
            return self._call(dw)
        lib = self.ua._lib.lib()
        lib.unet_debug_set_chunk_limit(self.chunk_limit_bytes())
        try:
            return self._call(dw)
        finally:
            lib.unet_debug_set_chunk_limit(0)      # (0: back to the default)

    def _call(self, dw):
        s, ops = self.s, self.ua.ops
        with ops.c32_winograd_scope(s.c32 if s.c32 is not None else True):
            if s.entry == "conv3x3":
                ops.conv3x3_bwd_weight(self.src, self.dyd, dw, s.off, s.stride,
                                       bf16=s.mode == "bf16")
            elif s.entry == "1x1":
                ops.conv1x1_bwd_weight(self.src, self.dyd, dw, s.off)
            elif s.entry == "up":
                ops.conv3x3_up_bwd_weight(self.src, SLOPE, self.dyd, dw, s.off)
            else:   # in, stem, u8
                src = self.src if s.entry != "stem" else ops.Act(self.src)
                ops.conv_in_bwd_weight(src, SLOPE, self.dyd, dw, s.off, s.ks, s.stride,
                                       x3=s.mode == "x3")
        return dw

    def cols(self, dw):
        return dw[:, self.s.off:self.s.off + self.s.Cx]

    def ref(self):
        s = self.s
        if s.entry == "u8":
            m = torch.tensor(self.src.mean, dtype=torch.float64)[None, :, None, None]
            sd = torch.tensor(self.src.std, dtype=torch.float64)[None, :, None, None]
            a = (self.u8.permute(0, 3, 1, 2).double() / 255.0 - m) / sd
        elif self.coef is None:
            a = self.x.double()
        elif s.entry == "up":
            # bf16: the activation in fp32, left unrounded as in the reference of
            # test_up_backward_b16 (conv_wgrad_taps_b16_kernel does round the activated operand to
            # bf16 on its way to LDS; the 8e-3 bound covers the difference)
            if s.mode == "b16":
                z = self.x * self.coef[0][:, :, None, None] + self.coef[1][:, :, None, None]
                a = F.leaky_relu(z, SLOPE).double()
            else:
                a = act_ref(self.x, *self.coef)
            a = F.interpolate(a, scale_factor=2, mode="bilinear", align_corners=False)
        else:
            a = act_ref(self.x, *self.coef, b16=s.mode == "b16")
        g = torch.nn.grad.conv2d_weight(a, (s.Cout, s.Cx, s.ks, s.ks), self.dy.double(),
                                        stride=s.stride, padding=s.ks // 2)
        return g.view(s.Cout, s.Cx) if s.entry == "1x1" else g

    def tol(self):
        s = self.s
        if s.mode == "b16":      # the bf16 operands: the tolerances of test_bf16_gpu.py
            return 8e-3 if s.entry == "up" else 5e-3
        return 2e-5 if s.c32 == "always" else 3e-5


def immediate(layer):
    assert pending(layer.ua) == 0
    dw = layer(layer.new_dw())
    assert pending(layer.ua) == 0, "a call outside a deferral scope queued a reduction"
    return dw


def short_name(name):
    """A recorded launch without what every weight-gradient kernel shares: the return type, the
    anonymous namespace and the parameter list.  Names the demangler gives up on (__bf16 template
    arguments) stay mangled."""
    if name.startswith("_Z"):
        return name
    return re.sub(r"\(.*\)$", "", name.replace("void ", "").replace("(anonymous namespace)::", ""))


def compute_launches(names):
    return tuple(short_name(n) for n in names if "wgrad_reduce_batched_kernel" not in n)


def outside_cols_kept(layer, dw):
    s = layer.s
    return bool((dw[:, :s.off] == SENTINEL).all()) and \
        bool((dw[:, s.off + s.Cx:] == SENTINEL).all())


def final_kind(s):
    """The final job's kind by the selection rule of emit_wgrad_reduction."""
    if s.Cx == 3:
        return "STEM"
    if s.ks == 1:
        return "CENTER"
    if s.Cx * s.Cout <= 128 * 128:
        return "TAP"
    if s.Cout % 64 == 0 and s.Cx % 16 == 0:
        return "WIDE16" if s.Cx * s.Cout >= 512 * 512 else "WIDE8"
    return "GENERIC"


# --------------------------------------------------------------------------- one call each way
@pytest.mark.parametrize("name", list(CASES))
def test_deferred_equals_immediate(ua, name):
    s = CASES[name]
    assert final_kind(s) == s.kind
    L = Layer(ua, s)
    if s.entry == "conv3x3" and s.stride == 1:
        with ua.ops.c32_winograd_scope(s.c32 if s.c32 is not None else True):
            wino = bool(ua._lib.lib().unet_conv3x3_bwd_weight_is_winograd(s.N, s.H, s.W, s.Cx,
                                                                           s.Cout, 1))
        assert wino == (name in ("conv3x3-winograd", "conv3x3-wino32")), "the case misses its form"
    with ua.ops.record_launches() as rec:
        dw_i = immediate(L)
    assert compute_launches(rec.names) == s.kernel, f"{name}: launched {rec.names}"
    e = relerr(L.cols(dw_i), L.ref())
    assert e <= L.tol(), f"{name}: per-call dw vs fp64: rel err {e:.3e} > {L.tol():.1e}"
    assert outside_cols_kept(L, dw_i)

    dw_d = L.new_dw()
    with ua.ops.wgrad_deferral() as d:
        assert pending(ua) == 0
        L(dw_d)
        n = pending(ua)
        assert n == s.stages, f"{name}: {n} stages queued, the case is for {s.stages}"
        torch.cuda.synchronize()
        assert bool((dw_d == SENTINEL).all()), "dw written before the flush"
        assert d.flush() == s.stages
        assert pending(ua) == 0
    assert torch.equal(dw_d, dw_i), f"{name}: deferred reduction differs from the per-call form"


# --------------------------------------------------------------------------- the batched table
def _check_twins(layers, twins, dws):
    for k, (L, a, b) in enumerate(zip(layers, twins, dws)):
        assert torch.equal(b, a), f"layer {k} ({L.s.entry} {L.s.mode} {L.s.kind}, " \
                                  f"{L.s.stages} stages) differs from its per-call twin"


def test_mixed_flush(ua):
    """One flush of every reduction kind with 1-, 2- and 3-stage layers side by side: the TAP jobs
    (nine blocks per grid cell) come first, so every later job's block_begin depends on them."""
    names = ["up-fp32", "conv3x3-4wave", "in-bf16x3-3stages", "in-b16-stride2", "wide8", "wide16",
             "generic-bf16x3", "center-ksize1", "conv1x1", "stem-rows", "up-b16", "generic"]
    layers = [Layer(ua, CASES[n], seed=3 + 7 * k) for k, n in enumerate(names)]
    assert {L.s.stages for L in layers} == {1, 2, 3}
    assert {final_kind(L.s) for L in layers} == {"TAP", "WIDE8", "WIDE16", "GENERIC", "CENTER",
                                                 "STEM"}
    twins = [immediate(L) for L in layers]
    with ua.ops.wgrad_deferral() as d:
        dws = [L(L.new_dw()) for L in layers]
        total = sum(L.s.stages for L in layers)
        assert pending(ua) == total
        assert d.flush() == total
        assert pending(ua) == 0
        _check_twins(layers, twins, dws)


SMALL = [   # one-stage layers of every kind but STEM, and two-stage ones
    Spec("conv3x3", "fp32", 1, 8, 8, 32, 32),                        # TAP
    Spec("in", "fp32", 1, 8, 8, 64, 64, ks=1, kind="CENTER"),
    Spec("in", "fp32", 1, 4, 8, 256, 128, kind="WIDE8"),
    Spec("up", "b16", 1, 8, 8, 64, 32),                              # TAP
    Spec("in", "fp32", 1, 4, 8, 256, 96, kind="GENERIC"),
    Spec("in", "fp32", 2, 24, 40, 32, 32, stages=2),                 # SLAB + TAP
]


def test_more_than_56_jobs_in_a_stage(ua):
    """60 layers: stage 0 holds 60 jobs, more than one table of 56 - the second launch's
    block_begin restarts at 0; stage 1 holds the final jobs of the two-stage layers."""
    layers = [Layer(ua, SMALL[k % len(SMALL)], seed=100 + k) for k in range(60)]
    assert sum(1 for L in layers if L.s.stages == 2) == 10
    twins = [immediate(L) for L in layers]
    with ua.ops.wgrad_deferral() as d:
        dws = []
        for k, L in enumerate(layers):
            dws.append(L(L.new_dw()))
            assert pending(ua) == sum(M.s.stages for M in layers[:k + 1])
        assert d.flush() == 70
    _check_twins(layers, twins, dws)


def test_flush_in_the_middle_of_a_scope(ua):
    """The data-parallel path: queue, flush (those gradients are final there), queue more, exit."""
    names = ["in-fp32", "stem-rows", "wide16", "up-b16", "generic-bf16x3"]
    layers = [Layer(ua, CASES[n], seed=200 + k) for k, n in enumerate(names)]
    twins = [immediate(L) for L in layers]
    dws = []
    with ua.ops.wgrad_deferral() as d:
        for L in layers[:2]:
            dws.append(L(L.new_dw()))
        assert d.flush() == 2 + 3
        assert pending(ua) == 0
        _check_twins(layers[:2], twins[:2], dws)      # final before the scope ends
        for L in layers[2:]:
            dws.append(L(L.new_dw()))
        assert pending(ua) == 1 + 2 + 2
    assert pending(ua) == 0
    _check_twins(layers, twins, dws)


def test_workspaces_are_held_until_the_flush(ua):
    """While a reduction is queued its slabs live in the call's workspace.  After queuing, tensors
    of the same sizes are allocated and filled with NaN: a workspace the allocator had already
    taken back would be handed out again and overwritten before the flush reads it."""
    names = ["in-bf16x3-3stages", "stem-rows", "conv3x3-winograd", "generic-bf16x3", "up-b16",
             "conv3x3-4wave"]
    layers = [Layer(ua, CASES[n], seed=300 + k) for k, n in enumerate(names)]
    twins = [immediate(L) for L in layers]
    torch.cuda.synchronize()
    torch.cuda.empty_cache()     # (only blocks freed from here on are in the cache)
    with ua.ops.wgrad_deferral() as d:
        dws = [L(L.new_dw()) for L in layers]
        decoys = []
        for L in layers:
            nbytes = max(int(L.workspace_bytes()), 16)
            decoys.append(torch.empty(nbytes, dtype=torch.uint8, device=DEV).fill_(255))  # NaN
        assert d.flush() == sum(L.s.stages for L in layers)
        del decoys
    for L, a, b in zip(layers, twins, dws):
        assert not torch.isnan(b).any(), f"{L.s.entry} {L.s.kind}: read a released workspace"
    _check_twins(layers, twins, dws)


@pytest.mark.parametrize("mode", ["fp32", "b16"])
def test_disjoint_column_slices_in_one_flush(ua, mode):
    """dec4.0: conv3x3(cat(upsample2x(act(low)), act(skip))), 64 up-sampled + 32 skip input
    channels, 32 outputs - both halves of ONE dw through their own entry points, queued together
    (two stages each) and reduced in one flush.  Each call writes only its columns."""
    N, h, w = 2, 64, 64
    up = Layer(ua, Spec("up", mode, N, h, w, 64, 32, extra=32, stages=2), seed=400)
    skip = Layer(ua, Spec("in", mode, N, 2 * h, 2 * w, 32, 32, off=64, stages=2), seed=410)
    dw_up, dw_skip = immediate(up), immediate(skip)
    assert outside_cols_kept(up, dw_up) and outside_cols_kept(skip, dw_skip)
    assert relerr(up.cols(dw_up), up.ref()) <= up.tol()
    assert relerr(skip.cols(dw_skip), skip.ref()) <= skip.tol()
    dw = torch.full((32, 96, 3, 3), SENTINEL, device=DEV)
    with ua.ops.wgrad_deferral() as d:
        up(dw)
        skip(dw)
        assert d.flush() == 4
    assert torch.equal(dw[:, :64], dw_up[:, :64]) and torch.equal(dw[:, 64:], dw_skip[:, 64:])
    # the 1x1 form of the same: two column slices of one [Cout, C0 + C1] gradient
    a = Layer(ua, Spec("1x1", "fp32", 2, 16, 16, 64, 64, ks=1, extra=32, kind="CENTER"), seed=420)
    b = Layer(ua, Spec("1x1", "fp32", 2, 16, 16, 32, 64, ks=1, off=64, kind="CENTER"), seed=430)
    da, db_ = immediate(a), immediate(b)
    dw2 = torch.full((64, 96), SENTINEL, device=DEV)
    with ua.ops.wgrad_deferral():
        a(dw2)
        b(dw2)
        assert pending(ua) == 2
    assert torch.equal(dw2[:, :64], da[:, :64]) and torch.equal(dw2[:, 64:], db_[:, 64:])


# --------------------------------------------------------------------------- scope semantics
def test_nested_scopes_join_the_outer_one(ua):
    """A nested scope on the same thread (a nested backward) joins the outer one: its exit
    flushes what is queued and leaves the queue on; only the outermost exit turns it off."""
    names = ["conv3x3-4wave", "stem-rows", "wide8", "up-b16"]
    layers = [Layer(ua, CASES[n], seed=500 + k) for k, n in enumerate(names)]
    twins = [immediate(L) for L in layers]
    dws = [L.new_dw() for L in layers]
    with ua.ops.wgrad_deferral():
        layers[0](dws[0])
        assert pending(ua) == 2
        with ua.ops.wgrad_deferral() as inner:
            layers[1](dws[1])
            assert pending(ua) == 2 + 3
            assert inner.flush() == 5
            layers[2](dws[2])
            assert pending(ua) == 1
        assert pending(ua) == 0
        _check_twins(layers[:3], twins[:3], dws[:3])
        layers[3](dws[3])                       # the outer scope still defers
        assert pending(ua) == 2
        torch.cuda.synchronize()
        assert bool((dws[3] == SENTINEL).all())
    assert pending(ua) == 0
    _check_twins(layers, twins, dws)
    dw = layers[0].new_dw()                     # and after the outermost exit nothing is queued
    layers[0](dw)
    assert pending(ua) == 0 and torch.equal(dw, twins[0])


def test_bias_gradient_is_refused_before_anything_is_queued(ua):
    """conv3x3_bwd_weight with db reuses the slab workspace, so it cannot be deferred: the call
    raises, queues nothing (no stray job writes its dw at the next flush), and the scope goes on."""
    L = Layer(ua, CASES["conv3x3-4wave"], seed=600)
    M = Layer(ua, CASES["in-fp32"], seed=610)
    twin = immediate(M)
    dw, dwm = L.new_dw(), M.new_dw()
    db = torch.full((L.s.Cout,), SENTINEL, device=DEV)
    with ua.ops.wgrad_deferral() as d:
        with pytest.raises(ua._lib.UNetHipError, match="deferred"):
            ua.ops.conv3x3_bwd_weight(L.src, L.dyd, dw, 0, 1, db=db)
        assert pending(ua) == 0
        M(dwm)
        assert pending(ua) == M.s.stages
        assert d.flush() == M.s.stages
    assert bool((dw == SENTINEL).all()) and bool((db == SENTINEL).all())
    assert torch.equal(dwm, twin)


# --------------------------------------------------------------------------- the whole network
class Immediate:
    """Stand-in for ops.wgrad_deferral: every reduction runs inside its entry point."""
    entered = 0

    def __enter__(self):
        Immediate.entered += 1
        return self

    def __exit__(self, *exc):
        return False

    def flush(self):
        return 0


def _train_grads(ua, mode, hook=None):
    sd0 = O.fill_state_dict(21)
    img, tgt = O.synthetic_batch(4, 2, 256, 256)
    model = ua.UNet()
    model.load_state_dict(sd0)
    model = model.to(DEV).train()
    model.matmul_precision = mode
    model.dropout_mask_override = O.draw_dropout_masks(8, 2)
    if hook is not None:
        model.grad_ready_hook = lambda off: hook(model, off)
    logits = model(img.to(DEV))
    ua.get_loss_function()(logits, tgt.to(DEV)).backward()
    _, garena = model.flat_parameters()
    return garena.clone()


@pytest.mark.parametrize("mode", ["fp32", "bf16x3", "bf16"])
def test_network_gradients_deferred_equal_immediate(ua, monkeypatch, mode):
    """The 44 reductions of a train step through the deferral queue against each one run inside
    its entry point: the whole gradient arena bit-identical, in all three operand modes."""
    deferred = _train_grads(ua, mode)
    Immediate.entered = 0
    with monkeypatch.context() as m:
        m.setattr(ua.ops, "wgrad_deferral", Immediate)
        imm = _train_grads(ua, mode)
    assert Immediate.entered == 1
    assert torch.equal(deferred, imm), "deferred weight-gradient reductions change the gradients"


def test_grad_ready_hook_receives_final_gradients(ua):
    """The data-parallel hook ships garena[off:] as soon as it is called: a snapshot taken in the
    hook (stream-ordered) must equal the gradients at the end of the backward.  A fresh model, so
    the arena does not already hold this step's gradients."""
    seen = []

    def hook(model, off):
        _, garena = model.flat_parameters()
        seen.append((off, garena[off:].clone()))

    final = _train_grads(ua, "fp32", hook=hook)
    assert len(seen) > 1
    assert [o for o, _ in seen] == sorted((o for o, _ in seen), reverse=True)
    for off, snap in seen:
        assert torch.equal(snap, final[off:]), f"gradients at offsets >= {off} changed later"
