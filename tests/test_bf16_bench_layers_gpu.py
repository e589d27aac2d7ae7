"""Every bf16 layer call of the bench step at the shape it runs (-m gpu; BASELINE config 4).

The mixed-precision step runs at bs 8 and 512 x 512, and most of its tile choices depend on how
many tiles a launch has (occupancy), not only on the layer's shape: the small shapes of
test_bf16_gpu.py never reach the big tiles.  So each row of LAYERS below is one convolution call
of that step with the exact geometry of UNet()'s layers at N = 8, 512 x 512 and the operand mode
the network passes (bf16 tensors, activation on load, the pre-rounded bf16 weight plane, the
BSTATS epilogue where the network asks for it), plus the kernel instantiations it must launch.
Each case
  * records the launches of the call (ops.record_launches) and asserts they are the row's names;
  * holds the result to a float64 evaluation of the SAME bf16 operands (inputs rounded, the
    activated operand rounded as the loaders round it, weights rounded as the kernels round
    them): stored bf16 results to one bf16 ulp of the tensor's max, fp32 weight gradients to
    5e-3 of the max and WGRAD_L2 in relative L2;
  * checks the fused statistics (forward) and the BSTATS summaries (data gradients) the network
    uses, as test_bf16_gpu.py does at small shapes.
test_every_bf16_step_kernel_is_held records one whole bs-8 training step and requires every
kernel it launches to be one of the table's - or a non-convolution kernel of ALLOWED, each held
against a reference by the test named next to it.  The references are evaluated on the GPU in
float64, one image at a time (tests/tools/fp64_layer_refs.py); the step recorder and the kernel
names that do not depend on the operand mode are those of tests/tools/step_kernel_harness.py, the
harness of the fp32 and split-bf16 tables.  This file keeps its own runners: they run at the
bench shape, on bf16 operands, against the two-figure bounds below."""
import importlib.util
import math
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("step_kernel_harness", os.path.join(
    os.path.dirname(os.path.abspath(__file__)), "tools", "step_kernel_harness.py"))
HS = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(HS)
R = HS.R
DEV, SLOPE = R.DEV, R.SLOPE
grand, coeffs, nchw64 = R.grand, R.coeffs, R.nchw64
BF = torch.bfloat16
N, HW = 8, 512           # the bench configuration
ULP = 2.0 ** -8          # one bf16 ulp of a tensor's max magnitude
WGRAD_MAX = 5e-3         # fp32 weight gradients: max error / max |ref| (test_conv_in_bwd_weight_b16)
WGRAD_L2 = 1e-4          # ... and relative L2: ~3x the largest measured (2.4e-7 .. 3.0e-5)


# --------------------------------------------------------------------------- operands
# (device-seeded tensors, activation coefficients, layouts: tests/tools/fp64_layer_refs.py)
def b16(shape, seed, scale=1.0, shift=0.0):
    return (grand(shape, seed, scale) + shift).to(BF)


def act_f32(x, al, be):
    """NHWC bf16 raw tensor -> NCHW float64 activated operand: the fp32 activation as the loaders
    compute it, WITHOUT the bf16 operand rounding of R.act64(.., rounded=True) - what the
    up-sampling loader blends and the head kernels read."""
    a = F.leaky_relu(x.float() * al[:, None, None, :] + be[:, None, None, :], SLOPE)
    return a.double().permute(0, 3, 1, 2)


def weights(ua, cout, cin, seed, fan):
    """fp32 OIHW weights and their pack (fp32 layouts + the bf16 plane the network passes)."""
    w = grand((cout, cin, 3, 3), seed, scale=math.sqrt(2.0 / fan))
    return w, HS.pack_one(ua, w, 1)


def next_norm(ua, H, W, C, seed):
    """The layer whose InstanceNorm-backward reductions a BSTATS epilogue emits: raw bf16 output,
    statistics, affine parameters, dropout mask."""
    y = b16((N, H, W, C), seed, 1.5, 0.3)
    gamma, beta = grand((C,), seed + 1) * 0.2 + 1.0, grand((C,), seed + 2) * 0.2
    yf = y.float()
    mean = yf.mean(dim=(1, 2))
    rstd = 1.0 / torch.sqrt(yf.var(dim=(1, 2), unbiased=False) + 1e-5)
    al = gamma[None] * rstd
    st = torch.stack([mean, rstd, al, beta[None] - mean * al]).contiguous()
    g = torch.Generator(device=DEV).manual_seed(seed + 3)
    mask = ((torch.rand((N, C), generator=g, device=DEV) < 0.8).float() / 0.8).contiguous()
    return ua.ops.NextNorm(y, st, gamma, beta, mask, SLOPE)


# --------------------------------------------------------------------------- comparisons
def errs(out, ref):
    """(max error / max |ref|, relative L2) of out against ref (same layout)."""
    d = out.double() - ref
    return (d.abs().max() / ref.abs().max()).item(), (d.norm() / ref.norm()).item()


def metric(what, out, ref, tol, tol_l2=None):
    e, l2 = errs(out, ref)
    return dict(what=what, max=e, l2=l2, tol=tol, tol_l2=tol_l2)


def m_b16(what, out, ref):
    """a stored bf16 result: one bf16 ulp of the tensor's max"""
    return metric(what, out, ref, ULP)


def m_wgrad(what, out, ref):
    return metric(what, out, ref, WGRAD_MAX, WGRAD_L2)


def failures(metrics):
    bad = []
    for m in metrics:
        if not m["max"] <= m["tol"]:
            bad.append(f"{m['what']}: max error {m['max']:.3e} > {m['tol']:.1e}")
        if m["tol_l2"] is not None and not m["l2"] <= m["tol_l2"]:
            bad.append(f"{m['what']}: relative L2 {m['l2']:.3e} > {m['tol_l2']:.1e}")
    return bad


def fused_stats(y_ref, st):
    """statistics of the fused forward (from the fp32 accumulators) against fp64"""
    mean = y_ref.mean(dim=(2, 3))
    rstd = 1.0 / torch.sqrt(y_ref.var(dim=(2, 3), unbiased=False) + 1e-5)
    e_mean = ((st[0].double() - mean).abs().max() / (y_ref.abs().max() + 1)).item()
    return [dict(what="mean", max=e_mean, l2=0.0, tol=2e-3, tol_l2=None),
            metric("rstd", st[1], rstd, 2e-3)]


def summaries(ua, g, nn):
    """The BSTATS summaries drive the InstanceNorm backward like the stand-alone reduction
    (which reads the bf16-stored gradient) does, to bf16 storage precision."""
    assert nn.tiles > 0, "no BSTATS epilogue ran"
    C = nn.y.shape[3]
    outs = []
    for partials in ((nn.partial, nn.tiles), None):
        dg, db, dbias = (torch.empty(C, device=DEV) for _ in range(3))
        dz = ua.ops.instnorm_lrelu_drop_bwd(g.clone(), nn.y, nn.st[0], nn.st[1], nn.gamma, nn.beta,
                                            nn.mask, SLOPE, dg, db, dbias, partials=partials)
        outs.append((dz.float(), dg, db))
    return [metric("dz via summaries", outs[0][0], outs[1][0].double(), 8e-3),
            metric("dgamma via summaries", outs[0][1], outs[1][1].double(), 3e-3),
            metric("dbeta via summaries", outs[0][2], outs[1][2].double(), 3e-3)]


# --------------------------------------------------------------------------- one runner per op
# Each returns (recorded kernel names, metrics).  H, W: the layer's input resolution.
def run_fwd(ua, H, W, C0, C1, Cout, stride):
    """unet_conv_in_fwd_b16_wb: fused forward, both sources activated on load, bf16 weight plane."""
    x0, c0 = b16((N, H, W, C0), 1), coeffs(N, C0, 10)
    x1, c1 = (b16((N, H, W, C1), 2), coeffs(N, C1, 20)) if C1 else (None, None)
    w, table = weights(ua, Cout, C0 + C1, 3, 9 * (C0 + C1))
    b, gamma, beta = grand((Cout,), 4, 0.3), grand((Cout,), 5) * 0.2 + 1.0, grand((Cout,), 6) * 0.2
    s0 = ua.ops.Act(x0, *c0)
    s1 = ua.ops.Act(x1, *c1) if C1 else None
    with ua.ops.record_launches() as rec:
        y, st = ua.ops.conv_in_fwd(s0, s1, SLOPE, table.wf[0], b, 3, stride, gamma, beta, 1e-5,
                                   None, b16=True, w3=table.wf3[0])
    assert y.dtype == BF
    a = R.act64(x0, *c0, rounded=True)
    if C1:
        a = torch.cat([a, R.act64(x1, *c1, rounded=True)], 1)
    y_ref = R.ref_conv(a, w.to(BF).double(), b.double(), stride)
    return rec.names, [m_b16("y", nchw64(y), y_ref)] + fused_stats(y_ref, st)


def run_up_fwd(ua, h, w, C0, C1, Cout):
    """unet_conv_up_in_fwd_b16: the decoder's first convolution, bilinear 2x up-sampling of the
    low-resolution source [N, h, w, C0] in the patch loader, skip [N, 2h, 2w, C1]."""
    low, cl = b16((N, h, w, C0), 1), coeffs(N, C0, 10)
    skip, cs = b16((N, 2 * h, 2 * w, C1), 2), coeffs(N, C1, 20)
    wt, table = weights(ua, Cout, C0 + C1, 3, 9 * (C0 + C1))
    b, gamma, beta = grand((Cout,), 4, 0.3), grand((Cout,), 5) * 0.2 + 1.0, grand((Cout,), 6) * 0.2
    s_low, s_skip = ua.ops.Act(low, *cl), ua.ops.Act(skip, *cs)
    assert ua.ops.conv_up_in_fwd_supported(s_low, s_skip, Cout)    # what UNet.forward asks
    with ua.ops.record_launches() as rec:
        y, st = ua.ops.conv_up_in_fwd(s_low, s_skip, SLOPE, table.wf[0], b, gamma, beta, 1e-5, None,
                                      w3=table.wf3[0])
    assert y.dtype == BF
    # the loader blends the ACTIVATED fp32 taps in PyTorch's order and rounds once
    a_low = act_f32(low, *cl).float()
    a_up = F.interpolate(a_low, scale_factor=2, mode="bilinear", align_corners=False).to(BF)
    a = torch.cat([a_up.double(), R.act64(skip, *cs, rounded=True)], 1)
    del a_low, a_up
    y_ref = R.ref_conv(a, wt.to(BF).double(), b.double(), 1)
    return rec.names, [m_b16("y", nchw64(y), y_ref)] + fused_stats(y_ref, st)


def run_stem_fwd(ua):
    """unet_conv_in_fwd_b16 on the fp32 RGB image (the stem stays fp32; y is stored as bf16)."""
    x = grand((N, HW, HW, 3), 1)
    w, table = weights(ua, 32, 3, 2, 27)
    b, gamma, beta = grand((32,), 3, 0.1), grand((32,), 5) * 0.2 + 1.0, grand((32,), 6) * 0.2
    with ua.ops.record_launches() as rec:
        y, st = ua.ops.conv_in_fwd(ua.ops.Act(x), None, SLOPE, table.wf[0], b, 3, 1, gamma, beta,
                                   1e-5, None, b16=True, w3=table.wf3[0])
    assert y.dtype == BF
    y_ref = R.ref_conv(nchw64(x), w.double(), b.double(), 1)
    return rec.names, [m_b16("y", nchw64(y), y_ref)] + fused_stats(y_ref, st)


def run_dgrad(ua, H, W, Cin, Cout, stride, nxt=False, acc=False, ci_off=0, cin_total=None,
              emits=True):
    """unet_conv3x3_bwd_data_bs_b16_wb: dx[N, H, W, Cin] (+)= the data gradient of dy for input
    channels [ci_off, ci_off + Cin) of a layer with cin_total inputs; nxt = asked for the BSTATS
    epilogue (emits = False: the shape has none, the network runs the stand-alone reduction);
    acc = accumulate into the skip gradient the decoder left."""
    cin_total = cin_total or Cin
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    dy = b16((N, Ho, Wo, Cout), 1)
    w, table = weights(ua, Cout, cin_total, 2, 9 * Cout)
    base = b16((N, H, W, Cin), 3) if acc else None
    nn = next_norm(ua, H, W, Cin, 10) if nxt else None
    wd, wd3 = table.wd[0], table.wd3[0]
    with ua.ops.record_launches() as rec:
        dx = ua.ops.conv3x3_bwd_data(dy, wd, ci_off, Cin, H, W, stride,
                                     out=base.clone() if acc else None, accumulate=acc, bf16="bf16",
                                     wd3=wd3, nxt=nn)
    assert dx.dtype == BF
    ref = R.ref_dgrad(nchw64(dy), w.to(BF).double()[:, ci_off:ci_off + Cin], stride, H, W)
    if acc:
        ref += nchw64(base)
    metrics = [m_b16("dx", nchw64(dx), ref)]
    del ref
    if nxt and not emits:
        assert nn.tiles == 0
    elif nxt:
        plain = ua.ops.conv3x3_bwd_data(dy, wd, ci_off, Cin, H, W, stride,
                                        out=base.clone() if acc else None, accumulate=acc,
                                        bf16="bf16", wd3=wd3)
        assert torch.equal(plain, dx), "the BSTATS epilogue changed the gradient"
        metrics += summaries(ua, dx, nn)
    return rec.names, metrics


def run_wgrad(ua, H, W, Cx, Cout, stride, ci_off=0, cin_total=None, drop_row=None):
    """unet_conv_in_bwd_weight_b16: dw[:, ci_off : ci_off + Cx] of a layer with cin_total inputs,
    operand x [N, H, W, Cx] activated on load.  drop_row = (image, output row): a test of the
    check itself - a second metrics list against a reference evaluated WITHOUT that row of dy."""
    cin_total = cin_total or Cx
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x, coef = b16((N, H, W, Cx), 1), coeffs(N, Cx, 30)
    dy = b16((N, Ho, Wo, Cout), 2)
    dw = torch.zeros(Cout, cin_total, 3, 3, device=DEV)
    with ua.ops.record_launches() as rec:
        ua.ops.conv_in_bwd_weight(ua.ops.Act(x, *coef), SLOPE, dy, dw, ci_off, 3, stride)
    outside = torch.cat([dw[:, :ci_off], dw[:, ci_off + Cx:]], 1)
    assert not outside.any(), "the weight gradient wrote outside its input-channel slice"
    a, dyd = R.act64(x, *coef, rounded=True), nchw64(dy)
    got = dw[:, ci_off:ci_off + Cx]
    metrics = [m_wgrad("dw", got, R.ref_wgrad(a, dyd, stride))]
    if drop_row is None:
        return rec.names, metrics
    n, r = drop_row
    dyd = dyd.clone()
    dyd[n, :, r, :] = 0
    return rec.names, metrics, [m_wgrad("dw against the reference without one dy row", got,
                                        R.ref_wgrad(a, dyd, stride))]


def run_stem_wgrad(ua):
    """unet_conv_in_bwd_weight_b16 of the stem: the fp32 image and bf16 dy."""
    x = grand((N, HW, HW, 3), 1)
    dy = b16((N, HW, HW, 32), 2)
    dw = torch.zeros(32, 3, 3, 3, device=DEV)
    with ua.ops.record_launches() as rec:
        ua.ops.conv_in_bwd_weight(ua.ops.Act(x), SLOPE, dy, dw, 0, 3, 1)
    return rec.names, [m_wgrad("dw", dw, R.ref_wgrad(nchw64(x), nchw64(dy), 1))]


def run_taps(ua, h, w, C):
    """unet_upsample2x_bwd_taps_b16: D[N, h, w, 9 C] from dy[N, 2h, 2w, C]."""
    dy = b16((N, 2 * h, 2 * w, C), 1)
    with ua.ops.record_launches() as rec:
        D = ua.ops.upsample2x_bwd_taps(dy)
    assert D.dtype == BF
    return rec.names, [m_b16("D", D, R.ref_taps(nchw64(dy)))]


def run_up_wgrad(ua, h, w, Cx, Cout, cin_total):
    """unet_conv3x3_up_bwd_weight_b16: dw[:, 0:Cx] of conv3x3(upsample2x(act(low))) as a GEMM over
    the low-resolution pixels q: dw[co, ci, t] = sum_q act(low)[q, ci] D[q, t Cout + co]."""
    low, coef = b16((N, h, w, Cx), 1), coeffs(N, Cx, 40)
    D = b16((N, h, w, 9 * Cout), 2)
    dw = torch.zeros(Cout, cin_total, 3, 3, device=DEV)
    with ua.ops.record_launches() as rec:
        ua.ops.conv3x3_up_bwd_weight(ua.ops.Act(low, *coef), SLOPE, D, dw, 0)
    assert not dw[:, Cx:].any(), "the weight gradient wrote outside its input-channel slice"
    a = R.act64(low, *coef, rounded=True)
    ref = torch.zeros(Cx, 9 * Cout, dtype=torch.double, device=DEV)
    for i in range(N):
        ref += a[i].reshape(Cx, h * w) @ D[i].double().reshape(h * w, 9 * Cout)
    ref = ref.reshape(Cx, 3, 3, Cout).permute(3, 0, 1, 2)
    return rec.names, [m_wgrad("dw", dw[:, :Cx], ref)]


def run_up_dgrad(ua, h, w, C0, Cout, cin_total):
    """unet_conv3x3_up_bwd_data_bs_b16_wb: the low-resolution data gradient of the up-sampled
    operand as a plain GEMM g = D B, B[t Cout + co][ci] = bf16(w[co][ci][t]), with the BSTATS
    epilogue of the layer that produced the low-resolution tensor."""
    wt, table = weights(ua, Cout, cin_total, 3, 9 * Cout)
    D = b16((N, h, w, 9 * Cout), 5)
    nn = next_norm(ua, h, w, C0, 20)
    with ua.ops.record_launches() as rec:
        g = ua.ops.conv3x3_up_bwd_data(D, table.wd[0], 0, C0, nxt=nn, wd3=table.wd3[0])
    assert g.dtype == BF
    wb = wt.to(BF).double()[:, :C0].permute(2, 3, 0, 1).reshape(9 * Cout, C0)
    ref = torch.cat([D[i].double().reshape(-1, 9 * Cout) @ wb for i in range(N)])
    metrics = [m_b16("g", g.reshape(-1, C0), ref)]
    plain = ua.ops.conv3x3_up_bwd_data(D, table.wd[0], 0, C0, wd3=table.wd3[0])
    assert torch.equal(plain, g), "the BSTATS epilogue changed the gradient"
    return rec.names, metrics + summaries(ua, g, nn)


def run_head_fwd(ua):
    """unet_head1x1_in_fwd_b16: fp32 logits (NCHW) of the 1x1 head over the activated bf16 output
    of the last decoder layer (fp32 arithmetic: 1e-4, as test_instnorm_bwd_upsample_head_b16)."""
    y, coef = b16((N, HW, HW, 32), 1), coeffs(N, 32, 50)
    w, b = grand((3, 32), 2, 0.2), grand((3,), 3, 0.1)
    with ua.ops.record_launches() as rec:
        logits = ua.ops.head1x1_in_fwd(ua.ops.Act(y, *coef), SLOPE, w, b)
    a = act_f32(y, *coef)
    ref = torch.einsum("nchw,kc->nkhw", a, w.double()) + b.double()[None, :, None, None]
    return rec.names, [metric("logits", logits, ref, 1e-4)]


def run_head_bwd(ua):
    """unet_head1x1_in_bwd_bs_b16: da = W^T dlogits (bf16), fp32 dW / db, and the InstanceNorm-
    backward reductions of the last decoder layer (whose raw output the head reads)."""
    nn = next_norm(ua, HW, HW, 32, 60)
    x = ua.ops.Act(nn.y, nn.st[2].contiguous(), nn.st[3].contiguous())
    dl = grand((N, 3, HW, HW), 2)
    w = grand((3, 32), 3, 0.2)
    dw, db = torch.empty(3, 32, device=DEV), torch.empty(3, device=DEV)
    with ua.ops.record_launches() as rec:
        da = ua.ops.head1x1_in_bwd(x, SLOPE, dl, w, dw, db, nxt=nn)
    assert da.dtype == BF
    a = act_f32(nn.y, nn.st[2], nn.st[3])
    dld = dl.double()
    metrics = [m_b16("da", nchw64(da), torch.einsum("nkhw,kc->nchw", dld, w.double())),
               metric("dw", dw, torch.einsum("nkhw,nchw->kc", dld, a), 1e-4),
               metric("db", db, dld.sum(dim=(0, 2, 3)), 1e-4)]
    return rec.names, metrics + summaries(ua, da, nn)


# --------------------------------------------------------------------------- the table
# Kernel names as ops.record_launches reports them: demangled, except where the demangler gives
# up on the __bf16 template arguments (mangled, as in profiles/*_kernel_stats.csv).  The names
# that do not depend on the operand mode: tests/tools/step_kernel_harness.py.
_NS, _AN = HS._NS, HS._AN
REDUCE, FIN_GRP, FIN_COMB, FIN_EQ = HS.REDUCE, HS.FIN_GRP, HS.FIN_COMB, HS.FIN_EQ
HEAD_BWD_FIN = HS.HEAD_BWD_FIN


def patch(targs):
    return f"void {_NS}conv_patch_b16_kernel<{targs}>(unet_conv::IgemmParams)"


def dgrad_s2_b16(targs):
    return f"void {_NS}conv_dgrad_s2_patch_b16_kernel<{targs}>(unet_conv::IgemmParams)"


def ring(targs):
    """conv_wgrad_b16_ring_kernel<CI_T, CO_T, S, ACT, DEPTH, RG, STRIDE>: RG = 2 is the
    eight-wave form (two rows a step)"""
    return f"void {_AN}conv_wgrad_b16_ring_kernel<{targs}>({_AN}WgradParams)"


def wtaps_b16(targs):
    return f"void {_AN}conv_wgrad_taps_b16_kernel<{targs}>({_AN}WgradParams)"


def igemm_b16(bm, bn, wm, wn, dense, kg, mode):
    """conv_igemm_bf16_kernel<BM, BN, WM, WN, __bf16, __bf16, FUSED, KG, MODE>"""
    return (f"_ZN9unet_conv12_GLOBAL__N_122conv_igemm_bf16_kernelILi{bm}ELi{bn}ELi{wm}ELi{wn}"
            f"EDF16bDF16bLb{dense}ELi{kg}ELi{mode}EEEvNS_11IgemmParamsE")


STEM_FWD_B16 = ("_ZN9unet_conv12_GLOBAL__N_125conv_stem_fwd_walk_kernelIfDF16bLi8EEEvPKT_PKfS6_PT0_iiii"
                "P15HIP_vector_typeIfLj2EENS0_8StemNormE")
STEM_WGRAD_B16 = "_ZN12_GLOBAL__N_127conv_stem_wgrad_rows_kernelIfDF16bEEvPKT_PKT0_PfiiiiixNS_9StemNormWE"
HEAD_FWD_B16 = "_ZN12_GLOBAL__N_115head_fwd_kernelIDF16bEEvPKT_PKfS5_PfxiiS5_S5_f"
HEAD_BWD_B16 = "_ZN12_GLOBAL__N_115head_bwd_kernelIDF16bEEvPKT_PKfS5_PS1_PfxiixS5_S5_fNS_6HeadBsE"
TAPS_B16 = "_ZN12_GLOBAL__N_126upsample2x_bwd_taps_kernelIDF16bLi2EEEvPKT_PS1_iiix"

# (id, the layers of UNet() it stands for, runner, arguments, expected kernel names in launch
# order).  Encoder stage e, conv k: "e<e>.<k>"; decoder stage d: "d<d>.<k>"; inputs of the
# decoder's first convolutions: the up-sampled lower stage, then the skip.  Layers with the
# same call and geometry share a row.
LAYERS = [
    # ---- forward
    ("stem fwd 3->32 512", "e0.0", run_stem_fwd, dict(),
     [STEM_FWD_B16, FIN_GRP, FIN_COMB]),
    ("fwd 32->32 512", "e0.1 d4.1", run_fwd, dict(H=512, W=512, C0=32, C1=0, Cout=32, stride=1),
     [patch("32, 64, 32, 8, true, true, false, true, false, 1"), FIN_GRP, FIN_COMB]),
    ("fwd 32->64 s2 512", "e1.0", run_fwd, dict(H=512, W=512, C0=32, C1=0, Cout=64, stride=2),
     [patch("64, 64, 32, 4, true, true, false, true, false, 2"), FIN_GRP, FIN_COMB]),
    ("fwd 64->64 256", "e1.1 d3.1", run_fwd, dict(H=256, W=256, C0=64, C1=0, Cout=64, stride=1),
     [patch("64, 64, 64, 8, true, true, false, true, false, 1"), FIN_EQ]),
    ("fwd 64->128 s2 256", "e2.0", run_fwd, dict(H=256, W=256, C0=64, C1=0, Cout=128, stride=2),
     [patch("64, 64, 32, 4, true, true, false, true, false, 2"), FIN_EQ]),
    ("fwd 128->128 128", "e2.1 d2.1", run_fwd, dict(H=128, W=128, C0=128, C1=0, Cout=128, stride=1),
     [patch("64, 64, 64, 8, true, true, false, true, false, 1"), FIN_EQ]),
    ("fwd 128->256 s2 128", "e3.0", run_fwd, dict(H=128, W=128, C0=128, C1=0, Cout=256, stride=2),
     [patch("64, 64, 32, 4, true, true, false, true, false, 2"), FIN_EQ]),
    ("fwd 256->256 64", "e3.1 d1.1", run_fwd, dict(H=64, W=64, C0=256, C1=0, Cout=256, stride=1),
     [patch("64, 64, 64, 8, true, true, false, true, false, 1"), FIN_EQ]),
    ("fwd 256->512 s2 64", "e4.0", run_fwd, dict(H=64, W=64, C0=256, C1=0, Cout=512, stride=2),
     [patch("64, 64, 32, 4, true, true, false, true, false, 2"), FIN_EQ]),
    ("fwd 512->512 32", "e4.1 d0.1", run_fwd, dict(H=32, W=32, C0=512, C1=0, Cout=512, stride=1),
     [patch("128, 64, 64, 4, true, true, false, true, false, 1"), FIN_EQ]),
    ("fwd 512->512 s2 32", "e5.0", run_fwd, dict(H=32, W=32, C0=512, C1=0, Cout=512, stride=2),
     [igemm_b16(64, 64, 32, 32, 1, 4, 1), FIN_EQ]),
    ("fwd 512->512 16", "e5.1", run_fwd, dict(H=16, W=16, C0=512, C1=0, Cout=512, stride=1),
     [igemm_b16(64, 64, 32, 32, 1, 4, 1), FIN_EQ]),
    ("up fwd 512+512->512 32", "d0.0", run_up_fwd, dict(h=16, w=16, C0=512, C1=512, Cout=512),
     [patch("64, 64, 32, 4, true, true, false, true, true, 1"), FIN_EQ]),
    ("up fwd 512+256->256 64", "d1.0", run_up_fwd, dict(h=32, w=32, C0=512, C1=256, Cout=256),
     [patch("64, 64, 64, 8, true, true, false, true, true, 1"), FIN_EQ]),
    ("up fwd 256+128->128 128", "d2.0", run_up_fwd, dict(h=64, w=64, C0=256, C1=128, Cout=128),
     [patch("64, 64, 64, 8, true, true, false, true, true, 1"), FIN_EQ]),
    ("up fwd 128+64->64 256", "d3.0", run_up_fwd, dict(h=128, w=128, C0=128, C1=64, Cout=64),
     [patch("64, 64, 64, 8, true, true, false, true, true, 1"), FIN_EQ]),
    ("up fwd 64+32->32 512", "d4.0", run_up_fwd, dict(h=256, w=256, C0=64, C1=32, Cout=32),
     [patch("32, 64, 32, 8, true, true, false, true, true, 1"), FIN_GRP, FIN_COMB]),
    ("head fwd 32->3 512", "head", run_head_fwd, dict(),
     [HEAD_FWD_B16]),
    # ---- backward: head, decoder (last to first), encoder (last to first)
    ("head bwd 32->3 512", "head", run_head_bwd, dict(),
     [HEAD_BWD_B16, HEAD_BWD_FIN]),
    ("dgrad 32<-32 512 bstats", "d4.1 e0.1", run_dgrad, dict(H=512, W=512, Cin=32, Cout=32, stride=1, nxt=True),
     [patch("32, 64, 32, 8, false, false, true, true, false, 1")]),
    ("wgrad 32->32 512", "d4.1 e0.1", run_wgrad, dict(H=512, W=512, Cx=32, Cout=32, stride=1),
     [ring("32, 32, 64, true, 2, 1, 1"), REDUCE, REDUCE, REDUCE]),
    ("taps 32 512", "d4.0", run_taps, dict(h=256, w=256, C=32),
     [TAPS_B16]),
    ("up wgrad 64->32 256", "d4.0", run_up_wgrad, dict(h=256, w=256, Cx=64, Cout=32, cin_total=96),
     [wtaps_b16("32, 32, 64, true"), REDUCE, REDUCE]),
    ("wgrad skip 32->32 512", "d4.0", run_wgrad, dict(H=512, W=512, Cx=32, Cout=32, stride=1, ci_off=64, cin_total=96),
     [ring("32, 32, 64, true, 2, 1, 1"), REDUCE, REDUCE, REDUCE]),
    ("up dgrad 64<-32 256 bstats", "d4.0", run_up_dgrad, dict(h=256, w=256, C0=64, Cout=32, cin_total=96),
     [igemm_b16(64, 64, 32, 32, 0, 1, 2)]),
    ("dgrad skip 32<-32 512", "d4.0", run_dgrad, dict(H=512, W=512, Cin=32, Cout=32, stride=1, ci_off=64, cin_total=96),
     [patch("32, 64, 32, 8, false, false, false, true, false, 1")]),
    ("dgrad 64<-64 256 bstats", "d3.1 e1.1", run_dgrad, dict(H=256, W=256, Cin=64, Cout=64, stride=1, nxt=True),
     [patch("64, 64, 64, 8, false, false, true, true, false, 1")]),
    ("wgrad 64->64 256", "d3.1 e1.1", run_wgrad, dict(H=256, W=256, Cx=64, Cout=64, stride=1),
     [ring("64, 64, 32, true, 2, 2, 1"), REDUCE, REDUCE]),
    ("taps 64 256", "d3.0", run_taps, dict(h=128, w=128, C=64),
     [TAPS_B16]),
    ("up wgrad 128->64 128", "d3.0", run_up_wgrad, dict(h=128, w=128, Cx=128, Cout=64, cin_total=192),
     [wtaps_b16("64, 64, 16, true"), REDUCE, REDUCE]),
    ("wgrad skip 64->64 256", "d3.0", run_wgrad, dict(H=256, W=256, Cx=64, Cout=64, stride=1, ci_off=128, cin_total=192),
     [ring("64, 64, 32, true, 2, 2, 1"), REDUCE, REDUCE]),
    ("up dgrad 128<-64 128 bstats", "d3.0", run_up_dgrad, dict(h=128, w=128, C0=128, Cout=64, cin_total=192),
     [igemm_b16(64, 64, 32, 32, 0, 1, 2)]),
    ("dgrad skip 64<-64 256", "d3.0", run_dgrad, dict(H=256, W=256, Cin=64, Cout=64, stride=1, ci_off=128, cin_total=192),
     [patch("64, 64, 64, 8, false, false, false, true, false, 1")]),
    ("dgrad 128<-128 128 bstats", "d2.1 e2.1", run_dgrad, dict(H=128, W=128, Cin=128, Cout=128, stride=1, nxt=True),
     [patch("64, 64, 64, 8, false, false, true, true, false, 1")]),
    ("wgrad 128->128 128", "d2.1 e2.1", run_wgrad, dict(H=128, W=128, Cx=128, Cout=128, stride=1),
     [ring("64, 64, 32, true, 2, 2, 1"), REDUCE, REDUCE]),
    ("taps 128 128", "d2.0", run_taps, dict(h=64, w=64, C=128),
     [TAPS_B16]),
    ("up wgrad 256->128 64", "d2.0", run_up_wgrad, dict(h=64, w=64, Cx=256, Cout=128, cin_total=384),
     [wtaps_b16("64, 64, 16, true"), REDUCE, REDUCE]),
    ("wgrad skip 128->128 128", "d2.0", run_wgrad, dict(H=128, W=128, Cx=128, Cout=128, stride=1, ci_off=256, cin_total=384),
     [ring("64, 64, 32, true, 2, 2, 1"), REDUCE, REDUCE]),
    ("up dgrad 256<-128 64 bstats", "d2.0", run_up_dgrad, dict(h=64, w=64, C0=256, Cout=128, cin_total=384),
     [igemm_b16(64, 64, 32, 32, 0, 1, 2)]),
    ("dgrad skip 128<-128 128", "d2.0", run_dgrad, dict(H=128, W=128, Cin=128, Cout=128, stride=1, ci_off=256, cin_total=384),
     [patch("64, 64, 64, 8, false, false, false, true, false, 1")]),
    ("dgrad 256<-256 64 bstats", "d1.1 e3.1", run_dgrad, dict(H=64, W=64, Cin=256, Cout=256, stride=1, nxt=True),
     [patch("64, 64, 64, 8, false, false, true, true, false, 1")]),
    ("wgrad 256->256 64", "d1.1 e3.1", run_wgrad, dict(H=64, W=64, Cx=256, Cout=256, stride=1),
     [ring("64, 64, 32, true, 2, 2, 1"), REDUCE]),
    ("taps 256 64", "d1.0", run_taps, dict(h=32, w=32, C=256),
     [TAPS_B16]),
    ("up wgrad 512->256 32", "d1.0", run_up_wgrad, dict(h=32, w=32, Cx=512, Cout=256, cin_total=768),
     [wtaps_b16("64, 64, 16, true"), REDUCE]),
    ("wgrad skip 256->256 64", "d1.0", run_wgrad, dict(H=64, W=64, Cx=256, Cout=256, stride=1, ci_off=512, cin_total=768),
     [ring("64, 64, 32, true, 2, 2, 1"), REDUCE]),
    ("up dgrad 512<-256 32 bstats", "d1.0", run_up_dgrad, dict(h=32, w=32, C0=512, Cout=256, cin_total=768),
     [igemm_b16(64, 64, 32, 32, 0, 1, 2)]),
    ("dgrad skip 256<-256 64", "d1.0", run_dgrad, dict(H=64, W=64, Cin=256, Cout=256, stride=1, ci_off=512, cin_total=768),
     [patch("64, 64, 64, 8, false, false, false, true, false, 1")]),
    ("dgrad 512<-512 32 bstats", "d0.1 e4.1", run_dgrad, dict(H=32, W=32, Cin=512, Cout=512, stride=1, nxt=True),
     [patch("128, 64, 64, 4, false, false, true, true, false, 1")]),
    ("wgrad 512->512 32", "d0.1 e4.1", run_wgrad, dict(H=32, W=32, Cx=512, Cout=512, stride=1),
     [ring("64, 64, 32, true, 2, 1, 1"), REDUCE]),
    ("taps 512 32", "d0.0", run_taps, dict(h=16, w=16, C=512),
     [TAPS_B16]),
    ("up wgrad 512->512 16", "d0.0", run_up_wgrad, dict(h=16, w=16, Cx=512, Cout=512, cin_total=1024),
     [wtaps_b16("64, 64, 16, true"), REDUCE]),
    ("wgrad skip 512->512 32", "d0.0", run_wgrad, dict(H=32, W=32, Cx=512, Cout=512, stride=1, ci_off=512, cin_total=1024),
     [ring("64, 64, 32, true, 2, 1, 1"), REDUCE]),
    ("up dgrad 512<-512 16 bstats", "d0.0", run_up_dgrad, dict(h=16, w=16, C0=512, Cout=512, cin_total=1024),
     [igemm_b16(64, 64, 32, 32, 0, 4, 2)]),
    ("dgrad skip 512<-512 32", "d0.0", run_dgrad, dict(H=32, W=32, Cin=512, Cout=512, stride=1, ci_off=512, cin_total=1024),
     [patch("128, 64, 64, 4, false, false, false, true, false, 1")]),
    ("dgrad 512<-512 16 bstats", "e5.1", run_dgrad, dict(H=16, W=16, Cin=512, Cout=512, stride=1, nxt=True),
     [igemm_b16(64, 64, 32, 32, 0, 4, 1)]),
    ("wgrad 512->512 16", "e5.1", run_wgrad, dict(H=16, W=16, Cx=512, Cout=512, stride=1),
     [ring("64, 64, 16, true, 2, 1, 1"), REDUCE]),
    ("dgrad s2 512<-512 32 bstats acc", "e5.0", run_dgrad, dict(H=32, W=32, Cin=512, Cout=512, stride=2, nxt=True, acc=True, emits=False),
     [igemm_b16(64, 64, 32, 32, 0, 4, 1)] * 4),
    ("wgrad s2 512->512 32", "e5.0", run_wgrad, dict(H=32, W=32, Cx=512, Cout=512, stride=2),
     [ring("64, 64, 16, true, 2, 1, 2"), REDUCE]),
    ("dgrad s2 256<-512 64 bstats acc", "e4.0", run_dgrad, dict(H=64, W=64, Cin=256, Cout=512, stride=2, nxt=True, acc=True),
     [dgrad_s2_b16("64, 32, 64, 4, true")]),
    ("wgrad s2 256->512 64", "e4.0", run_wgrad, dict(H=64, W=64, Cx=256, Cout=512, stride=2),
     [ring("64, 64, 16, true, 2, 1, 2"), REDUCE]),
    ("dgrad s2 128<-256 128 bstats acc", "e3.0", run_dgrad, dict(H=128, W=128, Cin=128, Cout=256, stride=2, nxt=True, acc=True),
     [dgrad_s2_b16("64, 32, 64, 4, true")]),
    ("wgrad s2 128->256 128", "e3.0", run_wgrad, dict(H=128, W=128, Cx=128, Cout=256, stride=2),
     [ring("64, 64, 16, true, 2, 2, 2"), REDUCE, REDUCE]),
    ("dgrad s2 64<-128 256 bstats acc", "e2.0", run_dgrad, dict(H=256, W=256, Cin=64, Cout=128, stride=2, nxt=True, acc=True),
     [dgrad_s2_b16("64, 32, 64, 4, true")]),
    ("wgrad s2 64->128 256", "e2.0", run_wgrad, dict(H=256, W=256, Cx=64, Cout=128, stride=2),
     [ring("64, 64, 16, true, 2, 2, 2"), REDUCE, REDUCE]),
    ("dgrad s2 32<-64 512 bstats acc", "e1.0", run_dgrad, dict(H=512, W=512, Cin=32, Cout=64, stride=2, nxt=True, acc=True),
     [dgrad_s2_b16("32, 64, 32, 8, true")]),
    ("wgrad s2 32->64 512", "e1.0", run_wgrad, dict(H=512, W=512, Cx=32, Cout=64, stride=2),
     [ring("32, 64, 32, true, 2, 1, 2"), REDUCE, REDUCE, REDUCE]),
    ("stem wgrad 3->32 512", "e0.0", run_stem_wgrad, dict(),
     [STEM_WGRAD_B16, REDUCE, REDUCE, REDUCE]),

]


@pytest.mark.parametrize("row", LAYERS, ids=[r[0] for r in LAYERS])
def test_bench_layer_b16(ua, row):
    ident, layers, runner, kw, expected = row
    names, metrics = runner(ua, **kw)
    assert names == list(expected), f"{ident} ({layers}) launched {names}"
    bad = failures(metrics)
    assert not bad, f"{ident} ({layers}):\n" + "\n".join(bad)


# The kernels of the bf16 step that are not convolutions, each with a test that launches the same
# instantiation against a reference.
ALLOWED = {
    # layout of the input image: test_kernels_gpu.py::test_layout_roundtrip
    HS.NCHW_TO_NHWC,
    # the once-per-step weight pack (incl. the bf16 plane):
    # test_kernels_gpu.py::test_pack_weights_batched_matches_per_layer
    HS.PACK_W,
    # loss forward / finalize / gradient of SimpleLoss (module backward):
    # test_kernels_gpu.py::test_loss_gradient_pass_applies_the_upstream_scalar
    HS.LOSS_REDUCE, HS.LOSS_FINALIZE, HS.LOSS_GRAD,
    # InstanceNorm + LeakyReLU + dropout backward on bf16 tensors, stand-alone reduction and the
    # apply pass: test_bf16_gpu.py::test_instnorm_bwd_upsample_head_b16; fed by BSTATS summaries:
    # test_bf16_gpu.py::test_data_gradient_b16_emits_next_norm_reductions (and the rows above)
    "_ZN12_GLOBAL__N_120in_bwd_reduce_kernelIDF16bEEvPKT_S3_PKfS5_S5_S5_S5_fP15HIP_vector_typeIfLj2EEiii",
    HS.IN_FIN1,
    "_ZN12_GLOBAL__N_119in_bwd_apply_kernelIDF16bEEvPKT_S3_PKfS5_S5_S5_S5_fPK15HIP_vector_typeIfLj2EE"
    "PS1_PfiiiS9_SB_SB_SB_",
    # SGD-Nesterov: test_kernels_gpu.py::test_sgd_golden
    HS.SGD,
}


def test_every_bf16_step_kernel_is_held(ua):
    """One bs-8 512 x 512 training step of UNet() in the mixed-precision mode (forward, loss,
    backward, SGD) launches only kernels that a row of LAYERS or an entry of ALLOWED holds: a
    dispatch change that brings in another bf16 kernel fails here until a case holds it."""
    HS.check_step_is_held(HS.record_step(ua, "bf16"), "bf16", LAYERS, ALLOWED)


def test_weight_gradient_check_sees_one_missing_row(ua):
    """The weight-gradient check at its largest shape (8 x 512^2, 32 -> 32: 2 M pixels) must still
    resolve the loss of one output row of one image (512 of 2 M pixels, the size of error a
    mis-indexed ring row or a dropped slab would make): the kernel passes against the fp64
    reference and the same check rejects it against a reference evaluated without that row."""
    _, good, bad = run_wgrad(ua, 512, 512, 32, 32, 1, drop_row=(5, 301))
    assert not failures(good), failures(good)
    assert failures(bad), f"the check cannot see a missing dy row: {bad}"
