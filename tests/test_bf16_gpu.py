"""Mixed-precision pipeline with bf16 activations in HBM (-m gpu; BASELINE config 4).

The reference's AMP path is fp16 autocast + GradScaler (Our_UNet/src/train.py:638-652); it
publishes no numerics to match.  What is checked here:
  * every *_b16 entry point against a torch fp64 evaluation of the SAME rounded operands
    (inputs are bf16-representable, weights are rounded as the kernels round them), so the only
    differences are fp32 accumulation order, the final bf16 store of the result and the rare
    bf16 rounding-boundary flip of an activated operand;
  * the whole network (forward, loss, all gradients) against the ORACLE evaluated with the same
    rounding points (`unet_forward(..., bf16_storage=True)`: operands of every convolution
    rounded to bf16, results and activation gradients stored as bf16) - not against the HIP fp32
    path;
  * the bs-8 512x512 layer shapes (the 128-column tile instantiations only a full-size launch
    selects) and full-size batch-split invariance.
Tolerances are relative to the tensor's max magnitude: 2^-8 (one bf16 ulp of a stored result)
plus accumulated operand-rounding noise."""
import pytest
import torch
import torch.nn.functional as F

from oracle import unet_ref as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
SLOPE = 0.01
BF = torch.bfloat16


def r16(t):
    return t.to(BF).float()


def to_nhwc_b16(t):
    return t.permute(0, 2, 3, 1).contiguous().to(DEV).to(BF)


def from_nhwc(t):
    return t.float().permute(0, 3, 1, 2).contiguous().cpu()


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def check(a, b, tol, what=""):
    assert a.shape == b.shape, f"{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    e = relerr(a, b)
    assert e <= tol, f"{what}: rel err {e:.3e} > {tol:.1e}"


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def coeffs(n, c, seed):
    al = rnd(n, c, seed=seed) * 0.5 + 1.0
    be = rnd(n, c, seed=seed + 1) * 0.7
    drop = torch.rand(n, c, generator=torch.Generator().manual_seed(seed + 2)) < 0.15
    return torch.where(drop, torch.zeros_like(al), al), torch.where(drop, torch.zeros_like(be), be)


def act_ref(x, al, be):
    """fp32 activation as the loaders compute it, then the bf16 operand rounding."""
    z = x.float() * al[:, :, None, None] + be[:, :, None, None]
    return r16(F.leaky_relu(z, SLOPE)).double()


def src(ua, x_nchw, coef):
    xb = to_nhwc_b16(x_nchw)
    if coef is None:
        return ua.ops.Act(xb)
    return ua.ops.Act(xb, coef[0].to(DEV).contiguous(), coef[1].to(DEV).contiguous())


FWD = [  # (N, H, W, C0, C1, Cout, stride, ksize)
    (2, 16, 32, 64, 32, 64, 1, 3),
    (1, 64, 64, 32, 0, 128, 2, 3),
    (3, 4, 4, 32, 32, 32, 1, 3),        # tiles span images, stand-alone statistics
    (2, 16, 16, 64, 0, 64, 1, 1),
    (1, 128, 128, 32, 32, 32, 1, 3),    # statistics epilogue, 128 x 32 tiles
    (8, 16, 16, 512, 0, 512, 1, 3),     # 1/32-resolution layer at bs 8: K-group gather-GEMM (KG 4)
    (8, 32, 32, 512, 0, 512, 2, 3),     # ... its stride-2 sibling (encoder_stages.5.block.0)
    (2, 16, 16, 64, 64, 64, 1, 3),      # two sources through the K-group form (KG 4)
    (2, 16, 16, 128, 128, 64, 1, 3),    # ... and, with the bf16 weight plane, its 64-wide K steps
    # the stride-2 fused forward on the patch kernel (conv_patch_b16_kernel<.., SD = 2>): one and
    # two 32-channel chunks, image borders on every side, H != W
    (4, 256, 256, 32, 0, 64, 2, 3),
    (2, 256, 128, 64, 0, 128, 2, 3),
    (8, 64, 128, 128, 0, 256, 2, 3),
]


@pytest.mark.parametrize("case", FWD)
def test_conv_in_fwd_b16(ua, case):
    N, H, W, C0, C1, Cout, stride, ks = case
    x0, x1 = r16(rnd(N, C0, H, W, seed=1)), (r16(rnd(N, C1, H, W, seed=2)) if C1 else None)
    c0, c1 = coeffs(N, C0, 10), (coeffs(N, C1, 20) if C1 else None)
    w = rnd(Cout, C0 + C1, ks, ks, seed=3, scale=(2.0 / (ks * ks * (C0 + C1))) ** 0.5)
    b = rnd(Cout, seed=4, scale=0.3)
    gamma, beta = rnd(Cout, seed=5) * 0.2 + 1.0, rnd(Cout, seed=6) * 0.2
    parts = [act_ref(x0, *c0)] + ([act_ref(x1, *c1)] if C1 else [])
    y_ref = F.conv2d(torch.cat(parts, 1), r16(w).double(), b.double(), stride=stride,
                     padding=ks // 2)
    mean_ref = y_ref.mean(dim=(2, 3))
    rstd_ref = 1.0 / torch.sqrt(y_ref.var(dim=(2, 3), unbiased=False) + 1e-5)
    wk = ua.ops.pack_conv3x3_weights(w.to(DEV), want_wd=False)[0] if ks == 3 \
        else w.view(Cout, C0 + C1).to(DEV).contiguous()
    y, st = ua.ops.conv_in_fwd(src(ua, x0, c0), src(ua, x1, c1) if C1 else None, SLOPE, wk,
                               b.to(DEV), ks, stride, gamma.to(DEV), beta.to(DEV), 1e-5, None,
                               b16=True)
    assert y.dtype == BF
    check(from_nhwc(y), y_ref, 6e-3, "y (stored as bf16)")
    # statistics come from the fp32 accumulators, not from the rounded y
    assert (st[0].cpu().double() - mean_ref).abs().max() <= 2e-3 * (y_ref.abs().max() + 1)
    check(st[1].cpu(), rstd_ref, 2e-3, "rstd")
    if ks == 3:
        # with the pack's pre-rounded bf16 weight plane (what the network passes): the patch
        # kernels stage their panels without conversion, the 1/32-resolution gather-GEMM runs on
        # 64-wide K steps (conv_igemm_bf16_kernel MODE 1, activation on the unpacked 16-byte rows)
        table = ua.ops.PackTable([w.to(DEV)], True, None)
        table.run()
        y3, st3 = ua.ops.conv_in_fwd(src(ua, x0, c0), src(ua, x1, c1) if C1 else None, SLOPE,
                                     table.wf[0], b.to(DEV), ks, stride, gamma.to(DEV),
                                     beta.to(DEV), 1e-5, None, b16=True, w3=table.wf3[0])
        check(from_nhwc(y3), y_ref, 6e-3, "y with the bf16 weight plane")
        assert (st3[0].cpu().double() - mean_ref).abs().max() <= 2e-3 * (y_ref.abs().max() + 1)
        check(st3[1].cpu(), rstd_ref, 2e-3, "rstd with the bf16 weight plane")


def test_rgb_stem_to_bf16(ua):
    x = rnd(2, 3, 8, 128, seed=1)
    w, b = rnd(32, 3, 3, 3, seed=2, scale=0.3), rnd(32, seed=3, scale=0.1)
    wf = ua.ops.pack_conv3x3_weights(w.to(DEV), want_wd=False)[0]
    g, be = torch.ones(32), torch.zeros(32)
    y, st = ua.ops.conv_in_fwd(ua.ops.Act(x.permute(0, 2, 3, 1).contiguous().to(DEV)), None, SLOPE,
                               wf, b.to(DEV), 3, 1, g.to(DEV), be.to(DEV), 1e-5, None, b16=True)
    y_ref = F.conv2d(x.double(), w.double(), b.double(), padding=1)    # the stem stays fp32
    assert y.dtype == BF
    check(from_nhwc(y), y_ref, 5e-3, "stem y")
    check(st[0].cpu(), y_ref.mean(dim=(2, 3)), 1e-4, "mean")


@pytest.mark.parametrize("case", [(2, 12, 64, 32, 32, 1, 3), (1, 16, 32, 64, 64, 1, 3),
                                  (2, 16, 32, 64, 64, 2, 3), (2, 32, 128, 32, 64, 2, 3),
                                  (3, 4, 4, 64, 128, 1, 3), (2, 2, 2, 512, 512, 1, 1),
                                  # the row-ring kernel with several strips, several workgroups
                                  # per strip and long walks: four waves (32 x 32 tile) and
                                  # eight waves / two rows a step (64 x 64 tiles)
                                  (2, 256, 192, 32, 32, 1, 3), (2, 128, 96, 64, 128, 1, 3),
                                  # a ragged last strip (W = 80 = 32 + 32 + 16) and an image
                                  # height that is not a power of two
                                  (2, 24, 80, 64, 64, 1, 3), (1, 40, 144, 32, 32, 1, 3),
                                  # stride 2 on the row ring (two input rows a step): 64 x 64
                                  # tiles / eight waves, 32 x 64 tiles, odd sizes
                                  (2, 128, 128, 64, 128, 2, 3), (2, 256, 192, 32, 64, 2, 3),
                                  (1, 48, 80, 64, 64, 2, 3)])
def test_conv_in_bwd_weight_b16(ua, case):
    """Stride 1, bf16 tensors: conv_wgrad_b16_ring_kernel (a workgroup walks down a column strip,
    input rows in an LDS ring, one new row a step at stride 1, two at stride 2; shapes whose row
    count does not split: conv_wgrad_bf16_kernel); 1x1: the centre tap."""
    N, H, W, Cx, Cout, stride, ks = case
    x, coef = r16(rnd(N, Cx, H, W, seed=1)), coeffs(N, Cx, 30)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    dy = r16(rnd(N, Cout, Ho, Wo, seed=2))
    wz = torch.zeros(Cout, Cx, ks, ks, dtype=torch.double, requires_grad=True)
    F.conv2d(act_ref(x, *coef), wz, None, stride=stride, padding=ks // 2).backward(dy.double())
    dw = torch.zeros(Cout, Cx + 32, ks, ks, device=DEV)
    ua.ops.conv_in_bwd_weight(src(ua, x, coef), SLOPE, to_nhwc_b16(dy), dw, 32, ks, stride)
    # the kernel rounds the ACTIVATED operand to bf16 (the fp64 reference above does not): 2^-8 slack
    check(dw[:, 32:].cpu(), wz.grad, 5e-3, "dw")


@pytest.mark.parametrize("case", [(2, 12, 20, 32, 64, 1), (1, 16, 32, 64, 64, 2),
                                  (2, 32, 32, 128, 32, 1),
                                  (2, 256, 256, 64, 32, 2),    # stride-2 patch kernel, 64 columns
                                  (2, 512, 512, 32, 64, 2),    # stride-2 patch kernel, 32 columns x 8 rows
                                  (1, 128, 256, 64, 96, 2)])   # three K chunks, H != W
def test_conv3x3_bwd_data_b16(ua, case):
    N, H, W, Cin, Cout, stride = case
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    dy = r16(rnd(N, Cout, Ho, Wo, seed=1))
    w = rnd(Cout, Cin, 3, 3, seed=2, scale=0.1)
    xz = torch.zeros(N, Cin, H, W, dtype=torch.double, requires_grad=True)
    F.conv2d(xz, r16(w).double(), None, stride=stride, padding=1).backward(dy.double())
    _, wd = ua.ops.pack_conv3x3_weights(w.to(DEV))
    dx = ua.ops.conv3x3_bwd_data(to_nhwc_b16(dy), wd, 0, Cin, H, W, stride)
    assert dx.dtype == BF
    check(from_nhwc(dx), xz.grad, 6e-3, "dx")
    # the same with the pack's pre-rounded bf16 plane (what the network passes): the kernels take
    # their panels from it without conversion, two register sets in flight - bit-identical
    table = ua.ops.PackTable([w.to(DEV)], 1, None)
    table.run()
    dx3 = ua.ops.conv3x3_bwd_data(to_nhwc_b16(dy), table.wd[0], 0, Cin, H, W, stride, bf16="bf16",
                                  wd3=table.wd3[0])
    assert torch.equal(dx3, dx)


@pytest.mark.parametrize("case", [(8, 16, 16, 512, 512, 1),    # the network's 1/32-resolution layers
                                  (8, 32, 32, 512, 512, 2),    # ... and the stride-2 layer into them
                                  (2, 16, 16, 128, 256, 1), (1, 10, 12, 64, 256, 1),   # ragged M
                                  (2, 16, 16, 128, 128, 1)])   # K steps not a multiple of 4: old form
def test_conv3x3_bwd_data_b16_wide_gather(ua, case):
    """Data gradients with at most one 64 x 64 tile per CU and the bf16 weight plane (round 4):
    conv_igemm_bf16_kernel<.., MODE 1> - 64-wide K steps, raw 16-byte loads of both operands, four
    K groups.  Against the fp64 gradient on the same bf16 operands (one rounding of the result)
    and the form without the plane."""
    N, H, W, Cin, Cout, stride = case
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    dy = r16(rnd(N, Cout, Ho, Wo, seed=1))
    w = rnd(Cout, Cin, 3, 3, seed=2, scale=(2.0 / (9 * Cout)) ** 0.5)
    xz = torch.zeros(N, Cin, H, W, dtype=torch.double, device=DEV, requires_grad=True)
    F.conv2d(xz, r16(w).double().to(DEV), None, stride=stride, padding=1).backward(dy.double().to(DEV))
    table = ua.ops.PackTable([w.to(DEV)], 1, None)
    table.run()
    dx = ua.ops.conv3x3_bwd_data(to_nhwc_b16(dy), table.wd[0], 0, Cin, H, W, stride, bf16="bf16",
                                 wd3=table.wd3[0])
    ref = xz.grad.permute(0, 2, 3, 1)
    err = (dx.double() - ref).abs().max().item()
    assert err <= 2.0 ** -8 * ref.abs().max().item() + 1e-6, err
    old = ua.ops.conv3x3_bwd_data(to_nhwc_b16(dy), table.wd[0], 0, Cin, H, W, stride)
    check(dx.float().cpu(), old.float().cpu(), 8e-3, "wide vs 32-wide gather")


def test_instnorm_bwd_upsample_head_b16(ua):
    N, H, W, C = 2, 16, 32, 32
    y = r16(rnd(N, C, H, W, seed=1))
    ga = r16(rnd(N, C, H, W, seed=2))
    gamma, beta = rnd(C, seed=3) * 0.2 + 1.0, rnd(C, seed=4) * 0.2
    mask = (torch.rand(N, C, generator=torch.Generator().manual_seed(5)) < 0.8).float() / 0.8
    yr = y.double().requires_grad_(True)
    a = F.leaky_relu(F.instance_norm(yr, weight=gamma.double(), bias=beta.double(), eps=1e-5),
                     SLOPE) * mask.double()[:, :, None, None]
    a.backward(ga.double())
    mean = y.double().mean(dim=(2, 3)).float()
    rstd = (1.0 / torch.sqrt(y.double().var(dim=(2, 3), unbiased=False) + 1e-5)).float()
    dg, db, dbias = (torch.empty(C, device=DEV) for _ in range(3))
    dy = ua.ops.instnorm_lrelu_drop_bwd(to_nhwc_b16(ga), to_nhwc_b16(y), mean.to(DEV),
                                        rstd.to(DEV), gamma.to(DEV), beta.to(DEV), mask.to(DEV),
                                        SLOPE, dg, db, dbias)
    assert dy.dtype == BF
    check(from_nhwc(dy), yr.grad, 6e-3, "dy")
    # up-sampling of the activated tensor, bf16 in / out
    coef = coeffs(N, C, 40)
    ref = F.interpolate(F.leaky_relu(y.double() * coef[0].double()[:, :, None, None]
                                     + coef[1].double()[:, :, None, None], SLOPE),
                        scale_factor=2, mode="bilinear", align_corners=False)
    up = ua.ops.upsample2x_in_fwd(src(ua, y, coef), SLOPE)
    assert up.dtype == BF
    check(from_nhwc(up), ref, 5e-3, "upsample")
    # head
    w, b = rnd(3, 32, seed=6, scale=0.2), rnd(3, seed=7, scale=0.1)
    ar = F.leaky_relu(y.double() * coef[0].double()[:, :, None, None]
                      + coef[1].double()[:, :, None, None], SLOPE).requires_grad_(True)
    wr = w.double().requires_grad_(True)
    lr = F.conv2d(ar, wr[:, :, None, None], b.double())
    dl = rnd(N, 3, H, W, seed=8)
    lr.backward(dl.double())
    s = src(ua, y, coef)
    logits = ua.ops.head1x1_in_fwd(s, SLOPE, w.to(DEV), b.to(DEV))
    assert logits.dtype == torch.float32
    check(logits.cpu(), lr.detach(), 1e-4, "logits")     # fp32 arithmetic on bf16 storage
    dw, dbv = torch.empty(3, 32, device=DEV), torch.empty(3, device=DEV)
    da = ua.ops.head1x1_in_bwd(s, SLOPE, dl.to(DEV), w.to(DEV), dw, dbv)
    assert da.dtype == BF
    check(from_nhwc(da), ar.grad, 5e-3, "da")
    check(dw.cpu(), wr.grad, 1e-4, "head dw")


@pytest.mark.parametrize("case", [(8, 512, 512), (2, 64, 128)])
def test_head_backward_emits_next_norm_reductions_b16(ua, case):
    """unet_head1x1_in_bwd_bs_b16: the head's backward on bf16 tensors also leaves the reductions of
    the last decoder layer's InstanceNorm backward (from its fp32 values of da, as the convolution
    epilogues do) - same da bits, summaries usable in place of the reduction pass."""
    N, H, W = case
    C, K = 32, 3
    y = r16(rnd(N, H, W, C, seed=30) * 1.5 + 0.3).to(DEV).to(BF)
    gamma, beta = (rnd(C, seed=31) * 0.2 + 1.0).to(DEV), (rnd(C, seed=32) * 0.2).to(DEV)
    yf = y.float()
    mean = yf.mean(dim=(1, 2))
    rstd = 1.0 / torch.sqrt(yf.var(dim=(1, 2), unbiased=False) + 1e-5)
    al = gamma[None] * rstd
    st = torch.stack([mean, rstd, al, beta[None] - mean * al]).contiguous()
    x = ua.ops.Act(y, st[2].contiguous(), st[3].contiguous())
    dl = rnd(N, K, H, W, seed=5).to(DEV)
    w = (rnd(K, C, seed=6) * 0.2).to(DEV)
    dw0, db0, dw1, db1 = (torch.empty(K, C, device=DEV), torch.empty(K, device=DEV),
                          torch.empty(K, C, device=DEV), torch.empty(K, device=DEV))
    ref = ua.ops.head1x1_in_bwd(x, SLOPE, dl, w, dw0, db0)
    nn = ua.ops.NextNorm(y, st, gamma, beta, None, SLOPE)
    g = ua.ops.head1x1_in_bwd(x, SLOPE, dl, w, dw1, db1, nxt=nn)
    assert g.dtype == BF and torch.equal(g, ref) and nn.tiles > 0
    check(dw1.cpu(), dw0.cpu(), 1e-5, "head dw")
    outs = []
    for partials in ((nn.partial, nn.tiles), None):
        dg, db, dbias = (torch.empty(C, device=DEV) for _ in range(3))
        dz = ua.ops.instnorm_lrelu_drop_bwd(g.clone(), y, st[0], st[1], gamma, beta, None, SLOPE,
                                            dg, db, dbias, partials=partials)
        outs.append((dz.float(), dg, db))
    check(outs[0][0], outs[1][0], 8e-3, "dz")
    check(outs[0][1], outs[1][1], 3e-3, "dgamma")
    check(outs[0][2], outs[1][2], 3e-3, "dbeta")


@pytest.mark.parametrize("case", [(2, 8, 16, 64, 64), (1, 16, 16, 32, 64), (3, 2, 2, 64, 64),
                                  (2, 32, 32, 128, 64), (1, 24, 40, 64, 128),
                                  # 32 x 32 channel tiles (the last decoder stage: 64 -> 32):
                                  # conv_wgrad_taps_b16_kernel<32, 32, 64>, ragged last segment
                                  (2, 24, 20, 64, 32), (1, 64, 64, 32, 32)])
def test_up_backward_b16(ua, case):
    N, h, w, Cx, Cout = case
    x, coef = r16(rnd(N, Cx, h, w, seed=1)), coeffs(N, Cx, 60)
    dy = r16(rnd(N, Cout, 2 * h, 2 * w, seed=2))
    wt = rnd(Cout, Cx, 3, 3, seed=3, scale=0.1)
    z = x.float() * coef[0][:, :, None, None] + coef[1][:, :, None, None]
    a = F.leaky_relu(z, SLOPE).double().requires_grad_(True)
    wr = r16(wt).double().requires_grad_(True)
    F.conv2d(F.interpolate(a, scale_factor=2, mode="bilinear", align_corners=False), wr, None,
             padding=1).backward(dy.double())
    D = ua.ops.upsample2x_bwd_taps(to_nhwc_b16(dy))
    assert D.dtype == BF
    dw = torch.zeros(Cout, Cx, 3, 3, device=DEV)
    ua.ops.conv3x3_up_bwd_weight(src(ua, x, coef), SLOPE, D, dw, 0)
    check(dw.cpu(), wr.grad, 8e-3, "dw (D and the operand are bf16)")
    _, wd = ua.ops.pack_conv3x3_weights(wt.to(DEV))
    g = ua.ops.conv3x3_up_bwd_data(D, wd, 0, Cx)
    assert g.dtype == BF
    check(from_nhwc(g), a.grad, 1e-2, "g low")
    # the same with the BSTATS epilogue (unet_conv3x3_up_bwd_data_bs_b16): identical bits, and its
    # summaries drive the InstanceNorm backward like the stand-alone reduction does
    if (h * w) % 64 == 0:
        yl = to_nhwc_b16(r16(rnd(N, Cx, h, w, seed=20) * 1.5 + 0.3))
        gamma = (rnd(Cx, seed=21) * 0.2 + 1.0).to(DEV)
        beta = (rnd(Cx, seed=22) * 0.2).to(DEV)
        yf = yl.float()
        mean = yf.mean(dim=(1, 2))
        rstd = 1.0 / torch.sqrt(yf.var(dim=(1, 2), unbiased=False) + 1e-5)
        st = torch.stack([mean, rstd, torch.zeros_like(mean), torch.zeros_like(mean)]).contiguous()
        nn = ua.ops.NextNorm(yl, st, gamma, beta, None, SLOPE)
        g2 = ua.ops.conv3x3_up_bwd_data(D, wd, 0, Cx, nxt=nn)
        assert torch.equal(g2, g) and nn.tiles > 0
        outs = []
        for partials in ((nn.partial, nn.tiles), None):
            dg, db, dbias = (torch.empty(Cx, device=DEV) for _ in range(3))
            dz = ua.ops.instnorm_lrelu_drop_bwd(g.clone(), yl, st[0], st[1], gamma, beta, None,
                                                SLOPE, dg, db, dbias, partials=partials)
            outs.append((dz.float(), dg, db))
        check(outs[0][0], outs[1][0], 8e-3, "dz")
        check(outs[0][1], outs[1][1], 3e-3, "dgamma")
        check(outs[0][2], outs[1][2], 3e-3, "dbeta")


@pytest.mark.parametrize("case", [
    (8, 64, 64, 128, 64, 0, False),     # K = 576, two column tiles
    (2, 128, 128, 64, 32, 0, False),    # K = 288: steps straddle taps, ragged last step
    (8, 16, 16, 128, 256, 0, False),    # four K groups per tile (64 tiles), K = 2304
    (8, 32, 32, 256, 128, 64, True),    # a column slice of a wider layer, accumulating
    (8, 16, 16, 512, 512, 0, False),    # the 1/32-resolution stage of the network: K = 4608
    (1, 8, 8, 64, 64, 0, False),        # one tile
    (1, 6, 6, 64, 64, 0, False),        # M % 64 != 0: the gather form runs (same entry point)
])
def test_up_backward_data_b16_plain_gemm(ua, case):
    """unet_conv3x3_up_bwd_data_bs_b16_wb (round 4): the low-resolution data gradient of the
    up-sampled operand as a plain bf16 GEMM over the 9 * Cout contiguous values of a D row
    (conv_igemm_bf16_kernel<.., DENSE>; weights from their bf16 plane).  Held to the same GEMM in
    fp64 on the SAME bf16 operands (D and the rounded weights), so only the fp32 accumulation and
    the final rounding differ; to the gather form of test_up_backward_b16 (which is held to
    autograd there); and the BSTATS epilogue must leave the same bits and usable summaries."""
    N, h, w, Cx, Cout, off, acc = case
    ctot = Cx + off + (32 if off else 0)
    wt = rnd(Cout, ctot, 3, 3, seed=3, scale=(2.0 / (9 * Cout)) ** 0.5).to(DEV)
    table = ua.ops.PackTable([wt], True, None)
    table.run()
    wd, wd3 = table.wd[0], table.wd3[0]
    D = r16(rnd(N, h, w, 9 * Cout, seed=5)).to(DEV).to(BF)
    g0 = r16(rnd(N, h, w, Cx, seed=6)).to(DEV).to(BF) if acc else None
    g = ua.ops.conv3x3_up_bwd_data(D, wd, off, Cx, out=g0.clone() if acc else None,
                                   accumulate=acc, wd3=wd3)
    assert g.dtype == BF and g.shape == (N, h, w, Cx)
    # fp64 GEMM on the bf16 operands: B[t * Cout + co][ci] = bf16(w[co][off + ci][t])
    wb = wt.to(BF).double()[:, off:off + Cx].permute(2, 3, 0, 1).reshape(9 * Cout, Cx)
    ref = D.double().reshape(-1, 9 * Cout) @ wb
    if acc:
        ref = ref + g0.double().reshape(-1, Cx)
    err = (g.double().reshape(-1, Cx) - ref).abs().max().item()
    assert err <= 2.0 ** -8 * ref.abs().max().item() + 1e-6, err    # one bf16 rounding of the result
    old = ua.ops.conv3x3_up_bwd_data(D, wd, off, Cx, out=g0.clone() if acc else None,
                                     accumulate=acc)
    check(g.float().cpu(), old.float().cpu(), 8e-3, "plain GEMM vs gather form")
    if (h * w) % 64 == 0 and not acc:
        yl = r16(rnd(N, h, w, Cx, seed=20) * 1.5 + 0.3).to(DEV).to(BF)
        gamma = (rnd(Cx, seed=21) * 0.2 + 1.0).to(DEV)
        beta = (rnd(Cx, seed=22) * 0.2).to(DEV)
        yf = yl.float()
        mean = yf.mean(dim=(1, 2))
        rstd = 1.0 / torch.sqrt(yf.var(dim=(1, 2), unbiased=False) + 1e-5)
        st = torch.stack([mean, rstd, torch.zeros_like(mean), torch.zeros_like(mean)]).contiguous()
        nn = ua.ops.NextNorm(yl, st, gamma, beta, None, SLOPE)
        g2 = ua.ops.conv3x3_up_bwd_data(D, wd, off, Cx, nxt=nn, wd3=wd3)
        assert torch.equal(g2, g) and nn.tiles > 0
        outs = []
        for partials in ((nn.partial, nn.tiles), None):
            dg, db, dbias = (torch.empty(Cx, device=DEV) for _ in range(3))
            dz = ua.ops.instnorm_lrelu_drop_bwd(g.clone(), yl, st[0], st[1], gamma, beta, None,
                                                SLOPE, dg, db, dbias, partials=partials)
            outs.append((dz.float(), dg, db))
        check(outs[0][0], outs[1][0], 8e-3, "dz")
        check(outs[0][1], outs[1][1], 3e-3, "dgamma")
        check(outs[0][2], outs[1][2], 3e-3, "dbeta")


@pytest.mark.parametrize("case", [(8, 256, 256, 64, 32, 32, True), (8, 32, 32, 512, 512, 512, True),
                                  (2, 128, 128, 256, 128, 128, True), (4, 256, 256, 128, 64, 64, True),
                                  (1, 256, 256, 128, 64, 64, True), (2, 16, 32, 64, 64, 64, False)])
def test_conv_up_in_fwd_b16_is_the_materialised_form_bit_for_bit(ua, case):
    """unet_conv_up_in_fwd_b16 (round 4): the first convolution of a decoder stage on bf16 tensors
    with the bilinear up-sampling in the patch loader.  The loader blends the ACTIVATED fp32 taps
    in PyTorch's order and rounds once - exactly what unet_upsample2x_in_fwd_b16 stores - so y and
    the statistics must be IDENTICAL to the materialised form (up-sampled bf16 tensor + the
    two-source convolution), which test_conv_in_fwd_b16 / the network tests hold to the oracle;
    and y is checked against fp64 directly."""
    N, H, W, C0, C1, Cout, tiled = case
    low, skip = r16(rnd(N, C0, H // 2, W // 2, seed=1)), r16(rnd(N, C1, H, W, seed=2))
    cl, cs = coeffs(N, C0, 10), coeffs(N, C1, 20)
    w = rnd(Cout, C0 + C1, 3, 3, seed=3, scale=(2.0 / (9 * (C0 + C1))) ** 0.5)
    b = rnd(Cout, seed=4, scale=0.3)
    gamma, beta = (rnd(Cout, seed=5) * 0.2 + 1.0).to(DEV), (rnd(Cout, seed=6) * 0.2).to(DEV)
    table = ua.ops.PackTable([w.to(DEV)], 1, None)
    table.run()
    wf, w3 = table.wf[0], table.wf3[0]
    s_low, s_skip = src(ua, low, cl), src(ua, skip, cs)
    assert ua.ops.conv_up_in_fwd_supported(s_low, s_skip, Cout) == tiled
    if not tiled:      # (too few tiles: UNet.forward materialises the up-sampled tensor)
        return
    y, st = ua.ops.conv_up_in_fwd(s_low, s_skip, SLOPE, wf, b.to(DEV), gamma, beta, 1e-5, None, w3=w3)
    up = ua.ops.upsample2x_in_fwd(s_low, SLOPE)
    y2, st2 = ua.ops.conv_in_fwd(ua.ops.Act(up), s_skip, SLOPE, wf, b.to(DEV), 3, 1, gamma, beta,
                                 1e-5, None, b16=True, w3=w3)
    assert y.dtype == BF and torch.equal(y, y2), "the loader form differs from the materialised form"
    # (the statistics come from the same fp32 accumulators, merged over tiles of different sizes
    # where the two launches pick different tile shapes: equal to rounding, not bit for bit)
    assert torch.allclose(st, st2, rtol=2e-5, atol=1e-6)
    z_low = low.float() * cl[0][:, :, None, None] + cl[1][:, :, None, None]
    a_up = r16(F.interpolate(F.leaky_relu(z_low, SLOPE), scale_factor=2, mode="bilinear",
                             align_corners=False)).double()      # fp32 blend, ONE rounding
    y_ref = F.conv2d(torch.cat([a_up, r16(act_ref(skip, *cs).float()).double()], 1), r16(w).double(),
                     b.double(), padding=1)
    check(from_nhwc(y), y_ref, 6e-3, "y (stored as bf16)")


# --------------------------------------------------------------------------- whole network
def _hip_run(ua, sd0, img, tgt, masks, mode, fused=True):
    model = ua.UNet()
    model.load_state_dict(sd0)
    model = model.to(DEV).train()
    model.matmul_precision = mode
    model.fused_pipeline = fused
    model.dropout_mask_override = masks
    logits = model(img.to(DEV))
    loss = ua.get_loss_function()(logits, tgt.to(DEV))
    loss.backward()
    return logits.detach().cpu(), loss.item(), {k: p.grad.detach().cpu()
                                                for k, p in model.named_parameters()}


def _rms(a, b):
    a, b = a.double(), b.double()
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()


def test_bf16_pipeline_vs_oracle_with_the_same_rounding_points(ua):
    """Whole network in the mixed-precision mode against the ORACLE evaluated with bf16 operand
    and storage rounding (`bf16_storage=True`), not against the HIP fp32 path.  bf16 noise is
    amplified through 23 conv + InstanceNorm layers, so two bf16 evaluations with different
    summation orders differ from each other as much as each differs from fp32 (relative L2
    0.25-0.45 on the encoder's activation gradients at this size): the check is therefore on the
    DISTANCE TO THE EXACT fp32 RESULT - the HIP pipeline must be no further from it than the
    oracle's own bf16 evaluation (x1.5 + a floor), on the logits (rms), the loss and EVERY
    gradient tensor, the 32..512-element InstanceNorm vectors included (relative L2).

    128 x 128 images: at 64 x 64 the 1/32-resolution layers normalise over four pixels, the
    relative error of every encoder gradient is 0.6-0.8 for the emulation and the HIP run alike,
    and the ratio of two such errors on a 32-element vector scatters by +-50 % (the 2-2.8x cosine
    gaps of round 2's diagnostic on four norm vectors; layer by layer the activation gradients of
    the two are equally far from fp32 at 64, 128 and 256 pixels -
    tests/tools/diag_bf16_layers.py, profiles/r03_bf16_layers_vs_emulation.txt)."""
    sd0 = O.fill_state_dict(3)
    img, tgt = O.synthetic_batch(1, 2, 128, 128)
    masks = O.draw_dropout_masks(4, 2)

    def oracle(emulate):
        osd = O.leaf_state_dict(sd0)
        ol = O.unet_forward(osd, img, masks, bf16_storage=emulate)
        oloss = O.simple_loss(ol, tgt)
        oloss.backward()
        return ol.detach(), oloss.item(), {k: v.grad for k, v in osd.items()}

    l32, loss32, g32 = oracle(False)
    lem, lossem, gem = oracle(True)
    logits, loss, grads = _hip_run(ua, sd0, img, tgt, masks, "bf16")
    e_hip, e_emu = _rms(logits, l32), _rms(lem, l32)
    assert e_hip <= 1.5 * e_emu + 1e-3, f"logits rms vs fp32: HIP {e_hip:.3e}, emulation {e_emu:.3e}"
    assert abs(loss - loss32) <= 1.5 * abs(lossem - loss32) + 5e-3 * abs(loss32)
    cosd = lambda a, b: 1 - F.cosine_similarity(a.double().reshape(1, -1),
                                                b.double().reshape(1, -1)).item()
    flat = lambda d: torch.cat([d[k].double().reshape(-1) for k in g32])
    d_hip, d_emu = cosd(flat(grads), flat(g32)), cosd(flat(gem), flat(g32))
    assert d_hip <= 1.3 * d_emu + 1e-2, f"gradient 1-cos vs fp32: HIP {d_hip:.3e}, emulation {d_emu:.3e}"

    def rel(a, b):
        a, b = a.double(), b.double()
        return ((a - b).norm() / b.norm()).item()

    bad = []
    for k, g in grads.items():
        if g32[k].abs().max() < 1e-4:      # conv biases under InstanceNorm: ~0 in every run
            continue
        r_hip, r_emu = rel(g, g32[k]), rel(gem[k], g32[k])
        if r_hip > 1.5 * r_emu + 0.05:
            bad.append(f"{k} ({g.numel()} elements): relative L2 vs fp32 HIP {r_hip:.3e}, "
                       f"emulation {r_emu:.3e}")
    assert not bad, "\n".join(bad)


def test_bf16_pipeline_trains(ua):
    sd0 = O.fill_state_dict(7)
    model = ua.UNet()
    model.load_state_dict(sd0)
    model = model.to(DEV).train()
    model.matmul_precision = "bf16"
    opt = ua.create_optimizer(model)
    lossf = ua.get_loss_function()
    img, tgt = O.synthetic_batch(3, 2, 64, 64)
    losses = [ua.train_step(model, opt, lossf, img.to(DEV), tgt.to(DEV)).item() for _ in range(12)]
    assert all(l == l for l in losses) and min(losses[-3:]) < losses[0]


def test_bf16_full_size_layers_and_batch_split(ua):
    """bs 8 at 512x512: the 128-column tile instantiations only a full-size launch selects; a
    bs-8 forward/backward must equal four bs-2 passes image by image (logits; gradients summed)."""
    sd0 = O.fill_state_dict(5)
    img, tgt = O.synthetic_batch(2, 8, 512, 512)
    lossf = ua.SimpleLoss(dynamic_weights=False, class_weights=torch.tensor([1.0, 1.0, 1.0]))
    model = ua.UNet()
    model.load_state_dict(sd0)
    model = model.to(DEV).eval()          # eval: no dropout, InstanceNorm is per sample anyway
    model.matmul_precision = "bf16"
    with torch.no_grad():
        full = model(img.to(DEV))
        parts = torch.cat([model(img[i:i + 2].to(DEV)) for i in range(0, 8, 2)])
    # the batch size selects other tiles, i.e. another summation order, and in bf16 a different
    # order flips stored roundings that the InstanceNorm layers amplify (fp32: 2e-5)
    assert _rms(full, parts) <= 3e-2
    model.train()
    model.dropout_mask_override = None
    for p in model.parameters():
        p.grad = None
    torch.manual_seed(0)
    lossf(model(img.to(DEV)), tgt.to(DEV)).backward()
    assert all(torch.isfinite(p.grad).all() for p in model.parameters())


def _bf16_batch_split_distances(ua):
    """bs 8 at 512 x 512 against the sum of four bs-2 runs on the tie-free network
    (negative_slope = 1, the same dropout masks): rms distance of the logits and, per gradient
    tensor, the relative L2 distance ||g8 - sum g2|| / ||g8||.  The biases of the convolutions
    that feed an InstanceNorm are left out: their gradient is zero up to rounding."""
    N, hw = 8, 512
    sd0 = O.fill_state_dict(78, trained_like=True)
    img, _ = O.synthetic_batch(4322, N, hw, hw)
    img = img.to(DEV)
    g = torch.Generator(device="cpu").manual_seed(6)
    dlogits = (torch.randn(N, 3, hw, hw, generator=g) * 1e-3).to(DEV)
    masks = O.draw_dropout_masks(92, N)

    def run(sl):
        model = ua.UNet(nonlin_kwargs={"negative_slope": 1.0, "inplace": True})
        model.load_state_dict(sd0)
        model = model.to(DEV).train()
        model.matmul_precision = "bf16"
        model.dropout_mask_override = [m[sl] for m in masks]
        out = model(img[sl])
        out.backward(dlogits[sl])
        head = model._head_module()
        skip = {f"{k}.bias" for k, m in model.named_modules()
                if isinstance(m, torch.nn.Conv2d) and m is not head}
        betas = {f"{k}.bias" for k, m in model.named_modules()
                 if isinstance(m, torch.nn.InstanceNorm2d)}
        return out.detach(), {k: p.grad.detach().double() for k, p in model.named_parameters()
                              if k not in skip}, betas

    full_logits, full, betas = run(slice(0, N))
    parts = {k: torch.zeros_like(v) for k, v in full.items()}
    logits = []
    for i in range(0, N, 2):
        lg, gr, _ = run(slice(i, i + 2))
        logits.append(lg)
        for k in parts:
            parts[k] += gr[k]
    dist = {k: ((full[k] - parts[k]).norm() / full[k].norm()).item() for k in full}
    return _rms(full_logits, torch.cat(logits)), dist, betas


def test_bf16_full_size_batch_split_tie_free_gradients(ua):
    """The bf16 twin of test_net_gpu.py::test_full_size_batch_split_tie_free_gradients_per_element:
    negative_slope = 1, so no LeakyReLU branch can flip, and bs 8 must equal the sum of four bs-2
    runs on every gradient tensor up to the bf16 storage-rounding noise of the different
    summation orders the two batch sizes select.  Measured on the MI355X (relative L2 per
    tensor): conv weights, InstanceNorm weights and the head 4.1e-3 .. 1.07e-2; InstanceNorm
    biases 1.9e-7 .. 9.5e-2, above 5e-2 only on the 512- and 256-pixel layers of the first two
    encoder stages and decoder stage 3; logits rms 5.8e-3.  Bounds: about 3x the largest of
    each group."""
    rms, dist, betas = _bf16_batch_split_distances(ua)
    assert rms <= 2e-2, f"bs-8 vs bs-2 logits rms {rms:.2e}"
    bad = [f"{k}: {d:.3e}" for k, d in dist.items() if d > (0.3 if k in betas else 3.5e-2)]
    assert len(dist) > 60 and not bad, "\n".join(bad)


@pytest.mark.parametrize("case", [(1, 256, 256, 32, 128, False, 1), (2, 256, 256, 64, 64, True, 1),
                                  (2, 256, 256, 32, 32, False, 1), (2, 16, 16, 64, 64, False, 1),
                                  (8, 16, 16, 512, 512, False, 1), (2, 32, 32, 128, 64, True, 1),
                                  (4, 256, 256, 64, 32, False, 2), (8, 128, 128, 256, 128, False, 2),
                                  (8, 128, 128, 128, 64, True, 2)])
def test_data_gradient_b16_emits_next_norm_reductions(ua, case):
    """unet_conv3x3_bwd_data_bs_b16: the BSTATS epilogue on bf16 tensors (sums from the fp32
    accumulators and the bf16 raw outputs of the layer) - the stride-1 patch kernel, and since
    round 4 the gather-GEMM (incl. its K-group form for the 1/32-resolution layers: the 16 x 16
    shapes) and the stride-2 patch kernel.  Same gradient bits as the plain call; the InstanceNorm
    backward fed by the summaries agrees with the stand-alone reduction (which reads the
    bf16-STORED gradient) to bf16 storage precision."""
    N, H, W, Cout, Ccols, acc, stride = case
    dy = to_nhwc_b16(r16(rnd(N, Cout, H // stride, W // stride, seed=1)))
    w = rnd(Cout, Ccols, 3, 3, seed=2, scale=0.1)
    _, wd = ua.ops.pack_conv3x3_weights(w.to(DEV))
    y = to_nhwc_b16(r16(rnd(N, Ccols, H, W, seed=10) * 1.5 + 0.3))
    gamma = (rnd(Ccols, seed=11) * 0.2 + 1.0).to(DEV)
    beta = (rnd(Ccols, seed=12) * 0.2).to(DEV)
    yf = y.float()
    mean = yf.mean(dim=(1, 2))
    rstd = 1.0 / torch.sqrt(yf.var(dim=(1, 2), unbiased=False) + 1e-5)
    st = torch.stack([mean, rstd, torch.zeros_like(mean), torch.zeros_like(mean)]).contiguous()
    mask = ((torch.rand(N, Ccols, generator=torch.Generator().manual_seed(13)) < 0.8).float()
            / 0.8).to(DEV)
    base = to_nhwc_b16(r16(rnd(N, Ccols, H, W, seed=3))) if acc else None
    ref = ua.ops.conv3x3_bwd_data(dy, wd, 0, Ccols, H, W, stride, out=base.clone() if acc else None,
                                  accumulate=acc)
    nn = ua.ops.NextNorm(y, st, gamma, beta, mask, SLOPE)
    g = ua.ops.conv3x3_bwd_data(dy, wd, 0, Ccols, H, W, stride, out=base.clone() if acc else None,
                                accumulate=acc, nxt=nn)
    assert torch.equal(g, ref)
    assert nn.tiles > 0
    outs = []
    for partials in ((nn.partial, nn.tiles), None):
        dg, db, dbias = (torch.empty(Ccols, device=DEV) for _ in range(3))
        dz = ua.ops.instnorm_lrelu_drop_bwd(g.clone(), y, st[0], st[1], gamma, beta, mask, SLOPE,
                                            dg, db, dbias, partials=partials)
        outs.append((dz.float(), dg, db))
    check(outs[0][0], outs[1][0], 8e-3, "dy")
    check(outs[0][1], outs[1][1], 3e-3, "dgamma")
    check(outs[0][2], outs[1][2], 3e-3, "dbeta")


@pytest.mark.parametrize("case", [(2, 64, 64, 128, 0, 128), (1, 128, 128, 64, 64, 64),
                                  (1, 64, 64, 32, 0, 32)])
def test_prerounded_bf16_weights_are_bit_identical(ua, case):
    """unet_conv_in_fwd_b16_wb / unet_conv3x3_bwd_data_bs_b16_wb: the patch kernels stage weight
    panels that were rounded to bf16 once per step (plane 0 of the pack's planes) instead of
    converting the fp32 weights per tile - the same rounding, so the results must be EQUAL."""
    N, H, W, C0, C1, Cout = case
    x0, c0 = r16(rnd(N, C0, H, W, seed=1)), coeffs(N, C0, 10)
    x1 = r16(rnd(N, C1, H, W, seed=2)) if C1 else None
    c1 = coeffs(N, C1, 20) if C1 else None
    w = rnd(Cout, C0 + C1, 3, 3, seed=3, scale=0.1).to(DEV)
    b = rnd(Cout, seed=4, scale=0.3).to(DEV)
    g1, b1 = torch.ones(Cout, device=DEV), torch.zeros(Cout, device=DEV)
    table = ua.ops.PackTable([w], True)
    table.run()
    wf, wd, wf3, wd3 = table.wf[0], table.wd[0], table.wf3[0], table.wd3[0]
    assert torch.equal(wf3[0].float(), wf.to(BF).float())   # plane 0 = the rounded weight
    s0 = src(ua, x0, c0)
    s1 = src(ua, x1, c1) if C1 else None
    args = (s0, s1, SLOPE, wf, b, 3, 1, g1, b1, 1e-5, None)
    y_a, st_a = ua.ops.conv_in_fwd(*args, b16=True)
    y_b, st_b = ua.ops.conv_in_fwd(*args, b16=True, w3=wf3)
    assert torch.equal(y_a, y_b) and torch.equal(st_a, st_b)
    dy = to_nhwc_b16(r16(rnd(N, Cout, H, W, seed=5)))
    dx_a = ua.ops.conv3x3_bwd_data(dy, wd, 0, C0, H, W, 1, bf16="bf16")
    dx_b = ua.ops.conv3x3_bwd_data(dy, wd, 0, C0, H, W, 1, bf16="bf16", wd3=wd3)
    assert torch.equal(dx_a, dx_b)


def test_weight_gradient_shape_sweep_b16(ua):
    """Twenty-four seeded shapes (heights that are and are not multiples of the ring's round,
    ragged strips, both strides, every channel tile) through unet_conv_in_bwd_weight_b16: each
    lands on the row-ring kernel (one or two row groups), or - when the rows do not split - on the
    segment kernel, and all are held against the fp64 evaluation of the same bf16 operands."""
    g = torch.Generator().manual_seed(1234)
    pick = lambda xs: xs[int(torch.randint(len(xs), (1,), generator=g))]
    for case in range(24):
        stride = pick([1, 1, 2])
        Cx, Cout = pick([32, 64, 128]), pick([32, 64, 128])
        N = pick([1, 2, 3])
        H = pick([8, 12, 16, 20, 24, 40, 64]) * stride
        W = pick([16, 32, 48, 80, 96]) * stride
        x, coef = r16(rnd(N, Cx, H, W, seed=100 + case)), coeffs(N, Cx, 200 + case)
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        dy = r16(rnd(N, Cout, Ho, Wo, seed=300 + case))
        wz = torch.zeros(Cout, Cx, 3, 3, dtype=torch.double, requires_grad=True)
        F.conv2d(act_ref(x, *coef), wz, None, stride=stride, padding=1).backward(dy.double())
        dw = torch.zeros(Cout, Cx, 3, 3, device=DEV)
        ua.ops.conv_in_bwd_weight(src(ua, x, coef), SLOPE, to_nhwc_b16(dy), dw, 0, 3, stride)
        check(dw.cpu(), wz.grad, 5e-3, f"dw case {case}: N={N} {H}x{W} {Cx}->{Cout} stride {stride}")
