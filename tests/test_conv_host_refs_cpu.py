"""CPU: tests/tools/conv_host_refs.py, the float64 references that tests/test_conv_host_fp64_gpu.py
holds every recorded convolution forward / data-gradient launch to, checked on tiny tensors
without the library:
  * each convolution reference against an independent nine-tap evaluation of the same packed
    weights - shifted slices and einsum in float64, no conv2d, the bilinear up-sampling written out
    as its 0.75 / 0.25 stencil - to 1e-12;
  * the tile merge against mean / var of the concatenated data;
  * the coherent weight planes of the table's generator, the uint8 normalisation;
  * closure: every recorded kernel name is launched by a row the GPU file parametrizes, and every
    family of the table has a reference function."""
import importlib.util
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(ROOT, "tests", "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load("make_conv_host_gpu_table")
C = _load("conv_host_refs")
TOL = 1e-12


def rnd(shape, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def close(got, want):
    want = want.double()
    return (got.double() - want).abs().max().item() <= TOL * max(1.0, want.abs().max().item())


# --------------------------------------------------------------------------- independent forms
def taps_fwd(a, wf, bias, stride):
    """a NHWC float64, wf [k*k][Cout][Cin] -> y NHWC: sum over the taps of shifted slices"""
    n, H, W, _ = a.shape
    k = 3 if wf.shape[0] == 9 else 1
    pad = k // 2
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    p = torch.zeros(n, H + 2 * pad, W + 2 * pad, a.shape[3], dtype=torch.double)
    p[:, pad:pad + H, pad:pad + W] = a
    y = torch.zeros(n, Ho, Wo, wf.shape[1], dtype=torch.double) + bias.double()
    for ky in range(k):
        for kx in range(k):
            sl = p[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
            y += torch.einsum("nhwc,oc->nhwo", sl, wf[ky * k + kx].double())
    return y


def taps_dgrad(dy, wd, ci_offset, Ccols, stride, H, W):
    """dy NHWC float64, wd [k*k][Cin_total][Cout] -> dx NHWC [n, H, W, Ccols]: every tap scatters
    into the padded gradient"""
    n, Ho, Wo, _ = dy.shape
    k = 3 if wd.shape[0] == 9 else 1
    pad = k // 2
    p = torch.zeros(n, H + 2 * pad, W + 2 * pad, Ccols, dtype=torch.double)
    for ky in range(k):
        for kx in range(k):
            w = wd[ky * k + kx, ci_offset:ci_offset + Ccols].double()
            p[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride] += \
                torch.einsum("nhwo,co->nhwc", dy, w)
    return p[:, pad:pad + H, pad:pad + W]


def up2(a):
    """bilinear 2x (align_corners = False) of an NHWC tensor as its stencil: out[2i] = 0.75 a[i] +
    0.25 a[i - 1], out[2i + 1] = 0.75 a[i] + 0.25 a[i + 1], indices clamped; rows, then columns"""
    def along(x, d):
        m = x.shape[d]
        idx = torch.arange(m)
        lo = x.index_select(d, (idx - 1).clamp_min(0))
        hi = x.index_select(d, (idx + 1).clamp_max(m - 1))
        even, odd = 0.75 * x + 0.25 * lo, 0.75 * x + 0.25 * hi
        shape = list(x.shape)
        shape[d] = 2 * m
        return torch.stack([even, odd], d + 1).reshape(shape)
    return along(along(a, 1), 2)


def lrelu(z):
    return torch.where(z > 0, z, C.SLOPE * z)


def act(x, al, be):
    return lrelu(x.double() * al.double()[:, None, None, :] + be.double()[:, None, None, :])


# --------------------------------------------------------------------------- convolutions
@pytest.mark.parametrize("stride", (1, 2))
def test_plain_forward_two_sources(stride):
    row = dict(C0=4, C1=8, stride=stride, H=5, W=6)
    t = dict(x0=rnd((2, 5, 6, 4), 1), x1=rnd((2, 5, 6, 8), 2), wf=rnd((9, 8, 12), 3, 0.1),
             bias=rnd((8,), 4))
    want = taps_fwd(torch.cat([t["x0"], t["x1"]], 3).double(), t["wf"], t["bias"], stride)
    assert close(C.REFS["fwd"](row, t, "f32")["y"], want)
    # bf16 cores on fp32 tensors: operands and weights rounded, the bias not
    BF = torch.bfloat16
    want = taps_fwd(torch.cat([t["x0"], t["x1"]], 3).to(BF).double(), t["wf"].to(BF), t["bias"],
                    stride)
    assert close(C.REFS["fwd"](row, t, "core")["y"], want)
    assert not close(C.REFS["fwd"](row, t, "f32")["y"], want)


def test_rgb_stem_stays_unrounded():
    row = dict(C0=3, H=5, W=6)
    t = dict(x0=rnd((2, 5, 6, 3), 1), wf=rnd((9, 8, 3), 3, 0.1), bias=rnd((8,), 4))
    want = taps_fwd(t["x0"].double(), t["wf"], t["bias"], 1)
    for mode in ("f32", "core"):
        assert close(C.REFS["fwd"](row, t, mode)["y"], want)


def test_one_by_one():
    row = dict(C0=4, C1=4, H=5, W=6)
    t = dict(x0=rnd((2, 5, 6, 4), 1), x1=rnd((2, 5, 6, 4), 2), wf=rnd((1, 8, 8), 3, 0.1),
             bias=rnd((8,), 4))
    want = taps_fwd(torch.cat([t["x0"], t["x1"]], 3).double(), t["wf"], t["bias"], 1)
    assert close(C.REFS["c1x1"](row, t, "f32")["y"], want)
    row = dict(H=5, W=6, Ccols=4, ci_offset=8)
    t = dict(dy=rnd((2, 5, 6, 8), 1), wd=rnd((1, 12, 8), 2, 0.1), base=rnd((2, 5, 6, 4), 3))
    want = taps_dgrad(t["dy"].double(), t["wd"], 8, 4, 1, 5, 6) + t["base"].double()
    assert close(C.REFS["c1x1"](row, t, "f32")["dx"], want)


@pytest.mark.parametrize("stride", (1, 2))
def test_data_gradient_channel_slice_accumulate(stride):
    H, W = 6, 8
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    row = dict(H=H, W=W, Ccols=4, ci_offset=8, stride=stride)
    t = dict(dy=rnd((2, Ho, Wo, 8), 1), wd=rnd((9, 12, 8), 2, 0.1), base=rnd((2, H, W, 4), 3))
    want = taps_dgrad(t["dy"].double(), t["wd"], 8, 4, stride, H, W) + t["base"].double()
    assert close(C.REFS["bwd"](row, t, "f32")["dx"], want)
    # bf16 tensors: the weights rounded, the bf16 base added
    BF = torch.bfloat16
    tb = dict(dy=t["dy"].to(BF), wd=t["wd"], base=t["base"].to(BF))
    want = taps_dgrad(tb["dy"].double(), t["wd"].to(BF), 8, 4, stride, H, W) + tb["base"].double()
    assert close(C.REFS["bs"](row, tb, "b16")["dx"], want)


def test_data_gradient_is_the_adjoint_of_the_forward():
    """<conv(x), dy> = <x, dgrad(dy)> with wd the transpose of wf: ties the two weight layouts"""
    wf = rnd((9, 8, 4), 1, 0.1)
    x, dy = rnd((2, 5, 6, 4), 2), rnd((2, 3, 3, 8), 3)
    y = C.REFS["fwd"](dict(C0=4, stride=2, H=5, W=6),
                      dict(x0=x, wf=wf, bias=torch.zeros(8)), "f32")["y"]
    dx = C.REFS["bwd"](dict(H=5, W=6, Ccols=4, stride=2),
                       dict(dy=dy, wd=wf.permute(0, 2, 1).contiguous()), "f32")["dx"]
    assert abs((y * dy.double()).sum().item() - (dx * x.double()).sum().item()) <= 1e-11


def test_fused_forward_activates_its_sources():
    row = dict(C0=4, C1=4, stride=2, H=5, W=6)
    t = dict(s0=rnd((2, 5, 6, 4), 1), a0=rnd((2, 4), 5), b0=rnd((2, 4), 6), s1=rnd((2, 5, 6, 4), 2),
             w=rnd((9, 8, 8), 3, 0.1), bias=rnd((8,), 4))
    a = torch.cat([act(t["s0"], t["a0"], t["b0"]), t["s1"].double()], 3)
    want = taps_fwd(a, t["w"], t["bias"], 2)
    got = C.REFS["in"](row, t, "f32")
    assert close(got["y"], want)
    assert close(got["stat_mean"], want.mean(dim=(1, 2)))
    assert close(got["stat_var"], want.var(dim=(1, 2), unbiased=False))
    # bf16 tensors: fp32 activation rounded to bf16, bf16 weights
    BF = torch.bfloat16
    tb = dict(t, s0=t["s0"].to(BF), s1=t["s1"].to(BF))
    z = tb["s0"].float() * t["a0"][:, None, None, :] + t["b0"][:, None, None, :]
    a0 = torch.where(z > 0, z, torch.tensor(C.SLOPE) * z).to(BF)
    want = taps_fwd(torch.cat([a0.double(), tb["s1"].double()], 3), t["w"].to(BF), t["bias"], 2)
    assert close(C.REFS["in"](row, tb, "b16")["y"], want)


def test_up_sampling_forward():
    row = dict(C0=4, C1=4, H=6, W=8)
    t = dict(s0=rnd((2, 3, 4, 4), 1), a0=rnd((2, 4), 5), b0=rnd((2, 4), 6), s1=rnd((2, 6, 8, 4), 2),
             a1=rnd((2, 4), 7), b1=rnd((2, 4), 8), w=rnd((9, 8, 8), 3, 0.1), bias=rnd((8,), 4))
    a = torch.cat([up2(act(t["s0"], t["a0"], t["b0"])), act(t["s1"], t["a1"], t["b1"])], 3)
    assert close(C.REFS["upf"](row, t, "f32")["y"], taps_fwd(a, t["w"], t["bias"], 1))


def test_up_sampled_data_gradient():
    row = dict(H=3, W=4, Ccols=4, ci_offset=4)
    D, wd = rnd((2, 3, 4, 9 * 8), 1), rnd((9, 12, 8), 2, 0.1)
    base = rnd((2, 3, 4, 4), 3)
    want = torch.einsum("nhwto,tco->nhwc", D.double().view(2, 3, 4, 9, 8), wd[:, 4:8].double())
    got = C.REFS["upb"](row, dict(dy=D, wd=wd, base=base), "f32")["dx"]
    assert close(got, want + base.double())


def test_up_sampled_data_gradient_is_the_adjoint_of_the_up_sampling_forward():
    """<conv(up(low)), dy> = <low, D(dy) B>: D from R.ref_taps, B from the same packed weight"""
    wf = rnd((9, 8, 4), 1, 0.1)
    low, dy = rnd((1, 3, 4, 4), 2), rnd((1, 6, 8, 8), 3)
    y = C.REFS["upf"](dict(C0=4, H=6, W=8), dict(s0=low, w=wf, bias=torch.zeros(8)), "f32")["y"]
    D = C.R.ref_taps(C.R.nchw64(dy))
    g = C.REFS["upb"](dict(H=3, W=4, Ccols=4), dict(dy=D, wd=wf.permute(0, 2, 1).contiguous()),
                      "f32")["dx"]
    assert abs((y * dy.double()).sum().item() - (g * low.double()).sum().item()) <= 1e-11


def test_dropped_row_changes_the_reference():
    row = dict(C0=4, H=5, W=6)
    t = dict(x0=rnd((2, 5, 6, 4), 1), wf=rnd((9, 8, 4), 3, 0.1), bias=rnd((8,), 4))
    x = t["x0"].double().clone()
    x[1, 2] = 0
    assert close(C.REFS["fwd"](row, t, "f32", drop=(1, 2))["y"], taps_fwd(x, t["wf"], t["bias"], 1))


# --------------------------------------------------------------------------- the side outputs
@pytest.mark.parametrize("tiles", (1, 2, 7))
def test_tile_merge(tiles):
    data = rnd((2, tiles, 16, 4), 1).double() + 0.7          # [n, tiles, count, c]
    pairs = torch.stack([data.mean(2), ((data - data.mean(2, keepdim=True)) ** 2).sum(2)], -1)
    mean, var = C.merge_tiles(pairs, 16)
    flat = data.reshape(2, tiles * 16, 4)
    assert close(mean, flat.mean(1)) and close(var, flat.var(1, unbiased=False))


def test_tile_sums_and_views():
    pairs = rnd((2, 3, 4, 2), 1)
    s1, s2 = C.sum_tiles(C.tile_pairs(pairs.contiguous().view(-1).view(torch.uint8), 2, 4))
    assert close(s1, pairs[..., 0].double().sum(1)) and close(s2, pairs[..., 1].double().sum(1))


def test_bstats_formula():
    g, y = rnd((2, 4, 5, 6), 1).double(), rnd((2, 4, 5, 6), 2).double()
    mean, rstd, mask = rnd((2, 4), 3), rnd((2, 4), 4).abs() + 0.5, (rnd((2, 4), 5) > 0).float() * 2
    gamma, beta = rnd((4,), 6), rnd((4,), 7)
    s1, s2 = C.bstats64(g, y, mean, rstd, gamma, beta, mask)
    for n in range(2):
        for c in range(4):
            xh = (y[n, c] - mean[n, c].double()) * rstd[n, c].double()
            z = gamma[c].double() * xh + beta[c].double()
            gz = g[n, c] * mask[n, c].double()
            gz = torch.where(z > 0, gz, C.SLOPE * gz)
            assert abs(s1[n, c] - gz.sum()) <= 1e-11 and abs(s2[n, c] - (gz * xh).sum()) <= 1e-11


@pytest.mark.parametrize("stats_px", (0, 12))
def test_finalize(stats_px):
    row = dict(stats_px=stats_px, W=6)
    y = rnd((2, 24, 4), 1) + 0.5
    gamma, beta, mask = rnd((4,), 2), rnd((4,), 3), (rnd((2, 4), 4) > 0).float() * 2
    d = y.double().view(2, 2, 12, 4)
    tiles = torch.stack([d.mean(2), ((d - d.mean(2, keepdim=True)) ** 2).sum(2)], -1).float()
    src = tiles.double().view(2, 2, 4, 2)
    got = C.REFS["fin"](row, dict(y=y, gamma=gamma, beta=beta, mask=mask, tiles=tiles), "f32")
    if stats_px:
        mean = src[..., 0].mean(1)
        var = (src[..., 1].sum(1) + 12 * ((src[..., 0] - mean[:, None]) ** 2).sum(1)) / 24
    else:
        mean, var = y.double().mean(1), y.double().var(1, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    assert close(got["mean"], mean) and close(got["rstd"], rstd)
    assert close(got["alpha"], gamma.double() * rstd * mask.double())
    assert close(got["beta"], (beta.double() - mean * gamma.double() * rstd) * mask.double())


def test_uint8_normalisation():
    g = torch.Generator().manual_seed(1)
    img = torch.randint(0, 256, (2, 5, 6, 3), generator=g, dtype=torch.uint8)
    mean3, std3 = torch.tensor((0.485, 0.456, 0.406)), torch.tensor((0.229, 0.224, 0.225))
    x = C.normalize_u8(img, mean3, std3)
    for c in range(3):
        want = (img[..., c].double() / 255.0 - float(mean3[c])) / float(std3[c])
        assert close(x[:, c], want)
    t = dict(image=img, mean3=mean3, std3=std3, wf=rnd((9, 8, 3), 2, 0.1), bias=rnd((8,), 3))
    want = taps_fwd(x.permute(0, 2, 3, 1), t["wf"], t["bias"], 1)     # zero padding after it
    assert close(C.REFS["u8"](dict(), t, "f32")["y"], want)


def test_coherent_planes():
    w = rnd((9, 8, 12), 1, 0.05)
    three = G.coherent_planes(w, 3)
    assert three.shape == (3, 9, 8, 12) and three.dtype == torch.bfloat16
    err = (three.double().sum(0) - w.double()).abs()
    assert bool((err <= 2.0 ** -24 * w.double().abs()).all())
    hh, mm, ll = C.R.split3(w)
    assert torch.equal(three.double(), torch.stack([hh, mm, ll]))
    one = G.coherent_planes(w, 1)
    assert one.shape == (1, 9, 8, 12) and torch.equal(one[0], w.bfloat16())
    # a 1x1 weight: its single tap in every slot
    assert torch.equal(G.coherent_planes(w[:1], 1)[0, 5], w[0].bfloat16())


# --------------------------------------------------------------------------- closure
def test_every_recorded_kernel_is_launched_by_a_row_of_the_gpu_file():
    import json
    with open(G.TABLE) as f:
        kernels = set(json.load(f)["kernels"])
    recorded = {r["id"]: r for r in G.load_table()}
    # (the GPU file parametrizes over G.ROWS and gives every row a reference: see below)
    held = {k for row in G.ROWS for k in recorded[row["id"]]["launches"]}
    assert kernels == held, sorted(kernels ^ held)
    assert len(G.ROWS) == len(recorded) == 378 and len(kernels) == 118


def test_rows_held_on_dx_alone_report_nothing():
    """A gradient row with a short partial buffer, without unet_bwd_stats or with a chunk limit
    is recorded with tiles_out 0 / -1 and without BSTATS bytes: the GPU file asserts the recorded
    report, so such a row is held on dx alone - and every other BSTATS row on S1 / S2 too or on
    a recorded 0 (a shape without the epilogue)."""
    recorded = {r["id"]: r for r in G.load_table()}
    grads = [r for r in G.ROWS if "Ccols" in r]
    assert grads
    for row in grads:
        rec = recorded[row["id"]]
        if row.get("bs") != "ok" or row.get("lim"):
            assert rec["report"] in (0, -1) and set(rec["crc"]) == {"dx"}, row
        else:
            assert (rec["report"] > 0) == ("partial" in rec["crc"]), row


def test_every_family_has_a_reference():
    assert set(C.REFS) == set(G.FAMILIES)
    assert all(callable(f) for f in C.REFS.values())


def test_gpu_file_parametrizes_every_row():
    """tests/test_conv_host_fp64_gpu.py: one case per row of G.ROWS, none marked skip / xfail"""
    F64 = _load_test("test_conv_host_fp64_gpu")
    assert [r["id"] for r in F64.CASES] == [r["id"] for r in G.ROWS]
    assert len(set(F64.IDS)) == len(G.ROWS)


def _load_test(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod
