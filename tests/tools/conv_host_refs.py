"""The float64 reference of every row of tests/tools/make_conv_host_gpu_table.py: one function per
family of G.FAMILIES, taking the row and the named tensors of G.build_row and returning the
outputs of the call as float64 tensors in the layout the library writes (NHWC).  Built on
fp64_layer_refs.py (R); the device is the tensors'.  Nothing here calls the library, so
tests/test_conv_host_refs_cpu.py checks these functions on the CPU against independent nine-tap
evaluations, and tests/test_conv_host_fp64_gpu.py holds the library to them.

Operands are rounded as each operand mode's loaders round them (`mode_of`):
  f32   unet_x and unet_x_bf16x3: the fp32 operands exactly (R.act64 unrounded);
  core  unet_x_bf16 (bf16 matrix cores on fp32 tensors): operands and weights rounded to bf16, the
        RGB stem unrounded;
  b16   bf16 tensors: an activated operand is evaluated in fp32 and rounded to bf16, the weights
        are bf16(w), an up-sampled operand is blended from the activated fp32 taps and rounded
        once, the RGB stem stays fp32, an accumulate row adds its bf16 base.
Weights come packed as the entry points take them: wf[tap][co][ci], wd[tap][ci][co], tap = 3 ky +
kx (include/unet_hip.h).

The per-tile side outputs are compared merged per image - which pixels make up tile t differs
from kernel to kernel and the consumers only sum: `merge_tiles` (the fused forward's (mean, M2)
pairs -> mean and variance per (n, c)) and `sum_tiles` (the BSTATS (S1, S2) pairs -> sums per
(n, c)), against `y_stats` of the fp64 y and `bstats64` of the fp64 gradient.

drop = (image, row) evaluates a reference with that row zeroed (a row of the assembled operand of
a forward, of dy for a gradient, of y for a finalize without tiles): the check of the check."""
import importlib.util
import os

import torch
import torch.nn.functional as F

_spec = importlib.util.spec_from_file_location("fp64_layer_refs", os.path.join(
    os.path.dirname(os.path.abspath(__file__)), "fp64_layer_refs.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

BF = torch.bfloat16
SLOPE, EPS = R.SLOPE, R.EPS          # what build_row passes (0.01, 1e-5)


def mode_of(fn, b16_exports):
    """"b16" (bf16 tensors), "core" (bf16 matrix cores on fp32 tensors) or "f32" (fp32 tensors
    at fp32 accuracy: the plain and the split-bf16 entries) of the export `fn`."""
    if fn in b16_exports:
        return "b16"
    return "core" if fn.endswith("_bf16") else "f32"


# --------------------------------------------------------------------------- weights
def oihw_fwd(wf):
    """wf[k*k][Cout][Cin] -> float64 OIHW [Cout][Cin][k][k]"""
    k = 3 if wf.shape[0] == 9 else 1
    return wf.double().permute(1, 2, 0).reshape(wf.shape[1], wf.shape[2], k, k)


def oihw_dgrad(wd, ci_offset, Ccols):
    """wd[k*k][Cin_total][Cout] -> float64 OIHW [Cout][Ccols][k][k] of the input-channel slice"""
    k = 3 if wd.shape[0] == 9 else 1
    w = wd.double().permute(2, 1, 0).reshape(wd.shape[2], wd.shape[1], k, k)
    return w[:, ci_offset:ci_offset + Ccols].contiguous()


def _w(w, mode, stem=False):
    """the weight as the mode's kernels contract it"""
    return w.to(BF).float() if mode in ("core", "b16") and not stem else w


# --------------------------------------------------------------------------- pieces
def conv64(a, w, b, stride):
    """a NCHW float64, w OIHW float64 (3x3 pad 1 or 1x1) -> NCHW, one image at a time"""
    if w.shape[2] == 3:
        return R.ref_conv(a, w, b, stride)
    return torch.cat([F.conv2d(a[i:i + 1].contiguous(), w, b) for i in range(a.shape[0])])


def dgrad64(dy, w, stride, H, W):
    """dy NCHW float64, w OIHW slice -> dx NCHW [n, Ccols, H, W]"""
    if w.shape[2] == 3:
        return R.ref_dgrad(dy, w, stride, H, W)
    return torch.cat([torch.einsum("ohw,oc->chw", dy[i], w[:, :, 0, 0])[None]
                      for i in range(dy.shape[0])])


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _dropped(a, drop):
    if drop is not None:
        a = a.clone()
        a[drop[0], :, drop[1], :] = 0
    return a


def normalize_u8(image, mean3, std3):
    """uint8 NHWC image -> NCHW float64 (x / 255 - mean3) / std3"""
    x = (image.double() / 255.0 - mean3.double()) / std3.double()
    return x.permute(0, 3, 1, 2)


def source64(x, al, be, mode):
    """One source of a fused forward -> NCHW float64 operand as the mode's loader forms it: plain
    (al is None) or lrelu(x alpha + beta); on bf16 tensors the activation is evaluated in fp32 and
    rounded to bf16 (an fp32 source of that mode - the RGB image - is plain)."""
    if al is None:
        return R.nchw64(x)
    return R.act64(x, al, be, rounded=(mode == "b16"))


def upsampled64(low, al, be, mode):
    """The bilinear 2x up-sampling of the (activated) low-resolution source -> NCHW float64; on
    bf16 tensors blended from the activated fp32 taps and rounded once."""
    if mode != "b16":
        return R.upsample64(source64(low, al, be, mode))
    a = low.float() if al is None else F.leaky_relu(
        low.float() * al[:, None, None, :] + be[:, None, None, :], SLOPE)
    a = a.permute(0, 3, 1, 2)
    up = torch.cat([F.interpolate(a[i:i + 1], scale_factor=2, mode="bilinear", align_corners=False)
                    for i in range(a.shape[0])])
    return up.to(BF).double()


def y_stats(y):
    """y NCHW float64 -> (mean, biased variance) [n, c]"""
    return y.mean(dim=(2, 3)), y.var(dim=(2, 3), unbiased=False)


def merge_tiles(pairs, count):
    """(mean, M2) pairs [n, tiles, c, 2] of `count` samples each -> (mean, biased variance) [n, c]
    in float64 (Chan's merge at equal counts; M2 below zero counts as zero)."""
    p = pairs.double()
    mean_t, m2_t = p[..., 0], p[..., 1].clamp_min(0)
    tiles = p.shape[1]
    mean = mean_t.mean(1)
    m2 = m2_t.sum(1) + count * ((mean_t - mean[:, None]) ** 2).sum(1)
    return mean, m2 / (tiles * count)


def tile_pairs(raw, N, C):
    """the bytes call_row cuts (stats / partial) -> float pairs [N, tiles, C, 2]"""
    return raw.view(torch.float32).view(N, -1, C, 2)


def sum_tiles(pairs):
    """(S1, S2) pairs [n, tiles, c, 2] -> (S1, S2) [n, c] in float64"""
    s = pairs.double().sum(1)
    return s[..., 0], s[..., 1]


def bstats64(g, y, mean, rstd, gamma, beta, mask, slope=SLOPE):
    """The two reductions of the InstanceNorm + LeakyReLU + dropout backward of the layer whose
    raw output is y, from its final gradient g (both NCHW float64), as csrc/instnorm.hip forms
    them: xhat = (y - mean) rstd, z = gamma xhat + beta (= y A + B0, A = gamma rstd, B0 = beta -
    mean A), gz = g mask (z > 0 ? 1 : slope) -> S1 = sum gz, S2 = sum gz xhat per (n, c).
    mean, rstd, mask [n, c] (mask may be None), gamma, beta [c]."""
    mu, rs = mean.double()[:, :, None, None], rstd.double()[:, :, None, None]
    A = gamma.double()[None, :, None, None] * rs
    z = y * A + (beta.double()[None, :, None, None] - mu * A)
    gz = g * torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))
    if mask is not None:
        gz = gz * mask.double()[:, :, None, None]
    return gz.sum(dim=(2, 3)), (gz * (y - mu) * rs).sum(dim=(2, 3))


def finalize64(mean, var, gamma, beta, mask, eps=EPS):
    """mean, rstd, alpha = gamma rstd mask, beta_out = (beta - mean gamma rstd) mask, as
    step_kernel_harness.fused_stats states them; mean, var [n, c] float64."""
    rstd = 1.0 / torch.sqrt(var + eps)
    al = gamma.double()[None] * rstd
    mk = 1.0 if mask is None else mask.double()
    return dict(mean=mean, rstd=rstd, alpha=al * mk, beta=(beta.double()[None] - mean * al) * mk)


def _with_stats(y):
    """the outputs of a forward with the statistics epilogue: y (NHWC) and the statistics of y"""
    mean, var = y_stats(y)
    return dict(y=nhwc(y), stat_mean=mean, stat_var=var)


def _with_bstats(row, t, g, out):
    if "by" in t:
        s1, s2 = bstats64(g, R.nchw64(t["by"]), t["mean"], t["rstd"], t["gamma"], t["beta"],
                          t.get("mask"))
        out.update(S1=s1, S2=s2)
    return out


# --------------------------------------------------------------------------- one per family
def ref_fwd(row, t, mode, drop=None):
    """unet_conv3x3_fwd[_bf16 | _bf16x3] and unet_conv1x1_fwd: y = conv(cat(x0, x1)) + bias"""
    stem = row["C0"] == 3
    xs = [t["x0"]] + ([t["x1"]] if "x1" in t else [])
    a = torch.cat([R.nchw64(x if mode == "f32" or stem else x.to(BF)) for x in xs], 1)
    w = oihw_fwd(_w(t["wf"], mode, stem))
    return dict(y=nhwc(conv64(_dropped(a, drop), w, t["bias"].double(), row.get("stride", 1))))


def ref_dgrad_rows(row, t, mode, drop=None):
    """unet_conv3x3_bwd_data[_bs][_bf16 | _bf16x3 | _b16[_wb]] and unet_conv1x1_bwd_data:
    dx (+)= the data gradient of dy for the input channels [ci_offset, ci_offset + Ccols), and the
    BSTATS sums of the layer the row's unet_bwd_stats describes"""
    dy = t["dy"].to(BF) if mode == "core" else t["dy"]
    w = oihw_dgrad(_w(t["wd"], mode), row.get("ci_offset", 0), row["Ccols"])
    g = dgrad64(_dropped(R.nchw64(dy), drop), w, row.get("stride", 1), row["H"], row["W"])
    if "base" in t:
        g = g + R.nchw64(t["base"])
    return _with_bstats(row, t, g, dict(dx=nhwc(g)))


def ref_in(row, t, mode, drop=None):
    """unet_conv_in_fwd[_bf16x3 | _b16[_wb]]: y = conv(cat(act(s0), act(s1))) + bias (3x3 at
    stride 1 / 2, or 1x1) and the statistics of y"""
    stem = row["C0"] == 3
    a = source64(t["s0"], t.get("a0"), t.get("b0"), mode)
    if "s1" in t:
        a = torch.cat([a, source64(t["s1"], t.get("a1"), t.get("b1"), mode)], 1)
    w = oihw_fwd(_w(t["w"], mode, stem))
    return _with_stats(conv64(_dropped(a, drop), w, t["bias"].double(), row.get("stride", 1)))


def ref_upf(row, t, mode, drop=None):
    """unet_conv_up_in_fwd[_b16]: y = conv3x3(cat(upsample2x(act(low)), act(skip))) + bias"""
    a = upsampled64(t["s0"], t.get("a0"), t.get("b0"), mode)
    if "s1" in t:
        a = torch.cat([a, source64(t["s1"], t.get("a1"), t.get("b1"), mode)], 1)
    w = oihw_fwd(_w(t["w"], mode))
    return _with_stats(conv64(_dropped(a, drop), w, t["bias"].double(), 1))


def ref_upb(row, t, mode, drop=None):
    """unet_conv3x3_up_bwd_data[_bs][_b16[_wb]]: g[q][ci] (+)= sum_{t, co} D[q][t Cout + co]
    wd[t][ci_offset + ci][co] over the low-resolution pixels q, and the BSTATS sums"""
    D = t["dy"].double()
    if drop is not None:
        D = D.clone()
        D[drop[0], drop[1]] = 0
    w = oihw_dgrad(_w(t["wd"], mode), row.get("ci_offset", 0), row["Ccols"])
    g = R.ref_up_dgrad(D, w)
    if "base" in t:
        g = g + t["base"].double()
    return _with_bstats(row, t, g.permute(0, 3, 1, 2), dict(dx=g))


def ref_u8(row, t, mode, drop=None):
    """unet_stem_u8_fwd[_b16]: the RGB stem on (x / 255 - mean3) / std3, zero padding after the
    normalisation, fp32 arithmetic in every mode"""
    a = normalize_u8(t["image"], t["mean3"], t["std3"])
    return _with_stats(conv64(_dropped(a, drop), oihw_fwd(t["wf"]), t["bias"].double(), 1))


def ref_fin(row, t, mode, drop=None):
    """unet_conv_in_stats_finalize[_b16]: the statistics of y [N, H W, Cout] - merged from the
    given per-tile (mean, M2) pairs when stats_px > 0, of y itself when stats_px = 0 - and the
    activation coefficients of the layer"""
    if row["stats_px"] > 0:
        mean, var = merge_tiles(t["tiles"], row["stats_px"])
    else:
        y = t["y"].double()
        if drop is not None:
            y = y.clone()
            y[drop[0], drop[1] * row["W"]:(drop[1] + 1) * row["W"]] = 0
        mean, var = y.mean(1), y.var(1, unbiased=False)
    return finalize64(mean, var, t["gamma"], t["beta"], t.get("mask"))


def ref_c1x1(row, t, mode, drop=None):
    """unet_conv1x1_fwd / unet_conv1x1_bwd_data: the plain forward / data gradient with one tap"""
    return (ref_fwd if "x0" in t else ref_dgrad_rows)(row, t, mode, drop)


REFS = {"fwd": ref_fwd, "bwd": ref_dgrad_rows, "bs": ref_dgrad_rows, "bs2": ref_dgrad_rows,
        "c1x1": ref_c1x1, "in": ref_in, "inp": ref_in, "fin": ref_fin, "upb": ref_upb,
        "upf": ref_upf, "u8": ref_u8}
