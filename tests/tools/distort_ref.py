"""Restatements of `unet_elastic_field` and `unet_augment_warp_u8`, written from their
specification (the comments in include/unet_hip.h), not from the kernels:

  field_f32 / augment_warp_f32   numpy in fp32 in the specification's operation order, every
                                 operation rounded on its own: what the kernels must reproduce
                                 bit for bit / byte for byte (Gaussian pixel noise apart, as in
                                 augment_ref.py);
  field_f64 / augment_warp_f64   fp64; the image goes through F.grid_sample(align_corners=False,
                                 padding_mode="zeros") on the warped-then-homography grid.  The
                                 Gaussian taps are the record's (fp32 values, used in fp64).

Philox, the pixel noise, the hole and salt / pepper come from augment_ref.py.  Arrays are numpy:
image uint8 [N,H,W,3], mask uint8 [N,H,W] or None, params fp32 [N,24], rng [N,4] integers or
None, warp fp32 [N,64], field [N,H,W,2] or None (zero displacement).

`cases(augment)` draws the records the CPU and the GPU test share."""
import importlib.util
import os

import numpy as np
import torch
import torch.nn.functional as F

_spec = importlib.util.spec_from_file_location(
    "augment_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "augment_ref.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

f32 = np.float32
WARP = 64
MAX_R = 16


# ------------------------------------------------------------------------------------ the field
def _field(warp, rng, N, H, W, dtype):
    out = np.zeros((N, H, W, 2), dtype=dtype)
    for n in range(N):
        w = np.asarray(warp[n], dtype=f32)
        if w[0] != 1:
            continue
        alpha, rad = dtype(w[7]), int(w[8])
        g = w[9:9 + MAX_R + 1].astype(dtype)
        if rng is None:
            noise = np.zeros((H, W, 2), dtype=dtype)
        else:
            words = R.pixel_words(int(rng[n][0]), int(rng[n][1]), H, W, 2)[..., :2]
            u = (words.astype(np.uint64) >> np.uint64(8)).astype(dtype) * dtype(2.0 ** -24)
            noise = dtype(2) * u - dtype(1)
        # noise outside the image is exactly 0
        pad = np.zeros((H, W + 2 * rad, 2), dtype=dtype)
        pad[:, rad:rad + W] = noise
        row = np.zeros((H, W, 2), dtype=dtype)
        for t in range(-rad, rad + 1):
            row = row + g[abs(t)] * pad[:, rad + t:rad + t + W]
        # rows outside the image: the row pass over zeros is 0
        pad = np.zeros((H + 2 * rad, W, 2), dtype=dtype)
        pad[rad:rad + H] = row
        col = np.zeros((H, W, 2), dtype=dtype)
        for t in range(-rad, rad + 1):
            col = col + g[abs(t)] * pad[rad + t:rad + t + H]
        out[n] = alpha * col
        assert out.dtype == dtype
    return out


def field_f32(warp, rng, N, H, W):
    return _field(warp, rng, N, H, W, f32)


def field_f64(warp, rng, N, H, W):
    return _field(warp, rng, N, H, W, np.float64)


def field_bound(warp_n):
    """|field_f32 - field_f64| <= (2 L + 4) 2^-24 alpha with L = 2 R + 1: two dot products of
    length L with non-negative weights summing to 1 over inputs in [-1, 1], each adding at most
    (L + 1) half-ulps of 1 (L products and L sums, the first sum exact), plus the multiply by
    alpha."""
    L = 2 * int(warp_n[8]) + 1
    return (2 * L + 4) * 2.0 ** -24 * float(warp_n[7])


# ------------------------------------------------------------------------------------ the warp
def warp_points(w, H, W, fld, dtype):
    """(xw, yw) [H, W] in `dtype`: the warp stage of one sample, w its record (fp32), fld its
    displacement [H, W, 2] or None."""
    w = np.asarray(w, dtype=f32).astype(dtype)
    xc = np.broadcast_to((np.arange(W, dtype=dtype) + dtype(0.5))[None, :], (H, W))
    yc = np.broadcast_to((np.arange(H, dtype=dtype) + dtype(0.5))[:, None], (H, W))
    mode = int(w[0]) if w[0] in (1, 2, 3) else 0
    if mode == 1:
        dx = fld[..., 0].astype(dtype) if fld is not None else np.zeros((H, W), dtype=dtype)
        dy = fld[..., 1].astype(dtype) if fld is not None else np.zeros((H, W), dtype=dtype)
        xw = ((w[1] * xc + w[2] * yc) + w[3]) + dx
        yw = ((w[4] * xc + w[5] * yc) + w[6]) + dy
    elif mode == 2:
        def axis(c, K, inv, a_at):
            k = np.minimum(np.floor(c * inv).astype(np.int64), int(K) - 1)
            return w[a_at + k] * c + w[a_at + 8 + k]
        xw, yw = axis(xc, w[1], w[2], 8), axis(yc, w[3], w[4], 24)
    elif mode == 3:
        cx, cy, k = w[1], w[2], w[3]
        ex, ey = xc - cx, yc - cy
        xn, yn = ex * w[4], ey * w[5]
        r2 = xn * xn + yn * yn
        kr = k * r2
        f = (dtype(1) + kr) + kr * r2
        xw, yw = cx + ex * f, cy + ey * f
    else:
        xw, yw = xc, yc
    assert xw.dtype == dtype and yw.dtype == dtype
    return xw, yw


def augment_warp_f32(image, mask, params, rng, warp, field=None):
    N, H, W, _ = image.shape
    out = np.empty_like(image)
    mout = np.empty_like(mask) if mask is not None else None
    one, half = f32(1), f32(0.5)
    for n in range(N):
        r = np.asarray(params[n], dtype=f32)
        xw, yw = warp_points(warp[n], H, W, None if field is None else field[n], f32)
        with np.errstate(all="ignore"):
            den = (r[6] * xw + r[7] * yw) + r[8]
            u = ((r[0] * xw + r[1] * yw) + r[2]) / den
            v = ((r[3] * xw + r[4] * yw) + r[5]) / den
            front = den > 0
            fx, fy = u - half, v - half
            x0, y0 = np.floor(fx), np.floor(fy)
            ax, ay = (fx - x0)[..., None], (fy - y0)[..., None]

            def tap(dy, dx):
                ty, tx = y0 + f32(dy), x0 + f32(dx)
                ok = front & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
                yi = np.where(ok, ty, 0).astype(np.int64)
                xi = np.where(ok, tx, 0).astype(np.int64)
                p = image[n][yi, xi].astype(f32)
                p[~ok] = 0
                return p, ok

            (p00, k00), (p01, k01), (p10, k10), (p11, k11) = tap(0, 0), tap(0, 1), tap(1, 0), \
                tap(1, 1)
            top = (one - ax) * p00 + ax * p01
            bot = (one - ax) * p10 + ax * p11
            s = (one - ay) * top + ay * bot
            s[~(k00 | k01 | k10 | k11)] = 0
        hole = R._hole(r, H, W)                     # on the integer output pixel
        s[hole] = r[19]
        a = np.clip(r[9] * s + r[10:13][None, None, :], f32(0), f32(255)).astype(f32)
        if r[13] != 0:
            g = (f32(0.299) * a[..., 0] + f32(0.587) * a[..., 1]) + f32(0.114) * a[..., 2]
            a = np.repeat(g[..., None], 3, -1)
        if rng is not None and r[14] > 0:
            a = a + r[14] * R.normals(R.pixel_words(int(rng[n][0]), int(rng[n][1]), H, W, 0), f32)
        assert a.dtype == f32
        q = np.clip(np.rint(a), 0, 255).astype(np.uint8)
        out[n] = R._salt_pepper(q, None if rng is None else rng[n], H, W)
        if mask is not None:
            with np.errstate(all="ignore"):
                mx, my = np.floor(u), np.floor(v)
                ok = front & (mx >= 0) & (mx < W) & (my >= 0) & (my < H)
            m = mask[n][np.where(ok, my, 0).astype(np.int64), np.where(ok, mx, 0).astype(np.int64)]
            m = np.where(ok, m, np.uint8(r[20]))
            mout[n] = np.where(hole, np.uint8(r[21]), m)
    return out, mout


def augment_warp_f64(image, mask, params, rng, warp, field=None):
    """-> (value before rounding, image uint8, mask uint8 or None, near), as
    augment_ref.augment_f64"""
    N, H, W, _ = image.shape
    val = np.empty(image.shape, dtype=np.float64)
    out = np.empty_like(image)
    mout = np.empty_like(mask) if mask is not None else None
    near = np.empty((N, H, W), dtype=np.float64)
    for n in range(N):
        r = np.asarray(params[n], dtype=f32).astype(np.float64)
        xw, yw = warp_points(warp[n], H, W, None if field is None else field[n], np.float64)
        den = r[6] * xw + r[7] * yw + r[8]
        assert (den > 0).all(), "the fp64 restatement takes validated records only"
        u = (r[0] * xw + r[1] * yw + r[2]) / den
        v = (r[3] * xw + r[4] * yw + r[5]) / den
        near[n] = np.minimum(np.abs(u - np.rint(u)), np.abs(v - np.rint(v)))
        grid = torch.from_numpy(np.stack([2 * u / W - 1, 2 * v / H - 1], -1))[None]
        x = torch.from_numpy(image[n].astype(np.float64)).permute(2, 0, 1)[None]
        s = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros",
                          align_corners=False)[0].permute(1, 2, 0).numpy().copy()
        hole = R._hole(np.asarray(params[n], dtype=f32), H, W)
        s[hole] = r[19]
        a = np.clip(r[9] * s + r[10:13][None, None, :], 0.0, 255.0)
        if r[13] != 0:
            g = 0.299 * a[..., 0] + 0.587 * a[..., 1] + 0.114 * a[..., 2]
            a = np.repeat(g[..., None], 3, -1)
        if rng is not None and r[14] > 0:
            a = a + r[14] * R.normals(R.pixel_words(int(rng[n][0]), int(rng[n][1]), H, W, 0),
                                      np.float64)
        val[n] = a
        q = np.clip(np.rint(a), 0, 255).astype(np.uint8)
        out[n] = R._salt_pepper(q, None if rng is None else rng[n], H, W)
        if mask is not None:
            both = np.stack([mask[n].astype(np.float64), np.ones((H, W))])[None]
            g = F.grid_sample(torch.from_numpy(both), grid, mode="nearest", padding_mode="zeros",
                              align_corners=False)[0].numpy()
            m = np.where(g[1] > 0.5, g[0], r[20]).astype(np.uint8)
            mout[n] = np.where(hole, np.uint8(r[21]), m)
    return val, out, mout, near


# ------------------------------------------------------------------------------------ the cases
SHAPES = [(2, 16, 24), (2, 33, 37), (2, 40, 52)]
SIGMAS = (0.5, 4.0, 6.0)            # R = 2, 12 and the cap of 16
MODES = {1: "elastic", 2: "grid", 3: "optical"}
# (mode, H) -> seed of the records, where the default 1000 mode + H drew a sample that the fp32
# restatement itself does not hold against fp64 within check_against_f64's cap (at 16 x 24 the cap
# of 1 % is 3 pixels: seed 1016 put 4 mask coordinates within 1e-3 px of a cell boundary)
SEEDS = {(1, 16): 1017}


def distort_config(augment, mode, shape, sigma):
    """One member of the group with probability 1, on top of the "perspective" geometry of
    augment_ref.record_configs.  alpha is scaled to the shape (3 px at 16 x 24, 8 px at the
    others) so that most of a sample stays inside the image."""
    _, H, W = shape
    base = vars(R.record_configs(augment)["perspective"])
    alpha = 3.0 if H == 16 else 8.0
    member = {1: dict(elastic_prob=1.0, elastic_alpha=alpha, elastic_sigma=sigma,
                      elastic_alpha_affine=0.04 * min(H, W)),
              2: dict(grid_distortion_prob=1.0, grid_num_steps=5, grid_distort_limit=0.3),
              3: dict(optical_distortion_prob=1.0, optical_distort_limit=0.2,
                      optical_shift_limit=0.15)}[mode]
    return augment.AugmentConfig(**{**base, "distort_group_prob": 1.0, **member})


def cases(augment, mode, shape):
    """Three batches of N = 2 records (six records) of one mode at one shape, each composed with a
    random perspective record: [(params, rng, warp)] as CPU tensors.  The elastic batches take
    the three sigmas in turn.  The records are validated."""
    N, H, W = shape
    gen = torch.Generator().manual_seed(SEEDS.get((mode, H), 1000 * mode + H))
    out = []
    for b in range(3):
        cfg = distort_config(augment, mode, shape, SIGMAS[b])
        p, r = augment.sample_params(cfg, N, H, W, gen)
        w = augment.sample_warp(cfg, N, H, W, gen)
        augment.validate_warp(w, p, H, W)
        assert (w[:, 0] == mode).all()
        out.append((p, r, w))
    return out
