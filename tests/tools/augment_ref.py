"""Two independent restatements of `unet_augment_u8`, written from its specification (the
comment in include/unet_hip.h / DESIGN 12), not from the kernel:

  augment_f32   numpy in fp32 with the specification's operation order, every operation rounded
                on its own: what the kernel must reproduce byte for byte (Gaussian noise apart,
                whose log / sin / cos come from different libraries);
  augment_f64   fp64 through torch.nn.functional.grid_sample (align_corners=False,
                padding_mode="zeros"; bilinear for the image, nearest for the mask), returning
                the value BEFORE rounding and the distance of every mask source coordinate to
                a cell boundary, so a test can tell a rounding tie from an error.

plus Philox4x32-10 (`philox4x32`) with the published known-answer vectors (`PHILOX_KAT`).
Arrays are numpy: image uint8 [N,H,W,3], mask uint8 [N,H,W] or None, params fp32 [N,24],
rng [N,4] integers in 0 .. 2^32 - 1 or None (all noise off)."""
import numpy as np
import torch
import torch.nn.functional as F

f32 = np.float32
M32 = np.uint64(0xFFFFFFFF)

# (counter, key, output) of Random123's kat_vectors for philox4x32-10
PHILOX_KAT = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def philox4x32(counter, key, rounds=10):
    """counter: four uint arrays (broadcastable), key: two -> uint32 array [..., 4]."""
    c = [np.asarray(x, dtype=np.uint64) & M32 for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF))
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    s = np.uint64(32)
    for _ in range(rounds):
        p0, p1 = m0 * c[0], m1 * c[2]           # 32 x 32 -> 64 bits, no overflow
        c = [(p1 >> s) ^ c[1] ^ k0, p1 & M32, (p0 >> s) ^ c[3] ^ k1, p0 & M32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack(c, -1).astype(np.uint32)


def pixel_words(seed_lo, seed_hi, H, W, stream):
    """uint32 [H, W, 4]: the words of every pixel of one sample (counter = pixel index i W + j)."""
    pix = np.arange(H * W, dtype=np.uint64).reshape(H, W)
    return philox4x32((pix & M32, pix >> np.uint64(32), stream, 0), (seed_lo, seed_hi))


def normals(words, dtype):
    """[H, W, 3]: Box-Muller on (w0, w1) -> cos, sin and on (w2, w3) -> cos, in `dtype`."""
    w = words.astype(np.uint64)
    out = []
    for a, b, fn in ((0, 1, np.cos), (0, 1, np.sin), (2, 3, np.cos)):
        u1 = ((w[..., a] >> np.uint64(8)) + np.uint64(1)).astype(dtype) * dtype(2.0 ** -24)
        u2 = (w[..., b] >> np.uint64(8)).astype(dtype) * dtype(2.0 ** -24)
        r = np.sqrt(dtype(-2.0) * np.log(u1))
        out.append(r * fn(dtype(2.0 * np.pi) * u2))
    return np.stack(out, -1).astype(dtype)


def _salt_pepper(q, rng_n, H, W):
    if rng_n is None or (int(rng_n[2]) == 0 and int(rng_n[3]) == 0):
        return q
    word = pixel_words(int(rng_n[0]), int(rng_n[1]), H, W, 1)[..., 0].astype(np.uint64)
    pepper = word < np.uint64(int(rng_n[2]))
    salt = ~pepper & (int(rng_n[3]) != 0) & (word >= np.uint64((1 << 32) - int(rng_n[3])))
    q = q.copy()
    q[pepper] = 0
    q[salt] = 255
    return q


def _hole(r, H, W):
    jj = np.arange(W, dtype=f32)[None, :]
    ii = np.arange(H, dtype=f32)[:, None]
    return (jj >= r[15]) & (jj < r[17]) & (ii >= r[16]) & (ii < r[18])


def augment_f32(image, mask, params, rng=None):
    N, H, W, _ = image.shape
    out = np.empty_like(image)
    mout = np.empty_like(mask) if mask is not None else None
    one, half = f32(1), f32(0.5)
    for n in range(N):
        r = np.asarray(params[n], dtype=f32)
        xc = (np.arange(W, dtype=f32) + half)[None, :]
        yc = (np.arange(H, dtype=f32) + half)[:, None]
        with np.errstate(all="ignore"):
            den = (r[6] * xc + r[7] * yc) + r[8]
            u = ((r[0] * xc + r[1] * yc) + r[2]) / den
            v = ((r[3] * xc + r[4] * yc) + r[5]) / den
            front = den > 0
            fx, fy = u - half, v - half
            x0, y0 = np.floor(fx), np.floor(fy)
            ax, ay = (fx - x0)[..., None], (fy - y0)[..., None]

            def tap(dy, dx):
                # range tests in float, before any conversion to an integer
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
            s[~(k00 | k01 | k10 | k11)] = 0         # no tap inside: exactly 0
        hole = _hole(r, H, W)
        s[hole] = r[19]
        a = np.clip(r[9] * s + r[10:13][None, None, :], f32(0), f32(255)).astype(f32)
        if r[13] != 0:
            g = (f32(0.299) * a[..., 0] + f32(0.587) * a[..., 1]) + f32(0.114) * a[..., 2]
            a = np.repeat(g[..., None], 3, -1)
        if rng is not None and r[14] > 0:
            z = normals(pixel_words(int(rng[n][0]), int(rng[n][1]), H, W, 0), f32)
            a = a + r[14] * z
        assert a.dtype == f32
        q = np.clip(np.rint(a), 0, 255).astype(np.uint8)
        out[n] = _salt_pepper(q, None if rng is None else rng[n], H, W)
        if mask is not None:
            with np.errstate(all="ignore"):
                mx, my = np.floor(u), np.floor(v)
                ok = front & (mx >= 0) & (mx < W) & (my >= 0) & (my < H)
            m = mask[n][np.where(ok, my, 0).astype(np.int64), np.where(ok, mx, 0).astype(np.int64)]
            m = np.where(ok, m, np.uint8(r[20]))
            mout[n] = np.where(hole, np.uint8(r[21]), m)
    return out, mout


def augment_f64(image, mask, params, rng=None):
    """-> (value before rounding fp64 [N,H,W,3], image uint8 (rounded, salt / pepper applied),
    mask uint8 or None, near fp64 [N,H,W]: distance of the mask's source coordinate to the
    nearest cell boundary, in pixels)."""
    N, H, W, _ = image.shape
    val = np.empty(image.shape, dtype=np.float64)
    out = np.empty_like(image)
    mout = np.empty_like(mask) if mask is not None else None
    near = np.empty((N, H, W), dtype=np.float64)
    for n in range(N):
        r = np.asarray(params[n], dtype=f32).astype(np.float64)
        xc = (np.arange(W) + 0.5)[None, :]
        yc = (np.arange(H) + 0.5)[:, None]
        den = r[6] * xc + r[7] * yc + r[8]
        assert (den > 0).all(), "the fp64 restatement takes validated records only"
        u = (r[0] * xc + r[1] * yc + r[2]) / den
        v = (r[3] * xc + r[4] * yc + r[5]) / den
        near[n] = np.minimum(np.abs(u - np.rint(u)), np.abs(v - np.rint(v)))
        grid = torch.from_numpy(np.stack([2 * u / W - 1, 2 * v / H - 1], -1))[None]
        x = torch.from_numpy(image[n].astype(np.float64)).permute(2, 0, 1)[None]
        s = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros",
                          align_corners=False)[0].permute(1, 2, 0).numpy().copy()
        hole = _hole(np.asarray(params[n], dtype=f32), H, W)
        s[hole] = r[19]
        a = np.clip(r[9] * s + r[10:13][None, None, :], 0.0, 255.0)
        if r[13] != 0:
            g = 0.299 * a[..., 0] + 0.587 * a[..., 1] + 0.114 * a[..., 2]
            a = np.repeat(g[..., None], 3, -1)
        if rng is not None and r[14] > 0:
            a = a + r[14] * normals(pixel_words(int(rng[n][0]), int(rng[n][1]), H, W, 0),
                                    np.float64)
        val[n] = a
        q = np.clip(np.rint(a), 0, 255).astype(np.uint8)
        out[n] = _salt_pepper(q, None if rng is None else rng[n], H, W)
        if mask is not None:
            both = np.stack([mask[n].astype(np.float64), np.ones((H, W))])[None]
            g = F.grid_sample(torch.from_numpy(both), grid, mode="nearest", padding_mode="zeros",
                              align_corners=False)[0].numpy()
            m = np.where(g[1] > 0.5, g[0], r[20]).astype(np.uint8)
            mout[n] = np.where(hole, np.uint8(r[21]), m)
    return val, out, mout, near


def check_against_f64(img, msk, val, m64, near, max_left_out=0.01):
    """The bounds that hold a result (the kernel's, or the fp32 restatement's) against fp64:
    image within 1 level, every differing pixel's fp64 value within 0.05 of a half-integer; mask
    equal except where the source coordinate lies within 1e-3 px of a cell boundary, at most
    `max_left_out` of a sample's pixels left out this way.  Returns the measured figures."""
    q64 = np.clip(np.rint(val), 0, 255)
    d = np.abs(img.astype(np.float64) - q64)
    tie = np.abs(val - np.floor(val) - 0.5)
    fig = {"max_level_diff": float(d.max()), "share_differing": float((d > 0).mean()),
           "max_tie_distance": float(tie[d > 0].max()) if (d > 0).any() else 0.0}
    assert d.max() <= 1, fig
    assert ((d == 0) | (tie < 0.05)).all(), fig
    if msk is not None:
        close = near <= 1e-3
        fig["mask_left_out"] = float(close.reshape(close.shape[0], -1).mean(1).max())
        fig["mask_mismatch_far"] = int(((msk != m64) & ~close).sum())
        assert fig["mask_mismatch_far"] == 0, fig
        assert fig["mask_left_out"] <= max_left_out, fig
    return fig


def record_configs(augment):
    """The two configurations the tests draw random geometry from: "affine" (flip, shift /
    scale / rotate, crop) and "perspective" (the same with a four-corner displacement on top)."""
    affine = augment.AugmentConfig(
        horizontal_flip_prob=0.5, shift_scale_rotate_prob=1.0, shift_limit=(-0.1, 0.1),
        scale_limit=(-0.15, 0.15), rotate_limit=(-15.0, 15.0), crop_prob=0.5,
        crop_scale=(0.8, 1.0), crop_ratio=(0.9, 1.1), mask_border_value=7.0)
    persp = augment.AugmentConfig(**{**vars(affine), "perspective_prob": 1.0,
                                     "perspective_scale": (0.05, 0.1)})
    return {"affine": affine, "perspective": persp}


def random_batch(N, H, W, seed):
    g = np.random.default_rng(seed)
    image = g.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    mask = g.choice(np.array([0, 1, 2, 255], dtype=np.uint8), (N, H, W))
    return image, mask
