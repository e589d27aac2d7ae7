"""Restatements of `unet_augment_post_u8`, written from its specification (the comment in
include/unet_hip.h), not from the kernels:

  post_f32   numpy in fp32 in the specification's operation order, every operation rounded on its
             own: what the kernels must reproduce byte for byte;
  post_f64   the same chain in fp64 (its own bytes from stage to stage).

The chain is a sequence of arithmetic SEGMENTS, each ending in a conversion to an integer (a byte,
a luma level, a clip limit, a LUT entry), and integers are what one segment hands to the next.
`check_against_f64` therefore holds every segment on its own: the fp64 value of the segment,
computed FROM THE INTEGERS THE fp32 CHAIN HANDED IT, against the integer the fp32 chain (or, for
the last stage, a kernel) made of it.  An integer may differ from the rounded fp64 value by at
most 1, and only where the fp64 value lies within the segment's bound of a rounding tie (x.5) -
or, for the clip limit, of an integer, its `floor` boundary.  The other floors (the hue wrap, the
hue sector, the CLAHE cell) sit where the value is continuous and need no allowance.

The bounds, with u = 2^-24 (half an ulp of 1; an fp32 operation errs by at most u times its
result).  They are derived from the operation counts below, not from what any code gives; the
fp64 chain's own error is 2^-29 of these and is covered by counting exact operations as rounded.

  HSV       M = 180 + |dh| bounds every hue value.  The hue goes through 8 roundings (the
            division by d, the product by 30, the sector offset, + 180, + dh, the product and
            the difference of the wrap, the division by 30; the clamp below 180 moves a value by
            at most 256 u, less than one of these), so hp errs by 8 u M / 30 and f = hp - k by
            e_f = 8 u M / 30 + u.  S' errs by e_S = 2 (255 u) (division, + ds), V' by
            e_V = 255 u (+ dv), c = (V' S') / 255 by e_c = e_V + e_S + 2 (255 u).  A channel is
            V' - c g with g in {0, f, 1 - f}: e_V + e_c + 255 (e_f + u) + 2 (255 u).
  luma      3 constants, 3 products, 2 sums of values <= 255:            8 (255 u).
  equalize  scale (1 division), the two conversions, 1 product:         4 (255 u).
  clip      t = (clip_limit area) / 256: one product (the division by 256 is exact): an integer
            boundary within 2 u t decides differently.
  CLAHE LUT 255 / area, the two conversions, 1 product:                 4 (255 u).
  CLAHE interpolation  fx = j (1 / tw) - 0.5 < 8: three roundings, e_a = 24 u for ax (fx - x1 is
            exact).  top = (1-ax) L1 + ax L2: 255 e_a from ax, u 255 from 1 - ax, 255 u for the
            two products together, 255 u for the sum: 27 (255 u); s the same again on top:
            54 (255 u).
  blur      L = 2R+1 taps: a pass of non-negative weights summing to 1 (within 1e-6) over values
            <= 255 adds (L + 1) (255 u) (the products together 255 u, each of L sums 255 u);
            separable: 2 (L + 1) (255 u); dense: (L L + 1) (255 u).

Arrays are numpy: image uint8 [N,H,W,3], post fp32 [N,64], rng [N,4] integers or None."""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location(
    "augment_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "augment_ref.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

f32 = np.float32
f64 = np.float64
U = 2.0 ** -24
POST = 64


def byte(v):
    """clamp(rint(v), 0, 255) with fmin / fmax (a NaN becomes 0) -> int64"""
    return np.fmin(np.fmax(np.rint(v), 0), 255).astype(np.int64)


# ------------------------------------------------------------------------------------ decoding
def modes(rec, H, W):
    """(hsv on, histogram op, (ty, tx), blur mode, R) of one record as the device decodes it"""
    rec = np.asarray(rec, dtype=f32)
    hsv = bool(rec[0] == 1)
    op, ty, tx = 0, 1, 1
    if rec[4] == 1:
        op = 1
    elif rec[4] == 2:
        fy, fx = rec[6], rec[7]
        if 1 <= fy <= 8 and 1 <= fx <= 8 and fy == np.floor(fy) and fx == np.floor(fx) and \
                H % int(fy) == 0 and W % int(fx) == 0:
            op, ty, tx = 2, int(fy), int(fx)
    bm = 1 if rec[8] == 1 else 2 if rec[8] == 2 else 0
    Rr = 0
    if bm:
        Rr = int(np.fmin(np.fmax(rec[9], f32(1)), f32(4 if bm == 1 else 3)))
    return hsv, op, (ty, tx), bm, Rr


# ------------------------------------------------------------------------------------ segments
def hsv_values(q, rec, dtype):
    """uint8 [H,W,3] -> the three channels before rounding, in `dtype`"""
    d_ = dtype
    r, g, b = (q[..., c].astype(d_) for c in range(3))
    dh, ds, dv = d_(rec[1]), d_(rec[2]), d_(rec[3])
    V, m = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    d = V - m
    with np.errstate(all="ignore"):
        S = np.where(V == 0, d_(0), (d_(255) * d) / np.where(V == 0, d_(1), V))
        dd = np.where(d == 0, d_(1), d)
        hr = d_(30) * ((g - b) / dd)
        hg = d_(60) + d_(30) * ((b - r) / dd)
        hb = d_(120) + d_(30) * ((r - g) / dd)
        h = np.where(d == 0, d_(0), np.where(V == r, hr, np.where(V == g, hg, hb)))
        h = np.where(h < 0, h + d_(180), h)
        h2 = h + dh
        h2 = h2 - d_(180) * np.floor(h2 / d_(180))
        h2 = np.fmin(np.fmax(h2, d_(0)), np.nextafter(d_(180), d_(0)))
        S2 = np.fmin(np.fmax(S + ds, d_(0)), d_(255))
        V2 = np.fmin(np.fmax(V + dv, d_(0)), d_(255))
        c = (V2 * S2) / d_(255)
        hp = h2 / d_(30)
        k = np.fmin(np.fmax(np.floor(hp), d_(0)), d_(5))
        f = hp - k
        P, Q, T = V2 - c, V2 - c * f, V2 - c * (d_(1) - f)
    table = ((V2, T, P), (Q, V2, P), (P, V2, T), (P, Q, V2), (T, P, V2), (V2, P, Q))
    out = np.zeros(q.shape, dtype=d_)
    for s, trio in enumerate(table):
        for ch in range(3):
            out[..., ch] = np.where(k == s, trio[ch], out[..., ch])
    assert out.dtype == d_
    return out


def hsv_bound(rec):
    M = 180.0 + abs(float(rec[1]))
    e_f = 8 * U * M / 30 + U
    e_S, e_V = 2 * 255 * U, 255 * U
    e_c = e_V + e_S + 2 * 255 * U
    return e_V + e_c + 255 * (e_f + U) + 2 * 255 * U


def luma_values(q, dtype):
    v = (dtype(0.299) * q[..., 0].astype(dtype) + dtype(0.587) * q[..., 1].astype(dtype)) + \
        dtype(0.114) * q[..., 2].astype(dtype)
    assert v.dtype == dtype
    return v


LUMA_BOUND = 8 * 255 * U
EQUALIZE_BOUND = 4 * 255 * U
CLAHE_LUT_BOUND = 4 * 255 * U
CLAHE_INTERP_BOUND = 54 * 255 * U


def equalize_lut_values(hist, dtype):
    """256 counts of one channel -> (values before rounding [256] in dtype, or None when the
    channel has one value only: it is unchanged)"""
    hist = np.asarray(hist, dtype=np.int64)
    total = int(hist.sum())
    i0 = int(np.nonzero(hist)[0][0])
    if hist[i0] == total:
        return None
    scale = dtype(255) / dtype(total - int(hist[i0]))
    run = np.cumsum(hist) - hist[i0]
    run[:i0 + 1] = 0
    v = run.astype(dtype) * scale
    assert v.dtype == dtype
    return v


def lut_of(values):
    return np.minimum(np.rint(values), 255).astype(np.int64)


def clahe_limit_value(rec, area, dtype):
    """t before the floor: (clip_limit area) / 256"""
    return (dtype(rec[5]) * dtype(area)) / dtype(256)


def clahe_limit(t, area, dtype):
    t = np.fmax(np.floor(t), dtype(1))
    return area if t >= dtype(area) else int(t)


def clahe_redistribute(hist, climit):
    """integers only: clip at climit, spread the excess (the specification's rule)"""
    h = np.asarray(hist, dtype=np.int64).copy()
    excess = int(np.maximum(h - climit, 0).sum())
    h = np.minimum(h, climit)
    batch = excess // 256
    resid = excess - 256 * batch
    h += batch
    if resid > 0:
        step = max(256 // resid, 1)
        i = np.arange(256)
        h[(i % step == 0) & (i // step < resid)] += 1
    return h


def clahe_lut_values(hist, climit, area, dtype):
    cdf = np.cumsum(clahe_redistribute(hist, climit))
    v = cdf.astype(dtype) * (dtype(255) / dtype(area))
    assert v.dtype == dtype
    return v


def clahe_interp_values(Y, luts, ty, tx, dtype):
    """Y int [H,W], luts int [ty,tx,256] -> s [H,W] before rounding"""
    H, W = Y.shape
    th, tw = H // ty, W // tx

    def axis(size, t, cells):
        fx = np.arange(size).astype(dtype) * (dtype(1) / dtype(t)) - dtype(0.5)
        x1 = np.floor(fx)
        a = fx - x1
        lo = np.fmin(np.fmax(x1, dtype(0)), dtype(cells - 1)).astype(np.int64)
        hi = np.fmin(np.fmax(x1 + dtype(1), dtype(0)), dtype(cells - 1)).astype(np.int64)
        return a, lo, hi

    ax, x1, x2 = axis(W, tw, tx)
    ay, y1, y2 = axis(H, th, ty)
    ax, ay = ax[None, :], ay[:, None]
    L = luts.astype(dtype)
    one = dtype(1)
    top = (one - ax) * L[y1[:, None], x1[None, :], Y] + ax * L[y1[:, None], x2[None, :], Y]
    bot = (one - ax) * L[y2[:, None], x1[None, :], Y] + ax * L[y2[:, None], x2[None, :], Y]
    s = (one - ay) * top + ay * bot
    assert s.dtype == dtype
    return s


def _reflect(idx, size):
    idx = np.where(idx < 0, -idx, idx)
    idx = np.where(idx > size - 1, 2 * (size - 1) - idx, idx)
    return np.clip(idx, 0, size - 1)


def blur_values(B, rec, bm, Rr, dtype):
    """bytes [H,W,3] -> the blurred value before rounding, in `dtype`"""
    H, W, _ = B.shape
    x = B.astype(dtype)
    ii, jj = np.arange(H), np.arange(W)
    if bm == 1:
        g = np.asarray(rec[10:15], dtype=f32).astype(dtype)
        row = np.zeros(x.shape, dtype=dtype)
        for t in range(-Rr, Rr + 1):
            row = row + g[abs(t)] * x[:, _reflect(jj + t, W)]
        out = np.zeros(x.shape, dtype=dtype)
        for t in range(-Rr, Rr + 1):
            out = out + g[abs(t)] * row[_reflect(ii + t, H)]
    else:
        L = 2 * Rr + 1
        w = np.asarray(rec[15:15 + L * L], dtype=f32).astype(dtype).reshape(L, L)
        out = np.zeros(x.shape, dtype=dtype)
        for dy in range(-Rr, Rr + 1):
            rows = x[_reflect(ii + dy, H)]
            for dx in range(-Rr, Rr + 1):
                out = out + w[dy + Rr, dx + Rr] * rows[:, _reflect(jj + dx, W)]
    assert out.dtype == dtype
    return out


def blur_bound(bm, Rr):
    L = 2 * Rr + 1
    return (2 * (L + 1) if bm == 1 else L * L + 1) * 255 * U * (1 + 1e-6)


# ------------------------------------------------------------------------------------ the chain
def _hist_stage(q, rec, op, grid, dtype, tr):
    H, W, _ = q.shape
    if op == 1:
        out = q.copy()
        tr["lut"] = []
        for c in range(3):
            v = equalize_lut_values(np.bincount(q[..., c].reshape(-1), minlength=256), dtype)
            lut = np.arange(256) if v is None else lut_of(v)
            tr["lut"].append(lut)
            out[..., c] = lut[q[..., c]]
        return out
    ty, tx = grid
    th, tw = H // ty, W // tx
    Y = byte(luma_values(q, dtype))
    climit = clahe_limit(clahe_limit_value(rec, th * tw, dtype), th * tw, dtype)
    luts = np.zeros((ty, tx, 256), dtype=np.int64)
    for a in range(ty):
        for b in range(tx):
            tile = Y[a * th:(a + 1) * th, b * tw:(b + 1) * tw]
            luts[a, b] = lut_of(clahe_lut_values(np.bincount(tile.reshape(-1), minlength=256),
                                                 climit, th * tw, dtype))
    Yp = byte(clahe_interp_values(Y, luts, ty, tx, dtype))
    tr.update(Y=Y, climit=climit, lut=luts)
    return np.clip(q.astype(np.int64) + (Yp - Y)[..., None], 0, 255).astype(np.uint8)


def _chain(image_n, rec, dtype):
    """one sample through HSV, the histogram op and the blur -> (bytes, trace of the integers
    every segment handed on)"""
    rec = np.asarray(rec, dtype=f32)
    H, W, _ = image_n.shape
    hsv, op, grid, bm, Rr = modes(rec, H, W)
    tr = {}
    q = image_n
    if hsv:
        q = byte(hsv_values(q, rec, dtype)).astype(np.uint8)
    tr["hsv"] = q
    if op:
        q = _hist_stage(q, rec, op, grid, dtype, tr)
    tr["hist"] = q
    if bm:
        q = byte(blur_values(q, rec, bm, Rr, dtype)).astype(np.uint8)
    tr["out"] = q
    return q, tr


def _post(image, post, rng, dtype):
    N, H, W, _ = image.shape
    out = np.empty_like(image)
    for n in range(N):
        q, _ = _chain(image[n], post[n], dtype)
        out[n] = R._salt_pepper(q, None if rng is None else rng[n], H, W)
    return out


def post_f32(image, post, rng=None):
    return _post(image, post, rng, f32)


def post_f64(image, post, rng=None):
    return _post(image, post, rng, f64)


def salt_pepper_hit(rng_n, H, W):
    """bool [H, W]: the pixels salt / pepper overwrites"""
    z = np.full((H, W, 3), 7, dtype=np.uint8)
    return (R._salt_pepper(z, rng_n, H, W) != 7).any(-1)


# ------------------------------------------------------------------------------------ the check
def _tie(v):
    return np.abs(v - np.floor(v) - 0.5)


def _hold(fig, name, got, want, tie, bound, skip=None):
    """got (integers) against want (integers from fp64) where tie is the fp64 value's distance
    to a rounding tie: at most 1 apart, and only within `bound` of a tie"""
    d = np.abs(np.asarray(got, dtype=np.int64) - want)
    tie = np.broadcast_to(tie, d.shape)
    if skip is not None:
        keep = ~np.broadcast_to(skip, d.shape)
        d, tie = d[keep], tie[keep]
    fig[name] = {"max_diff": int(d.max()) if d.size else 0, "differing": int((d > 0).sum()),
                 "max_tie_distance": float(tie[d > 0].max()) if (d > 0).any() else 0.0,
                 "bound": float(bound)}
    assert d.size == 0 or d.max() <= 1, (name, fig[name])
    assert ((d == 0) | (tie <= bound)).all(), (name, fig[name])


def check_against_f64(image_n, rec, final=None, skip=None):
    """Hold every segment of the fp32 chain of one sample against fp64 (module docstring).
    `final`: the bytes to hold against the LAST active stage in place of the fp32 chain's (a
    kernel's output; `skip` marks pixels to leave out there, such as salt / pepper hits).
    Returns the measured figures per segment."""
    rec = np.asarray(rec, dtype=f32)
    H, W, _ = image_n.shape
    hsv, op, (ty, tx), bm, Rr = modes(rec, H, W)
    _, tr = _chain(image_n, rec, f32)
    last = "blur" if bm else "hist" if op else "hsv" if hsv else None
    fig = {}

    def got(stage, key):
        if final is not None and stage == last:
            return final, skip
        return tr[key], None

    if final is not None and last is None:
        assert np.array_equal(final[~skip] if skip is not None else final,
                              image_n[~skip] if skip is not None else image_n)
    if hsv:
        v = hsv_values(image_n, rec, f64)
        g, s = got("hsv", "hsv")
        _hold(fig, "hsv", g, byte(v), _tie(v), hsv_bound(rec), s)
    q = tr["hsv"]
    if op == 1:
        g, s = got("hist", "hist")
        for c in range(3):
            v = equalize_lut_values(np.bincount(q[..., c].reshape(-1), minlength=256), f64)
            if v is None:
                want, tie = q[..., c].astype(np.int64), np.full(q.shape[:2], 0.5)
            else:
                _hold(fig, f"equalize_lut{c}", tr["lut"][c], lut_of(v), _tie(v), EQUALIZE_BOUND)
                want, tie = lut_of(v)[q[..., c]], _tie(v)[q[..., c]]
            _hold(fig, f"equalize{c}", g[..., c], want, tie, EQUALIZE_BOUND, s)
    elif op == 2:
        th, tw = H // ty, W // tx
        v = luma_values(q, f64)
        _hold(fig, "luma", tr["Y"], byte(v), _tie(v), LUMA_BOUND)
        t = float(clahe_limit_value(rec, th * tw, f64))
        c64 = clahe_limit(f64(t), th * tw, f64)
        fig["climit"] = {"fp32": int(tr["climit"]), "fp64": int(c64), "t": t}
        assert tr["climit"] == c64 or abs(t - np.rint(t)) <= 2 * U * t, fig["climit"]
        Y = tr["Y"]
        for a in range(ty):
            for b in range(tx):
                tile = Y[a * th:(a + 1) * th, b * tw:(b + 1) * tw]
                v = clahe_lut_values(np.bincount(tile.reshape(-1), minlength=256), tr["climit"],
                                     th * tw, f64)
                _hold(fig, f"clahe_lut{a}{b}", tr["lut"][a, b], lut_of(v), _tie(v),
                      CLAHE_LUT_BOUND)
        sv = clahe_interp_values(Y, tr["lut"], ty, tx, f64)
        want = np.clip(q.astype(np.int64) + (byte(sv) - Y)[..., None], 0, 255)
        g, s = got("hist", "hist")
        _hold(fig, "clahe", g, want, _tie(sv)[..., None], CLAHE_INTERP_BOUND, s)
    if bm:
        v = blur_values(tr["hist"], rec, bm, Rr, f64)
        g, s = got("blur", "out")
        _hold(fig, "blur", g, byte(v), _tie(v), blur_bound(bm, Rr), s)
    return fig


# ------------------------------------------------------------------------------------ the cases
SHAPES = [(2, 16, 24), (3, 33, 37), (2, 40, 52), (2, 64, 64)]
STAGES = ("hsv", "equalize", "clahe", "separable", "dense", "all")


def noise_batch(N, H, W, seed):
    """seeded uint8 noise, with a gray run (d == 0) and a black run (V == 0) planted in rows 0, 1
    and sample 0's channel 1 constant (an equalize channel that stays as it is)"""
    g = np.random.default_rng(seed)
    image = g.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    image[:, 0, :6] = image[:, 0, :6, :1]
    image[:, 1, :6] = 0
    image[0, :, :, 1] = 77
    return image


def ramp_batch(N, H, W, seed):
    """a smooth diagonal ramp plus +-12 levels of noise: CLAHE tiles that are neither flat nor
    uniform"""
    g = np.random.default_rng(seed)
    ii, jj = np.mgrid[0:H, 0:W]
    base = 30.0 + 180.0 * (ii / max(H - 1, 1) * 0.6 + jj / max(W - 1, 1) * 0.4)
    tint = np.array([1.0, 0.85, 0.7])
    image = base[None, ..., None] * tint + g.integers(-12, 13, (N, H, W, 3))
    return np.clip(np.rint(image), 0, 255).astype(np.uint8)


def batch(shape, stage):
    N, H, W = shape
    return ramp_batch(N, H, W, H) if stage in ("clahe", "all") else noise_batch(N, H, W, H)


def grids(shape):
    """the CLAHE tile grids a shape is tested with (each divides it)"""
    _, H, W = shape
    return {(16, 24): [(1, 1), (2, 3), (4, 8)], (33, 37): [(1, 1), (3, 1), (3, 1)],
            (40, 52): [(1, 1), (2, 2), (8, 4)], (64, 64): [(1, 1), (8, 8), (2, 4)]}[(H, W)]


def records(augment, shape, stage, seed=None):
    """Three batches of N records of one stage at one shape: [post fp32 [N, 64]].  HSV: shifts
    over the full range, dh beyond +-180 in batch 2.  CLAHE: the shape's grids in turn, a clip
    limit that clips nothing (sample 0 of batch 0: every bin <= area), one that clips every
    non-empty bin (sample 1 of batch 0: climit 1) and random ones.  Separable: R = 1, 2, 4 by
    batch, Gaussian taps; dense: R = 1, 3, 2, motion lines.  "all": everything at once."""
    N, H, W = shape
    g = np.random.default_rng(1000 + H if seed is None else seed)
    out = []
    for b in range(3):
        q = np.zeros((N, POST), dtype=np.float64)
        for n in range(N):
            if stage in ("hsv", "all"):
                q[n, 0] = 1
                q[n, 1] = g.uniform(-90, 90) if b < 2 else g.choice([-1, 1]) * g.uniform(200, 500)
                q[n, 2], q[n, 3] = g.uniform(-120, 120), g.uniform(-100, 100)
            if stage == "equalize" or (stage == "all" and (b + n) % 2 == 0):
                q[n, 4] = 1
            if stage == "clahe" or (stage == "all" and (b + n) % 2 == 1):
                q[n, 4] = 2
                q[n, 6], q[n, 7] = grids(shape)[b]
                q[n, 5] = g.uniform(1.0, 4.0)
                if stage == "clahe" and b == 0 and n == 0:
                    q[n, 5] = 300.0                 # t >= area: nothing is clipped
                if stage == "clahe" and b == 0 and n == 1:
                    q[n, 5] = 0.01                  # climit 1: every non-empty bin is clipped
            if stage == "separable" or (stage == "all" and n % 2 == 0):
                k = (3, 5, 9)[b]
                Rr, taps = augment.gaussian_taps(0.3 * ((k - 1) * 0.5 - 1) + 0.8,
                                                 radius=(k - 1) // 2)
                q[n, 8], q[n, 9] = 1, Rr
                q[n, 10:10 + Rr + 1] = taps[:Rr + 1]
            if stage == "dense" or (stage == "all" and n % 2 == 1):
                k = (3, 7, 5)[b]
                a, c = g.choice(k * k, 2, replace=False)
                q[n, 8], q[n, 9] = 2, (k - 1) // 2
                q[n, 15:15 + k * k] = augment.motion_line(
                    k, (int(a % k), int(a // k)), (int(c % k), int(c // k))).reshape(-1)
        out.append(q.astype(np.float32))
    return out
