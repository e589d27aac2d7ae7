"""Restatements of `unet_augment_light_u8`, written from its specification (the comment in
include/unet_hip.h), not from the kernels:

  light_f32   numpy in the specification's number formats and operation order, every operation
              rounded on its own - fp32, except HLS, which the specification carries in fp64 and
              rounds to fp32 before `byte`: what the kernels must reproduce byte for byte (the
              hue noise of ISO apart, whose log / cos come from different libraries; with S = 0
              or sigma_h = 0 the hue noise cannot act and ISO is byte-exact too);
  light_f64   the same chain in fp64 throughout, without the rounding to fp32 (its own bytes
              from segment to segment).

The chain is a sequence of arithmetic SEGMENTS, each ending in `byte`: ISO noise, the shadow, every
single blend of the sun flare and of the fog, the box mean.  What one segment hands to the next
is bytes.  DECISIONS are shared by both chains, as the integers of post_ref.py are: lambda and the
Poisson draw k (the integer path: fp64 sums, the fp32 table), and every geometric inside test
(made in fp32, as the specification states).  `check_against_f64` holds every segment on its own:
the fp64 value computed FROM THE BYTES THE fp32 CHAIN HANDED IT against the byte the fp32 chain
(or, for the last segment, a kernel) made of it: at most 1 apart, and only where the fp64 value is
within the segment's bound of a rounding tie.

The bounds, with u = 2^-24 (an fp32 operation errs by at most u times its result), derived from
operation counts:

  blend     o' = (a ov) + ((1 - a) o) with a in [0, 1], ov, o <= 255: the product a ov 255 u,
            1 - a one u (255 u on the second product), that product 255 u, the sum 255 u:
            4 (255 u).  The fog's constant a 255 is one product: the same count.  A step of the
            flare's source forms a = (q q) q from q = n / d: u on q, then 2 u + u, then 3 u + u + u:
            6 u on a, which enters both products: 4 (255 u) + 2 (6 u) 255 = 16 (255 u).
  box       the sum of at most 81 bytes is exact in fp32; one division: 255 u; 2 (255 u) taken.
  HLS       both chains evaluate it in fp64 (error some 1e-13 of a level, counted as nothing
            beside u); the normative chain then rounds the channel to fp32: 255 u.
            HLS_BOUND = 2 (255 u).
  ISO       on top of HLS: h2 = H + sigma_h z, with z from a float library held to E_Z = 2^-17
            absolute (log, cos and the argument 2 pi u2 in fp32: a few 1e-6 on |z| < 6): the hue
            errs by |sigma_h| E_Z, the fraction f by a sixtieth of it, a channel by 255 times
            that.

Arrays are numpy: image uint8 [N,H,W,3], light fp32 [N, 272], rng [N,4] integers or None."""
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
E_Z = 2.0 ** -17
LIGHT = 272
# record layout (include/unet_hip.h)
A_ISO, A_SIGMA, A_INTENSITY, A_MODE, A_COUNT = 0, 1, 2, 3, 4
A_SRC_X, A_SRC_Y, A_SRC_R, A_STEPS = 5, 6, 7, 8                 # flare
A_FOG_R, A_FOG_A, A_FOG_K = 5, 6, 7                             # fog
A_BODY = 16
MODE_SHADOW, MODE_FLARE, MODE_FOG = 1, 2, 3
MAX_POLYGONS, MAX_CIRCLES, MAX_POINTS, MAX_STEPS, MAX_BOX, MAX_LAMBDA = 2, 10, 128, 40, 9, 64
BLEND_BOUND = 4 * 255 * U
SOURCE_BOUND = 16 * 255 * U
BOX_BOUND = 2 * 255 * U
HLS_BOUND = 2 * 255 * U
FLT_MIN = f32(np.finfo(np.float32).tiny)


def byte(v):
    """clamp(rint(v), 0, 255) with fmin / fmax (a NaN becomes 0) -> int64"""
    with np.errstate(all="ignore"):
        return np.fmin(np.fmax(np.rint(v), 0), 255).astype(np.int64)


def _clampi(v, lo, hi):
    """a record value clamped in fp32 to lo..hi (a NaN becomes lo), then truncated"""
    return int(np.fmin(np.fmax(f32(v), f32(lo)), f32(hi)))


# ------------------------------------------------------------------------------------ decoding
def modes(rec):
    """(ISO on, mode 0..3) of one record as the device decodes it"""
    rec = np.asarray(rec, dtype=f32)
    m = rec[A_MODE]
    return bool(rec[A_ISO] == 1), 1 if m == 1 else 2 if m == 2 else 3 if m == 3 else 0


# ------------------------------------------------------------------------------------ HLS
def hls_forward(q, d_):
    """uint8 [..., 3] -> (H degrees, L, S) in dtype d_"""
    r, g, b = (q[..., c].astype(d_) for c in range(3))
    V, m = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    s, d = V + m, V - m
    L = s / d_(510)
    with np.errstate(all="ignore"):
        S = np.where(d == 0, d_(0), np.where(s <= 255, d / np.where(s == 0, d_(1), s),
                                             d / np.where(s == 510, d_(1), d_(510) - s)))
        dd = np.where(d == 0, d_(1), d)
        hr = d_(60) * ((g - b) / dd)
        hg = d_(120) + d_(60) * ((b - r) / dd)
        hb = d_(240) + d_(60) * ((r - g) / dd)
    H = np.where(d == 0, d_(0), np.where(V == r, hr, np.where(V == g, hg, hb)))
    H = np.where(H < 0, H + d_(360), H)
    assert H.dtype == d_ and L.dtype == d_ and S.dtype == d_
    return H, L, S


def hls_back(H, L, S, d_):
    """-> the three channels before rounding, in d_"""
    with np.errstate(all="ignore"):
        l2 = d_(510) * L
        c = np.where(l2 <= 255, l2 * S, (d_(510) - l2) * S)
        hp = H / d_(60)
        k = np.fmin(np.fmax(np.floor(hp), d_(0)), d_(5))
        f = hp - k
        odd = (k == 1) | (k == 3) | (k == 5)
        x = np.where(odd, c * (d_(1) - f), c * f)
        lo = d_(0.5) * (l2 - c)
        hi, mid = lo + c, lo + x
    table = ((hi, mid, lo), (mid, hi, lo), (lo, hi, mid), (lo, mid, hi), (mid, lo, hi),
             (hi, lo, mid))
    out = np.zeros(np.shape(H) + (3,), dtype=d_)
    for sct, trio in enumerate(table):
        for ch in range(3):
            out[..., ch] = np.where(k == sct, trio[ch], out[..., ch])
    assert out.dtype == d_
    return out


# ------------------------------------------------------------------------------------ ISO noise
def iso_sums(q):
    """the exact integer sums of s = V + m and of s^2 over one sample"""
    s = q.max(-1).astype(np.int64) + q.min(-1).astype(np.int64)
    return int(s.sum()), int((s * s).sum())


def iso_lambda(rec, sums, HW):
    """lambda in fp64 from the integer sums, rounded to fp32"""
    n = f64(HW)
    mean = f64(sums[0]) / n
    var = np.fmax(f64(sums[1]) / n - mean * mean, f64(0))
    std = np.sqrt(var) / f64(510)
    with np.errstate(all="ignore"):
        lam = np.fmin(np.fmax((f64(f32(rec[A_INTENSITY])) * f64(255)) * std, f64(0)),
                      f64(MAX_LAMBDA))
    return f32(lam)


def poisson_table(lam):
    """fp32 [256]: the running sums c_k of t_0 = 1, t_k = (t_{k-1} lam) / k, an entry below FLT_MIN
    set to 0; T = c[255]"""
    lam = f32(lam)
    t = f32(1)
    c = np.empty(256, dtype=f32)
    acc = f32(0)
    for k in range(256):
        if k:
            t = f32(f32(t * lam) / f32(k))
            if t < FLT_MIN:
                t = f32(0)
        acc = f32(acc + t)
        c[k] = acc
    return c


def poisson_draw(c, words):
    """k [H, W]: the number of c_j <= u T, capped at 255; u = (w2 >> 8) 2^-24"""
    u = (words[..., 2].astype(np.uint64) >> np.uint64(8)).astype(f32) * f32(2.0 ** -24)
    uT = u * c[255]
    assert uT.dtype == f32
    return np.minimum(np.searchsorted(c, uT, side="right"), 255).astype(np.int64)


def _snap(v, d_):
    """what the normative chain does to a channel that comes out of HLS: round it to fp32"""
    return v.astype(f32) if d_ is f32 else v


def iso_values(q, rec, z, k, d_):
    """bytes [H,W,3], the normal z [H,W] (of the chain d_) and the draw k [H,W] -> values before
    `byte`; HLS in fp64 for both chains"""
    z, chain, d_ = z.astype(f64), d_, f64
    H, L, S = hls_forward(q, d_)
    with np.errstate(all="ignore"):
        h2 = H + d_(rec[A_SIGMA]) * z
        h2 = h2 - d_(360) * np.floor(h2 / d_(360))
        h2 = np.fmin(np.fmax(h2, d_(0)), np.nextafter(d_(360), d_(0)))
        L2 = np.fmin(L + (k.astype(d_) / d_(255)) * (d_(1) - L), d_(1))
    assert h2.dtype == d_ and L2.dtype == d_
    return _snap(hls_back(h2, L2, S, d_), chain)


def iso_bound(rec):
    return HLS_BOUND + 255 * abs(float(rec[A_SIGMA])) * E_Z / 60


def iso_draws(rec, q, rng_n):
    """(lambda, table, k [H,W], words) of one sample's ISO stage; the decisions both chains share"""
    Hh, Ww, _ = q.shape
    lam = iso_lambda(rec, iso_sums(q), Hh * Ww)
    c = poisson_table(lam)
    words = R.pixel_words(int(rng_n[0]), int(rng_n[1]), Hh, Ww, 3)
    return lam, c, poisson_draw(c, words), words


# ------------------------------------------------------------------------------------ geometry
def _grid(Hh, Ww, centre):
    off = f32(0.5) if centre else f32(0)
    return (np.arange(Ww, dtype=f32)[None, :] + off), (np.arange(Hh, dtype=f32)[:, None] + off)


def polygon_inside(rec, p, Hh, Ww):
    """bool [H, W]: the pixel centre is inside polygon p by the even-odd rule, in fp32"""
    xc, yc = _grid(Hh, Ww, True)
    v = np.asarray(rec[A_BODY + 10 * p:A_BODY + 10 * p + 10], dtype=f32).reshape(5, 2)
    cross = np.zeros((Hh, Ww), dtype=np.int64)
    for e in range(5):
        (x1, y1), (x2, y2) = v[e], v[(e + 1) % 5]
        with np.errstate(all="ignore"):
            span = (y1 <= yc) != (y2 <= yc)
            t = (yc - y1) / (y2 - y1)
            xi = x1 + t * (x2 - x1)
            assert xi.dtype == f32
            cross += span & (xc < xi)
    return (cross % 2) == 1


def circle_inside(cx, cy, r, Hh, Ww):
    """bool [H, W]: pixel (i, j) at (x, y) = (j, i) within r of (cx, cy), in fp32"""
    xf, yf = _grid(Hh, Ww, False)
    with np.errstate(all="ignore"):
        dx, dy = xf - f32(cx), yf - f32(cy)
        d2 = dx * dx + dy * dy
        rr = np.fmax(f32(r), f32(0))
        return d2 <= rr * rr


# ------------------------------------------------------------------------------------ segments
def _blend(a, ov, o, d_):
    a = d_(a)
    with np.errstate(all="ignore"):
        v = a * ov.astype(d_) + (d_(1) - a) * o.astype(d_)
    assert v.dtype == d_
    return v


def _segments(image_n, rec, rng_n):
    """The segments of one sample, in order: (name, fn(state, d_) -> values, after(state, bytes),
    bound).  state is a dict with "o" (the bytes so far) and what a mode carries ("ov")."""
    rec = np.asarray(rec, dtype=f32)
    Hh, Ww, _ = image_n.shape
    iso, mode = modes(rec)
    segs = []

    def put(state, b):
        state["o"] = b

    if iso and rng_n is not None:
        def iso_fn(state, d_):
            _, _, k, words = iso_draws(rec, state["o"].astype(np.uint8), rng_n)
            state["k"] = k
            return iso_values(state["o"].astype(np.uint8), rec, R.normals(words, d_)[..., 0], k, d_)
        segs.append(("iso", iso_fn, put, iso_bound(rec)))

    if mode == MODE_SHADOW:
        count = _clampi(rec[A_COUNT], 0, MAX_POLYGONS)
        m = sum(polygon_inside(rec, p, Hh, Ww).astype(np.int64) for p in range(count)) \
            if count else np.zeros((Hh, Ww), dtype=np.int64)

        def shadow_fn(state, d_):
            q = state["o"].astype(np.uint8)
            H, L, S = hls_forward(q, f64)
            L2 = L * np.where(m == 2, f64(0.25), f64(0.5))
            v = _snap(hls_back(H, L2, S, f64), d_)
            return np.where((m > 0)[..., None], v, q.astype(d_))
        segs.append(("shadow", shadow_fn, put, HLS_BOUND))

    elif mode == MODE_FLARE:
        count = _clampi(rec[A_COUNT], 0, MAX_CIRCLES)
        T = _clampi(rec[A_STEPS], 2, MAX_STEPS)

        def circle_seg(c):
            cx, cy, r, a = rec[A_BODY + 7 * c:A_BODY + 7 * c + 4]
            col = rec[A_BODY + 7 * c + 4:A_BODY + 7 * c + 7]
            inside = circle_inside(cx, cy, r, Hh, Ww)

            def fn(state, d_):
                ov = state.get("ov", state["o"].astype(f32))
                ov = np.where(inside[..., None], col[None, None, :], ov).astype(f32)
                state["ov"] = ov
                return _blend(a, ov, state["o"], d_)
            return (f"circle{c}", fn, put, BLEND_BOUND)

        def source_seg(i):
            Tm1 = f32(T - 1)
            ri = f32(1) + f32(f32(f32(rec[A_SRC_R] - f32(1)) * f32(i)) / Tm1)
            inside = circle_inside(rec[A_SRC_X], rec[A_SRC_Y], ri, Hh, Ww)

            def fn(state, d_):
                ov = state.get("ov", state["o"].astype(f32))
                ov = np.where(inside[..., None], f32(255), ov).astype(f32)
                state["ov"] = ov
                q = d_(T - 1 - i) / d_(T - 1)
                return _blend((q * q) * q, ov, state["o"], d_)
            return (f"source{i}", fn, put, SOURCE_BOUND)

        segs += [circle_seg(c) for c in range(count)] + [source_seg(i) for i in range(T)]

    elif mode == MODE_FOG:
        P = _clampi(rec[A_COUNT], 0, MAX_POINTS)
        kb = _clampi(rec[A_FOG_K], 1, MAX_BOX)
        a = rec[A_FOG_A]

        def point_seg(p):
            inside = circle_inside(rec[A_BODY + 2 * p], rec[A_BODY + 2 * p + 1], rec[A_FOG_R],
                                   Hh, Ww)

            def fn(state, d_):
                o = state["o"].astype(d_)
                with np.errstate(all="ignore"):
                    v = d_(a) * d_(255) + (d_(1) - d_(a)) * o
                assert v.dtype == d_
                return np.where(inside[..., None], v, o)
            return (f"point{p}", fn, put, BLEND_BOUND)

        segs += [point_seg(p) for p in range(P)]
        if kb >= 2:
            def box_fn(state, d_):
                x = state["o"].astype(d_)
                lo = kb // 2
                ii, jj = np.arange(Hh), np.arange(Ww)
                s = np.zeros(x.shape, dtype=d_)
                for dy in range(-lo, kb - lo):
                    rows = x[_reflect(ii + dy, Hh)]
                    for dx in range(-lo, kb - lo):
                        s = s + rows[:, _reflect(jj + dx, Ww)]
                v = s / d_(kb * kb)
                assert v.dtype == d_
                return v
            segs.append(("box", box_fn, put, BOX_BOUND))
    return segs


def _reflect(idx, size):
    idx = np.where(idx < 0, -idx, idx)
    idx = np.where(idx > size - 1, 2 * (size - 1) - idx, idx)
    return np.clip(idx, 0, size - 1)


# ------------------------------------------------------------------------------------ the chain
def _chain(image_n, rec, rng_n, d_):
    state = {"o": image_n.astype(np.int64)}
    for _, fn, after, _ in _segments(image_n, rec, rng_n):
        after(state, byte(fn(state, d_)))
    return state["o"].astype(np.uint8), state


def _light(image, light, rng, d_):
    out = np.empty_like(image)
    for n in range(image.shape[0]):
        out[n], _ = _chain(image[n], light[n], None if rng is None else rng[n], d_)
    return out


def light_f32(image, light, rng=None):
    return _light(image, light, rng, f32)


def light_f64(image, light, rng=None):
    return _light(image, light, rng, f64)


def iso_k(image_n, rec, rng_n):
    """(lambda, k [H, W]) the ISO stage of one sample draws"""
    lam, _, k, _ = iso_draws(np.asarray(rec, dtype=f32), image_n, rng_n)
    return lam, k


# ------------------------------------------------------------------------------------ the check
def _tie(v):
    return np.abs(v - np.floor(v) - 0.5)


def check_against_f64(image_n, rec, rng_n=None, final=None):
    """Hold every segment of the fp32 chain of one sample against fp64 (module docstring).
    `final`: the bytes to hold against the LAST segment in place of the fp32 chain's (a kernel's
    output).  Returns the measured figures per segment."""
    segs = _segments(image_n, rec, rng_n)
    state = {"o": image_n.astype(np.int64)}
    fig = {}
    if final is not None and not segs:
        assert np.array_equal(final, image_n)
    for at, (name, fn, after, bound) in enumerate(segs):
        before = dict(state)
        got = byte(fn(state, f32))
        v = fn(dict(before), f64)
        if final is not None and at == len(segs) - 1:
            got_held = np.asarray(final, dtype=np.int64)
        else:
            got_held = got
        d = np.abs(got_held - byte(v))
        tie = _tie(v)
        fig[name] = {"max_diff": int(d.max()), "differing": int((d > 0).sum()),
                     "max_tie_distance": float(tie[d > 0].max()) if (d > 0).any() else 0.0,
                     "bound": float(bound)}
        assert d.max() <= 1, (name, fig[name])
        assert ((d == 0) | (tie <= bound)).all(), (name, fig[name])
        after(state, got)
    return fig


# ------------------------------------------------------------------------------------ the cases
SHAPES = [(3, 16, 24), (3, 33, 37), (3, 40, 52)]
STAGES = ("shadow", "flare", "fog")
RNG = np.array([[11, 22, 0, 0], [33, 44, 0, 0], [55, 66, 0, 0]], dtype=np.int64)


def noise_batch(N, H, W, seed):
    """seeded uint8 noise with a gray run (d == 0), a black run and a white run planted in rows
    0..2, and a dark half (s <= 255) on the left"""
    g = np.random.default_rng(seed)
    image = g.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    image[:, :, :W // 2] //= 2
    image[:, 0, :6] = image[:, 0, :6, :1]
    image[:, 1, :6] = 0
    image[:, 2, :6] = 255
    return image


def gray_batch(N, H, W, lo=0, hi=60):
    """a gray image of two levels in a checker of 4 x 4 cells: S = 0 everywhere"""
    ii, jj = np.mgrid[0:H, 0:W]
    level = np.where(((ii // 4) + (jj // 4)) % 2 == 0, lo, hi).astype(np.uint8)
    return np.broadcast_to(level[None, ..., None], (N, H, W, 3)).copy()


def identity(n):
    return np.zeros((n, LIGHT), dtype=np.float32)


def shadow_record(polygons):
    """polygons: one or two lists of five (x, y)"""
    q = np.zeros(LIGHT, dtype=np.float64)
    q[A_MODE], q[A_COUNT] = MODE_SHADOW, len(polygons)
    for p, poly in enumerate(polygons):
        q[A_BODY + 10 * p:A_BODY + 10 * p + 10] = np.asarray(poly, dtype=np.float64).reshape(-1)
    return q.astype(np.float32)


def flare_record(src, Rs, T, circles):
    """circles: (cx, cy, r, a, (c0, c1, c2)) each"""
    q = np.zeros(LIGHT, dtype=np.float64)
    q[A_MODE], q[A_COUNT] = MODE_FLARE, len(circles)
    q[A_SRC_X], q[A_SRC_Y], q[A_SRC_R], q[A_STEPS] = src[0], src[1], Rs, T
    for c, (cx, cy, r, a, col) in enumerate(circles):
        q[A_BODY + 7 * c:A_BODY + 7 * c + 7] = (cx, cy, r, a) + tuple(col)
    return q.astype(np.float32)


def fog_record(points, radius, a, k):
    q = np.zeros(LIGHT, dtype=np.float64)
    q[A_MODE], q[A_COUNT] = MODE_FOG, len(points)
    q[A_FOG_R], q[A_FOG_A], q[A_FOG_K] = radius, a, k
    if len(points):
        q[A_BODY:A_BODY + 2 * len(points)] = np.asarray(points, dtype=np.float64).reshape(-1)
    return q.astype(np.float32)


def with_iso(rec, sigma_h, intensity):
    rec = np.array(rec, dtype=np.float32)
    rec[A_ISO], rec[A_SIGMA], rec[A_INTENSITY] = 1, sigma_h, intensity
    return rec


def records(shape, stage):
    """Two batches of N = 3 records of one stage at one shape: [light fp32 [3, 272]], six records.
    Shadow: record 0 a self-intersecting polygon (a pentagram), record 1 two overlapping
    polygons, the rest random (one or two polygons, vertices uniform over the image).  Flare:
    record 0 has its centre outside the image, all have 6-10 circles on a line through the
    centre and Rs in 20..60 (T = Rs // 10).  Fog: k = 2, 3, 4, 5, 9 and 1 (no box) in turn,
    P = 0, 1, 128 and random counts, record 3 also has ISO noise on (the halo regenerates it) with
    sigma_h = 0, so that no library function enters and the bytes are exact."""
    N, H, W = shape
    g = np.random.default_rng(2000 + H)
    recs = []
    for i in range(6):
        if stage == "shadow":
            if i == 0:
                cx, cy, r = W / 2.0, H / 2.0, 0.45 * min(H, W)
                ang = [np.pi / 2 + 2 * np.pi * (2 * v) / 5 for v in range(5)]
                polys = [[(cx + r * np.cos(t), cy - r * np.sin(t)) for t in ang]]
            elif i == 1:
                polys = [[(1, 1), (W * 0.7, 2), (W * 0.8, H * 0.7), (W * 0.4, H * 0.9),
                          (2, H * 0.6)],
                         [(W * 0.3, H * 0.2), (W - 1, H * 0.3), (W - 2, H - 1),
                          (W * 0.5, H - 2), (W * 0.2, H * 0.5)]]
            else:
                polys = [np.stack([g.uniform(0, W, 5), g.uniform(0, H, 5)], 1)
                         for _ in range(1 + i % 2)]
            recs.append(shadow_record(polys))
        elif stage == "flare":
            src = (-3.5, H + 2.0) if i == 0 else (g.uniform(0, W), g.uniform(0, H))
            Rs = int(g.integers(20, 61))
            ang = 2 * np.pi * g.uniform()
            circles = []
            for _ in range(int(g.integers(6, 11))):
                d = g.uniform(-W, W)
                circles.append((src[0] + d * np.cos(ang), src[1] + d * np.sin(ang),
                                int(g.integers(1, 9)), g.uniform(0.05, 0.2),
                                tuple(int(v) for v in g.integers(205, 256, 3))))
            recs.append(flare_record(src, Rs, Rs // 10, circles))
        else:
            k = (2, 3, 4, 5, 9, 1)[i]
            P = (0, 1, 128, 17, 40, 9)[i]
            pts = np.stack([g.uniform(-2, W + 2, P), g.uniform(-2, H + 2, P)], 1)
            rec = fog_record(pts, g.uniform(2, 0.3 * min(H, W)), g.uniform(0.02, 0.3), k)
            recs.append(with_iso(rec, 0.0, 0.4) if i == 3 else rec)
    return [np.stack(recs[0:3]), np.stack(recs[3:6])]
