"""References and inputs for the InstanceNorm-backward tests (tests/test_in_bwd_refs_cpu.py,
tests/test_in_bwd_fp64_gpu.py and the `gen` mode of tests/tools/step_kernel_harness.py).  torch
only, on whatever device the tensors live; nothing here calls the library.  Loaded by path like
the other tools modules; the plane families are those of tests/tools/in_stats_refs.py (S).  Here:
  * the fp64 reference (`reference`), evaluated from exactly the fp32 (or bf16-rounded) values the
    kernel is given - g, y, mean, rstd, gamma, beta, mask, slope - and NOT through autograd over
    recomputed statistics (the rounding of the statistics to fp32, ~6e-8 |mean| / std in xhat,
    would otherwise be charged to the kernel):
        al = gamma rstd    be = beta - mean al    z = y al + be    sel = 1 if z > 0 else slope
        gz = g mask sel    xhat = (y - mean) rstd
        S1 = sum gz    S2 = sum gz xhat    A1 = sum |gz|    A2 = sum |gz xhat|      (per n, c)
        dz = al (gz - S1 / HW - xhat S2 / HW)    dgamma_c = sum_n S2    dbeta_c = sum_n S1
  * ties: an element with |z| < 4 2^-23 (|y al| + |mean al| + |beta|).  Either selection is a
    correct fp32 answer there, so ties are left out of the dz comparison and what they could
    contribute, sum_ties |g mask| (1 - slope) (times |xhat| for S2), is added to the permitted
    error of S1, S2, dgamma and dbeta - and, through c1 = S1 / HW and c2 = S2 / HW, as
    |al| (T1 + |xhat| T2) / HW to that of every dz of the tie's own plane: a plain fp32 evaluation
    that selects the other way on ONE tie of a 128-pixel plane moves c1 by |g| / 128, 1.6e-2 of
    the scale of a dz whose own gz is on the slope side (`level` x `offset`, 8 x 16 x 1024), so
    without this term the rule "either selection is correct" would hold for S1 and not for the
    dz formed from it.  The term is 0 on every plane without a tie.  At most TIE_CAP = 0.1 % of a
    case's elements may be ties: a condition on the inputs (metric `ties`), asserted for every
    family and shape by the CPU test;
  * the metric (`compare`, with `failures`, `report`, `worst_of` in the style of in_stats_refs):
    every quantity on its own scale, per plane or per element, with the position of the worst;
  * an fp32 restatement of the pass (`restate32`: running sums per tile of 64 or 256 pixels, fp64
    merge, fp32 c1, c2, dz) for the CPU check of the check;
  * the gradient families (G_FAMILIES), the fixed list of (gradient, plane) pairs (CASES), the
    shapes of the stand-alone pass (PASS_SHAPES) and the altered references (ALTERED)."""
import importlib.util
import os

import torch

_spec = importlib.util.spec_from_file_location("in_stats_refs", os.path.join(
    os.path.dirname(os.path.abspath(__file__)), "in_stats_refs.py"))
S = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(S)

SLOPE = 0.01         # nn.LeakyReLU's default
TOL_BS = 2e-5        # the harness's TOL_BS: S1, S2, dgamma, dbeta, dbias, each on its own sum of |terms|
TOL_IN = 5e-5        # the harness's TOL_IN: dz, per element
TOL_STAT = S.TOL_STAT   # the forward's a on the scale |y al| + |mean al| + |beta|
TIE_BAND = 4.0 * 2.0 ** -23
TIE_CAP = 1e-3
B16_STORE = 2.0 ** -8   # the one rounding of a bf16 store, relative to the stored value

_nc = S._nc


# --------------------------------------------------------------------------- inputs
def affine(N, C, seed, device="cpu"):
    """S.affine (gamma in [0.5, 1.5], beta in [-1, 1], a mask / 0.7 with a 0 entry) with beta kept
    at least 0.05 from 0.  Weakened on purpose: on a constant plane (and on a plane of one pixel)
    xhat = 0 and z = beta on every element, while the tie band 4 2^-23 (|y al| + |mean al| +
    |beta|) reaches 0.023 at |y| = 50, rstd = 1 / sqrt(eps): a |beta| inside it makes the whole
    plane a tie, which the 0.1 % cap does not admit (and no fp32 expression decides)."""
    gamma, beta, mask = S.affine(N, C, seed, device)
    beta = torch.where(beta < 0, -1.0, 1.0) * beta.abs().clamp_min(0.05)
    return gamma, beta.contiguous(), mask


def stats_once(y, eps=S.EPS):
    """(mean, rstd) [2, N, C] fp32: the fp64 statistics of the values y holds, rounded once"""
    ref = S.plane_stats(y)
    return torch.stack([ref["mean"], ref["rstd"]]).float().contiguous()


def g_gauss(N, H, W, C, seed, device="cpu", y=None, st=None):
    """zero-mean unit Gaussian: the control, what the older tests use"""
    return S._noise(N, H, W, C, S._gen(seed, device), device).contiguous()


def g_level(N, H, W, C, seed, device="cpu", y=None, st=None):
    """a level per plane with |level| / sigma spread over 1 .. 1000 (S.offset): what reaches a
    layer after the lrelu' and dropout of the layer above.  S1 is large, dz = gz - c1 cancels."""
    return S.offset(N, H, W, C, seed, device)


def g_corner(N, H, W, C, seed, device="cpu", y=None, st=None):
    """S.corner + 0.1 noise: the first 8 x 32 tile holds nearly the whole sum.  Weakened on purpose:
    with the 0.01 noise of S.corner alone the terms behind an A = 100 corner are alike to 2 ulp of
    the running sum, every add rounds the same way, and a plain 231-term fp32 running sum (33 x 7
    pixels in one tile of 256) drifts to 6.3e-6 of A2 - over a quarter of the bound.  With 0.1
    noise the roundings are independent."""
    g = S._gen(seed + 100, device)
    return (S.corner(N, H, W, C, seed, device) + 0.1 * S._noise(N, H, W, C, g, device)).contiguous()


def g_aligned(N, H, W, C, seed, device="cpu", y=None, st=None):
    """a xhat + b + 0.1 noise, a and b in +-[0.5, 2] per plane with one sign each: S2 is large and
    nearly all of dz cancels.  Needs y and st = (mean, rstd)."""
    g = S._gen(seed, device)
    a = S._sign((N, C), g, device) * S._uniform((N, C), 0.5, 2, g, device)
    b = S._sign((N, C), g, device) * S._uniform((N, C), 0.5, 2, g, device)
    xh = ((y.double() - _nc(st[0].double())) * _nc(st[1].double())).float()
    return (_nc(a) * xh + _nc(b) + 0.1 * S._noise(N, H, W, C, g, device)).contiguous()


def g_signed_tiles(N, H, W, C, seed, device="cpu", y=None, st=None):
    """8 x 32 tiles at +L and -L in a checkerboard (L in [3, 5] per plane, so a tile's sum is
    ~1e3), 0.01 noise and 1 / HW on top (the plane's sum is ~1): the tile sums cancel in the
    merge, which is what the double merge of in_bwd_finalize1_kernel was written for."""
    g = S._gen(seed, device)
    L = S._uniform((N, C), 3, 5, g, device)
    hh = torch.arange(H, device=device)[:, None] // S.CORNER_ROWS
    ww = torch.arange(W, device=device)[None, :] // S.CORNER_COLS
    sign = (1.0 - 2.0 * ((hh + ww) % 2).float())[None, :, :, None]
    return (sign * _nc(L) + 0.01 * S._noise(N, H, W, C, g, device) + 1.0 / (H * W)).contiguous()


def g_zero(N, H, W, C, seed, device="cpu", y=None, st=None):
    return torch.zeros((N, H, W, C), device=device)


G_FAMILIES = dict(gauss=g_gauss, level=g_level, corner=g_corner, aligned=g_aligned,
                  signed_tiles=g_signed_tiles, zero=g_zero)

# (gradient family, plane family): every family of either kind at least twice
CASES = [("level", "offset"), ("aligned", "offset"), ("corner", "corner"), ("aligned", "corner"),
         ("signed_tiles", "ramp"), ("gauss", "noise"), ("zero", "halves"), ("gauss", "constant"),
         ("level", "constant"), ("signed_tiles", "halves"), ("corner", "ramp"), ("zero", "noise")]
# The stand-alone pass (H, W, C) at N = 2: one pixel; 2 x 2 pixels at 128 lanes per pixel; a split
# that does not divide H W; several pixel groups; C = 4 (256 pixel groups per block); C = 1024 (one
# group); many blocks per image.
PASS_SHAPES = [(1, 1, 32), (2, 2, 512), (33, 7, 128), (12, 20, 32), (16, 32, 4), (8, 16, 1024),
               (128, 128, 32)]


def make_case(gfam, yfam, N, H, W, C, device="cpu", b16=False, seed=3):
    """-> dict(g, y, mean, rstd, gamma, beta, mask): the operands of one case.  b16: y and g
    rounded to bf16 (the statistics are those of the rounded y)."""
    y = S.FAMILIES[yfam](N, H, W, C, seed, device)
    if b16:
        y = y.to(torch.bfloat16).contiguous()
    st = stats_once(y)
    g = G_FAMILIES[gfam](N, H, W, C, seed + 8, device, y=y, st=st)
    if b16:
        g = g.to(torch.bfloat16).contiguous()
    gamma, beta, mask = affine(N, C, 5, device)
    return dict(g=g, y=y, mean=st[0].contiguous(), rstd=st[1].contiguous(), gamma=gamma, beta=beta,
                mask=mask)


# --------------------------------------------------------------------------- the fp64 reference
def reference(g, y, mean, rstd, gamma, beta, mask, slope=SLOPE, sel_one=False):
    """The formulas of the header in fp64 on the values given -> dict: dz, gz-free scales and
    sums (S1, S2, A1, A2, T1, T2 [N, C]; T = what the ties could contribute), dgamma, dbeta and
    their scales, tie [N, H, W, C], kept [N, C], z and lrelu(z) mask (for the forward).
    sel_one: the altered reference "lrelu'(z) ignored"."""
    N, H, W, C = y.shape
    HW = H * W
    gd, yd = g.double(), y.double()
    mu, rs = _nc(mean.double()), _nc(rstd.double())
    gm, bt = gamma.double()[None, None, None, :], beta.double()[None, None, None, :]
    mk = torch.ones_like(mu) if mask is None else _nc(mask.double())
    al = gm * rs
    z = yd * al + (bt - mu * al)
    zscale = (yd * al).abs() + (mu * al).abs() + bt.abs()
    kept = mk != 0
    tie = (z.abs() < TIE_BAND * zscale) & kept
    sel = torch.ones_like(z) if sel_one else torch.where(z > 0, 1.0, float(slope)).double()
    gz = gd * mk * sel
    xh = (yd - mu) * rs
    S1, S2 = gz.sum(dim=(1, 2)), (gz * xh).sum(dim=(1, 2))
    A1, A2 = gz.abs().sum(dim=(1, 2)), (gz * xh).abs().sum(dim=(1, 2))
    flip = torch.where(tie, (gd * mk).abs() * (1.0 - slope), torch.zeros_like(gd))
    T1, T2 = flip.sum(dim=(1, 2)), (flip * xh.abs()).sum(dim=(1, 2))
    dz = al * (gz - _nc(S1) / HW - xh * _nc(S2) / HW)
    dz_scale = al.abs() * (gz.abs() + _nc(A1) / HW + xh.abs() * _nc(A2) / HW)
    dz_ties = al.abs() * (_nc(T1) / HW + xh.abs() * _nc(T2) / HW)
    al_nc = al[:, 0, 0, :].expand(N, C)
    return dict(dz=dz, dz_scale=dz_scale, dz_ties=dz_ties, S1=S1, S2=S2, A1=A1, A2=A2, T1=T1, T2=T2,
                dgamma=S2.sum(0), dbeta=S1.sum(0), dbias_scale=(al_nc.abs() * A1).sum(0),
                tie=tie, kept=kept[:, 0, 0, :].expand(N, C), z=z, zscale=zscale,
                a=torch.where(z > 0, z, z * slope) * mk, HW=HW)


def mask_of_image_1_on_image_0(mask):
    m = mask.clone()
    m[0] = m[1]
    return m


def altered(kind, c, slope=SLOPE):
    """The altered references of the check of the check, from the operands c of `make_case`:
    "sel" (lrelu'(z) ignored), "mask" (the mask of image 1 applied to image 0: a tile taken from
    the neighbouring image's coefficients), "rows" (the last image's first 8 rows of g zeroed)."""
    g, mask, sel_one = c["g"], c["mask"], False
    if kind == "sel":
        sel_one = True
    elif kind == "mask":
        mask = mask_of_image_1_on_image_0(mask)
    elif kind == "rows":
        g = S.rows_zeroed(g)
    else:
        raise KeyError(kind)
    return reference(g, c["y"], c["mean"], c["rstd"], c["gamma"], c["beta"], mask, slope, sel_one)


ALTERED = ("sel", "mask", "rows")


# --------------------------------------------------------------------------- the fp32 restatement
def restate32(g, y, mean, rstd, gamma, beta, mask, slope=SLOPE, tile=64, b16_store=False):
    """A plain fp32 evaluation of the pass: gz and xhat per element, running fp32 sums over tiles
    of `tile` consecutive pixels, an fp64 merge of the tile sums rounded once, fp32 c1, c2 and dz
    -> dict(dz, sums [N, C, 2], dgamma, dbeta, dbias) like the library's results."""
    N, H, W, C = y.shape
    HW = H * W
    gf, yf = g.float().reshape(N, HW, C), y.float().reshape(N, HW, C)
    mu, rs = mean[:, None, :], rstd[:, None, :]
    mk = torch.ones_like(mu) if mask is None else mask[:, None, :]
    al = gamma[None, None, :] * rs
    be = beta[None, None, :] - mu * al
    z = yf * al + be
    gz = gf * mk * torch.where(z > 0, 1.0, float(slope))
    xh = (yf - mu) * rs
    T = -(-HW // tile)
    pad = T * tile - HW

    def tiles(t):
        return torch.cat([t, t.new_zeros(N, pad, C)], 1).reshape(N, T, tile, C)

    t1, t2 = tiles(gz), tiles(gz * xh)
    s1, s2 = torch.zeros(N, T, C, device=y.device), torch.zeros(N, T, C, device=y.device)
    for i in range(tile):
        s1, s2 = s1 + t1[:, :, i], s2 + t2[:, :, i]
    sums = torch.stack([s1.double().sum(1), s2.double().sum(1)], dim=-1).float()     # [N, C, 2]
    coef = sums * torch.tensor(1.0 / HW, dtype=torch.float32, device=y.device)
    dz = al * ((gz - coef[:, None, :, 0]) - xh * coef[:, None, :, 1])
    dbias = (gamma[None] * rstd * (sums[..., 0] - float(HW) * coef[..., 0])).sum(0)
    dz = dz.reshape(N, H, W, C)
    if b16_store:
        dz = dz.to(torch.bfloat16)
    return dict(dz=dz, sums=sums, dgamma=sums[..., 1].sum(0), dbeta=sums[..., 0].sum(0), dbias=dbias)


# --------------------------------------------------------------------------- the metric
def _rel(diff, scale, allow=None):
    """max(|diff| - allow, 0) / scale; where the scale is 0 the value must be exact"""
    e = diff.abs() if allow is None else (diff.abs() - allow).clamp_min(0)
    inf = torch.full_like(e, float("inf"))
    return torch.where(scale > 0, e / torch.where(scale > 0, scale, torch.ones_like(scale)),
                       torch.where(e == 0, torch.zeros_like(e), inf))


def _worst(what, err, tol):
    err = torch.nan_to_num(err, nan=float("inf"))
    i = int(err.argmax())
    return dict(what=what, err=err.flatten()[i].item(), tol=tol,
                at=tuple(int(v) for v in torch.unravel_index(torch.tensor(i), err.shape)))


def compare(got, ref, b16=False):
    """got: dict with any of dz [N, H, W, C], sums [N, C, 2] = (S1, S2), dgamma, dbeta, dbias [C];
    ref: a dict of `reference` -> a list of dict(what, err, tol, at):
      S1, S2        |got - ref| beyond what the ties could contribute, on A1, A2 of its own plane;
      dgamma, dbeta the same summed over the images, on sum_n A2, sum_n A1;
      dz            per element on |al| (|gz| + A1 / HW + |xhat| A2 / HW), ties and dropped planes
                    left out, beyond |al| (T1 + |xhat| T2) / HW (see the header: zero on a plane
                    without ties); b16: also beyond 2^-8 |dz_ref|, the rounding of the bf16 store;
      dbias         (mathematically 0) on sum_n |al| A1;
      nonzero       the count of values that must be exactly 0 and are not: dz, S1, S2 on a
                    plane whose mask is 0 (a scale of 0, as for g = 0, makes any error infinite);
      ties          the share of tie elements against TIE_CAP (a condition on the inputs)."""
    out, nonzero = [], 0
    kept = ref["kept"]
    if "sums" in got:
        s = got["sums"].double()
        out.append(_worst("S1", _rel(s[..., 0] - ref["S1"], ref["A1"], ref["T1"]), TOL_BS))
        out.append(_worst("S2", _rel(s[..., 1] - ref["S2"], ref["A2"], ref["T2"]), TOL_BS))
        nonzero += int((s[~kept] != 0).sum())
    if "dgamma" in got:
        out.append(_worst("dgamma", _rel(got["dgamma"].double() - ref["dgamma"], ref["A2"].sum(0),
                                         ref["T2"].sum(0)), TOL_BS))
    if "dbeta" in got:
        out.append(_worst("dbeta", _rel(got["dbeta"].double() - ref["dbeta"], ref["A1"].sum(0),
                                        ref["T1"].sum(0)), TOL_BS))
    if "dz" in got:
        dz = got["dz"].double()
        allow = ref["dz_ties"] + B16_STORE * ref["dz"].abs() if b16 else ref["dz_ties"]
        err = _rel(dz - ref["dz"], ref["dz_scale"], allow)
        skip = ref["tie"] | ~_nc(kept)
        out.append(_worst("dz", torch.where(skip, torch.zeros_like(err), err), TOL_IN))
        nonzero += int((dz != 0)[(~_nc(kept)).expand_as(dz)].sum())
    if "dbias" in got:
        out.append(_worst("dbias", _rel(got["dbias"].double(), ref["dbias_scale"]), TOL_BS))
    out.append(dict(what="nonzero", err=float(nonzero), tol=0.0, at=()))
    out.append(dict(what="ties", err=float(ref["tie"].sum()) / ref["tie"].numel(), tol=TIE_CAP, at=()))
    return out


def tie_count(ref):
    return int(ref["tie"].sum())


def failures(metrics, scale=1.0):
    """The metrics that exceed `scale` x their bound (scale = 1/4: the fairness condition; the
    conditions `nonzero` and `ties` are never scaled)"""
    bad = []
    for m in metrics:
        tol = m["tol"] if m["what"] in ("nonzero", "ties") else scale * m["tol"]
        if not m["err"] <= tol:
            bad.append(f"{m['what']}: {m['err']:.3e} > {tol:.2e} at {m['at']}")
    return bad


def report(metrics):
    return "  ".join(f"{m['what']} {m['err']:.2e}/{m['tol']:.0e}@{','.join(map(str, m['at']))}"
                     for m in metrics if m["what"] != "nonzero")


def worst_of(metrics):
    """The metric closest to (or furthest over) its bound, the two conditions aside"""
    return max((m for m in metrics if m["what"] not in ("nonzero", "ties") and m["tol"] > 0),
               key=lambda m: m["err"] / m["tol"])


# --------------------------------------------------------------------------- the forward
def compare_forward(a, ref):
    """The forward's a = lrelu(z) mask against the reference: `selection`, the count of kept
    elements outside the ties whose sign(a) is not the reference's selection (must be 0), and
    `a` on the scale |y al| + |mean al| + |beta| at TOL_STAT (ties included: at a tie both
    selections give |a| within the scale's rounding of 0)."""
    kept = _nc(ref["kept"])
    wrong = ((a > 0) != (ref["z"] > 0)) & kept & ~ref["tie"]
    i = int(wrong.flatten().double().argmax())
    at = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), wrong.shape))
    return [dict(what="selection", err=float(wrong.sum()), tol=0.0, at=at),
            _worst("a", _rel(a.double() - ref["a"], ref["zscale"].expand_as(ref["a"])), TOL_STAT),
            dict(what="nonzero", err=float((a != 0)[(~kept).expand_as(a)].sum()), tol=0.0, at=()),
            dict(what="ties", err=float(ref["tie"].sum()) / ref["tie"].numel(), tol=TIE_CAP, at=())]
