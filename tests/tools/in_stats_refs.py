"""References and inputs for the InstanceNorm statistics tests (tests/test_in_stats_refs_cpu.py,
tests/test_in_stats_fp64_gpu.py).  torch only, on whatever device the caller names; nothing here
calls the library.  Loaded by path like the other tools modules.  Here:
  * the fp64 references: the statistics of a plane tensor (plane_stats) and the exact merge of
    (mean_t, M2_t) summaries of tiles (merge_exact), both ending in `finish` (rstd and the folded
    coefficients alpha = gamma rstd mask, beta = (beta - mean gamma rstd) mask);
  * three fp32 restatements, for the CPU check of the check only: a well-conditioned one (chunked
    two-pass + Chan merge, what the header comment of csrc/instnorm.hip describes), the naive
    one-pass E[x^2] - E[x]^2, and the shifted-sum form of the two-level finalizer, without and
    with the conditioning test the tests of this module brought it;
  * the plane families (FAMILIES): functions of (N, H, W, C, seed, device) whose levels and noise
    differ per (image, channel), so that a channel or image mix-up changes the answer;
  * the per-element relative metric (compare) with the project's bounds.
All planes are NHWC fp32 tensors; all statistics are [N, C]."""
import math

import torch

EPS = 1e-5           # nn.InstanceNorm2d's default
TOL_STAT = 5e-5      # rstd, alpha, beta (the harness's TOL_STAT), here per element
TOL_Y = 2e-5         # mean, on the scale max |y| of its own plane (the harness's TOL_Y)
TOL_CONST = 1e-6     # rstd of a constant plane against 1 / sqrt(eps)


# --------------------------------------------------------------------------- plane families
# Every family keeps the plane's mean away from 0 (|mean| at least a tenth of the plane's
# spread): without an affine beta the folded coefficient is beta = -mean gamma rstd, held on the
# scale of its own value, and no fp32 evaluation holds a mean that cancels to 0 RELATIVE to
# itself - the mean's own bound (on the scale max |y|) is the one that applies there.
def _gen(seed, device):
    return torch.Generator(device=device).manual_seed(seed)


def _uniform(shape, lo, hi, g, device):
    return torch.rand(shape, generator=g, device=device) * (hi - lo) + lo


def _noise(N, H, W, C, g, device):
    return torch.randn((N, H, W, C), generator=g, device=device)


def _centred(N, H, W, C, g, device):
    """Gaussian noise with the mean of every plane taken out: a small plane's mean is then its
    level and not a sample of it (which could land on 0)"""
    z = _noise(N, H, W, C, g, device)
    return z - z.mean(dim=(1, 2), keepdim=True)


def _nc(t):
    """[N, C] -> [N, 1, 1, C]"""
    return t[:, None, None, :]


def _sign(shape, g, device):
    return torch.where(torch.rand(shape, generator=g, device=device) < 0.5, -1.0, 1.0)


def _index(N, C, device):
    """k = n C + c as [N, C]"""
    return torch.arange(N * C, device=device).reshape(N, C)


def offset(N, H, W, C, seed, device="cpu"):
    """mu + sigma noise with |mu| / sigma = 1000^u, u a low-discrepancy sequence over (n, c) (so
    that even a few planes spread over 1 .. 1000), sigma in [0.02, 1] and |mu| <= 50."""
    g = _gen(seed, device)
    u = torch.frac(_index(N, C, device).double() * 0.6180339887498949 + 0.37 * seed)
    ratio = torch.pow(torch.tensor(1000.0, dtype=torch.double, device=device), u)
    sigma = torch.exp(_uniform((N, C), math.log(0.02), 0.0, g, device).double())
    sigma = torch.minimum(sigma, 50.0 / ratio)
    mu = _sign((N, C), g, device).double() * sigma * ratio
    return (_centred(N, H, W, C, g, device) * _nc(sigma.float()) + _nc(mu.float())).contiguous()


CORNER_ROWS, CORNER_COLS = 8, 32
_CORNER = ((3.0, 0.01), (100.0, 1.0), (100.0, 0.01))


def corner(N, H, W, C, seed, device="cpu"):
    """A flat plane (level +-[0.25, 0.75]) at noise sigma with its first 8 rows x 32 columns lifted
    by A away from 0; (A, sigma) cycles over (3, 0.01), (100, 1), (100, 0.01) with (n, c).  The
    outlier first tile, whatever the tile shape.  On a plane smaller than 16 x 64 the lifted
    corner is at most half of each side, so that it stays a corner."""
    g = _gen(seed, device)
    k = (_index(N, C, device) + seed) % 3
    A = torch.tensor([a for a, _ in _CORNER], device=device)[k]
    sigma = torch.tensor([s for _, s in _CORNER], device=device)[k]
    sign = _sign((N, C), g, device)
    y = _noise(N, H, W, C, g, device) * _nc(sigma) + _nc(sign * _uniform((N, C), 0.25, 0.75, g, device))
    y[:, :min(CORNER_ROWS, H // 2), :min(CORNER_COLS, W // 2), :] += _nc(sign * A)
    return y.contiguous()


def ramp(N, H, W, C, seed, device="cpu"):
    """level + a h / H + b w / W + 0.01 noise, a and b in [-4, 4], the level +-[0.5, 2] beyond the
    ramps' range (the plane keeps one sign): structure inside every tile and across tiles."""
    g = _gen(seed, device)
    a, b = _uniform((N, C), -4, 4, g, device), _uniform((N, C), -4, 4, g, device)
    lvl = _sign((N, C), g, device) * (_uniform((N, C), 0.5, 2, g, device) + a.abs() + b.abs())
    hh = (torch.arange(H, device=device, dtype=torch.float32) / H)[None, :, None, None]
    ww = (torch.arange(W, device=device, dtype=torch.float32) / W)[None, None, :, None]
    return (_noise(N, H, W, C, g, device) * 0.01 + _nc(lvl) + _nc(a) * hh + _nc(b) * ww).contiguous()


def halves(N, H, W, C, seed, device="cpu"):
    """Left and right halves at different levels, top and bottom halves likewise (each level in
    [0.5, 5], one sign per plane), 0.02 noise."""
    g = _gen(seed, device)
    sign = _sign((N, C), g, device)
    lv = [_nc(sign * _uniform((N, C), 0.5, 5, g, device)) for _ in range(4)]
    y = _noise(N, H, W, C, g, device) * 0.02
    y[:, :, :W // 2] += lv[0]
    y[:, :, W // 2:] += lv[1]
    y[:, :H // 2] += lv[2]
    y[:, H // 2:] += lv[3]
    return y.contiguous()


_DYADIC = (2.5, -0.75, 0.5, -3.0, 1.25, 8.0, -0.125, 6.5, -40.0, 0.0625, 17.0)


def constant(N, H, W, C, seed, device="cpu"):
    """One dyadic constant per (n, c): every partial sum is exact, the variance is exactly 0 and
    rstd = 1 / sqrt(eps)."""
    lvl = torch.tensor(_DYADIC, device=device)[(_index(N, C, device) * 7 + seed) % len(_DYADIC)]
    return _nc(lvl).expand(N, H, W, C).contiguous()


def noise(N, H, W, C, seed, device="cpu"):
    """The stationary planes of the older tests: mu + sigma noise, |mu| in [0.2, 0.5], sigma in
    [0.5, 1.5]."""
    g = _gen(seed, device)
    mu = _sign((N, C), g, device) * _uniform((N, C), 0.2, 0.5, g, device)
    sigma = _uniform((N, C), 0.5, 1.5, g, device)
    return (_centred(N, H, W, C, g, device) * _nc(sigma) + _nc(mu)).contiguous()


FAMILIES = dict(offset=offset, corner=corner, ramp=ramp, halves=halves, constant=constant,
                noise=noise)


def affine(N, C, seed, device="cpu", keep=0.7):
    """gamma in [0.5, 1.5], beta in [-1, 1], a dropout mask [N, C] divided by the keep probability
    (with at least one dropped and one kept entry)."""
    g = _gen(seed, device)
    gamma, beta = _uniform((C,), 0.5, 1.5, g, device), _uniform((C,), -1, 1, g, device)
    mask = (torch.rand((N, C), generator=g, device=device) < keep).float() / keep
    mask[0, 0], mask[-1, -1] = 0.0, 1.0 / keep
    return gamma.contiguous(), beta.contiguous(), mask.contiguous()


# --------------------------------------------------------------------------- shapes
# The merges: (tiles, px per tile, H, W, tile rows, tile columns) with tiles px = H W.  Fewer than
# 512 tiles take the one-level finalizer, 512 or more the two-level pair; 511 / 512 is that
# threshold, 1024 x 256, 2048 x 128 and 512 x 128 are the counts of the train step's 512^2 and
# 256^2 layers, 4096 x 64 the largest count the workspace formula admits at 512^2.
MERGE_ONE_LEVEL = [(2, 64, 4, 32, 2, 32), (48, 256, 96, 128, 8, 32), (511, 128, 292, 224, 4, 32)]
MERGE_TWO_LEVEL = [(512, 128, 128, 512, 4, 32), (1024, 256, 512, 512, 8, 32),
                   (2048, 128, 512, 512, 4, 32), (4096, 64, 512, 512, 2, 32)]
MERGE_CHANNELS = (32, 64, 96)       # 96: a partly filled 32-channel block of the finalizers
# The stand-alone pass (N, H, W, C): one pixel; fewer pixels than lanes; a split that does not
# divide H W; one and several chunks per lane; C / 4 = 128 and 256 lanes per pixel (256 is the
# most the kernel's shape test admits).
PASS_SHAPES = [(2, 2, 2, 512), (1, 1, 1, 32), (2, 33, 7, 128), (2, 12, 20, 32), (1, 128, 128, 32),
               (2, 64, 64, 64), (1, 5, 3, 1024)]


# --------------------------------------------------------------------------- fp64 references
def finish(mean, var, gamma=None, beta=None, mask=None, eps=EPS):
    """(mean, biased variance) [N, C] fp64 -> dict(mean, var, rstd, alpha, beta) and, for the
    metric, kept (mask != 0) and beta_scale = (|beta_c| + |mean gamma rstd|) mask"""
    rstd = 1.0 / torch.sqrt(var + eps)
    gm = torch.ones_like(mean) if gamma is None else gamma.double()[None].expand_as(mean)
    bt = torch.zeros_like(mean) if beta is None else beta.double()[None].expand_as(mean)
    mk = torch.ones_like(mean) if mask is None else mask.double()
    return dict(mean=mean, var=var, rstd=rstd, alpha=gm * rstd * mk, beta=(bt - mean * gm * rstd) * mk,
                kept=mk != 0, beta_scale=(bt.abs() + (mean * gm * rstd).abs()) * mk)


def plane_stats(y, gamma=None, beta=None, mask=None, eps=EPS):
    """The statistics of the NHWC plane tensor y (of any float type) in fp64, two passes."""
    yd = y.double()
    mean = yd.mean(dim=(1, 2))
    var = ((yd - _nc(mean)) ** 2).mean(dim=(1, 2))
    return finish(mean, var, gamma, beta, mask, eps)


def plane_max(y):
    """max |y| per plane [N, C]: the scale of the mean's bound"""
    return y.abs().amax(dim=(1, 2)).double()


def tile_summaries(y, th, tw):
    """(mean_t, M2_t) [N, tiles, C] in fp64 of the th x tw tiles of y, tiles in row-major order of
    the tile grid (H, W multiples of th, tw)."""
    N, H, W, C = y.shape
    assert H % th == 0 and W % tw == 0
    t = y.double().reshape(N, H // th, th, W // tw, tw, C).permute(0, 1, 3, 2, 4, 5)
    t = t.reshape(N, (H // th) * (W // tw), th * tw, C)
    mean_t = t.mean(dim=2)
    return mean_t, ((t - mean_t[:, :, None]) ** 2).sum(dim=2)


def merge_moments(mean_t, m2_t, counts):
    """Chan's merge of (count, mean, M2) summaries in fp64 -> (mean, biased variance).  counts: one
    number for equal tiles, or a [tiles] tensor."""
    mean_t, m2_t = mean_t.double(), m2_t.double()
    T = mean_t.shape[1]
    cnt = torch.as_tensor(counts, dtype=torch.double, device=mean_t.device).expand(T)[None, :, None]
    total = cnt.sum()
    mean = (cnt * mean_t).sum(dim=1) / total
    m2 = m2_t.sum(dim=1) + (cnt * (mean_t - mean[:, None]) ** 2).sum(dim=1)
    return mean, m2 / total


def merge_exact(mean_t, m2_t, counts, gamma=None, beta=None, mask=None, eps=EPS):
    """The statistics of the image whose tiles have the summaries (mean_t, M2_t) [N, tiles, C]."""
    return finish(*merge_moments(mean_t, m2_t, counts), gamma, beta, mask, eps)


def tile_replaced(mean_t, m2_t, dst=0, src=1):
    """The perturbation "a tile written to the wrong slot": summary dst replaced by summary src."""
    mean_t, m2_t = mean_t.clone(), m2_t.clone()
    mean_t[:, dst], m2_t[:, dst] = mean_t[:, src], m2_t[:, src]
    return mean_t, m2_t


def count_halved(T, px, which=0):
    """The perturbation "a merge with a wrong count constant": tile `which` counted at half."""
    counts = torch.full((T,), float(px), dtype=torch.double)
    counts[which] = px / 2
    return counts


def rows_zeroed(y, image=-1, rows=8):
    """The perturbation of the plane reference: one image's first rows zeroed."""
    y = y.clone()
    y[image, :rows] = 0
    return y


def first_tile_replaced(y, image=-1, rows=CORNER_ROWS, cols=CORNER_COLS):
    """The same perturbation on a plane: one image's first 8 x 32 tile replaced by the tile to
    its right (narrower where the plane has fewer than 64 columns)."""
    y = y.clone()
    cols = min(cols, y.shape[2] // 2)
    y[image, :rows, :cols] = y[image, :rows, cols:2 * cols]
    return y


# --------------------------------------------------------------------------- fp32 restatements
def _finish32(mean, var, gamma=None, beta=None, mask=None, eps=EPS):
    """The tail of every finalizer, in fp32 -> [4, N, C] like the library's statistics tensor"""
    rs = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32, device=var.device))
    a = rs if gamma is None else gamma[None] * rs
    b2 = -mean * a if beta is None else beta[None] - mean * a
    if mask is not None:
        a, b2 = a * mask, b2 * mask
    return torch.stack([mean, rs, a, b2])


def well_conditioned32(y, gamma=None, beta=None, mask=None, chunk=64):
    """Chunked two-pass + Chan merge in fp32: per chunk of `chunk` pixels the mean and the sum of
    squared deviations from it, then a pairwise tree of Chan merges over the chunks."""
    N, H, W, C = y.shape
    HW = H * W
    x = y.float().reshape(N, HW, C)
    cnts, means, m2s = [], [], []
    nfull = HW // chunk
    for part, k in ((x[:, :nfull * chunk].reshape(N, nfull, chunk, C), chunk),
                    (x[:, nfull * chunk:].reshape(N, 1, HW - nfull * chunk, C), HW - nfull * chunk)):
        if part.shape[1] == 0 or k == 0:
            continue
        m = part.sum(dim=2) / k
        means.append(m)
        m2s.append(((part - m[:, :, None]) ** 2).sum(dim=2))
        cnts.append(torch.full((part.shape[1],), float(k), device=y.device))
    cnt, mean, m2 = torch.cat(cnts), torch.cat(means, 1), torch.cat(m2s, 1)
    while cnt.shape[0] > 1:
        if cnt.shape[0] % 2:
            cnt = torch.cat([cnt, cnt.new_zeros(1)])
            mean = torch.cat([mean, mean.new_zeros(N, 1, C)], 1)
            m2 = torch.cat([m2, m2.new_zeros(N, 1, C)], 1)
        na, nb = cnt[0::2], cnt[1::2]
        n = na + nb
        f = (nb / n)[None, :, None]
        d = mean[:, 1::2] - mean[:, 0::2]
        mean = mean[:, 0::2] + d * f
        m2 = m2[:, 0::2] + m2[:, 1::2] + d * d * (na[None, :, None] * f)
        cnt = n
    return _finish32(mean[:, 0], m2[:, 0] / HW, gamma, beta, mask)


def naive32(y, gamma=None, beta=None, mask=None):
    """One pass, E[x^2] - E[x]^2 in fp32."""
    N, H, W, C = y.shape
    x = y.float().reshape(N, H * W, C)
    m = x.sum(dim=1) / (H * W)
    var = ((x * x).sum(dim=1) / (H * W) - m * m).clamp_min(0)
    return _finish32(m, var, gamma, beta, mask)


GUARD = 16.0     # in_stats_finalize_comb_kernel: the shifted result stands while S2 <= 16 M2


def _fma32(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def shifted32(mean_t, m2_t, px, gamma=None, beta=None, mask=None, groups=16, lanes=32, guard=None,
              taken=None):
    """The shifted-sum two-level merge of fp32 summaries [N, tiles, C], with the lane striding and
    the trees of in_stats_finalize_grp / _comb_kernel: per group S1 = sum(mean_t - K), S2 =
    sum(M2_t + px (mean_t - K)^2) with K = the mean of tile 0, then M2 = S2 - tiles px (S1 /
    tiles)^2.  guard=None: unguarded, as the kernels were before the tests of this module
    rejected them; guard=16: with the combine kernel's conditioning test (GUARD), the planes that
    fail it merged again around their own mean (taken, a list: gets the [N, C] mask of those)."""
    mean_t, m2_t = mean_t.float(), m2_t.float()
    N, T, C = mean_t.shape
    dev = mean_t.device
    per = torch.tensor(float(px), dtype=torch.float32, device=dev)
    K = mean_t[:, 0]
    gi = torch.arange(groups, device=dev)
    t0, t1 = T * gi // groups, T * (gi + 1) // groups
    s1 = torch.zeros(N, groups, lanes, C, device=dev)
    s2 = torch.zeros_like(s1)
    for i in range((int((t1 - t0).max()) + lanes - 1) // lanes):
        t = t0[:, None] + torch.arange(lanes, device=dev)[None] + lanes * i
        ok = (t < t1[:, None])[None, :, :, None]
        t = t.clamp_max(T - 1)
        d = mean_t[:, t] - K[:, None, None]
        s1 = torch.where(ok, s1 + d, s1)
        s2 = torch.where(ok, s2 + _fma32(per * d, d, m2_t[:, t]), s2)
    stride = lanes // 2
    while stride >= 1:
        s1[:, :, :stride] += s1[:, :, stride:2 * stride].clone()
        s2[:, :, :stride] += s2[:, :, stride:2 * stride].clone()
        stride //= 2
    a1, a2 = torch.zeros(N, C, device=dev), torch.zeros(N, C, device=dev)
    for g in range(groups):
        a1, a2 = a1 + s1[:, g, 0], a2 + s2[:, g, 0]
    tiles = torch.tensor(float(T), dtype=torch.float32, device=dev)
    d = a1 / tiles
    mu, q = K + d, a2 - tiles * per * d * d
    if guard is not None:
        # the combine kernel's test: S2 > guard M2 -> the plane is merged again around its mean
        again = ~(a2 <= guard * q)
        m = mean_t.sum(dim=1) / tiles
        dd = mean_t - m[:, None]
        mu = torch.where(again, m, mu)
        q = torch.where(again, (m2_t + per * dd * dd).sum(dim=1), q)
        if taken is not None:
            taken.append(again)
    return _finish32(mu, q.clamp_min(0) / float(T * px), gamma, beta, mask)


# --------------------------------------------------------------------------- the metric
def _worst(what, err, tol):
    err = torch.nan_to_num(err, nan=float("inf"))
    i = int(err.argmax())
    C = err.shape[1]
    return dict(what=what, err=err.flatten()[i].item(), tol=tol, at=(i // C, i % C))


def compare(st, ref, ymax, const=False):
    """st: the statistics [4, N, C] under test (mean, rstd, alpha, beta); ref: a dict of `finish`;
    ymax: plane_max of the planes.  Every quantity element by element, maximised over (n, c) ->
    a list of dict(what, err, tol, at):
      rstd, alpha   |got - ref| / |ref|;
      mean          on the scale max |y| of its own plane;
      beta          on the scale (|beta_c| + |mean gamma rstd|) mask of its own element;
      dropped       where the mask is 0, alpha and beta must be exactly 0: the count of entries
                    that are not;
      const=True:   rstd against 1 / sqrt(eps) within TOL_CONST as well."""
    st = st.double()
    kept = ref["kept"]
    one, zero = torch.ones_like(ref["mean"]), torch.zeros_like(ref["mean"])
    out = [_worst("mean", (st[0] - ref["mean"]).abs() / (ymax + 1e-300), TOL_Y),
           _worst("rstd", (st[1] - ref["rstd"]).abs() / ref["rstd"], TOL_STAT),
           _worst("alpha", torch.where(kept, (st[2] - ref["alpha"]).abs() /
                                       torch.where(kept, ref["alpha"].abs(), one), zero), TOL_STAT),
           _worst("beta", torch.where(kept, (st[3] - ref["beta"]).abs() /
                                      torch.where(kept, ref["beta_scale"] + 1e-300, one), zero), TOL_STAT)]
    dropped = int(((st[2] != 0) | (st[3] != 0))[~kept].sum())
    out.append(dict(what="dropped", err=float(dropped), tol=0.0, at=(0, 0)))
    if const:
        out.append(_worst("rstd of a constant", (st[1] * math.sqrt(EPS) - 1.0).abs(), TOL_CONST))
    return out


def failures(metrics, scale=1.0):
    """The metrics that exceed `scale` x their bound (scale = 1/4: the fairness condition)"""
    return [f"{m['what']}: max error {m['err']:.3e} > {scale * m['tol']:.2e} at (n, c) = {m['at']}"
            for m in metrics if not m["err"] <= scale * m["tol"]]


def report(metrics):
    return "  ".join(f"{m['what']} {m['err']:.2e}/{m['tol']:.0e}@{m['at'][0]},{m['at'][1]}"
                     for m in metrics if m["what"] != "dropped")


def worst_of(metrics):
    """The metric closest to (or furthest over) its bound, `dropped` aside"""
    return max((m for m in metrics if m["tol"] > 0), key=lambda m: m["err"] / m["tol"])
