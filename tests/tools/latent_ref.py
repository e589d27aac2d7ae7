"""NumPy restatement of the latent-space analysis (`ua.latent`, csrc/latent.hip), written from the
specification in include/unet_hip.h and from the documented behaviour of scikit-learn's exact
t-SNE, not from the kernels.  Every routine takes the working precision as an argument: fp64 is
the reference the fixture records, fp32 is "the same formula in the kernels' precision", whose
distance from fp64 (times 4 for another summation order) is what tests/test_latent_gpu.py allows.

tests/tools/make_golden_latent.py holds these restatements against scikit-learn itself and writes
tests/golden/latent.npz; tests/test_latent_cpu.py replays the fixture through them."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)

# (name, N, D, scale, perplexities): the recorded shapes
SHAPES = (("base", 192, 2048, 1.0, (30.0,)),
          ("ragged", 150, 1028, 1.0, (30.0,)),
          ("splitk", 96, 8192, 1.0, (30.0, 5.0)),
          ("x30", 192, 2048, 30.0, (30.0,)))
STATE_ITERS = (0, 5, 50, 260, 600)


STREAM_SEED = 1


def codes(rng, n, d, scale=1.0):
    """Three Gaussian clusters plus an offset, fp32: centres 0.6 + noise + 0.4 -> (x, labels)."""
    centres = rng.standard_normal((3, d))
    labels = rng.integers(0, 3, n)
    noise = rng.standard_normal((n, d))
    x = ((centres[labels] * 0.6 + noise + 0.4) * scale).astype(np.float32)
    return x, labels.astype(np.uint8)


def all_codes():
    """{name: (x, labels)} of SHAPES: one PCG64 stream (STREAM_SEED), the shapes drawn in order;
    the scaled shape is the base shape's draw times its scale."""
    rng = np.random.Generator(np.random.PCG64(STREAM_SEED))
    out = {}
    for name, n, d, scale, _ in SHAPES:
        if scale == 1.0:
            out[name] = codes(rng, n, d)
        else:
            x, labels = out["base"]
            out[name] = ((x.astype(np.float64) * scale).astype(np.float32), labels)
    return out


# ---- Gram and distances ---------------------------------------------------------------------
def gram(x, dtype=np.float64):
    x = x.astype(dtype)
    mean = (x.sum(axis=0, dtype=dtype) / dtype(x.shape[0])).astype(dtype)
    xc = x - mean
    return xc @ xc.T


def sqdist(g):
    d = np.diag(g)
    out = np.maximum((d[:, None] + d[None, :]) - 2 * g, 0)
    np.fill_diagonal(out, 0)
    return out


# ---- PCA in the dual form -------------------------------------------------------------------
def hash_block(n, cols=8):
    """splitmix64 of the counter, the top 24 bits in [-1, 1): the iteration's start block."""
    z = np.arange(n * cols, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(40)).astype(np.float64) / float(1 << 23) - 1.0).reshape(n, cols)


def svd_flip_rows(components, scores):
    """scikit-learn's svd_flip(u_based_decision=False): the largest |v| of each row positive."""
    k = np.abs(components).argmax(axis=1)
    sign = np.sign(components[np.arange(components.shape[0]), k])
    sign[sign == 0] = 1
    return components * sign[:, None], scores * sign[None, :]


def pca_dual(x, dtype=np.float64, tol=1e-5, max_iter=500):
    """Top-2 PCA of x through the eigenpairs of G by subspace iteration on 8 columns ->
    (scores, components, variances, residuals, iterations).  G, G Q and the results in `dtype`."""
    n = x.shape[0]
    g = gram(x, dtype)
    xc = x.astype(dtype) - (x.astype(dtype).sum(axis=0, dtype=dtype) / dtype(n)).astype(dtype)
    q = np.linalg.qr(hash_block(n))[0]
    for it in range(1, max_iter + 1):
        qf = q.astype(dtype)
        z = (g @ qf).astype(np.float64)
        qd = qf.astype(np.float64)
        b = qd.T @ z
        lam, w = np.linalg.eigh((b + b.T) * 0.5)
        lam, w = lam[::-1][:2], w[:, ::-1][:, :2]
        u, gu = qd @ w, z @ w
        res = np.linalg.norm(gu - u * lam, axis=0) / lam
        if res.max() <= tol:
            break
        q = np.linalg.qr(z)[0]
    u = u / np.linalg.norm(u, axis=0)
    root = np.sqrt(lam)
    comp = ((u / root).astype(dtype).T @ xc).astype(np.float64)
    comp, scores = svd_flip_rows(comp, u * root)
    # what an implementation in `dtype` hands back: its outputs rounded to that type
    return (scores.astype(dtype).astype(np.float64), comp.astype(dtype).astype(np.float64),
            (lam / (n - 1)).astype(dtype).astype(np.float64), res, it)


# ---- t-SNE ------------------------------------------------------------------------------------
def cond_p(dist, perplexity, exp_dtype=np.float64):
    """sklearn.manifold._utils._binary_search_perplexity on the rows of the squared distances, each
    minus its off-diagonal minimum: 100 steps, tolerance 1e-5 on the entropy, beta from 1, doubled
    or halved while unbounded and bisected after, the 1e-8 floor on the row sum, P_ii = 0.  exp and
    the products with beta in `exp_dtype`, the sums in fp64."""
    n = dist.shape[0]
    off = ~np.eye(n, dtype=bool)
    dist = dist.astype(exp_dtype)
    dmin = np.where(off, dist, np.inf).min(axis=1).astype(exp_dtype)
    dd = np.where(off, dist - dmin[:, None], 0).astype(exp_dtype)
    target = np.log(perplexity)
    beta = np.ones(n)
    bmin, bmax = np.full(n, -np.inf), np.full(n, np.inf)
    live = np.ones(n, dtype=bool)
    S = np.ones(n)
    for _ in range(100):
        fb = beta.astype(exp_dtype)
        p = np.where(off, np.exp(-dd * fb[:, None]), 0).astype(exp_dtype)
        s = p.sum(axis=1, dtype=np.float64)
        s[s == 0] = 1e-8
        sdp = (dd * p).astype(exp_dtype).sum(axis=1, dtype=np.float64)
        diff = np.log(s) + beta * (sdp / s) - target
        S = np.where(live, s, S)
        live &= np.abs(diff) > 1e-5
        if not live.any():
            break
        up = live & (diff > 0)
        dn = live & ~(diff > 0)
        bmin[up] = beta[up]
        beta[up] = np.where(np.isinf(bmax[up]), beta[up] * 2, (beta[up] + bmax[up]) * 0.5)
        bmax[dn] = beta[dn]
        beta[dn] = np.where(np.isinf(bmin[dn]), beta[dn] * 0.5, (beta[dn] + bmin[dn]) * 0.5)
    fb = beta.astype(exp_dtype)
    p = np.where(off, np.exp(-dd * fb[:, None]), 0).astype(exp_dtype)
    return (p.astype(np.float64) / S[:, None]).astype(exp_dtype)


def joint_p(pc):
    """_joint_probabilities: (Pc + Pc^T) / max(sum, eps), floored at eps; zero diagonal."""
    p = pc.astype(np.float64) + pc.astype(np.float64).T
    p = np.maximum(p / max(p.sum(), EPS), EPS)
    np.fill_diagonal(p, 0)
    return p.astype(pc.dtype)


def squareform_f32(condensed, n):
    """The [N, N] matrix of a condensed (upper triangle, row-major) vector."""
    out = np.zeros((n, n), dtype=condensed.dtype)
    out[np.triu_indices(n, 1)] = condensed
    return out + out.T


def tsne_step(P, y, update, gains, exaggeration, momentum, lr, dtype=np.float64):
    """One iteration of scikit-learn's _gradient_descent on _kl_divergence ->
    dict(y, update, gains, kl, grad_norm, grad).  With q_ij = 1 / (1 + |y_i - y_j|^2), Z the sum of
    q over i != j: grad_i = 4 (sum_j eP q (y_i - y_j) - sum_j q^2 (y_i - y_j) / Z); gains + 0.2 where
    update grad < 0, else gains 0.8, floored at 0.01; update = momentum update - lr gains grad;
    KL = sum eP log(eP / (q / Z)); the norm is that of gains grad, as _gradient_descent tests it."""
    n = y.shape[0]
    off = ~np.eye(n, dtype=bool)
    y, update, gains = y.astype(dtype), update.astype(dtype), gains.astype(dtype)
    ep = (P.astype(dtype) * dtype(exaggeration)).astype(dtype)
    diff = y[:, None, :] - y[None, :, :]
    d1 = (dtype(1) + (diff * diff).sum(axis=2)).astype(dtype)
    q = np.where(off, dtype(1) / d1, 0).astype(dtype)
    first = ((ep * q)[:, :, None] * diff).sum(axis=1, dtype=dtype)
    second = ((q * q)[:, :, None] * diff).sum(axis=1, dtype=dtype)
    Z = q.sum(axis=1, dtype=dtype).sum(dtype=np.float64)
    grad = (dtype(4) * (first - second * dtype(1.0 / Z))).astype(dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = np.where(off, ep * (np.log(ep) + np.log(d1)), 0).astype(dtype)
    kl = float(terms.sum(axis=1, dtype=dtype).sum(dtype=np.float64) +
               np.log(Z) * ep.sum(axis=1, dtype=dtype).sum(dtype=np.float64))
    inc = ((update < 0) & (grad > 0)) | ((update > 0) & (grad < 0))
    gains = np.maximum(np.where(inc, gains + dtype(0.2), gains * dtype(0.8)), dtype(0.01))
    gg = (gains * grad).astype(dtype)
    update = (dtype(momentum) * update - dtype(lr) * gg).astype(dtype)
    return dict(y=(y + update).astype(dtype), update=update, gains=gains.astype(dtype), kl=kl,
                grad_norm=float(np.sqrt((gg.astype(np.float64) ** 2).sum())), grad=grad)


def kl_divergence(P, y):
    """KL(P || Q) of an embedding in fp64, Q = q / Z (what _kl_divergence reports)."""
    out = tsne_step(P.astype(np.float64), y.astype(np.float64), np.zeros_like(y, dtype=np.float64),
                    np.ones_like(y, dtype=np.float64), 1.0, 0.0, 0.0)
    return out["kl"]


def learning_rate(n, early_exaggeration=12.0):
    return max(n / early_exaggeration / 4.0, 50.0)


def scaled_init(scores):
    """init='pca' of TSNE: the scores with column 0 at standard deviation 1e-4, fp32."""
    return (scores / np.std(scores[:, 0]) * 1e-4).astype(np.float32)


# ---- the picture -----------------------------------------------------------------------------
def pixel_centres(coords, size):
    H, W = size
    c = np.asarray(coords, dtype=np.float64)
    lo, hi = c.min(axis=0), c.max(axis=0)
    span = np.where(hi > lo, hi - lo, 1.0)
    t = (c - (lo - 0.05 * span)) / (1.1 * span)
    return np.stack([np.round(t[:, 0] * (W - 1)), np.round((1.0 - t[:, 1]) * (H - 1))],
                    axis=1).astype(np.int32)


def raster(centres, labels, palette, size, radius):
    """uint8 [H, W, 3]: white ground; the points in index order, each covering dx^2 + dy^2 <= r^2,
    dst = (dst 77 + src 179 + 128) >> 8 per channel.  Integers throughout."""
    H, W = size
    img = np.full((H, W, 3), 255, dtype=np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    for (cx, cy), l in zip(np.asarray(centres, dtype=np.int64), labels):
        cover = (xx - cx) ** 2 + (yy - cy) ** 2 <= radius * radius
        src = np.asarray(palette[int(l)], dtype=np.int64)
        img[cover] = (img[cover] * 77 + src * 179 + 128) >> 8
    return img.astype(np.uint8)
