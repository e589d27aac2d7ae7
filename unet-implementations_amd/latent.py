"""Latent-space analysis of the autoencoder's codes on the HIP path (`ua.latent`): the PCA and
t-SNE scatter pictures of AE_pretrained/reconstruction/utils/visualize.py:179-231
(`visualize_latent_space`), which `analyze_latent_space` of src/evaluate.py:380-440 writes.

One centred Gram matrix G = (X - mean)(X - mean)^T of the [N, D] codes (fp32 matrix cores,
`ops.latent_gram`) serves both reductions: PCA in its dual form (the top eigenpairs of G by block
subspace iteration, `G Q` in HIP) and the exact t-SNE, whose squared distances are
G_ii + G_jj - 2 G_ij.  The t-SNE is scikit-learn's `method='exact'` algorithm restated
(`_binary_search_perplexity`, `_joint_probabilities`, `_kl_divergence`, `_gradient_descent`,
`TSNE._tsne`); the picture is a raster kernel, without axes, title or colour bar.
Torch is plumbing here: the 8-column orthonormalisation and the 8 x 8 Rayleigh-Ritz step, the sign
rule, the map from coordinates to pixel centres.
"""
import collections
import math
import warnings

import numpy as np
import torch

from . import ops

TSNE_MAX_N = ops.TSNE_MAX_N
PCA_BLOCK = 8            # columns of the subspace iteration
PCA_TOL = 1e-5           # |G q - lambda q| / lambda of both kept pairs
PCA_MAX_ITER = 500
# matplotlib's viridis at 0, 0.5 and 1 (what `c=labels` gives the labels 0 / 1 / 2), as bytes
VIRIDIS3 = ((68, 1, 84), (33, 145, 140), (253, 231, 37))

LatentGram = collections.namedtuple("LatentGram", "g x mean")
PCA2D = collections.namedtuple("PCA2D", "scores components explained_variance residuals n_iter")
TSNE2D = collections.namedtuple("TSNE2D", "y kl_divergence n_iter")


def _shape_of(a):
    shape = tuple(getattr(a, "shape", ()))
    if len(shape) != 2:
        raise ValueError("expected an [N, D] matrix of latent codes")
    return shape


def _device_matrix(latents):
    """numpy or torch [N, D] -> contiguous fp32 on the device."""
    N, D = _shape_of(latents)
    if N < 2 or D < 4 or D % 4:
        raise ValueError(f"latent codes must be [N >= 2, D a multiple of 4], got {N} x {D}")
    t = torch.as_tensor(latents)
    if not t.is_cuda:
        t = t.to("cuda")
    return t.float().contiguous()


def gram(latents):
    """LatentGram(g, x, mean): the centred Gram matrix fp32 [N, N] of the codes [N, D] (numpy or
    torch), with the device copy of the codes and their column mean (the PCA components need
    them)."""
    x = _device_matrix(latents)
    mean = ops.latent_col_mean(x)
    return LatentGram(ops.latent_gram(x, mean), x, mean)


def _as_gram(latents_or_gram):
    if isinstance(latents_or_gram, LatentGram):
        return latents_or_gram
    return gram(latents_or_gram)


def _hash_block(n, cols):
    """The start block of the subspace iteration: splitmix64 of the counter i * cols + c, the top
    24 bits as a value in [-1, 1).  No generator state: the same block on every call."""
    z = np.arange(n * cols, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    v = (z >> np.uint64(40)).astype(np.float64) / float(1 << 23) - 1.0
    return v.reshape(n, cols)


def pca_2d(latents_or_gram, tol=PCA_TOL, max_iter=PCA_MAX_ITER):
    """PCA2D(scores [N, 2], components [2, D], explained_variance [2], residuals, n_iter) of the
    codes: `PCA(n_components=2).fit_transform` in the dual form.  The top two eigenpairs
    (lambda, u) of G come from a subspace iteration on 8 columns (G Q in HIP; QR and the 8 x 8
    Rayleigh-Ritz problem through torch) that stops when |G u - lambda u| / lambda <= tol for both,
    or warns at max_iter.  scores = u sqrt(lambda); components = (X - mean)^T u / sqrt(lambda), one
    pass over X; the sign is scikit-learn's svd_flip(u_based_decision=False): the largest-magnitude
    entry of each component is positive.  explained_variance = lambda / (N - 1), fp64."""
    G = _as_gram(latents_or_gram)
    g = G.g
    N = g.shape[0]
    q = torch.linalg.qr(torch.from_numpy(_hash_block(N, PCA_BLOCK)).to(g.device)).Q
    z = torch.empty((N, PCA_BLOCK), dtype=torch.float32, device=g.device)
    residuals, n_iter = [math.inf, math.inf], 0
    for n_iter in range(1, max_iter + 1):
        qf = q.float().contiguous()
        ops.latent_gram_apply(g, qf, out=z)
        qd, zd = qf.double(), z.double()
        b = qd.T @ zd
        lam, w = torch.linalg.eigh((b + b.T) * 0.5)          # ascending
        lam, w = lam.flip(0)[:2], w.flip(1)[:, :2]
        u, gu = qd @ w, zd @ w
        residuals = ((gu - u * lam).norm(dim=0) / lam).tolist()   # the iteration's one host sync
        if not all(r == r for r in residuals) or min(lam.tolist()) <= 0:
            raise ValueError("pca_2d: the codes span fewer than two directions")
        if max(residuals) <= tol:
            break
        q = torch.linalg.qr(zd).Q
    else:
        warnings.warn(f"pca_2d: the subspace iteration stopped at {max_iter} iterations with "
                      f"residuals {residuals[0]:.3e}, {residuals[1]:.3e} (tolerance {tol:g})",
                      RuntimeWarning)
    root = lam.sqrt()
    u = u / u.norm(dim=0)
    scores = u * root
    w2 = (u / root).float().contiguous()
    components = ops.latent_project(G.x, G.mean, w2)
    k = components.abs().argmax(dim=1, keepdim=True)
    sign = torch.sign(components.gather(1, k)).squeeze(1)
    sign = torch.where(sign == 0, torch.ones_like(sign), sign)
    components = components * sign[:, None]
    scores = (scores * sign.double()[None, :]).float()
    return PCA2D(scores, components, lam / (N - 1), residuals, n_iter)


def _check_tsne(N, perplexity):
    if N > TSNE_MAX_N:
        raise ValueError(f"tsne_2d holds the exact N x N problem on the device: N = {N} exceeds "
                         f"{TSNE_MAX_N}")
    if not perplexity > 0:
        raise ValueError("perplexity must be positive")
    if perplexity >= N:
        raise ValueError(f"perplexity ({perplexity}) must be less than n_samples ({N})")


def tsne_2d(latents_or_gram, perplexity=30.0, max_iter=1000, init=None):
    """TSNE2D(y [N, 2], kl_divergence, n_iter): scikit-learn's TSNE(method='exact') restated on the
    device.  init: None = the PCA scores scaled so that column 0 has standard deviation 1e-4
    (init='pca'), or an [N, 2] array used as it is.  learning rate max(N / 12 / 4, 50); 250
    iterations with the exaggeration and momentum 0.5, then momentum 0.8 up to max_iter; the error
    and the gradient norm are read back every 50 iterations only, with scikit-learn's stopping
    rules (no progress in 250 / 300 iterations, gradient norm <= 1e-7).  max_iter >= 250, as
    scikit-learn requires."""
    if max_iter < 250:
        raise ValueError("max_iter should be at least 250")
    if isinstance(latents_or_gram, LatentGram):
        N = latents_or_gram.g.shape[0]
    else:
        N = _shape_of(latents_or_gram)[0]
    _check_tsne(N, perplexity)
    if init is not None and tuple(getattr(init, "shape", ())) != (N, 2):
        raise ValueError("init must be an [N, 2] array")
    G = _as_gram(latents_or_gram)
    g = G.g
    if init is None:
        s = pca_2d(G).scores.double()
        y0 = s / s[:, 0].std(unbiased=False) * 1e-4
    else:
        y0 = torch.as_tensor(init).to(g.device)
    p, _ = ops.tsne_joint_p(g, perplexity)
    state = torch.zeros((2, N, 6), dtype=torch.float32, device=g.device)
    state[0, :, :2] = y0.float()
    state[0, :, 4:] = 1.0
    rows = torch.empty((N, 8), dtype=torch.float32, device=g.device)
    stats = torch.zeros(2, dtype=torch.float64, device=g.device)
    lr = max(N / 12.0 / 4.0, 50.0)
    cur = 0

    def descend(it, stop, momentum, exaggeration, patience):
        # sklearn.manifold._t_sne._gradient_descent, n_iter_check = 50
        nonlocal cur
        error, best_error, best_iter, i = math.inf, math.inf, it, it
        for i in range(it, stop):
            check = (i + 1) % 50 == 0
            want = check or i == stop - 1
            ops.tsne_step(p, state[cur], state[1 - cur], rows, exaggeration, momentum, lr,
                          stats=stats if want else None)
            cur = 1 - cur
            if want:
                error, grad_norm = stats.tolist()
            if check:
                if error < best_error:
                    best_error, best_iter = error, i
                elif i - best_iter > patience:
                    break
                if grad_norm <= 1e-7:
                    break
        return error, i

    kl, it = descend(0, 250, 0.5, 12.0, 250)
    if it < 250 or max_iter > 250:
        kl, it = descend(it + 1, max_iter, 0.8, 1.0, 300)
    return TSNE2D(state[cur, :, :2].clone(), kl, it)


def pixel_centres(coords, size):
    """int32 [N, 2] pixel centres (x, y) of the coordinates on an H x W canvas: per axis the range
    [min, max] widened by 5 % on each side maps to the canvas, the second axis pointing up;
    rounded to the nearest pixel (ties to even)."""
    H, W = int(size[0]), int(size[1])
    c = torch.as_tensor(coords).double()
    lo, hi = c.min(dim=0).values, c.max(dim=0).values
    span = torch.where(hi > lo, hi - lo, torch.ones_like(hi))
    t = (c - (lo - 0.05 * span)) / (1.1 * span)
    x = torch.round(t[:, 0] * (W - 1))
    y = torch.round((1.0 - t[:, 1]) * (H - 1))
    return torch.stack([x, y], dim=1).to(torch.int32)


def _palette(palette):
    pal = np.asarray(VIRIDIS3 if palette is None else palette)
    if pal.ndim != 2 or pal.shape[1] != 3 or not 1 <= pal.shape[0] <= 256 or \
            pal.min() < 0 or pal.max() > 255:
        raise ValueError("palette must be [K, 3] bytes, K in 1..256")
    return pal.astype(np.uint8)


def _labels(labels, n, k):
    lab = torch.as_tensor(labels).reshape(-1)
    if lab.numel() != n:
        raise ValueError(f"expected {n} labels, got {lab.numel()}")
    if lab.is_floating_point():
        raise TypeError("labels must be integers")
    if n and (int(lab.min()) < 0 or int(lab.max()) >= k):
        raise ValueError(f"a label lies outside the palette (0..{k - 1}): "
                         f"{int(lab.min())}..{int(lab.max())}")
    return lab.to(torch.uint8)


def scatter_figure(coords, labels, size=(600, 800), radius=4, palette=None):
    """uint8 [H, W, 3] on the device: the points as discs of `radius` pixels on a white ground,
    coloured by label and blended in index order with alpha = 0.7 (plt.scatter(..., c=labels,
    alpha=0.7) of the reference).  palette: [K, 3] bytes, by default viridis at 0, 0.5 and 1 for
    the labels 0 / 1 / 2; a label outside the palette raises."""
    n = _shape_of(coords)[0]
    if _shape_of(coords)[1] != 2:
        raise ValueError("coords must be [N, 2]")
    pal = _palette(palette)
    lab = _labels(labels, n, pal.shape[0])
    c = torch.as_tensor(coords)
    if not c.is_cuda:
        c = c.to("cuda")
    centres = pixel_centres(c, size).contiguous()
    return ops.latent_scatter(centres, lab.to(c.device), torch.from_numpy(pal).to(c.device), size,
                              radius)


def visualize_latent_space(latents, labels, save_path, method="pca", perplexity=30.0):
    """utils/visualize.py:179 of the reference: reduce the codes [N, D] (numpy or torch) to 2-D
    with 'pca' or 'tsne' and write the scatter picture coloured by label as a PNG.  `latents` may
    be a `LatentGram`.  Returns the PCA2D / TSNE2D result."""
    m = method.lower()
    if m not in ("pca", "tsne"):
        raise ValueError(f"Unknown method '{method}'. Use 'pca' or 'tsne'.")
    from .render import write_png
    n = latents.g.shape[0] if isinstance(latents, LatentGram) else _shape_of(latents)[0]
    _labels(labels, n, len(VIRIDIS3))             # refuse bad labels before the reduction
    if m == "pca":
        result = pca_2d(latents)
        coords = result.scores
    else:
        result = tsne_2d(latents, perplexity=perplexity)
        coords = result.y
    write_png(save_path, scatter_figure(coords, labels))
    return result
