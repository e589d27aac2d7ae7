"""Writes tests/golden/latent.npz and tests/golden/latent.md: the fixture of the latent-space
analysis (`ua.latent`), recorded on the CPU from scikit-learn and matplotlib (Agg) and from the
reference's own `visualize_latent_space`.

    python tests/tools/make_golden_latent.py --reference /path/to/UNet-Implementations

The fixture stores seeds, not inputs (`latent_ref.codes`), and per shape of `latent_ref.SHAPES`:
  (a) what the reference's visualize_latent_space(method='pca') hands to plt.scatter;
  (b) PCA(2, svd_solver='full') of the fp64 codes: scores, components, variances;
  (c) scikit-learn's _joint_probabilities of the fp64 squared distances (condensed, fp32);
  (d) for the base shape, five states (Y, update, gains) of the descent with scikit-learn's own
      _kl_divergence as the objective, each with the fp64 result of one more iteration;
  (e) kl_divergence_ of TSNE(method='exact') from the scaled PCA scores and three perturbed starts;
  (f) raster cases with their pictures;
and the bounds tests/test_latent_gpu.py holds the kernels to: for every compared quantity, the
distance of the fp32 restatement of the same formula (`latent_ref`, dtype=float32) from the fp64
record, times 4 for another summation order.  None comes from the code under test."""
import argparse
import importlib.util
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import latent_ref as R  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(HERE), "golden")
F32, F64 = np.float32, np.float64


def reference_scatter_arrays(reference, x, labels):
    """(a): run the reference's visualize_latent_space with plt.scatter patched to keep its
    arguments."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    path = os.path.join(reference, "AE_pretrained", "reconstruction", "utils", "visualize.py")
    spec = importlib.util.spec_from_file_location("reference_visualize", path)
    mod = importlib.util.module_from_spec(spec)
    try:
        import cv2  # noqa: F401
    except ImportError:       # the module imports OpenCV for its other figures; this one needs none
        import types
        sys.modules["cv2"] = types.ModuleType("cv2")
    spec.loader.exec_module(mod)
    kept = {}
    real = plt.scatter

    def scatter(xs, ys, *a, **k):
        kept["x"], kept["y"] = np.array(xs, dtype=F64), np.array(ys, dtype=F64)
        kept["alpha"] = k.get("alpha")
        return real(xs, ys, *a, **k)
    plt.scatter = mod.plt.scatter = scatter
    try:
        with tempfile.TemporaryDirectory() as tmp:
            mod.visualize_latent_space(x, labels, os.path.join(tmp, "pca.png"), method="pca")
    finally:
        plt.scatter = mod.plt.scatter = real
    assert kept["alpha"] == 0.7
    return np.stack([kept["x"], kept["y"]], axis=1)


def rel(a, b):
    return float(np.abs(np.asarray(a, F64) - np.asarray(b, F64)).max() / np.abs(b).max())


def up_to_sign(a, b):
    """max |a s - b| / max |b| with the best sign per column."""
    return max(min(rel(a[:, c], b[:, c]), rel(-a[:, c], b[:, c])) for c in range(b.shape[1]))


def sklearn_objective_descent(P_condensed, n, start, stop, momentum, lr, keep, state):
    """_gradient_descent restated around scikit-learn's own _kl_divergence, state in fp32 as
    scikit-learn holds it; `keep[i]` receives (Y, update, gains) in front of iteration i."""
    from sklearn.manifold._t_sne import _kl_divergence
    p, update, gains = state
    for i in range(start, stop):
        if i in keep:
            keep[i] = (p.reshape(n, 2).copy(), update.reshape(n, 2).copy(),
                       gains.reshape(n, 2).copy())
        _, grad = _kl_divergence(p, P_condensed, 1, n, 2, compute_error=False)
        inc = update * grad < 0.0
        gains[inc] += 0.2
        gains[~inc] *= 0.8
        np.clip(gains, 0.01, np.inf, out=gains)
        grad *= gains
        update = momentum * update - lr * grad
        p += update
    return p, update, gains


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    import sklearn
    from scipy.spatial.distance import squareform
    from sklearn.decomposition import PCA
    from sklearn.manifold import TSNE
    from sklearn.manifold._t_sne import _gradient_descent, _joint_probabilities, _kl_divergence
    from sklearn.manifold._utils import _binary_search_perplexity

    out, md = {"sklearn_version": np.array(sklearn.__version__)}, []
    margins = {}
    drawn = R.all_codes()
    out["stream_seed"] = np.array(R.STREAM_SEED)
    for name, n, d, scale, perps in R.SHAPES:
        x, labels = drawn[name]
        # (b) and (a)
        pca = PCA(2, svd_solver="full").fit(x.astype(F64))
        scores = pca.transform(x.astype(F64))
        comp, var = pca.components_, pca.explained_variance_
        ref_xy = reference_scatter_arrays(args.reference, x, labels)
        ab = up_to_sign(ref_xy, scores)
        assert ab <= 1e-5, (name, ab)
        a = np.sort(np.abs(comp), axis=1)
        margins[name] = float((a[:, -2] / a[:, -1]).max())
        out[f"{name}_scatter_xy"] = ref_xy.astype(F32)
        out[f"{name}_scores"], out[f"{name}_components"], out[f"{name}_variances"] = scores, comp, var
        # the restatement, fp64 and fp32
        s64, c64, v64, res64, it64 = R.pca_dual(x, F64)
        s32, c32, v32, res32, it32 = R.pca_dual(x, F32)
        # the iteration stops at a residual of 1e-5: the vectors are good to that over the gap
        assert rel(s64, scores) <= 2e-5 and rel(c64, comp) <= 2e-5, (name, rel(s64, scores))
        assert res32.max() <= 1e-5 and it32 <= 50, (name, res32, it32)
        g64, g32 = R.gram(x, F64), R.gram(x, F32)
        d64, d32 = R.sqdist(g64), R.sqdist(g32)
        b = {"gram": 4 * rel(g32, g64), "dist": 4 * rel(d32, d64),
             "scores": 4 * rel(s32, scores), "components": 4 * rel(c32, comp),
             "variances": 4 * rel(v32, var)}
        md.append(f"| {name} {n} x {d}" + (f" x{scale:g}" if scale != 1 else "") +
                  f" | (a) vs (b) {ab:.1e}; sign margin {margins[name]:.4f}; dual PCA fp32 "
                  f"{it32} iterations, residuals {res32.max():.1e} |")
        # (c)
        for perp in perps:
            tag = f"{name}_p{int(perp)}"
            Pc = _joint_probabilities(d64, perp, 0)
            P64 = squareform(Pc)
            mine = R.joint_p(R.cond_p(d64.astype(F32), perp, F64))
            p32 = R.joint_p(R.cond_p(d32, perp, F32))
            out[f"{tag}_P"] = Pc.astype(F32)
            out[f"{tag}_rowsum"] = P64.sum(axis=1)
            b[f"P_p{int(perp)}"] = 4 * rel(p32, P64)
            b[f"P_rowsum_p{int(perp)}"] = 4 * rel(p32.astype(F64).sum(axis=1), P64.sum(axis=1))
            # how far the rows' entropies end from log(perplexity): scikit-learn's unshifted search
            # loses its bracket where exp(-d beta) underflows on the way (far points, low perplexity)
            def miss(pc):
                with np.errstate(divide="ignore", invalid="ignore"):
                    h = -np.where(pc > 0, pc * np.log(pc), 0).sum(axis=1)
                return float(np.abs(h - np.log(perp)).max())
            own = _binary_search_perplexity(d64.astype(F32), perp, 0)
            md.append(f"| {tag} | restatement (fp64, shifted) vs scikit-learn {rel(mine, P64):.1e}; "
                      f"fp32 restatement vs scikit-learn {rel(p32, P64):.1e}; rows miss the entropy "
                      f"by {miss(own):.1e} (scikit-learn), "
                      f"{miss(R.cond_p(d64.astype(F32), perp, F64)):.1e} (restatement) |")
        for k, v in b.items():
            out[f"{name}_bound_{k}"] = np.array(v)
    sign_shape = min(margins, key=margins.get)
    assert margins[sign_shape] <= 0.99, margins
    out["sign_shape"] = np.array(sign_shape)

    # (d), (e): the base shape
    name, n, d, scale, _ = R.SHAPES[0]
    x, labels = drawn[name]
    Pc = _joint_probabilities(R.sqdist(R.gram(x, F64)), 30.0, 0)
    P64 = squareform(Pc)
    init = R.scaled_init(out[f"{name}_scores"])
    lr = R.learning_rate(n)
    # the restated loop against scikit-learn's own _gradient_descent, 20 iterations, both forms
    kw = dict(it=0, max_iter=20, n_iter_check=50, momentum=0.5, learning_rate=lr,
              args=[Pc * 12.0, 1, n, 2], kwargs=dict(skip_num_points=0))
    p_sk, _, _ = _gradient_descent(_kl_divergence, init.ravel().copy(), **kw)
    p_me, _, _ = sklearn_objective_descent(Pc * 12.0, n, 0, 20, 0.5, lr, {},
                                           (init.ravel().copy(), np.zeros(2 * n, F32),
                                            np.ones(2 * n, F32)))
    assert np.array_equal(p_sk, p_me), np.abs(p_sk - p_me).max()
    p_sk64, _, _ = _gradient_descent(_kl_divergence, init.astype(F64).ravel().copy(), **kw)
    st = dict(y=init.astype(F64), update=np.zeros((n, 2)), gains=np.ones((n, 2)))
    for _ in range(20):
        st = R.tsne_step(P64, st["y"], st["update"], st["gains"], 12.0, 0.5, lr)
    loop = rel(st["y"].ravel(), p_sk64)
    assert loop <= 1e-8, loop
    md.append(f"| descent | latent_ref.tsne_step x 20 vs scikit-learn's _gradient_descent (fp64) "
              f"{loop:.1e} |")

    keep = {i: None for i in R.STATE_ITERS}
    state = (init.ravel().copy(), np.zeros(2 * n, F32), np.ones(2 * n, F32))
    state = sklearn_objective_descent(Pc * 12.0, n, 0, 250, 0.5, lr, keep, state)
    sklearn_objective_descent(Pc, n, 250, max(R.STATE_ITERS) + 1, 0.8, lr, keep, state)
    for i in R.STATE_ITERS:
        y, u, gn = keep[i]
        e, mom = (12.0, 0.5) if i < 250 else (1.0, 0.8)
        r64 = R.tsne_step(P64, y, u, gn, e, mom, lr, F64)
        r32 = R.tsne_step(P64.astype(F32), y, u, gn, e, mom, lr, F32)
        ug = np.abs(u.astype(F64) * r64["grad"])
        mask = ug < 1e-6 * ug.max()
        assert mask.mean() <= 0.02, (i, mask.mean())
        okm = ~mask
        assert np.abs(r32["gains"][okm] - r64["gains"][okm]).max() <= 1e-6, i
        out[f"state{i}_in"] = np.stack([y, u, gn]).astype(F32)
        out[f"state{i}_out"] = np.stack([r64["y"], r64["update"], r64["gains"]])
        out[f"state{i}_scalars"] = np.array([r64["kl"], r64["grad_norm"], e, mom, lr])
        out[f"state{i}_mask"] = mask
        bounds = [4 * float(np.abs(r32[k][okm] - r64[k][okm]).max() / np.abs(r64[k]).max())
                  for k in ("y", "update", "gains")]
        bounds += [4 * abs(r32["kl"] - r64["kl"]) / abs(r64["kl"]),
                   4 * abs(r32["grad_norm"] - r64["grad_norm"]) / r64["grad_norm"]]
        out[f"state{i}_bounds"] = np.array(bounds)
        md.append(f"| state {i} | excluded {mask.sum()} of {mask.size}; 4 x fp32 restatement: Y "
                  f"{bounds[0]:.1e}, update {bounds[1]:.1e}, gains {bounds[2]:.1e}, KL "
                  f"{bounds[3]:.1e}, gradient norm {bounds[4]:.1e} |")

    kls = []
    rng = np.random.Generator(np.random.PCG64(100))
    for k in range(4):
        start = init if k == 0 else \
            (init.astype(F64) * (1 + 1e-7 * rng.standard_normal(init.shape))).astype(F32)
        t = TSNE(n_components=2, perplexity=30.0, method="exact", init=start, random_state=42)
        t.fit(x)
        kls.append(float(t.kl_divergence_))
    out["tsne_kls"] = np.array(kls)
    md.append("| whole run | kl_divergence_ of TSNE(method='exact'), four starts: " +
              ", ".join(f"{k:.4f}" for k in kls) + " |")

    # (f)
    import matplotlib
    pal = np.array([[round(255 * c) for c in matplotlib.colormaps["viridis"](v)[:3]]
                    for v in (0.0, 0.5, 1.0)], dtype=np.uint8)
    out["palette"] = pal
    rr = np.random.Generator(np.random.PCG64(7))
    H, W = 40, 56
    cases = {
        "overlap": (np.array([[20, 20], [22, 21], [21, 19], [40, 10], [22, 21]]),
                    np.array([0, 1, 2, 1, 0]), 4),
        "edges": (np.array([[0, 0], [W - 1, H - 1], [0, H - 1], [W - 1, 0], [W + 2, 5], [-3, -3]]),
                  np.array([0, 1, 2, 0, 1, 2]), 5),
        "radius1": (np.array([[10, 10], [11, 10], [30, 30]]), np.array([2, 0, 1]), 1),
        "absent_label": (np.stack([rr.integers(0, W, 300), rr.integers(0, H, 300)], axis=1),
                         rr.integers(0, 2, 300) * 2, 3),
    }
    for cname, (centres, lab, radius) in cases.items():
        out[f"raster_{cname}_centres"] = centres.astype(np.int32)
        out[f"raster_{cname}_labels"] = lab.astype(np.uint8)
        out[f"raster_{cname}_radius"] = np.array(radius)
        out[f"raster_{cname}_picture"] = R.raster(centres, lab, pal, (H, W), radius)

    os.makedirs(args.out, exist_ok=True)
    np.savez_compressed(os.path.join(args.out, "latent.npz"), **out)
    with open(os.path.join(args.out, "latent.md"), "w") as f:
        f.write("# tests/golden/latent.npz\n\n"
                "Written by `python tests/tools/make_golden_latent.py --reference <checkout of the "
                f"reference>` with scikit-learn {sklearn.__version__}, NumPy {np.__version__} on "
                "the CPU.  Seeds, not inputs, are stored (`latent_ref.codes`).  Every bound of "
                "tests/test_latent_gpu.py is 4 x the distance of the fp32 NumPy restatement of the "
                "same formula (`tests/tools/latent_ref.py`, dtype=float32) from the fp64 record; "
                f"the sign rule is checked on the shape `{sign_shape}`.  Stream seed 0 was tried "
                "first and refused by the generator's own assert (a point in flight at iteration "
                "600 put 4.7 % of the elements under the gain-branch threshold, over the 2 % cap); "
                f"seed {R.STREAM_SEED} passes every assert.  A second run reproduces every array "
                "except `*_scatter_xy`: the reference's PCA picks the randomized solver, whose "
                "last digits differ run to run.\n\n"
                "## What the generator measured\n\n| what | figures |\n|---|---|\n" +
                "\n".join(md) + "\n\n## Bounds (4 x fp32 restatement)\n\n| key | bound |\n|---|---|\n" +
                "\n".join(f"| {k} | {float(v):.2e} |" for k, v in sorted(out.items())
                          if "_bound_" in k) + "\n")
    for line in md:
        print(line)


if __name__ == "__main__":
    main()
