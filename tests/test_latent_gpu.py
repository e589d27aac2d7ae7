"""GPU (-m gpu): the latent-space analysis kernels (csrc/latent.hip) and `ua.latent` against the
fixture tests/golden/latent.npz (scikit-learn 1.7.2 and the reference, recorded by
tests/tools/make_golden_latent.py) and the fp64 restatement of tests/tools/latent_ref.py.

Bounds.  Every `*_bound_*` / `state*_bounds` entry of the fixture is 4 x the distance of the fp32
NumPy restatement of the same formula from the fp64 record (4 for another summation order),
measured by the generator and listed in tests/golden/latent.md; none comes from the kernels.
The shapes (latent_ref.SHAPES): 192 x 2048 the base case; 150 x 1028 a ragged tile and a ragged
last 32-deep chunk; 96 x 8192 more than one slab of D; 192 x 2048 scaled by 30, where exp of the
raw distances underflows.  One descent step is compared from five recorded states; elements whose
fp64 |update grad| lies below 1e-6 of its maximum may take the other gain branch and are left out
of the Y / update / gains comparison (the fixture's mask, at most 2 % per state).  Free-running
trajectories are not compared: fp32 and fp64 part ways within 20 iterations of the 1e-4 start."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
F64 = np.float64


def _load(name):
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(ROOT, "tests", "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load("latent_ref")
NAMES = [s[0] for s in R.SHAPES]


@pytest.fixture(scope="module")
def fx(golden):
    return golden("latent")


@functools.lru_cache(maxsize=None)
def drawn():
    return R.all_codes()          # shared by the tests: nothing writes to it


@functools.lru_cache(maxsize=None)
def device_gram(name):
    """LatentGram of a shape, computed once and shared (nothing writes to it)."""
    import unet_implementations_amd as ua
    return ua.latent.gram(torch.from_numpy(drawn()[name][0]).to(DEV))


@functools.lru_cache(maxsize=None)
def gram64(name):
    return R.gram(drawn()[name][0], F64)


def rel(a, b):
    return float(np.abs(np.asarray(a, F64) - np.asarray(b, F64)).max() / np.abs(b).max())


def host(t):
    return t.detach().cpu().numpy().astype(F64)


@pytest.mark.parametrize("name", NAMES)
def test_gram_and_distances_against_fp64(ua, fx, name):
    x = drawn()[name][0]
    G = device_gram(name)
    n, d = x.shape
    assert rel(host(G.mean), x.astype(F64).mean(axis=0)) <= 1e-6
    g = G.g.cpu().numpy()
    err = rel(g, gram64(name))
    print(f"{name}: gram {err:.2e} (bound {float(fx[name + '_bound_gram']):.2e})")
    assert err <= float(fx[f"{name}_bound_gram"])
    derr = rel(R.sqdist(g), R.sqdist(gram64(name)))       # fp32, the kernel's expression
    print(f"{name}: distances {derr:.2e} (bound {float(fx[name + '_bound_dist']):.2e})")
    assert derr <= float(fx[f"{name}_bound_dist"])
    assert torch.equal(G.g, G.g.T)
    again = ua.ops.latent_gram(G.x, ua.ops.latent_col_mean(G.x))
    assert torch.equal(again, G.g)
    slabs = ua.ops.latent_gram_splitk(n, d)
    assert slabs >= 1
    if name == "splitk":
        assert slabs > 1


def test_gram_apply_and_projection_against_fp64(ua):
    G = device_gram("ragged")
    n = G.g.shape[0]
    q = torch.from_numpy(R.hash_block(n)).float().to(DEV)
    z = ua.ops.latent_gram_apply(G.g, q)
    want = host(G.g) @ host(q)
    assert rel(host(z), want) <= 4 * n * 2.0 ** -24
    w = q[:, :2].contiguous()
    v = ua.ops.latent_project(G.x, G.mean, w)
    xc = host(G.x) - host(G.mean)
    wantv = host(w).T @ xc
    assert rel(host(v), wantv) <= 4 * n * 2.0 ** -24
    assert torch.equal(ua.ops.latent_gram_apply(G.g, q), z)
    assert torch.equal(ua.ops.latent_project(G.x, G.mean, w), v)


@pytest.mark.parametrize("name", NAMES)
def test_pca_against_scikit_learn(ua, fx, name):
    res = ua.latent.pca_2d(device_gram(name))
    scores, comp, var = host(res.scores), host(res.components), host(res.explained_variance)
    assert max(res.residuals) <= 1e-5 and res.n_iter <= 50
    want_s, want_c = fx[f"{name}_scores"], fx[f"{name}_components"]
    for c in range(2):
        s = 1.0
        if name != str(fx["sign_shape"]):       # elsewhere the rule's margin is below fp32 noise
            s = np.sign(np.dot(scores[:, c], want_s[:, c]))
        es, ec = rel(s * scores[:, c], want_s[:, c]), rel(s * comp[c], want_c[c])
        print(f"{name} component {c}: scores {es:.2e}, axis {ec:.2e}")
        assert es <= float(fx[f"{name}_bound_scores"])
        assert ec <= float(fx[f"{name}_bound_components"])
        k = np.abs(comp[c]).argmax()
        assert comp[c, k] > 0                   # svd_flip(u_based_decision=False)
    ev = rel(var, fx[f"{name}_variances"])
    print(f"{name}: variances {ev:.2e}")
    assert ev <= float(fx[f"{name}_bound_variances"])


@pytest.mark.parametrize("name,perp", [(s[0], p) for s in R.SHAPES for p in s[4]])
def test_joint_probabilities_against_scikit_learn(ua, fx, name, perp):
    G = device_gram(name)
    n = G.g.shape[0]
    p, pc = ua.ops.tsne_joint_p(G.g, perp)
    want = R.squareform_f32(fx[f"{name}_p{int(perp)}_P"], n).astype(F64)
    got = host(p)
    err = rel(got, want)
    print(f"{name} perplexity {perp}: P {err:.2e}")
    assert err <= float(fx[f"{name}_bound_P_p{int(perp)}"])
    rs = rel(got.sum(axis=1), fx[f"{name}_p{int(perp)}_rowsum"])
    assert rs <= float(fx[f"{name}_bound_P_rowsum_p{int(perp)}"])
    assert torch.equal(p, p.T) and not p.diagonal().any()
    assert not pc.diagonal().any() and rel(host(pc).sum(axis=1), np.ones(n)) <= 1e-6
    p2, _ = ua.ops.tsne_joint_p(G.g, perp)
    assert torch.equal(p2, p)


@pytest.mark.parametrize("it", R.STATE_ITERS)
def test_one_step_from_each_recorded_state(ua, fx, it):
    n = fx[f"state{it}_in"].shape[1]
    P = torch.from_numpy(R.squareform_f32(fx["base_p30_P"], n)).to(DEV)
    y, u, g = fx[f"state{it}_in"]
    kl, gnorm, e, mom, lr = fx[f"state{it}_scalars"]
    state_in = torch.from_numpy(np.concatenate([y, u, g], axis=1)).to(DEV)
    state_out = torch.empty_like(state_in)
    rows = torch.empty((n, 8), device=DEV)
    stats = torch.zeros(2, dtype=torch.float64, device=DEV)
    ua.ops.tsne_step(P, state_in, state_out, rows, e, mom, lr, stats=stats)
    out = host(state_out)
    keep = ~fx[f"state{it}_mask"]
    assert fx[f"state{it}_mask"].mean() <= 0.02
    bounds = fx[f"state{it}_bounds"]
    got_kl, got_norm = stats.tolist()
    errs = []
    for k, want in enumerate(fx[f"state{it}_out"]):
        gotk = out[:, 2 * k:2 * k + 2]
        errs.append(float(np.abs(gotk[keep] - want[keep]).max() / np.abs(want).max()))
    errs += [abs(got_kl - kl) / abs(kl), abs(got_norm - gnorm) / gnorm]
    print(f"state {it}: Y, update, gains, KL, norm " + ", ".join(f"{v:.2e}" for v in errs) +
          " (bounds " + ", ".join(f"{v:.2e}" for v in bounds) + ")")
    for v, b in zip(errs, bounds):
        assert v <= b
    # without the statistics the step is the same
    other = torch.empty_like(state_in)
    ua.ops.tsne_step(P, state_in, other, rows, e, mom, lr)
    assert torch.equal(other, state_out)


def test_whole_run_reaches_scikit_learns_divergence(ua, fx):
    G = device_gram("base")
    n = G.g.shape[0]
    res = ua.latent.tsne_2d(G, perplexity=30.0)
    P = R.squareform_f32(fx["base_p30_P"], n).astype(F64)
    kl = R.kl_divergence(P, host(res.y))
    kls = fx["tsne_kls"]
    print(f"KL {kl:.4f} (returned {res.kl_divergence:.4f}, {res.n_iter} iterations); "
          f"scikit-learn {kls.min():.4f} .. {kls.max():.4f}")
    assert kl <= kls.max() + (kls.max() - kls.min())
    assert abs(res.kl_divergence - kl) <= 1e-3 * kl
    assert 250 < res.n_iter <= 999
    again = ua.latent.tsne_2d(G, perplexity=30.0)
    assert torch.equal(again.y, res.y) and again.n_iter == res.n_iter


@pytest.mark.parametrize("case", ["overlap", "edges", "radius1", "absent_label"])
def test_raster_is_bit_exact(ua, fx, case):
    pic = fx[f"raster_{case}_picture"]
    out = ua.ops.latent_scatter(torch.from_numpy(fx[f"raster_{case}_centres"]).to(DEV),
                                torch.from_numpy(fx[f"raster_{case}_labels"]).to(DEV),
                                torch.from_numpy(fx["palette"]).to(DEV), pic.shape[:2],
                                int(fx[f"raster_{case}_radius"]))
    assert np.array_equal(out.cpu().numpy(), pic)


def test_scatter_figure_more_points_than_one_pass(ua, fx):
    rng = np.random.Generator(np.random.PCG64(11))
    coords = rng.standard_normal((700, 2))
    labels = rng.integers(0, 3, 700)
    got = ua.latent.scatter_figure(coords, labels, size=(90, 130), radius=3)
    want = R.raster(R.pixel_centres(coords, (90, 130)), labels, fx["palette"], (90, 130), 3)
    assert np.array_equal(got.cpu().numpy(), want)


def test_analyze_latent_space_end_to_end(ua, tmp_path):
    render_ref = _load("render_ref")
    torch.manual_seed(0)
    model = ua.ae.create_model(DEV)
    g = torch.Generator().manual_seed(5)

    class Loader(list):
        dataset = range(12)

    imgs = [torch.rand(4, 3, 64, 64, generator=g) for _ in range(3)]
    labels = [torch.tensor([0, 1, 2, 1]), torch.tensor([2, 2, 0, 1]), torch.tensor([0, 0, 1, 2])]
    loader = Loader([{"image": i, "target": i, "label": l} for i, l in zip(imgs, labels)])
    res = ua.ae.analyze_latent_space(model, loader, DEV, tmp_path, perplexity=3.0)
    out = tmp_path / "latent_analysis"
    assert sorted(os.listdir(out)) == ["latent_space_pca.png", "latent_space_tsne.png"]
    for name in os.listdir(out):
        assert render_ref.read_png(str(out / name)).shape == (600, 800, 3)
    assert res["num_samples"] == 12 and tuple(res["pca"].shape) == tuple(res["tsne"].shape) == (12, 2)
    assert max(res["pca_residuals"]) <= 1e-5 and res["kl_divergence"] > 0 and res["n_iter"] <= 999
    assert torch.equal(res["labels"].cpu(), torch.cat(labels))
    model.eval()
    with torch.no_grad():
        codes = torch.cat([model.encode(i.to(DEV)) for i in imgs])
        whole = model.encode(torch.cat(imgs).to(DEV))
    assert torch.equal(ua.latent.pca_2d(codes).scores, res["pca"])
    both = host(ua.latent.pca_2d(whole).scores)
    for c in range(2):
        s = np.sign(np.dot(both[:, c], host(res["pca"])[:, c]))
        assert rel(s * both[:, c], host(res["pca"])[:, c]) <= 1e-3
    # the picture is the raster of the returned coordinates
    want = R.raster(R.pixel_centres(host(res["pca"]), (600, 800)), torch.cat(labels).numpy(),
                    np.array(ua.latent.VIRIDIS3), (600, 800), 4)
    assert np.array_equal(render_ref.read_png(str(out / "latent_space_pca.png")), want)
    bare = Loader([{"image": imgs[0], "target": imgs[0]}])
    with pytest.raises(KeyError, match="mask.max"):
        ua.ae.analyze_latent_space(model, bare, DEV, tmp_path / "bare")
