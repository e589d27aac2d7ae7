"""CPU (-m "not gpu"): the latent-space analysis (`ua.latent`, csrc/latent.hip) without a device.

The NumPy restatement of tests/tools/latent_ref.py reproduces the fixture tests/golden/latent.npz
(recorded from scikit-learn and the reference by tests/tools/make_golden_latent.py): the PCA scores
up to the recorded sign, the joint probabilities, one descent step from every recorded state, the
raster pictures.  `ua.latent` refuses what it cannot do before it touches a device; the header
declares the entry points and the built object passes the register / hazard checks."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import latent_ref as R  # noqa: E402

HEADER = os.path.join(ROOT, "include", "unet_hip.h")
EXPORTS = ("unet_latent_col_mean", "unet_latent_project", "unet_latent_gram",
           "unet_latent_gram_apply", "unet_tsne_cond_p", "unet_tsne_joint_p", "unet_tsne_step",
           "unet_latent_scatter")


@pytest.fixture(scope="module")
def fx(golden):
    return golden("latent")


@pytest.fixture(scope="module")
def drawn():
    return R.all_codes()


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() /
                 np.abs(b).max())


def test_fixture_metadata(fx):
    assert str(fx["sklearn_version"]) == "1.7.2"
    assert int(fx["stream_seed"]) == R.STREAM_SEED
    assert str(fx["sign_shape"]) in [s[0] for s in R.SHAPES]
    md = open(os.path.join(ROOT, "tests", "golden", "latent.md")).read()
    assert "make_golden_latent.py --reference" in md
    for name, *_ in R.SHAPES:
        for key in ("gram", "dist", "scores", "components", "variances", "P_p30"):
            assert f"{name}_bound_{key}" in md and float(fx[f"{name}_bound_{key}"]) > 0


@pytest.mark.parametrize("name", [s[0] for s in R.SHAPES])
def test_restated_pca_reproduces_the_recorded_scores(fx, drawn, name):
    x, _ = drawn[name]
    scores, comp, var, res, it = R.pca_dual(x)
    # the sign rule: the restatement lands on scikit-learn's own sign where the rule has a margin
    if name == str(fx["sign_shape"]):
        assert rel(scores, fx[f"{name}_scores"]) <= 2e-5
        assert rel(comp, fx[f"{name}_components"]) <= 2e-5
    for c in range(2):
        s = np.sign(np.dot(scores[:, c], fx[f"{name}_scores"][:, c]))
        assert rel(s * scores[:, c], fx[f"{name}_scores"][:, c]) <= 2e-5
        assert rel(s * comp[c], fx[f"{name}_components"][c]) <= 2e-5
        # what the reference's own figure plots
        assert rel(s * scores[:, c], fx[f"{name}_scatter_xy"][:, c].astype(np.float64)) <= 2e-5
    assert rel(var, fx[f"{name}_variances"]) <= 1e-8
    assert res.max() <= 1e-5 and it <= 50


@pytest.mark.parametrize("name,perp", [(s[0], p) for s in R.SHAPES for p in s[4]])
def test_restated_joint_probabilities(fx, drawn, name, perp):
    x, _ = drawn[name]
    n = x.shape[0]
    d = R.sqdist(R.gram(x)).astype(np.float32)
    P = R.joint_p(R.cond_p(d, perp))
    want = R.squareform_f32(fx[f"{name}_p{int(perp)}_P"], n).astype(np.float64)
    assert rel(P, want) <= float(fx[f"{name}_bound_P_p{int(perp)}"])
    assert np.array_equal(P, P.T) and not P.diagonal().any()
    assert abs(P.sum() - 1.0) <= n * n * R.EPS + 1e-13       # the floor lifts up to N^2 entries
    assert rel(P.sum(axis=1), fx[f"{name}_p{int(perp)}_rowsum"]) <= \
        float(fx[f"{name}_bound_P_rowsum_p{int(perp)}"])
    # the shifted search reaches the perplexity on every row
    pc = R.cond_p(d, perp)
    with np.errstate(divide="ignore", invalid="ignore"):
        h = -np.where(pc > 0, pc * np.log(pc), 0).sum(axis=1)
    assert np.abs(h - np.log(perp)).max() <= 1.5e-5


@pytest.mark.parametrize("it", R.STATE_ITERS)
def test_restated_step_from_each_state(fx, it):
    n = fx[f"state{it}_in"].shape[1]
    P = R.squareform_f32(fx["base_p30_P"], n).astype(np.float64)
    y, u, g = fx[f"state{it}_in"]
    kl, gnorm, e, mom, lr = fx[f"state{it}_scalars"]
    assert (e, mom) == ((12.0, 0.5) if it < 250 else (1.0, 0.8)) and lr == R.learning_rate(n)
    out = R.tsne_step(P, y, u, g, e, mom, lr)
    wy, wu, wg = fx[f"state{it}_out"]
    # P is stored in fp32: 6e-8 relative per entry
    assert rel(out["y"], wy) <= 1e-6 and rel(out["update"], wu) <= 1e-4
    keep = ~fx[f"state{it}_mask"]
    assert np.abs(out["gains"][keep] - wg[keep]).max() <= 1e-12
    assert fx[f"state{it}_mask"].mean() <= 0.02
    assert abs(out["kl"] - kl) <= 1e-6 * abs(kl) and abs(out["grad_norm"] - gnorm) <= 1e-4 * gnorm


def test_recorded_kl_divergences(fx):
    kls = fx["tsne_kls"]
    assert kls.shape == (4,) and 0.3 < kls.min() <= kls.max() < 0.7


@pytest.mark.parametrize("case", ["overlap", "edges", "radius1", "absent_label"])
def test_restated_raster(fx, case):
    pic = fx[f"raster_{case}_picture"]
    got = R.raster(fx[f"raster_{case}_centres"], fx[f"raster_{case}_labels"], fx["palette"],
                   pic.shape[:2], int(fx[f"raster_{case}_radius"]))
    assert np.array_equal(got, pic)
    assert (pic != 255).any()
    if case == "absent_label":
        assert 1 not in fx[f"raster_{case}_labels"]
    if case == "radius1":      # a radius-1 disc is the plus of five pixels
        lone = pic[28:33, 28:33].astype(int).sum(axis=2) != 765
        assert lone.sum() == 5 and lone[2].sum() == 3 and lone[:, 2].sum() == 3


def test_default_palette_is_viridis(ua, fx):
    assert np.array_equal(np.array(ua.latent.VIRIDIS3, dtype=np.uint8), fx["palette"])


def test_pixel_centres_match_the_restatement(ua):
    import torch
    rng = np.random.Generator(np.random.PCG64(3))
    c = rng.standard_normal((50, 2)) * [3.0, 0.01]
    got = ua.latent.pixel_centres(torch.from_numpy(c), (600, 800)).numpy()
    assert np.array_equal(got, R.pixel_centres(c, (600, 800)))
    assert got.min() >= 0 and got[:, 0].max() <= 799 and got[:, 1].max() <= 599
    assert np.array_equal(ua.latent._hash_block(17, 8), R.hash_block(17, 8))


def test_refusals_before_any_device_work(ua):
    L = ua.latent
    x = np.zeros((20, 8), dtype=np.float32)
    with pytest.raises(ValueError, match="perplexity"):
        L.tsne_2d(x, perplexity=20.0)
    with pytest.raises(ValueError, match="perplexity"):
        L.tsne_2d(x, perplexity=25.0)
    big = np.lib.stride_tricks.as_strided(np.zeros(4, dtype=np.float32), shape=(8193, 4),
                                          strides=(0, 4))
    with pytest.raises(ValueError, match="8192"):
        L.tsne_2d(big, perplexity=30.0)
    coords = np.zeros((5, 2))
    with pytest.raises(ValueError, match="outside the palette"):
        L.scatter_figure(coords, np.array([0, 1, 2, 3, 0]))
    with pytest.raises(ValueError, match="outside the palette"):
        L.scatter_figure(coords, np.array([0, 1, 1, 0, 0]), palette=[(0, 0, 0)])
    with pytest.raises(ValueError, match="outside the palette"):
        L.visualize_latent_space(x, np.full(20, 7), "unused.png")
    with pytest.raises(ValueError, match="Unknown method"):
        L.visualize_latent_space(x, np.zeros(20, dtype=int), "unused.png", method="umap")
    with pytest.raises(ValueError, match="multiple of 4"):
        L.gram(np.zeros((20, 6), dtype=np.float32))
    assert not os.path.exists("unused.png")


def test_header_exports_and_workspace_queries(ua):
    text = open(HEADER).read()
    for name in EXPORTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), f"{name} not declared in unet_hip.h"
    assert "latent.hip" in open(os.path.join(ROOT, "unet-implementations_amd", "csrc",
                                             "Makefile")).read()
    lib = ua.lib()
    assert lib.unet_latent_gram_workspace_bytes(192, 2048) >= 3 * 128 * 128 * 4
    assert lib.unet_latent_gram_workspace_bytes(192, 2046) == 0
    assert lib.unet_latent_gram_splitk(96, 8192) > 1
    assert lib.unet_latent_gram_splitk(3669, 131072) >= 1
    assert lib.unet_latent_colsum_workspace_bytes(150, 1028) >= 2 * 1028 * 4
    # host-side refusals: no launch happens
    assert lib.unet_latent_gram(None, None, None, None, 0, 192, 2048, None) == -1
    assert b"null" in lib.unet_last_error()
    assert lib.unet_latent_gram(16, 16, 16, 16, 1 << 30, 192, 2046, None) == -1
    assert b"multiple of 4" in lib.unet_last_error()
    assert lib.unet_latent_gram(16, 16, 16, 16, 16, 192, 2048, None) == -3
    assert lib.unet_tsne_cond_p(16, 16, 30.0, 16, 16, 8193, None) == -1
    assert lib.unet_tsne_cond_p(16, 16, 30.0, 16, 16, 30, None) == -1
    assert b"perplexity" in lib.unet_last_error()
    assert lib.unet_tsne_step(16, 16, 16, 16, 16, 1.0, 0.5, 50.0, 0, 100, None) == -1
    assert b"differ" in lib.unet_last_error()


def test_latent_object_has_no_scratch_and_no_hazard():
    obj = os.path.join(ROOT, "unet-implementations_amd", "csrc", "build", "latent.o")
    if not os.path.exists(obj):
        pytest.skip("no built objects (run __graft_entry__.build() first)")
    txt = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_regs.sh"), obj],
                         capture_output=True, text=True, check=True).stdout
    rows = re.findall(r"(\S+)\s+vgpr (\d+) agpr (\d+) sgpr \d+ lds \d+ scratch (\d+)", txt)
    assert len(rows) >= 12 and all(int(r[3]) == 0 for r in rows), txt
    gram = [r for r in rows if "gram_kernel" in r[0]]
    assert gram and int(gram[0][2]) == 64, "the Gram kernel keeps 4 x 16 accumulators in AGPRs"
    r = subprocess.run(["python3", os.path.join(ROOT, "tools", "asm_hazard_check.py"), obj],
                       capture_output=True, text=True)
    m = re.search(r"(\d+) kernels checked, (\d+) hazards, (\d+) incomplete", r.stdout)
    assert m and int(m.group(1)) >= 12 and int(m.group(2)) == 0 and int(m.group(3)) == 0, \
        r.stdout[-2000:]
