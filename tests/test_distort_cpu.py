"""CPU (-m "not gpu"): elastic / grid / optical distortion without a device - the ABI surface of
unet_elastic_field / unet_augment_warp_u8 and their host-side argument checks, the warp-record
sampler (`augment.sample_warp`) against the probabilities and limits of the reference's settings
file, `validate_warp`, and the restatements of tests/tools/distort_ref.py against each other on
the very records the GPU test uses."""
import ctypes
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "unet_hip.h")
YAML = os.path.join(ROOT, "tests", "golden", "augmentation_config.yaml")


def _load(name):
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(ROOT, "tests", "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


D = _load("distort_ref")
R = D.R


def test_entry_points_declared_exported_and_bound(ua):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    handle = ctypes.CDLL(ua.LIB_PATH)
    for name in ("unet_augment_warp_params_per_sample", "unet_augment_warp_u8",
                 "unet_elastic_field"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), f"{name} not declared in unet_hip.h"
        assert hasattr(handle, name), f"{name} not exported"
        assert name in ua._lib.SIGNATURES
    assert len(ua._lib.SIGNATURES["unet_augment_warp_u8"][1]) == 12
    assert len(ua._lib.SIGNATURES["unet_elastic_field"][1]) == 7
    assert len(ua._lib.SIGNATURES["unet_augment_u8"][1]) == 10
    assert re.search(r"#define\s+UNET_ABI_VERSION\s+11\b", open(HEADER).read())
    assert ua._lib.ABI_VERSION == 11 and ua.lib().unet_abi_version() == 11
    assert ua.lib().unet_augment_warp_params_per_sample() == 64 == ua.augment.WARP_PER_SAMPLE
    assert ua.lib().unet_augment_params_per_sample() == 24
    for name in ("elastic_field", "augment_warp_u8"):
        assert callable(getattr(ua.ops, name))
    for name in ("sample_warp", "identity_warp", "validate_warp"):
        assert callable(getattr(ua.augment, name))
    assert tuple(ua.augment.identity_warp(3).shape) == (3, 64)
    assert ua.augment.identity_warp(3).dtype == torch.float32
    assert not ua.augment.identity_warp(3).any()


def test_host_arguments_are_rejected_before_any_launch(ua):
    lib = ua.lib()
    A, B, C, D_, P, G, Wp, F_ = (0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000,
                                 0x60000000, 0x70000000, 0x80000000)
    call = lib.unet_augment_warp_u8
    for args in ((None, B, C, D_, P, G, Wp, F_), (A, B, None, D_, P, G, Wp, F_),
                 (A, B, C, D_, None, G, Wp, F_), (A, B, C, D_, P, G, None, F_)):
        assert call(*args, 1, 8, 8, None) == -1 and b"null" in lib.unet_last_error()
    assert call(A, B, C, None, P, G, Wp, F_, 1, 8, 8, None) == -1
    assert b"without mask_out" in lib.unet_last_error()
    for shape in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8), (1, 32769, 8)):
        assert call(A, B, C, D_, P, G, Wp, F_, *shape, None) == -1
        assert b"bad shape" in lib.unet_last_error()
    assert call(A, B, C, D_, P, G, Wp, F_ + 4, 1, 8, 8, None) == -1
    assert b"aligned" in lib.unet_last_error()
    # 2 x 8 x 8: image 384 bytes, mask 128, warp 512, field 1024
    for args in ((A, B, A + 383, D_, P, G, Wp, F_), (A, B, C, B + 127, P, G, Wp, F_),
                 (A, B, Wp + 511, D_, P, G, Wp, F_), (A, B, C, Wp - 127, P, G, Wp, F_),
                 (A, B, F_ + 1023, D_, P, G, Wp, F_), (A, B, C, F_ - 120, P, G, Wp, F_),
                 (A, B, C, C + 8, P, G, Wp, F_)):
        assert call(*args, 2, 8, 8, None) == -1 and b"overlaps" in lib.unet_last_error()

    call = lib.unet_elastic_field
    for args in ((None, Wp, G), (F_, None, G)):
        assert call(*args, 1, 8, 8, None) == -1 and b"null" in lib.unet_last_error()
    for shape in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (65536, 8, 8)):
        assert call(F_, Wp, G, *shape, None) == -1 and b"bad shape" in lib.unet_last_error()
    assert call(F_ + 4, Wp, G, 1, 8, 8, None) == -1 and b"aligned" in lib.unet_last_error()
    for args in ((Wp - 1016, Wp, G), (Wp + 504, Wp, G), (G - 8, Wp, G), (G + 24, Wp, G)):
        assert call(*args, 2, 8, 8, None) == -1 and b"overlaps" in lib.unet_last_error()


def test_python_surface_has_no_cpu_fallback(ua):
    x = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ua.ops.augment_warp_u8(x, None, ua.augment.identity_params(1), None,
                               ua.augment.identity_warp(1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ua.ops.elastic_field(ua.augment.identity_warp(1), None, (8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ua.BatchAugment(ua.AugmentConfig(distort_group_prob=1.0, elastic_prob=1.0))(x)


def test_identity_warp_is_the_plain_restatement(ua):
    N, H, W = 2, 33, 37
    image, mask = R.random_batch(N, H, W, seed=3)
    cfg = ua.AugmentConfig(**{**vars(R.record_configs(ua.augment)["perspective"]),
                              "salt_pepper_prob": 1.0, "salt_p": (0.02, 0.05),
                              "pepper_p": (0.02, 0.05), "dropout_prob": 1.0,
                              "dropout_height": (3, 9), "dropout_width": (3, 9)})
    p, r = ua.augment.sample_params(cfg, N, H, W, torch.Generator().manual_seed(2))
    w = ua.augment.identity_warp(N)
    ua.augment.validate_warp(w, p, H, W)
    o, m = D.augment_warp_f32(image, mask, p.numpy(), r.numpy(), w.numpy())
    o0, m0 = R.augment_f32(image, mask, p.numpy(), r.numpy())
    assert np.array_equal(o, o0) and np.array_equal(m, m0)
    # a field is ignored unless the record says "elastic"
    junk = np.full((N, H, W, 2), 5.0, dtype=np.float32)
    o, m = D.augment_warp_f32(image, mask, p.numpy(), r.numpy(), w.numpy(), junk)
    assert np.array_equal(o, o0) and np.array_equal(m, m0)
    val, o64, m64, _ = D.augment_warp_f64(image, mask, p.numpy(), r.numpy(), w.numpy())
    val0, o640, m640, _ = R.augment_f64(image, mask, p.numpy(), r.numpy())
    assert np.array_equal(val, val0) and np.array_equal(o64, o640) and np.array_equal(m64, m640)


def test_from_yaml_reads_the_group_only_when_asked(ua):
    import yaml
    raw = yaml.safe_load(open(YAML))
    for section in ("cat", "dog"):
        plain = ua.AugmentConfig.from_yaml(YAML, section)
        cfg = ua.AugmentConfig.from_yaml(YAML, section, distortion=True)
        s = raw[section]
        assert cfg.distort_group_prob == s["elastic_transform_prob"] > 0
        assert (cfg.elastic_prob, cfg.elastic_alpha, cfg.elastic_sigma,
                cfg.elastic_alpha_affine) == tuple(
            float(s["elastic"][k]) for k in ("prob", "alpha", "sigma", "alpha_affine"))
        assert (cfg.grid_distortion_prob, cfg.grid_num_steps, cfg.grid_distort_limit) == (
            s["grid_distortion"]["prob"], s["grid_distortion"]["num_steps"],
            s["grid_distortion"]["distort_limit"])
        assert isinstance(cfg.grid_num_steps, int)
        if section == "cat":
            o = s["optical_distortion"]
            assert (cfg.optical_distortion_prob, cfg.optical_distort_limit,
                    cfg.optical_shift_limit) == (o["prob"], o["distort_limit"], o["shift_limit"])
        else:
            assert "optical_distortion" not in s
            assert (cfg.optical_distortion_prob, cfg.optical_distort_limit,
                    cfg.optical_shift_limit) == (0.0, 0.0, 0.0)
        # every geometric group of the file is live
        for name in ("horizontal_flip_prob", "shift_scale_rotate_prob", "crop_prob",
                     "perspective_prob", "dropout_prob", "distort_group_prob", "elastic_prob",
                     "grid_distortion_prob"):
            assert getattr(cfg, name) > 0, name
        # the default: exactly what it returned before the group existed
        names = ("distort_group_prob", "elastic_prob", "elastic_alpha", "elastic_sigma",
                 "elastic_alpha_affine", "grid_distortion_prob", "grid_num_steps",
                 "grid_distort_limit", "optical_distortion_prob", "optical_distort_limit",
                 "optical_shift_limit")
        assert all(getattr(plain, k) == 0 for k in names)
        assert plain == ua.AugmentConfig(**{**vars(cfg), **{k: 0 for k in names}})
        assert plain == ua.AugmentConfig.from_yaml(YAML, section, distortion=False)


def _within(share, p, n, what):
    sd = math.sqrt(p * (1 - p) / n)
    assert abs(share - p) <= 4 * sd, f"{what}: share {share:.4f}, probability {p:.4f}, sd {sd:.4f}"


@pytest.mark.parametrize("section", ["cat", "dog"])
def test_yaml_probabilities_and_limits(ua, section):
    import yaml
    raw = yaml.safe_load(open(YAML))[section]
    cfg = ua.AugmentConfig.from_yaml(YAML, section, distortion=True)
    n, H, W = 20000, 512, 512
    w, ap = ua.augment.sample_warp(cfg, n, H, W, torch.Generator().manual_seed(21),
                                   return_applied=True)
    assert w.dtype == torch.float32 and tuple(w.shape) == (n, 64)
    ua.augment.validate_warp(w, ua.augment.identity_params(n), H, W)
    w = w.numpy().astype(np.float64)
    probs = {"elastic": raw["elastic"]["prob"], "grid_distortion": raw["grid_distortion"]["prob"],
             "optical_distortion": raw.get("optical_distortion", {}).get("prob", 0.0)}
    tot = sum(probs.values())
    assert set(ap) == set(probs)
    for k, prob in probs.items():
        _within(ap[k].mean(), raw["elastic_transform_prob"] * prob / tot, n, f"{section}/{k}")
    fired = ap["elastic"].astype(int) + ap["grid_distortion"] + ap["optical_distortion"]
    assert fired.max() == 1                                             # OneOf
    assert np.array_equal(w[:, 0], 1 * ap["elastic"] + 2 * ap["grid_distortion"]
                          + 3 * ap["optical_distortion"])
    assert (w[fired == 0] == 0).all()

    e = w[ap["elastic"]]
    el = raw["elastic"]
    assert (e[:, 7] == np.float32(el["alpha"])).all()
    rad = min(math.ceil(3 * el["sigma"]), 16)
    assert (e[:, 8] == rad).all()
    g = e[:, 9:26]
    assert (g[:, rad + 1:] == 0).all() and (g[:, :rad + 1] > 0).all()
    assert np.allclose(g[:, 0] + 2 * g[:, 1:].sum(1), 1.0, atol=1e-6)
    assert np.allclose(g[0, 1] / g[0, 0], math.exp(-1 / (2 * el["sigma"] ** 2)), rtol=1e-6)
    assert (np.diff(g[:, :rad + 1], axis=1) < 0).all()
    assert (e[:, 26:] == 0).all()
    # the affine part: the forward map moves each anchor by at most alpha_affine pixels
    q = min(H, W) / 3.0
    anchors = np.array([[W / 2 + q, H / 2 + q], [W / 2 + q, H / 2 - q], [W / 2 - q, H / 2 - q]])
    inv = np.zeros((e.shape[0], 3, 3))
    inv[:, 0], inv[:, 1], inv[:, 2, 2] = e[:, 1:4], e[:, 4:7], 1.0
    fwd = np.linalg.inv(inv)
    moved = np.einsum("nij,kj->nki", fwd, np.concatenate([anchors, np.ones((3, 1))], 1))[..., :2]
    shift = moved - anchors[None]
    assert (np.abs(shift) <= el["alpha_affine"] + 1e-2).all()
    assert np.abs(shift).max() > 0.9 * el["alpha_affine"]                # the range is used

    gr = w[ap["grid_distortion"]]
    K, lim = raw["grid_distortion"]["num_steps"], raw["grid_distortion"]["distort_limit"]
    assert (gr[:, 1] == K).all() and (gr[:, 3] == K).all()
    assert (gr[:, 2] == np.float32(K / W)).all() and (gr[:, 4] == np.float32(K / H)).all()
    assert (gr[:, 5:8] == 0).all() and (gr[:, 40:] == 0).all()
    for a_at, size in ((8, W), (24, H)):
        a, b = gr[:, a_at:a_at + 8], gr[:, a_at + 8:a_at + 16]
        assert (a[:, K:] == 0).all() and (b[:, K:] == 0).all()
        # slope of cell k is s_k / mean(s): within the limits, strictly increasing
        assert (a[:, :K] >= (1 - lim) / (1 + lim) - 1e-6).all()
        assert (a[:, :K] <= (1 + lim) / (1 - lim) + 1e-6).all()
        assert (a[:, :K] > 0).all()
        assert a[:, :K].max() > 1.2 and a[:, :K].min() < 0.85
        knots = size * np.arange(K + 1) / K
        lo = a[:, :K] * knots[None, :K] + b[:, :K]          # value at the left end of each cell
        hi = a[:, :K] * knots[None, 1:] + b[:, :K]          # and at the right end
        assert np.abs(lo[:, 0]).max() <= 1e-4 and np.abs(hi[:, -1] - size).max() <= 1e-3
        assert np.abs(hi[:, :-1] - lo[:, 1:]).max() <= 1e-3             # continuous
        assert (hi > lo).all()

    o = w[ap["optical_distortion"]]
    if section == "cat":
        od = raw["optical_distortion"]
        assert (np.abs(o[:, 3]) <= od["distort_limit"] + 1e-6).all()
        assert np.abs(o[:, 3]).max() > 0.9 * od["distort_limit"]
        assert (np.abs(o[:, 1] - W / 2) <= od["shift_limit"] * W + 1e-3).all()
        assert (np.abs(o[:, 2] - H / 2) <= od["shift_limit"] * H + 1e-3).all()
        assert np.abs(o[:, 1] - W / 2).max() > 0.9 * od["shift_limit"] * W
        assert (o[:, 4] == np.float32(1 / W)).all() and (o[:, 5] == np.float32(1 / H)).all()
        assert (o[:, 6:] == 0).all()
    else:
        assert o.shape[0] == 0


def test_sample_params_is_untouched(ua):
    """The values below were printed by the parent commit's `sample_params` for this seed."""
    cfg = ua.AugmentConfig(
        horizontal_flip_prob=0.5, shift_scale_rotate_prob=1.0, shift_limit=(-0.1, 0.1),
        scale_limit=(-0.15, 0.15), rotate_limit=(-15.0, 15.0), perspective_prob=1.0,
        perspective_scale=(0.05, 0.1), color_prob=1.0, brightness_contrast_prob=1.0,
        brightness_limit=(-0.1, 0.1), contrast_limit=(-0.3, 0.2), noise_group_prob=1.0,
        gauss_noise_prob=1.0, gauss_var_limit=(4.0, 16.0), salt_pepper_prob=1.0,
        salt_p=(0.01, 0.05), pepper_p=(0.01, 0.05))
    want = [float.fromhex(h) for h in (
        "-0x1.90a404p-1", "-0x1.31d724p-5", "0x1.f603ep+4", "0x1.791b6cp-5", "0x1.90f8bep-1",
        "0x1.942188p+1", "0x1.58edfp-8", "-0x1.d4ab0ep-9", "0x1.ec5aa2p-1", "0x1.afbda4p-1",
        "-0x1.133852p+3", "-0x1.133852p+3", "-0x1.133852p+3", "0x0p+0", "0x1.663796p+1")]
    want_rng = [[1147013802, 920218071, 123014303, 210090932],
                [762601684, 1843682066, 127487663, 128026269]]
    for with_group in (False, True):
        c = ua.AugmentConfig(**{**vars(cfg), **({"distort_group_prob": 1.0, "elastic_prob": 1.0}
                                                if with_group else {})})
        gen = torch.Generator().manual_seed(1234)
        p, r = ua.augment.sample_params(c, 2, 33, 37, gen)
        assert p[0, :15].tolist() == want
        assert r.tolist() == want_rng
    # sample_warp draws from a block of its own, after the fact
    g1, g2 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    a = ua.augment.sample_params(cfg, 4, 16, 24, g1)
    ua.augment.sample_warp(ua.AugmentConfig(distort_group_prob=1.0, elastic_prob=1.0), 4, 16, 24,
                           g2)
    b = ua.augment.sample_params(cfg, 4, 16, 24, torch.Generator().manual_seed(5))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(torch.rand(1, generator=g1), torch.rand(1, generator=g2))


def test_which_selects_the_configuration_per_sample(ua):
    cat = ua.AugmentConfig(distort_group_prob=1.0, grid_distortion_prob=1.0, grid_num_steps=5,
                           grid_distort_limit=0.2)
    dog = ua.AugmentConfig(distort_group_prob=1.0, grid_distortion_prob=1.0, grid_num_steps=4,
                           grid_distort_limit=0.15)
    none = ua.AugmentConfig()
    which = torch.tensor([0, 1, 2, 0, 1])
    w = ua.augment.sample_warp([cat, dog, none], 5, 40, 52, torch.Generator().manual_seed(0),
                               which=which)
    assert w[:, 0].tolist() == [2, 2, 0, 2, 2]
    assert w[:, 1].tolist() == [5, 4, 0, 5, 4]
    with pytest.raises(ValueError):
        ua.augment.sample_warp([cat, dog], 5, 40, 52, torch.Generator())


def test_bad_records_are_refused(ua):
    H, W = 40, 52
    good_p = ua.augment.identity_params(2)
    cfg = D.distort_config(ua.augment, 2, (2, H, W), 4.0)
    grid = ua.augment.sample_warp(cfg, 2, H, W, torch.Generator().manual_seed(1))
    ua.augment.validate_warp(grid, good_p, H, W)
    ua.augment.validate_warp(ua.augment.identity_warp(2), good_p, H, W)
    bad = grid.clone()
    bad[1, 9] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        ua.augment.validate_warp(bad, good_p, H, W)
    bad = grid.clone()
    bad[0, 0] = 4.0
    with pytest.raises(ValueError, match="mode"):
        ua.augment.validate_warp(bad, good_p, H, W)
    for at in (1, 3):
        for K in (9.0, 0.0, 2.5):
            bad = grid.clone()
            bad[0, at] = K
            with pytest.raises(ValueError, match="K"):
                ua.augment.validate_warp(bad, good_p, H, W)
    bad = grid.clone()
    bad[1, 8 + 2] = 0.0                                   # a flat cell: not increasing
    with pytest.raises(ValueError, match="increasing"):
        ua.augment.validate_warp(bad, good_p, H, W)
    for limit in (1.0, 1.5, -0.1):
        c = ua.AugmentConfig(distort_group_prob=1.0, grid_distortion_prob=1.0, grid_num_steps=5,
                             grid_distort_limit=limit)
        with pytest.raises(ValueError, match="distort_limit"):
            ua.augment.sample_warp(c, 2, H, W, torch.Generator())
    for steps in (0, 9):
        c = ua.AugmentConfig(distort_group_prob=1.0, grid_distortion_prob=1.0,
                             grid_num_steps=steps, grid_distort_limit=0.2)
        with pytest.raises(ValueError, match="num_steps"):
            ua.augment.sample_warp(c, 2, H, W, torch.Generator())
    with pytest.raises(ValueError):
        ua.augment.validate_warp(torch.zeros(2, 63), good_p, H, W)
    with pytest.raises(ValueError):
        ua.augment.validate_warp(grid, ua.augment.identity_params(3), H, W)

    # den = 1 - x / (W + 6): positive on the output rectangle, and on it grown by < 6 px
    p = good_p.clone()
    p[:, 6], p[:, 8] = -1.0 / (W + 6.0), 1.0
    ua.augment.validate_params(p, H, W)
    ua.augment.validate_warp(grid, p, H, W)               # a grid record reaches nothing outside
    el = ua.augment.identity_warp(2)
    el[:, 0], el[:, 1], el[:, 5], el[:, 8], el[:, 9] = 1.0, 1.0, 1.0, 0.0, 1.0
    el[:, 7] = 5.0
    ua.augment.validate_warp(el, p, H, W)
    el[:, 7] = 6.5                                        # alpha alone carries a pixel past W + 6
    with pytest.raises(ValueError, match="den <= 0"):
        ua.augment.validate_warp(el, p, H, W)
    el[:, 7], el[:, 3] = 5.0, 1.5                         # alpha plus the affine part's shift
    with pytest.raises(ValueError, match="den <= 0"):
        ua.augment.validate_warp(el, p, H, W)
    op = ua.augment.identity_warp(2)
    op[:, 0], op[:, 1], op[:, 2], op[:, 4], op[:, 5] = 3.0, W / 2, H / 2, 1.0 / W, 1.0 / H
    op[:, 3] = 0.2                # corner: r2 = 0.5, |f - 1| = 0.15, extent 26 -> 3.9 px
    ua.augment.validate_warp(op, p, H, W)
    op[:, 3] = 0.4                # 7.8 px
    with pytest.raises(ValueError, match="den <= 0"):
        ua.augment.validate_warp(op, p, H, W)
    for bad_alpha, bad_r in ((-1.0, 2.0), (1.0, 17.0), (1.0, 1.5)):
        el = ua.augment.identity_warp(1)
        el[0, 0], el[0, 1], el[0, 5], el[0, 7], el[0, 8] = 1.0, 1.0, 1.0, bad_alpha, bad_r
        with pytest.raises(ValueError, match="radius"):
            ua.augment.validate_warp(el, ua.augment.identity_params(1), H, W)


def test_degenerate_records_are_the_identity_map(ua):
    H, W = 33, 37
    c = ua.AugmentConfig(distort_group_prob=1.0, grid_distortion_prob=1.0, grid_num_steps=5,
                         grid_distort_limit=0.0)
    w = ua.augment.sample_warp(c, 2, H, W, torch.Generator().manual_seed(0)).numpy()
    assert (w[:, 0] == 2).all()
    assert (w[:, 8:13] == 1).all() and (w[:, 16:21] == 0).all()
    assert (w[:, 24:29] == 1).all() and (w[:, 32:37] == 0).all()
    xw, yw = D.warp_points(w[0], H, W, None, np.float32)
    x0, y0 = D.warp_points(np.zeros(64, np.float32), H, W, None, np.float32)
    assert np.array_equal(xw, x0) and np.array_equal(yw, y0)
    c = ua.AugmentConfig(distort_group_prob=1.0, optical_distortion_prob=1.0)
    w = ua.augment.sample_warp(c, 2, H, W, torch.Generator().manual_seed(0)).numpy()
    assert (w[:, 0] == 3).all() and (w[:, 3] == 0).all()
    assert (w[:, 1] == W / 2).all() and (w[:, 2] == H / 2).all()
    xw, yw = D.warp_points(w[0], H, W, None, np.float32)
    assert np.array_equal(xw, x0) and np.array_equal(yw, y0)
    c = ua.AugmentConfig(distort_group_prob=1.0, elastic_prob=1.0)     # alpha 0, sigma 0
    w = ua.augment.sample_warp(c, 2, H, W, torch.Generator().manual_seed(0)).numpy()
    assert (w[:, 0] == 1).all() and (w[:, 8] == 0).all() and (w[:, 9] == 1).all()
    xw, yw = D.warp_points(w[0], H, W, None, np.float64)
    assert np.abs(xw - x0).max() < 1e-4 and np.abs(yw - y0).max() < 1e-4


@pytest.mark.parametrize("shape", D.SHAPES, ids=str)
def test_field_restatements_agree_within_the_rounding_bound(ua, shape):
    N, H, W = shape
    for p, r, w in D.cases(ua.augment, 1, shape):
        w, r = w.numpy(), r.numpy()
        a, b = D.field_f32(w, r, N, H, W), D.field_f64(w, r, N, H, W)
        assert a.dtype == np.float32 and b.dtype == np.float64
        for n in range(N):
            err = float(np.abs(a[n].astype(np.float64) - b[n]).max())
            print(shape, "R", int(w[n, 8]), "alpha", float(w[n, 7]), "max |f32 - f64|", err,
                  "bound", D.field_bound(w[n]), "max |field|", float(np.abs(b[n]).max()))
            assert err <= D.field_bound(w[n])
            assert np.abs(b[n]).max() <= w[n, 7] and np.abs(b[n]).max() > 0
        assert not D.field_f32(w, None, N, H, W).any()
        w0 = w.copy()
        w0[1, 0] = 0
        assert not D.field_f32(w0, r, N, H, W)[1].any()
        assert np.array_equal(D.field_f32(w0, r, N, H, W)[0], a[0])
    radii = sorted({int(w[0, 8]) for _, _, w in D.cases(ua.augment, 1, shape)})
    assert radii == [2, 12, 16]


def test_field_noise_is_philox_stream_two(ua):
    """R = 0, g = [1], alpha = 1: the field is the noise itself."""
    H, W = 5, 7
    w = np.zeros((1, 64), np.float32)
    w[0, 0], w[0, 7], w[0, 9] = 1, 1, 1
    rng = np.array([[123, 456, 0, 0]], dtype=np.int64)
    fld = D.field_f32(w, rng, 1, H, W)[0]
    for (i, j) in ((0, 0), (2, 3), (4, 6)):
        words = R.philox4x32((i * W + j, 0, 2, 0), (123, 456)).reshape(4)
        for c in range(2):
            assert fld[i, j, c] == np.float32(2 * ((int(words[c]) >> 8) * 2.0 ** -24) - 1)
    assert fld.min() >= -1 and fld.max() < 1


@pytest.mark.parametrize("mode", sorted(D.MODES), ids=lambda m: D.MODES[m])
@pytest.mark.parametrize("shape", D.SHAPES, ids=str)
def test_fp32_restatement_against_fp64(ua, shape, mode):
    """The records of the GPU test: the fp32 restatement alone stays inside the bounds of
    `check_against_f64` (1 level, only at rounding ties; the mask only at cell boundaries, at
    most 1 % of a sample left out)."""
    N, H, W = shape
    image, mask = R.random_batch(N, H, W, seed=H + mode)
    for p, r, w in D.cases(ua.augment, mode, shape):
        p, r, w = p.numpy(), r.numpy(), w.numpy()
        f32_field = D.field_f32(w, r, N, H, W) if mode == 1 else None
        f64_field = D.field_f64(w, r, N, H, W) if mode == 1 else None
        o, m = D.augment_warp_f32(image, mask, p, r, w, f32_field)
        val, _, m64, near = D.augment_warp_f64(image, mask, p, r, w, f64_field)
        fig = R.check_against_f64(o, m, val, m64, near, max_left_out=0.01)
        o0, _ = R.augment_f32(image, mask, p, r)
        moved = float((o != o0).mean())
        print(shape, D.MODES[mode], fig, "share of bytes the warp changed", moved)
        assert moved > 0.3                              # the warp did something
        assert (o != 0).mean() > 0.5                    # and most of the sample stays inside
