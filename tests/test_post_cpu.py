"""CPU (-m "not gpu"): the second augmentation stage without a device - the ABI surface of
unet_augment_post_u8 and its host-side argument checks, `validate_post`, the record sampler
(`augment.sample_post`) against the probabilities and limits of the reference's settings file and
the OneOf structure of the three photometric groups, and the restatements of
tests/tools/post_ref.py against each other on the very records the GPU test uses."""
import ctypes
import hashlib
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


P = _load("post_ref")
R = P.R


def test_entry_points_declared_exported_and_bound(ua):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    handle = ctypes.CDLL(ua.LIB_PATH)
    for name in ("unet_augment_post_params_per_sample", "unet_augment_post_workspace_bytes",
                 "unet_augment_post_u8", "unet_augment_post_hist", "unet_augment_post_apply"):
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, text), f"{name} not declared"
        assert hasattr(handle, name), f"{name} not exported"
        assert name in ua._lib.SIGNATURES
    assert len(ua._lib.SIGNATURES["unet_augment_post_u8"][1]) == 10
    assert re.search(r"#define\s+UNET_ABI_VERSION\s+11\b", open(HEADER).read())
    assert ua._lib.ABI_VERSION == 11 and ua.lib().unet_abi_version() == 11
    assert ua.lib().unet_augment_post_params_per_sample() == 64 == ua.augment.POST_PER_SAMPLE
    assert ua.lib().unet_augment_params_per_sample() == 24
    assert ua.lib().unet_augment_warp_params_per_sample() == 64
    # counts [N][3][256] uint32 + LUTs [N][64][256] bytes
    assert ua.lib().unet_augment_post_workspace_bytes(3) == 3 * (3 * 256 * 4 + 64 * 256)
    assert ua.lib().unet_augment_post_workspace_bytes(0) == 0
    assert callable(ua.ops.augment_post_u8)
    for name in ("sample_post", "identity_post", "validate_post", "motion_line"):
        assert callable(getattr(ua.augment, name))
    q = ua.augment.identity_post(3)
    assert tuple(q.shape) == (3, 64) and q.dtype == torch.float32 and not q.any()


def test_host_arguments_are_rejected_before_any_launch(ua):
    lib = ua.lib()
    call = lib.unet_augment_post_u8
    A, B, Q, G, Wk = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000
    need = lib.unet_augment_post_workspace_bytes(2)
    for args in ((None, B, Q, G, Wk), (A, None, Q, G, Wk), (A, B, None, G, Wk)):
        assert call(*args, need, 2, 8, 8, None) == -1 and b"null pointer" in lib.unet_last_error()
    for shape in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8), (1, 32769, 8), (65536, 8, 8)):
        assert call(A, B, Q, G, Wk, 1 << 30, *shape, None) == -1
        assert b"bad shape" in lib.unet_last_error()
    assert call(A, B, Q, G, None, need, 2, 8, 8, None) == -1
    assert b"workspace is null or smaller" in lib.unet_last_error()
    assert call(A, B, Q, G, Wk, need - 1, 2, 8, 8, None) == -1
    assert b"workspace is null or smaller" in lib.unet_last_error()
    assert call(A, B, Q, G, Wk + 4, need, 2, 8, 8, None) == -1
    assert b"aligned" in lib.unet_last_error()
    # 2 x 8 x 8: image 384 bytes, post 512, rng 32, workspace `need`
    for args in ((A, A + 383, Q, G, Wk), (A, A - 383, Q, G, Wk), (A, Q + 511, Q, G, Wk),
                 (A, G + 31, Q, G, Wk), (A, G - 383, Q, G, Wk), (A, Wk + need - 1, Q, G, Wk),
                 (A, Wk - 383, Q, G, Wk)):
        assert call(*args, need, 2, 8, 8, None) == -1
        assert b"image_out overlaps" in lib.unet_last_error()
    for args in ((A, B, Q, G, A + 368), (A, B, Q, G, Q + 496), (A, B, Q, G, G + 16)):
        assert call(*args, need, 2, 8, 8, None) == -1
        assert b"workspace overlaps" in lib.unet_last_error()
    # the two halves go through the same checks
    hist, apply = lib.unet_augment_post_hist, lib.unet_augment_post_apply
    assert hist(None, Q, Wk, need, 2, 8, 8, None) == -1 and b"null" in lib.unet_last_error()
    assert hist(A, Q, Wk, need - 1, 2, 8, 8, None) == -1 and b"smaller" in lib.unet_last_error()
    assert hist(A, Q, A + 368, need, 2, 8, 8, None) == -1
    assert b"workspace overlaps" in lib.unet_last_error()
    assert hist(A, Q, Wk, need, 2, 0, 8, None) == -1 and b"bad shape" in lib.unet_last_error()
    assert apply(A, None, Q, G, Wk, need, 2, 8, 8, None) == -1 and b"null" in lib.unet_last_error()
    assert apply(A, B, Q, G, None, need, 2, 8, 8, None) == -1
    assert b"workspace is null" in lib.unet_last_error()
    assert apply(A, Q + 511, Q, G, Wk, need, 2, 8, 8, None) == -1
    assert b"image_out overlaps" in lib.unet_last_error()


def test_python_surface_has_no_cpu_fallback(ua):
    x = torch.zeros(1, 16, 16, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ua.ops.augment_post_u8(x, ua.augment.identity_post(1))
    aug = ua.BatchAugment(ua.AugmentConfig(color_prob=1.0, hsv_prob=1.0))
    assert aug.photometric and not aug.distortion
    assert not ua.BatchAugment(ua.AugmentConfig(color_prob=1.0, rgb_shift_prob=1.0)).photometric
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        aug(x)


def _gauss(ua, R_):
    k = 2 * R_ + 1
    return ua.augment.gaussian_taps(0.3 * ((k - 1) * 0.5 - 1) + 0.8, radius=R_)[1][:R_ + 1]


def test_bad_records_are_refused(ua):
    H, W = 40, 52
    V = ua.augment.validate_post
    good = ua.augment.identity_post(2)
    good[0, 0], good[0, 1:4] = 1.0, torch.tensor([400.0, -30.0, 20.0])
    good[0, 4], good[0, 5], good[0, 6], good[0, 7] = 2.0, 2.5, 8.0, 4.0
    good[0, 8], good[0, 9] = 1.0, 4.0
    good[0, 10:15] = torch.from_numpy(_gauss(ua, 4))
    good[1, 4], good[1, 8], good[1, 9] = 1.0, 2.0, 1.0
    good[1, 15:24] = torch.from_numpy(ua.augment.motion_line(3, (0, 0), (2, 1)).reshape(-1))
    V(good, H, W)
    V(ua.augment.identity_post(2), H, W)

    def bad(match, **at):
        q = good.clone()
        for k, v in at.items():
            q[int(k[1]), int(k[3:])] = v
        with pytest.raises(ValueError, match=match):
            V(q, H, W)

    bad("non-finite", s0_2=float("nan"))
    bad("non-finite", s1_40=float("inf"))
    bad("HSV flag", s0_0=2.0)
    bad("HSV flag", s1_0=0.5)
    bad("histogram op", s0_4=3.0)
    bad("histogram op", s1_4=-1.0)
    bad("blur mode", s0_8=3.0)
    bad("blur mode", s1_8=1.5)
    for ty in (0.0, 9.0, 2.5, 3.0):                         # 3 does not divide 40
        bad("tile grid", s0_6=ty)
    for tx in (0.0, 9.0, 8.0):                              # 8 does not divide 52
        bad("tile grid", s0_7=tx)
    bad("clip_limit", s0_5=0.0)
    bad("clip_limit", s0_5=-1.0)
    for R_ in (0.0, 5.0, 1.5, -1.0):
        bad("radius", s0_9=R_)
    for R_ in (0.0, 4.0, 2.5):
        bad("radius", s1_9=R_)
    bad("negative", s0_12=-0.01)
    bad("negative", s1_16=-0.5)
    bad("sum to 1", s0_10=float(good[0, 10]) + 1e-4)
    bad("sum to 1", s1_15=0.0)
    q = good.clone()
    q[0, 4] = 0.0                                           # no CLAHE: no grid to divide a shape
    V(q, 5, 52)
    with pytest.raises(ValueError, match="across the image"):
        V(q, 4, 52)                                         # R = 4 >= min(H, W)
    with pytest.raises(ValueError, match="across the image"):
        V(q[1:], 1, 52)                                     # R = 1 >= 1
    with pytest.raises(ValueError):
        V(torch.zeros(2, 63), H, W)
    # the sampler refuses limits it cannot draw from
    for kw in (dict(gaussian_blur_prob=1.0, gaussian_blur_limit=(3, 11)),
               dict(gaussian_blur_prob=1.0, gaussian_blur_limit=(4, 4)),
               dict(motion_blur_prob=1.0, motion_blur_limit=(3, 9)),
               dict(hsv_prob=1.0, hue_shift_limit=-1.0),
               dict(clahe_prob=1.0, clahe_clip_limit=0.5)):
        p, r, g = ua.augment.sample_params(ua.AugmentConfig(**kw), 2, H, W, torch.Generator(),
                                           return_groups=True)
        with pytest.raises(ValueError):
            ua.augment.sample_post(ua.AugmentConfig(**kw), 2, H, W, torch.Generator(), p, r, g)


def test_identity_record_leaves_the_restatement_equal_to_its_input(ua):
    image = P.noise_batch(2, 33, 37, 5)
    q = ua.augment.identity_post(2).numpy()
    assert np.array_equal(P.post_f32(image, q), image)
    assert np.array_equal(P.post_f64(image, q), image)
    # salt / pepper alone: the rule of augment_ref on the input
    rng = np.array([[11, 22, 1 << 28, 1 << 27], [33, 44, 0, 0]], dtype=np.int64)
    want = np.stack([R._salt_pepper(image[n], rng[n], 33, 37) for n in range(2)])
    got = P.post_f32(image, q, rng)
    assert np.array_equal(got, want) and (got[0] != image[0]).any()
    assert np.array_equal(got[1], image[1])
    # an HSV record with zero shifts moves a byte only through the float round trip: never by
    # more than a level
    q[:, 0] = 1
    assert np.abs(P.post_f32(image, q).astype(int) - image).max() <= 1


PHOTO = ("hsv_prob", "hue_shift_limit", "sat_shift_limit", "val_shift_limit", "clahe_prob",
         "clahe_clip_limit", "clahe_tile_grid", "equalize_prob", "gaussian_blur_prob",
         "gaussian_blur_limit", "motion_blur_prob", "motion_blur_limit")


def test_from_yaml_reads_the_new_members_only_when_asked(ua):
    import yaml
    raw = yaml.safe_load(open(YAML))
    default = ua.AugmentConfig()
    for section in ("cat", "dog"):
        s = raw[section]
        plain = ua.AugmentConfig.from_yaml(YAML, section)
        assert plain == ua.AugmentConfig.from_yaml(YAML, section, photometric=False)
        assert all(getattr(plain, k) == getattr(default, k) for k in PHOTO)
        for distortion in (False, True):
            cfg = ua.AugmentConfig.from_yaml(YAML, section, distortion=distortion,
                                             photometric=True)
            old = ua.AugmentConfig.from_yaml(YAML, section, distortion=distortion)
            assert old == ua.AugmentConfig(**{**vars(cfg), **{k: getattr(default, k)
                                                              for k in PHOTO}})
        h, c = s["hsv"], s["clahe_equalize"]
        assert (cfg.hsv_prob, cfg.hue_shift_limit, cfg.sat_shift_limit, cfg.val_shift_limit) == (
            h["prob"], h["hue_shift_limit"], h["sat_shift_limit"], h["val_shift_limit"])
        assert (cfg.clahe_prob, cfg.clahe_clip_limit, cfg.equalize_prob) == (
            c["clahe_prob"], c["clahe_clip_limit"], c["equalize_prob"])
        assert cfg.clahe_tile_grid == (8, 8) == tuple(c["clahe_tile_grid_size"])
        assert cfg.gaussian_blur_prob == s["gaussian_blur"]["prob"] > 0
        assert cfg.gaussian_blur_limit == (0, 9) == tuple(s["gaussian_blur"]["blur_limit"])
        assert cfg.motion_blur_prob == s["motion_blur"]["prob"] > 0
        assert cfg.motion_blur_limit == (3, 3) and s["motion_blur"]["blur_limit"] == 3
        assert ua.BatchAugment(cfg).photometric and not ua.BatchAugment(plain).photometric


def _within(share, p, n, what):
    sd = math.sqrt(p * (1 - p) / n)
    assert abs(share - p) <= 4 * sd, f"{what}: share {share:.4f}, probability {p:.4f}, sd {sd:.4f}"


@pytest.mark.parametrize("section", ["cat", "dog"])
def test_yaml_probabilities_limits_and_one_of(ua, section):
    import yaml
    raw = yaml.safe_load(open(YAML))[section]
    cfg = ua.AugmentConfig.from_yaml(YAML, section, photometric=True)
    n, H, W = 20000, 512, 512
    gen = torch.Generator().manual_seed(22)
    p0, r0, ap, groups = ua.augment.sample_params(cfg, n, H, W, gen, return_applied=True,
                                                  return_groups=True)
    p, r, q, new = ua.augment.sample_post(cfg, n, H, W, gen, p0, r0, groups, return_applied=True)
    assert q.dtype == torch.float32 and tuple(q.shape) == (n, 64)
    assert torch.equal(r, r0) and p.dtype == torch.float32
    ua.augment.validate_post(q, H, W)
    ua.augment.validate_params(p, H, W)
    p, p0, q = (t.numpy().astype(np.float64) for t in (p, p0, q))
    assert np.array_equal(p[:, :9], p0[:, :9]) and np.array_equal(p[:, 15:], p0[:, 15:])

    # what acts on a sample, read from the records
    bc = (p[:, 9] != 1) | ((p[:, 10] == p[:, 11]) & (p[:, 11] == p[:, 12]) & (p[:, 10] != 0))
    act = {"brightness_contrast": ap["brightness_contrast"] & ~new["hsv"],
           "rgb_shift": ap["rgb_shift"] & ~new["hsv"], "hsv": q[:, 0] == 1,
           "gray": p[:, 13] == 1, "equalize": q[:, 4] == 1, "clahe": q[:, 4] == 2,
           "gauss_noise": p[:, 14] > 0, "gaussian_blur": q[:, 8] == 1, "motion_blur": q[:, 8] == 2}
    for k in new:
        assert np.array_equal(new[k], act[k]), k
    assert not (bc & act["hsv"]).any()
    assert (p[act["hsv"], 9] == 1).all() and (p[act["hsv"], 10:13] == 0).all()
    c = raw["clahe_equalize"]
    member = {"color": {"brightness_contrast": raw["brightness_contrast"]["prob"],
                        "rgb_shift": raw["rgb_shift"]["prob"], "hsv": raw["hsv"]["prob"]},
              "gray": {"gray": c["to_gray_prob"], "clahe": c["clahe_prob"],
                       "equalize": c["equalize_prob"]},
              "noise": {"gauss_noise": raw["gauss_noise"]["prob"],
                        "gaussian_blur": raw["gaussian_blur"]["prob"],
                        "motion_blur": raw["motion_blur"]["prob"]}}
    group_prob = {"color": raw["color_transform_prob"], "gray": c["prob"],
                  "noise": raw["noise_transform_prob"]}
    for gname, members in member.items():
        tot = sum(members.values())
        fired = sum(act[k].astype(int) for k in members)
        assert fired.max() == 1, gname                                      # OneOf
        _within(groups[gname].mean(), group_prob[gname], n, f"{section}/{gname}")
        for k, prob in members.items():
            share = act[k].mean()
            if k == "gauss_noise":      # var_limit starts at 0: sigma > 0 almost surely
                share = (ap["gauss_noise"] & ~new["gaussian_blur"] & ~new["motion_blur"]).mean()
            _within(share, group_prob[gname] * prob / tot, n, f"{section}/{k}")
        assert not (fired.astype(bool) & ~groups[gname]).any()

    # limits
    h = raw["hsv"]
    hs = q[act["hsv"]]
    for col, key in ((1, "hue_shift_limit"), (2, "sat_shift_limit"), (3, "val_shift_limit")):
        assert (np.abs(hs[:, col]) <= h[key] + 1e-5).all()
        assert np.abs(hs[:, col]).max() > 0.95 * h[key]
    assert (q[~act["hsv"], :4] == 0).all()
    cl = q[act["clahe"]]
    assert (cl[:, 5] >= 1).all() and (cl[:, 5] <= c["clahe_clip_limit"] + 1e-6).all()
    assert cl[:, 5].max() > 0.95 * c["clahe_clip_limit"] and cl[:, 5].min() < 1.1
    assert (cl[:, 6] == 8).all() and (cl[:, 7] == 8).all()
    assert (q[~act["clahe"], 5:8] == 0).all()
    gb = q[act["gaussian_blur"]]
    assert set(np.unique(gb[:, 9])) == {1.0, 2.0, 3.0, 4.0}                 # k = 3, 5, 7, 9
    for R_ in (1, 2, 3, 4):
        rows = gb[gb[:, 9] == R_]
        _within(len(rows) / len(gb), 0.25, len(gb), f"{section}/gaussian R={R_}")
        assert np.allclose(rows[:, 10:15], np.float32(np.pad(_gauss(ua, R_), (0, 4 - R_))))
        assert (rows[:, 15:] == 0).all()
    assert np.allclose(gb[:, 10] + 2 * gb[:, 11:15].sum(1), 1.0, atol=1e-6)
    mb = q[act["motion_blur"]]
    assert (mb[:, 9] == 1).all() and (mb[:, 10:15] == 0).all() and (mb[:, 24:] == 0).all()
    assert np.allclose(mb[:, 15:24].sum(1), 1.0, atol=1e-6)
    assert ((mb[:, 15:24] > 0).sum(1) >= 2).all()
    assert (q[q[:, 8] == 0, 8:] == 0).all()


def test_sample_params_and_sample_warp_are_untouched(ua):
    """The digests and values below were printed by the parent commit's `sample_params` and
    `sample_warp` for this configuration and seed."""
    cfg = ua.AugmentConfig(
        horizontal_flip_prob=0.5, shift_scale_rotate_prob=1.0, shift_limit=(-0.1, 0.1),
        scale_limit=(-0.15, 0.15), rotate_limit=(-15.0, 15.0), crop_prob=0.5,
        crop_scale=(0.8, 1.0), crop_ratio=(0.9, 1.1), perspective_prob=0.5,
        perspective_scale=(0.05, 0.1), dropout_prob=0.5, dropout_height=(2, 9),
        dropout_width=(2, 9), color_prob=0.8, brightness_contrast_prob=0.8,
        brightness_limit=(-0.1, 0.1), contrast_limit=(-0.3, 0.2), rgb_shift_prob=0.5,
        rgb_shift_limit=(15.0, 15.0, 15.0), gray_group_prob=0.5, to_gray_prob=0.2,
        noise_group_prob=0.5, gauss_noise_prob=0.5, gauss_var_limit=(4.0, 16.0),
        salt_pepper_prob=0.5, salt_p=(0.01, 0.05), pepper_p=(0.01, 0.05),
        distort_group_prob=0.8, elastic_prob=0.6, elastic_alpha=3.0, elastic_sigma=2.0,
        elastic_alpha_affine=1.0, grid_distortion_prob=0.5, grid_num_steps=5,
        grid_distort_limit=0.2, optical_distortion_prob=0.5, optical_distort_limit=0.2,
        optical_shift_limit=0.15)
    want = ("3000cbe4d21e78e4c650702c95e33c18bbb7e207127352371027b3d6c6f89d52",
            "69248b28505d877f4cba1410048ac7959779f5cbff13780582d3f4589a7eb03f",
            "9b6c80b02e6df62b7a8e4eb251c37542671e47ab3f694fc63147ea7a2d5b9ac1")

    def digest(t):
        return hashlib.sha256(t.numpy().tobytes()).hexdigest()

    photo = dict(hsv_prob=0.5, hue_shift_limit=10.0, clahe_prob=0.5, equalize_prob=0.5,
                 gaussian_blur_prob=0.4, gaussian_blur_limit=(0, 9), motion_blur_prob=0.4)
    for extra in ({}, photo):
        c = ua.AugmentConfig(**{**vars(cfg), **extra})
        for groups in (False, True):
            gen = torch.Generator().manual_seed(4321)
            out = ua.augment.sample_params(c, 6, 33, 37, gen, return_groups=groups)
            p, r = out[:2]
            w = ua.augment.sample_warp(c, 6, 33, 37, gen)
            assert (digest(p), digest(r), digest(w)) == want
            assert r[0].tolist() == [552364799, 105291058, 0, 0]
            assert w[:, 0].tolist() == [3.0, 0.0, 1.0, 0.0, 3.0, 3.0]
            assert len(out) == (3 if groups else 2)
    # sample_post draws from a block of its own, after the fact
    g1, g2 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    c = ua.AugmentConfig(**{**vars(cfg), **photo})
    a = ua.augment.sample_params(c, 4, 16, 24, g1, return_groups=True)
    b = ua.augment.sample_params(cfg, 4, 16, 24, g2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ua.augment.sample_post(c, 4, 16, 24, g1, *a)
    assert not torch.equal(torch.rand(1, generator=g1), torch.rand(1, generator=g2))


def test_which_selects_the_configuration_per_sample(ua):
    cat = ua.AugmentConfig(color_prob=1.0, hsv_prob=1.0, hue_shift_limit=10.0,
                           gray_group_prob=1.0, clahe_prob=1.0, clahe_clip_limit=4.0,
                           clahe_tile_grid=(2, 4))
    dog = ua.AugmentConfig(gray_group_prob=1.0, equalize_prob=1.0, noise_group_prob=1.0,
                           motion_blur_prob=1.0, motion_blur_limit=(3, 7))
    which = torch.tensor([0, 1, 2, 0, 1])
    gen = torch.Generator().manual_seed(0)
    cfgs = [cat, dog, ua.AugmentConfig()]
    p, r, g = ua.augment.sample_params(cfgs, 5, 40, 52, gen, which=which, return_groups=True)
    p, r, q = ua.augment.sample_post(cfgs, 5, 40, 52, gen, p, r, g, which=which)
    assert q[:, 0].tolist() == [1, 0, 0, 1, 0] and q[:, 4].tolist() == [2, 1, 0, 2, 1]
    assert q[:, 6].tolist() == [2, 0, 0, 2, 0] and q[:, 7].tolist() == [4, 0, 0, 4, 0]
    assert q[:, 8].tolist() == [0, 2, 0, 0, 2]
    ua.augment.validate_post(q, 40, 52)


def test_blur_weights_sum_to_one_and_lines_have_two_cells(ua):
    for R_ in (1, 2, 3, 4):
        g = _gauss(ua, R_)
        assert len(g) == R_ + 1 and abs(g[0] + 2 * g[1:].sum() - 1) < 1e-12
        assert (np.diff(g) < 0).all() and (g > 0).all()
        sigma = 0.3 * (R_ - 1) + 0.8
        assert math.isclose(g[1] / g[0], math.exp(-1 / (2 * sigma * sigma)), rel_tol=1e-12)
    # the existing call is unchanged: R from sigma
    assert ua.augment.gaussian_taps(4.0)[0] == 12 and ua.augment.gaussian_taps(0.0)[0] == 0
    for k in (3, 5, 7):
        cells = [(x, y) for y in range(k) for x in range(k)]
        for a in cells:
            for b in cells:
                if a == b:
                    with pytest.raises(ValueError):
                        ua.augment.motion_line(k, a, b)
                    continue
                w = ua.augment.motion_line(k, a, b)
                n = max(abs(a[0] - b[0]), abs(a[1] - b[1]))
                assert w.shape == (k, k) and abs(w.sum() - 1) < 1e-12
                assert (w > 0).sum() == n + 1 >= 2 and np.allclose(w[w > 0], 1 / (n + 1))
                assert w[a[1], a[0]] > 0 and w[b[1], b[0]] > 0
                assert np.abs(np.float32(w).astype(np.float64).sum() - 1) <= 1e-6
    w = ua.augment.motion_line(5, (0, 0), (4, 2))          # x runs, y follows by floor(. + 0.5)
    assert [int(np.argmax(w[:, x])) for x in range(5)] == [0, 1, 1, 2, 2]


def test_clahe_redistribution_conserves_the_area():
    def hist_of(counts):
        h = np.zeros(256, dtype=np.int64)
        for i, c in counts.items():
            h[i] = c
        return h

    cases = [
        (hist_of({7: 4096}), 16),                           # a one-value tile: excess 4080
        (hist_of({0: 3, 1: 2, 255: 1}), 2),                 # resid 1
        (hist_of({10: 300, 11: 45}), 45),                   # excess 255: resid 255, step 1
        (hist_of({10: 256 * 3 + 5, 200: 5}), 5),            # excess 256 m: resid 0
        (hist_of({i: 16 for i in range(256)}), 16),         # nothing clipped
        (hist_of({i: 16 for i in range(256)}), 1),          # every bin clipped: excess 256 * 15
        (hist_of({3: 129, 4: 1}), 1),                       # resid 128: step 2
    ]
    for h, climit in cases:
        out = P.clahe_redistribute(h, climit)
        area = int(h.sum())
        assert out.sum() == area and (out >= 0).all()
        excess = int(np.maximum(h - climit, 0).sum())
        assert out.max() <= climit + excess // 256 + 1
        lut = P.lut_of(P.clahe_lut_values(h, climit, area, np.float32))
        assert lut[255] == 255 and (np.diff(lut) >= 0).all()
    assert np.array_equal(P.clahe_redistribute(cases[4][0], 16), cases[4][0])
    out = P.clahe_redistribute(cases[1][0], 2)             # excess 1 -> bin 0 only
    assert out.tolist()[:3] == [3, 2, 0] and out[255] == 1
    assert P.clahe_limit(np.float32(300 * 64 / 256), 64, np.float32) == 64      # t >= area
    assert P.clahe_limit(np.float32(0.01 * 64 / 256), 64, np.float32) == 1
    assert P.clahe_limit(np.float32("nan"), 64, np.float32) == 1


def test_equalize_on_a_constant_channel_is_the_identity(ua):
    image = P.noise_batch(2, 16, 24, 9)
    assert (image[0, :, :, 1] == 77).all()
    q = ua.augment.identity_post(2).numpy()
    q[:, 4] = 1
    for out in (P.post_f32(image, q), P.post_f64(image, q)):
        assert np.array_equal(out[0, :, :, 1], image[0, :, :, 1])
        assert (out[0, :, :, 0] != image[0, :, :, 0]).any()
        for n, c in ((0, 0), (0, 2), (1, 0), (1, 1), (1, 2)):
            assert out[n, :, :, c].min() == 0 and out[n, :, :, c].max() == 255
    assert P.equalize_lut_values(np.bincount([5] * 10, minlength=256), np.float32) is None
    # two values: the lower goes to 0, the upper to 255
    v = P.equalize_lut_values(np.bincount([5] * 10 + [9] * 6, minlength=256), np.float32)
    assert P.lut_of(v)[5] == 0 and P.lut_of(v)[9] == 255


def test_special_pixels_of_the_hsv_stage():
    """gray pixels (d == 0) keep hue 0 and move only in value, black pixels stay black under a
    saturation shift, and a hue shift of a whole turn is the identity within a level"""
    px = np.array([[[90, 90, 90], [0, 0, 0], [200, 10, 10], [10, 200, 10], [10, 10, 200],
                    [255, 255, 0]]], dtype=np.uint8)
    rec = np.zeros(64, np.float32)
    rec[0], rec[3] = 1, 15
    out = P.byte(P.hsv_values(px, rec, np.float32))
    assert out[0, 0].tolist() == [105, 105, 105] and out[0, 1].tolist() == [15, 15, 15]
    rec[1:4] = (0, 80, 0)
    out = P.byte(P.hsv_values(px, rec, np.float32))
    assert out[0, 1].tolist() == [0, 0, 0] and out[0, 0, 0] == 90 and out[0, 0, 1] < 90
    rec[1:4] = (60, 0, 0)                                   # 120 degrees: r -> g -> b -> r
    out = P.byte(P.hsv_values(px, rec, np.float32))
    assert out[0, 2].tolist() == [10, 200, 10] and out[0, 3].tolist() == [10, 10, 200]
    assert out[0, 4].tolist() == [200, 10, 10]
    for dh in (180.0, -180.0, 540.0, -900.0):
        rec[1:4] = (dh, 0, 0)
        for dt in (np.float32, np.float64):
            assert np.abs(P.byte(P.hsv_values(px, rec, dt)) - px).max() <= 1


@pytest.mark.parametrize("stage", P.STAGES)
@pytest.mark.parametrize("shape", P.SHAPES, ids=str)
def test_fp32_restatement_against_fp64(ua, shape, stage):
    """The records and images of the GPU test: every segment of the fp32 restatement stays
    inside its bound against fp64 (post_ref: at most 1 apart, only at rounding ties)."""
    N, H, W = shape
    image = P.batch(shape, stage)
    radii, ops_seen = set(), set()
    for q in P.records(ua.augment, shape, stage):
        ua.augment.validate_post(q, H, W)
        out = P.post_f32(image, q)
        assert out.dtype == np.uint8 and (out != image).mean() > 0.3
        for n in range(N):
            fig = P.check_against_f64(image[n], q[n])
            hsv, op, grid, bm, R_ = P.modes(q[n], H, W)
            radii.add((bm, R_))
            ops_seen.add((op, grid if op == 2 else None))
            worst = max((v["max_tie_distance"] / v["bound"] for v in fig.values()
                         if "bound" in v), default=0.0)
            print(shape, stage, "hsv", hsv, "op", op, grid, "blur", bm, R_, "segments",
                  len(fig), "differing", sum(v.get("differing", 0) for v in fig.values()),
                  "largest tie distance / bound", round(worst, 4))
    if stage == "separable":
        assert radii == {(1, 1), (1, 2), (1, 4)}
    if stage == "dense":
        assert radii == {(2, 1), (2, 2), (2, 3)}
    if stage == "clahe":
        assert ops_seen == {(2, g) for g in P.grids(shape)}
    if stage == "clahe" and shape[1] == 64:
        # the two clip limits of batch 0: nothing clipped, every non-empty bin clipped
        q = P.records(ua.augment, shape, stage)[0]
        _, tr = P._chain(image[0], q[0], np.float32)
        assert tr["climit"] == H * W
        _, tr = P._chain(image[1], q[1], np.float32)
        assert tr["climit"] == 1


def test_a_grid_that_does_not_divide_is_no_histogram_op(ua):
    image = P.ramp_batch(1, 33, 37, 1)
    q = ua.augment.identity_post(1).numpy()
    q[0, 4], q[0, 5], q[0, 6], q[0, 7] = 2, 2.0, 2, 1        # 33 % 2 != 0
    assert np.array_equal(P.post_f32(image, q), image)
    q[0, 6] = 3
    assert not np.array_equal(P.post_f32(image, q), image)
    for ty in (0, 9, 2.5, float("nan")):
        q[0, 6] = ty
        assert np.array_equal(P.post_f32(image, q), image)
