"""CPU (-m "not gpu"): online batch augmentation without a device - the ABI surface of
unet_augment_u8 and its host-side argument checks, the record sampler (`augment.sample_params`)
against the probabilities and limits of the reference's settings file
(tests/golden/augmentation_config.yaml, a copy of data_augmentation/config/augmentation_config.yaml),
and the two restatements of tests/tools/augment_ref.py against the published Philox vectors and
against each other."""
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


R = _load("augment_ref")


def test_entry_points_declared_exported_and_bound(ua):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    handle = ctypes.CDLL(ua.LIB_PATH)
    for name in ("unet_augment_params_per_sample", "unet_augment_u8"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), f"{name} not declared in unet_hip.h"
        assert hasattr(handle, name), f"{name} not exported"
        assert name in ua._lib.SIGNATURES
    assert len(ua._lib.SIGNATURES["unet_augment_u8"][1]) == 10
    assert re.search(r"#define\s+UNET_ABI_VERSION\s+11\b", open(HEADER).read())
    assert ua._lib.ABI_VERSION == 11 and ua.lib().unet_abi_version() == 11
    assert ua.lib().unet_augment_params_per_sample() == 24 == ua.augment.PARAMS_PER_SAMPLE
    assert callable(ua.ops.augment_u8)
    for name in ("AugmentConfig", "BatchAugment"):
        assert getattr(ua, name) is getattr(ua.augment, name)
    for name in ("sample_params", "validate_params", "identity_params", "pack_rng"):
        assert callable(getattr(ua.augment, name))


def test_host_arguments_are_rejected_before_any_launch(ua):
    lib = ua.lib()
    A, B, C, D, P, G = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000
    call = lib.unet_augment_u8
    for args in ((None, B, C, D, P, G), (A, B, None, D, P, G), (A, B, C, D, None, G)):
        assert call(*args, 1, 8, 8, None) == -1 and b"null" in lib.unet_last_error()
    assert call(A, B, C, None, P, G, 1, 8, 8, None) == -1
    assert b"without mask_out" in lib.unet_last_error()
    for shape in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8)):
        assert call(A, B, C, D, P, G, *shape, None) == -1
        assert b"bad shape" in lib.unet_last_error()
    # 2 x 8 x 8: the image is 384 bytes, the mask 128
    for args in ((A, B, A, D, P, G), (A, B, A + 383, D, P, G), (A, B, B - 383, D, P, G),
                 (A, B, C, A + 383, P, G), (A, B, C, B + 127, P, G), (A, B, C, B - 127, P, G),
                 (A, B, P, D, P, G), (A, B, C, G, P, G)):
        assert call(*args, 2, 8, 8, None) == -1 and b"overlaps" in lib.unet_last_error()


def test_python_surface_has_no_cpu_fallback(ua):
    x = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ua.ops.augment_u8(x, None, ua.augment.identity_params(1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ua.BatchAugment(ua.AugmentConfig())(x)


def test_default_config_draws_the_identity_record(ua):
    g = torch.Generator().manual_seed(1)
    p, r = ua.augment.sample_params(ua.AugmentConfig(), 5, 37, 50, g)
    assert p.dtype == torch.float32 and tuple(p.shape) == (5, 24)
    assert torch.equal(p, ua.augment.identity_params(5))
    assert tuple(r.shape) == (5, 4) and (r[:, 2:] == 0).all()
    assert (r[:, :2] >= 0).all() and (r[:, :2] < 2 ** 32).all()
    ident = np.zeros(24, dtype=np.float32)
    ident[[0, 4, 8, 9]] = 1
    assert np.array_equal(p[0].numpy(), ident)
    # the same generator state gives the same records
    a = ua.augment.sample_params(ua.AugmentConfig(horizontal_flip_prob=0.5), 64, 8, 8,
                                 torch.Generator().manual_seed(3))
    b = ua.augment.sample_params(ua.AugmentConfig(horizontal_flip_prob=0.5), 64, 8, 8,
                                 torch.Generator().manual_seed(3))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    flipped = a[0][:, 0] < 0
    assert 0 < int(flipped.sum()) < 64
    assert torch.equal(a[0][flipped][:, :3], torch.tensor([[-1.0, 0.0, 8.0]]).expand(
        int(flipped.sum()), 3))


def _within(share, p, n, what):
    sd = math.sqrt(p * (1 - p) / n)
    assert abs(share - p) <= 4 * sd, f"{what}: share {share:.4f}, probability {p:.4f}, sd {sd:.4f}"


@pytest.mark.parametrize("section", ["cat", "dog"])
def test_yaml_probabilities_and_limits(ua, section):
    import yaml
    raw = yaml.safe_load(open(YAML))[section]
    cfg = ua.AugmentConfig.from_yaml(YAML, section)
    n, H, W = 20000, 512, 512
    p, r, ap = ua.augment.sample_params(cfg, n, H, W, torch.Generator().manual_seed(20),
                                        return_applied=True)
    ua.augment.validate_params(p, H, W)
    p, r = p.numpy().astype(np.float64), r.numpy()
    assert np.isfinite(p).all()
    pb, pr = raw["brightness_contrast"]["prob"], raw["rgb_shift"]["prob"]
    want = {"flip": raw["horizontal_flip_prob"],
            "shift_scale_rotate": raw["shift_scale_rotate_prob"],
            "crop": raw["random_resized_crop"]["prob"],
            "perspective": raw["perspective"]["prob"],
            "dropout": raw["coarse_dropout"]["prob"],
            "brightness_contrast": raw["color_transform_prob"] * pb / (pb + pr),
            "rgb_shift": raw["color_transform_prob"] * pr / (pb + pr),
            "gray": raw["clahe_equalize"]["prob"],          # the only supported member
            "gauss_noise": raw["noise_transform_prob"],     # the only supported member
            "salt_pepper": raw["salt_pepper"]["prob"]}
    assert set(want) == set(ap)
    for k, prob in want.items():
        _within(ap[k].mean(), prob, n, f"{section}/{k}")
    assert not (ap["brightness_contrast"] & ap["rgb_shift"]).any()      # OneOf

    # what the record shows agrees with what was reported as applied
    assert np.array_equal(p[:, 13] == 1, ap["gray"]) and set(np.unique(p[:, 13])) <= {0.0, 1.0}
    assert np.array_equal(p[:, 14] > 0, ap["gauss_noise"] & (p[:, 14] > 0))
    assert (p[~ap["gauss_noise"], 14] == 0).all()
    assert (r[~ap["salt_pepper"], 2:] == 0).all()
    assert (p[~ap["dropout"], 15:19] == 0).all()
    assert (p[~ap["brightness_contrast"], 9] == 1).all()
    assert (p[~(ap["brightness_contrast"] | ap["rgb_shift"]), 10:13] == 0).all()
    assert (p[:, 22:] == 0).all() and (p[:, 19:22] == 0).all()

    # limits
    eps = 1e-5
    c0, c1 = raw["brightness_contrast"]["contrast_limit"]
    bc = ap["brightness_contrast"]
    assert (p[bc, 9] >= 1 + c0 - eps).all() and (p[bc, 9] <= 1 + c1 + eps).all()
    assert p[bc, 9].min() < 1 + c0 + 0.1 and p[bc, 9].max() > 1 + c1 - 0.05     # the range is used
    bl = raw["brightness_contrast"]["brightness_limit"] * 255
    assert (np.abs(p[bc, 10]) <= bl + 1e-3).all()
    assert (p[bc, 10] == p[bc, 11]).all() and (p[bc, 10] == p[bc, 12]).all()
    for c, key in enumerate(("r_shift_limit", "g_shift_limit", "b_shift_limit")):
        assert (np.abs(p[ap["rgb_shift"], 10 + c]) <= raw["rgb_shift"][key] + 1e-3).all()
    assert (p[:, 14] <= math.sqrt(raw["gauss_noise"]["var_limit"][1]) + eps).all()
    for k, key in ((2, "pepper_p"), (3, "salt_p")):
        assert (r[:, k] <= round(raw["salt_pepper"][key][1] * 2 ** 32)).all()
        assert r[ap["salt_pepper"], k].max() > 0.9 * raw["salt_pepper"][key][1] * 2 ** 32
    assert (r >= 0).all() and (r < 2 ** 32).all()
    d = ap["dropout"]
    hw, hh = p[d, 17] - p[d, 15], p[d, 18] - p[d, 16]
    cd = raw["coarse_dropout"]
    assert (hw >= cd["min_width"]).all() and (hw <= cd["max_width"]).all() and hw.max() == cd["max_width"]
    assert (hh >= cd["min_height"]).all() and (hh <= cd["max_height"]).all()
    assert (p[d, 15] >= 0).all() and (p[d, 16] >= 0).all()
    assert (p[d, 17] <= W).all() and (p[d, 18] <= H).all()
    assert (p[d, 15:19] == np.rint(p[d, 15:19])).all()

    geo = {k: ap[k] for k in ("flip", "shift_scale_rotate", "crop", "perspective")}

    def only(name):
        m = geo[name].copy()
        for k, v in geo.items():
            if k != name:
                m &= ~v
        assert m.sum() > 50
        return p[m, 0:9].reshape(-1, 3, 3)

    none = ~(geo["flip"] | geo["shift_scale_rotate"] | geo["crop"] | geo["perspective"])
    assert (p[none, 0:9] == np.eye(3).reshape(9)).all()
    f = only("flip")
    assert (f == np.array([[-1, 0, W], [0, 1, 0], [0, 0, 1]])).all()
    s = only("shift_scale_rotate")
    assert (s[:, 2] == [0, 0, 1]).all()
    scale = 1 / np.hypot(s[:, 0, 0], s[:, 0, 1])
    assert (np.abs(scale - 1) <= raw["scale_limit"] + 1e-4).all()
    assert (np.abs(np.degrees(np.arctan2(s[:, 0, 1], s[:, 0, 0]))) <= raw["rotate_limit"] + 1e-3).all()
    assert np.allclose(s[:, 1, 1], s[:, 0, 0], atol=1e-6) and np.allclose(s[:, 1, 0], -s[:, 0, 1], atol=1e-6)
    centre = np.linalg.inv(s) @ np.array([W / 2, H / 2, 1.0])       # where the centre lands
    assert (np.abs(centre[:, 0] - W / 2) <= raw["shift_limit"] * W + 1e-2).all()
    assert (np.abs(centre[:, 1] - H / 2) <= raw["shift_limit"] * H + 1e-2).all()
    c = only("crop")
    rc = raw["random_resized_crop"]
    assert (c[:, 0, 1] == 0).all() and (c[:, 1, 0] == 0).all() and (c[:, 2] == [0, 0, 1]).all()
    fw, fh = c[:, 0, 0], c[:, 1, 1]
    assert (fw <= 1).all() and (fh <= 1).all() and (fw * fh <= rc["scale"][1] + eps).all()
    assert (fw * fh >= rc["scale"][0] / rc["ratio"][1] - eps).all()
    assert (fw / fh >= rc["ratio"][0] - 1e-4).all() or (np.minimum(fw, fh) < 1).all()
    assert (c[:, 0, 2] >= 0).all() and (c[:, 0, 2] + fw * W <= W + 1e-2).all()
    assert (c[:, 1, 2] >= 0).all() and (c[:, 1, 2] + fh * H <= H + 1e-2).all()
    q = only("perspective")
    lim = ua.augment.PERSPECTIVE_CLIP * raw["perspective"]["scale"][1]
    for (x, y) in ((0, 0), (W, 0), (W, H), (0, H)):
        src = q @ np.array([x, y, 1.0])
        sx, sy = src[:, 0] / src[:, 2], src[:, 1] / src[:, 2]
        assert (np.abs(sx - x) <= lim * W + 1e-2).all() and (np.abs(sy - y) <= lim * H + 1e-2).all()
        assert (sx >= -1e-2).all() and (sx <= W + 1e-2).all()       # the corners move inward
        assert (sy >= -1e-2).all() and (sy <= H + 1e-2).all()


def test_which_selects_the_configuration_per_sample(ua):
    cat = ua.AugmentConfig(gray_group_prob=1.0, to_gray_prob=1.0)
    dog = ua.AugmentConfig(horizontal_flip_prob=1.0)
    which = torch.tensor([0, 1, 1, 0, 1])
    p, _ = ua.augment.sample_params([cat, dog], 5, 16, 24, torch.Generator().manual_seed(0),
                                    which=which)
    assert torch.equal(p[:, 13] == 1, which == 0)
    assert torch.equal(p[:, 0] == -1, which == 1)
    with pytest.raises(ValueError):
        ua.augment.sample_params([cat, dog], 5, 16, 24, torch.Generator())
    with pytest.raises(ValueError):
        ua.augment.sample_params([cat, dog], 5, 16, 24, torch.Generator(), which=[0, 1, 2, 0, 0])


def test_from_yaml_ignores_unsupported_transforms_and_missing_keys(ua, tmp_path):
    path = tmp_path / "a.yaml"
    path.write_text("cat:\n  horizontal_flip_prob: 0.25\n  elastic:\n    alpha: 40.0\n"
                    "  fog:\n    prob: 0.2\n  scale_limit: 0.1\n")
    cfg = ua.AugmentConfig.from_yaml(str(path), "cat")
    want = ua.AugmentConfig(horizontal_flip_prob=0.25, scale_limit=(-0.1, 0.1))
    assert cfg == want
    with pytest.raises(KeyError):
        ua.AugmentConfig.from_yaml(str(path), "dog")
    # the package ships no preset: everything off is the identity
    assert all(v == 0 for k, v in vars(ua.AugmentConfig()).items() if k.endswith("_prob"))


def test_bad_records_are_refused(ua):
    good = ua.augment.identity_params(2)
    ua.augment.validate_params(good, 8, 8)
    for idx, value in ((3, float("nan")), (9, float("inf")), (14, float("-inf"))):
        bad = good.clone()
        bad[1, idx] = value
        with pytest.raises(ValueError, match="non-finite"):
            ua.augment.validate_params(bad, 8, 8)
    for h6, h7, h8 in ((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (-0.2, 0.0, 1.0), (0.0, -0.125, 1.0)):
        bad = good.clone()
        bad[0, 6], bad[0, 7], bad[0, 8] = h6, h7, h8
        with pytest.raises(ValueError, match="den <= 0"):
            ua.augment.validate_params(bad, 8, 8)
    with pytest.raises(ValueError):
        ua.augment.validate_params(torch.zeros(2, 23), 8, 8)
    with pytest.raises(ValueError):
        ua.augment.pack_rng(torch.tensor([[0, 0, 0, 2 ** 32]]))
    packed = ua.augment.pack_rng(torch.tensor([[0, 1, 2 ** 31, 2 ** 32 - 1]]))
    assert packed.dtype == torch.int32 and packed.tolist() == [[0, 1, -2 ** 31, -1]]


def test_philox_known_answers():
    for counter, key, want in R.PHILOX_KAT:
        got = R.philox4x32(counter, key)
        assert [int(x) for x in got.reshape(4)] == list(want)
    # vectorised over the counter as the restatements use it
    w = R.pixel_words(0xa4093822, 0x299f31d0, 3, 5, 1)
    one = R.philox4x32((7, 0, 1, 0), (0xa4093822, 0x299f31d0)).reshape(4)
    assert w.shape == (3, 5, 4) and np.array_equal(w[1, 2], one)
    z = R.normals(R.pixel_words(1, 2, 64, 64, 0), np.float64)
    assert abs(z.mean()) < 0.03 and abs(z.std() - 1) < 0.03


@pytest.mark.parametrize("H,W", [(37, 50), (64, 128), (96, 160), (512, 512)])
def test_fp32_restatement_against_fp64(ua, H, W):
    """Identity and flip exact; random affine and perspective records within the bounds of
    `check_against_f64` (1 level, only at rounding ties; mask only at cell boundaries)."""
    image, mask = R.random_batch(1, H, W, seed=H)
    ident = ua.augment.identity_params(1)
    flip = ident.clone()
    flip[0, 0], flip[0, 2] = -1.0, float(W)
    o, m = R.augment_f32(image, mask, ident.numpy())
    assert np.array_equal(o, image) and np.array_equal(m, mask)
    o, m = R.augment_f32(image, mask, flip.numpy())
    assert np.array_equal(o, image[:, :, ::-1]) and np.array_equal(m, mask[:, :, ::-1])
    _, o, m, _ = R.augment_f64(image, mask, flip.numpy())
    assert np.array_equal(o, image[:, :, ::-1]) and np.array_equal(m, mask[:, :, ::-1])
    n = 2 if H == 512 else 6
    for kind, cfg in R.record_configs(ua.augment).items():
        p, _ = ua.augment.sample_params(cfg, n, H, W, torch.Generator().manual_seed(W))
        img, msk = R.random_batch(n, H, W, seed=W + 1)
        o, m = R.augment_f32(img, msk, p.numpy())
        val, _, m64, near = R.augment_f64(img, msk, p.numpy())
        fig = R.check_against_f64(o, m, val, m64, near)
        print(kind, H, W, fig)
