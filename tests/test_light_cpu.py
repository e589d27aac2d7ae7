"""CPU (-m "not gpu"): the third augmentation stage without a device - the ABI surface of
unet_augment_light_u8 and its host-side argument checks, `from_yaml(lighting=True)` against the
reference's settings file (no key left unread), the record sampler (`augment.sample_light`) against
the file's probabilities and the reference library's draw rules, `validate_light`, and the
restatements of tests/tools/light_ref.py: the Poisson table against the exact distribution, the
fp32 chain against fp64 on the very records the GPU test uses."""
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


L = _load("light_ref")
NAMES = ("unet_augment_light_params_per_sample", "unet_augment_light_workspace_bytes",
         "unet_augment_light_u8", "unet_augment_light_stats", "unet_augment_light_apply")


def test_entry_points_declared_exported_and_bound(ua):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    handle = ctypes.CDLL(ua.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, text), f"{name} not declared"
        assert hasattr(handle, name), f"{name} not exported"
        assert name in ua._lib.SIGNATURES
    assert len(ua._lib.SIGNATURES["unet_augment_light_u8"][1]) == 10
    assert len(ua._lib.SIGNATURES["unet_augment_light_apply"][1]) == 10
    assert len(ua._lib.SIGNATURES["unet_augment_light_stats"][1]) == 8
    assert re.search(r"#define\s+UNET_ABI_VERSION\s+11\b", open(HEADER).read())
    assert ua._lib.ABI_VERSION == 11 and ua.lib().unet_abi_version() == 11
    assert ua.lib().unet_augment_light_params_per_sample() == 272 == ua.augment.LIGHT_PER_SAMPLE
    assert L.LIGHT == 272
    assert ua.lib().unet_augment_post_params_per_sample() == 64
    assert ua.lib().unet_augment_light_workspace_bytes(3) == 3 * 16        # sums [N][2] uint64
    assert ua.lib().unet_augment_light_workspace_bytes(0) == 0
    for name in ("augment_light_u8", "augment_light_stats", "augment_light_apply"):
        assert callable(getattr(ua.ops, name))
    for name in ("sample_light", "identity_light", "validate_light"):
        assert callable(getattr(ua.augment, name))
    q = ua.augment.identity_light(3)
    assert tuple(q.shape) == (3, 272) and q.dtype == torch.float32 and not q.any()


def test_host_arguments_are_rejected_before_any_launch(ua):
    """Every refused call differs in ONE argument from (A, B, Q, G, Wk, need, 2, 8, 8), which
    passes every check (it is not made: there is no device to launch on)."""
    lib = ua.lib()
    call = lib.unet_augment_light_u8
    A, B, Q, G, Wk = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000
    need = lib.unet_augment_light_workspace_bytes(2)
    assert need == 32
    for args in ((None, B, Q, G, Wk), (A, None, Q, G, Wk), (A, B, None, G, Wk)):
        assert call(*args, need, 2, 8, 8, None) == -1 and b"null pointer" in lib.unet_last_error()
    for shape in ((0, 8, 8), (2, 0, 8), (2, 8, 0), (-1, 8, 8), (2, 32769, 8), (2, 8, 32769),
                  (65536, 8, 8)):
        assert call(A, B, Q, G, Wk, 1 << 30, *shape, None) == -1
        assert b"bad shape" in lib.unet_last_error()
    assert call(A, B, Q, G, None, need, 2, 8, 8, None) == -1
    assert b"workspace is null or smaller" in lib.unet_last_error()
    assert call(A, B, Q, G, Wk, need - 1, 2, 8, 8, None) == -1
    assert b"workspace is null or smaller" in lib.unet_last_error()
    for off in (4, 8):
        assert call(A, B, Q, G, Wk + off, need, 2, 8, 8, None) == -1
        assert b"aligned" in lib.unet_last_error()
    # 2 x 8 x 8: image 384 bytes, light 2176, rng 32, workspace 32
    for args in ((A, A + 383, Q, G, Wk), (A, A - 383, Q, G, Wk), (A, Q + 2175, Q, G, Wk),
                 (A, Q - 383, Q, G, Wk), (A, G + 31, Q, G, Wk), (A, G - 383, Q, G, Wk),
                 (A, Wk + need - 1, Q, G, Wk), (A, Wk - 383, Q, G, Wk)):
        assert call(*args, need, 2, 8, 8, None) == -1
        assert b"image_out overlaps" in lib.unet_last_error()
    for args in ((A, B, Q, G, A + 368), (A, B, Q, G, Q + 2160), (A, B, Q, G, G + 16),
                 (A, B, Q, G, A - 16)):
        assert call(*args, need, 2, 8, 8, None) == -1
        assert b"workspace overlaps" in lib.unet_last_error()
    # the two halves go through the same checks
    stats, apply = lib.unet_augment_light_stats, lib.unet_augment_light_apply
    assert stats(None, Q, Wk, need, 2, 8, 8, None) == -1 and b"null" in lib.unet_last_error()
    assert stats(A, None, Wk, need, 2, 8, 8, None) == -1 and b"null" in lib.unet_last_error()
    assert stats(A, Q, None, need, 2, 8, 8, None) == -1
    assert b"workspace is null" in lib.unet_last_error()
    assert stats(A, Q, Wk, need - 1, 2, 8, 8, None) == -1 and b"smaller" in lib.unet_last_error()
    assert stats(A, Q, Wk + 8, need, 2, 8, 8, None) == -1 and b"aligned" in lib.unet_last_error()
    assert stats(A, Q, A + 368, need, 2, 8, 8, None) == -1
    assert b"workspace overlaps" in lib.unet_last_error()
    assert stats(A, Q, Wk, need, 2, 0, 8, None) == -1 and b"bad shape" in lib.unet_last_error()
    assert apply(None, B, Q, G, Wk, need, 2, 8, 8, None) == -1 and b"null" in lib.unet_last_error()
    assert apply(A, None, Q, G, Wk, need, 2, 8, 8, None) == -1 and b"null" in lib.unet_last_error()
    assert apply(A, B, None, G, Wk, need, 2, 8, 8, None) == -1 and b"null" in lib.unet_last_error()
    assert apply(A, B, Q, G, None, need, 2, 8, 8, None) == -1
    assert b"workspace is null" in lib.unet_last_error()
    assert apply(A, B, Q, G, Wk, need - 1, 2, 8, 8, None) == -1
    assert b"smaller" in lib.unet_last_error()
    assert apply(A, B, Q, G, Wk + 4, need, 2, 8, 8, None) == -1
    assert b"aligned" in lib.unet_last_error()
    assert apply(A, B, Q, G, Wk, need, 2, 8, -3, None) == -1
    assert b"bad shape" in lib.unet_last_error()
    assert apply(A, Q + 2175, Q, G, Wk, need, 2, 8, 8, None) == -1
    assert b"image_out overlaps" in lib.unet_last_error()
    assert apply(A, B, Q, G, G + 16, need, 2, 8, 8, None) == -1
    assert b"workspace overlaps" in lib.unet_last_error()


def test_python_surface_has_no_cpu_fallback(ua):
    x = torch.zeros(1, 16, 16, 3, dtype=torch.uint8)
    for fn, args in ((ua.ops.augment_light_u8, (x, ua.augment.identity_light(1))),
                     (ua.ops.augment_light_stats, (x, ua.augment.identity_light(1), None)),
                     (ua.ops.augment_light_apply, (x, ua.augment.identity_light(1), None, None))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(*args)
    for kw in (dict(iso_noise_prob=0.5), dict(lighting_group_prob=0.5, shadow_prob=1.0)):
        aug = ua.BatchAugment(ua.AugmentConfig(**kw))
        assert aug.lighting and not aug.photometric and not aug.distortion
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            aug(x)
    assert not ua.BatchAugment(ua.AugmentConfig(color_prob=1.0, hsv_prob=1.0)).lighting
    assert not ua.BatchAugment(ua.AugmentConfig(shadow_prob=1.0, fog_prob=1.0)).lighting


# ------------------------------------------------------------------------------------ from_yaml
LIGHTING = ("iso_noise_prob", "iso_color_shift", "iso_intensity", "lighting_group_prob",
            "shadow_prob", "sunflare_prob", "sunflare_src_radius", "fog_prob", "fog_coef",
            "fog_alpha_coef")


def test_from_yaml_reads_the_lighting_keys_only_when_asked(ua):
    import yaml
    raw = yaml.safe_load(open(YAML))
    default = ua.AugmentConfig()
    assert all(getattr(default, k) in (0.0, (0.0, 0.0), 400) for k in LIGHTING)
    assert default.sunflare_src_radius == 400
    for section in ("cat", "dog"):
        s = raw[section]
        for kw in ({}, {"distortion": True}, {"photometric": True},
                   {"distortion": True, "photometric": True}):
            old = ua.AugmentConfig.from_yaml(YAML, section, **kw)
            assert old == ua.AugmentConfig.from_yaml(YAML, section, lighting=False, **kw)
            assert all(getattr(old, k) == getattr(default, k) for k in LIGHTING)
            cfg = ua.AugmentConfig.from_yaml(YAML, section, lighting=True, **kw)
            assert old == ua.AugmentConfig(**{**vars(cfg), **{k: getattr(default, k)
                                                              for k in LIGHTING}})
            assert not ua.BatchAugment(old).lighting and ua.BatchAugment(cfg).lighting
        iso, fog = s["iso_noise"], s["fog"]
        assert (cfg.iso_noise_prob, cfg.iso_color_shift, cfg.iso_intensity) == (
            iso["prob"], tuple(iso["color_shift"]), tuple(iso["intensity"]))
        assert cfg.lighting_group_prob == s["lighting_transform_prob"] > 0
        assert (cfg.shadow_prob, cfg.sunflare_prob, cfg.fog_prob) == (
            s["shadow"]["prob"], s["sunflare"]["prob"], fog["prob"])
        assert cfg.fog_coef == (fog["fog_coef_lower"], fog["fog_coef_upper"])
        assert cfg.fog_alpha_coef == fog["alpha_coef"] and cfg.sunflare_src_radius == 400


class _Tracked(dict):
    """a mapping that remembers which of its keys were asked for"""

    def __init__(self, d):
        super().__init__({k: _Tracked(v) if isinstance(v, dict) else v for k, v in d.items()})
        self.asked = set()

    def get(self, k, default=None):
        self.asked.add(k)
        return super().get(k, default)

    def __getitem__(self, k):
        self.asked.add(k)
        return super().__getitem__(k)


def _unread(d, path=""):
    out = [path + k for k in d if k not in d.asked]
    for k, v in d.items():
        if isinstance(v, _Tracked) and k in d.asked:
            out += _unread(v, path + k + ".")
    return out


def test_from_yaml_with_all_three_flags_leaves_no_key_unread(ua, monkeypatch):
    import yaml
    raw = yaml.safe_load(open(YAML))
    docs = []

    def tracked_load(stream):
        docs.append(_Tracked(raw))
        return docs[-1]

    monkeypatch.setattr(yaml, "safe_load", tracked_load)
    for section in ("cat", "dog"):
        ua.AugmentConfig.from_yaml(YAML, section, distortion=True, photometric=True,
                                   lighting=True)
        assert _unread(dict.__getitem__(docs[-1], section)) == [], section
        # the check can fail: without the lighting flag exactly the lighting keys stay unread
        ua.AugmentConfig.from_yaml(YAML, section, distortion=True, photometric=True)
        left = set(_unread(dict.__getitem__(docs[-1], section)))
        assert left == {"iso_noise", "lighting_transform_prob", "shadow", "sunflare", "fog"}


# ------------------------------------------------------------------------------------ the draws
# sha256 over (params, rng, warp, params', rng', post) of sample_params / sample_warp / sample_post
# with from_yaml(section, distortion=True, photometric=True), n = 64, 96 x 128, seed 1234, and
# three of the values, as the commit before the third stage printed them
PARENT = {
    "cat": ("f4b8811a4acef0ed1f7bb9cf9347de2da14e15355334b2900cfb2dd1131cd8c4",
            134.3316192626953, 53.0, 231.39370727539062, 142670228),
    "dog": ("5a8d3f526939acdba4dd85cba5b4e67c9cc4c777158386f0ef5ee2b3be65922d",
            133.76736450195312, 26.0, 151.45761108398438, 142670228),
}


@pytest.mark.parametrize("lighting", [False, True])
@pytest.mark.parametrize("section", ["cat", "dog"])
def test_the_three_older_samplers_draw_what_they_drew(ua, section, lighting):
    A = ua.augment
    cfg = A.AugmentConfig.from_yaml(YAML, section, distortion=True, photometric=True,
                                    lighting=lighting)
    gen = torch.Generator().manual_seed(1234)
    n, H, W = 64, 96, 128
    p, r, groups = A.sample_params(cfg, n, H, W, gen, return_groups=True)
    w = A.sample_warp(cfg, n, H, W, gen)
    p2, r2, q = A.sample_post(cfg, n, H, W, gen, p, r, groups)
    h = hashlib.sha256()
    for t in (p, r, w, p2, r2, q):
        h.update(np.ascontiguousarray(t.numpy()).tobytes())
    digest, p32, wsum, qsum, seed = PARENT[section]
    assert (float(p[3, 2]), float(w[:, 0].sum()), float(q.sum()), int(r[5, 0])) == \
        (p32, wsum, qsum, seed)
    assert h.hexdigest() == digest
    # sample_light comes after them, from a block of its own: the next draw of the generator
    # without it is the first uniform it consumes
    state = gen.get_state()
    nxt = torch.rand(1, dtype=torch.float64, generator=gen)
    gen.set_state(state)
    lt, ap = A.sample_light(cfg, n, H, W, gen, return_applied=True)
    assert tuple(lt.shape) == (n, 272) and lt.dtype == torch.float32
    assert bool(ap["iso_noise"][0]) == bool(float(nxt) < cfg.iso_noise_prob)
    if not lighting:
        assert not lt.any()


def _within(share, p, n, what):
    sd = math.sqrt(p * (1 - p) / n)
    assert abs(share - p) <= 4 * sd, f"{what}: share {share:.4f}, probability {p:.4f}, sd {sd:.4f}"


@pytest.mark.parametrize("section", ["cat", "dog"])
def test_yaml_probabilities_one_of_and_limits(ua, section):
    import yaml
    raw = yaml.safe_load(open(YAML))[section]
    A = ua.augment
    cfg = A.AugmentConfig.from_yaml(YAML, section, lighting=True)
    n, H, W = 20000, 512, 512
    lt, ap = A.sample_light(cfg, n, H, W, torch.Generator().manual_seed(31), return_applied=True)
    A.validate_light(lt, H, W)
    q = lt.numpy().astype(np.float64)
    act = {"iso_noise": q[:, 0] == 1, "shadow": q[:, 3] == 1, "sunflare": q[:, 3] == 2,
           "fog": q[:, 3] == 3}
    for k in act:
        assert np.array_equal(act[k], ap[k]), k
    _within(act["iso_noise"].mean(), raw["iso_noise"]["prob"], n, f"{section}/iso_noise")
    members = {k: raw[k]["prob"] for k in ("shadow", "sunflare", "fog")}
    tot = sum(members.values())
    assert (sum(act[k].astype(int) for k in members) <= 1).all()               # OneOf
    for k, prob in members.items():
        _within(act[k].mean(), raw["lighting_transform_prob"] * prob / tot, n, f"{section}/{k}")
    # ISO fires on its own, whatever the group does
    both = (act["iso_noise"] & (q[:, 3] != 0)).mean()
    _within(both, raw["iso_noise"]["prob"] * raw["lighting_transform_prob"], n, "independence")

    iso = q[act["iso_noise"]]
    lo_i, hi_i = raw["iso_noise"]["intensity"]
    lo_c, hi_c = raw["iso_noise"]["color_shift"]
    assert (iso[:, 2] >= lo_i - 1e-6).all() and (iso[:, 2] <= hi_i + 1e-6).all()
    assert iso[:, 2].max() > 0.95 * hi_i and iso[:, 2].min() < lo_i + 0.05 * (hi_i - lo_i)
    shift = iso[:, 1] / (360.0 * iso[:, 2])
    assert (shift >= lo_c - 1e-6).all() and (shift <= hi_c + 1e-6).all()
    assert (q[~act["iso_noise"], :3] == 0).all()

    sh = q[act["shadow"]]
    assert set(np.unique(sh[:, 4])) == {1.0, 2.0}
    _within((sh[:, 4] == 2).mean(), 0.5, len(sh), "two polygons")
    v = sh[:, 16:36].reshape(-1, 10, 2)
    assert (v == np.rint(v)).all() and (v >= 0).all()
    assert (v[..., 0] <= W).all() and (v[..., 1] <= H).all() and v[..., 0].max() > 0.95 * W
    assert (v[sh[:, 4] == 1, 5:] == 0).all() and (sh[:, 36:] == 0).all()

    fl = q[act["sunflare"]]
    assert set(np.unique(fl[:, 4])) == {6.0, 7.0, 8.0, 9.0, 10.0}
    assert (fl[:, 7] == 400).all() and (fl[:, 8] == 40).all()
    assert (fl[:, 5] >= 0).all() and (fl[:, 5] < W).all() and (fl[:, 6] >= 0).all() and \
        (fl[:, 6] < H).all()
    for row in fl[:200]:
        c = row[16:16 + 7 * int(row[4])].reshape(-1, 7)
        assert (row[16 + 7 * int(row[4]):] == 0).all()
        assert (c[:, 2] >= 1).all() and (c[:, 2] <= max(H // 100 - 2, 2)).all()
        assert (c[:, 2] == np.rint(c[:, 2])).all()
        assert (c[:, 3] >= 0.05).all() and (c[:, 3] <= 0.2).all()
        assert (c[:, 4:] >= 205).all() and (c[:, 4:] <= 255).all()
        assert (c[:, 4:] == np.rint(c[:, 4:])).all()
        # on a line through the centre: the cross products of the offsets vanish within the
        # truncation of the positions to integers
        d = c[:, :2] - row[5:7]
        far = d[np.argmax(np.abs(d).sum(1))]
        assert (np.abs(d[:, 0] * far[1] - d[:, 1] * far[0]) <= 2 * np.abs(far).sum() + 2).all()

    fg = q[act["fog"]]
    lo_f, hi_f = raw["fog"]["fog_coef_lower"], raw["fog"]["fog_coef_upper"]
    coef = fg[:, 6] / raw["fog"]["alpha_coef"]
    assert (coef >= lo_f - 1e-6).all() and (coef <= hi_f + 1e-6).all()
    hw = np.floor((W // 3) * coef + 1e-9)
    near = np.abs((W // 3) * coef - np.rint((W // 3) * coef)) < 1e-4       # coef is known to fp32
    assert (fg[~near, 5] == hw[~near] // 2).all()
    assert (fg[~near, 7] == np.maximum(hw[~near] // 10, 1)).all()
    assert (fg[:, 4] <= 128).all() and fg[:, 4].min() >= 1 and (fg[:, 7] <= 9).all()
    for row in fg[:200]:
        assert int(row[4]) == A.fog_point_count(int(row[5]) * 2, H, W) or \
            int(row[4]) == A.fog_point_count(int(row[5]) * 2 + 1, H, W)
        assert (row[16 + 2 * int(row[4]):] == 0).all()
    assert (q[q[:, 3] == 0, 3:] == 0).all()


def test_fog_point_count_stays_under_the_cap_and_a_draw_beyond_it_raises(ua):
    A = ua.augment
    counts = {c: A.fog_point_count(max(1, int((512 // 3) * c)), 512, 512)
              for c in (0.08, 0.1, 0.2, 0.3)}
    assert counts == {0.08: 105, 0.1: 66, 0.2: 63, 0.3: 50}
    for c in np.linspace(0.08, 0.3, 221):
        hw = max(1, int((512 // 3) * float(c)))
        assert A.fog_point_count(hw, 512, 512) <= 128 and hw // 10 <= 9, c
        pts = A.fog_points(hw, 512, 512, iter(np.random.default_rng(hw).uniform(size=400)))
        assert len(pts) == A.fog_point_count(hw, 512, 512)
    cfg = A.AugmentConfig(lighting_group_prob=1.0, fog_prob=1.0, fog_coef=(1.0, 1.0),
                          fog_alpha_coef=0.08)
    with pytest.raises(ValueError, match="record holds 128 points"):
        A.sample_light(cfg, 2, 4096, 4096, torch.Generator())
    # the sampler refuses limits it cannot draw from
    for kw in (dict(iso_noise_prob=1.0, iso_intensity=(0.1, 1.5)),
               dict(iso_noise_prob=1.0, iso_intensity=(-0.1, 0.5)),
               dict(lighting_group_prob=1.0, sunflare_prob=1.0, sunflare_src_radius=19),
               dict(lighting_group_prob=1.0, sunflare_prob=1.0, sunflare_src_radius=401),
               dict(lighting_group_prob=1.0, fog_prob=1.0, fog_coef=(0.1, 1.2))):
        with pytest.raises(ValueError):
            A.sample_light(A.AugmentConfig(**kw), 2, 64, 64, torch.Generator())
    cfg = A.AugmentConfig(lighting_group_prob=1.0, sunflare_prob=1.0, sunflare_src_radius=57)
    lt = A.sample_light(cfg, 4, 64, 64, torch.Generator())
    assert (lt[:, 7] == 57).all() and (lt[:, 8] == 5).all()                # T = Rs // 10


def test_bad_records_are_refused(ua):
    H, W = 40, 52
    V = ua.augment.validate_light
    good = np.stack([L.with_iso(L.records((3, 40, 52), "shadow")[0][1], 12.0, 0.4),
                     L.records((3, 40, 52), "flare")[0][1],
                     L.records((3, 40, 52), "fog")[1][1]])                  # k = 9
    good = torch.from_numpy(good)
    V(good, H, W)
    V(ua.augment.identity_light(2), H, W)
    for stage in L.STAGES:
        for q in L.records((3, 40, 52), stage):
            V(q, H, W)

    def bad(match, **at):
        q = good.clone()
        for k, v in at.items():
            q[int(k[1]), int(k[3:])] = v
        with pytest.raises(ValueError, match=match):
            V(q, H, W)

    bad("non-finite", s0_20=float("nan"))
    bad("non-finite", s2_271=float("inf"))
    bad("ISO flag", s0_0=2.0)
    bad("ISO flag", s1_0=0.5)
    bad("sigma_h", s0_1=-1.0)
    bad("intensity", s0_2=1.5)
    bad("intensity", s0_2=-0.1)
    bad("mode", s0_3=4.0)
    bad("mode", s1_3=1.5)
    for c in (0.0, 3.0, 1.5):
        bad("polygon count", s0_4=c)
    for c in (-1.0, 11.0, 2.5):
        bad("circle count", s1_4=c)
    for t in (1.0, 41.0, 3.5):
        bad("step count", s1_8=t)
    bad("source radius", s1_7=0.5)
    bad("negative radius", s1_18=-1.0)
    bad(r"a must be in \[0, 1\]", s1_19=1.5)
    bad(r"a must be in \[0, 1\]", s1_19=-0.1)
    bad("colour", s1_20=256.0)
    bad("colour", s1_22=-1.0)
    for c in (-1.0, 129.0, 0.5):
        bad("point count", s2_4=c)
    for k in (0.0, 10.0, 2.5):
        bad("box size", s2_7=k)
    bad("radius must not be negative", s2_5=-1.0)
    bad(r"a must be in \[0, 1\]", s2_6=1.01)
    V(good[2:], 5, 52)                                          # k = 9 reaches 4 pixels: 4 < 5
    with pytest.raises(ValueError, match="across the image"):
        V(good[2:], 4, 52)
    with pytest.raises(ValueError):
        V(torch.zeros(2, 271), H, W)


# ------------------------------------------------------------------------------------ restatements
@pytest.mark.parametrize("lam", [0.05, 1.0, 8.0, 38.25, 64.0])
def test_poisson_table_against_the_exact_distribution(lam):
    c = L.poisson_table(lam)
    assert c.dtype == np.float32 and c.shape == (256,) and np.isfinite(c).all()
    assert (np.diff(c) >= 0).all() and c[0] == 1
    k = np.arange(256, dtype=np.float64)
    lg = np.array([math.lgamma(v + 1.0) for v in k])
    cdf = np.cumsum(np.exp(-lam + k * math.log(lam) - lg))
    err = np.abs(c.astype(np.float64) / np.float64(c[255]) - cdf)
    print("lambda", lam, "T", float(c[255]), "max |c_k / T - CDF(k)|", float(err.max()))
    assert err.max() <= 256 * 2.0 ** -23
    u = ((np.arange(1 << 16) + 0.5) / (1 << 16)).astype(np.float32)
    draw = np.minimum(np.searchsorted(c, u * c[255], side="right"), 255)
    mean, var = float(draw.mean()), float(draw.var())
    print("stratified mean", mean, "variance", var)
    assert abs(mean - lam) <= 4 * math.sqrt(lam / (1 << 16))
    # the draw of the restatement is this rule on the word's upper 24 bits
    words = np.zeros((1, 1 << 12, 4), dtype=np.uint32)
    words[0, :, 2] = np.arange(1 << 12, dtype=np.uint32) << np.uint32(20)
    uu = (words[0, :, 2] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    assert np.array_equal(L.poisson_draw(c, words)[0],
                          np.minimum(np.searchsorted(c, uu * c[255], side="right"), 255))


def test_poisson_table_at_zero_and_lambda_from_the_sums():
    c = L.poisson_table(0.0)
    assert (c == 1).all()
    words = np.full((2, 2, 4), 0xFFFFFFFF, dtype=np.uint32)
    assert (L.poisson_draw(c, words) == 0).all()                # u T < c_0 for every u < 1
    g = L.gray_batch(1, 96, 160, 0, 60)[0]
    rec = L.with_iso(L.identity(1)[0], 12.0, 0.5)
    assert L.iso_sums(g) == (96 * 160 // 2 * 120, 96 * 160 // 2 * 120 * 120)
    lam = L.iso_lambda(rec, L.iso_sums(g), 96 * 160)            # std(L) = 60 / 510
    assert lam.dtype == np.float32 and lam == np.float32(0.5 * 255 * 60 / 510)
    rec[2] = 1.0
    assert L.iso_lambda(rec, L.iso_sums(L.gray_batch(1, 8, 8, 0, 255)[0]), 64) == 64    # the cap
    rec[2] = float("nan")
    assert L.iso_lambda(rec, L.iso_sums(g), 96 * 160) == 0


@pytest.fixture(scope="module")
def batches():
    return {s: L.noise_batch(*s, seed=s[1]) for s in L.SHAPES}


@pytest.mark.parametrize("stage", L.STAGES)
@pytest.mark.parametrize("shape", L.SHAPES, ids=str)
def test_fp32_restatement_is_inside_the_fp64_bounds_on_the_gpu_records(batches, shape, stage):
    N, H, W = shape
    image = batches[shape]
    for q in L.records(shape, stage):
        o32, o64 = L.light_f32(image, q, L.RNG), L.light_f64(image, q, L.RNG)
        assert (o32 != image).mean() > 0.1
        print(shape, stage, "fp32 and fp64 chains differ in", int((o32 != o64).sum()), "bytes")
        for n in range(N):
            fig = L.check_against_f64(image[n], q[n], L.RNG[n])
            print(shape, stage, n, "segments", len(fig), "apart from fp64 (count, tie distance):",
                  {k: (v["differing"], v["max_tie_distance"]) for k, v in fig.items()
                   if v["differing"]})
            assert all(v["max_diff"] <= 1 for v in fig.values())


@pytest.mark.parametrize("shape", L.SHAPES, ids=str)
def test_iso_restatements_on_colour_noise_and_gray(batches, shape):
    N, H, W = shape
    image = batches[shape]
    q = np.stack([L.with_iso(L.identity(1)[0], s, i) for s, i in
                  ((3.6, 0.1), (18.0, 0.5), (90.0, 1.0))])
    o32 = L.light_f32(image, q, L.RNG)
    assert (o32 != image).mean() > 0.5
    assert np.array_equal(L.light_f32(image, q, None), image)   # no words: ISO is off
    for n in range(N):
        fig = L.check_against_f64(image[n], q[n], L.RNG[n])
        print(shape, n, fig)
    # S = 0: the hue cannot act, the lightness moves up by k (255 - p) / 255
    g = L.gray_batch(N, H, W, 0, 60)
    o = L.light_f32(g, q, L.RNG)
    assert np.array_equal(o, L.light_f64(g, q, L.RNG))
    for n in range(N):
        lam, k = L.iso_k(g[n], q[n], L.RNG[n])
        assert (o[n][..., 0] == o[n][..., 1]).all() and (o[n][..., 0] == o[n][..., 2]).all()
        assert np.array_equal(o[n][..., 0][g[n][..., 0] == 0], k[g[n][..., 0] == 0])
        want = np.rint(60 + k * 195.0 / 255.0)
        assert np.abs(o[n][..., 0][g[n][..., 0] == 60] - want[g[n][..., 0] == 60]).max() <= 1


def test_identity_and_out_of_range_records_in_the_restatement():
    image = L.noise_batch(3, 33, 37, 5)
    assert np.array_equal(L.light_f32(image, L.identity(3), L.RNG), image)
    assert np.array_equal(L.light_f64(image, L.identity(3), L.RNG), image)
    q = L.records((3, 33, 37), "fog")[0]
    q[:, 4] = (float("nan"), -3.0, 1e30)                        # counts: 0, 0, 128
    q[:, 7] = (float("nan"), 0.0, 1e30)                         # box: 1, 1, 9
    o = L.light_f32(image, q, None)
    assert np.array_equal(o[:2], image[:2]) and (o[2] != image[2]).mean() > 0.3
    q = L.records((3, 33, 37), "shadow")[0]
    q[:, 4] = (0.0, float("nan"), 7.0)                          # polygons: 0, 0, 2
    o = L.light_f32(image, q, None)
    assert np.array_equal(o[:2], image[:2]) and (o[2] != image[2]).any()


def _dark_pixels():
    """every triple over 17 levels with s = max + min <= 255, as a 1 x 1 x n image, and the record
    of one polygon that covers it"""
    vals = np.array([0, 1, 2, 3, 7, 16, 31, 63, 64, 100, 101, 126, 127, 128, 191, 254, 255])
    r, g, b = np.meshgrid(vals, vals, vals, indexing="ij")
    px = np.stack([r, g, b], -1).reshape(-1, 3)
    px = px[px.max(1) + px.min(1) <= 255].astype(np.uint8)
    assert len(px) > 1500
    Wd = len(px)
    rec = L.shadow_record([[(-1, -1), (Wd + 1, -1), (Wd + 1, 2), (Wd / 2.0, 3), (-1, 2)]])
    assert L.polygon_inside(rec, 0, 1, Wd).all()
    return px, rec


def test_shadow_on_a_dark_pixel_is_exactly_half_per_channel():
    """With s = max + min <= 255 the shadow gives exactly byte(p / 2) per channel, ties to even
    included.  Halving L scales every operation of the way back by an exact power of two, so the
    shadowed channel is half of what the unshadowed round trip gives; S and the hue's fraction
    are rounded quotients, and it is HLS in fp64 with the channel rounded to fp32 that makes the
    round trip return p itself (in fp32 throughout, 1.30 M of the 25.3 M bytes of all such pixels
    fell a level beside byte(p / 2), all at odd p, where the half is a rounding tie)."""
    px, rec = _dark_pixels()
    out = L.light_f32(px.reshape(1, 1, -1, 3), rec[None], None)[0, 0].astype(np.int64)
    want = np.rint(px.astype(np.float64) / 2).astype(np.int64)              # ties to even
    d = np.abs(out - want)
    print("pixels", len(px), "bytes beside byte(p / 2):", int((d > 0).sum()), "of", d.size)
    assert np.array_equal(out, want)
    assert (px % 2 == 1).sum() > 3000                                       # ties are tested
    # before rounding to bytes the value is p / 2 itself, and the identity round trip is p
    H, Lm, S = L.hls_forward(px, np.float64)
    assert np.array_equal(L.hls_back(H, Lm * 0.5, S, np.float64).astype(np.float32),
                          px.astype(np.float32) / 2)
    assert np.array_equal(L.hls_back(H, Lm, S, np.float64).astype(np.float32), px)


def test_shadow_on_gray_and_twice():
    gray = np.repeat(np.arange(0, 128, dtype=np.uint8)[:, None], 3, 1).reshape(1, 1, -1, 3)
    Wg = gray.shape[2]
    poly = [(-1, -1), (Wg + 1, -1), (Wg + 1, 2), (Wg / 2.0, 3), (-1, 2)]
    one = L.light_f32(gray, L.shadow_record([poly])[None], None)[0, 0]
    assert np.array_equal(one[:, 0], np.rint(np.arange(128) / 2.0)) and \
        (one[:, 0] == one[:, 1]).all() and (one[:, 0] == one[:, 2]).all()
    # twice shadowed: a quarter
    two = L.light_f32(gray, L.shadow_record([poly, poly])[None], None)[0, 0]
    assert np.array_equal(two[:, 0], np.rint(np.arange(128) / 4.0))
