"""GPU (-m gpu): `unet_augment_light_u8` (ISO noise, shadow / sun flare / fog) and `BatchAugment`
with a lighting configuration.

Yardsticks as in test_post_gpu.py: the kernels' arithmetic is normative, so the output must be
BYTE equal to the fp32 restatement of tests/tools/light_ref.py, and it must stay inside the
analytic bounds of `check_against_f64` (every byte-rounded segment at most 1 apart from fp64, only
at rounding ties).  The one exception is the hue noise of ISO on a coloured image, whose normal
comes from log / cos of different libraries: there the kernel is held against fp64 alone.  Shapes:
N = 3 at 16 x 24 (smaller than a 32 x 32 tile), 33 x 37 (crosses the tile edge by one pixel on both
axes, odd width) and 40 x 52 (several tiles, the fog's halo crosses a tile edge).  The records are
those of light_ref.records, which test_light_cpu.py holds against fp64 on the CPU."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from oracle import unet_ref as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(ROOT, "tests", "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


L = _load("light_ref")
P = _load("post_ref")
R = L.R
RNG = L.RNG


@pytest.fixture(scope="module")
def batches():
    """{shape: image} as numpy uint8; drawn once, never modified"""
    return {s: L.noise_batch(*s, seed=s[1]) for s in L.SHAPES}


def dev_rng(ua, rng):
    return ua.augment.pack_rng(rng).to(DEV) if rng is not None else None


def run(ua, image, light, rng=None, **kw):
    out = ua.ops.augment_light_u8(torch.from_numpy(image).to(DEV),
                                  torch.as_tensor(light, dtype=torch.float32).to(DEV),
                                  dev_rng(ua, rng), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def iso_records(pairs):
    return np.stack([L.with_iso(L.identity(1)[0], s, i) for s, i in pairs])


@pytest.mark.parametrize("shape", L.SHAPES, ids=str)
def test_identity_record_copies_and_no_words_turn_iso_off(ua, batches, shape):
    N, H, W = shape
    image = batches[shape]
    q = ua.augment.identity_light(N)
    assert np.array_equal(run(ua, image, q), image)
    assert np.array_equal(run(ua, image, q, RNG), image)
    iso = iso_records(((12.0, 0.4),) * N)
    assert np.array_equal(run(ua, image, iso, None), image)             # rng=None: a no-op
    assert (run(ua, image, iso, RNG) != image).mean() > 0.5
    # a caller's workspace and output; the refusals reach Python as errors
    x = torch.from_numpy(image).to(DEV)
    ws = torch.empty(ua.lib().unet_augment_light_workspace_bytes(N), dtype=torch.uint8,
                     device=DEV)
    buf = torch.empty_like(x)
    out = ua.ops.augment_light_u8(x, q.to(DEV), dev_rng(ua, RNG), out=buf, workspace=ws)
    assert out.data_ptr() == buf.data_ptr() and torch.equal(out, x)
    with pytest.raises(ua.UNetHipError):
        ua.ops.augment_light_u8(x, q.to(DEV), out=x)
    with pytest.raises(ua.UNetHipError):
        ua.ops.augment_light_u8(x, q.to(DEV), workspace=ws[:-16])


@pytest.mark.parametrize("shape", L.SHAPES + [(1, 96, 160)], ids=str)
def test_iso_on_gray_is_byte_exact(ua, shape):
    """S = 0, so the hue noise cannot act: lambda, the table and the draw bit for bit."""
    N, H, W = shape
    image = L.gray_batch(N, H, W, 0, 60)
    q = iso_records(((12.0, 0.5), (3.0, 0.1), (90.0, 1.0))[:N])
    got = run(ua, image, q, RNG[:N])
    want = L.light_f32(image, q, RNG[:N])
    print(shape, "differs from fp32 restatement:", int((got != want).sum()))
    assert np.array_equal(got, want)
    assert (got != image).mean() > 0.5
    for n in range(N):
        lam, k = L.iso_k(image[n], q[n], RNG[n])
        dark = image[n][..., 0] == 0
        assert np.array_equal(got[n][..., 0][dark], k[dark])            # level 0 becomes k
        tol = 4 * math.sqrt(float(lam) / (H * W))
        print(shape, n, "lambda", float(lam), "mean k", float(k.mean()), "allowed", tol)
        if (H, W) == (96, 160):
            assert abs(float(k.mean()) - float(lam)) <= tol
            assert abs(float(got[n][..., 0][dark].mean()) - float(lam)) <= \
                4 * math.sqrt(float(lam) / dark.sum())


@pytest.mark.parametrize("shape", L.SHAPES, ids=str)
def test_iso_on_colour_noise_against_fp64(ua, batches, shape):
    N, H, W = shape
    image = batches[shape]
    q = iso_records(((3.6, 0.1), (18.0, 0.5), (45.0, 1.0)))
    got = run(ua, image, q, RNG)
    o64 = L.light_f64(image, q, RNG)
    d = np.abs(got.astype(int) - o64.astype(int))
    print(shape, "bytes apart from fp64:", int((d > 0).sum()), "max", int(d.max()))
    assert d.max() <= 1
    for n in range(N):
        fig = L.check_against_f64(image[n], q[n], RNG[n], final=got[n])
        print(shape, n, fig)
    assert (got != image).mean() > 0.5


@pytest.mark.parametrize("stage", L.STAGES)
@pytest.mark.parametrize("shape", L.SHAPES, ids=str)
def test_random_records_against_both_restatements(ua, batches, shape, stage):
    """Six records per stage and shape: the bytes of the fp32 restatement, the bounds against
    fp64.  The fourth fog record also has ISO noise on (sigma_h = 0)."""
    N, H, W = shape
    image = batches[shape]
    for q in L.records(shape, stage):
        got = run(ua, image, q, RNG)
        want = L.light_f32(image, q, RNG)
        print(shape, stage, "differs from fp32 restatement:", int((got != want).sum()),
              "changed", float((got != image).mean()))
        for n in range(N):
            fig = L.check_against_f64(image[n], q[n], RNG[n], final=got[n])
            print(shape, stage, n, "segments", len(fig), "apart from fp64:",
                  {k: (v["differing"], v["max_tie_distance"]) for k, v in fig.items()
                   if v["differing"]})
        assert np.array_equal(got, want)
        assert (got != image).mean() > 0.1


def test_mixed_batch_changes_the_right_samples_only(ua, batches):
    shape = (3, 33, 37)
    image = batches[shape]
    q = L.identity(3)
    q[1] = L.records(shape, "shadow")[0][1]
    q[2] = L.with_iso(L.records(shape, "fog")[0][2], 0.0, 0.3)
    got = run(ua, image, q, RNG)
    assert np.array_equal(got[0], image[0])
    assert np.array_equal(got, L.light_f32(image, q, RNG))
    assert (got[1] != image[1]).mean() > 0.1 and (got[2] != image[2]).mean() > 0.3
    inside = L.polygon_inside(q[1], 0, 33, 37) | L.polygon_inside(q[1], 1, 33, 37)
    assert np.array_equal(got[1][~inside], image[1][~inside])


def test_the_two_halves_are_the_whole(ua, batches):
    shape = (3, 40, 52)
    N, H, W = shape
    image = L.gray_batch(N, H, W, 10, 90)
    q = L.records(shape, "fog")[1]
    q[0] = L.with_iso(L.records(shape, "flare")[0][1], 5.0, 0.6)
    q[2] = L.with_iso(q[2], 7.0, 0.3)
    x, dq, dr = torch.from_numpy(image).to(DEV), torch.from_numpy(q).to(DEV), dev_rng(ua, RNG)
    ws = torch.zeros(ua.lib().unet_augment_light_workspace_bytes(N), dtype=torch.uint8,
                     device=DEV)
    ua.ops.augment_light_stats(x, dq, ws)
    out = ua.ops.augment_light_apply(x, dq, dr, ws)
    torch.cuda.synchronize()
    sums = ws.cpu().numpy().view(np.uint64).reshape(N, 2)
    for n in range(N):              # sample 1 has no ISO noise: its workgroups returned at once
        assert tuple(int(v) for v in sums[n]) == (L.iso_sums(image[n]) if n != 1 else (0, 0))
    whole = run(ua, image, q, RNG)
    assert np.array_equal(out.cpu().numpy(), whole)
    assert np.array_equal(whole, L.light_f32(image, q, RNG))


def test_deterministic_and_independent_of_the_batch_slot(ua, batches):
    shape = (3, 33, 37)
    image = batches[shape]
    q = np.stack([L.with_iso(L.records(shape, "shadow")[1][0], 20.0, 0.5),
                  L.with_iso(L.records(shape, "flare")[1][1], 10.0, 0.2),
                  L.with_iso(L.records(shape, "fog")[1][1], 15.0, 0.8)])
    a = run(ua, image, q, RNG)
    assert np.array_equal(a, run(ua, image, q, RNG))
    perm = [2, 0, 1]
    b = run(ua, image[perm], q[perm], RNG[perm])
    for slot, n in enumerate(perm):
        assert np.array_equal(b[slot], a[n])
    c = run(ua, image[[1, 1, 1]], q[[1, 1, 1]], RNG[[1, 1, 1]])
    assert all(np.array_equal(c[s], a[1]) for s in range(3))
    other = RNG.copy()
    other[:, 0] += 1
    assert (run(ua, image, q, other) != a).mean() > 0.3         # another seed, other noise


def test_out_of_range_values_have_their_defined_result(ua, batches):
    """Raw records `validate_light` would refuse: the device clamps every count, T and k in float
    and decodes every unknown mode as none; the restatement decodes the same raw record."""
    shape = (3, 40, 52)
    image = batches[shape]
    odd = (3.0 + 1e-3, -1.0, 1.5, 1e30, float("inf"), float("nan"))
    for stage in L.STAGES:
        base = L.records(shape, stage)[0]
        for v in odd + (4.0, 0.0):                              # the mode
            q = base.copy()
            q[:, 3] = v
            assert np.array_equal(run(ua, image, q), image), (stage, v)
        for v in odd + (0.0, 1000.0):                           # the count
            q = base.copy()
            q[:, 4] = v
            assert np.array_equal(run(ua, image, q), L.light_f32(image, q)), (stage, v)
    fog = L.records(shape, "fog")[1]
    for v in odd + (0.0, 10.0, 100.0, 2.5, 8.9):                # k
        q = fog.copy()
        q[:, 7] = v
        assert np.array_equal(run(ua, image, q), L.light_f32(image, q)), v
    for v in (-1.0, float("nan"), float("inf"), 1e30, 0.0):     # the radius
        q = fog.copy()
        q[:, 5] = v
        got = run(ua, image, q)
        assert np.array_equal(got, L.light_f32(image, q)), v
    flare = L.records(shape, "flare")[1]
    for v in odd + (0.0, 1.0, 41.0, 1000.0):                    # T
        q = flare.copy()
        q[:, 8] = v
        assert np.array_equal(run(ua, image, q), L.light_f32(image, q)), v
    for v in (-5.0, float("nan"), 1e30):                        # Rs and a circle's radius
        q = flare.copy()
        q[:, 7] = v
        q[:, 18] = v
        assert np.array_equal(run(ua, image, q), L.light_f32(image, q)), v
    iso = iso_records(((12.0, float("nan")), (float("nan"), 0.5), (12.0, -3.0)))
    gray = L.gray_batch(3, 40, 52, 0, 60)
    assert np.array_equal(run(ua, gray, iso, RNG), L.light_f32(gray, iso, RNG))
    iso[:, 0] = (2.0, float("nan"), 0.5)                        # the flag: anything but 1 is off
    assert np.array_equal(run(ua, gray, iso, RNG), gray)


def test_captured_sequence_follows_new_records(ua, batches):
    shape = (3, 40, 52)
    N, H, W = shape
    image = L.gray_batch(N, H, W, 0, 60)
    x = torch.from_numpy(image).to(DEV)
    q1 = L.records(shape, "fog")[1]
    q1[0] = L.with_iso(q1[0], 0.0, 0.5)
    q2 = L.records(shape, "flare")[0]
    q2[1] = L.with_iso(L.records(shape, "shadow")[0][0], 9.0, 0.2)
    q2[2] = L.identity(1)[0]
    r1, r2 = RNG, RNG[[1, 2, 0]]
    q, r = torch.from_numpy(q1).to(DEV), dev_rng(ua, r1)
    out = torch.empty_like(x)
    ws = torch.empty(ua.lib().unet_augment_light_workspace_bytes(N), dtype=torch.uint8,
                     device=DEV)

    def sequence():
        ua.ops.augment_light_u8(x, q, r, out=out, workspace=ws)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sequence()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sequence()
    q.copy_(torch.from_numpy(q2))
    r.copy_(ua.augment.pack_rng(r2))
    graph.replay()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got, L.light_f32(image, q2, r2))
    assert not np.array_equal(got, L.light_f32(image, q1, r1))
    graph.replay()                                          # the sums are zeroed on every replay
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), got)


# ------------------------------------------------------------------------------------ end to end
E2E = (2, 64, 128)


def _e2e_config(ua, lighting, photometric=False):
    base = {**vars(R.record_configs(ua.augment)["perspective"]), "mask_border_value": 0.0,
            "dropout_prob": 1.0, "dropout_height": (4, 12), "dropout_width": (4, 12),
            "color_prob": 1.0, "brightness_contrast_prob": 0.5, "brightness_limit": (-0.1, 0.1),
            "contrast_limit": (-0.3, 0.2), "rgb_shift_prob": 0.5,
            "rgb_shift_limit": (10.0, 10.0, 10.0), "gray_group_prob": 1.0, "to_gray_prob": 1.0,
            "salt_pepper_prob": 1.0, "salt_p": (0.0, 0.05), "pepper_p": (0.0, 0.05)}
    if photometric:
        base.update(noise_group_prob=1.0, gaussian_blur_prob=1.0, gaussian_blur_limit=(0, 9))
    if lighting:
        # ToGray always fires, so the hue noise has no chroma to act on (sigma_h = 0 besides)
        # and the restatement is exact
        base.update(iso_noise_prob=1.0, iso_color_shift=(0.0, 0.0), iso_intensity=(0.2, 0.5),
                    lighting_group_prob=1.0, shadow_prob=0.3, sunflare_prob=0.3,
                    sunflare_src_radius=40, fog_prob=0.4, fog_coef=(0.3, 0.9),
                    fog_alpha_coef=0.08)
    return ua.augment.AugmentConfig(**base)


def _e2e_batch():
    image, mask = R.random_batch(*E2E, seed=300)
    return torch.from_numpy(image).to(DEV), torch.from_numpy(mask).to(DEV)


def _model(ua):
    model = ua.UNet()
    model.load_state_dict(O.fill_state_dict(23))
    model = model.to(DEV).train()
    model.matmul_precision = "bf16"
    model.dropout_mask_override = [m.to(DEV) if m is not None else None
                                   for m in O.draw_dropout_masks(5, E2E[0])]
    return model


def _draw(ua, cfg, seed, photometric):
    """the records BatchAugment(cfg, seed) draws on its first call"""
    N, H, W = E2E
    gen = torch.Generator().manual_seed(seed)
    q = None
    if photometric:
        p, r, groups = ua.augment.sample_params(cfg, N, H, W, gen, return_groups=True)
        p, r, q = ua.augment.sample_post(cfg, N, H, W, gen, p, r, groups)
    else:
        p, r = ua.augment.sample_params(cfg, N, H, W, gen)
    return p, r, q, ua.augment.sample_light(cfg, N, H, W, gen)


def _restate(x, m, p, r, q, lt):
    """the gather (salt / pepper there, or in the post stage when there is one), then light"""
    if q is None:
        mid, m32 = R.augment_f32(x.cpu().numpy(), m.cpu().numpy(), p.numpy(), r.numpy())
    else:
        r0 = r.numpy().copy()
        r0[:, 2:] = 0
        mid, m32 = R.augment_f32(x.cpu().numpy(), m.cpu().numpy(), p.numpy(), r0)
        mid = P.post_f32(mid, q.numpy(), r.numpy())
    return L.light_f32(mid, lt.numpy(), r.numpy()), m32


@pytest.mark.parametrize("photometric", [False, True], ids=["gather", "gather+post"])
def test_batch_augment_with_a_lighting_configuration_into_train_step(ua, photometric):
    x, m = _e2e_batch()
    cfg = _e2e_config(ua, True, photometric)
    seed = 5
    p, r, q, lt = _draw(ua, cfg, seed, photometric)
    assert (lt[:, 0] == 1).all() and (lt[:, 3] > 0).all() and (r[:, 2:] > 0).any()
    x32, m32 = _restate(x, m, p, r, q, lt)
    aug = ua.BatchAugment(cfg, seed=seed)
    assert aug.lighting and aug.photometric == photometric
    xa, ma = aug(x, m)
    assert xa.dtype == torch.uint8 and ma.dtype == torch.uint8
    assert np.array_equal(ma.cpu().numpy(), m32)
    print("differs from the restatement:", int((xa.cpu().numpy() != x32).sum()))
    assert np.array_equal(xa.cpu().numpy(), x32)
    # explicit records through params=(params, rng, warp, post, light), the other slot
    xb, mb = aug(x, m, params=(p, r, None, q, lt))
    assert torch.equal(xa, xb) and torch.equal(ma, mb)
    # the light stage off: what the stages in front of it wrote
    xc, _ = aug(x, m, params=(p, r, None, q, ua.augment.identity_light(E2E[0])))
    xd, _ = aug(x, m, params=(p, r, None, q))
    assert torch.equal(xc, xd) and not torch.equal(xc, xa)
    res = []
    for xi, mi in ((xa, ma), (torch.from_numpy(x32).to(DEV), torch.from_numpy(m32).to(DEV))):
        model = _model(ua)
        opt = ua.create_optimizer(model)
        loss = ua.train_step(model, opt, ua.SimpleLoss(target_layout="u8"), xi, mi,
                             input_layout="nhwc_u8")
        res.append((loss.clone(), model.flat_parameters()[0].detach().clone()))
    assert torch.isfinite(res[0][0])
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_batch_augment_without_a_lighting_configuration_is_unchanged(ua):
    x, m = _e2e_batch()
    cfg = _e2e_config(ua, False)
    N, H, W = E2E
    aug = ua.BatchAugment(cfg, seed=9)
    assert not aug.lighting and not aug.photometric and not aug.distortion
    gen = torch.Generator().manual_seed(9)
    for _ in range(3):                          # the generator is consumed as before, call by call
        p, r = ua.augment.sample_params(cfg, N, H, W, gen)
        want = ua.ops.augment_u8(x, m, p.to(DEV), dev_rng(ua, r))
        got = aug(x, m)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not aug._scratch and "light" not in aug._ring["slots"][0]["host"]
    # with the post stage and without lighting: the bytes of gather + post from the same seed
    cfg = _e2e_config(ua, False, photometric=True)
    aug = ua.BatchAugment(cfg, seed=4)
    gen = torch.Generator().manual_seed(4)
    p, r, groups = ua.augment.sample_params(cfg, N, H, W, gen, return_groups=True)
    p, r, q = ua.augment.sample_post(cfg, N, H, W, gen, p, r, groups)
    r0 = r.clone()
    r0[:, 2:] = 0
    mid, mw = ua.ops.augment_u8(x, m, p.to(DEV), dev_rng(ua, r0))
    want = ua.ops.augment_post_u8(mid, q.to(DEV), dev_rng(ua, r))
    got = aug(x, m)
    assert torch.equal(got[0], want) and torch.equal(got[1], mw)
    assert not any(key[0] == "light" for key in aug._scratch)
    assert "light" not in aug._ring["slots"][0]["host"]


def test_lighting_through_out_and_train_one_epoch(ua):
    x, m = _e2e_batch()
    cfg = _e2e_config(ua, True, photometric=True)
    model = _model(ua)
    opt = ua.create_optimizer(model)
    step = ua.GraphedTrainStep(model, opt, ua.SimpleLoss(target_layout="u8"), x, m,
                               input_layout="nhwc_u8")
    aug = ua.BatchAugment(cfg, seed=2)
    xa, ma = aug(x, m, out=(step.images, step.masks))
    assert xa.data_ptr() == step.images.data_ptr() and ma.data_ptr() == step.masks.data_ptr()
    want = ua.BatchAugment(cfg, seed=2)(x, m)
    assert torch.equal(xa, want[0]) and torch.equal(ma, want[1])
    assert torch.isfinite(step(xa, ma))
    # with the distortion group as well: the warp in front, post and light behind
    both = ua.augment.AugmentConfig(**{**vars(cfg), "distort_group_prob": 1.0,
                                       "grid_distortion_prob": 1.0, "grid_num_steps": 5,
                                       "grid_distort_limit": 0.3})
    xw, mw = ua.BatchAugment(both, seed=2)(x, m)
    assert not torch.equal(xw, xa) and xw.shape == xa.shape
    loader = [{"image": x, "mask": m, "which": torch.tensor([0, 1])}]
    res = []
    for augment in (ua.BatchAugment([_e2e_config(ua, False), cfg], seed=1),
                    ua.BatchAugment([cfg, _e2e_config(ua, False)], seed=1)):
        mdl = _model(ua)
        res.append(ua.train_one_epoch(mdl, loader, ua.create_optimizer(mdl),
                                      ua.SimpleLoss(target_layout="u8"), DEV, augment=augment,
                                      input_layout="nhwc_u8"))
    assert all(np.isfinite(v) for v in res) and res[0] != res[1]


# ----------------------------------------------------- the chain of stages, record by record
@pytest.fixture(scope="module")
def chain_records(ua):
    """(params, rng, warp, post, light) of one draw with every stage on; never modified"""
    N, H, W = E2E
    cfg = ua.augment.AugmentConfig(**{
        **vars(_e2e_config(ua, True, photometric=True)), "distort_group_prob": 1.0,
        "elastic_prob": 0.5, "elastic_alpha": 3.0, "elastic_sigma": 2.0,
        "elastic_alpha_affine": 2.0, "grid_distortion_prob": 0.5, "grid_num_steps": 5,
        "grid_distort_limit": 0.3})
    for seed in range(20):          # a draw with one elastic and one grid sample
        gen = torch.Generator().manual_seed(seed)
        p, r, groups = ua.augment.sample_params(cfg, N, H, W, gen, return_groups=True)
        w = ua.augment.sample_warp(cfg, N, H, W, gen)
        if sorted(w[:, 0].tolist()) == [ua.augment.WARP_ELASTIC, ua.augment.WARP_GRID]:
            break
    p, r, q = ua.augment.sample_post(cfg, N, H, W, gen, p, r, groups)
    lt = ua.augment.sample_light(cfg, N, H, W, gen)
    assert sorted(w[:, 0].tolist()) == [ua.augment.WARP_ELASTIC, ua.augment.WARP_GRID]
    assert (q[:, ua.augment.Q_BLUR] > 0).all() and (lt[:, 3] > 0).all() and (r[:, 2:] > 0).any()
    return p, r, w, q, lt


@pytest.mark.parametrize("light", [False, True], ids=["", "light"])
@pytest.mark.parametrize("post", [False, True], ids=["", "post"])
@pytest.mark.parametrize("warp", [False, True], ids=["gather", "warp"])
def test_batch_augment_is_the_explicit_chain_of_stages(ua, chain_records, warp, post, light):
    """every on / off combination of the three optional records through params=: the bytes of
    the chain of `ops.*` calls written out here, with and without `out=`; the last stage writes
    the caller's tensor, and no scratch of a stage that is off is allocated"""
    N, H, W = E2E
    x, m = _e2e_batch()
    p, r, w, q, lt = chain_records
    w, q, lt = w if warp else None, q if post else None, lt if light else None
    # the chain: gather or warp gather (salt / pepper off in front of a post stage), post, light
    dp, dr = p.to(DEV), dev_rng(ua, r)
    r0 = r.clone()
    r0[:, 2:] = 0
    gather_rng = dev_rng(ua, r0) if post else dr
    if warp:
        field = ua.ops.elastic_field(w.to(DEV), dr, (H, W))
        want, want_mask = ua.ops.augment_warp_u8(x, m, dp, gather_rng, w.to(DEV), field)
    else:
        want, want_mask = ua.ops.augment_u8(x, m, dp, gather_rng)
    if post:
        want = ua.ops.augment_post_u8(want, q.to(DEV), dr)
    if light:
        want = ua.ops.augment_light_u8(want, lt.to(DEV), dr)

    aug = ua.BatchAugment(ua.augment.AugmentConfig(), seed=0)
    got, got_mask = aug(x, m, params=(p, r, w, q, lt))
    assert torch.equal(got, want) and torch.equal(got_mask, want_mask)
    out = (torch.full_like(x, 7), torch.full_like(m, 7))
    got, got_mask = aug(x, m, params=(p, r, w, q, lt), out=out)
    assert got.data_ptr() == out[0].data_ptr() and got_mask.data_ptr() == out[1].data_ptr()
    assert torch.equal(out[0], want) and torch.equal(out[1], want_mask)
    ran = {k for k, on in (("field", warp), ("post", post), ("light", light)) if on}
    assert {key[0] for key in aug._scratch} == ran
    assert len(aug._scratch) == len(ran)
    staged = {k for k, on in (("warp", warp), ("post", post), ("gather_rng", post),
                              ("light", light)) if on}
    assert set(aug._ring["slots"][0]["host"]) == {"params", "rng"} | staged
