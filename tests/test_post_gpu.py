"""GPU (-m gpu): `unet_augment_post_u8` (HSV shift, equalize / CLAHE, blur, salt / pepper) and
`BatchAugment` with a photometric configuration.

Yardsticks as in test_distort_gpu.py: the kernels' arithmetic is normative, so the output must be
BYTE equal to the fp32 restatement of tests/tools/post_ref.py, and it must stay inside the
analytic bounds of `check_against_f64` (every segment at most 1 apart from fp64, only at rounding
ties).  Shapes: 16 x 24 (smaller than a 32 x 32 tile), 33 x 37 with N = 3 (crosses the tile edge
by one pixel on both axes), 40 x 52 and 64 x 64 (several tiles, the 8 x 8 CLAHE grid); at every
shape the reflected border lies inside a halo.  The records are those of post_ref.records, which
test_post_cpu.py holds against fp64 on the CPU."""
import importlib.util
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


P = _load("post_ref")
R = P.R
RNG = np.array([[11, 22, 1 << 28, 1 << 27], [33, 44, 1 << 27, 0], [55, 66, 0, 1 << 28]],
               dtype=np.int64)


@pytest.fixture(scope="module")
def batches():
    """{(shape, stage): image} as numpy uint8; drawn once, never modified"""
    return {(s, st): P.batch(s, st) for s in P.SHAPES for st in P.STAGES}


def dev_rng(ua, rng):
    return ua.augment.pack_rng(rng).to(DEV) if rng is not None else None


def run(ua, image, post, rng=None, **kw):
    out = ua.ops.augment_post_u8(torch.from_numpy(image).to(DEV),
                                 torch.as_tensor(post, dtype=torch.float32).to(DEV),
                                 dev_rng(ua, rng), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("shape", P.SHAPES, ids=str)
def test_identity_record_copies_and_salt_pepper_is_that_of_augment_u8(ua, batches, shape):
    N, H, W = shape
    image = batches[(shape, "hsv")]
    q = ua.augment.identity_post(N)
    assert np.array_equal(run(ua, image, q), image)
    rng = RNG[:N]
    got = run(ua, image, q, rng)
    x = torch.from_numpy(image).to(DEV)
    want, _ = ua.ops.augment_u8(x, None, ua.augment.identity_params(N).to(DEV), dev_rng(ua, rng))
    assert np.array_equal(got, want.cpu().numpy())
    assert np.array_equal(got, P.post_f32(image, q.numpy(), rng))
    assert (got != image).any()
    # zero thresholds, and a caller's workspace and output
    zero = rng.copy()
    zero[:, 2:] = 0
    ws = torch.empty(ua.lib().unet_augment_post_workspace_bytes(N), dtype=torch.uint8, device=DEV)
    buf = torch.empty_like(x)
    out = ua.ops.augment_post_u8(x, q.to(DEV), dev_rng(ua, zero), out=buf, workspace=ws)
    assert out.data_ptr() == buf.data_ptr() and torch.equal(out, x)
    with pytest.raises(ua.UNetHipError):
        ua.ops.augment_post_u8(x, q.to(DEV), out=x)
    with pytest.raises(ua.UNetHipError):
        ua.ops.augment_post_u8(x, q.to(DEV), workspace=ws[:-16])


@pytest.mark.parametrize("stage", P.STAGES)
@pytest.mark.parametrize("shape", P.SHAPES, ids=str)
def test_random_records_against_both_restatements(ua, batches, shape, stage):
    """Six (nine at N = 3) records per stage and shape: the bytes of the fp32 restatement, the
    bounds against fp64.  "all" also carries salt / pepper."""
    N, H, W = shape
    image = batches[(shape, stage)]
    rng = RNG[:N] if stage == "all" else None
    for q in P.records(ua.augment, shape, stage):
        got = run(ua, image, q, rng)
        want = P.post_f32(image, q, rng)
        print(shape, stage, "differs from fp32 restatement:", int((got != want).sum()),
              "changed", float((got != image).mean()))
        for n in range(N):
            skip = P.salt_pepper_hit(rng[n], H, W)[..., None] if rng is not None else None
            fig = P.check_against_f64(image[n], q[n], final=got[n], skip=skip)
            print(shape, stage, n, "segments", len(fig), "apart from fp64 (count, tie distance):",
                  {k: (v["differing"], v["max_tie_distance"]) for k, v in fig.items()
                   if v.get("differing")})
        assert np.array_equal(got, want)
        assert (got != image).mean() > 0.3


def test_mixed_batch_changes_the_right_samples_only(ua, batches):
    shape = (3, 33, 37)
    N, H, W = shape
    image = batches[(shape, "clahe")]
    q = ua.augment.identity_post(N).numpy()
    q[1, 4] = 1                                             # none / equalize / CLAHE 3 x 1
    q[2, 4], q[2, 5], q[2, 6], q[2, 7] = 2, 2.0, 3, 1
    got = run(ua, image, q)
    assert np.array_equal(got[0], image[0])
    assert np.array_equal(got, P.post_f32(image, q))
    assert (got[1] != image[1]).mean() > 0.3 and (got[2] != image[2]).mean() > 0.3
    # a grid that does not divide the shape behaves as none, in both kernels
    q[2, 6] = 2
    got = run(ua, image, q)
    assert np.array_equal(got[2], image[2]) and np.array_equal(got, P.post_f32(image, q))


def test_the_two_halves_are_the_whole(ua, batches):
    shape = (2, 64, 64)
    N, H, W = shape
    image = batches[(shape, "all")]
    q = P.records(ua.augment, shape, "all")[1]
    x, dq, dr = torch.from_numpy(image).to(DEV), torch.from_numpy(q).to(DEV), dev_rng(ua, RNG[:N])
    lib = ua.lib()
    need = lib.unet_augment_post_workspace_bytes(N)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.empty_like(x)
    stream = ua.ops._stream()
    ua._lib.check(lib.unet_augment_post_hist(x.data_ptr(), dq.data_ptr(), ws.data_ptr(), need,
                                             N, H, W, stream))
    ua._lib.check(lib.unet_augment_post_apply(x.data_ptr(), out.data_ptr(), dq.data_ptr(),
                                              dr.data_ptr(), ws.data_ptr(), need, N, H, W, stream))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), run(ua, image, q, RNG[:N]))


def test_deterministic_and_independent_of_the_batch_slot(ua, batches):
    shape = (3, 33, 37)
    N, H, W = shape
    image = batches[(shape, "all")]
    q = P.records(ua.augment, shape, "all")[1]
    a = run(ua, image, q, RNG)
    assert np.array_equal(a, run(ua, image, q, RNG))
    perm = [2, 0, 1]
    b = run(ua, image[perm], q[perm], RNG[perm])
    for slot, n in enumerate(perm):
        assert np.array_equal(b[slot], a[n])
    c = run(ua, image[[1, 1, 1]], q[[1, 1, 1]], RNG[[1, 1, 1]])
    assert all(np.array_equal(c[s], a[1]) for s in range(3))


def test_out_of_range_modes_and_radii_have_their_defined_result(ua, batches):
    """Raw records `validate_post` would refuse: the device clamps in float and decodes every
    unknown mode as off; the restatement decodes the same raw record."""
    shape = (2, 40, 52)
    N, H, W = shape
    image = batches[(shape, "all")]
    base = P.records(ua.augment, shape, "all")[0]
    sep = P.records(ua.augment, shape, "separable")[2]      # R = 4 taps
    den = P.records(ua.augment, shape, "dense")[1]          # R = 3 weights
    for at, vals in ((4, (3.0, -1.0, 1.5, 1e30, float("nan"))),
                     (8, (3.0, -2.0, 0.5, float("inf"))),
                     (0, (2.0, -1.0, float("nan")))):
        for v in vals:
            q = base.copy()
            q[:, at] = v
            assert np.array_equal(run(ua, image, q), P.post_f32(image, q)), (at, v)
    for rec in (sep, den):
        for v in (0.0, -5.0, 100.0, 2.5, 1e30, float("inf"), float("nan")):
            q = rec.copy()
            q[:, 9] = v
            got = run(ua, image, q)
            assert np.array_equal(got, P.post_f32(image, q)), v
    q = base.copy()
    q[:, 4], q[:, 5], q[:, 6], q[:, 7] = 2, float("nan"), 4, 4       # a NaN clip limit: climit 1
    assert np.array_equal(run(ua, image, q), P.post_f32(image, q))
    for grid in ((9, 4), (4, 0), (2.5, 4), (float("nan"), 4), (-3, 1e30)):
        q[:, 5], q[:, 6], q[:, 7] = 2.0, grid[0], grid[1]
        assert np.array_equal(run(ua, image, q), P.post_f32(image, q)), grid


def test_captured_sequence_follows_new_records(ua, batches):
    shape = (2, 40, 52)
    N, H, W = shape
    image = batches[(shape, "all")]
    x = torch.from_numpy(image).to(DEV)
    q1 = P.records(ua.augment, shape, "all")[0]
    q2 = P.records(ua.augment, shape, "all")[2]
    q2[0, 4] = 0                                            # sample 0 drops its histogram op
    r1, r2 = RNG[:N], RNG[1:N + 1]
    q, r = torch.from_numpy(q1).to(DEV), dev_rng(ua, r1)
    out = torch.empty_like(x)
    ws = torch.empty(ua.lib().unet_augment_post_workspace_bytes(N), dtype=torch.uint8, device=DEV)

    def sequence():
        ua.ops.augment_post_u8(x, q, r, out=out, workspace=ws)

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
    assert np.array_equal(got, P.post_f32(image, q2, r2))
    assert not np.array_equal(got, P.post_f32(image, q1, r1))
    graph.replay()                                          # the counts are zeroed on every replay
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), got)


# ------------------------------------------------------------------------------------ end to end
E2E = (2, 64, 128)


def _e2e_config(ua, photometric):
    base = {**vars(R.record_configs(ua.augment)["perspective"]), "mask_border_value": 0.0,
            "dropout_prob": 1.0, "dropout_height": (4, 12), "dropout_width": (4, 12),
            "color_prob": 1.0, "brightness_contrast_prob": 0.5, "brightness_limit": (-0.1, 0.1),
            "contrast_limit": (-0.3, 0.2), "rgb_shift_prob": 0.5,
            "rgb_shift_limit": (10.0, 10.0, 10.0), "gray_group_prob": 1.0, "to_gray_prob": 0.2,
            "salt_pepper_prob": 1.0, "salt_p": (0.0, 0.05), "pepper_p": (0.0, 0.05)}
    if photometric:
        base.update(hsv_prob=1.0, hue_shift_limit=10.0, sat_shift_limit=30.0,
                    val_shift_limit=20.0, clahe_prob=0.5, clahe_clip_limit=4.0,
                    clahe_tile_grid=(8, 8), equalize_prob=0.5, noise_group_prob=1.0,
                    gaussian_blur_prob=0.5, gaussian_blur_limit=(0, 9), motion_blur_prob=0.5,
                    motion_blur_limit=(3, 7))
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


def _draw(ua, cfg, seed):
    """the records BatchAugment(cfg, seed) draws on its first call"""
    N, H, W = E2E
    gen = torch.Generator().manual_seed(seed)
    p, r, groups = ua.augment.sample_params(cfg, N, H, W, gen, return_groups=True)
    return ua.augment.sample_post(cfg, N, H, W, gen, p, r, groups)


def _restate(x, m, p, r, q):
    """the gather with salt / pepper off, then the post stage with it on"""
    r0 = r.numpy().copy()
    r0[:, 2:] = 0
    mid, m32 = R.augment_f32(x.cpu().numpy(), m.cpu().numpy(), p.numpy(), r0)
    return P.post_f32(mid, q.numpy(), r.numpy()), m32


def test_batch_augment_with_photometric_members_into_train_step(ua):
    x, m = _e2e_batch()
    cfg = _e2e_config(ua, True)
    seed = 5
    p, r, q = _draw(ua, cfg, seed)
    assert (q[:, 0] == 1).any() or (q[:, 4] > 0).any()
    assert (q[:, 8] > 0).all() and (r[:, 2:] > 0).any()
    x32, m32 = _restate(x, m, p, r, q)
    aug = ua.BatchAugment(cfg, seed=seed)
    assert aug.photometric
    xa, ma = aug(x, m)
    assert xa.dtype == torch.uint8 and ma.dtype == torch.uint8
    assert np.array_equal(xa.cpu().numpy(), x32) and np.array_equal(ma.cpu().numpy(), m32)
    # explicit records through params=(params, rng, warp, post), a second call (the other slot)
    xb, mb = aug(x, m, params=(p, r, None, q))
    assert torch.equal(xa, xb) and torch.equal(ma, mb)
    res = []
    for xi, mi in ((xa, ma), (torch.from_numpy(x32).to(DEV), torch.from_numpy(m32).to(DEV))):
        model = _model(ua)
        opt = ua.create_optimizer(model)
        loss = ua.train_step(model, opt, ua.SimpleLoss(target_layout="u8"), xi, mi,
                             input_layout="nhwc_u8")
        res.append((loss.clone(), model.flat_parameters()[0].detach().clone()))
    assert torch.isfinite(res[0][0])
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_batch_augment_without_photometric_members_is_unchanged(ua):
    x, m = _e2e_batch()
    cfg = _e2e_config(ua, False)
    N, H, W = E2E
    aug = ua.BatchAugment(cfg, seed=9)
    assert not aug.photometric and not aug.distortion
    gen = torch.Generator().manual_seed(9)
    for _ in range(3):                          # the generator is consumed as before, call by call
        p, r = ua.augment.sample_params(cfg, N, H, W, gen)
        want = ua.ops.augment_u8(x, m, p.to(DEV), dev_rng(ua, r))
        got = aug(x, m)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not aug._scratch and "post" not in aug._ring["slots"][0]["host"]


def test_photometric_through_out_and_train_one_epoch(ua):
    x, m = _e2e_batch()
    cfg = _e2e_config(ua, True)
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
    # with the distortion group as well: the warp in front, the post stage behind
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
