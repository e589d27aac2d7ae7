"""GPU (-m gpu): `unet_elastic_field`, `unet_augment_warp_u8` and `BatchAugment` with a
distortion configuration.

Yardsticks as in test_augment_gpu.py: the kernels' arithmetic is normative, so the field must be
BIT equal and the augmented pair BYTE equal to the fp32 restatements of tests/tools/distort_ref.py;
the fp64 restatements bound both (the field within (2 L + 4) 2^-24 alpha, the pair within
`check_against_f64`).  Shapes, N = 2 each: 16 x 24 (smaller than a 32 x 32 tile and than 2 R + 1:
the halo covers more than the image), 33 x 37 (one pixel per thread, partial tiles on both axes),
40 x 52 (four pixels per thread, several tiles); sigma 0.5 / 4 / 6 gives R = 2, 12 and the cap
of 16.  The records are those of distort_ref.cases, which test_distort_cpu.py holds against fp64
on the CPU."""
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


D = _load("distort_ref")
R = D.R
SHAPES = D.SHAPES


@pytest.fixture(scope="module")
def batch():
    """{shape: (image, mask)} as numpy uint8; drawn once, never modified"""
    return {s: R.random_batch(*s, seed=s[1]) for s in SHAPES}


def dev_rng(ua, rng):
    return ua.augment.pack_rng(rng).to(DEV) if rng is not None else None


def run_field(ua, warp, rng, shape, out=None):
    N, H, W = shape
    f = ua.ops.elastic_field(torch.as_tensor(warp, dtype=torch.float32).to(DEV), dev_rng(ua, rng),
                             (H, W), out=out)
    torch.cuda.synchronize()
    return f


def run(ua, image, mask, params, rng, warp, field=None):
    """one gather launch on numpy / CPU inputs -> numpy outputs; field is a device tensor"""
    o, m = ua.ops.augment_warp_u8(
        torch.from_numpy(image).to(DEV),
        torch.from_numpy(mask).to(DEV) if mask is not None else None,
        torch.as_tensor(params, dtype=torch.float32).to(DEV), dev_rng(ua, rng),
        torch.as_tensor(warp, dtype=torch.float32).to(DEV), field)
    torch.cuda.synchronize()
    return o.cpu().numpy(), (m.cpu().numpy() if m is not None else None)


# ------------------------------------------------------------------------------------ the field
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_field_is_the_fp32_restatement_bit_for_bit(ua, shape):
    N, H, W = shape
    for _, r, w in D.cases(ua.augment, 1, shape):
        got = run_field(ua, w, r, shape).cpu().numpy()
        f32, f64 = D.field_f32(w.numpy(), r.numpy(), N, H, W), D.field_f64(w.numpy(), r.numpy(),
                                                                           N, H, W)
        for n in range(N):
            err = float(np.abs(got[n].astype(np.float64) - f64[n]).max())
            print(shape, "R", int(w[n, 8]), "differs from fp32 restatement:",
                  int((got[n].view(np.uint32) != f32[n].view(np.uint32)).sum()),
                  "max |gpu - f64|", err, "bound", D.field_bound(w[n].numpy()))
            assert err <= D.field_bound(w[n].numpy())
        assert np.array_equal(got.view(np.uint32), f32.view(np.uint32))
        assert np.abs(got).max() > 0


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_field_touches_elastic_samples_only(ua, shape):
    N, H, W = shape
    _, r, w = D.cases(ua.augment, 1, shape)[1]
    for other in (0.0, 2.0, 3.0):
        w2 = w.clone()
        w2[1, 0] = other                        # sample 1 is not elastic
        buf = torch.full((N, H, W, 2), 7.25, dtype=torch.float32, device=DEV)
        got = run_field(ua, w2, r, shape, out=buf)
        assert got.data_ptr() == buf.data_ptr()
        got = got.cpu().numpy()
        assert (got[1] == 7.25).all()           # its slice of the pre-filled buffer is untouched
        want = D.field_f32(w.numpy(), r.numpy(), N, H, W)
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
    # a fresh tensor: exactly 0 for the neighbours of an elastic sample
    w2 = w.clone()
    w2[0, 0] = 0.0
    got = run_field(ua, w2, r, shape).cpu().numpy()
    assert not got[0].any() and got[1].any()


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_field_without_rng_is_zero(ua, shape):
    N, H, W = shape
    _, r, w = D.cases(ua.augment, 1, shape)[2]
    buf = torch.full((N, H, W, 2), 7.25, dtype=torch.float32, device=DEV)
    got = run_field(ua, w, None, shape, out=buf).cpu().numpy()
    assert not got.any()


def test_field_depends_on_seed_and_pixel_not_on_the_slot(ua):
    shape = (2, 40, 52)
    N, H, W = shape
    _, r, w = D.cases(ua.augment, 1, shape)[1]
    a = run_field(ua, w, r, shape).cpu().numpy()
    b = run_field(ua, w, r, shape).cpu().numpy()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # the same record and seed in slot 0 and slot 1: the same field
    c = run_field(ua, w[[0, 0]], r[[0, 0]], shape).cpu().numpy()
    assert np.array_equal(c[0].view(np.uint32), c[1].view(np.uint32))
    assert np.array_equal(c[0].view(np.uint32), a[0].view(np.uint32))
    d = run_field(ua, w[[1, 0]], r[[1, 0]], shape).cpu().numpy()
    assert np.array_equal(d[1].view(np.uint32), a[0].view(np.uint32))
    assert np.array_equal(d[0].view(np.uint32), a[1].view(np.uint32))
    r2 = r.clone()
    r2[:, 0] += 1
    e = run_field(ua, w, r2, shape).cpu().numpy()
    assert all((a[n] != e[n]).mean() > 0.9 for n in range(N))


# ------------------------------------------------------------------------------------ the gather
def _noisy(ua, shape, seed):
    """perspective + Gaussian noise + salt and pepper (+ a hole): everything of the plain kernel"""
    N, H, W = shape
    cfg = ua.augment.AugmentConfig(**{
        **vars(R.record_configs(ua.augment)["perspective"]), "noise_group_prob": 1.0,
        "gauss_noise_prob": 1.0, "gauss_var_limit": (9.0, 16.0), "salt_pepper_prob": 1.0,
        "salt_p": (0.02, 0.05), "pepper_p": (0.02, 0.05), "dropout_prob": 1.0,
        "dropout_height": (3, 9), "dropout_width": (3, 9), "color_prob": 1.0,
        "brightness_contrast_prob": 1.0, "contrast_limit": (-0.3, 0.2)})
    return ua.augment.sample_params(cfg, N, H, W, torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_mode_none_is_augment_u8_byte_for_byte(ua, batch, shape):
    N, H, W = shape
    image, mask = batch[shape]
    p, r = _noisy(ua, shape, 40)
    x, t = torch.from_numpy(image).to(DEV), torch.from_numpy(mask).to(DEV)
    want = ua.ops.augment_u8(x, t, p.to(DEV), dev_rng(ua, r))
    junk = torch.full((N, H, W, 2), 3.5, dtype=torch.float32, device=DEV)
    for field in (None, junk):
        o, m = run(ua, image, mask, p, r, ua.augment.identity_warp(N), field)
        assert np.array_equal(o, want[0].cpu().numpy())
        assert np.array_equal(m, want[1].cpu().numpy())
    # without a mask, and degenerate records of modes 2 and 3: still those bytes
    o, m = run(ua, image, None, p, r, ua.augment.identity_warp(N))
    assert m is None and np.array_equal(o, want[0].cpu().numpy())
    gen = torch.Generator().manual_seed(0)
    flat = ua.augment.sample_warp(ua.AugmentConfig(
        distort_group_prob=1.0, grid_distortion_prob=1.0, grid_num_steps=5,
        grid_distort_limit=0.0), N, H, W, gen)
    centred = ua.augment.sample_warp(ua.AugmentConfig(
        distort_group_prob=1.0, optical_distortion_prob=1.0), N, H, W, gen)
    assert (flat[:, 0] == 2).all() and (centred[:, 0] == 3).all() and (centred[:, 3] == 0).all()
    for w in (flat, centred):
        o, m = run(ua, image, mask, p, r, w)
        assert np.array_equal(o, want[0].cpu().numpy())
        assert np.array_equal(m, want[1].cpu().numpy())


@pytest.mark.parametrize("mode", sorted(D.MODES), ids=lambda m: D.MODES[m])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_random_records_against_both_restatements(ua, batch, shape, mode):
    """Six records per mode and shape, each composed with a random perspective record: the bytes
    of the fp32 restatement, the bounds against fp64."""
    N, H, W = shape
    image, mask = batch[shape]
    for p, r, w in D.cases(ua.augment, mode, shape):
        field = run_field(ua, w, r, shape) if mode == 1 else None
        o, m = run(ua, image, mask, p, r, w, field)
        pn, rn, wn = p.numpy(), r.numpy(), w.numpy()
        f32 = D.field_f32(wn, rn, N, H, W) if mode == 1 else None
        f64 = D.field_f64(wn, rn, N, H, W) if mode == 1 else None
        o32, m32 = D.augment_warp_f32(image, mask, pn, rn, wn, f32)
        val, _, m64, near = D.augment_warp_f64(image, mask, pn, rn, wn, f64)
        print(shape, D.MODES[mode], "differs from fp32 restatement:", int((o != o32).sum()),
              int((m != m32).sum()))
        fig = R.check_against_f64(o, m, val, m64, near, max_left_out=0.01)
        print(shape, D.MODES[mode], fig)
        assert np.array_equal(o, o32)
        assert np.array_equal(m, m32)
        plain, _ = R.augment_f32(image, mask, pn, rn)
        assert (o != plain).mean() > 0.3        # the warp did something
    if mode == 1:       # a null field: the affine part alone
        o, m = run(ua, image, mask, p, r, w, None)
        o32, m32 = D.augment_warp_f32(image, mask, pn, rn, wn, None)
        assert np.array_equal(o, o32) and np.array_equal(m, m32)


def test_mixed_batch_with_noise_is_deterministic_and_slot_independent(ua, batch):
    shape = (2, 40, 52)
    N, H, W = shape
    image, mask = batch[shape]
    p, r = _noisy(ua, shape, 41)
    q = p.clone()
    q[:, 14] = 0                                # the restatement holds bytes without Gaussian noise
    w = torch.stack([D.cases(ua.augment, 1, shape)[1][2][0],
                     D.cases(ua.augment, 3, shape)[0][2][1]])
    ua.augment.validate_warp(w, p, H, W)
    field = run_field(ua, w, r, shape)
    a, am = run(ua, image, mask, p, r, w, field)
    b, bm = run(ua, image, mask, p, r, w, field)
    assert np.array_equal(a, b) and np.array_equal(am, bm)
    o, m = run(ua, image, mask, q, r, w, field)
    o32, m32 = D.augment_warp_f32(image, mask, q.numpy(), r.numpy(), w.numpy(),
                                  D.field_f32(w.numpy(), r.numpy(), N, H, W))
    assert np.array_equal(o, o32) and np.array_equal(m, m32) and np.array_equal(am, m32)
    perm = [1, 0]
    field2 = run_field(ua, w[perm], r[perm], shape)
    d, dm = run(ua, image[perm], mask[perm], p[perm], r[perm], w[perm], field2)
    for slot, n in enumerate(perm):
        assert np.array_equal(d[slot], a[n]) and np.array_equal(dm[slot], am[n])


def test_captured_launch_pair_follows_new_records(ua, batch):
    shape = (2, 40, 52)
    N, H, W = shape
    image, mask = batch[shape]
    x, t = torch.from_numpy(image).to(DEV), torch.from_numpy(mask).to(DEV)
    p1, r1, w1 = D.cases(ua.augment, 1, shape)[0]
    p2, r2, w2 = D.cases(ua.augment, 1, shape)[2]
    w2 = w2.clone()
    w2[1] = D.cases(ua.augment, 2, shape)[0][2][1]      # sample 1 turns from elastic to grid
    ua.augment.validate_warp(w2, p2, H, W)
    p, r, w = p1.to(DEV), dev_rng(ua, r1), w1.to(DEV)
    field = torch.zeros((N, H, W, 2), dtype=torch.float32, device=DEV)
    out = (torch.empty_like(x), torch.empty_like(t))

    def pair():
        ua.ops.elastic_field(w, r, (H, W), out=field)
        ua.ops.augment_warp_u8(x, t, p, r, w, field, out=out)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pair()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pair()
    p.copy_(p2)
    r.copy_(ua.augment.pack_rng(r2))
    w.copy_(w2)
    graph.replay()
    torch.cuda.synchronize()
    got = (out[0].cpu().numpy(), out[1].cpu().numpy())
    f32 = D.field_f32(w2.numpy(), r2.numpy(), N, H, W)
    o32, m32 = D.augment_warp_f32(image, mask, p2.numpy(), r2.numpy(), w2.numpy(), f32)
    assert np.array_equal(got[0], o32) and np.array_equal(got[1], m32)
    first = D.augment_warp_f32(image, mask, p1.numpy(), r1.numpy(), w1.numpy(),
                               D.field_f32(w1.numpy(), r1.numpy(), N, H, W))
    assert not np.array_equal(got[0], first[0])
    assert np.array_equal(field[0].cpu().numpy().view(np.uint32), f32[0].view(np.uint32))


# ------------------------------------------------------------------------------------ end to end
E2E = (2, 64, 128)


def _e2e_config(ua, distortion):
    base = {**vars(R.record_configs(ua.augment)["perspective"]), "mask_border_value": 0.0,
            "dropout_prob": 1.0, "dropout_height": (4, 12), "dropout_width": (4, 12),
            "color_prob": 1.0, "brightness_contrast_prob": 0.5, "brightness_limit": (-0.1, 0.1),
            "contrast_limit": (-0.3, 0.2), "rgb_shift_prob": 0.5,
            "rgb_shift_limit": (10.0, 10.0, 10.0), "salt_pepper_prob": 1.0,
            "salt_p": (0.0, 0.05), "pepper_p": (0.0, 0.05)}
    if distortion:
        base.update(distort_group_prob=1.0, elastic_prob=1.0, elastic_alpha=8.0,
                    elastic_sigma=4.0, elastic_alpha_affine=3.0, grid_distortion_prob=1.0,
                    grid_num_steps=5, grid_distort_limit=0.3, optical_distortion_prob=1.0,
                    optical_distort_limit=0.2, optical_shift_limit=0.15)
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


def test_batch_augment_with_distortion_into_train_step(ua):
    x, m = _e2e_batch()
    cfg = _e2e_config(ua, True)
    N, H, W = E2E
    seed = 5
    # the records BatchAugment(seed) will draw: params first, then the warp, from one generator
    gen = torch.Generator().manual_seed(seed)
    p, r = ua.augment.sample_params(cfg, N, H, W, gen)
    w = ua.augment.sample_warp(cfg, N, H, W, gen)
    assert (w[:, 0] > 0).all()
    f32 = D.field_f32(w.numpy(), r.numpy(), N, H, W)
    x32, m32 = D.augment_warp_f32(x.cpu().numpy(), m.cpu().numpy(), p.numpy(), r.numpy(),
                                  w.numpy(), f32)
    aug = ua.BatchAugment(cfg, seed=seed)
    assert aug.distortion
    xa, ma = aug(x, m)
    assert xa.dtype == torch.uint8 and ma.dtype == torch.uint8
    assert np.array_equal(xa.cpu().numpy(), x32) and np.array_equal(ma.cpu().numpy(), m32)
    # explicit records through params=(params, rng, warp), a second call (the other ring slot)
    xb, mb = aug(x, m, params=(p, r, w))
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


def test_batch_augment_without_distortion_is_unchanged(ua):
    x, m = _e2e_batch()
    cfg = _e2e_config(ua, False)
    N, H, W = E2E
    aug = ua.BatchAugment(cfg, seed=9)
    assert not aug.distortion
    gen = torch.Generator().manual_seed(9)
    for _ in range(3):                          # the generator is consumed as before, call by call
        p, r = ua.augment.sample_params(cfg, N, H, W, gen)
        want = ua.ops.augment_u8(x, m, p.to(DEV), dev_rng(ua, r))
        got = aug(x, m)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not aug._scratch and "warp" not in aug._ring["slots"][0]["host"]


def test_distortion_through_out_and_train_one_epoch(ua):
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
    loader = [{"image": x, "mask": m, "which": torch.tensor([0, 1])}]
    res = []
    for augment in (ua.BatchAugment([_e2e_config(ua, False), cfg], seed=1),
                    ua.BatchAugment([cfg, _e2e_config(ua, False)], seed=1)):
        mdl = _model(ua)
        res.append(ua.train_one_epoch(mdl, loader, ua.create_optimizer(mdl),
                                      ua.SimpleLoss(target_layout="u8"), DEV, augment=augment,
                                      input_layout="nhwc_u8"))
    assert all(np.isfinite(v) for v in res) and res[0] != res[1]
