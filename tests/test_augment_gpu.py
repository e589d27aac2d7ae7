"""GPU (-m gpu): `unet_augment_u8` and what is built on it.

The kernel's arithmetic is normative (every fp32 operation rounded on its own), so the first
yardstick is BYTE EQUALITY with the fp32 restatement of tests/tools/augment_ref.py; the second is
the fp64 restatement through F.grid_sample, within the bounds `check_against_f64` states (1
level, only at rounding ties; mask only at cell boundaries, at most 1 % of a case's pixels left
out).  Shapes: (3, 37, 50) takes the one-pixel-per-thread path, (3, 96, 160) and (2, 64, 128) the
four-pixel path with more than one workgroup, and one (2, 512, 512) case the flagship size (one
affine and one perspective record: the restatements need seconds there).  Only finite, modest
records reach the device; the NaN / Inf guard of the kernel is a matter of reading its code."""
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
SMALL = [(3, 37, 50), (3, 96, 160), (2, 64, 128)]
SHAPES = SMALL + [(2, 512, 512)]
BORDER = 9.0


def _load(name):
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(ROOT, "tests", "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load("augment_ref")


@pytest.fixture(scope="module")
def batch():
    """{shape: (image, mask)} as numpy uint8; drawn once, never modified"""
    return {s: R.random_batch(*s, seed=s[1]) for s in SHAPES}


def run(ua, image, mask, params, rng=None):
    """one launch on numpy inputs -> numpy outputs"""
    p = torch.as_tensor(params, dtype=torch.float32).to(DEV)
    r = ua.augment.pack_rng(rng).to(DEV) if rng is not None else None
    o, m = ua.ops.augment_u8(torch.from_numpy(image).to(DEV),
                             torch.from_numpy(mask).to(DEV) if mask is not None else None, p, r)
    torch.cuda.synchronize()
    return o.cpu().numpy(), (m.cpu().numpy() if m is not None else None)


def ident(ua, n):
    p = ua.augment.identity_params(n)
    p[:, 20] = BORDER
    return p


# ------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_identity_flip_shift_and_far_away(ua, batch, shape):
    N, H, W = shape
    image, mask = batch[shape]
    o, m = run(ua, image, mask, ident(ua, N))
    assert np.array_equal(o, image) and np.array_equal(m, mask)

    p = ident(ua, N)
    p[:, 0], p[:, 2] = -1.0, float(W)
    o, m = run(ua, image, mask, p)
    x, t = torch.from_numpy(image), torch.from_numpy(mask)
    assert torch.equal(torch.from_numpy(o), torch.flip(x, [2]))
    assert torch.equal(torch.from_numpy(m), torch.flip(t, [2]))

    # output (i, j) shows source (i - 2, j + 3)
    p = ident(ua, N)
    p[:, 2], p[:, 5] = 3.0, -2.0
    o, m = run(ua, image, mask, p)
    want = np.zeros_like(image)
    want[:, 2:, :W - 3] = image[:, :H - 2, 3:]
    wantm = np.full_like(mask, int(BORDER))
    wantm[:, 2:, :W - 3] = mask[:, :H - 2, 3:]
    assert np.array_equal(o, want) and np.array_equal(m, wantm)

    p = ident(ua, N)
    p[:, 2] = 10.0 * W
    o, m = run(ua, image, mask, p)
    assert (o == 0).all() and (m == int(BORDER)).all()


# ------------------------------------------------------------------------------------ geometry
def _geometry_records(ua, shape, kind):
    N, H, W = shape
    cfgs = R.record_configs(ua.augment)
    gen = torch.Generator().manual_seed(100 + H + (kind == "perspective"))
    if H == 512:        # the single flagship case: record 0 affine, record 1 perspective
        p, _ = ua.augment.sample_params([cfgs["affine"], cfgs["perspective"]], N, H, W, gen,
                                        which=[0, 1])
        return [p]
    return [ua.augment.sample_params(cfgs[kind], N, H, W, gen)[0] for _ in range(6 // N)]


GEOMETRY_CASES = [(s, k) for s in SMALL for k in ("affine", "perspective")] + \
    [((2, 512, 512), "affine+perspective")]


@pytest.mark.parametrize("shape,kind", GEOMETRY_CASES, ids=str)
def test_random_geometry_against_both_restatements(ua, batch, shape, kind):
    """Six random records per small shape and kind: the bytes of the fp32 restatement, the
    bounds against fp64."""
    image, mask = batch[shape]
    for p in _geometry_records(ua, shape, kind):
        ua.augment.validate_params(p, shape[1], shape[2])
        o, m = run(ua, image, mask, p)
        o32, m32 = R.augment_f32(image, mask, p.numpy())
        val, _, m64, near = R.augment_f64(image, mask, p.numpy())
        print(shape, kind, "differs from fp32 restatement:", int((o != o32).sum()),
              int((m != m32).sum()))
        fig = R.check_against_f64(o, m, val, m64, near)
        print(shape, kind, fig)
        assert np.array_equal(o, o32)
        assert np.array_equal(m, m32)
        assert (o != image).mean() > 0.5        # the record did something


# ------------------------------------------------------------------------------------ photometric
def _photometric_records(ua, H, W):
    rec = []
    for alpha, beta, gray, hole in ((1.3, (10.0, -20.0, 5.0), 0, None),
                                    (0.4, (-30.0, -30.0, -30.0), 0, None),
                                    (1.1, (3.5, 0.25, -7.75), 1, None),
                                    (1.0, (0.0, 0.0, 0.0), 0, (5, 3, W - 7, H - 11)),
                                    (0.77, (40.0, 1.5, -3.0), 1, (0, 0, 9, 4)),
                                    (1.25, (0.0, 0.0, 0.0), 0, (8, 8, 8, 20))):      # empty hole
        p = ident(ua, 1)[0]
        p[9] = alpha
        p[10:13] = torch.tensor(beta)
        p[13] = gray
        if hole is not None:
            p[15:19] = torch.tensor(hole, dtype=torch.float32)
            p[19], p[21] = 17.0, 2.0
        rec.append(p)
    return rec


@pytest.mark.parametrize("shape", SMALL, ids=str)
def test_photometric_stage_with_identity_geometry(ua, batch, shape):
    N, H, W = shape
    image, mask = batch[shape]
    rec = _photometric_records(ua, H, W)
    for k in range(0, len(rec), N):
        p = torch.stack([rec[(k + i) % len(rec)] for i in range(N)])
        o, m = run(ua, image, mask, p)
        o32, m32 = R.augment_f32(image, mask, p.numpy())
        val, o64, m64, _ = R.augment_f64(image, mask, p.numpy())
        print(shape, k, "differs from fp32:", int((o != o32).sum()), "max vs fp64:",
              int(np.abs(o.astype(int) - o64.astype(int)).max()))
        assert np.array_equal(o, o32) and np.array_equal(m, m32)
        assert np.abs(o.astype(int) - o64.astype(int)).max() <= 1
        assert np.array_equal(m, m64)
        assert (o != image).any()
    # the hole really is where the record puts it
    p = torch.stack([rec[3]] * N)
    o, m = run(ua, image, mask, p)
    assert (o[:, 3:H - 11, 5:W - 7] == 17).all() and (m[:, 3:H - 11, 5:W - 7] == 2).all()
    keep = np.ones((H, W), dtype=bool)
    keep[3:H - 11, 5:W - 7] = False
    assert np.array_equal(o[:, keep], image[:, keep]) and np.array_equal(m[:, keep], mask[:, keep])


# ------------------------------------------------------------------------------------ noise
def test_salt_and_pepper_positions_and_shares(ua):
    N, H, W = 3, 96, 160
    image = np.full((N, H, W, 3), 100, dtype=np.uint8)
    pp, ps = 0.10, 0.05
    rng = np.array([[11 + n, 0x9000_0000 + n, round(pp * 2 ** 32), round(ps * 2 ** 32)]
                    for n in range(N)], dtype=np.int64)
    rng[2, 3] = 0                               # salt_thr == 0: never
    o, _ = run(ua, image, None, ident(ua, N), rng)
    assert (o[..., 0] == o[..., 1]).all() and (o[..., 0] == o[..., 2]).all()
    for n in range(N):
        word = R.pixel_words(int(rng[n, 0]), int(rng[n, 1]), H, W, 1)[..., 0].astype(np.uint64)
        pepper = word < np.uint64(int(rng[n, 2]))
        salt = (word >= np.uint64(2 ** 32 - int(rng[n, 3]))) if rng[n, 3] else np.zeros_like(pepper)
        assert np.array_equal(o[n, ..., 0] == 0, pepper)
        assert np.array_equal(o[n, ..., 0] == 255, salt)
        assert np.array_equal(o[n, ..., 0] == 100, ~(pepper | salt))
        for got, prob in ((pepper.mean(), pp), (salt.mean(), ps if rng[n, 3] else 0.0)):
            sd = math.sqrt(prob * (1 - prob) / (H * W))
            print("share", got, "probability", prob, "sd", sd)
            assert abs(got - prob) <= 4 * sd
    o32, _ = R.augment_f32(image, None, ident(ua, N).numpy(), rng)
    assert np.array_equal(o, o32)


def test_gaussian_noise_against_fp64_box_muller(ua):
    N, H, W = 3, 96, 160
    image = np.full((N, H, W, 3), 128, dtype=np.uint8)
    p = ident(ua, N)
    p[:, 14] = 4.0
    rng = np.array([[5 + n, 77, 0, 0] for n in range(N)], dtype=np.int64)
    o, _ = run(ua, image, None, p, rng)
    val, o64, _, _ = R.augment_f64(image, None, p.numpy(), rng)
    d = np.abs(o.astype(int) - o64.astype(int))
    tie = np.abs(val - np.floor(val) - 0.5)
    print("differing", int((d > 0).sum()), "max", int(d.max()), "max tie distance of a differing pixel",
          float(tie[d > 0].max()) if (d > 0).any() else 0.0)
    assert d.max() <= 1
    assert ((d == 0) | (tie < 1e-2)).all()
    want = math.sqrt(4.0 ** 2 + 1.0 / 12.0)
    std = float(o.astype(np.float64).std())
    print("sample std", std, "expected", want)
    assert abs(std - want) <= 0.02 * want
    assert abs(float(o.mean()) - 128) < 0.1
    # the three channels and the samples draw different normals
    assert (o[..., 0] != o[..., 1]).mean() > 0.8 and (o[..., 0] != o[..., 2]).mean() > 0.8
    assert (o[0] != o[1]).mean() > 0.8


def _noisy_records(ua, shape, seed):
    N, H, W = shape
    cfg = ua.augment.AugmentConfig(**{
        **vars(R.record_configs(ua.augment)["perspective"]), "noise_group_prob": 1.0,
        "gauss_noise_prob": 1.0, "gauss_var_limit": (9.0, 16.0), "salt_pepper_prob": 1.0,
        "salt_p": (0.02, 0.05), "pepper_p": (0.02, 0.05)})
    return ua.augment.sample_params(cfg, N, H, W, torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("shape", [(3, 37, 50), (3, 96, 160)], ids=str)
def test_determinism_seed_and_batch_slot(ua, batch, shape):
    N, H, W = shape
    image, mask = batch[shape]
    p, r = _noisy_records(ua, shape, 7)
    a, am = run(ua, image, mask, p, r.numpy())
    b, bm = run(ua, image, mask, p, r.numpy())
    assert np.array_equal(a, b) and np.array_equal(am, bm)
    r2 = r.clone()
    r2[:, 0] += 1
    c, cm = run(ua, image, mask, p, r2.numpy())
    assert all((a[n] != c[n]).any() for n in range(N)) and np.array_equal(am, cm)
    # sample 0 moved to slot 2 with its record and seed: the same pixels
    perm = [1, 2, 0]
    d, dm = run(ua, image[perm], mask[perm], p[perm], r[perm].numpy())
    for slot, n in enumerate(perm):
        assert np.array_equal(d[slot], a[n]) and np.array_equal(dm[slot], am[n])


def test_without_a_mask_mask_out_is_untouched(ua, batch):
    shape = (3, 96, 160)
    N, H, W = shape
    image, _ = batch[shape]
    x = torch.from_numpy(image).to(DEV)
    p, _ = _noisy_records(ua, shape, 8)
    p = p.to(DEV)
    out = torch.empty_like(x)
    mask_out = torch.full((N, H, W), 77, dtype=torch.uint8, device=DEV)
    rc = ua.lib().unet_augment_u8(x.data_ptr(), None, out.data_ptr(), mask_out.data_ptr(),
                                  p.data_ptr(), None, N, H, W,
                                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    assert (mask_out == 77).all()
    o, m = ua.ops.augment_u8(x, None, p)
    assert m is None and torch.equal(o, out)


@pytest.mark.parametrize("shape", [(3, 37, 50), (2, 64, 128)], ids=str)
def test_rng_none_is_noise_off(ua, batch, shape):
    image, mask = batch[shape]
    p, r = _noisy_records(ua, shape, 9)
    assert (p[:, 14] > 0).all() and (r[:, 2:] > 0).all()
    a, am = run(ua, image, mask, p, None)
    q = p.clone()
    q[:, 14] = 0
    r0 = r.clone()
    r0[:, 2:] = 0
    b, bm = run(ua, image, mask, q, r0.numpy())
    assert np.array_equal(a, b) and np.array_equal(am, bm)
    c, _ = run(ua, image, mask, p, r.numpy())
    assert (a != c).any()


def test_captured_launch_follows_new_records(ua, batch):
    shape = (2, 64, 128)
    image, mask = batch[shape]
    x, t = torch.from_numpy(image).to(DEV), torch.from_numpy(mask).to(DEV)
    p1, r1 = _noisy_records(ua, shape, 10)
    p2, r2 = _noisy_records(ua, shape, 11)
    p = p1.to(DEV)
    r = ua.augment.pack_rng(r1).to(DEV)
    out = (torch.empty_like(x), torch.empty_like(t))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ua.ops.augment_u8(x, t, p, r, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ua.ops.augment_u8(x, t, p, r, out=out)
    p.copy_(p2)
    r.copy_(ua.augment.pack_rng(r2))
    graph.replay()
    torch.cuda.synchronize()
    got = (out[0].clone(), out[1].clone())
    want = ua.ops.augment_u8(x, t, p2.to(DEV), ua.augment.pack_rng(r2).to(DEV))
    first = ua.ops.augment_u8(x, t, p1.to(DEV), ua.augment.pack_rng(r1).to(DEV))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(got[0], first[0])


# ------------------------------------------------------------------------------------ end to end
E2E = (2, 64, 128)


def _e2e_config(ua):
    """geometry, colour, a hole, salt and pepper - everything the fp32 restatement holds bytewise"""
    return ua.augment.AugmentConfig(**{
        **vars(R.record_configs(ua.augment)["perspective"]), "mask_border_value": 0.0,
        "dropout_prob": 1.0, "dropout_height": (4, 12), "dropout_width": (4, 12),
        "color_prob": 1.0, "brightness_contrast_prob": 0.5, "brightness_limit": (-0.1, 0.1),
        "contrast_limit": (-0.3, 0.2), "rgb_shift_prob": 0.5, "rgb_shift_limit": (10.0, 10.0, 10.0),
        "salt_pepper_prob": 1.0, "salt_p": (0.0, 0.05), "pepper_p": (0.0, 0.05)})


def _e2e_batches(k):
    out = []
    for i in range(k):
        image, mask = R.random_batch(*E2E, seed=300 + i)
        out.append((torch.from_numpy(image).to(DEV), torch.from_numpy(mask).to(DEV)))
    return out


def _model(ua):
    model = ua.UNet()
    model.load_state_dict(O.fill_state_dict(23))
    model = model.to(DEV).train()
    model.matmul_precision = "bf16"
    model.dropout_mask_override = [m.to(DEV) if m is not None else None
                                   for m in O.draw_dropout_masks(5, E2E[0])]
    return model


def test_batch_augment_into_train_step_matches_the_restatement(ua):
    (x, m), = _e2e_batches(1)
    cfg = _e2e_config(ua)
    N, H, W = E2E
    # the records BatchAugment(seed=5) will draw
    p, r = ua.augment.sample_params(cfg, N, H, W, torch.Generator().manual_seed(5))
    x32, m32 = R.augment_f32(x.cpu().numpy(), m.cpu().numpy(), p.numpy(), r.numpy())
    res = []
    for restated in (False, True):
        model = _model(ua)
        opt = ua.create_optimizer(model)
        lossf = ua.SimpleLoss(target_layout="u8")
        if restated:
            xa, ma = torch.from_numpy(x32).to(DEV), torch.from_numpy(m32).to(DEV)
        else:
            xa, ma = ua.BatchAugment(cfg, seed=5)(x, m)
            assert xa.dtype == torch.uint8 and ma.dtype == torch.uint8
            assert xa.shape == x.shape and ma.shape == m.shape and not torch.equal(xa, x)
        loss = ua.train_step(model, opt, lossf, xa, ma, input_layout="nhwc_u8")
        res.append((loss.clone(), model.flat_parameters()[0].detach().clone()))
    assert torch.isfinite(res[0][0])
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_graphed_step_fed_through_out_matches_eager_twin(ua):
    batches = _e2e_batches(2)
    cfg = _e2e_config(ua)
    N, H, W = E2E
    gen = torch.Generator().manual_seed(6)
    records = [ua.augment.sample_params(cfg, N, H, W, gen) for _ in batches]

    twin = _model(ua)
    opt = ua.create_optimizer(twin)
    lossf = ua.SimpleLoss(target_layout="u8")
    aug = ua.BatchAugment(cfg, seed=0)
    eager = []
    for (x, m), rec in zip(batches, records):
        xa, ma = aug(x, m, params=rec)
        eager.append(ua.train_step(twin, opt, lossf, xa, ma, input_layout="nhwc_u8").clone())
    p_eager = twin.flat_parameters()[0].detach().clone()

    model = _model(ua)
    opt = ua.create_optimizer(model)
    step = ua.GraphedTrainStep(model, opt, ua.SimpleLoss(target_layout="u8"), *batches[0],
                               input_layout="nhwc_u8")
    aug = ua.BatchAugment(cfg, seed=0)
    graphed = []
    for (x, m), rec in zip(batches, records):
        xa, ma = aug(x, m, out=(step.images, step.masks), params=rec)
        assert xa.data_ptr() == step.images.data_ptr() and ma.data_ptr() == step.masks.data_ptr()
        graphed.append(step(xa, ma).clone())
    torch.cuda.synchronize()
    for a, b in zip(graphed, eager):
        assert torch.equal(a, b)
    assert torch.equal(model.flat_parameters()[0].detach(), p_eager)
    assert float(eager[0]) != float(eager[1])


def test_train_one_epoch_with_augment(ua):
    batches = _e2e_batches(2)
    loader = [{"image": x, "mask": m} for x, m in batches]
    cfg = _e2e_config(ua)
    res = []
    for augment in (None, ua.BatchAugment(cfg, seed=1), ua.BatchAugment(cfg, seed=1)):
        model = _model(ua)
        opt = ua.create_optimizer(model)
        res.append(ua.train_one_epoch(model, loader, opt, ua.SimpleLoss(target_layout="u8"), DEV,
                                      augment=augment, input_layout="nhwc_u8"))
    assert all(math.isfinite(v) for v in res)
    assert res[1] == res[2] and res[0] != res[1]
    # per-sample configuration through the batch's "which" entry
    model = _model(ua)
    loader = [{"image": x, "mask": m, "which": torch.tensor([0, 1])} for x, m in batches]
    both = ua.BatchAugment([ua.AugmentConfig(), cfg], seed=1)
    v = ua.train_one_epoch(model, loader, ua.create_optimizer(model),
                           ua.SimpleLoss(target_layout="u8"), DEV, augment=both,
                           input_layout="nhwc_u8")
    assert math.isfinite(v) and v not in (res[0], res[1])


def test_bench_tool_feeds_a_batch_through_the_staged_record():
    """part 3 of tools/bench_augment.py (copies, plus drawing and staging the records, plus the
    kernel) runs in a child process: the one caller of `BatchAugment._stage` outside the package"""
    import json
    import subprocess
    import sys
    proc = subprocess.run(
        [sys.executable, os.path.join(ROOT, "tools", "bench_augment.py"), "--parts", "feed",
         "--batch", "2", "--hw", "64", "--warmup", "1", "--rounds", "1", "--steps", "2"],
        capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    res = json.loads(proc.stdout.strip().splitlines()[-1])
    assert "kernel" not in res and not res["step_ms"]
    assert sorted(res["feed_us"]) == ["copy", "copy+records", "copy+records+kernel"]
    for form, v in res["feed_us"].items():
        assert math.isfinite(v["median_us"]) and v["median_us"] > 0, form
