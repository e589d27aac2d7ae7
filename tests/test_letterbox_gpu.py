"""GPU (-m gpu): unet_letterbox_u8 / unet_byte_histogram_u8 and `ua.dataprep` on the device, byte
for byte against the numpy restatement of tests/tools/resize_ref.py (which test_letterbox_cpu.py
holds against F.interpolate and the hand cases)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)


def _load(name):
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(ROOT, "tests", "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load("resize_ref")
RAGGED = [(h, w) for h, w, _ in R.SHAPES]


@pytest.fixture(scope="module")
def samples():
    return R.make_samples(RAGGED, seed=11)


@pytest.fixture(scope="module")
def real():
    return R.make_samples([(500, 375)], seed=12)


def _collate(ua, data, **extra):
    items = []
    for k, (img, msk) in enumerate(data):
        item = {"image": img, "mask": msk}
        item.update({key: val[k] for key, val in extra.items()})
        items.append(item)
    return ua.dataprep.ragged_collate(items)


def _pack(data, start=0, gap=0):
    """A byte arena with NO alignment between the samples (offsets as they fall, odd included)."""
    rows, chunks, off = [], [np.zeros(start, dtype=np.uint8)], start
    for img, msk in data:
        h, w = img.shape[:2]
        rows.append([off, off + img.size + gap, h, w])
        chunks += [img.reshape(-1), np.zeros(gap, dtype=np.uint8), msk.reshape(-1)]
        off += img.size + gap + msk.size
    return np.concatenate(chunks), rows


def test_one_ragged_call_with_each_sample_at_its_own_size(ua, samples):
    """All seven samples in one launch into 48 x 48 tiles, each record carrying the letterbox of
    its own target size (32, 48 or 16): both orientations, both area cases, an enlargement, a
    single source row; packed without alignment, so most offsets are odd."""
    arena, rows = _pack(samples, start=1)
    assert sum(r[0] % 2 for r in rows) >= 2 and sum(r[1] % 2 for r in rows) >= 2
    table, want_i, want_m = [], [], []
    for (h, w, S), row, (img, msk) in zip(R.SHAPES, rows, samples):
        oh, ow, py, px = R.letterbox_geometry(h, w, S)
        table.append(row + [oh, ow, py, px])
        want_i.append(R.place(R.resize_linear(img, oh, ow), (48, 48), py, px))
        want_m.append(R.place(R.resize_nearest(msk, oh, ow), (48, 48), py, px))
    assert [R.is_area_case(r[2], r[3], r[4], r[5]) for r in table] == \
        [False, False, True, True, False, False, False]
    d_arena = torch.from_numpy(arena).to(DEV)
    d_table = torch.tensor(table, dtype=torch.int64, device=DEV)
    images, masks = ua.ops.letterbox_u8(d_arena, d_table, 48)
    assert np.array_equal(images.cpu().numpy(), np.stack(want_i))
    assert np.array_equal(masks.cpu().numpy(), np.stack(want_m))
    # mask_out = NULL: the same images, no mask
    only, none = ua.ops.letterbox_u8(d_arena, d_table, 48, want_mask=False)
    assert none is None and torch.equal(only, images)
    # with a table per sample
    luts = np.stack([np.random.default_rng(b).integers(0, 256, 256).astype(np.uint8)
                     for b in range(len(samples))])
    _, mapped = ua.ops.letterbox_u8(d_arena, d_table, 48, lut=torch.from_numpy(luts).to(DEV))
    want = [R.place(luts[b][R.resize_nearest(msk, t[4], t[5])], (48, 48), t[6], t[7])
            for b, ((_, msk), t) in enumerate(zip(samples, table))]
    assert np.array_equal(mapped.cpu().numpy(), np.stack(want))


@pytest.mark.parametrize("size,mode", [(32, "letterbox"), ((32, 24), "stretch"),
                                       (31, "letterbox"), ((18, 30), "stretch")])
def test_device_letterbox_equals_the_restatement(ua, samples, size, mode):
    """Through ragged_collate and DeviceLetterbox: letterbox to 32, stretch to the non-square
    32 x 24; 31 and 18 x 30 take the narrower store paths (S_w % 16 != 0, S_w % 4 != 0)."""
    loader = [_collate(ua, samples, which=list(range(len(samples))))]
    batch, = list(ua.dataprep.DeviceLetterbox(loader, size=size, mode=mode, device=DEV))
    hw = (size, size) if isinstance(size, int) else size
    want_i, want_m = R.letterbox_batch(samples, hw, mode)
    assert batch["image"].dtype == torch.uint8 and batch["image"].is_cuda
    assert tuple(batch["image"].shape) == (len(samples),) + hw + (3,)
    assert np.array_equal(batch["image"].cpu().numpy(), want_i)
    assert np.array_equal(batch["mask"].cpu().numpy(), want_m)
    assert batch["original_dims"].tolist() == [list(s) for s in RAGGED]
    assert batch["which"].tolist() == list(range(len(samples)))
    assert "arena" not in batch and "table" not in batch


@pytest.mark.parametrize("mode", ["letterbox", "stretch"])
def test_real_sizes_with_the_clip_image(ua, real, mode):
    """500 x 375 to 512 and to 224 (several row bands and many chunks per row)."""
    loader = [_collate(ua, real)]
    batch, = list(ua.dataprep.DeviceLetterbox(loader, size=512, mode=mode, clip_size=224,
                                              device=DEV))
    want_i, want_m = R.letterbox_batch(real, (512, 512), mode)
    want_c, _ = R.letterbox_batch(real, (224, 224), mode)
    assert np.array_equal(batch["image"].cpu().numpy(), want_i)
    assert np.array_equal(batch["mask"].cpu().numpy(), want_m)
    assert tuple(batch["clip_image"].shape) == (1, 224, 224, 3)
    assert np.array_equal(batch["clip_image"].cpu().numpy(), want_c)
    if mode == "letterbox":
        assert (want_i[0][:, :64] == 0).all() and (want_i[0][:, 64:448] > 0).any()


def test_masks_with_and_without_a_fixed_lut(ua, samples):
    assert set(np.unique(np.concatenate([m.ravel() for _, m in samples]))) == {0, 1, 2, 255}
    lut = np.arange(256, dtype=np.uint8)
    lut[[1, 2, 255]] = [2, 1, 0]
    loader = [_collate(ua, samples)]
    plain, = list(ua.dataprep.DeviceLetterbox(loader, size=32, device=DEV))
    mapped, = list(ua.dataprep.DeviceLetterbox(loader, size=32, label_lut=lut, device=DEV))
    _, want_plain = R.letterbox_batch(samples, (32, 32))
    _, want_mapped = R.letterbox_batch(samples, (32, 32), luts=[lut] * len(samples))
    assert np.array_equal(plain["mask"].cpu().numpy(), want_plain)
    assert np.array_equal(mapped["mask"].cpu().numpy(), want_mapped)
    assert not np.array_equal(want_plain, want_mapped)
    assert torch.equal(plain["image"], mapped["image"])


def test_bad_records_give_zero_tiles_and_leave_their_neighbours_alone(ua, samples):
    data = samples[:2]
    arena, rows = _pack(data, start=3)
    good = [rows[b] + list(R.letterbox_geometry(*RAGGED[b], 32)) for b in range(2)]
    g = good[0]
    bad = [
        [g[0], g[1], 0, g[3]] + g[4:],                    # h = 0
        [g[0], g[1], g[2], 16385] + g[4:],                # w too large
        g[:4] + [33, g[5], 0, g[7]],                      # out_h > S
        g[:4] + [0, g[5], g[6], g[7]],                    # out_h = 0
        g[:6] + [g[6] + 6, g[7]],                         # pad_y + out_h > S
        g[:6] + [g[6], -1],                               # negative pad
        [arena.size - 10, g[1]] + g[2:],                  # the image leaves the arena
        [-5, g[1]] + g[2:],                               # negative image offset
    ]
    table = [good[0]] + bad + [good[1]]
    images, masks = ua.ops.letterbox_u8(torch.from_numpy(arena).to(DEV),
                                        torch.tensor(table, dtype=torch.int64, device=DEV), 32)
    want_i, want_m = R.letterbox_batch(data, (32, 32))
    images, masks = images.cpu().numpy(), masks.cpu().numpy()
    assert np.array_equal(images[0], want_i[0]) and np.array_equal(masks[0], want_m[0])
    assert np.array_equal(images[-1], want_i[1]) and np.array_equal(masks[-1], want_m[1])
    assert want_i[0].any() and want_m[0].any()
    for b in range(1, 1 + len(bad)):
        assert not images[b].any(), b
        assert not masks[b].any(), b
    # a mask that leaves the arena, or a sample without one: zero mask tile, the image is served
    table = [g[:1] + [arena.size - 5] + g[2:], g[:1] + [-1] + g[2:]]
    images, masks = ua.ops.letterbox_u8(torch.from_numpy(arena).to(DEV),
                                        torch.tensor(table, dtype=torch.int64, device=DEV), 32)
    assert np.array_equal(images.cpu().numpy(), np.stack([want_i[0]] * 2))
    assert not masks.cpu().numpy().any()
    hist = ua.ops.byte_histogram_u8(torch.from_numpy(arena).to(DEV),
                                    torch.tensor(table + [bad[0], good[1]], dtype=torch.int64,
                                                 device=DEV)).cpu().numpy()
    assert not hist[:3].any()
    assert np.array_equal(hist[3].astype(np.uint64), R.histogram(data[1][1]))


def test_byte_histogram(ua, samples, real):
    data = samples + real
    for start in (0, 5):                                   # aligned and odd mask offsets
        arena, rows = _pack(data, start=start)
        table = [r + [1, 1, 0, 0] for r in rows]
        hist = ua.ops.byte_histogram_u8(torch.from_numpy(arena).to(DEV),
                                        torch.tensor(table, dtype=torch.int64, device=DEV))
        assert hist.dtype == torch.int64 and tuple(hist.shape) == (len(data), 256)
        want = np.stack([R.histogram(m) for _, m in data]).astype(np.int64)
        assert np.array_equal(hist.cpu().numpy(), want)
    rng = np.random.default_rng(5)
    batch = rng.integers(0, 256, size=(3, 33, 37), dtype=np.uint8)
    batch[1] = rng.choice(np.array([0, 1, 2, 255], dtype=np.uint8), size=(33, 37))
    hist = ua.ops.byte_histogram_u8(torch.from_numpy(batch).to(DEV)).cpu().numpy()
    want = np.stack([np.bincount(m.ravel(), minlength=256) for m in batch])
    assert np.array_equal(hist, want)


def test_trimap_labels_end_to_end(ua):
    """label_lut="trimap": histogram, device-built tables and the gather, against the host table
    of each mask's value set."""
    shapes = [(37, 53), (53, 37), (20, 31), (64, 48), (30, 41)]
    value_sets = [(0, 128, 255), (0, 1, 255), (0, 255), (0, 3, 7, 255), (0, 5, 128, 255)]
    is_cat = [True, False, True, False, False]
    data = [R.make_samples([s], seed=40 + k, mask_values=v)[0]
            for k, (s, v) in enumerate(zip(shapes, value_sets))]
    luts = []
    for (_, msk), values, cat in zip(data, value_sets, is_cat):
        assert set(np.unique(msk)) == set(values)
        luts.append(R.trimap_lut(np.unique(msk), cat))
    loader = [_collate(ua, data, is_cat=is_cat)]
    batch, = list(ua.dataprep.DeviceLetterbox(loader, size=32, label_lut="trimap", device=DEV))
    want_i, want_m = R.letterbox_batch(data, (32, 32), luts=luts)
    assert np.array_equal(batch["mask"].cpu().numpy(), want_m)
    assert np.array_equal(batch["image"].cpu().numpy(), want_i)
    assert set(np.unique(want_m)) == {0, 1, 2, 255}
    assert batch["is_cat"].tolist() == is_cat


def _model(ua, train, n):
    from oracle import unet_ref as O
    model = ua.UNet()
    model.load_state_dict(O.fill_state_dict(23))
    model = model.to(DEV)
    model.train(train)
    if train:
        model.dropout_mask_override = [m.to(DEV) if m is not None else None
                                       for m in O.draw_dropout_masks(5, n)]
    return model


def test_training_and_evaluation_on_a_device_letterbox_loader(ua):
    """64 x 64 network size, three ragged samples: one train_one_epoch step (uint8 images, uint8
    targets) and evaluate_model give the loss and the confusion matrix, bit for bit, of the same
    calls fed the batch the restatement produced on the host."""
    shapes = [(90, 61), (47, 100), (128, 128)]
    data = R.make_samples(shapes, seed=60, mask_values=(0, 1, 2, 255))
    host_i, host_m = R.letterbox_batch(data, (64, 64))
    dims = torch.tensor(shapes, dtype=torch.int64)
    ragged = [_collate(ua, data)]

    losses = []
    for device_side in (True, False):
        loader = ua.dataprep.DeviceLetterbox(ragged, size=64, device=DEV) if device_side else \
            [{"image": torch.from_numpy(host_i), "mask": torch.from_numpy(host_m)}]
        model = _model(ua, True, len(shapes))
        loss = ua.train_one_epoch(model, loader, ua.create_optimizer(model),
                                  ua.SimpleLoss(target_layout="u8"), DEV, input_layout="nhwc_u8")
        losses.append((loss, model.flat_parameters()[0].detach().clone()))
    assert np.isfinite(losses[0][0]) and losses[0][0] == losses[1][0]
    assert torch.equal(losses[0][1], losses[1][1])

    # evaluate_model calls model(images) without a layout: the wrapper hands it the normalised
    # NCHW view (image_format="nchw_f32"), the host twin gets ops.preprocess_u8 of the host batch
    model = _model(ua, False, len(shapes))
    loader = ua.dataprep.DeviceLetterbox(ragged, size=64, device=DEV, image_format="nchw_f32")
    got = ua.evaluate.evaluate_model(model, loader, DEV)
    x = ua.ops.preprocess_u8(torch.from_numpy(host_i).to(DEV))[0].permute(0, 3, 1, 2)
    want = ua.evaluate.evaluate_model(
        model, [{"image": x, "mask": torch.from_numpy(host_m), "original_dims": dims}], DEV)
    assert np.array_equal(got["confusion_matrix"], want["confusion_matrix"])
    assert got["confusion_matrix"].sum() > 0
    assert {k: v for k, v in got.items() if k != "confusion_matrix"} == \
        {k: v for k, v in want.items() if k != "confusion_matrix"}
    val = [ua.validate(model, ld, ua.SimpleLoss(target_layout="u8"), DEV, input_layout="nhwc_u8")
           for ld in (ua.dataprep.DeviceLetterbox(ragged, size=64, device=DEV),
                      [{"image": torch.from_numpy(host_i), "mask": torch.from_numpy(host_m)}])]
    assert val[0] == val[1]


def test_float_image_format_and_autoencoder_target(ua, samples):
    """image_format="nchw_f32" is ops.preprocess_u8 of the uint8 tile; target="image" hands the
    uint8 tile itself on (the ua.ae loops read "image" and "target")."""
    items = [{"image": img} for img, _ in samples]                       # no masks at all
    loader = [ua.dataprep.ragged_collate(items)]
    batch, = list(ua.dataprep.DeviceLetterbox(loader, size=32, device=DEV, image_format="nchw_f32",
                                              mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0),
                                              target="image"))
    want_i, _ = R.letterbox_batch(samples, (32, 32))
    assert "mask" not in batch
    assert batch["target"].dtype == torch.uint8
    assert np.array_equal(batch["target"].cpu().numpy(), want_i)
    x = batch["image"]
    assert x.dtype == torch.float32 and tuple(x.shape) == (len(samples), 3, 32, 32)
    want = ua.ops.preprocess_u8(torch.from_numpy(want_i).to(DEV), None, (0.0, 0.0, 0.0),
                                (1.0, 1.0, 1.0))[0].permute(0, 3, 1, 2)
    assert torch.equal(x, want)
    # one fp32 division per value: within an ulp of v / 255
    exact = torch.from_numpy(want_i).permute(0, 3, 1, 2).double() / 255.0
    assert (x.cpu().double() - exact).abs().max() <= 2.0 ** -24


def test_static_class_weights_on_the_device(ua):
    shapes = [(90, 61), (47, 100), (128, 128), (64, 64)]
    data = R.make_samples(shapes, seed=61, mask_values=(0, 0, 0, 1, 2, 255))
    ragged = [_collate(ua, data[:3]), _collate(ua, data[3:])]
    got = ua.dataprep.static_class_weights(ua.dataprep.DeviceLetterbox(ragged, size=64, device=DEV))
    # the scan of src/train.py main over the host batches
    class_pixels, total = torch.zeros(3), torch.zeros(())
    for part in (data[:3], data[3:]):
        masks = torch.from_numpy(R.letterbox_batch(part, (64, 64))[1]).long()
        valid = masks != 255
        valid_masks = masks * valid.long()
        for c in range(3):
            class_pixels[c] += torch.sum((valid_masks == c) & valid).float()
        total += torch.sum(valid).float()
    want = total / torch.clamp(class_pixels, min=1.0)
    want = want * (3 / want.sum())
    assert got.is_cuda and got.dtype == torch.float32 and torch.equal(got.cpu(), want)
    loss = ua.SimpleLoss(class_weights=got, dynamic_weights=False, target_layout="u8")
    logits = torch.randn(1, 3, 64, 64, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
    masks = torch.from_numpy(R.letterbox_batch(data[:1], (64, 64))[1]).to(DEV)
    assert torch.isfinite(loss(logits, masks))
