"""CPU (-m "not gpu"): the letterbox / resize stage without a device - the numpy restatement of
tests/tools/resize_ref.py against what exists here (F.interpolate in float64 for the linear path,
its nearest mode index for index, hand cases), the host side of `ua.dataprep` (geometry, label
table, breed rule, class-weight arithmetic, the ragged collate) and the argument checks of the two
new entry points.  OpenCV is not installed where this project is built, so no fixture is recorded
from it: parity with cv2 itself is not pinned here."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "unet_hip.h")


def _load(name):
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(ROOT, "tests", "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load("resize_ref")
ENTRY_POINTS = ("unet_letterbox_u8", "unet_byte_histogram_u8")

# (h, w, out_h, out_w): every sample at its letterbox size and stretched to 32 x 24
RESIZES = [(h, w) + R.letterbox_geometry(h, w, S)[:2] for h, w, S in R.SHAPES + R.REAL] + \
          [(h, w) + R.STRETCH for h, w, _ in R.SHAPES]


def _exact_bilinear(img, out_h, out_w):
    x = torch.from_numpy(img).permute(2, 0, 1)[None].double()
    y = F.interpolate(x, size=(out_h, out_w), mode="bilinear", align_corners=False)
    return y[0].permute(1, 2, 0).numpy()


# ---- the restatement against what exists here ----------------------------------------------------
@pytest.mark.parametrize("h,w,out_h,out_w", RESIZES)
def test_linear_is_within_one_level_of_float64_bilinear(h, w, out_h, out_w):
    """Same half-pixel sampling as F.interpolate(bilinear, align_corners=False); the fixed-point
    form (11-bit weights, two truncating shifts, one rounding) stays strictly less than one level
    from the exact value: 0.785 at worst over these shapes, exactly 0.5 on the area path (which is
    the exact 2 x 2 mean rounded half up).  A wrong coefficient or shift breaks the bound."""
    (img, _), = R.make_samples([(h, w)], seed=1000 + h * 64 + w)
    got = R.resize_linear(img, out_h, out_w)
    assert got.shape == (out_h, out_w, 3) and got.dtype == np.uint8
    err = np.abs(got.astype(np.float64) - _exact_bilinear(img, out_h, out_w)).max()
    print(f"{h}x{w} -> {out_h}x{out_w}: max |fixed - exact| = {err:.4f}")
    assert err < 1.0
    if R.is_area_case(h, w, out_h, out_w):
        assert err <= 0.5


@pytest.mark.parametrize("h,w,out_h,out_w", RESIZES)
def test_nearest_reads_the_index_interpolate_reads(ua, h, w, out_h, out_w):
    from unet_implementations_amd.train import nearest_source_index
    for src, dst in ((h, out_h), (w, out_w)):
        ramp = torch.arange(src, dtype=torch.float32).view(1, 1, src)
        want = F.interpolate(ramp, size=dst, mode="nearest")[0, 0].long().numpy()
        # ATen's rule is in fp32, the restated one in fp64: they agree on these sizes, which is
        # what makes the comparison a fair one
        assert np.array_equal(nearest_source_index(src, dst), want)
        assert np.array_equal(R.nearest_index(src, dst), want), (src, dst)
    (_, msk), = R.make_samples([(h, w)], seed=7)
    t = torch.from_numpy(msk)[None, None].float()
    want = F.interpolate(t, size=(out_h, out_w), mode="nearest")[0, 0].numpy().astype(np.uint8)
    assert np.array_equal(R.resize_nearest(msk, out_h, out_w), want)


def test_hand_cases():
    (img, msk), = R.make_samples([(13, 17)], seed=3)
    assert np.array_equal(R.resize_linear(img, 13, 17), img)              # same size: identity
    assert np.array_equal(R.resize_nearest(msk, 13, 17), msk)
    for value in (0, 1, 127, 200, 255):                                   # constants stay constant
        const = np.full((9, 14, 3), value, dtype=np.uint8)
        for out in ((9, 14), (5, 31), (20, 3), (1, 1), (18, 28), (4, 7)):
            assert (R.resize_linear(const, *out) == value).all(), (value, out)
    (big, _), = R.make_samples([(12, 10)], seed=4)                        # exact halving
    v = big.astype(np.int32)
    want = (v[0::2, 0::2] + v[0::2, 1::2] + v[1::2, 0::2] + v[1::2, 1::2] + 2) >> 2
    assert np.array_equal(R.resize_linear(big, 6, 5), want.astype(np.uint8))
    assert not R.is_area_case(12, 10, 6, 4) and not R.is_area_case(1024, 683, 512, 341)
    (row, _), = R.make_samples([(1, 9)], seed=5)                          # one source row
    out = R.resize_linear(row, 4, 16)
    assert (out == out[:1]).all()
    y0, y1, b0, b1 = R.linear_taps(1, 4)
    assert (y0 == 0).all() and (y1 == 0).all() and (b0 == 2048).all() and (b1 == 0).all()
    x0, x1, a0, a1 = R.linear_taps(9, 16)
    assert ((a0 + a1) == 2048).all() and x0.min() == 0 and x1.max() == 8
    assert a1[0] == 0 and a1[-1] == 0                                     # both ends clamp


def test_padding_is_zero_and_the_tile_is_centred():
    samples = R.make_samples([(37, 53), (53, 37), (7, 5)], seed=6, mask_values=(1, 2, 255))
    for s in samples:
        s[0][...] = np.maximum(s[0], 1)                                   # no zero inside
    images, masks = R.letterbox_batch(samples, (32, 32))
    for b, (img, _) in enumerate(samples):
        oh, ow, py, px = R.letterbox_geometry(*img.shape[:2], 32)
        assert py == (32 - oh) // 2 and px == (32 - ow) // 2
        inside = np.zeros((32, 32), dtype=bool)
        inside[py:py + oh, px:px + ow] = True
        assert (images[b][~inside] == 0).all() and (masks[b][~inside] == 0).all()
        assert (images[b][inside] > 0).all() and (masks[b][inside] > 0).all()
    assert R.letterbox_geometry(37, 53, 32) == (22, 32, 5, 0)
    assert R.letterbox_geometry(53, 37, 32) == (32, 22, 0, 5)


# ---- ua.dataprep, host side ----------------------------------------------------------------------
def test_letterbox_geometry(ua):
    D = ua.dataprep
    assert D.letterbox_geometry(500, 375, 512) == (512, 384, 0, 64)
    assert D.letterbox_geometry(375, 500, 512) == (384, 512, 64, 0)
    assert D.letterbox_geometry(1024, 683, 512) == (512, 341, 0, 85)      # not the area case
    assert D.letterbox_geometry(500, 375, 224) == (224, 168, 0, 28)
    assert D.letterbox_geometry(64, 64, 32) == (32, 32, 0, 0)
    for h, w, S in R.SHAPES + R.REAL:
        assert D.letterbox_geometry(h, w, S) == R.letterbox_geometry(h, w, S)
    assert D.letterbox_geometry(1, 9, 16) == (1, 16, 7, 0)
    with pytest.raises(ValueError):
        D.letterbox_geometry(1, 100, 16)                                  # a side becomes 0
    assert D.stretch_geometry(37, 53, (32, 24)) == (32, 24, 0, 0)
    assert D.stretch_geometry(37, 53, 512) == (512, 512, 0, 0)


@pytest.mark.parametrize("is_cat", [True, False])
def test_trimap_lut(ua, is_cat):
    cls = 1 if is_cat else 2
    cases = [({0, 128, 255}, 128), ({0, 1, 255}, 1), ({0, 255}, None), ({0, 3, 7, 255}, 3)]
    for present, fg in cases:
        lut = ua.dataprep.trimap_lut(present, is_cat)
        assert lut.dtype == np.uint8 and lut.shape == (256,)
        want = np.zeros(256, dtype=np.uint8)
        want[255] = 255
        if fg is not None:
            want[fg] = cls
        assert np.array_equal(lut, want), present
        assert np.array_equal(R.trimap_lut(present, is_cat), want)
    # 128 wins over a smaller foreground candidate
    assert ua.dataprep.trimap_lut({0, 5, 128, 255}, is_cat)[[5, 128]].tolist() == [0, cls]


def test_device_lut_builder_matches_the_host_rule_on_cpu_tensors(ua):
    """The torch expression DeviceLetterbox runs on the device, evaluated here on host tensors."""
    sets = [{0, 128, 255}, {0, 1, 255}, {0, 255}, {0, 3, 7, 255}, {255}, {0}, {128}, {9}]
    hist = torch.zeros((2 * len(sets), 256), dtype=torch.int64)
    is_cat = torch.zeros(2 * len(sets), dtype=torch.bool)
    want = []
    for i, present in enumerate(sets + sets):
        hist[i, list(present)] = 5 + i
        is_cat[i] = i < len(sets)
        want.append(ua.dataprep.trimap_lut(present, bool(is_cat[i])))
    got = ua.dataprep._device_trimap_luts(hist, is_cat)
    assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), np.stack(want))


def test_is_cat_image(ua):
    f = ua.dataprep.is_cat_image
    for name in ("Abyssinian_12", "british_shorthair_3.jpg", "Maine_Coon_7", "Egyptian_Mau_1",
                 "Russian_Blue_99", "sphynx_4", "Bengal_1", "Birman_2", "Bombay_3", "Persian_4",
                 "Ragdoll_5", "Siamese_6"):
        assert f(name), name
    for name in ("beagle_1", "american_bulldog_4", "yorkshire_terrier_9", "pug_2", "samoyed_1"):
        assert not f(name), name


def test_static_class_weight_arithmetic(ua):
    counts = np.zeros(256, dtype=np.int64)
    counts[[0, 1, 2, 255]] = [700, 200, 100, 50]
    w = ua.dataprep.class_weights_from_counts(counts)
    raw = np.array([1000 / 700, 1000 / 200, 1000 / 100])
    assert w.dtype == torch.float32 and np.allclose(w.numpy(), raw * 3 / raw.sum(), rtol=1e-6)
    assert abs(float(w.sum()) - 3.0) < 1e-5
    counts[2] = 0                                                          # an absent class: clamp
    w = ua.dataprep.class_weights_from_counts(counts)
    raw = np.array([900 / 700, 900 / 200, 900 / 1])
    assert np.allclose(w.numpy(), raw * 3 / raw.sum(), rtol=1e-6)
    # against the scan as src/train.py main writes it, on a mask batch
    rng = np.random.default_rng(0)
    masks = torch.from_numpy(rng.choice(np.array([0, 1, 2, 255], dtype=np.uint8), size=(3, 33, 37),
                                        p=[0.6, 0.2, 0.15, 0.05])).long()
    class_pixels, total = torch.zeros(3), 0
    valid = masks != 255
    valid_masks = masks * valid.long()
    for c in range(3):
        class_pixels[c] += torch.sum((valid_masks == c) & valid).float()
    total += torch.sum(valid).float()
    want = total / torch.clamp(class_pixels, min=1.0)
    want = want * (3 / want.sum())
    hist = np.stack([R.histogram(m.numpy().astype(np.uint8)) for m in masks]).astype(np.int64)
    assert torch.equal(ua.dataprep.class_weights_from_counts(hist), want)


def test_ragged_collate(ua):
    shapes = [(37, 53), (7, 5), (1, 9)]
    data = R.make_samples(shapes, seed=8)
    samples = [{"image": torch.from_numpy(i) if k == 1 else i, "mask": m, "which": k,
                "is_cat": k == 0} for k, (i, m) in enumerate(data)]
    batch = ua.dataprep.ragged_collate(samples)
    arena, table = batch["arena"], batch["table"]
    assert arena.dtype == torch.uint8 and arena.dim() == 1
    assert table.dtype == torch.int64 and tuple(table.shape) == (3, 4)
    assert batch["original_dims"].dtype == torch.int64
    assert batch["original_dims"].tolist() == [list(s) for s in shapes]
    assert batch["which"].tolist() == [0, 1, 2] and batch["is_cat"].tolist() == [True, False, False]
    end = 0
    flat = arena.numpy()
    for (io, mo, h, w), (img, msk) in zip(table.tolist(), data):
        assert io % 16 == 0 and mo % 16 == 0 and io >= end and mo >= io + h * w * 3
        assert np.array_equal(flat[io:io + h * w * 3].reshape(h, w, 3), img)
        assert np.array_equal(flat[mo:mo + h * w].reshape(h, w), msk)
        end = mo + h * w
    assert end <= arena.numel() < end + 16
    # without masks: offset -1, and the full table of a stretch / a letterbox
    batch = ua.dataprep.ragged_collate([{"image": i} for i, _ in data])
    assert batch["table"][:, 1].tolist() == [-1, -1, -1] and "mask" not in batch
    full = ua.dataprep.full_table(batch["table"], 16, "letterbox")
    assert tuple(full.shape) == (3, 8)
    assert full[:, 4:].tolist() == [list(R.letterbox_geometry(h, w, 16)) for h, w in shapes]
    full = ua.dataprep.full_table(batch["table"], (32, 24), "stretch")
    assert full[:, 4:].tolist() == [[32, 24, 0, 0]] * 3
    with pytest.raises(TypeError):
        ua.dataprep.ragged_collate([{"image": np.zeros((4, 4, 3), dtype=np.float32)}])
    with pytest.raises(ValueError):
        ua.dataprep.ragged_collate([{"image": np.zeros((4, 4, 3), dtype=np.uint8),
                                     "mask": np.zeros((4, 5), dtype=np.uint8)}])


# ---- the ABI surface -----------------------------------------------------------------------------
def test_entry_points_declared_exported_and_bound(ua):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    handle = ctypes.CDLL(ua.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), f"{name} not declared in unet_hip.h"
        assert hasattr(handle, name), f"{name} not exported"
        assert name in ua._lib.SIGNATURES
    assert len(ua._lib.SIGNATURES["unet_letterbox_u8"][1]) == 10
    assert len(ua._lib.SIGNATURES["unet_byte_histogram_u8"][1]) == 6
    assert re.search(r"#define\s+UNET_LETTERBOX_FIELDS\s+8\b", text)
    assert ua.ops.LETTERBOX_FIELDS == 8
    for name in ("letterbox_u8", "byte_histogram_u8"):
        assert callable(getattr(ua.ops, name))
    for name in ("letterbox_geometry", "stretch_geometry", "ragged_collate", "DeviceLetterbox",
                 "trimap_lut", "is_cat_image", "static_class_weights"):
        assert callable(getattr(ua.dataprep, name))
    header = int(re.search(r"#define\s+UNET_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert header == ua._lib.ABI_VERSION == ua.lib().unet_abi_version()


def test_host_arguments_are_rejected_before_any_launch(ua):
    lib = ua.lib()
    ok = dict(arena=1, nbytes=64, table=1, B=1, S_h=8, S_w=8, image=1, mask=1, lut=None)

    def letterbox(**kw):
        a = dict(ok, **kw)
        return lib.unet_letterbox_u8(a["arena"], a["nbytes"], a["table"], a["B"], a["S_h"],
                                     a["S_w"], a["image"], a["mask"], a["lut"], None)

    for name in ("arena", "table", "image"):
        assert letterbox(**{name: None}) == -1 and b"null" in lib.unet_last_error()
    assert letterbox(mask=None, lut=1) == -1 and b"lut" in lib.unet_last_error()
    for bad in (0, -3, 65536):
        assert letterbox(B=bad) == -1 and b"batch" in lib.unet_last_error()
    for bad in (0, -1, 4097):
        assert letterbox(S_h=bad) == -1 and b"bad size" in lib.unet_last_error()
        assert letterbox(S_w=bad) == -1 and b"bad size" in lib.unet_last_error()
    for args in ((None, 64, 1, 1, 1), (1, 64, None, 1, 1), (1, 64, 1, 1, None)):
        assert lib.unet_byte_histogram_u8(*args, None) == -1 and b"null" in lib.unet_last_error()
    for bad in (0, -1, 65536):
        assert lib.unet_byte_histogram_u8(1, 64, 1, bad, 1, None) == -1
        assert b"batch" in lib.unet_last_error()


def test_python_surface_has_no_cpu_fallback(ua):
    arena = torch.zeros(64, dtype=torch.uint8)
    table = torch.tensor([[0, 16, 2, 2, 4, 4, 0, 0]], dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ua.ops.letterbox_u8(arena, table, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ua.ops.byte_histogram_u8(arena, table)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ua.ops.byte_histogram_u8(torch.zeros((1, 4, 4), dtype=torch.uint8))
    with pytest.raises(ValueError):
        ua.dataprep.DeviceLetterbox([], size=(32, 24), mode="letterbox")
    with pytest.raises(ValueError):
        ua.dataprep.DeviceLetterbox([], mode="crop")
