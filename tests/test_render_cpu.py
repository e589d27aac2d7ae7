"""CPU (-m "not gpu"): the evaluation pictures without a device - the numpy restatement
(tests/tools/render_ref.py) against the arrays recorded from the reference's own figure code
(tests/golden/render.npz, tests/tools/make_golden_render.py), the jet table against matplotlib,
the PNG writer, the ABI surface of unet_render_seg_panels / unet_render_recon_panels and the
argument checks of their wrappers."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "unet_hip.h")


def _load(name):
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(ROOT, "tests", "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load("render_ref")


def test_restatement_reproduces_the_reference_arrays(golden):
    g = golden("render")
    image, logits, mask = g["image"], g["logits"], g["mask"]
    u8, f32, z, m = R.make_seg_case(int(g["seed"]), *mask.shape)
    assert np.array_equal(f32, image) and np.array_equal(z, logits) and np.array_equal(m, mask)
    assert np.array_equal(R.seg_panel("image", image), g["ref_image_u8"])
    assert np.array_equal(R.seg_panel("gt", image, logits, mask), g["ref_gt"])
    assert np.array_equal(R.seg_panel("pred", image, logits, mask), g["ref_pred"])
    assert np.array_equal(R.seg_panel("error", image, logits, mask), g["ref_error"])
    # line :277 of the reference on the float image it shows
    assert np.array_equal((g["ref_image_float"] * 255).astype(np.uint8), g["ref_image_u8"])
    # the blend is the truncating half-sum
    colour = R.ERROR_COLOURS[R.error_code(logits.argmax(axis=1), mask)]
    want = (g["ref_image_u8"] * 0.5 + colour * 0.5).astype(np.uint8)
    assert np.array_equal(g["ref_error"], want)
    # the case exercises what it is meant to: both sides of a truncation boundary, clipping,
    # every mask value, every error category, ties
    back = g["ref_image_u8"]
    assert (back == u8).any() and (back.astype(int) == u8.astype(int) - 1).any()
    assert set(np.unique(mask)) == {0, 1, 2, 7, 255}
    assert set(np.unique(R.error_code(logits.argmax(axis=1), mask))) == {0, 1, 2, 3, 4}
    assert ((logits[:, 0] == logits[:, 1]) & (logits[:, 1] == logits[:, 2])).any()
    # 255 and the out-of-range label are black in the ground-truth panel
    assert not g["ref_gt"][(mask == 255) | (mask == 7)].any()


def test_jet_table_is_matplotlibs(ua):
    matplotlib = pytest.importorskip("matplotlib")
    lut = ua.render.jet_lut()
    assert lut.dtype == np.uint8 and lut.shape == (256, 3)
    assert np.array_equal(lut, R.jet_lut())
    want = matplotlib.colormaps["jet"](np.arange(256), bytes=True)[:, :3]
    assert np.array_equal(lut, want)
    # the index rule: a value in [0, 1] shows entry min(int(v * 256), 255)
    v = np.concatenate([np.random.default_rng(0).random(20000).astype(np.float32),
                        np.arange(257, dtype=np.float32) / 256])
    assert np.array_equal(matplotlib.colormaps["jet"](v, bytes=True)[:, :3], lut[R.lut_index(v)])
    reds = matplotlib.colormaps["Reds"]
    assert tuple(reds(0.0, bytes=True)[:3]) == ua.render.REDS_LOW == R.REDS_LOW
    assert tuple(reds(1.0, bytes=True)[:3]) == ua.render.REDS_HIGH == R.REDS_HIGH


def test_write_png_round_trips(ua, tmp_path):
    rng = np.random.default_rng(3)
    for shape in ((1, 1, 3), (5, 7, 3), (64, 192, 3)):
        a = rng.integers(0, 256, size=shape, dtype=np.uint8)
        path = str(tmp_path / f"p{shape[0]}.png")
        ua.render.write_png(path, torch.from_numpy(a) if shape[0] == 5 else a)
        assert np.array_equal(R.read_png(path), a)
    a = rng.integers(0, 256, size=(6, 8, 3), dtype=np.uint8)
    ua.render.write_png(str(tmp_path / "strided.png"), a[::2, ::2])      # not contiguous
    assert np.array_equal(R.read_png(str(tmp_path / "strided.png")), a[::2, ::2])
    PIL = pytest.importorskip("PIL.Image")
    assert np.array_equal(np.asarray(PIL.open(str(tmp_path / "p64.png"))), R.read_png(
        str(tmp_path / "p64.png")))
    with pytest.raises(TypeError):
        ua.render.write_png(str(tmp_path / "bad.png"), np.zeros((4, 4), dtype=np.uint8))
    with pytest.raises(TypeError):
        ua.render.write_png(str(tmp_path / "bad.png"), np.zeros((4, 4, 3), dtype=np.float32))


def test_entry_points_declared_exported_and_bound(ua):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    handle = ctypes.CDLL(ua.LIB_PATH)
    for name, nargs in (("unet_render_seg_panels", 14), ("unet_render_recon_panels", 10)):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), f"{name} not declared in unet_hip.h"
        assert hasattr(handle, name), f"{name} not exported"
        assert len(ua._lib.SIGNATURES[name][1]) == nargs
    ids = dict(re.findall(r"#define\s+UNET_RENDER_(\w+)\s+(\d+)", text))
    assert [int(ids[p.upper()]) for p in ua.ops.RENDER_PANELS] == list(range(9))
    assert ua.ops.RENDER_PANELS == R.PANELS
    assert ua._lib.ABI_VERSION == 11                    # new exports only
    for name in ("prediction_figure", "confidence_figure", "error_figure", "gradcam_figure",
                 "write_png", "jet_lut"):
        assert callable(getattr(ua.render, name))


def test_host_arguments_are_rejected_before_any_launch(ua):
    lib = ua.lib()
    one = lambda *names: sum((ua.ops.RENDER_PANELS.index(n) + 1) << (4 * k)  # noqa: E731
                             for k, n in enumerate(names))
    seg = lambda image, logits, mask, heat, panels, B=1, H=8, W=8: \
        lib.unet_render_seg_panels(image, 0, logits, mask, 0, heat, 1, 1, panels, 1, B, H, W, None)  # noqa: E731
    assert seg(None, 1, 1, 1, one("image")) == -1 and b"null" in lib.unet_last_error()
    assert seg(1, 1, 1, 1, one("image"), H=0) == -1 and b"bad shape" in lib.unet_last_error()
    assert seg(1, 1, 1, 1, one("image"), B=0) == -1 and b"bad shape" in lib.unet_last_error()
    assert seg(1, 1, 1, 1, 0) == -1 and b"panel list" in lib.unet_last_error()
    assert seg(1, 1, 1, 1, one(*["image"] * 10)) == -1 and b"panel list" in lib.unet_last_error()
    assert seg(1, 1, 1, 1, 10) == -1 and b"unknown panel" in lib.unet_last_error()
    for p in ("gt", "error", "target"):
        assert seg(1, 1, None, 1, one("image", p)) == -1 and b"mask" in lib.unet_last_error()
    for p in ("pred", "error", "conf0", "conf2"):
        assert seg(1, None, 1, 1, one(p)) == -1 and b"logits" in lib.unet_last_error()
    assert seg(1, 1, 1, None, one("image", "heat")) == -1 and b"heat" in lib.unet_last_error()
    rec = lambda o, r, jet, mx, out, B=1, H=8, W=8: \
        lib.unet_render_recon_panels(o, 0, r, jet, mx, out, B, H, W, None)  # noqa: E731
    for args in ((None, 1, 1, 4, 1), (1, None, 1, 4, 1), (1, 1, None, 4, 1), (1, 1, 1, None, 1),
                 (1, 1, 1, 4, None)):
        assert rec(*args) == -1 and b"null" in lib.unet_last_error()
    assert rec(1, 1, 1, 4, 1, W=0) == -1 and b"bad shape" in lib.unet_last_error()


def test_python_surface_has_no_cpu_fallback(ua, tmp_path):
    img, z = torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8)
    u8 = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    t = torch.zeros(1, 8, 8, dtype=torch.int64)
    for image in (img, u8):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ua.ops.render_seg_panels(image, z, t)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ua.ops.render_recon_panels(image, z)
    for bad in (img.double(), img.half(), torch.zeros(1, 8, 8, 3), torch.zeros(1, 3, 8, 8,
                                                                              dtype=torch.uint8)):
        with pytest.raises(TypeError, match="fp32 .B,3,H,W. or uint8 .B,H,W,3."):
            ua.ops.render_seg_panels(bad, z, t)
        with pytest.raises(TypeError, match="fp32 .B,3,H,W. or uint8 .B,H,W,3."):
            ua.ops.render_recon_panels(bad, z)
    for p in ("gt", "error", "target"):
        with pytest.raises(TypeError, match="need the mask"):
            ua.ops.render_seg_panels(img, z, None, panels=("image", p))
    with pytest.raises(TypeError, match="need the logits"):
        ua.ops.render_seg_panels(img, None, t, panels=("image", "pred"))
    with pytest.raises(TypeError, match="needs the heat map"):
        ua.ops.render_seg_panels(img, z, t, panels=("heat",))
    with pytest.raises(ValueError, match="unknown panel"):
        ua.ops.render_seg_panels(img, z, t, panels=("image", "jet"))
    with pytest.raises(ValueError, match="1 to 9 panels"):
        ua.ops.render_seg_panels(img, z, t, panels=("image",) * 10)
    # the entry points still raise without somewhere to put the pictures
    with pytest.raises(NotImplementedError):
        ua.evaluate.evaluate_model(None, [], "cpu", visualize_samples=3)
    with pytest.raises(NotImplementedError):
        ua.ae.evaluate_reconstruction_quality(None, [], "cpu", visualize_samples=3)


def test_recon_restatement_properties():
    """What the comparison picture's definition promises, on the restatement the GPU test
    compares against: identical images give a zero map (jet[0]), the maximum is per image, and
    the gray weights sum to 2^14 so a gray error keeps its value."""
    lut = R.jet_lut()
    o, r = R.make_recon_case(5, 3, 6, 10)
    same = R.recon_panels(o, o.copy())
    assert np.array_equal(same[:, :, 0], same[:, :, 1]) and (same[:, :, 2] == lut[0]).all()
    assert tuple(same[0, 0, 0, :3, 0]) == (0, 255, 255)                # -0.25, 1.5, 1.0 clamped
    full = R.recon_panels(o, r)
    for b in range(3):
        alone = R.recon_panels(o[b:b + 1], r[b:b + 1])
        assert np.array_equal(full[b], alone[0])
    d = [np.abs(R.unit_bytes(o)[b].astype(int) - R.unit_bytes(r)[b].astype(int)).max()
         for b in range(3)]
    assert len(set(d)) == 3, d
    assert 4899 + 9617 + 1868 == 1 << 14
    u8 = np.zeros((1, 4, 4, 3), dtype=np.uint8)
    r0 = np.zeros((1, 3, 4, 4), dtype=np.float32)
    r0[0, :, 1, 2] = 1.0                                               # one gray pixel differs
    one = R.recon_panels(u8, r0)
    assert (one[0, 1, 2, 2] == lut[255]).all() and (one[0, 0, 2, 0] == lut[0]).all()
