"""GPU (-m gpu): unet_render_seg_panels / unet_render_recon_panels against the numpy restatement
(tests/tools/render_ref.py, pinned to the reference's own arrays by tests/test_render_cpu.py), and
the entry points that write PNGs - evaluate_model, evaluate_reconstruction_quality, gradcam_figure.

Shapes: (3, 5, 7) has an odd width (the scalar path, a ragged last group per row), (2, 33, 40) the
16-byte path with an odd height and several workgroups per image, (1, 64, 64) the size of the
end-to-end runs.

Tolerances.  image, gt, pred, error and target are integer arithmetic or correctly rounded double
arithmetic in a fixed order: byte-equal.  conf0..2 index a 256-entry table with p * 256, p the
fp32 softmax: against an fp64 softmax the index can differ only where p * 256 lies within the fp32
softmax's error of an integer.  That error is a few ulp of p <= 1, about 3e-5 in units of p * 256;
the band left out is 1e-3 (30 x), at most 1 % of the pixels may fall in it (the reference alone
leaves out 0.24 % at (2, 33, 40)), and inside it the index may differ by 1.
"""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3, 5, 7), (2, 33, 40), (1, 64, 64)]
EXACT = ("image", "gt", "pred", "error", "target")


def _load(name):
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(ROOT, "tests", "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load("render_ref")
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def seg_case(shape):
    """The seeded inputs of a shape and their reference panels, computed once and shared."""
    u8, f32, logits, mask = R.make_seg_case(100 + shape[1], *shape)
    for a in (u8, f32, logits, mask):
        a.setflags(write=False)
    want = {(form, p): R.seg_panel(p, img, logits, mask, None, 2)
            for form, img in (("f32", f32), ("u8", u8)) for p in EXACT}
    return u8, f32, logits, mask, want


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)        # a copy: the shared inputs are read-only


@pytest.mark.parametrize("mask_dtype", ["int64", "uint8"])
@pytest.mark.parametrize("form", ["f32", "u8"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_exact_panels_are_byte_equal(ua, shape, form, mask_dtype):
    u8, f32, logits, mask, want = seg_case(shape)
    image = _dev(f32 if form == "f32" else u8)
    m = _dev(mask if mask_dtype == "int64" else mask.astype(np.uint8))
    got = ua.ops.render_seg_panels(image, _dev(logits), m, panels=EXACT, target_class=2)
    B, H, W = shape
    assert got.dtype == torch.uint8 and tuple(got.shape) == (B, H, len(EXACT), W, 3)
    got = got.cpu().numpy()
    for k, p in enumerate(EXACT):
        bad = int((got[:, :, k] != want[form, p]).sum())
        print(f"{shape} {form} {mask_dtype} {p}: {bad} bytes differ")
        assert bad == 0, p
    # the memory is the picture of the whole batch
    pic = ua.render.figure(image, _dev(logits), m, EXACT, target_class=2).cpu().numpy()
    assert np.array_equal(pic, got.reshape(B * H, len(EXACT) * W, 3))


def test_panel_order_repeats_and_out_argument(ua):
    shape = SHAPES[1]
    u8, f32, logits, mask, want = seg_case(shape)
    panels = ("pred", "image", "pred", "gt", "image", "error", "target", "gt", "image")   # 9
    out = torch.full((shape[0], shape[1], 9, shape[2], 3), 77, dtype=torch.uint8, device=DEV)
    got = ua.ops.render_seg_panels(_dev(u8), _dev(logits), _dev(mask), panels=panels,
                                   target_class=2, out=out)
    assert got is out
    got = got.cpu().numpy()
    for k, p in enumerate(panels):
        assert np.array_equal(got[:, :, k], want["u8", p]), (k, p)
    # an image panel alone needs neither logits nor mask
    alone = ua.ops.render_seg_panels(_dev(f32), None, panels=("image",)).cpu().numpy()
    assert np.array_equal(alone[:, :, 0], want["f32", "image"])
    with pytest.raises(TypeError, match="out must be"):
        ua.ops.render_seg_panels(_dev(u8), _dev(logits), _dev(mask), out=out)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_confidence_panels_against_fp64_softmax(ua, shape):
    u8, f32, logits, mask, _ = seg_case(shape)
    if shape == (2, 33, 40):
        # the case the band's share was measured on
        logits = (np.random.default_rng(0).standard_normal((2, 3, 33, 40)) * 2).astype(np.float32)
    names = ("conf0", "conf1", "conf2")
    got = ua.ops.render_seg_panels(_dev(u8), _dev(logits), panels=names).cpu().numpy()
    lut = R.jet_lut()
    idx64 = [R.lut_index(R.softmax64(logits)[:, c]) for c in range(3)]
    band = np.stack([R.conf_band(logits, c) for c in range(3)])
    share = band.mean()
    print(f"{shape}: share of pixels inside the 1e-3 band {share:.4%}")
    assert share <= 0.01
    for c, name in enumerate(names):
        want = R.half_sum(u8, lut[idx64[c]])
        out = ~band[c]
        bad = int((got[:, :, c][out] != want[out]).sum())
        print(f"{shape} {name}: {bad} bytes differ outside the band")
        assert bad == 0, name
        # inside the band the table index is the fp64 one or a neighbour
        near = np.zeros(band[c].shape, dtype=bool)
        for d in (-1, 0, 1):
            cand = R.half_sum(u8, lut[np.clip(idx64[c] + d, 0, 255)])
            near |= (got[:, :, c] == cand).all(axis=-1)
        assert near[band[c]].all(), name


def test_heat_panel_covers_every_table_entry(ua):
    B, H, W = 2, 9, 33                                        # 297 >= 256 + 5 values per image
    u8 = np.random.default_rng(4).integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)
    vals = np.concatenate([(np.arange(256) + 0.5) / 256, [0.0, 1.0, -0.1, 1.5, np.nan],
                           np.arange(36) / 36]).astype(np.float32)
    heat = np.stack([vals, vals[::-1]]).reshape(B, H, W)
    for W_, h_, u_ in ((W, heat, u8), (32, heat[:, :, :32].copy(), u8[:, :, :32].copy())):
        got = ua.ops.render_seg_panels(_dev(u_), None, None, _dev(h_), panels=("heat", "image"))
        want = R.seg_panel("heat", u_, heat=h_)
        assert np.array_equal(got.cpu().numpy()[:, :, 0], want), W_
        assert np.array_equal(got.cpu().numpy()[:, :, 1], u_), W_
    lut = R.jet_lut()
    k = np.arange(256)
    assert np.array_equal(R.lut_index(vals[:256]), k)
    assert list(R.lut_index(vals[256:261])) == [0, 255, 0, 255, 0]
    assert np.array_equal(R.seg_panel("heat", u8, heat=heat)[0].reshape(-1, 3)[:256],
                          R.half_sum(u8[0].reshape(-1, 3)[:256], lut))


def _recon_check(ua, original, recon):
    got = ua.ops.render_recon_panels(_dev(original), _dev(recon)).cpu().numpy()
    want = R.recon_panels(original, recon)
    assert got.shape == want.shape
    for k, name in enumerate(("original", "reconstruction", "error map")):
        bad = int((got[:, :, k] != want[:, :, k]).sum())
        print(f"recon {original.shape} {original.dtype} {name}: {bad} bytes differ")
        assert bad == 0, name
    return want


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_recon_panels_are_byte_equal(ua, shape):
    B, H, W = shape
    o, r = R.make_recon_case(7 + H, 3, H, W)                 # B = 3: the maxima differ per image
    want = _recon_check(ua, o, r)
    maxima = [int(np.abs(want[b, :, 0].astype(int) - want[b, :, 1].astype(int)).max())
              for b in range(3)]
    assert len(set(maxima)) == 3, maxima                      # a batch-wide maximum would show
    _recon_check(ua, R.unit_bytes(o), r)                      # uint8 original
    lut = R.jet_lut()
    same = _recon_check(ua, o, o.copy())                      # m = 0
    assert (same[:, :, 2] == lut[0]).all()
    one = o.copy()
    one[2, 1, H // 2, W - 1] += 0.5                           # one differing value
    w1 = _recon_check(ua, o, one)
    assert ((w1[:, :, 2] != lut[0]).any(axis=-1).sum()) == 1


# ---- end to end ----------------------------------------------------------------------------------
def _seg_batches(n, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n):
        mask = torch.randint(0, 3, (2, 64, 64), generator=g)
        mask[:, :4] = 255
        out.append({"image": torch.randn(2, 3, 64, 64, generator=g), "mask": mask,
                    "original_dims": torch.tensor([[64, 64], [50, 70]])})
    return out


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def test_evaluate_model_writes_the_three_figures(ua, tmp_path):
    torch.manual_seed(0)
    model = ua.create_model(DEV)
    model.eval()
    loader = _seg_batches(2, 1)
    plain = ua.evaluate.evaluate_model(model, loader, DEV)
    out = tmp_path / "figs"
    res = ua.evaluate.evaluate_model(model, loader, DEV, visualize_samples=1, output_dir=str(out))
    assert _same(res, plain)                                  # bit for bit
    assert sorted(os.listdir(out)) == ["confidence_batch0.png", "errors_batch0.png",
                                       "predictions_batch0.png"]
    images, masks = loader[0]["image"].to(DEV), loader[0]["mask"]
    logits = ua.evaluate._eval_logits(model, images).cpu().numpy()
    img, m = loader[0]["image"].numpy(), masks.numpy()
    want = R.seg_panels(img, logits, m, None, ("image", "gt", "pred", "error"))
    B, H, P, W, _ = want.shape
    err = R.read_png(str(out / "errors_batch0.png"))
    assert np.array_equal(err, want.reshape(B * H, P * W, 3))
    pred = R.read_png(str(out / "predictions_batch0.png"))
    assert np.array_equal(pred, want[:, :, :3].reshape(B * H, 3 * W, 3))
    conf = R.read_png(str(out / "confidence_batch0.png"))
    assert conf.shape == (B * H, 4 * W, 3)
    assert np.array_equal(conf[:, :W], want[:, :, 0].reshape(B * H, W, 3))
    # the figure builders give the same pictures from their own forward
    assert np.array_equal(ua.render.error_figure(model, loader[0], DEV).cpu().numpy(), err)
    assert np.array_equal(ua.render.prediction_figure(model, loader[0], DEV).cpu().numpy(), pred)
    assert np.array_equal(ua.render.confidence_figure(model, loader[0], DEV).cpu().numpy(), conf)
    with pytest.raises(NotImplementedError):
        ua.evaluate.evaluate_model(model, loader, DEV, visualize_samples=1)


def test_evaluate_reconstruction_quality_writes_comparisons(ua, tmp_path):
    torch.manual_seed(0)
    model = ua.ae.create_model(DEV)
    g = torch.Generator().manual_seed(2)

    class Loader(list):
        dataset = range(4)

    imgs = [torch.rand(2, 3, 64, 64, generator=g) for _ in range(2)]
    loader = Loader([{"image": imgs[0], "target": imgs[0], "filename": ["a.jpg", "b.png"]},
                     {"image": imgs[1], "target": imgs[1], "filename": ["c.PNG", "d"]}])
    plain = ua.ae.evaluate_reconstruction_quality(model, loader, DEV)
    res = ua.ae.evaluate_reconstruction_quality(model, loader, DEV, output_dir=str(tmp_path),
                                                visualize_samples=3)
    assert res == plain
    vis = tmp_path / "visualizations"
    assert sorted(os.listdir(vis)) == ["comparison_0_a.jpg.png", "comparison_1_b.png",
                                       "comparison_2_c.PNG"]
    model.eval()
    with torch.no_grad():
        recon = torch.cat([model(x.to(DEV)).float() for x in imgs]).cpu().numpy()
    want = R.recon_panels(torch.cat(imgs).numpy(), recon)
    for i, name in enumerate(sorted(os.listdir(vis))):
        assert np.array_equal(R.read_png(str(vis / name)), want[i].reshape(64, 3 * 64, 3)), name
    # without names: sample_{i}.png
    bare = Loader([{"image": imgs[0], "target": imgs[0]}])
    ua.ae.evaluate_reconstruction_quality(model, bare, DEV, output_dir=str(tmp_path / "bare"),
                                          visualize_samples=1)
    assert os.listdir(tmp_path / "bare" / "visualizations") == ["comparison_0_sample_0.png"]
    with pytest.raises(NotImplementedError):
        ua.ae.evaluate_reconstruction_quality(model, loader, DEV, visualize_samples=3)


def test_gradcam_figure_skips_images_without_the_class(ua):
    torch.manual_seed(0)
    model = ua.create_model(DEV)
    model.eval()
    g = torch.Generator().manual_seed(3)
    mask = torch.randint(0, 3, (3, 64, 64), generator=g)
    mask[1][mask[1] == 1] = 2                                 # image 1 lacks class 1
    batch = {"image": torch.randn(3, 3, 64, 64, generator=g), "mask": mask}
    heat, present = ua.evaluate.gradcam_batch(model, batch, DEV, target_class=1)
    assert present.tolist() == [True, False, True]
    fig = ua.render.gradcam_figure(model, batch, DEV, target_class=1)
    assert fig.dtype == torch.uint8 and tuple(fig.shape) == (2 * 64, 3 * 64, 3)
    keep = [0, 2]
    want = R.seg_panels(batch["image"].numpy()[keep], None, mask.numpy()[keep],
                        heat.cpu().numpy()[keep], ("image", "target", "heat"), 1)
    assert np.array_equal(fig.cpu().numpy(), want.reshape(2 * 64, 3 * 64, 3))
