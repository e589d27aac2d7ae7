"""GPU (-m gpu): connected components, mask cleanup and the class-map confusion count
(csrc/postprocess.hip, unet_eval_confusion_classes) against tests/tools/postprocess_ref.py.

Everything is integer work, so every comparison is exact (np.array_equal / torch.equal), and every
call asks for the kernels' status word (check=True): a bounded loop that ran into its limit fails
the test.  Shapes are the smallest that cross the seams of the 64 x 32 tile: below one tile,
no multiple of the tile in either axis, at least 3 x 3 tiles.

Figures: nothing here is a tolerance; there are no figures to record."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _load(name):
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(ROOT, "tests", "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load("postprocess_ref")
DEV = "cuda:0"

LABEL_SHAPES = [(1, 1, 1), (1, 7, 5), (2, 37, 53), (3, 96, 160), (2, 130, 67)]
NOISE = (0.41, 0.5, 0.59, 0.8)


# ------------------------------------------------------------------------------ labelling inputs
def label_patterns(B, H, W):
    """name -> uint8 [B, H, W]; K = 3 everywhere (bytes 3..5 of "bytes" read as 0)."""
    z = lambda: np.zeros((B, H, W), dtype=np.uint8)   # noqa: E731
    yy, xx = np.mgrid[0:H, 0:W]
    pats = {"zeros": z(), "ones": z() + 1}
    m = z(); m[:, 0, 0] = m[:, 0, -1] = m[:, -1, 0] = m[:, -1, -1] = 1
    pats["corners"] = m
    m = z(); m[:] = ((yy + xx) % 2 == 0)
    pats["checkerboard"] = m
    m = z(); m[:, :, ::2] = 1; m[:, -1, :] = 1        # teeth down the image, joined at the bottom
    pats["vcomb"] = m
    m = z(); m[:, ::2, :] = 1; m[:, :, -1] = 1        # teeth along the image, joined at the right
    pats["hcomb"] = m
    m = z(); m[:, :, 0] = 1; m[:, :, -1] = 1; m[:, -1, :] = 1
    pats["u"] = m
    m = z(); m[:, ::2, :] = 1                         # one-pixel path through every tile
    for y in range(1, H, 2):
        m[:, y, -1 if (y // 2) % 2 == 0 else 0] = 1
    pats["serpentine"] = m
    for d in NOISE:
        pats[f"noise{d}"] = (np.random.RandomState(int(d * 100) + H * W).rand(B, H, W) < d) \
            .astype(np.uint8)
    rs = np.random.RandomState(7 + H + W)
    pats["two_class"] = ((rs.rand(B, H, W) < 0.62) * rs.randint(1, 3, (B, H, W))).astype(np.uint8)
    pats["bytes"] = rs.randint(0, 6, (B, H, W)).astype(np.uint8)
    m = z(); m[:, 0, :] = 1; m[:, -1, :] = 2          # image b ends full, image b + 1 starts full
    pats["batch_seam"] = m
    m = z(); m[:, :, 0] = 1; m[:, :, -1] = 1          # the rows must not join through the wrap
    pats["wrap"] = m
    return pats


@functools.lru_cache(maxsize=None)
def label_case(shape):
    return label_patterns(*shape)


@functools.lru_cache(maxsize=None)
def label_reference(shape, name, connectivity, mode):
    return R.cc(label_case(shape)[name], connectivity, mode, 3)


def selected(classes, mode):
    c = R.sanitize(classes, 3)
    return int(((c == 0) if mode == "background" else (c != 0)).sum())


# ---------------------------------------------------------------------------------- labelling
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("shape", LABEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_labels_and_areas_equal_the_reference(ua, shape, connectivity, mode):
    for name, classes in label_case(shape).items():
        want_l, want_a = label_reference(shape, name, connectivity, mode)
        dev = torch.from_numpy(classes).to(DEV)
        labels, areas = ua.ops.cc_label(dev, connectivity, mode, 3, check=True)
        assert labels.dtype == torch.uint32 and areas.dtype == torch.uint32
        got_l, got_a = labels.cpu().numpy(), areas.cpu().numpy()
        assert np.array_equal(got_l, want_l), (name, "labels")
        assert np.array_equal(got_a, want_a), (name, "areas")
        assert int(got_a.astype(np.int64).sum()) == selected(classes, mode), name
        again = ua.ops.cc_label(dev, connectivity, mode, 3, check=True)
        assert torch.equal(again[0].view(torch.int32), labels.view(torch.int32)), name
        assert torch.equal(again[1].view(torch.int32), areas.view(torch.int32)), name


def test_known_component_counts_of_the_structured_patterns():
    """The reference itself on the patterns whose answer is known in closed form."""
    shape = (2, 37, 53)
    H, W = shape[1:]
    n = lambda name, c, m="foreground": [   # noqa: E731
        len(np.unique(l[l != 0])) for l in label_reference(shape, name, c, m)[0]]
    assert n("checkerboard", 8) == [1, 1] and n("checkerboard", 4) == [(H * W + 1) // 2] * 2
    for name in ("vcomb", "hcomb", "u", "serpentine"):
        assert n(name, 4) == [1, 1] and n(name, 8) == [1, 1], name
    assert n("batch_seam", 8) == [2, 2] and n("wrap", 8) == [2, 2]
    assert n("corners", 8) == [4, 4] and n("zeros", 8) == [0, 0] and n("ones", 4) == [1, 1]
    assert n("ones", 8, "background") == [0, 0] and n("zeros", 4, "background") == [1, 1]


def test_connected_components_wrapper_and_default_class_count(ua):
    """ua.postprocess.connected_components passes 32 classes when none is given: a byte of 31 is
    a class, a byte of 32 reads as 0."""
    m = np.zeros((1, 5, 7), dtype=np.uint8)
    m[0, 1, 1:3] = 31
    m[0, 3, 4:6] = 32
    labels, areas = ua.postprocess.connected_components(torch.from_numpy(m).to(DEV))
    want = R.cc(m, 8, "foreground", 32)
    assert np.array_equal(labels.cpu().numpy(), want[0])
    assert np.array_equal(areas.cpu().numpy(), want[1])
    assert int(areas.cpu().numpy().sum()) == 2


@pytest.mark.parametrize("mode", R.MODES)
def test_memory_around_labels_and_areas_is_untouched(ua, mode):
    """The C entry point writes B * H * W words of each output and nothing beside them."""
    B, H, W = 2, 37, 53
    classes = torch.from_numpy(label_case((B, H, W))["two_class"]).to(DEV)
    n, guard = B * H * W, 4096
    poison = 0x5EADBEE5
    buf = torch.full((2 * n + 3 * guard,), poison, dtype=torch.int32, device=DEV)
    lab, are = buf[guard:guard + n], buf[2 * guard + n:2 * guard + 2 * n]
    L = ua.lib()
    ws = torch.empty(L.unet_cc_workspace_bytes(B, H, W), dtype=torch.uint8, device=DEV)
    ua._lib.check(L.unet_cc_label_u8(classes.data_ptr(), lab.data_ptr(), are.data_ptr(),
                                     ws.data_ptr(), ws.numel(), B, 3, H, W, 8,
                                     ua.ops.CC_MODES[mode],
                                     torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert ua.ops.postprocess_status(ws) == 0
    host = buf.cpu().numpy()
    for a, b in ((0, guard), (guard + n, 2 * guard + n), (2 * guard + 2 * n, len(host))):
        assert (host[a:b] == poison).all()
    want = label_reference((B, H, W), "two_class", 8, mode)
    assert np.array_equal(host[guard:guard + n].view(np.uint32), want[0].reshape(-1))
    assert np.array_equal(host[2 * guard + n:2 * guard + 2 * n].view(np.uint32),
                          want[1].reshape(-1))


def test_spiral_at_512_is_one_component_and_so_is_its_complement(ua):
    """The longest path the bounded loops can meet, in closed form: a one-pixel-wide rectangular
    spiral with a one-pixel gap.  Under 4-connectivity it is one component whose first pixel is
    (0, 0) and whose area is the number of set pixels; its complement is one background
    component."""
    s = R.spiral(512, 512)
    classes = np.stack([s, s[:, ::-1]])                 # (row 0 is full in both)
    n_set = int(s.sum())
    dev = torch.from_numpy(np.ascontiguousarray(classes)).to(DEV)
    labels, areas = ua.ops.cc_label(dev, 4, "foreground", 3, check=True)
    labels, areas = labels.cpu().numpy(), areas.cpu().numpy()
    for b in range(2):
        assert np.array_equal(labels[b], classes[b].astype(np.uint32))      # label 1 = pixel (0, 0)
        assert areas[b, 0, 0] == n_set and int(areas[b].astype(np.int64).sum()) == n_set
    labels, areas = ua.ops.cc_label(dev, 4, "background", 3, check=True)
    labels, areas = labels.cpu().numpy(), areas.cpu().numpy()
    for b in range(2):
        first = int(np.argmax(classes[b].reshape(-1) == 0))
        assert np.array_equal(labels[b], np.where(classes[b] == 0, first + 1, 0).astype(np.uint32))
        assert areas[b].reshape(-1)[first] == 512 * 512 - n_set
        assert int(areas[b].astype(np.int64).sum()) == 512 * 512 - n_set


# ------------------------------------------------------------------------------------ cleanup
SETTINGS = {
    "off": dict(),
    "vote_image": dict(vote="image"),
    "vote_component": dict(vote="component"),
    "keep_largest": dict(keep_largest=True),
    "min_area": dict(min_area=5),
    "fill_holes": dict(fill_holes=True),
    "fill_small_holes": dict(fill_holes=True, max_hole_area=9),
    "pet": dict(vote="image", keep_largest=True, fill_holes=True),
    "all_image": dict(vote="image", keep_largest=True, min_area=5, fill_holes=True,
                      max_hole_area=9),
    "all_component": dict(vote="component", keep_largest=True, min_area=5, fill_holes=True,
                          max_hole_area=9),
    "component_small": dict(vote="component", min_area=5, fill_holes=True, max_hole_area=9),
}


def blob_batch(B, H, W, hi, lo):
    """(speckled, clean): the speckled blob of the reference tools with classes (lo, hi) for
    (1, 2)."""
    lut = np.array([0, lo, hi], dtype=np.uint8)
    pairs = [R.speckled_blob(H, W, seed=b) for b in range(B)]
    return np.stack([lut[p[0]] for p in pairs]), np.stack([lut[p[1]] for p in pairs])


@functools.lru_cache(maxsize=None)
def cleanup_inputs(B, H, W, K):
    """uint8 [n * B, H, W]: every input family stacked along the batch (images never interact)."""
    hi, lo = K - 1, (1 if K == 3 else 7)
    z = lambda: np.zeros((B, H, W), dtype=np.uint8)   # noqa: E731
    yy, xx = np.mgrid[0:H, 0:W]
    maps = [blob_batch(B, H, W, hi, lo)[0]]
    ring = np.minimum(np.minimum(yy, H - 1 - yy), np.minimum(xx, W - 1 - xx))
    m = z(); m[:] = np.where(ring % 4 == 1, lo, np.where(ring % 4 == 3, hi, 0))   # nested rings
    maps.append(m)
    m = z(); m[:, 3:16, 4:20] = hi; m[:, 6:13, 8:16] = 0; m[:, 8:11, 10:13] = lo   # island in hole
    maps.append(m)
    m = z(); m[:, 2:9, 0:9] = lo; m[:, 4:7, 1:4] = 0; m[:, 12:20, 0:6] = hi; m[:, 14, 1] = 0
    maps.append(m)                                                                  # hole at x = 1
    m = z() + hi                                                                    # holes on edges
    m[:, 0, 5:8] = 0; m[:, -1, 9:12] = 0; m[:, 10:13, 0] = 0; m[:, 15:18, -1] = 0
    m[:, 20:23, 20:23] = 0
    maps.append(m)
    maps.append(z())
    maps.append(z() + lo)
    rs = np.random.RandomState(H * W + K)
    maps.append(((rs.rand(B, H, W) < 0.6) * rs.randint(1, K, (B, H, W))).astype(np.uint8))
    maps.append(rs.randint(0, K + 3, (B, H, W)).astype(np.uint8))                  # bytes >= K
    return np.ascontiguousarray(np.concatenate(maps))


@functools.lru_cache(maxsize=None)
def cleanup_reference(B, H, W, K, connectivity, name):
    return R.cleanup(cleanup_inputs(B, H, W, K), K, connectivity=connectivity, **SETTINGS[name])


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("K", [3, 21])
@pytest.mark.parametrize("shape", [(2, 37, 53), (3, 96, 160)], ids=lambda s: "x".join(map(str, s)))
def test_cleanup_equals_the_reference(ua, shape, K, connectivity):
    classes = cleanup_inputs(*shape, K)
    dev = torch.from_numpy(classes).to(DEV)
    changed = 0
    for name, kw in SETTINGS.items():
        want = cleanup_reference(*shape, K, connectivity, name)
        pp = ua.MaskCleanup(connectivity=connectivity, **kw)
        got = pp(dev, K, check=True)
        assert got.dtype == torch.uint8 and got.data_ptr() != dev.data_ptr()
        bad = np.nonzero((got.cpu().numpy() != want).reshape(len(want), -1).any(axis=1))[0]
        assert len(bad) == 0, (name, "images", bad.tolist())
        changed += int((want != R.sanitize(classes, K)).sum())
        # in == out gives the out-of-place result
        alias = dev.clone()
        assert ua.ops.mask_cleanup(alias, K, connectivity=connectivity, out=alias, check=True,
                                   **kw) is alias
        assert torch.equal(alias, got), (name, "aliased")
    assert torch.equal(dev, torch.from_numpy(classes).to(DEV))      # the input is left alone
    assert changed > 0


def test_cleanup_with_everything_off_is_the_identity_but_for_bytes_past_k(ua):
    classes = cleanup_inputs(2, 37, 53, 3)
    got = ua.MaskCleanup()(torch.from_numpy(classes).to(DEV), 3, check=True).cpu().numpy()
    assert np.array_equal(got, np.where(classes >= 3, 0, classes))
    assert (classes >= 3).any()


def test_pet_cleanup_replays_from_a_graph_on_new_bytes(ua):
    """Nothing in the cleanup depends on the host: captured once on one stream, replayed on new
    bytes copied into the captured input, it equals the eager result."""
    K = 3
    a = cleanup_inputs(2, 37, 53, K)
    b = np.ascontiguousarray(a[::-1])
    buf = torch.from_numpy(a).to(DEV)
    pp = ua.MaskCleanup.pet()
    ws = ua.ops.mask_cleanup_workspace(buf, K)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pp(buf, K, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = pp(buf, K, workspace=ws)
    for src in (a, b):
        buf.copy_(torch.from_numpy(src).to(DEV))
        graph.replay()
        got = out.clone()
        assert ua.ops.postprocess_status(ws) == 0
        assert torch.equal(got, pp(buf, K, check=True))
        assert np.array_equal(got.cpu().numpy(), R.cleanup(src, K, **pp.settings()))


def test_pet_cleanup_raises_the_iou_of_both_foreground_classes(ua):
    """Speckled blobs with their clean blobs as the target - a dog speckled with cat, a cat
    speckled with dog, each with pinholes and stray islands: the one-animal rule strictly raises
    the IoU of both foreground classes (here to 1: it restores the clean blobs)."""
    dog, cat = blob_batch(1, 96, 160, 2, 1), blob_batch(1, 96, 160, 1, 2)
    noisy = torch.from_numpy(np.concatenate([dog[0], cat[0]])).to(DEV)
    target = torch.from_numpy(np.concatenate([dog[1], cat[1]])).to(DEV).long()
    before, after = ua.SegmentationMetrics(), ua.SegmentationMetrics()
    before.update_from_classes(noisy, target)
    after.update_from_classes(ua.MaskCleanup.pet()(noisy, 3, check=True), target)
    for cls in (1, 2):
        assert 0.0 < before.compute_iou(cls) < after.compute_iou(cls) == 1.0
    assert before.compute_mean_iou() < after.compute_mean_iou()


# ---------------------------------------------------------------------------------- confusion
def _logits_and_target(seed, B, K, H, W):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, K, H, W, generator=g)
    target = torch.randint(0, K, (B, H, W), generator=g)
    target[torch.rand(B, H, W, generator=g) < 0.05] = 255
    return logits.to(DEV), target.to(DEV)


@pytest.mark.parametrize("dims", [None, [(24, 40), (13, 17), (61, 100)]],
                         ids=["network_size", "original_sizes"])
@pytest.mark.parametrize("K", [3, 5])
def test_confusion_of_the_class_map_equals_the_confusion_of_the_logits(ua, K, dims):
    """(3, 24, 40) with original sizes equal, smaller and larger: the class-map kernel counts what
    the logits kernels count, bit for bit, and what the reference counts on a cleaned map."""
    logits, target = _logits_and_target(5 + K, 3, K, 24, 40)
    d = None if dims is None else torch.tensor(dims, dtype=torch.int64, device=DEV)
    preds = ua.ops.argmax_classes(logits)
    got = ua.ops.eval_confusion_classes(preds, target, d, K)
    assert got.dtype == torch.int64 and tuple(got.shape) == (3, K, K)
    assert torch.equal(got, ua.ops.eval_confusion(logits, target, d))
    assert got.sum().item() > 0
    cleaned = ua.MaskCleanup(vote="component", min_area=3, fill_holes=True)(preds, K, check=True)
    want = R.confusion_at_original_size(cleaned.cpu().numpy(), target.cpu().numpy(), dims, K,
                                        nearest_source_index=ua.train.nearest_source_index)
    assert np.array_equal(ua.ops.eval_confusion_classes(cleaned, target, d, K).cpu().numpy(), want)
    m = ua.SegmentationMetrics(num_classes=K)
    m.update_from_classes(cleaned, target, dims)
    assert np.array_equal(m.confusion_matrix, want.sum(axis=0))


# --------------------------------------------------------------------------------- end to end
def _model_and_loader(ua):
    from oracle import unet_ref as O
    model = ua.UNet()
    model.load_state_dict(O.fill_state_dict(7))
    model = model.to(DEV).eval()
    images, masks = O.synthetic_batch(11, 2, 64, 64)
    dims = torch.tensor([(82, 94), (40, 50)], dtype=torch.int64)
    return model, [{"image": images, "mask": masks.long(), "original_dims": dims}]


def _same(a, b):
    """equality that takes NaN (a class without pixels) for equal to NaN"""
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b or (a != a and b != b)


def test_predict_masks_and_evaluate_model_with_a_cleanup(ua):
    """2 x 64 x 64 with seeded weights: the postprocess argument is the reference's cleanup of what
    the same call returns without it, and without it nothing changes."""
    model, loader = _model_and_loader(ua)
    batch = loader[0]
    images = batch["image"].to(DEV)
    plain = ua.evaluate.evaluate_model(model, loader, DEV)
    pp = ua.MaskCleanup(vote="component", min_area=4, fill_holes=True)
    raw = ua.predict_masks(model, images)
    want = R.cleanup(raw.cpu().numpy(), 3, **pp.settings())
    got = ua.predict_masks(model, images, postprocess=pp)
    assert np.array_equal(got.cpu().numpy(), want)
    assert (want != raw.cpu().numpy()).any()            # the cleanup had something to do

    resized = ua.predict_masks(model, images, batch["original_dims"], postprocess=pp)
    for b, (oh, ow) in enumerate(batch["original_dims"].tolist()):
        rows = ua.train.nearest_source_index(64, oh)
        cols = ua.train.nearest_source_index(64, ow)
        assert np.array_equal(resized[b].cpu().numpy(), want[b][rows][:, cols])

    res = ua.evaluate.evaluate_model(model, loader, DEV, postprocess=pp)
    cm = R.confusion_at_original_size(want, batch["mask"].numpy(), batch["original_dims"].tolist(),
                                      3, nearest_source_index=ua.train.nearest_source_index)
    assert np.array_equal(res["confusion_matrix"], cm.sum(axis=0))
    ref = ua.SegmentationMetrics()
    ref.update_from_confusion(cm)
    assert res["mean_iou"] == ref.compute_mean_iou()
    assert res["dog"]["dice"] == ref.compute_dice(2)

    again = ua.evaluate.evaluate_model(model, loader, DEV)
    assert set(again) == set(plain)
    for key in plain:
        assert _same(again[key], plain[key]), key
    assert not np.array_equal(res["confusion_matrix"], plain["confusion_matrix"])
