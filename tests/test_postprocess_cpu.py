"""Mask post-processing without a GPU: the new exports and the ABI version, the refusals of the C
entry points before any launch and of the Python surface before any device is touched, the
reference of tests/test_postprocess_gpu.py against scipy.ndimage (where it imports) and on
hand-written cases, and the signatures the new keyword-only argument was added to."""
import ctypes
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location(
    "postprocess_ref", os.path.join(ROOT, "tests", "tools", "postprocess_ref.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

EXPORTS = ("unet_cc_workspace_bytes", "unet_cc_label_u8", "unet_mask_cleanup_workspace_bytes",
           "unet_mask_cleanup_u8", "unet_eval_confusion_classes")
UNET_E_INVALID = -1


def test_new_exports_are_present_and_bound_and_the_abi_version_is_11(ua):
    handle = ctypes.CDLL(ua.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    for name in EXPORTS:
        assert hasattr(handle, name), name
        assert name + "(" in header, name
        assert hasattr(ua.lib(), name) and name in ua._lib.SIGNATURES, name
    assert ua.lib().unet_abi_version() == 11
    assert "#define UNET_ABI_VERSION 11" in header
    vp, i, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    assert ua._lib.SIGNATURES["unet_cc_label_u8"] == (i, [vp, vp, vp, vp, sz] + [i] * 6 + [vp])
    assert ua._lib.SIGNATURES["unet_mask_cleanup_u8"] == (i, [vp, vp, vp, sz] + [i] * 10 + [vp])
    assert ua._lib.SIGNATURES["unet_cc_workspace_bytes"] == (sz, [i, i, i])
    assert ua.MaskCleanup is ua.postprocess.MaskCleanup and "MaskCleanup" in ua.__all__


def test_workspaces_are_at_most_16_bytes_a_pixel_whatever_k(ua):
    L = ua.lib()
    for B, H, W in ((1, 1, 1), (8, 512, 512), (3, 96, 160)):
        px = B * H * W
        assert 4 * px <= L.unet_cc_workspace_bytes(B, H, W) <= 4 * px + 4096
        sizes = {L.unet_mask_cleanup_workspace_bytes(B, K, H, W) for K in (2, 3, 21, 32)}
        assert len(sizes) == 1
        assert 0 < sizes.pop() <= 16 * px + 4096 + 256 * B
    assert L.unet_cc_workspace_bytes(0, 8, 8) == 0 and L.unet_cc_workspace_bytes(1, 16385, 8) == 0
    assert L.unet_mask_cleanup_workspace_bytes(1, 33, 8, 8) == 0


def test_c_entry_points_refuse_before_any_launch(ua):
    """Every UNET_E_INVALID case of the header; the pointers point nowhere, so a launch would
    fault and a refusal never reads them."""
    L = ua.lib()
    p, big = 4096, 1 << 40

    def label(classes=p, labels=p, areas=p, ws=p, nbytes=big, B=2, K=3, H=8, W=8, conn=8, mode=0):
        return L.unet_cc_label_u8(classes, labels, areas, ws, nbytes, B, K, H, W, conn, mode, None)

    def clean(cin=p, cout=p, ws=p, nbytes=big, B=2, K=3, H=8, W=8, conn=8, vote=1, keep=1,
              min_area=0, fill=1, max_hole=0):
        return L.unet_mask_cleanup_u8(cin, cout, ws, nbytes, B, K, H, W, conn, vote, keep, min_area,
                                      fill, max_hole, None)

    def count(preds=p, target=p, dims=None, cm=p, B=2, K=3, H=8, W=8, ignore=255):
        return L.unet_eval_confusion_classes(preds, target, dims, cm, B, K, H, W, ignore, None)

    def refused(rc, word):
        assert rc == UNET_E_INVALID
        assert word in L.unet_last_error().decode(), (word, L.unet_last_error())

    for fn, pointers in ((label, ("classes", "labels", "areas", "ws")),
                         (clean, ("cin", "cout", "ws")), (count, ("preds", "target", "cm"))):
        for name in pointers:
            refused(fn(**{name: None}), "null")
        for B in (0, -1, 65536):
            refused(fn(B=B), "B")
        for K in (1, 0, 33):
            refused(fn(K=K), "K")
        for H, W in ((0, 8), (8, 0), (16385, 8), (8, 16385), (-3, 8)):
            refused(fn(H=H, W=W), "H")
    # 16384 x 16384 is 2^28 pixels and passes the shape test; 2^30 is reached only beyond the
    # per-axis limit, so H * W > 2^30 is refused through it
    for conn in (0, 6, 5, -8):
        refused(label(conn=conn), "connectivity")
        refused(clean(conn=conn), "connectivity")
    for mode in (-1, 3):
        refused(label(mode=mode), "mode")
    for vote in (-1, 3):
        refused(clean(vote=vote), "vote")
    refused(clean(min_area=-1), "min_area")
    refused(clean(max_hole=-1), "max_hole_area")
    refused(label(nbytes=L.unet_cc_workspace_bytes(2, 8, 8) - 1), "workspace")
    refused(clean(nbytes=L.unet_mask_cleanup_workspace_bytes(2, 3, 8, 8) - 1), "workspace")
    for ignore in (0, 1, 2):
        refused(count(ignore=ignore), "ignore_index")
    refused(count(K=5, ignore=4), "ignore_index")


def test_python_surface_refuses_before_touching_a_device(ua):
    u8 = torch.zeros(1, 8, 8, dtype=torch.uint8)
    target = torch.zeros(1, 8, 8, dtype=torch.int64)
    pp = ua.MaskCleanup.pet()
    # a CPU tensor: no fallback
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ua.ops.cc_label(u8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ua.ops.mask_cleanup(u8, 3, vote="image")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ua.ops.eval_confusion_classes(u8, target)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pp(u8, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ua.postprocess.connected_components(u8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ua.SegmentationMetrics().update_from_classes(u8, target)
    # wrong dtypes and shapes
    for bad in (u8.long(), u8.float(), u8.to(torch.int8)):
        with pytest.raises(TypeError, match="uint8"):
            ua.ops.cc_label(bad)
        with pytest.raises(TypeError, match="uint8"):
            ua.ops.mask_cleanup(bad, 3)
        with pytest.raises(TypeError, match="uint8"):
            ua.ops.eval_confusion_classes(bad, target)
        with pytest.raises(TypeError, match="uint8"):
            ua.SegmentationMetrics().update_from_classes(bad, target)
    with pytest.raises(TypeError, match="uint8"):
        ua.ops.cc_label(np.zeros((1, 8, 8), dtype=np.uint8))
    with pytest.raises(TypeError, match="int64"):
        ua.ops.eval_confusion_classes(u8, target.int())
    for bad in (u8[0], u8[None], torch.zeros(1, 0, 8, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="B, H, W"):
            ua.ops.cc_label(bad)
        with pytest.raises(ValueError, match="B, H, W"):
            ua.ops.mask_cleanup(bad, 3)
    for K in (1, 33):
        with pytest.raises(ValueError, match="32"):
            ua.ops.mask_cleanup(u8, K)
        with pytest.raises(ValueError, match="32"):
            ua.ops.cc_label(u8, num_classes=K)
    with pytest.raises(ValueError, match="mode"):
        ua.ops.cc_label(u8, mode="holes")
    with pytest.raises(ValueError, match="connectivity"):
        ua.ops.cc_label(u8, connectivity=6)
    with pytest.raises(ValueError, match="vote"):
        ua.ops.mask_cleanup(u8, 3, vote="pixel")
    with pytest.raises(ValueError, match="connectivity"):
        ua.ops.mask_cleanup(u8, 3, connectivity=5)
    with pytest.raises(ValueError, match=">= 0"):
        ua.ops.mask_cleanup(u8, 3, min_area=-1)


def test_mask_cleanup_settings_are_validated_without_a_device(ua):
    pp = ua.MaskCleanup()
    assert pp.settings() == dict(vote=None, keep_largest=False, min_area=0, fill_holes=False,
                                 max_hole_area=0, connectivity=8)
    assert ua.MaskCleanup.pet().settings() == dict(vote="image", keep_largest=True, min_area=0,
                                                   fill_holes=True, max_hole_area=0,
                                                   connectivity=8)
    assert "keep_largest=True" in repr(ua.MaskCleanup.pet())
    for kw, err in ((dict(vote="pixel"), ValueError), (dict(vote=1), ValueError),
                    (dict(connectivity=6), ValueError), (dict(connectivity="8"), ValueError),
                    (dict(min_area=-1), ValueError), (dict(max_hole_area=-5), ValueError),
                    (dict(min_area=2.5), TypeError), (dict(max_hole_area="9"), TypeError),
                    (dict(min_area=True), TypeError), (dict(min_area=(1 << 30) + 1), ValueError)):
        with pytest.raises(err):
            ua.MaskCleanup(**kw)


def test_postprocess_with_pictures_is_refused_and_only_a_mask_cleanup_is_taken(ua):
    model = ua.UNet()
    with pytest.raises(ValueError, match="drawn from the logits"):
        ua.evaluate.evaluate_model(model, [], "cpu", visualize_samples=1, output_dir="unused",
                                   postprocess=ua.MaskCleanup.pet())
    with pytest.raises(TypeError, match="MaskCleanup"):
        ua.evaluate.evaluate_model(model, [], "cpu", postprocess=lambda x, k: x)
    with pytest.raises(TypeError, match="MaskCleanup"):
        ua.predict_masks(model, torch.zeros(1, 3, 64, 64), postprocess="pet")
    # an empty loader with a cleanup: the loop body never runs, the result is the empty one
    res = ua.evaluate.evaluate_model(model, [], "cpu", postprocess=ua.MaskCleanup.pet())
    assert res["confusion_matrix"].tolist() == [[0] * 3] * 3


def test_old_positional_calls_still_bind_and_the_new_parameter_is_keyword_only_and_last(ua):
    for fn, old in ((ua.predict_masks, ["model", "images", "original_dims"]),
                    (ua.evaluate.evaluate_model,
                     ["model", "test_loader", "device", "visualize_samples", "output_dir"]),
                    (ua.metrics.accumulate_test_metrics,
                     ["model", "data_loader", "device", "ignore_index", "on_batch",
                      "num_classes"])):
        params = list(inspect.signature(fn).parameters.values())
        assert [p.name for p in params[:-1]] == old, fn.__name__
        assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in params[:-1])
        last = params[-1]
        assert last.name == "postprocess" and last.kind is inspect.Parameter.KEYWORD_ONLY
        assert last.default is None
        inspect.signature(fn).bind(*range(len(old)))
    call = inspect.signature(ua.MaskCleanup.__call__)
    assert list(call.parameters)[:3] == ["self", "classes_u8", "num_classes"]
    m = inspect.signature(ua.SegmentationMetrics.update_from_classes)
    assert list(m.parameters) == ["self", "preds_u8", "target", "original_dims"]
    assert m.parameters["original_dims"].default is None


# ------------------------------------------------------------------- the reference against scipy
def _rank(labels):
    """Distinct non-zero labels replaced by their rank 1, 2, ... in increasing order."""
    u = np.unique(labels[labels != 0])
    lut = np.zeros(int(labels.max()) + 1, dtype=np.int64)
    lut[u] = np.arange(1, len(u) + 1)
    return lut[labels]


def test_reference_equals_scipy_on_random_masks():
    ndi = pytest.importorskip("scipy.ndimage")
    cross, full = ndi.generate_binary_structure(2, 1), np.ones((3, 3), dtype=bool)
    rng = np.random.RandomState(20240)
    n = 0
    for density in (0.3, 0.45, 0.6, 0.8):
        for _ in range(12):
            H, W = int(rng.randint(1, 41)), int(rng.randint(1, 41))
            mask = (rng.rand(H, W) < density).astype(np.uint8)
            classes = mask * rng.randint(1, 3, (H, W)).astype(np.uint8)
            for connectivity, own, dual in ((4, cross, full), (8, full, cross)):
                labels, areas = R.cc(classes, connectivity, "foreground", 3)
                want, count = ndi.label(mask, structure=own)
                assert np.array_equal(_rank(labels), want)
                assert np.array_equal(areas[areas != 0],
                                      np.bincount(want.reshape(-1))[1:count + 1])
                inverse, _ = R.cc(classes, connectivity, "background", 3)
                assert np.array_equal(_rank(inverse), ndi.label(mask == 0, structure=own)[0])
                # holes are background components under the DUAL connectivity
                filled = R.cleanup(classes, 3, fill_holes=True, connectivity=connectivity)
                assert np.array_equal(filled != 0, ndi.binary_fill_holes(mask, structure=dual))
                assert np.array_equal(filled[mask != 0], classes[mask != 0])
                # ... and the other pairing is a different function on some of these masks
                n += int(not np.array_equal(filled != 0,
                                            ndi.binary_fill_holes(mask, structure=own)))
            per_class, _ = R.cc(classes, 8, "class", 3)
            for c in (1, 2):
                assert np.array_equal(_rank(np.where(classes == c, per_class, 0)),
                                      ndi.label(classes == c, structure=full)[0])
    assert n > 0


# ---------------------------------------------------------------------------- hand-written cases
def _a(rows):
    return np.array([[int(ch) for ch in r] for r in rows], dtype=np.uint8)


def test_a_hole_takes_the_rings_class_and_not_the_islands():
    ring = _a(["0000000",
               "0222220",
               "0200020",
               "0201020",
               "0200020",
               "0222220",
               "0000000"])
    want = _a(["0000000",
               "0222220",
               "0222220",
               "0221220",
               "0222220",
               "0222220",
               "0000000"])
    assert np.array_equal(R.cleanup(ring, 3, fill_holes=True), want)
    assert np.array_equal(R.cleanup(ring, 3, fill_holes=True, connectivity=4), want)
    # the hole has 8 pixels
    assert np.array_equal(R.cleanup(ring, 3, fill_holes=True, max_hole_area=7), ring)
    assert np.array_equal(R.cleanup(ring, 3, fill_holes=True, max_hole_area=8), want)


def test_a_hole_open_to_the_edge_is_not_filled():
    m = _a(["11111",
            "10001",
            "10001",
            "11011"])
    assert np.array_equal(R.cleanup(m, 3, fill_holes=True), m)
    closed = m.copy()
    closed[3, 2] = 2
    want = np.where(closed == 0, 1, closed)
    assert np.array_equal(R.cleanup(closed, 3, fill_holes=True), want)
    # through a diagonal gap the background leaks only when the BACKGROUND is 8-connected,
    # i.e. when the foreground uses 4
    gap = _a(["01111",
              "10001",
              "10001",
              "11111"])
    assert np.array_equal(R.cleanup(gap, 3, fill_holes=True, connectivity=4), gap)
    assert np.array_equal(R.cleanup(gap, 3, fill_holes=True, connectivity=8) != 0,
                          _a(["01111", "11111", "11111", "11111"]) != 0)


def test_diagonal_contact_joins_under_8_and_not_under_4():
    m = _a(["100",
            "010",
            "002"])
    l8, a8 = R.cc(m, 8, "foreground", 3)
    assert l8.tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 1]] and a8[0, 0] == 3 and a8.sum() == 3
    l4, a4 = R.cc(m, 4, "foreground", 3)
    assert l4.tolist() == [[1, 0, 0], [0, 5, 0], [0, 0, 9]]
    assert a4.tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    lc, _ = R.cc(m, 8, "class", 3)
    assert lc.tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 9]]
    lb, ab = R.cc(m, 4, "background", 3)
    assert lb.tolist() == [[0, 2, 2], [4, 0, 2], [4, 4, 0]] and ab[0, 1] == 3 and ab[1, 0] == 3
    assert np.unique(R.cc(m, 8, "background", 3)[0]).tolist() == [0, 2]


def test_keep_largest_tie_goes_to_the_first_component():
    m = _a(["1100022",
            "1100022",
            "0000000",
            "0011000"])
    want = np.zeros_like(m)
    want[:2, :2] = 1
    assert np.array_equal(R.cleanup(m, 3, keep_largest=True), want)
    # the largest is chosen among all components: below min_area the image ends up empty
    assert not R.cleanup(m, 3, keep_largest=True, min_area=5).any()
    assert np.array_equal(R.cleanup(m, 3, keep_largest=True, min_area=4), want)


def test_vote_ties_go_to_the_lower_class():
    m = _a(["1122",
            "0000",
            "2210"])
    assert np.array_equal(R.cleanup(m, 3, vote="component"),
                          _a(["1111", "0000", "2220"]))
    # 3 pixels of class 1, 4 of class 2 in the image; one more 1 makes the tie
    assert np.array_equal(R.cleanup(m, 3, vote="image"), _a(["2222", "0000", "2220"]))
    m[2, 3] = 1
    assert np.array_equal(R.cleanup(m, 3, vote="image"), _a(["1111", "0000", "1111"]))
    empty = np.zeros((3, 4), dtype=np.uint8)
    assert np.array_equal(R.cleanup(empty, 3, vote="image"), empty)
    # the vote counts survivors only: with the two-pixel island of 1s gone, class 2 leads 2 : 1
    assert np.array_equal(R.cleanup(_a(["122", "000", "110"]), 3, vote="image"),
                          _a(["111", "000", "110"]))
    assert np.array_equal(R.cleanup(_a(["122", "000", "110"]), 3, vote="image", min_area=3),
                          _a(["222", "000", "000"]))


def test_min_area_larger_than_everything_gives_an_empty_image():
    m = _a(["1100022",
            "1100022",
            "0000000",
            "0011000"])
    assert not R.cleanup(m, 3, min_area=5).any()
    assert np.array_equal(R.cleanup(m, 3, min_area=4), np.where(_a(["1100011"] * 2 + ["0" * 7] * 2)
                                                                 != 0, m, 0))
    assert np.array_equal(R.cleanup(m, 3, min_area=1), m)


def test_all_off_is_the_identity_and_a_byte_past_k_reads_as_0():
    rng = np.random.RandomState(3)
    m = rng.randint(0, 3, (2, 9, 11)).astype(np.uint8)
    assert np.array_equal(R.cleanup(m, 3), m)
    big = m.copy()
    big[0, 4, 4:7] = (3, 200, 255)
    want = big.copy()
    want[0, 4, 4:7] = 0
    assert np.array_equal(R.cleanup(big, 3), want)
    assert np.array_equal(R.cc(big, 8, "foreground", 3)[0], R.cc(want, 8, "foreground", 3)[0])
    assert np.array_equal(R.cc(big, 8, "background", 3)[1], R.cc(want, 8, "background", 3)[1])
    # K = 21: 20 is a class, 21 is not
    k21 = np.array([[20, 21]], dtype=np.uint8)
    assert R.cleanup(k21, 21).tolist() == [[20, 0]]


def test_confusion_at_original_size_is_the_gather_it_says(ua):
    rng = np.random.RandomState(5)
    preds = rng.randint(0, 4, (2, 6, 9)).astype(np.uint8)
    target = rng.randint(0, 3, (2, 6, 9)).astype(np.int64)
    target[0, 0, :3] = 255
    cm = R.confusion_at_original_size(preds, target, None, 3)
    assert cm.sum() == 2 * 54 - 3 and cm.shape == (2, 3, 3)
    assert cm[1, 2, 0] == ((target[1] == 2) & ((preds[1] == 0) | (preds[1] == 3))).sum()
    twice = R.confusion_at_original_size(preds, target, [(12, 18), (12, 18)], 3)
    assert np.array_equal(twice, 4 * cm)            # an exact 2x up-size shows every pixel 4 times


def test_spiral_and_speckled_blob_are_what_the_gpu_tests_assume():
    s = R.spiral(64, 48)
    labels, areas = R.cc(s, 4, "foreground", 3)
    assert np.array_equal(labels, s.astype(np.uint32)) and areas[0, 0] == s.sum()
    assert len(np.unique(R.cc(s, 4, "background", 3)[0])) == 2
    assert s[0].all() and s[:, -1].all() and not s[1, :-2].any()
    noisy, clean = R.speckled_blob(96, 160, seed=1)
    assert set(np.unique(noisy)) == {0, 1, 2} and set(np.unique(clean)) == {0, 2}
    assert np.array_equal(R.cleanup(noisy, 3, vote="image", keep_largest=True, fill_holes=True),
                          clean)
    holes = R.cc(np.where(clean != 0, noisy, 1), 4, "background", 3)[1]
    assert sorted(holes[holes != 0].tolist()) == [1, 9, 10]
