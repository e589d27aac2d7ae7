"""CPU (-m "not gpu"): test-set evaluation without a device - the ABI surface of
unet_eval_confusion / unet_eval_maps and their host-side argument checks, the nearest-resize index
rule against F.interpolate, the fixture's bit-stable inputs, and `SegmentationMetrics` fed the
reference's per-image confusion matrices (tests/golden/eval.npz, recorded from the reference's own
evaluate_model_metrics by tests/tools/make_golden_eval.py) through its host-only path."""
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


E = _load("eval_inputs")
ENTRY_POINTS = ("unet_eval_confusion", "unet_eval_maps")


def test_entry_points_declared_exported_and_bound(ua):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    handle = ctypes.CDLL(ua.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), f"{name} not declared in unet_hip.h"
        assert hasattr(handle, name), f"{name} not exported"
        assert name in ua._lib.SIGNATURES
    assert len(ua._lib.SIGNATURES["unet_eval_confusion"][1]) == 9
    assert len(ua._lib.SIGNATURES["unet_eval_maps"][1]) == 9
    for name in ("eval_confusion", "eval_maps"):
        assert callable(getattr(ua.ops, name))
    for name in ("load_model", "evaluate_model", "confidence_maps", "error_maps"):
        assert callable(getattr(ua.evaluate, name))
    for name in ("compute_dice", "compute_iou", "compute_pixel_accuracy", "evaluate_model_metrics"):
        assert callable(getattr(ua, name))


def test_host_arguments_are_rejected_before_any_launch(ua):
    lib = ua.lib()
    rc = lib.unet_eval_confusion(None, 1, None, 1, 1, 8, 8, 255, None)
    assert rc == -1 and b"null" in lib.unet_last_error()
    rc = lib.unet_eval_confusion(1, 1, None, None, 1, 8, 8, 255, None)
    assert rc == -1 and b"null" in lib.unet_last_error()
    rc = lib.unet_eval_confusion(1, 1, None, 1, 1, 0, 8, 255, None)
    assert rc == -1 and b"bad shape" in lib.unet_last_error()
    rc = lib.unet_eval_confusion(1, 1, None, 1, 0, 8, 8, 255, None)
    assert rc == -1 and b"bad shape" in lib.unet_last_error()
    for bad in (0, 1, 2):
        rc = lib.unet_eval_confusion(1, 1, None, 1, 1, 8, 8, bad, None)
        assert rc == -1 and b"ignore_index" in lib.unet_last_error()
    rc = lib.unet_eval_maps(None, None, 1, None, None, 1, 8, 8, None)
    assert rc == -1 and b"null" in lib.unet_last_error()
    rc = lib.unet_eval_maps(1, None, None, None, None, 1, 8, 8, None)
    assert rc == -1 and b"no output" in lib.unet_last_error()
    rc = lib.unet_eval_maps(1, None, None, None, 1, 1, 8, 8, None)
    assert rc == -1 and b"target" in lib.unet_last_error()
    rc = lib.unet_eval_maps(1, None, 1, None, None, 1, 8, 0, None)
    assert rc == -1 and b"bad shape" in lib.unet_last_error()


def test_python_surface_has_no_cpu_fallback(ua):
    z, t = torch.zeros(1, 3, 8, 8), torch.zeros(1, 8, 8, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ua.ops.eval_confusion(z, t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ua.ops.eval_maps(z, t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ua.SegmentationMetrics().update_from_logits(z, t, torch.tensor([[8, 8]]))
    with pytest.raises(NotImplementedError):
        ua.evaluate.evaluate_model(None, [], "cpu", visualize_samples=3)
    with pytest.raises(NotImplementedError):
        ua.evaluate_model_metrics(None, [], "cpu", num_classes=4)


@pytest.mark.parametrize("n_in", [64, 128, 512])
def test_index_rule_is_what_interpolate_nearest_reads(ua, n_in):
    """min(floor(fp32(d) * fp32(in / out)), in - 1) for every out in 1..1400, against
    F.interpolate(mode="nearest") of an index ramp; the integer rule d * in // out is not it."""
    ramp = torch.arange(n_in, dtype=torch.float32).view(1, 1, n_in)
    from unet_implementations_amd.train import nearest_source_index
    integer_rule_differs = []
    for n_out in range(1, 1401):
        want = F.interpolate(ramp, size=n_out, mode="nearest")[0, 0].long().numpy()
        got = E.nearest_index(n_in, n_out)
        assert np.array_equal(got, want), (n_in, n_out)
        assert np.array_equal(nearest_source_index(n_in, n_out), want), (n_in, n_out)
        if not np.array_equal(E.integer_rule_index(n_in, n_out), want):
            integer_rule_differs.append(n_out)
    assert integer_rule_differs[:4] == [82, 94, 110, 122], integer_rule_differs[:8]
    for pair_in, pair_out in E.DISCRIMINATING:
        if pair_in == n_in:
            assert pair_out in integer_rule_differs


def test_fixture_inputs_regenerate_bit_identically(golden):
    g = golden("eval")
    assert [str(c) for c in g["cases"]] == [c[0] for c in E.CASES]
    for name, seed, H, W, dims, classes in E.CASES:
        assert int(g[f"seed_{name}"]) == seed and list(g[f"size_{name}"]) == [H, W]
        assert np.array_equal(g[f"dims_{name}"], np.array(dims))
        logits, target = E.make_case(seed, len(dims), H, W, classes)
        assert np.array_equal(E.case_digest(logits, target), g[f"sha256_{name}"]), name
        # two- and three-way ties are present, and so is the ignore band
        if classes == 3:        # (the one-class case pushes planes 1 and 2 down by 100)
            assert ((logits[:, 0] == logits[:, 1]) & (logits[:, 1] > logits[:, 2])).any()
            assert ((logits[:, 0] == logits[:, 1]) & (logits[:, 1] == logits[:, 2])).any()
        assert (target == 255).any()
    assert not (E.make_case(101, 4, 64, 64)[1][0] == 2).any()       # image 0 lacks class 2


def test_weighted_count_form_equals_the_references_gather(golden):
    """The identity unet_eval_confusion rests on: counting source pixels with the weight
    (rows that map to y) x (columns that map to x) gives the confusion matrix of the resized
    maps - here against the matrices of the reference's own resized pairs."""
    g = golden("eval")
    for name, seed, H, W, dims, classes in E.CASES:
        logits, target = E.make_case(seed, len(dims), H, W, classes)
        pred = logits.argmax(axis=1)
        for b, (oh, ow) in enumerate(dims):
            wy = np.bincount(E.nearest_index(H, oh), minlength=H)
            wx = np.bincount(E.nearest_index(W, ow), minlength=W)
            w = (wy[:, None] * wx[None, :]).ravel()
            t, p = target[b].ravel(), pred[b].ravel()
            keep = t != 255
            cm = np.bincount(t[keep] * 3 + p[keep], weights=w[keep], minlength=9)
            assert np.array_equal(cm.reshape(3, 3).astype(np.int64), g[f"cm_{name}"][b]), (name, b)


def _accumulators(m):
    return np.concatenate([m.intersections, m.unions, m.true_positives, m.false_positives,
                           m.false_negatives, [m.total_pixels, m.correct_pixels]])


def _flat_metrics(res, keys):
    out = []
    for k in keys:
        v = res
        for part in str(k).split("/"):
            v = v["class_metrics"][part] if part.startswith("class_") else v[part]
        out.append(v)
    return np.array(out, dtype=np.float64)


def test_metrics_from_confusion_matrices_equal_the_reference_exactly(ua, golden):
    """Every accumulator after every image, and every value of get_all_metrics(), bit for bit
    (ratios of the same integers in float64), nan where the reference has nan."""
    g = golden("eval")
    keys = list(g["metric_keys"])
    assert len(keys) == 18
    saw_nan = False
    for name in [str(c) for c in g["cases"]] + ["all"]:
        m = ua.SegmentationMetrics(num_classes=3, ignore_index=255)
        for i, cm in enumerate(g[f"cm_{name}"]):
            m.update_from_confusion(torch.from_numpy(cm) if i % 2 else cm)
            assert np.array_equal(_accumulators(m), g[f"acc_{name}"][i]), (name, i)
        assert m.intersections.dtype == np.float64 and isinstance(m.total_pixels, int)
        assert np.array_equal(m.confusion_matrix, g[f"cm_{name}"].sum(axis=0))
        got, want = _flat_metrics(m.get_all_metrics(), keys), g[f"metrics_{name}"]
        assert np.array_equal(np.isnan(got), np.isnan(want)), name
        assert np.array_equal(got, want, equal_nan=True), (name, got - want)
        saw_nan |= bool(np.isnan(want).any())
        m.reset()
        assert not _accumulators(m).any() and not m.confusion_matrix.any()
    assert saw_nan
    # a batch of matrices in one call is the sum of its images
    m = ua.SegmentationMetrics()
    m.update_from_confusion(g["cm_b128"])
    assert np.array_equal(_accumulators(m), g["acc_b128"][-1])
