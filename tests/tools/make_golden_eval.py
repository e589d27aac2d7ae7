#!/usr/bin/env python3
"""Generates tests/golden/eval.npz by running the REFERENCE's test-set evaluation on CPU.

Runs only in the build container (needs the reference checkout).  Loads
`Our_UNet/utils/metrics.py` by file path (torch and numpy only) and calls its own
`evaluate_model_metrics` with a stub module that returns prepared logits and a list of batches
whose `original_dims` is an int64 [B, 2] tensor, as the default collate builds it.  The
reference's `SegmentationMetrics` is subclassed to record the accumulators after every image and
the confusion matrix of the resized pair it was handed.

Per case of eval_inputs.CASES the fixture holds: the seed, the network size, the dims, a SHA-256
of the regenerated inputs, the accumulators after every image (`acc_<case>`, float64 [n, 17] =
intersections, unions, true / false positives, false negatives (3 each), total_pixels,
correct_pixels), the per-image confusion matrices of the reference's resized maps
(`cm_<case>`, int64 [n, 3, 3]) and every value of `get_all_metrics()` (`metrics_<case>`, in the
order of METRIC_KEYS, nan kept).  `acc_all` / `cm_all` / `metrics_all` are one run over all cases
in order.  Data only: nothing from the reference's source travels.

Usage: python tests/tools/make_golden_eval.py [--out PATH] [--reference DIR]
"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import eval_inputs as E  # noqa: E402

METRIC_KEYS = ["pixel_accuracy", "mean_iou", "mean_dice"] + [
    f"class_{c}/{k}" for c in range(3) for k in ("iou", "dice", "precision", "recall", "f1_score")]


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def flatten_metrics(res):
    out = [res["pixel_accuracy"], res["mean_iou"], res["mean_dice"]]
    for c in range(3):
        m = res["class_metrics"][f"class_{c}"]
        out += [m[k] for k in ("iou", "dice", "precision", "recall", "f1_score")]
    return np.array(out, dtype=np.float64)


class Identity(torch.nn.Module):
    """The stub network: the batch's "image" already is the logits."""

    def forward(self, x):
        return x


def recording_class(M, log):
    class Recording(M.SegmentationMetrics):
        def update(self, pred, target):
            super().update(pred, target)
            acc = np.concatenate([self.intersections, self.unions, self.true_positives,
                                  self.false_positives, self.false_negatives,
                                  [self.total_pixels, self.correct_pixels]]).astype(np.float64)
            p, t = np.asarray(pred).astype(np.int64).ravel(), np.asarray(target).astype(np.int64).ravel()
            keep = t != self.ignore_index
            cm = np.bincount(t[keep] * 3 + p[keep], minlength=9).reshape(3, 3).astype(np.int64)
            log.append((acc, cm))
    return Recording


def run(M, batches, log):
    del log[:]
    res = M.evaluate_model_metrics(Identity(), batches, torch.device("cpu"))
    acc = np.stack([a for a, _ in log])
    cm = np.stack([c for _, c in log])
    # the recorded matrices are consistent with the reference's own accumulators
    d = np.diff(np.concatenate([np.zeros((1, 17)), acc]), axis=0)
    for i in range(len(cm)):
        assert np.array_equal(np.diagonal(cm[i]), d[i, 0:3])
        assert np.array_equal(cm[i].sum(axis=1), d[i, 6:9] + d[i, 12:15])     # TP + FN
        assert np.array_equal(cm[i].sum(axis=0), d[i, 6:9] + d[i, 9:12])      # TP + FP
    return acc, cm, flatten_metrics(res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "eval.npz"))
    ap.add_argument("--reference", default="/root/reference")
    args = ap.parse_args()
    M = _load("ref_unet_metrics", os.path.join(args.reference, "Our_UNet", "utils", "metrics.py"))
    log = []
    M.SegmentationMetrics = recording_class(M, log)
    torch.set_num_threads(1)

    # the chosen sizes discriminate ATen's fp32 rule from the integer rule, and the fp32
    # restatement is what F.interpolate does
    for n_in, n_out in E.DISCRIMINATING:
        assert (E.nearest_index(n_in, n_out) != E.integer_rule_index(n_in, n_out)).any(), (n_in, n_out)
    for name, seed, H, W, dims, classes in E.CASES:
        for oh, ow in dims:
            src = F.interpolate(torch.arange(H * W, dtype=torch.float32).view(1, 1, H, W),
                                size=(oh, ow), mode="nearest")[0, 0].long().numpy()
            want = E.nearest_index(H, oh)[:, None] * W + E.nearest_index(W, ow)[None, :]
            assert np.array_equal(src, want), (name, oh, ow)

    out = {"cases": np.array([c[0] for c in E.CASES]), "metric_keys": np.array(METRIC_KEYS)}
    all_batches = []
    for name, seed, H, W, dims, classes in E.CASES:
        logits, target = E.make_case(seed, len(dims), H, W, classes)
        batch = {"image": torch.from_numpy(logits), "mask": torch.from_numpy(target),
                 "original_dims": torch.tensor(dims, dtype=torch.int64)}
        all_batches.append(batch)
        acc, cm, metrics = run(M, [batch], log)
        # the weighted-count form the kernel implements equals the reference's gather
        pred = logits.argmax(axis=1)
        for b, d in enumerate(dims):
            assert np.array_equal(E.resized_confusion(pred[b], target[b], d), cm[b]), (name, b)
        out[f"seed_{name}"] = np.int64(seed)
        out[f"size_{name}"] = np.array([H, W], dtype=np.int64)
        out[f"dims_{name}"] = np.array(dims, dtype=np.int64)
        out[f"sha256_{name}"] = E.case_digest(logits, target)
        out[f"acc_{name}"], out[f"cm_{name}"], out[f"metrics_{name}"] = acc, cm, metrics
        print(f"  {name}: {len(dims)} images, pixel accuracy {metrics[0]:.6f}, "
              f"nan metrics {int(np.isnan(metrics).sum())}")
    out["acc_all"], out["cm_all"], out["metrics_all"] = run(M, all_batches, log)
    with open(args.out, "wb") as f:
        np.savez_compressed(f, **dict(sorted(out.items())))
    print(os.path.basename(args.out), "written,", os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
