#!/usr/bin/env python3
"""Mask post-processing on one MI355X at 8 x 512^2, K = 3: device-event times over N repetitions
after warm-up, in one process.

Three inputs: (a) speckled blobs with pinholes and stray islands, which stand for a real
prediction; (b) the one-pixel spiral, the longest path the bounded loops meet; (c) noise at 0.5.
Per input: `unet_cc_label_u8` alone (both connectivities, foreground and background), the switches
of the cleanup one at a time, `MaskCleanup.pet()`, and `unet_eval_confusion_classes` beside the two
logits kernels.  Beside them: the byte floor of each call at the project's 6.29 TB/s copy rate
((1 + 1) B/pixel for the map in and out plus 4 B for every pass over a label-sized plane the call
makes), the eval-mode forward of the same batch, the `evaluate_model` loop per batch with
postprocess=None and with pet(), and the host route a user takes today (`preds.cpu()` plus
scipy.ndimage.label / binary_fill_holes per image) where scipy imports.

Per-kernel times come from kernel traces of this same program, one run per input started by the
caller (`--kernels-only --input NAME` under the profiler); `--merge --input NAME --kernel-stats
FILE --out JSON` then adds the trace's *_kernel_stats.csv to the result without touching a device.

    python tools/bench_postprocess.py 50 [--out profiles/postprocess_bench.json]
"""
import argparse
import csv
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import unet_implementations_amd as ua  # noqa: E402

_spec = importlib.util.spec_from_file_location(
    "postprocess_ref", os.path.join(ROOT, "tests", "tools", "postprocess_ref.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

DEV = torch.device("cuda", 0)
B, HW, K = 8, 512, 3
COPY_RATE = 6.29e12            # bytes/s, the project's measured copy rate
PET_DIMS = [(500, 375), (333, 500), (375, 500), (500, 333), (225, 300), (400, 600), (358, 500),
            (500, 500)]
# passes over a 4-byte plane of B * H * W words that a call makes (reads and writes counted
# alike): zero areas, tile writes parents, finish reads parents + writes parents, labels and
# touches areas -> 6 for one labelling (the merge touches seams only); the byte rewrites read
# labels and areas where they need them
PLANE_PASSES = {"cc_label": 6, "keep_largest": 6 + 1 + 2, "min_area": 6 + 2, "vote_image": 0,
                "vote_component": 6 + 2 + (K - 1) * 3 + 2, "fill_holes": 6 + 2,
                "pet": 6 + 1 + 2 + 6 + 2}
MAP_PASSES = {"cc_label": 1, "keep_largest": 2 + 2 + 2, "min_area": 2 + 2 + 2,
              "vote_image": 2 + 1 + 2, "vote_component": 2 + 2 + (K - 1) + 2,
              "fill_holes": 2 + 2 + 2, "pet": 2 + 2 + 2 + 1 + 2 + 2 + 2}


def floor_us(kind):
    px = B * HW * HW
    return 1e6 * px * (MAP_PASSES[kind] + 4 * PLANE_PASSES[kind]) / COPY_RATE


def event_us(fn, n, warmup=5):
    """median over 5 groups of the mean device time of n back-to-back calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    groups = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        groups.append(1e3 * e0.elapsed_time(e1) / n)
    return statistics.median(groups), [min(groups), max(groups)]


def wall_ms(fn, reps=3):
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(times)


def inputs():
    blobs = np.stack([R.speckled_blob(HW, HW, seed=b)[0] for b in range(B)])
    s = R.spiral(HW, HW)
    spiral = np.stack([s if b % 2 == 0 else s[:, ::-1] for b in range(B)])
    noise = ((np.random.RandomState(0).rand(B, HW, HW) < 0.5) *
             np.random.RandomState(1).randint(1, K, (B, HW, HW))).astype(np.uint8)
    return {"blobs": blobs, "spiral": np.ascontiguousarray(spiral), "noise0.5": noise}


def host_route_ms(classes):
    """preds.cpu() + scipy per image: largest component, image vote, binary_fill_holes"""
    try:
        from scipy import ndimage as ndi
    except ImportError:
        return None
    full = np.ones((3, 3), dtype=bool)

    def run():
        maps = classes.cpu().numpy()
        out = np.zeros_like(maps)
        for b in range(len(maps)):
            lab, n = ndi.label(maps[b] != 0, structure=full)
            if n == 0:
                continue
            sizes = np.bincount(lab.reshape(-1))[1:]
            keep = lab == 1 + int(np.argmax(sizes))
            votes = np.bincount(maps[b][keep], minlength=K)[1:K]
            keep = ndi.binary_fill_holes(keep)
            out[b][keep] = 1 + int(np.argmax(votes))
        return out
    run()
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        run()
        t.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(t)


def merge_kernel_stats(path):
    """name -> {calls, avg_us} of the post-processing kernels in a *_kernel_stats.csv"""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row["Name"]
            if any(k in name for k in ("cc_tile", "cc_merge", "cc_finish", "cleanup_", "pp_zero",
                                       "eval_confusion")):
                short = name.split("::")[-1].split("(")[0]
                out[short] = {"calls": int(row["Calls"]),
                              "avg_us": float(row["AverageNs"]) / 1e3,
                              "min_us": float(row["MinNs"]) / 1e3,
                              "max_us": float(row["MaxNs"]) / 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int, nargs="?", default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--kernels-only", action="store_true",
                    help="run only the device calls (what a kernel trace should see)")
    ap.add_argument("--input", default=None, help="only this input (blobs, spiral, noise0.5)")
    ap.add_argument("--merge", action="store_true",
                    help="no device work: add --kernel-stats under --input to the JSON at --out")
    args = ap.parse_args()
    if args.merge:
        with open(args.out) as f:
            result = json.load(f)
        result["inputs"][args.input]["kernels"] = merge_kernel_stats(args.kernel_stats)
        with open(args.out, "w") as f:
            f.write(json.dumps(result) + "\n")
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_postprocess.py needs an MI355X (no CPU fallback exists)")
    n = args.n
    result = {"shape": [B, HW, HW], "K": K, "n": n, "device": torch.cuda.get_device_name(0),
              "copy_rate_TBps": COPY_RATE / 1e12,
              "floor_us": {k: floor_us(k) for k in PLANE_PASSES}, "inputs": {}}
    pet = ua.MaskCleanup.pet()
    g = torch.Generator().manual_seed(0)
    target = torch.randint(0, K, (B, HW, HW), generator=g).to(DEV)
    dims = torch.tensor(PET_DIMS[:B], dtype=torch.int64, device=DEV)
    for name, host in inputs().items():
        if args.input not in (None, name):
            continue
        classes = torch.from_numpy(host).to(DEV)
        ws = ua.ops.mask_cleanup_workspace(classes, K)
        out = torch.empty_like(classes)
        r = {}
        for conn in (4, 8):
            for mode in ("foreground", "background"):
                us, spread = event_us(lambda: ua.ops.cc_label(classes, conn, mode, K,
                                                              workspace=ws), n)
                r[f"cc_label_{mode}_{conn}_us"] = us
                r[f"cc_label_{mode}_{conn}_spread_us"] = spread
        ua.ops.cc_label(classes, 8, "foreground", K, check=True)
        for key, kw in (("keep_largest", dict(keep_largest=True)), ("min_area", dict(min_area=5)),
                        ("vote_image", dict(vote="image")),
                        ("vote_component", dict(vote="component")),
                        ("fill_holes", dict(fill_holes=True)), ("pet", pet.settings())):
            us, spread = event_us(lambda: ua.ops.mask_cleanup(classes, K, out=out, workspace=ws,
                                                              **kw), n)
            r[f"cleanup_{key}_us"] = us
            r[f"cleanup_{key}_spread_us"] = spread
        ua.ops.mask_cleanup(classes, K, out=out, workspace=ws, check=True, **pet.settings())
        onehot = torch.nn.functional.one_hot(classes.long(), K).permute(0, 3, 1, 2).float() \
            .contiguous()
        r["eval_confusion_classes_us"] = event_us(
            lambda: ua.ops.eval_confusion_classes(classes, target, dims, K), n)[0]
        r["eval_confusion_us"] = event_us(lambda: ua.ops.eval_confusion(onehot, target, dims), n)[0]
        lib, st = ua.lib(), torch.cuda.current_stream().cuda_stream
        cm = torch.empty((B, K, K), dtype=torch.int64, device=DEV)
        r["eval_confusionk_us"] = event_us(lambda: lib.unet_eval_confusionk(
            onehot.data_ptr(), target.data_ptr(), dims.data_ptr(), cm.data_ptr(), B, K, HW, HW, 255,
            st), n)[0]
        if not args.kernels_only:
            r["host_route_scipy_ms"] = host_route_ms(classes)
        result["inputs"][name] = r

    if not args.kernels_only:
        model = ua.create_model(DEV).eval()
        images = torch.randn(B, 3, HW, HW, generator=g)
        loader = [{"image": images, "mask": target.cpu(), "original_dims": dims.cpu()}] * 8
        dev_images = images.to(DEV)

        def forward():
            with torch.no_grad():
                model(dev_images)
        result["forward_us"] = event_us(forward, max(4, n // 5))[0]
        plain, cleaned = [], []
        for _ in range(2):
            ua.evaluate.evaluate_model(model, loader, DEV)
            ua.evaluate.evaluate_model(model, loader, DEV, postprocess=pet)
        for _ in range(5):               # alternate the two forms
            plain.append(wall_ms(lambda: ua.evaluate.evaluate_model(model, loader, DEV), 1))
            cleaned.append(wall_ms(lambda: ua.evaluate.evaluate_model(model, loader, DEV,
                                                                      postprocess=pet), 1))
        result["evaluate_model_ms_per_batch"] = {
            "postprocess_none": statistics.median(plain) / len(loader),
            "postprocess_pet": statistics.median(cleaned) / len(loader),
            "none_spread": [min(plain) / len(loader), max(plain) / len(loader)],
            "pet_spread": [min(cleaned) / len(loader), max(cleaned) / len(loader)]}
        if result["inputs"]["blobs"].get("host_route_scipy_ms") is None:
            result["host_route"] = "scipy.ndimage does not import here: omitted"
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
