#!/usr/bin/env python3
"""Test-set evaluation loop on one MI355X: images/s at 512^2 with pet-like original sizes.

Two forms of the loop of Our_UNet/src/evaluate.py:150-268 over the same batches, timed in
alternation:
  (a) what a user of the package wrote before `evaluate_model` existed: `ua.UNet` forward, then
      the reference's per-image tail restated with torch / numpy - argmax, F.interpolate(nearest)
      of prediction and mask to the original size, both copied to the host, and the per-class
      numpy passes of SegmentationMetrics._update_single;
  (b) `ua.evaluate.evaluate_model`: forward, then one `unet_eval_confusion` launch per batch.
Also the forward alone, and the two kernels alone (time and algorithmic bytes/s: logits and
targets read once, plus what `unet_eval_maps` writes).  Prints one JSON line.

    python tools/bench_eval.py [--batches 32] [--reps 5] [--warmup 2] [--hw 512]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import unet_implementations_amd as ua  # noqa: E402

DEV = torch.device("cuda", 0)
# (orig_h, orig_w) as they occur in the Oxford-IIIT Pet test split
PET_DIMS = [(500, 375), (333, 500), (375, 500), (500, 333), (225, 300), (400, 600), (358, 500),
            (500, 500)]


def make_loader(batches, batch, hw, seed=0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(batches):
        images = torch.randn(batch, 3, hw, hw, generator=g)
        blocks = torch.randint(0, 3, (batch, 1, hw // 32, hw // 32), generator=g).float()
        masks = F.interpolate(blocks, size=(hw, hw), mode="nearest")[:, 0].long()
        masks[:, hw // 2 - 2: hw // 2 + 2] = 255
        dims = torch.tensor([PET_DIMS[(i * batch + j) % len(PET_DIMS)] for j in range(batch)],
                            dtype=torch.int64)
        out.append({"image": images, "mask": masks, "original_dims": dims})
    return out


def host_tail_loop(model, loader):
    """Form (a): accumulators as numpy arrays, one image at a time."""
    inter, union = np.zeros(3), np.zeros(3)
    tp, fp, fn = np.zeros(3), np.zeros(3), np.zeros(3)
    total = correct = 0
    model.eval()
    with torch.no_grad():
        for batch in loader:
            images, masks = batch["image"].to(DEV), batch["mask"].to(DEV)
            preds = torch.argmax(model(images), dim=1)
            for j in range(preds.size(0)):
                oh, ow = batch["original_dims"][j]
                p = F.interpolate(preds[j][None, None].float(), size=(oh, ow),
                                  mode="nearest").squeeze().cpu().numpy().astype(np.uint8)
                t = F.interpolate(masks[j][None, None].float(), size=(oh, ow),
                                  mode="nearest").squeeze().cpu().numpy().astype(np.uint8)
                valid = t != 255
                total += valid.sum()
                correct += ((p == t) & valid).sum()
                for c in range(3):
                    pc, tc = (p == c) & valid, (t == c) & valid
                    i = (pc & tc).sum()
                    inter[c] += i
                    union[c] += pc.sum() + tc.sum() - i
                    tp[c] += i
                    fp[c] += pc.sum() - i
                    fn[c] += tc.sum() - i
    return {"pixel_accuracy": float(correct / total), "inter": inter, "union": union}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def kernel_ms(fn, steps=50, reps=5):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / steps)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--hw", type=int, default=512)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval.py needs an MI355X (no CPU fallback exists)")
    model = ua.create_model(DEV).eval()
    result = {"hw": args.hw, "batches": args.batches, "device": torch.cuda.get_device_name(0)}
    for batch in (4, 8):
        loader = make_loader(args.batches, batch, args.hw)
        n_img = args.batches * batch

        def form_a():
            return host_tail_loop(model, loader)

        def form_b():
            return ua.evaluate.evaluate_model(model, loader, DEV)

        def forward_only():
            with torch.no_grad():
                for b in loader:
                    model(b["image"].to(DEV))
                    b["mask"].to(DEV)

        for _ in range(args.warmup):
            ra, rb = form_a(), form_b()
            forward_only()
        assert ra["pixel_accuracy"] == rb["pixel_accuracy"], (ra["pixel_accuracy"], rb["pixel_accuracy"])
        ta, tb, tf = [], [], []
        for _ in range(args.reps):          # alternate the forms: other work shares the host
            ta.append(wall(form_a)[0])
            tb.append(wall(form_b)[0])
            tf.append(wall(forward_only)[0])
        a, b_, f = (statistics.median(t) for t in (ta, tb, tf))
        # the kernels alone, on one batch
        with torch.no_grad():
            logits = model(loader[0]["image"].to(DEV)).float().contiguous()
        masks, dims = loader[0]["mask"].to(DEV), loader[0]["original_dims"].to(DEV)
        px = batch * args.hw * args.hw
        k_cm = kernel_ms(lambda: ua.ops.eval_confusion(logits, masks, dims))
        k_cm0 = kernel_ms(lambda: ua.ops.eval_confusion(logits, masks))
        k_old = kernel_ms(lambda: ua.ops.argmax_dice_counts(logits, masks, want_preds=False))
        k_maps = kernel_ms(lambda: ua.ops.eval_maps(logits, masks))
        result[f"batch{batch}"] = {
            "images": n_img,
            "a_host_tail_img_per_s": n_img / a, "b_evaluate_model_img_per_s": n_img / b_,
            "forward_only_img_per_s": n_img / f, "b_over_a": a / b_,
            "a_ms_per_batch": 1e3 * a / args.batches, "b_ms_per_batch": 1e3 * b_ / args.batches,
            "forward_ms_per_batch": 1e3 * f / args.batches,
            "a_spread_s": [min(ta), max(ta)], "b_spread_s": [min(tb), max(tb)],
            "eval_confusion_ms": k_cm, "eval_confusion_GBps": px * 20 / k_cm / 1e6,
            "eval_confusion_no_dims_ms": k_cm0, "argmax_dice_counts_ms": k_old,
            "eval_maps_all_outputs_ms": k_maps, "eval_maps_GBps": px * (20 + 12 + 2) / k_maps / 1e6,
        }
    print(json.dumps(result))


if __name__ == "__main__":
    main()
