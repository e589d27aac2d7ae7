#!/usr/bin/env python3
"""Grad-CAM on one MI355X: eight 512^2 images, targets decoder_stages[0] and decoder_stages[-1].

Two forms over the same images, in one process, timed in alternation:
  (a) the hook formulation: the reference's per-image algorithm (Our_UNet/utils/visualize.py:
      372-439) driven through stage-level hooks on `ua.UNet` in fp32 - eval forward, zero_grad,
      a full backward with every weight gradient, torch ops for the tail, `.cpu()` per image;
  (b) `ua.evaluate.gradcam` on the batch (gradient-only backward to the target, unet_gradcam_*),
      read back to the host once, as (a) is.
Also the two HBM-bound kernels alone on the decoder_stages[-1] tensors ([8, 512, 512, 32] fp32):
time and algorithmic bytes/s.  Prints one JSON line.

    python tools/bench_gradcam.py [--batch 8] [--hw 512] [--reps 5] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import unet_implementations_amd as ua  # noqa: E402

DEV = torch.device("cuda", 0)


def hook_heatmap(model, x, cls, target):
    """generate_gradcam_heatmap restated on a stage-level target (returns the numpy map)."""
    model.eval()
    keep = {}
    h1 = target.register_forward_hook(lambda m, i, o: keep.__setitem__("a", o.detach()))
    h2 = target.register_full_backward_hook(lambda m, gi, go: keep.__setitem__("g", go[0].detach()))
    out = model(x)
    score = out[0, cls].mean()
    model.zero_grad()
    score.backward()
    h1.remove()
    h2.remove()
    cam = F.relu(torch.sum(torch.mean(keep["g"], dim=(2, 3), keepdim=True) * keep["a"], dim=1))
    cam = cam - cam.min()
    if cam.max() != 0:
        cam = cam / cam.max()
    heat = F.interpolate(cam.unsqueeze(1), size=x.shape[2:], mode="bilinear", align_corners=False)
    return heat.squeeze().cpu().numpy()


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def kernel_ms(fn, steps=20, reps=5):
    for _ in range(3):
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
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--hw", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gradcam.py needs an MI355X (no CPU fallback exists)")
    torch.manual_seed(0)
    model = ua.create_model(DEV).eval()
    x = torch.randn(args.batch, 3, args.hw, args.hw, device=DEV)
    cls = 1
    result = {"hw": args.hw, "batch": args.batch, "device": torch.cuda.get_device_name(0)}
    for key, target in (("decoder_stages[0]", model.decoder_stages[0]),
                        ("decoder_stages[-1]", model.decoder_stages[-1])):
        def form_a():
            return [hook_heatmap(model, x[b:b + 1], cls, target) for b in range(args.batch)]

        def form_b():
            return ua.evaluate.gradcam(model, x, cls, target).cpu().numpy()

        for _ in range(args.warmup):
            ra, rb = form_a(), form_b()
        diff = max(float(abs(a - b).max()) for a, b in zip(ra, rb))
        ta, tb = [], []
        for _ in range(args.reps):          # alternate the forms: other work shares the host
            ta.append(wall(form_a)[0])
            tb.append(wall(form_b)[0])
        a, b_ = statistics.median(ta), statistics.median(tb)
        result[key] = {"a_hook_loop_ms": 1e3 * a, "b_gradcam_ms": 1e3 * b_, "a_over_b": a / b_,
                       "a_spread_ms": [1e3 * min(ta), 1e3 * max(ta)],
                       "b_spread_ms": [1e3 * min(tb), 1e3 * max(tb)],
                       "max_abs_difference_a_b": diff}
    # the two single-pass kernels on the largest tensors (decoder_stages[-1] / encoder_stages[0])
    N, HW, C = args.batch, args.hw * args.hw, 32
    g = torch.randn(N, args.hw, args.hw, C, device=DEV)
    y = torch.randn(N, args.hw, args.hw, C, device=DEV)
    act = ua.ops.Act(y, torch.rand(N, C, device=DEV) + 0.5, torch.randn(N, C, device=DEV))
    w = ua.ops.gradcam_weights(g)
    ws = ua.ops.gradcam_workspace(N, HW, C, g)
    k_w = kernel_ms(lambda: ua.ops.gradcam_weights(g, ws))
    k_m = kernel_ms(lambda: ua.ops.gradcam_map(act, 0.01, w, ws))
    cam, _ = ua.ops.gradcam_map(act, 0.01, w, ws)
    k_h = kernel_ms(lambda: ua.ops.gradcam_heatmap(cam, ws, (args.hw, args.hw)))
    result["kernels"] = {
        "tensor_MB": 4e-6 * N * HW * C,
        "gradcam_weights_ms": k_w, "gradcam_weights_GBps": 4.0 * N * HW * C / k_w / 1e6,
        "gradcam_map_ms": k_m, "gradcam_map_GBps": 4.0 * N * HW * (C + 1) / k_m / 1e6,
        "gradcam_heatmap_ms": k_h}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
