#!/usr/bin/env python3
"""What the uint8 batch path buys per train step on one MI355X.

The dataset produces a uint8 [N,H,W,3] image and a uint8 [N,H,W] mask.  Two ways to feed a step
from pinned host memory, timed in alternation in one process:
  (a) "f32+i64": the fp32 NCHW image and the int64 mask the reference's loader makes on the host
      (25.2 MB + 16.8 MB at 8 x 512^2), `model(images)`, `SimpleLoss()`;
  (b) "u8+u8":   the dataset's own bytes (6.3 MB + 2.1 MB), `input_layout="nhwc_u8"`,
      `SimpleLoss(target_layout="u8")`.
For `matmul_precision` fp32 and bf16, each as the eager `train_step` and as `GraphedTrainStep`
replays; a timed step is host-to-device copy + step, ended by a device synchronise.  Also the
loss and metric kernels alone on either target type (device events).  Medians over `--rounds`
rounds of `--steps` steps behind `--warmup` untimed ones.  Prints a table and one JSON line.

    python tools/bench_u8_step.py [--batch 8] [--hw 512] [--steps 20] [--rounds 7] [--warmup 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import unet_implementations_amd as ua  # noqa: E402


def host_batches(k, n, hw, seed=0):
    """k batches in both forms, pinned: [(u8 image, u8 mask)], [(fp32 NCHW image, int64 mask)] -
    form (a) holds exactly what form (b) turns into on the device."""
    g = torch.Generator().manual_seed(seed)
    mean = torch.tensor(ua.ops.IMAGENET_MEAN).view(1, 3, 1, 1)
    std = torch.tensor(ua.ops.IMAGENET_STD).view(1, 3, 1, 1)
    u8, f32 = [], []
    for _ in range(k):
        img = torch.randint(0, 256, (n, hw, hw, 3), generator=g, dtype=torch.uint8)
        blocks = torch.randint(0, 3, (n, 1, hw // 32, hw // 32), generator=g).float()
        mask = torch.nn.functional.interpolate(blocks, size=(hw, hw), mode="nearest")[:, 0]
        mask = mask.to(torch.uint8)
        mask[:, hw // 2 - 2: hw // 2 + 2] = 255
        u8.append((img.pin_memory(), mask.pin_memory()))
        x = ((img.permute(0, 3, 1, 2).float() / 255.0) - mean) / std
        f32.append((x.contiguous().pin_memory(), mask.long().pin_memory()))
    return u8, f32


class Variant:
    """One way to feed the step: its own model, optimizer and loss (same initial weights)."""

    def __init__(self, name, mode, graphed, batches, dev, u8):
        torch.manual_seed(0)
        self.name, self.batches, self.dev = name, batches, dev
        self.model = ua.create_model(dev).train()
        self.model.matmul_precision = mode
        self.opt = ua.create_optimizer(self.model)
        self.lossf = ua.SimpleLoss(target_layout="u8") if u8 else ua.get_loss_function()
        self.layout = "nhwc_u8" if u8 else None
        self.k = 0
        self.graph = None
        if graphed:
            x, m = (t.to(dev) for t in batches[0])
            self.graph = ua.GraphedTrainStep(self.model, self.opt, self.lossf, x, m,
                                             input_layout=self.layout)

    def step(self):
        x, m = self.batches[self.k % len(self.batches)]
        self.k += 1
        if self.graph is not None:     # copies the pinned batch straight into its static buffers
            return self.graph(x, m)
        x = x.to(self.dev, non_blocking=True)
        m = m.to(self.dev, non_blocking=True)
        return ua.train_step(self.model, self.opt, self.lossf, x, m, input_layout=self.layout)

    def timed(self, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps


def bench_steps(mode, graphed, u8_b, f32_b, dev, args):
    a = Variant("f32+i64", mode, graphed, f32_b, dev, u8=False)
    b = Variant("u8+u8", mode, graphed, u8_b, dev, u8=True)
    for v in (a, b):
        v.timed(args.warmup)
    ms = {a.name: [], b.name: []}
    for _ in range(args.rounds):          # alternating: both see the same neighbours on the box
        for v in (a, b):
            ms[v.name].append(v.timed(args.steps))
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
            for k, v in ms.items()}


def event_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def bench_kernels(n, hw, dev, args):
    """The loss (reduce + finalize + gradient) and the validation counts alone, per target type."""
    g = torch.Generator().manual_seed(1)
    logits = (torch.randn(n, 3, hw, hw, generator=g) * 2).to(dev)
    t8 = torch.randint(0, 3, (n, hw, hw), generator=g).to(torch.uint8)
    t8[:, hw // 2 - 2: hw // 2 + 2] = 255
    targets = {"int64": t8.long().to(dev), "uint8": t8.to(dev)}
    ws = ua.ops.dice_wce_loss_workspace(logits)
    one = torch.ones((), device=dev)

    def loss(t):
        ua.ops.dice_wce_loss_fwd_bwd(logits, t, 1e-5, 1.0, 1.0, 255, True, want_grad=False, ws=ws)
        ua.ops.dice_wce_loss_grad(logits, t, ws, one, 255)

    def counts(t):
        ua.ops.argmax_dice_counts(logits, t, 255, want_preds=False)

    out = {}
    for name, fn in (("loss_fwd_and_grad", loss), ("argmax_dice_counts", counts)):
        ms = {k: [] for k in targets}
        for k, t in targets.items():
            event_ms(lambda: fn(t), 20)
        for _ in range(args.rounds):
            for k, t in targets.items():
                ms[k].append(event_ms(lambda: fn(t), 100))
        out[name] = {k: {"median_us": 1e3 * statistics.median(v), "min_us": 1e3 * min(v),
                         "max_us": 1e3 * max(v)} for k, v in ms.items()}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--hw", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20, help="timed steps per round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--modes", default="fp32,bf16")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_u8_step: no ROCm device (there is nothing to measure on a CPU)")
    dev = torch.device("cuda", 0)
    n, hw = args.batch, args.hw
    u8_b, f32_b = host_batches(4, n, hw)
    bytes_in = {"f32+i64": n * hw * hw * (3 * 4 + 8), "u8+u8": n * hw * hw * (3 + 1)}
    res = {"tool": "bench_u8_step", "device": torch.cuda.get_device_name(0), "batch": n, "hw": hw,
           "steps": args.steps, "rounds": args.rounds, "warmup": args.warmup,
           "host_bytes_per_step": bytes_in, "step_ms": {}}
    print(f"# {res['device']}  batch {n} x {hw}^2  {args.rounds} rounds x {args.steps} steps "
          f"(warm-up {args.warmup}); step = pinned H2D copy + train step + synchronise")
    print(f"# host bytes per step: f32+i64 {bytes_in['f32+i64'] / 1e6:.1f} MB, "
          f"u8+u8 {bytes_in['u8+u8'] / 1e6:.1f} MB")
    print(f"{'mode':6s} {'step':6s} {'input':8s} {'median ms':>10s} {'min':>8s} {'max':>8s}")
    for mode in args.modes.split(","):
        for graphed in (False, True):
            r = bench_steps(mode, graphed, u8_b, f32_b, dev, args)
            kind = "graph" if graphed else "eager"
            res["step_ms"][f"{mode}/{kind}"] = r
            for name, v in r.items():
                print(f"{mode:6s} {kind:6s} {name:8s} {v['median_ms']:10.3f} {v['min_ms']:8.3f} "
                      f"{v['max_ms']:8.3f}", flush=True)
            torch.cuda.empty_cache()
    res["kernels_us"] = bench_kernels(n, hw, dev, args)
    print(f"{'kernels alone':28s} {'target':6s} {'median us':>10s} {'min':>8s} {'max':>8s}")
    for name, r in res["kernels_us"].items():
        for k, v in r.items():
            print(f"{name:28s} {k:6s} {v['median_us']:10.1f} {v['min_us']:8.1f} {v['max_us']:8.1f}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
