#!/usr/bin/env python3
"""What online augmentation costs on one MI355X, at the flagship batch (8 x 512^2 by default).

  1. `unet_augment_u8` alone: device events around `--calls` calls behind a warm-up, median of
     `--rounds`, for the identity record and for a full record (perspective, colour, gray, hole,
     Gaussian noise, salt and pepper), beside the bytes the call moves (image and mask read once
     and written once; the gather re-reads neighbours from cache).
  2. The composition a user would write today on the same inputs with PyTorch: float conversion,
     `F.affine_grid` + `F.grid_sample` for the image (bilinear) and for the mask (nearest),
     gain / offset, Gaussian noise, `clamp().round().to(uint8)`.  (An affine grid: PyTorch has
     no perspective grid generator; the kernel's record is the harder perspective one.)
  3. Feeding one batch from pinned host memory: the copies alone, plus drawing and staging the
     records, plus the kernel on the batch that has just arrived (where the extra time of an
     augmented step goes).
  4. `train_step` fed uint8 batches from pinned host memory with and without `BatchAugment`,
     alternated in one process, eager and as `GraphedTrainStep` replays (the augmented replay
     writes through `out=(step.images, step.masks)`); a timed step ends in a device synchronise.

Prints a table and one JSON line; `--out FILE` also writes the JSON there.  `--parts` selects
what runs: `kernel` (1 and 2), `feed` (3), `steps` (4).

    python tools/bench_augment.py [--batch 8] [--hw 512] [--calls 100] [--steps 20] [--rounds 5]
                                  [--parts kernel,feed,steps]
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


def full_config():
    return ua.AugmentConfig(
        horizontal_flip_prob=0.5, shift_scale_rotate_prob=1.0, shift_limit=(-0.1, 0.1),
        scale_limit=(-0.15, 0.15), rotate_limit=(-15.0, 15.0), crop_prob=1.0,
        crop_scale=(0.8, 1.0), crop_ratio=(0.9, 1.1), perspective_prob=1.0,
        perspective_scale=(0.05, 0.1), dropout_prob=1.0, dropout_height=(20, 45),
        dropout_width=(20, 45), color_prob=1.0, brightness_contrast_prob=1.0,
        brightness_limit=(-0.176, 0.176), contrast_limit=(-0.5, 0.25), gray_group_prob=0.5,
        to_gray_prob=1.0, noise_group_prob=1.0, gauss_noise_prob=1.0, gauss_var_limit=(4.0, 18.0),
        salt_pepper_prob=1.0, salt_p=(0.01, 0.05), pepper_p=(0.01, 0.05))


def host_batches(k, n, hw, seed=0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(k):
        img = torch.randint(0, 256, (n, hw, hw, 3), generator=g, dtype=torch.uint8)
        blocks = torch.randint(0, 3, (n, 1, hw // 32, hw // 32), generator=g).float()
        mask = F.interpolate(blocks, size=(hw, hw), mode="nearest")[:, 0].to(torch.uint8)
        mask[:, hw // 2 - 2: hw // 2 + 2] = 255
        out.append((img.pin_memory(), mask.pin_memory()))
    return out


def event_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def summary(v, scale=1.0):
    return {"median": scale * statistics.median(v), "min": scale * min(v), "max": scale * max(v)}


def bench_kernel(x, m, dev, args):
    n, hw = x.shape[0], x.shape[1]
    gen = torch.Generator().manual_seed(1)
    p_full, r_full = ua.augment.sample_params(full_config(), n, hw, hw, gen)
    recs = {"identity": (ua.augment.identity_params(n).to(dev), None),
            "full": (p_full.to(dev), ua.augment.pack_rng(r_full).to(dev))}
    out = (torch.empty_like(x), torch.empty_like(m))
    theta = torch.tensor([[0.95, 0.12, 0.03], [-0.12, 0.95, -0.02]], device=dev).repeat(n, 1, 1)

    def torch_composition():
        xf = x.permute(0, 3, 1, 2).float()
        grid = F.affine_grid(theta, (n, 3, hw, hw), align_corners=False)
        s = F.grid_sample(xf, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
        t = F.grid_sample(m[:, None].float(), grid, mode="nearest", padding_mode="zeros",
                          align_corners=False)
        a = (s * 1.1 + 5.0).clamp(0, 255)
        a = a + 3.0 * torch.randn_like(a)
        return (a.clamp(0, 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous(),
                t[:, 0].to(torch.uint8))

    fns = {k: (lambda pr=pr: ua.ops.augment_u8(x, m, pr[0], pr[1], out=out))
           for k, pr in recs.items()}
    fns["torch_composition"] = torch_composition
    ms = {k: [] for k in fns}
    for fn in fns.values():
        event_ms(fn, 20)
    for _ in range(args.rounds):
        for k, fn in fns.items():
            ms[k].append(event_ms(fn, args.calls))
    moved = 2 * n * hw * hw * 4         # image + mask, read once and written once
    res = {"bytes_moved": moved}
    for k, v in ms.items():
        res[k] = {f"{a}_us": b for a, b in summary(v, 1e3).items()}
        if k != "torch_composition":
            res[k]["GBps_at_median"] = moved / (res[k]["median_us"] * 1e-6) / 1e9
    return res


def bench_feed(batches, dev, args):
    """Where an augmented step's extra time goes: feeding one batch from pinned host memory,
    host clock around `--steps` feeds ended by a synchronise, the three forms alternated -
    (a) the two batch copies alone, (b) plus drawing and staging the records (`sample_params`,
    two pinned buffers, two small copies, an event), (c) plus the kernel on the batch that has
    just arrived over the link."""
    n, hw = batches[0][0].shape[0], batches[0][0].shape[1]
    aug = ua.BatchAugment(full_config(), seed=4)
    out = (torch.empty(batches[0][0].shape, dtype=torch.uint8, device=dev),
           torch.empty(batches[0][1].shape, dtype=torch.uint8, device=dev))

    def feed(form, k):
        x, m = batches[k % len(batches)]
        x = x.to(dev, non_blocking=True)
        m = m.to(dev, non_blocking=True)
        if form == "copy":
            return
        p, r = ua.augment.sample_params(aug.cfg, n, hw, hw, aug.generator)
        staged = aug._stage(p, r, dev)
        if form == "copy+records+kernel":
            ua.ops.augment_u8(x, m, staged.params, staged.rng, out=out)

    forms = ("copy", "copy+records", "copy+records+kernel")
    ms = {f: [] for f in forms}
    for f in forms:
        for k in range(args.warmup):
            feed(f, k)
    for _ in range(args.rounds):
        for f in forms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(args.steps):
                feed(f, k)
            torch.cuda.synchronize()
            ms[f].append((time.perf_counter() - t0) * 1e6 / args.steps)
    return {f: {f"{a}_us": b for a, b in summary(v).items()} for f, v in ms.items()}


class Variant:
    def __init__(self, name, mode, graphed, batches, dev, augment):
        torch.manual_seed(0)
        self.name, self.batches, self.dev = name, batches, dev
        self.model = ua.create_model(dev).train()
        self.model.matmul_precision = mode
        self.opt = ua.create_optimizer(self.model)
        self.lossf = ua.SimpleLoss(target_layout="u8")
        self.aug = ua.BatchAugment(full_config(), seed=3) if augment else None
        self.k = 0
        self.graph = None
        if graphed:
            x, m = (t.to(dev) for t in batches[0])
            self.graph = ua.GraphedTrainStep(self.model, self.opt, self.lossf, x, m,
                                             input_layout="nhwc_u8")

    def step(self):
        x, m = self.batches[self.k % len(self.batches)]
        self.k += 1
        if self.graph is not None and self.aug is None:
            return self.graph(x, m)         # pinned batch straight into the static buffers
        x = x.to(self.dev, non_blocking=True)
        m = m.to(self.dev, non_blocking=True)
        if self.graph is not None:
            x, m = self.aug(x, m, out=(self.graph.images, self.graph.masks))
            return self.graph(x, m)
        if self.aug is not None:
            x, m = self.aug(x, m)
        return ua.train_step(self.model, self.opt, self.lossf, x, m, input_layout="nhwc_u8")

    def timed(self, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps


def bench_steps(mode, graphed, batches, dev, args):
    a = Variant("plain", mode, graphed, batches, dev, augment=False)
    b = Variant("augmented", mode, graphed, batches, dev, augment=True)
    for v in (a, b):
        v.timed(args.warmup)
    ms = {a.name: [], b.name: []}
    for _ in range(args.rounds):          # alternating: both see the same neighbours on the box
        for v in (a, b):
            ms[v.name].append(v.timed(args.steps))
    res = {k: {f"{a_}_ms": b_ for a_, b_ in summary(v).items()} for k, v in ms.items()}
    # host time of drawing and staging one batch of records (no device work waited for)
    t0 = time.perf_counter()
    for _ in range(50):
        ua.augment.sample_params(b.aug.cfg, batches[0][0].shape[0], batches[0][0].shape[1],
                                 batches[0][0].shape[2], b.aug.generator)
    res["sample_params_host_ms"] = (time.perf_counter() - t0) * 1e3 / 50
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--hw", type=int, default=512)
    ap.add_argument("--calls", type=int, default=100, help="kernel calls per timed window")
    ap.add_argument("--steps", type=int, default=20, help="timed steps per round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--modes", default="fp32,bf16")
    ap.add_argument("--parts", default="kernel,feed,steps",
                    help="which parts run: kernel (1 and 2), feed (3), steps (4)")
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    parts = args.parts.split(",")
    if not parts or set(parts) - {"kernel", "feed", "steps"}:
        raise SystemExit("bench_augment: --parts takes kernel, feed, steps")
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment: no ROCm device (there is nothing to measure on a CPU)")
    dev = torch.device("cuda", 0)
    n, hw = args.batch, args.hw
    batches = host_batches(4, n, hw)
    res = {"tool": "bench_augment", "device": torch.cuda.get_device_name(0), "batch": n, "hw": hw,
           "calls": args.calls, "steps": args.steps, "rounds": args.rounds, "warmup": args.warmup}
    print(f"# {res['device']}  batch {n} x {hw}^2")
    x, m = (t.to(dev) for t in batches[0])
    if "kernel" in parts:
        res["kernel"] = bench_kernel(x, m, dev, args)
        print(f"{'call':20s} {'median us':>10s} {'min':>8s} {'max':>8s}   "
              f"({res['kernel']['bytes_moved'] / 1e6:.1f} MB moved)")
        for k, v in res["kernel"].items():
            if isinstance(v, dict):
                print(f"{k:20s} {v['median_us']:10.1f} {v['min_us']:8.1f} {v['max_us']:8.1f}",
                      flush=True)
    if "feed" in parts:
        res["feed_us"] = bench_feed(batches, dev, args)
        print(f"{'feeding one batch':20s} {'median us':>10s} {'min':>8s} {'max':>8s}")
        for k, v in res["feed_us"].items():
            print(f"{k:20s} {v['median_us']:10.1f} {v['min_us']:8.1f} {v['max_us']:8.1f}",
                  flush=True)
    res["step_ms"] = {}
    if "steps" in parts:
        print(f"{'mode':6s} {'step':6s} {'input':10s} {'median ms':>10s} {'min':>8s} {'max':>8s}")
    for mode in args.modes.split(",") if "steps" in parts else ():
        for graphed in (False, True):
            r = bench_steps(mode, graphed, batches, dev, args)
            kind = "graph" if graphed else "eager"
            res["step_ms"][f"{mode}/{kind}"] = r
            for name in ("plain", "augmented"):
                v = r[name]
                print(f"{mode:6s} {kind:6s} {name:10s} {v['median_ms']:10.3f} {v['min_ms']:8.3f} "
                      f"{v['max_ms']:8.3f}", flush=True)
            print(f"{'':13s} sample_params on the host: {r['sample_params_host_ms']:.3f} ms / batch")
            torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
