#!/usr/bin/env python3
"""What elastic / grid / optical distortion costs on one MI355X, at the flagship batch
(8 x 512^2 by default).  Device events around `--calls` calls behind a warm-up, medians of
`--rounds`, as tools/bench_augment.py:

  1. `unet_elastic_field` alone with every sample elastic, at sigma 4 (R = 12), at the radius
     cap (sigma 6, R = 16) and at sigma 0.5 (R = 2), and with no elastic sample (every workgroup
     returns at once).
  2. `unet_augment_warp_u8` alone per mode (0 none, 1 elastic reading a field, 2 grid, 3 optical)
     on the full record of bench_augment.py, beside `unet_augment_u8` on the same record,
     re-measured in the same process.
  3. field + gather (all samples elastic) against `unet_augment_u8`, and against the composition a
     user would write with PyTorch: `rand`, two 1-D `conv2d`, added to `F.affine_grid`,
     `F.grid_sample` x 2.
  4. `train_step` fed uint8 batches from pinned host memory with `BatchAugment` without and with
     a distortion configuration, alternated in one process, fp32 and bf16, eager and as
     `GraphedTrainStep` replays.

Prints a table and one JSON line; `--out FILE` also writes the JSON there.

    python tools/bench_distort.py [--batch 8] [--hw 512] [--calls 100] [--steps 20] [--rounds 5]
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import unet_implementations_amd as ua  # noqa: E402
from bench_augment import event_ms, full_config, host_batches, summary  # noqa: E402


def distort_config(**member):
    """bench_augment's full record plus the distortion group with the given member(s)"""
    return ua.AugmentConfig(**{**vars(full_config()), "distort_group_prob": 1.0, **member})


ELASTIC = dict(elastic_prob=1.0, elastic_alpha=40.0, elastic_sigma=4.0, elastic_alpha_affine=15.0)
GRID = dict(grid_distortion_prob=1.0, grid_num_steps=5, grid_distort_limit=0.2)
OPTICAL = dict(optical_distortion_prob=1.0, optical_distort_limit=0.2, optical_shift_limit=0.15)


def us(v):
    return {f"{a}_us": b for a, b in summary(v, 1e3).items()}


def bench_kernels(x, m, dev, args):
    n, hw = x.shape[0], x.shape[1]
    gen = torch.Generator().manual_seed(1)
    p, r = ua.augment.sample_params(full_config(), n, hw, hw, gen)
    dp, dr = p.to(dev), ua.augment.pack_rng(r).to(dev)
    warps = {"none": ua.augment.identity_warp(n)}
    for name, member in (("elastic", ELASTIC), ("elastic_cap", {**ELASTIC, "elastic_sigma": 6.0}),
                         ("elastic_r2", {**ELASTIC, "elastic_sigma": 0.5}),
                         ("grid", GRID), ("optical", OPTICAL)):
        w = ua.augment.sample_warp(distort_config(**member), n, hw, hw, gen)
        ua.augment.validate_warp(w, p, hw, hw)
        warps[name] = w
    dw = {k: v.to(dev) for k, v in warps.items()}
    field = torch.zeros((n, hw, hw, 2), dtype=torch.float32, device=dev)
    out = (torch.empty_like(x), torch.empty_like(m))
    ua.ops.elastic_field(dw["elastic"], dr, (hw, hw), out=field)

    theta = torch.tensor([[0.95, 0.12, 0.03], [-0.12, 0.95, -0.02]], device=dev).repeat(n, 1, 1)
    R, g1 = ua.augment.gaussian_taps(4.0)
    taps = torch.tensor(list(g1[R:0:-1]) + list(g1[:R + 1]), dtype=torch.float32, device=dev)
    k_row = taps.view(1, 1, 1, -1).repeat(2, 1, 1, 1)
    k_col = taps.view(1, 1, -1, 1).repeat(2, 1, 1, 1)

    def torch_composition():
        noise = torch.rand((n, 2, hw, hw), device=dev) * 2 - 1
        d = F.conv2d(F.conv2d(noise, k_row, padding=(0, R), groups=2), k_col, padding=(R, 0),
                     groups=2)
        grid = F.affine_grid(theta, (n, 3, hw, hw), align_corners=False) + \
            d.permute(0, 2, 3, 1) * (40.0 * 2.0 / hw)
        xf = x.permute(0, 3, 1, 2).float()
        s = F.grid_sample(xf, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
        t = F.grid_sample(m[:, None].float(), grid, mode="nearest", padding_mode="zeros",
                          align_corners=False)
        return (s.clamp(0, 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous(),
                t[:, 0].to(torch.uint8))

    def pair(name):
        ua.ops.elastic_field(dw[name], dr, (hw, hw), out=field)
        ua.ops.augment_warp_u8(x, m, dp, dr, dw[name], field, out=out)

    fns = {
        "augment_u8_full": lambda: ua.ops.augment_u8(x, m, dp, dr, out=out),
        "field_sigma4_R12": lambda: ua.ops.elastic_field(dw["elastic"], dr, (hw, hw), out=field),
        "field_sigma0.5_R2": lambda: ua.ops.elastic_field(dw["elastic_r2"], dr, (hw, hw),
                                                          out=field),
        "field_sigma6_R16": lambda: ua.ops.elastic_field(dw["elastic_cap"], dr, (hw, hw),
                                                         out=field),
        "field_no_elastic_sample": lambda: ua.ops.elastic_field(dw["grid"], dr, (hw, hw),
                                                                out=field),
    }
    for name in ("none", "elastic", "grid", "optical"):
        fns[f"gather_{name}"] = (lambda name=name: ua.ops.augment_warp_u8(
            x, m, dp, dr, dw[name], field, out=out))
    fns["field+gather_elastic"] = lambda: pair("elastic")
    fns["field+gather_elastic_cap"] = lambda: pair("elastic_cap")
    fns["field+gather_grid"] = lambda: pair("grid")
    fns["torch_composition"] = torch_composition
    ms = {k: [] for k in fns}
    for fn in fns.values():
        event_ms(fn, 20)
    for _ in range(args.rounds):
        for k, fn in fns.items():
            if k == "gather_elastic":       # the field the gather reads: sigma 4, not the cap's
                ua.ops.elastic_field(dw["elastic"], dr, (hw, hw), out=field)
            ms[k].append(event_ms(fn, args.calls))
    res = {k: us(v) for k, v in ms.items()}
    res["field_bytes"] = n * hw * hw * 2 * 4
    return res


class Variant:
    def __init__(self, name, mode, graphed, batches, dev, cfg):
        torch.manual_seed(0)
        self.name, self.batches, self.dev = name, batches, dev
        self.model = ua.create_model(dev).train()
        self.model.matmul_precision = mode
        self.opt = ua.create_optimizer(self.model)
        self.lossf = ua.SimpleLoss(target_layout="u8")
        self.aug = ua.BatchAugment(cfg, seed=3)
        self.k = 0
        self.graph = None
        if graphed:
            x, m = (t.to(dev) for t in batches[0])
            self.graph = ua.GraphedTrainStep(self.model, self.opt, self.lossf, x, m,
                                             input_layout="nhwc_u8")

    def step(self):
        x, m = self.batches[self.k % len(self.batches)]
        self.k += 1
        x = x.to(self.dev, non_blocking=True)
        m = m.to(self.dev, non_blocking=True)
        if self.graph is not None:
            x, m = self.aug(x, m, out=(self.graph.images, self.graph.masks))
            return self.graph(x, m)
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
    """every sample elastic: the dearest member, both kernels at full work"""
    a = Variant("augment", mode, graphed, batches, dev, full_config())
    b = Variant("augment+distortion", mode, graphed, batches, dev, distort_config(**ELASTIC))
    for v in (a, b):
        v.timed(args.warmup)
    ms = {a.name: [], b.name: []}
    for _ in range(args.rounds):          # alternating: both see the same neighbours on the box
        for v in (a, b):
            ms[v.name].append(v.timed(args.steps))
    res = {k: {f"{a_}_ms": b_ for a_, b_ in summary(v).items()} for k, v in ms.items()}
    n, hw = batches[0][0].shape[0], batches[0][0].shape[1]
    t0 = time.perf_counter()
    for _ in range(50):
        ua.augment.sample_warp(b.aug.cfg, n, hw, hw, b.aug.generator)
    res["sample_warp_host_ms"] = (time.perf_counter() - t0) * 1e3 / 50
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
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_distort: no ROCm device (there is nothing to measure on a CPU)")
    dev = torch.device("cuda", 0)
    n, hw = args.batch, args.hw
    batches = host_batches(4, n, hw)
    res = {"tool": "bench_distort", "device": torch.cuda.get_device_name(0), "batch": n, "hw": hw,
           "calls": args.calls, "steps": args.steps, "rounds": args.rounds, "warmup": args.warmup}
    print(f"# {res['device']}  batch {n} x {hw}^2")
    x, m = (t.to(dev) for t in batches[0])
    res["kernel"] = bench_kernels(x, m, dev, args)
    print(f"{'call':28s} {'median us':>10s} {'min':>8s} {'max':>8s}")
    for k, v in res["kernel"].items():
        if isinstance(v, dict):
            print(f"{k:28s} {v['median_us']:10.1f} {v['min_us']:8.1f} {v['max_us']:8.1f}",
                  flush=True)
    res["step_ms"] = {}
    print(f"{'mode':6s} {'step':6s} {'input':20s} {'median ms':>10s} {'min':>8s} {'max':>8s}")
    for mode in args.modes.split(","):
        for graphed in (False, True):
            r = bench_steps(mode, graphed, batches, dev, args)
            kind = "graph" if graphed else "eager"
            res["step_ms"][f"{mode}/{kind}"] = r
            for name in ("augment", "augment+distortion"):
                v = r[name]
                print(f"{mode:6s} {kind:6s} {name:20s} {v['median_ms']:10.3f} {v['min_ms']:8.3f} "
                      f"{v['max_ms']:8.3f}", flush=True)
            print(f"{'':13s} sample_warp on the host: {r['sample_warp_host_ms']:.3f} ms / batch")
            torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
