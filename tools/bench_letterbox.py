#!/usr/bin/env python3
"""What producing a network-size batch on the device costs on one MI355X: 8 decoded samples with
sides in the dataset's range (about 200..600) letterboxed to 512 x 512, with masks.

  1. `unet_letterbox_u8` alone (image + mask, one launch) and the histogram + trimap tables +
     letterbox chain of `label_lut="trimap"`: device events around `--calls` calls behind a
     warm-up, median of `--rounds`.
  2. The same output from the obvious PyTorch composition in the same process: per sample
     `F.interpolate` (bilinear for the image, nearest for the mask) and `F.pad`, stacked.  Not
     byte-equal to cv2 (float arithmetic, ATen's nearest rule): a cost yardstick only.
  3. A device-to-device copy of as many bytes as the kernel's output, as the floor.
  4. The eager uint8 train step (`train_step(..., input_layout="nhwc_u8")`, `SimpleLoss("u8")`) fed
     by `DeviceLetterbox.convert` from pinned ragged arenas against the same step fed pre-resized
     pinned batches, alternated in one process; a timed window ends in a device synchronise.

Prints a table and one JSON line; `--out FILE` also writes the JSON there.

    python tools/bench_letterbox.py [--batch 8] [--size 512] [--calls 100] [--steps 20] [--rounds 5]
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

D = ua.dataprep


def ragged_samples(n, seed):
    """n decoded samples, sides uniform in 200..600, blocky trimap-like masks (0, 128, 255)."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        h, w = (int(v) for v in rng.integers(200, 601, size=2))
        img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        coarse = rng.choice(np.array([0, 128, 255], dtype=np.uint8), p=[0.6, 0.3, 0.1],
                            size=((h + 15) // 16, (w + 15) // 16))
        msk = np.ascontiguousarray(np.kron(coarse, np.ones((16, 16), dtype=np.uint8))[:h, :w])
        out.append({"image": img, "mask": msk, "is_cat": bool(k % 2)})
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


def bench_kernel(batch, size, dev, args):
    table = D.full_table(batch["table"], size, "letterbox").to(dev)
    arena = batch["arena"].to(dev)
    is_cat = torch.as_tensor(batch["is_cat"]).to(dev)
    B = table.shape[0]
    out = (torch.empty((B, size, size, 3), dtype=torch.uint8, device=dev),
           torch.empty((B, size, size), dtype=torch.uint8, device=dev))
    rows = table.cpu().tolist()
    imgs = [arena[r[0]:r[0] + r[2] * r[3] * 3].view(r[2], r[3], 3) for r in rows]
    msks = [arena[r[1]:r[1] + r[2] * r[3]].view(r[2], r[3]) for r in rows]

    def torch_composition():
        xi, xm = [], []
        for r, img, msk in zip(rows, imgs, msks):
            oh, ow, py, px = r[4:]
            pad = (px, size - ow - px, py, size - oh - py)
            a = F.interpolate(img.permute(2, 0, 1)[None].float(), size=(oh, ow), mode="bilinear",
                              align_corners=False)
            xi.append(F.pad(a.round().to(torch.uint8), pad)[0].permute(1, 2, 0))
            m = F.interpolate(msk[None, None].float(), size=(oh, ow), mode="nearest")
            xm.append(F.pad(m.to(torch.uint8), pad)[0, 0])
        return torch.stack(xi), torch.stack(xm)

    def trimap_chain():
        lut = D._device_trimap_luts(ua.ops.byte_histogram_u8(arena, table), is_cat)
        return ua.ops.letterbox_u8(arena, table, size, lut=lut, out=out)

    floor_src = torch.empty(out[0].numel() + out[1].numel(), dtype=torch.uint8, device=dev)
    floor_dst = torch.empty_like(floor_src)
    fns = {"letterbox_u8": lambda: ua.ops.letterbox_u8(arena, table, size, out=out),
           "letterbox_u8_image_only": lambda: ua.ops.letterbox_u8(arena, table, size,
                                                                  want_mask=False, out=(out[0], None)),
           "byte_histogram_u8": lambda: ua.ops.byte_histogram_u8(arena, table),
           "histogram+tables+letterbox": trimap_chain,
           "torch_composition": torch_composition,
           "device_copy_of_output_bytes": lambda: floor_dst.copy_(floor_src)}
    # the composition agrees with the kernel to within one level off the area path (sanity)
    ki, km = ua.ops.letterbox_u8(arena, table, size)
    ti, tm = torch_composition()
    res = {"bytes_in": int(sum(r[2] * r[3] * 4 for r in rows)), "bytes_out": int(floor_src.numel()),
           "sizes": [[r[2], r[3]] for r in rows],
           "max_abs_diff_vs_torch_composition": int((ki.int() - ti.int()).abs().max()),
           "mask_mismatch_vs_torch_composition": int((km != tm).sum())}
    ms = {k: [] for k in fns}
    for fn in fns.values():
        event_ms(fn, 20)
    for _ in range(args.rounds):
        for k, fn in fns.items():
            ms[k].append(event_ms(fn, args.calls))
    for k, v in ms.items():
        res[k] = {f"{a}_us": b for a, b in summary(v, 1e3).items()}
    med = res["letterbox_u8"]["median_us"] * 1e-6
    res["letterbox_u8"]["GBps_in_plus_out_at_median"] = (res["bytes_in"] + res["bytes_out"]) / med / 1e9
    return res


class Variant:
    def __init__(self, name, mode, feeds, dev, letterbox):
        torch.manual_seed(0)
        self.name, self.feeds, self.dev, self.lb = name, feeds, dev, letterbox
        self.model = ua.create_model(dev).train()
        self.model.matmul_precision = mode
        self.opt = ua.create_optimizer(self.model)
        self.lossf = ua.SimpleLoss(target_layout="u8")
        self.k = 0

    def step(self):
        batch = self.feeds[self.k % len(self.feeds)]
        self.k += 1
        if self.lb is not None:
            batch = self.lb.convert(batch)
        x = batch["image"].to(self.dev, non_blocking=True)
        m = batch["mask"].to(self.dev, non_blocking=True)
        return ua.train_step(self.model, self.opt, self.lossf, x, m, input_layout="nhwc_u8")

    def timed(self, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps


def bench_steps(mode, ragged, resized, size, dev, args):
    lb = D.DeviceLetterbox(None, size=size, label_lut="trimap", device=dev)
    a = Variant("pre_resized", mode, resized, dev, None)
    b = Variant("device_letterbox", mode, ragged, dev, lb)
    for v in (a, b):
        v.timed(args.warmup)
    ms = {a.name: [], b.name: []}
    for _ in range(args.rounds):          # alternating: both see the same neighbours on the box
        for v in (a, b):
            ms[v.name].append(v.timed(args.steps))
    return {k: {f"{a_}_ms": b_ for a_, b_ in summary(v).items()} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--calls", type=int, default=100, help="kernel calls per timed window")
    ap.add_argument("--steps", type=int, default=20, help="timed steps per round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--modes", default="fp32,bf16")
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_letterbox: no ROCm device (there is nothing to measure on a CPU)")
    dev = torch.device("cuda", 0)
    n, size = args.batch, args.size
    ragged = [D.ragged_collate(ragged_samples(n, seed)) for seed in range(4)]
    res = {"tool": "bench_letterbox", "device": torch.cuda.get_device_name(0), "batch": n,
           "size": size, "calls": args.calls, "steps": args.steps, "rounds": args.rounds,
           "warmup": args.warmup}
    print(f"# {res['device']}  {n} samples -> {size}^2")
    res["kernel"] = bench_kernel(ragged[0], size, dev, args)
    k = res["kernel"]
    print(f"{'call':30s} {'median us':>10s} {'min':>8s} {'max':>8s}   "
          f"({k['bytes_in'] / 1e6:.1f} MB in, {k['bytes_out'] / 1e6:.1f} MB out)")
    for name, v in k.items():
        if isinstance(v, dict):
            print(f"{name:30s} {v['median_us']:10.1f} {v['min_us']:8.1f} {v['max_us']:8.1f}",
                  flush=True)
    # the pre-resized twin of every ragged batch, produced once by the wrapper itself
    lb = D.DeviceLetterbox(None, size=size, label_lut="trimap", device=dev)
    resized = []
    for batch in ragged:
        out = lb.convert(batch)
        resized.append({"image": out["image"].cpu().pin_memory(),
                        "mask": out["mask"].cpu().pin_memory()})
    res["step_ms"] = {}
    print(f"{'mode':6s} {'input':18s} {'median ms':>10s} {'min':>8s} {'max':>8s}")
    for mode in args.modes.split(","):
        r = bench_steps(mode, ragged, resized, size, dev, args)
        res["step_ms"][f"{mode}/eager"] = r
        for name, v in r.items():
            print(f"{mode:6s} {name:18s} {v['median_ms']:10.3f} {v['min_ms']:8.3f} "
                  f"{v['max_ms']:8.3f}", flush=True)
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
