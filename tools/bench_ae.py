#!/usr/bin/env python3
"""Autoencoder pretraining step (ua.ae) throughput on one MI355X, against the segmentation step
timed in the same process.

For each operand mode (fp32, bf16) and batch size (8, and the reference's 32) at 512x512: AE
img/s eager and graph-replayed (GraphedTrainStep with FusedAdam), and the segmentation step
(UNet + SimpleLoss + FusedSGD, graph-replayed) timed in alternation with the AE's graph so the
ratio does not depend on the box.  One eager AE step under ops.KernelTimer gives the achieved
bytes/s of the four new kernels (algorithmic byte counts of ops.py).  Prints one JSON line.

    python tools/bench_ae.py [--steps 10] [--warmup 3] [--reps 3] [--batches 8,32]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import unet_implementations_amd as ua  # noqa: E402

DEV = "cuda"


def _timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def _images(n, hw, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 256, (n, 3, hw, hw), generator=g).float() / 255.0).to(DEV)


def ae_setup(mode, n, hw):
    model = ua.ae.create_model(DEV).train()
    model.matmul_precision = mode
    opt = ua.ae.create_optimizer(model)
    lossf = ua.ae.get_loss_function()
    img = _images(n, hw, 1)
    return model, opt, lossf, img


def seg_setup(mode, n, hw):
    model = ua.create_model(DEV).train()
    model.matmul_precision = mode
    opt = ua.create_optimizer(model)
    lossf = ua.get_loss_function()
    g = torch.Generator().manual_seed(2)
    img = torch.randn(n, 3, hw, hw, generator=g).to(DEV)
    tgt = torch.randint(0, 3, (n, hw, hw), generator=g).to(DEV)
    return model, opt, lossf, img, tgt


def kernel_rates(model, opt, lossf, img):
    timer = ua.ops.KernelTimer()
    ua.ops.set_timer(timer)
    try:
        ua.train_step(model, opt, lossf, img, img)
    finally:
        ua.ops.set_timer(None)
    s = timer.summary()
    out = {}
    for tag in ("recon_fwd", "recon_bwd", "mse_loss", "mse_grad", "adam"):
        if tag in s:
            d = s[tag]
            out[tag] = dict(us=round(1e3 * d["ms"], 1), MB=round(d["bytes"] / 1e6, 1),
                            TBps=round(d["bytes"] / (d["ms"] * 1e-3) / 1e12, 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--hw", type=int, default=512)
    ap.add_argument("--batches", default="8,32")
    ap.add_argument("--modes", default="fp32,bf16")
    args = ap.parse_args()
    res = {"hw": args.hw, "steps": args.steps, "reps": args.reps, "device":
           torch.cuda.get_device_name(0), "runs": []}
    for mode in args.modes.split(","):
        for n in [int(b) for b in args.batches.split(",")]:
            model, opt, lossf, img = ae_setup(mode, n, args.hw)
            for _ in range(args.warmup):
                ua.train_step(model, opt, lossf, img, img)
            eager_ms = _timed(lambda: ua.train_step(model, opt, lossf, img, img), args.steps)
            rates = kernel_rates(model, opt, lossf, img)
            step = ua.GraphedTrainStep(model, opt, lossf, img, img, warmup=args.warmup)
            smodel, sopt, slossf, simg, stgt = seg_setup(mode, n, args.hw)
            sstep = ua.GraphedTrainStep(smodel, sopt, slossf, simg, stgt, warmup=args.warmup)
            ae_ms, seg_ms = [], []
            for _ in range(args.reps):      # alternate the two graphs
                ae_ms.append(_timed(lambda: step(img, img), args.steps))
                seg_ms.append(_timed(lambda: sstep(simg, stgt), args.steps))
            a, s = statistics.median(ae_ms), statistics.median(seg_ms)
            res["runs"].append(dict(
                mode=mode, batch=n, ae_eager_ms=round(eager_ms, 3),
                ae_eager_img_s=round(n / eager_ms * 1e3, 1), ae_graph_ms=round(a, 3),
                ae_graph_img_s=round(n / a * 1e3, 1), seg_graph_ms=round(s, 3),
                seg_graph_img_s=round(n / s * 1e3, 1), ae_over_seg=round(a / s, 4),
                kernels=rates))
            del step, sstep, model, smodel, opt, sopt
            torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
