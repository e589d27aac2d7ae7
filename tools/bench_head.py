#!/usr/bin/env python3
"""Times of the network's tail at bs 8, 512 x 512: the 1x1 head on the activated 32-channel tensor
(forward and backward, fp32 and bf16 layer tensors) and, with --classes K other than 3, the K-class
loss (its three launches) and argmax / counts - each beside a torch composition on the device
(1x1 F.conv2d, the reference SimpleLoss formula, argmax) and beside the bytes the kernel must move
at the HBM rate.  --step also times a whole K-class training step (graph replay) for the tail's
share of it.

Usage: [UNET_HIP_LIB=...] python tools/bench_head.py [reps] [--classes K] [--step] [--json FILE]"""
import argparse
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
import unet_implementations_amd as ua
ops = ua.ops

ap = argparse.ArgumentParser()
ap.add_argument("reps", nargs="?", type=int, default=20)
ap.add_argument("--classes", type=int, default=3)
ap.add_argument("--step", action="store_true")
ap.add_argument("--json")
args = ap.parse_args()
reps = args.reps
N, H, C, K = 8, 512, 32, args.classes
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12      # bytes/s: spec, and what a float4 copy reaches
result = {"shape": [N, H, H], "classes": K, "reps": reps, "kernels": {}}


def timeit(fn):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def row(name, us, nbytes, torch_us=None):
    floor = nbytes / HBM_COPY * 1e6
    result["kernels"][name] = {"us": round(us, 1), "MB": round(nbytes / 1e6, 1),
                               "us_at_6.29_TBps": round(floor, 1), "share_of_that": round(floor / us, 3),
                               "TBps": round(nbytes / us / 1e6, 2),
                               "torch_us": None if torch_us is None else round(torch_us, 1)}
    extra = "" if torch_us is None else f"   torch {torch_us:8.1f} us"
    print(f"{name:28s} {us:8.1f} us   {nbytes / 1e6:7.1f} MB   {nbytes / us / 1e6:5.2f} TB/s "
          f"({floor / us:4.0%} of the copy rate){extra}", flush=True)


px = N * H * H
w = torch.randn(K, C, device="cuda") * 0.2
b = torch.zeros(K, device="cuda")
al = torch.rand(N, C, device="cuda") + 0.5
be = torch.randn(N, C, device="cuda")
dl = torch.randn(N, K, H, H, device="cuda")
for b16 in (False, True):
    y = torch.randn(N, H, H, C, device="cuda")
    if b16:
        y = y.to(torch.bfloat16)
    s = ops.Act(y, al, be)
    t_f = timeit(lambda: ops.head1x1_in_fwd(s, 0.01, w, b))
    dw, db = torch.empty(K, C, device="cuda"), torch.empty(K, device="cuda")
    t_b = timeit(lambda: ops.head1x1_in_bwd(s, 0.01, dl, w, dw, db))
    tag, es = ("bf16" if b16 else "fp32"), y.element_size()
    t_tf = t_tb = None
    if not b16:      # the torch composition: activation, then conv2d and its backward (NCHW fp32)
        a = F.leaky_relu(y * al[:, None, None, :] + be[:, None, None, :], 0.01).permute(0, 3, 1, 2)
        a = a.contiguous().requires_grad_(True)
        w4 = w[:, :, None, None].clone().requires_grad_(True)
        t_tf = timeit(lambda: F.conv2d(a, w4, b))
        out = F.conv2d(a, w4, b)
        t_tb = timeit(lambda: torch.autograd.grad(out, (a, w4), dl, retain_graph=True))
    row(f"head forward {tag}", t_f, px * (C * es + K * 4), t_tf)
    row(f"head backward {tag}", t_b, px * (2 * C * es + K * 4), t_tb)

if K != 3:
    logits = torch.randn(N, K, H, H, device="cuda") * 2
    t64 = torch.randint(0, K, (N, H, H), device="cuda")
    t64[:, :8] = 255
    t8 = t64.to(torch.uint8)

    def torch_loss():
        z = logits.detach().requires_grad_(True)
        valid = t64 != 255
        counts = torch.stack([((t64 == c) & valid).sum().float() for c in range(K)])
        counts = torch.where(counts == 0, torch.ones_like(counts), counts)
        wt = valid.sum().float() / counts
        wt = wt * (K / wt.sum())
        ce = F.cross_entropy(z, t64, weight=wt, ignore_index=255)
        prob, vf, tot = F.softmax(z, dim=1), valid.float(), 0
        for c in range(K):
            t = ((t64 == c).float() * vf).reshape(N, -1)
            p = (prob[:, c] * vf).reshape(N, -1)
            tot = tot + (1.0 - ((2.0 * (p * t).sum(1) + 1e-5) / (p.sum(1) + t.sum(1) + 1e-5)).mean())
        (ce + tot / K).backward()
        return z.grad

    t_torch = timeit(torch_loss)
    for tag, tg, tb in (("int64", t64, 8), ("uint8", t8, 1)):
        ws = ops.dice_wce_loss_workspace(logits)
        t_fwd = timeit(lambda: ops.dice_wce_loss_fwd_bwd(logits, tg, 1e-5, 1.0, 1.0, 255, True,
                                                        want_grad=False, ws=ws))
        t_grad = timeit(lambda: ops.dice_wce_loss_grad(logits, tg, ws, None, 255))
        row(f"loss reduce+finalize {tag}", t_fwd, px * (K * 4 + tb))
        row(f"loss gradient {tag}", t_grad, px * (2 * K * 4 + tb))
        result["kernels"][f"loss three launches {tag}"] = {
            "us": round(t_fwd + t_grad, 1), "torch_us": round(t_torch, 1) if tb == 8 else None}
        t_c = timeit(lambda: ops.argmax_dice_counts(logits, tg))
        row(f"argmax + counts {tag}", t_c, px * (K * 4 + tb + 1),
            timeit(lambda: logits.argmax(1)) if tb == 8 else None)
    print(f"torch SimpleLoss formula, forward + backward: {t_torch:8.1f} us")

if args.step:
    model = ua.UNet(num_classes=K).to("cuda").train()
    opt = ua.create_optimizer(model)
    lossf = ua.SimpleLoss()
    img = torch.randn(N, 3, H, H, device="cuda")
    tgt = torch.randint(0, K, (N, H, H), device="cuda")
    step = ua.GraphedTrainStep(model, opt, lossf, img, tgt)
    t_step = timeit(lambda: step(img, tgt))
    k = result["kernels"]
    tail = k["head forward fp32"]["us"] + k["head backward fp32"]["us"]
    if K != 3:
        tail += k["loss three launches int64"]["us"]
    result["step"] = {"us": round(t_step, 1), "tail_us": round(tail, 1),
                      "tail_share": round(tail / t_step, 4), "img_per_s": round(N / t_step * 1e6, 1)}
    print(f"train step (graph replay, fp32 mode): {t_step:9.1f} us = {N / t_step * 1e6:6.1f} img/s; "
          f"tail (head + loss) {tail:7.1f} us = {tail / t_step:.1%}")

if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
