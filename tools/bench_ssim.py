#!/usr/bin/env python3
"""Fused SSIM kernels (unet_ssim_fwd / unet_ssim_grad) on one MI355X, against the torch
formulation of the reference's SSIMLoss on the same GPU, and the cost of the SSIM term in the
graph-replayed autoencoder step.

At N x 3 x H x W (default 8 x 3 x 512 x 512): the forward (reduce + finalize) and the gradient
launch under ops.KernelTimer (achieved bytes/s from ops.py's algorithmic byte counts); the whole
SSIMLoss forward + backward call; the reference's formulation (five grouped F.conv2d with the
11 x 11 window, autograd through all of it) forward and forward + backward; and the AE step
(GraphedTrainStep + FusedAdam) under MSELoss against the same step under
ReconstructionLoss(1, 0, 0.1), timed in alternation.  Prints one JSON line.

    python tools/bench_ssim.py [--steps 20] [--warmup 3] [--reps 3] [--batch 8] [--hw 512]
    python tools/bench_ssim.py --profile-step   # 3 eager AE steps with the SSIM term, for a trace
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

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


def _median(fn, steps, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return statistics.median(_timed(fn, steps) for _ in range(reps))


def _pair(n, hw, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(n, 3, hw, hw, generator=g)
    p = (t + 0.1 * torch.randn(t.shape, generator=g)).clamp(0, 1)
    return p.to(DEV).contiguous(), t.to(DEV).contiguous()


def torch_ssim_loss(window):
    """The reference's SSIMLoss._ssim (models/losses.py:204-224) with its intended window."""
    def f(img1, img2):
        ch = img1.shape[1]
        mu1 = F.conv2d(img1, window, padding=5, groups=ch)
        mu2 = F.conv2d(img2, window, padding=5, groups=ch)
        mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
        s1 = F.conv2d(img1 * img1, window, padding=5, groups=ch) - mu1_sq
        s2 = F.conv2d(img2 * img2, window, padding=5, groups=ch) - mu2_sq
        s12 = F.conv2d(img1 * img2, window, padding=5, groups=ch) - mu1_mu2
        m = ((2 * mu1_mu2 + 1e-4) * (2 * s12 + 9e-4)) / ((mu1_sq + mu2_sq + 1e-4) * (s1 + s2 + 9e-4))
        return 1 - m.mean()
    return f


def kernel_times(fn, reps):
    out = {}
    for _ in range(reps):
        timer = ua.ops.KernelTimer()
        ua.ops.set_timer(timer)
        try:
            fn()
        finally:
            ua.ops.set_timer(None)
        for tag, d in timer.summary().items():
            out.setdefault(tag, []).append((d["ms"], d["bytes"]))
    res = {}
    for tag, v in out.items():
        ms = statistics.median(m for m, _ in v)
        b = v[0][1]
        res[tag] = dict(us=round(1e3 * ms, 1), MB=round(b / 1e6, 1),
                        TBps=round(b / (ms * 1e-3) / 1e12, 2))
    return res


def ae_step_compare(n, hw, steps, reps, warmup):
    img = (torch.randint(0, 256, (n, 3, hw, hw), generator=torch.Generator().manual_seed(1))
           .float() / 255.0).to(DEV)
    graphs = {}
    for name, lossf in (("mse", ua.MSELoss()), ("mse_ssim", ua.ReconstructionLoss(1.0, 0.0, 0.1))):
        model = ua.ae.create_model(DEV).train()
        opt = ua.ae.create_optimizer(model)
        graphs[name] = (ua.GraphedTrainStep(model, opt, lossf, img, img, warmup=warmup), model)
    ms = {k: [] for k in graphs}
    for _ in range(reps):     # alternate the two graphs
        for k, (step, _) in graphs.items():
            ms[k].append(_timed(lambda: step(img, img), steps))
    a, b = statistics.median(ms["mse"]), statistics.median(ms["mse_ssim"])
    return dict(ae_graph_ms_mse=round(a, 3), ae_graph_ms_mse_ssim=round(b, 3),
                ssim_term_overhead=round(b / a - 1, 4))


def profile_step(n, hw):
    img = (torch.randint(0, 256, (n, 3, hw, hw), generator=torch.Generator().manual_seed(1))
           .float() / 255.0).to(DEV)
    model = ua.ae.create_model(DEV).train()
    opt = ua.ae.create_optimizer(model)
    lossf = ua.ReconstructionLoss(1.0, 0.0, 0.1)
    for _ in range(3):
        ua.train_step(model, opt, lossf, img, img)
    torch.cuda.synchronize()
    print(json.dumps({"profile_step": "done", "batch": n, "hw": hw}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--hw", type=int, default=512)
    ap.add_argument("--profile-step", action="store_true")
    ap.add_argument("--skip-ae", action="store_true")
    args = ap.parse_args()
    if args.profile_step:
        profile_step(args.batch, args.hw)
        return
    n, hw = args.batch, args.hw
    p, t = _pair(n, hw, 0)
    res = {"shape": [n, 3, hw, hw], "steps": args.steps, "reps": args.reps,
           "device": torch.cuda.get_device_name(0)}
    one = torch.ones((), device=DEV)

    def fused_both():
        ua.ops.ssim_fwd(p, t)
        ua.ops.ssim_grad(p, t, one)

    for _ in range(args.warmup):
        fused_both()
    res["kernels"] = kernel_times(fused_both, max(args.reps, 5))
    res["fused_fwd_ms"] = round(_median(lambda: ua.ops.ssim_fwd(p, t), args.steps, args.reps,
                                        args.warmup), 4)
    res["fused_grad_ms"] = round(_median(lambda: ua.ops.ssim_grad(p, t, one), args.steps,
                                         args.reps, args.warmup), 4)
    lossf = ua.SSIMLoss()

    def fused_call():
        x = p.detach().requires_grad_(True)
        lossf(x, t).backward()

    res["fused_loss_fwd_bwd_ms"] = round(_median(fused_call, args.steps, args.reps,
                                                 args.warmup), 4)
    w = torch.tensor(ua.ops.gaussian_window(), device=DEV)
    window = (w.view(-1, 1) * w.view(1, -1)).expand(3, 1, 11, 11).contiguous()
    tf = torch_ssim_loss(window)

    def torch_fwd():
        with torch.no_grad():
            tf(p, t)

    def torch_call():
        x = p.detach().requires_grad_(True)
        tf(x, t).backward()

    res["torch_fwd_ms"] = round(_median(torch_fwd, args.steps, args.reps, args.warmup), 4)
    res["torch_fwd_bwd_ms"] = round(_median(torch_call, args.steps, args.reps, args.warmup), 4)
    res["speedup_fwd"] = round(res["torch_fwd_ms"] / res["fused_fwd_ms"], 2)
    res["speedup_fwd_bwd"] = round(res["torch_fwd_bwd_ms"] / res["fused_loss_fwd_bwd_ms"], 2)
    with torch.no_grad():
        res["check_loss_fused_vs_torch"] = abs(lossf(p, t).item() - tf(p, t).item())
    if not args.skip_ae:
        res.update(ae_step_compare(n, hw, max(args.steps // 2, 5), args.reps, args.warmup))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
