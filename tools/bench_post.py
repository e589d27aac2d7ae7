#!/usr/bin/env python3
"""What the second augmentation stage (HSV shift, equalize / CLAHE, blur) costs on one MI355X, at
the flagship batch (8 x 512^2 by default).  Device events around `--calls` calls behind a
warm-up, medians of `--rounds`, as tools/bench_distort.py:

  1. the histogram half (`unet_augment_post_hist`: the memset of the counts and the histogram
     kernel) with no histogram op in the batch (every workgroup returns at once), every sample
     equalize, every sample CLAHE 8 x 8.
  2. the apply half (`unet_augment_post_apply`) per mode: copy only, HSV, equalize, CLAHE,
     separable R = 1 and 4, dense R = 1 and 3, everything (HSV + CLAHE + separable R = 4 + salt /
     pepper), on a workspace the histogram half filled for that record.
  3. gather + post (`unet_augment_u8` with salt / pepper off into an intermediate image, then
     `unet_augment_post_u8` with everything) against `unet_augment_u8` with the full record of
     bench_augment.py, in this process; and the composition a user would write with PyTorch for
     equalize + Gaussian blur (per-channel `bincount`, `cumsum`, a LUT `gather`, two `conv2d`).
  4. `train_step` fed uint8 batches from pinned host memory with `BatchAugment` without and with
     a photometric configuration, alternated in one process, fp32 and bf16, eager and as
     `GraphedTrainStep` replays.

Prints a table and one JSON line; `--out FILE` also writes the JSON there.

    python tools/bench_post.py [--batch 8] [--hw 512] [--calls 100] [--steps 20] [--rounds 5]
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
from bench_distort import Variant, us  # noqa: E402

A = ua.augment


def photo_config():
    """bench_augment's full record with every group handing its samples to a new member"""
    return ua.AugmentConfig(**{
        **vars(full_config()), "gray_group_prob": 1.0, "brightness_contrast_prob": 0.0,
        "to_gray_prob": 0.0, "gauss_noise_prob": 0.0, "hsv_prob": 1.0, "hue_shift_limit": 10.0,
        "sat_shift_limit": 30.0, "val_shift_limit": 20.0, "clahe_prob": 0.5,
        "clahe_clip_limit": 4.0, "clahe_tile_grid": (8, 8), "equalize_prob": 0.5,
        "gaussian_blur_prob": 0.5, "gaussian_blur_limit": (0, 9), "motion_blur_prob": 0.5,
        "motion_blur_limit": (3, 7)})


def record(n, hsv=False, op=0, blur=0, R=0):
    q = A.identity_post(n).numpy()
    if hsv:
        q[:, A.Q_HSV], q[:, A.Q_DH], q[:, A.Q_DS], q[:, A.Q_DV] = 1, 7.0, -20.0, 12.0
    q[:, A.Q_HIST] = op
    if op == A.HIST_CLAHE:
        q[:, A.Q_CLIP], q[:, A.Q_TY], q[:, A.Q_TX] = 3.0, 8, 8
    if blur == A.BLUR_SEPARABLE:
        k = 2 * R + 1
        _, g = A.gaussian_taps(0.3 * ((k - 1) * 0.5 - 1) + 0.8, radius=R)
        q[:, A.Q_BLUR], q[:, A.Q_RADIUS] = blur, R
        q[:, A.Q_TAPS:A.Q_TAPS + R + 1] = g[:R + 1]
    if blur == A.BLUR_DENSE:
        k = 2 * R + 1
        q[:, A.Q_BLUR], q[:, A.Q_RADIUS] = blur, R
        q[:, A.Q_DENSE:A.Q_DENSE + k * k] = A.motion_line(k, (0, 0), (k - 1, k // 2)).reshape(-1)
    return torch.from_numpy(q)


def bench_kernels(x, m, dev, args):
    n, hw = x.shape[0], x.shape[1]
    lib, stream = ua.lib(), ua.ops._stream
    p, r = A.sample_params(full_config(), n, hw, hw, torch.Generator().manual_seed(1))
    dp, dr = p.to(dev), A.pack_rng(r).to(dev)
    r0 = r.clone()
    r0[:, 2:] = 0
    dr0 = A.pack_rng(r0).to(dev)
    recs = {"copy": record(n), "hsv": record(n, hsv=True), "equalize": record(n, op=1),
            "clahe8x8": record(n, op=2), "separable_R1": record(n, blur=1, R=1),
            "separable_R4": record(n, blur=1, R=4), "dense_R1": record(n, blur=2, R=1),
            "dense_R3": record(n, blur=2, R=3),
            "everything": record(n, hsv=True, op=2, blur=1, R=4)}
    for q in recs.values():
        A.validate_post(q, hw, hw)
    dq = {k: v.to(dev) for k, v in recs.items()}
    need = lib.unet_augment_post_workspace_bytes(n)
    ws = {k: torch.empty(need, dtype=torch.uint8, device=dev) for k in recs}
    mid, out, mout = torch.empty_like(x), torch.empty_like(x), torch.empty_like(m)

    def hist(k):
        ua._lib.check(lib.unet_augment_post_hist(x.data_ptr(), dq[k].data_ptr(),
                                                 ws[k].data_ptr(), need, n, hw, hw, stream()))

    def apply(k, rng=None):
        ua._lib.check(lib.unet_augment_post_apply(
            x.data_ptr(), out.data_ptr(), dq[k].data_ptr(),
            rng.data_ptr() if rng is not None else None, ws[k].data_ptr(), need, n, hw, hw,
            stream()))

    for k in recs:
        hist(k)                     # the workspace each apply reads
    R4, g4 = A.gaussian_taps(0.3 * 3 + 0.8, radius=4)
    taps = torch.tensor(list(g4[R4:0:-1]) + list(g4[:R4 + 1]), dtype=torch.float32, device=dev)
    k_row = taps.view(1, 1, 1, -1).repeat(3, 1, 1, 1)
    k_col = taps.view(1, 1, -1, 1).repeat(3, 1, 1, 1)
    offs = (torch.arange(n * 3, device=dev) * 256).view(n, 1, 1, 3)

    def torch_composition():
        idx = x.long() + offs
        hist_ = torch.bincount(idx.reshape(-1), minlength=n * 3 * 256).view(n, 3, 256)
        cdf = hist_.cumsum(-1)
        first = (cdf == 0).sum(-1, keepdim=True).clamp(max=255)
        h0 = hist_.gather(-1, first)
        lut = ((cdf - h0).clamp(min=0).float() * (255.0 / (hw * hw - h0).clamp(min=1).float()))
        lut = lut.round().clamp(0, 255)
        eq = lut.reshape(-1)[idx.reshape(-1)].view(n, hw, hw, 3).permute(0, 3, 1, 2)
        b = F.conv2d(F.pad(eq, (R4, R4, 0, 0), mode="reflect"), k_row, groups=3)
        b = F.conv2d(F.pad(b, (0, 0, R4, R4), mode="reflect"), k_col, groups=3)
        return b.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()

    def gather_post():
        ua.ops.augment_u8(x, m, dp, dr0, out=(mid, mout))
        ua.ops.augment_post_u8(mid, dq["everything"], dr, out=out, workspace=ws["everything"])

    fns = {"augment_u8_full": lambda: ua.ops.augment_u8(x, m, dp, dr, out=(out, mout))}
    for k in ("copy", "equalize", "clahe8x8"):
        fns[f"hist_{'none' if k == 'copy' else k}"] = lambda k=k: hist(k)
    for k in recs:
        fns[f"apply_{k}"] = lambda k=k: apply(k, dr if k == "everything" else None)
    eqblur = record(n, op=1, blur=1, R=4).to(dev)
    fns["post_equalize+separable_R4"] = lambda: ua.ops.augment_post_u8(
        x, eqblur, None, out=out, workspace=ws["equalize"])
    fns["gather+post_everything"] = gather_post
    fns["torch_equalize+gaussian_R4"] = torch_composition
    ms = {k: [] for k in fns}
    for fn in fns.values():
        event_ms(fn, 20)
    for _ in range(args.rounds):
        for k, fn in fns.items():
            if k.startswith("apply_"):
                hist(k[6:])         # re-fill: the counts of equalize are what apply reads
            ms[k].append(event_ms(fn, args.calls))
    res = {k: us(v) for k, v in ms.items()}
    res["bytes_in_plus_out"] = 2 * n * hw * hw * 3
    return res


def bench_steps(mode, graphed, batches, dev, args):
    a = Variant("augment", mode, graphed, batches, dev, full_config())
    b = Variant("augment+photometric", mode, graphed, batches, dev, photo_config())
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
        p, r, g = A.sample_params(b.aug.cfg, n, hw, hw, b.aug.generator, return_groups=True)
        q = A.sample_post(b.aug.cfg, n, hw, hw, b.aug.generator, p, r, g)[2]
        A.validate_post(q, hw, hw)
    res["sample_params+post_host_ms"] = (time.perf_counter() - t0) * 1e3 / 50
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
        raise SystemExit("bench_post: no ROCm device (there is nothing to measure on a CPU)")
    dev = torch.device("cuda", 0)
    n, hw = args.batch, args.hw
    batches = host_batches(4, n, hw)
    res = {"tool": "bench_post", "device": torch.cuda.get_device_name(0), "batch": n, "hw": hw,
           "calls": args.calls, "steps": args.steps, "rounds": args.rounds, "warmup": args.warmup}
    print(f"# {res['device']}  batch {n} x {hw}^2")
    x, m = (t.to(dev) for t in batches[0])
    res["kernel"] = bench_kernels(x, m, dev, args)
    print(f"{'call':30s} {'median us':>10s} {'min':>8s} {'max':>8s}")
    for k, v in res["kernel"].items():
        if isinstance(v, dict):
            print(f"{k:30s} {v['median_us']:10.1f} {v['min_us']:8.1f} {v['max_us']:8.1f}",
                  flush=True)
    res["step_ms"] = {}
    print(f"{'mode':6s} {'step':6s} {'input':20s} {'median ms':>10s} {'min':>8s} {'max':>8s}")
    for mode in [s for s in args.modes.split(",") if s]:
        for graphed in (False, True):
            r = bench_steps(mode, graphed, batches, dev, args)
            kind = "graph" if graphed else "eager"
            res["step_ms"][f"{mode}/{kind}"] = r
            for name in ("augment", "augment+photometric"):
                v = r[name]
                print(f"{mode:6s} {kind:6s} {name:20s} {v['median_ms']:10.3f} {v['min_ms']:8.3f} "
                      f"{v['max_ms']:8.3f}", flush=True)
            print(f"{'':13s} sample_params + sample_post + validate_post on the host: "
                  f"{r['sample_params+post_host_ms']:.3f} ms / batch")
            torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
