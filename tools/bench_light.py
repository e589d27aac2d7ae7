#!/usr/bin/env python3
"""What the third augmentation stage (ISO noise, shadow / sun flare / fog) costs on one MI355X, at
the flagship batch (8 x 512^2 by default).  Device events around `--calls` calls behind a
warm-up, medians of `--rounds`, as tools/bench_post.py:

  1. the statistics half (`unet_augment_light_stats`: the memset of the sums and the statistics
     kernel) with ISO noise on every sample, and with it on none (every workgroup returns at
     once).
  2. the apply half (`unet_augment_light_apply`) per mode: copy only, ISO noise, shadow (two
     polygons), sun flare (10 circles, T = 40), fog with 50 and with 105 points and a box of 5,
     ISO + fog, on a workspace the statistics half filled for that record.
  3. gather + post + light against gather + post (bench_post's "everything" record), re-measured
     in this process, and the composition a user would write with PyTorch for the fog (a masked
     blend per point, then `avg_pool2d` behind a reflecting pad).
  4. `train_step` fed uint8 batches from pinned host memory with `BatchAugment` without and with
     a lighting configuration, alternated in one process, fp32 and bf16, eager and as
     `GraphedTrainStep` replays.

Prints a table and one JSON line; `--out FILE` also writes the JSON there.

    python tools/bench_light.py [--batch 8] [--hw 512] [--calls 100] [--steps 20] [--rounds 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import unet_implementations_amd as ua  # noqa: E402
from bench_augment import event_ms, full_config, host_batches, summary  # noqa: E402
from bench_distort import Variant, us  # noqa: E402
from bench_post import record as post_record  # noqa: E402

A = ua.augment


def light_config():
    """bench_augment's full record with ISO noise and a lighting member on every sample (the
    reference file's member probabilities and limits; the default source radius of 400)"""
    return ua.AugmentConfig(**{
        **vars(full_config()), "iso_noise_prob": 1.0, "iso_color_shift": (0.01, 0.05),
        "iso_intensity": (0.1, 0.5), "lighting_group_prob": 1.0, "shadow_prob": 0.3,
        "sunflare_prob": 0.2, "fog_prob": 0.2, "fog_coef": (0.1, 0.3), "fog_alpha_coef": 0.08})


def record(n, hw, iso=False, mode=0, points=0, seed=0):
    g = np.random.default_rng(seed)
    q = A.identity_light(n).numpy()
    if iso:
        q[:, A.L_ISO], q[:, A.L_SIGMA_H], q[:, A.L_INTENSITY] = 1, 3.0, 0.3
    q[:, A.L_MODE] = mode
    for i in range(n):
        if mode == A.LIGHT_SHADOW:
            q[i, A.L_COUNT] = 2
            q[i, A.L_BODY:A.L_BODY + 20] = g.integers(0, hw + 1, 20)
        elif mode == A.LIGHT_FLARE:
            q[i, A.L_COUNT], q[i, A.L_SRC_RADIUS], q[i, A.L_STEPS] = 10, 400, 40
            q[i, A.L_SRC_X], q[i, A.L_SRC_Y] = g.integers(0, hw, 2)
            for c in range(10):
                q[i, A.L_BODY + 7 * c:A.L_BODY + 7 * c + 7] = [
                    g.integers(0, hw), g.integers(0, hw), g.integers(1, 4), g.uniform(0.05, 0.2),
                    *g.integers(205, 256, 3)]
        elif mode == A.LIGHT_FOG:
            q[i, A.L_COUNT], q[i, A.L_FOG_RADIUS], q[i, A.L_FOG_ALPHA] = points, 25, 0.016
            q[i, A.L_FOG_BOX] = 5
            q[i, A.L_BODY:A.L_BODY + 2 * points] = g.integers(0, hw, 2 * points)
    return torch.from_numpy(q)


def bench_kernels(x, m, dev, args):
    n, hw = x.shape[0], x.shape[1]
    lib, stream = ua.lib(), ua.ops._stream
    p, r = A.sample_params(full_config(), n, hw, hw, torch.Generator().manual_seed(1))
    dp, dr = p.to(dev), A.pack_rng(r).to(dev)
    r0 = r.clone()
    r0[:, 2:] = 0
    dr0 = A.pack_rng(r0).to(dev)
    recs = {"copy": record(n, hw), "iso": record(n, hw, iso=True),
            "shadow_2": record(n, hw, mode=A.LIGHT_SHADOW),
            "flare_10_T40": record(n, hw, mode=A.LIGHT_FLARE),
            "fog_P50_k5": record(n, hw, mode=A.LIGHT_FOG, points=50),
            "fog_P105_k5": record(n, hw, mode=A.LIGHT_FOG, points=105),
            "iso+fog_P105_k5": record(n, hw, iso=True, mode=A.LIGHT_FOG, points=105)}
    for q in recs.values():
        A.validate_light(q, hw, hw)
    dq = {k: v.to(dev) for k, v in recs.items()}
    need = lib.unet_augment_light_workspace_bytes(n)
    ws = {k: torch.empty(need, dtype=torch.uint8, device=dev) for k in recs}
    mid, mid2 = torch.empty_like(x), torch.empty_like(x)
    out, mout = torch.empty_like(x), torch.empty_like(m)
    post = post_record(n, hsv=True, op=2, blur=1, R=4).to(dev)
    post_ws = torch.empty(lib.unet_augment_post_workspace_bytes(n), dtype=torch.uint8, device=dev)

    def stats(k):
        ua._lib.check(lib.unet_augment_light_stats(x.data_ptr(), dq[k].data_ptr(),
                                                   ws[k].data_ptr(), need, n, hw, hw, stream()))

    def apply(k):
        ua._lib.check(lib.unet_augment_light_apply(
            x.data_ptr(), out.data_ptr(), dq[k].data_ptr(), dr.data_ptr(), ws[k].data_ptr(),
            need, n, hw, hw, stream()))

    for k in recs:
        stats(k)
    pts = recs["fog_P50_k5"][:, A.L_BODY:A.L_BODY + 100].reshape(n, 50, 2).to(dev)
    jj = torch.arange(hw, device=dev, dtype=torch.float32).view(1, 1, hw)
    ii = torch.arange(hw, device=dev, dtype=torch.float32).view(1, hw, 1)

    def torch_fog():
        o = x.float()
        for k in range(50):
            inside = (jj - pts[:, k, 0].view(n, 1, 1)) ** 2 + \
                (ii - pts[:, k, 1].view(n, 1, 1)) ** 2 <= 625.0
            o = torch.where(inside.unsqueeze(-1), (0.016 * 255 + 0.984 * o).round(), o)
        b = F.avg_pool2d(F.pad(o.permute(0, 3, 1, 2), (2, 2, 2, 2), mode="reflect"), 5, stride=1)
        return b.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()

    def gather_post(dst):
        ua.ops.augment_u8(x, m, dp, dr0, out=(mid, mout))
        ua.ops.augment_post_u8(mid, post, dr, out=dst, workspace=post_ws)

    def gather_post_light(k):
        gather_post(mid2)
        ua.ops.augment_light_u8(mid2, dq[k], dr, out=out, workspace=ws[k])

    fns = {"stats_iso": lambda: stats("iso"), "stats_none": lambda: stats("copy")}
    for k in recs:
        fns[f"apply_{k}"] = lambda k=k: apply(k)
    fns["gather+post_everything"] = lambda: gather_post(out)
    fns["gather+post+light_iso+fog"] = lambda: gather_post_light("iso+fog_P105_k5")
    fns["gather+post+light_flare"] = lambda: gather_post_light("flare_10_T40")
    fns["torch_fog_P50_k5"] = torch_fog
    ms = {k: [] for k in fns}
    for fn in fns.values():
        event_ms(fn, 20)
    for _ in range(args.rounds):
        for k, fn in fns.items():
            if k.startswith("apply_"):
                stats(k[6:])        # re-fill: the sums are what apply reads
            ms[k].append(event_ms(fn, args.calls))
    res = {k: us(v) for k, v in ms.items()}
    res["bytes_in_plus_out"] = 2 * n * hw * hw * 3
    return res


def bench_steps(mode, graphed, batches, dev, args):
    a = Variant("augment", mode, graphed, batches, dev, full_config())
    b = Variant("augment+lighting", mode, graphed, batches, dev, light_config())
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
        A.sample_params(b.aug.cfg, n, hw, hw, b.aug.generator)
        A.sample_light(b.aug.cfg, n, hw, hw, b.aug.generator)
    res["sample_params+light_host_ms"] = (time.perf_counter() - t0) * 1e3 / 50
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
        raise SystemExit("bench_light: no ROCm device (there is nothing to measure on a CPU)")
    dev = torch.device("cuda", 0)
    n, hw = args.batch, args.hw
    batches = host_batches(4, n, hw)
    res = {"tool": "bench_light", "device": torch.cuda.get_device_name(0), "batch": n, "hw": hw,
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
            for name in ("augment", "augment+lighting"):
                v = r[name]
                print(f"{mode:6s} {kind:6s} {name:20s} {v['median_ms']:10.3f} {v['min_ms']:8.3f} "
                      f"{v['max_ms']:8.3f}", flush=True)
            print(f"{'':13s} sample_params + sample_light (validated) on the host: "
                  f"{r['sample_params+light_host_ms']:.3f} ms / batch")
            torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
