#!/usr/bin/env python3
"""Evaluation pictures on one MI355X: the fused render kernels against the composition that was
available before them, at 8 x 512^2.

Workload: the three segmentation figures of evaluate_model (image | gt | pred, image | conf0..2,
image | gt | pred | error) from one batch's normalised image, logits and int64 mask, and the
autoencoder's comparison picture (original | reconstruction | error map).
  fused        `ops.render_seg_panels` (one launch per figure) / `ops.render_recon_panels` (two).
  composition  `ops.eval_maps` for softmax / argmax / error category, then torch on the device:
               the denormalisation in float64, table look-ups by indexing, `where`, shifts and
               `cat` - what a user could write without the render kernels.  Same bytes out.
The two are timed in alternation (device events around `steps` calls, median of `reps`), after
their pictures were compared.  Bytes per second are the algorithmic bytes of the fused form - every
operand read once per launch that needs it, every picture byte written once - against the
achievable HBM rate of a float4 copy on this chip (6.29 TB/s measured, 8 TB/s specified).

    python tools/bench_render.py [--batch 8] [--hw 512] [--steps 50] [--reps 7] [--out PATH]
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
from unet_implementations_amd import render  # noqa: E402

DEV = torch.device("cuda", 0)
HBM_ACHIEVABLE = 6.29e12
FIGURES = {"predictions": render.PREDICTION_PANELS, "confidence": render.CONFIDENCE_PANELS,
           "errors": render.ERROR_PANELS}


class Composition:
    """The same pictures from ops.eval_maps and torch indexing on the device."""

    def __init__(self):
        self.jet = torch.from_numpy(render.jet_lut()).to(DEV)
        self.palette = torch.tensor([[0, 0, 0], [255, 0, 0], [0, 255, 0]], dtype=torch.uint8,
                                    device=DEV)
        self.err = torch.tensor([[0, 0, 0], [0, 255, 0], [255, 0, 0], [0, 0, 255], [255, 255, 0]],
                                dtype=torch.uint8, device=DEV)
        self.mean = torch.tensor(ua.ops.IMAGENET_MEAN, dtype=torch.float64, device=DEV)
        self.std = torch.tensor(ua.ops.IMAGENET_STD, dtype=torch.float64, device=DEV)

    def image(self, images):
        x = images.permute(0, 2, 3, 1).double() * self.std + self.mean
        return (x.clamp(0, 1) * 255).to(torch.uint8)

    @staticmethod
    def blend(img, colour):
        return ((img.to(torch.int16) + colour.to(torch.int16)) >> 1).to(torch.uint8)

    def seg(self, images, logits, masks, panels):
        img = self.image(images)
        need_p = any(p.startswith("conf") for p in panels)
        probs, classes, errors = ua.ops.eval_maps(logits, masks, want_probs=need_p,
                                                  want_classes="pred" in panels,
                                                  want_errors="error" in panels)
        tiles = []
        for p in panels:
            if p == "image":
                tiles.append(img)
            elif p == "gt":
                tiles.append(self.palette[torch.where(masks > 2, 0, masks)])
            elif p == "pred":
                tiles.append(self.palette[classes.long()])
            elif p == "error":
                tiles.append(self.blend(img, self.err[errors.long()]))
            else:
                idx = (probs[:, int(p[4])] * 256).long().clamp(max=255)
                tiles.append(self.blend(img, self.jet[idx]))
        return torch.stack(tiles, dim=2)

    def recon(self, original, recon):
        o = (original.clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1)
        r = (recon.clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1)
        d = (o.float() - r.float()).abs()
        m = d.amax(dim=(1, 2, 3), keepdim=True)
        e = torch.where(m > 0, d / m * 255, torch.zeros_like(d)).to(torch.uint8).long()
        gray = (4899 * e[..., 0] + 9617 * e[..., 1] + 1868 * e[..., 2] + 8192) >> 14
        return torch.stack([o, r, self.jet[gray]], dim=2)


def timed_pair(fused, composed, steps, reps):
    """Median ms per call of the two, timed in alternation."""
    for _ in range(5):
        fused()
        composed()
    torch.cuda.synchronize()
    tf, tc = [], []
    for _ in range(reps):
        for fn, acc in ((fused, tf), (composed, tc)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            acc.append(e0.elapsed_time(e1) / steps)
    return statistics.median(tf), statistics.median(tc), [min(tf), max(tf)], [min(tc), max(tc)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--hw", type=int, default=512)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_render.py needs an MI355X (no CPU fallback exists)")
    B, hw = args.batch, args.hw
    g = torch.Generator().manual_seed(0)
    images = torch.randn(B, 3, hw, hw, generator=g).to(DEV)
    logits = (torch.randn(B, 3, hw, hw, generator=g) * 2).to(DEV)
    masks = torch.randint(0, 3, (B, hw, hw), generator=g)
    masks[:, hw // 2 - 2: hw // 2 + 2] = 255
    masks = masks.to(DEV)
    original = torch.rand(B, 3, hw, hw, generator=g).to(DEV)
    recon = (original + 0.05 * torch.randn(B, 3, hw, hw, generator=g).to(DEV)).contiguous()
    comp = Composition()
    px = B * hw * hw
    result = {"batch": B, "hw": hw, "steps": args.steps, "reps": args.reps,
              "device": torch.cuda.get_device_name(0), "hbm_achievable_TBps": HBM_ACHIEVABLE / 1e12}

    def record(name, fused, composed, nbytes):
        a, b = fused(), composed()
        same = bool(torch.equal(a, b))
        diff = int((a != b).sum().item())
        f_ms, c_ms, f_spread, c_spread = timed_pair(fused, composed, args.steps, args.reps)
        result[name] = {"fused_ms": f_ms, "composition_ms": c_ms, "composition_over_fused": c_ms / f_ms,
                        "fused_spread_ms": f_spread, "composition_spread_ms": c_spread,
                        "pictures_equal": same, "bytes_that_differ": diff,
                        "fused_algorithmic_bytes": nbytes,
                        "fused_TBps": nbytes / (f_ms * 1e-3) / 1e12,
                        "fused_share_of_achievable_hbm": nbytes / (f_ms * 1e-3) / HBM_ACHIEVABLE}

    for name, panels in FIGURES.items():
        need_mask = any(p in ("gt", "error") for p in panels)
        nbytes = px * (12 + 12 + (8 if need_mask else 0) + 3 * len(panels))
        m = masks if need_mask else None
        record(name, lambda: ua.ops.render_seg_panels(images, logits, m, panels=panels),
               lambda: comp.seg(images, logits, masks, panels), nbytes)
    # comparison picture: both images read by the maximum pass and again by the render pass
    record("comparison", lambda: ua.ops.render_recon_panels(original, recon),
           lambda: comp.recon(original, recon), px * (24 + 24 + 27))
    for k in ("fused_ms", "composition_ms"):
        result["all_four_" + k] = sum(result[n][k] for n in list(FIGURES) + ["comparison"])
    result["all_four_composition_over_fused"] = result["all_four_composition_ms"] / \
        result["all_four_fused_ms"]
    line = json.dumps(result)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
