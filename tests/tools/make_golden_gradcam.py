#!/usr/bin/env python3
"""Generates tests/golden/gradcam.npz by running the REFERENCE's Grad-CAM helper on CPU.

Runs only in the build container (needs the reference checkout).  Loads
`Our_UNet/models/unet.py` and `Our_UNet/utils/visualize.py` by file path (matplotlib on the Agg
backend) and calls the reference's own `generate_gradcam_heatmap`, one image at a time, on the
reference UNet in float64 and again in float32, for every case of gradcam_inputs.CASES.

The fixture holds: the seeds, a SHA-256 of the regenerated weights and images, and per case the
float64 heatmaps rounded to float32 (`heat_<case>` [n, H, W]), the minimum and maximum of the
pre-ReLU map in float64 (`premin_<case>`, `premax_<case>` [n]) and `ref32_err_<case>`, the
maximum of |reference float32 - reference float64| over the case.  Data only: nothing from the
reference's source travels.

Usage: python tests/tools/make_golden_gradcam.py [--out PATH] [--reference DIR]
"""
import argparse
import importlib.util
import os
import sys

import matplotlib
matplotlib.use("Agg")
import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import gradcam_inputs as GI  # noqa: E402


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def pre_relu_range(model, x, cls, target):
    """min / max of sum_c w_c A_c BEFORE the ReLU, through the same hooks the reference helper
    registers (it only returns the normalised map)."""
    keep = {}
    h1 = target.register_forward_hook(lambda m, i, o: keep.__setitem__("a", o.detach()))
    h2 = target.register_backward_hook(lambda m, gi, go: keep.__setitem__("g", go[0].detach()))
    model.zero_grad()
    model(x)[0, cls].mean().backward()
    h1.remove()
    h2.remove()
    cam = (keep["g"].mean(dim=(2, 3), keepdim=True) * keep["a"]).sum(dim=1)
    return float(cam.min()), float(cam.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "gradcam.npz"))
    ap.add_argument("--reference", default="/root/reference")
    args = ap.parse_args()
    R = _load("ref_unet_model", os.path.join(args.reference, "Our_UNet", "models", "unet.py"))
    V = _load("ref_unet_visualize", os.path.join(args.reference, "Our_UNet", "utils", "visualize.py"))
    torch.set_num_threads(8)
    cpu = torch.device("cpu")

    sd = GI.state_dict()
    imgs = {name: GI.images(name) for name in GI.BATCHES}
    models = {}
    for dt in (torch.float64, torch.float32):
        m = R.UNet()
        m.load_state_dict(sd)
        models[dt] = m.to(dt).eval()

    out = {"cases": np.array([c[0] for c in GI.CASES]), "weight_seed": np.int64(GI.WEIGHT_SEED),
           "sha256_inputs": GI.digest(sd, imgs)}
    for name, (seed, n, h, w) in GI.BATCHES.items():
        out[f"batch_{name}"] = np.array([seed, n, h, w], dtype=np.int64)
    for name, batch, layer, cls in GI.CASES:
        x = imgs[batch]
        heat = {}
        for dt, m in models.items():
            t = GI.target_module(m, layer)
            heat[dt] = np.stack([V.generate_gradcam_heatmap(m, x[b:b + 1].to(dt), cls, t, cpu)
                                 for b in range(x.shape[0])])
            assert heat[dt].shape == (x.shape[0],) + tuple(x.shape[2:])
        m64 = models[torch.float64]
        rng = [pre_relu_range(m64, x[b:b + 1].double(), cls, GI.target_module(m64, layer))
               for b in range(x.shape[0])]
        out[f"heat_{name}"] = heat[torch.float64].astype(np.float32)
        out[f"premin_{name}"] = np.array([r[0] for r in rng])
        out[f"premax_{name}"] = np.array([r[1] for r in rng])
        err = float(np.abs(heat[torch.float32].astype(np.float64) - heat[torch.float64]).max())
        out[f"ref32_err_{name}"] = np.float64(err)
        zero = [not heat[torch.float64][b].any() for b in range(x.shape[0])]
        print(f"  {name}: ref fp32 vs fp64 {err:.2e}, all-zero maps {zero}, pre-ReLU max "
              + " ".join(f"{r[1]:+.2e}" for r in rng))
        if name == GI.ZERO_CASE:
            # the case that tests the per-image normalisation and the zero guard must keep its
            # shape: zero and non-zero maps in one batch, the zero ones far from the ReLU's edge
            assert any(zero) and not all(zero), zero
            for b, z in enumerate(zero):
                if z:
                    assert rng[b][1] < -0.1 * (rng[b][1] - rng[b][0]), (b, rng[b])
    with open(args.out, "wb") as f:
        np.savez_compressed(f, **dict(sorted(out.items())))
    print(os.path.basename(args.out), "written,", os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
