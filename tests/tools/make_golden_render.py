#!/usr/bin/env python3
"""Generates tests/golden/render.npz by running the REFERENCE's figure code on CPU.

Runs only in the build container (needs the reference checkout and matplotlib, which
`Our_UNet/utils/visualize.py` imports).  Loads that module by file path, selects the Agg backend,
and calls its own `visualize_error_analysis_batch` with a stub network that returns prepared
logits.  Two hooks record what the function computes before it draws: `Axes.imshow` (the four
tiles of every row: the denormalised image of :274-276 as float64, `colorize_mask` of the mask and
of the argmax, the blended error picture) and the module's `create_error_visualization` (its third
argument is the uint8 image of :277).

The fixture holds the inputs of render_ref.make_seg_case(SEED, 2, 12, 20) (normalised image,
logits, mask) and those recorded outputs.  Data only: nothing from the reference's source travels.
The autoencoder's visualize.py imports cv2 and sklearn, which are not installed: its panels are
not recorded (tests/golden/render.md).

Usage: python tests/tools/make_golden_render.py [--out PATH] [--reference DIR]
"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import render_ref as R  # noqa: E402

SEED, B, H, W = 20240, 2, 12, 20


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Stub(torch.nn.Module):
    """The stub network: returns the prepared logits whatever the image is."""

    def __init__(self, logits):
        super().__init__()
        self.logits = logits

    def forward(self, x):
        return self.logits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "render.npz"))
    ap.add_argument("--reference", default="/root/reference")
    args = ap.parse_args()
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.axes
    import matplotlib.pyplot as plt
    V = _load("ref_unet_visualize", os.path.join(args.reference, "Our_UNet", "utils", "visualize.py"))

    _, image, logits, mask = R.make_seg_case(SEED, B, H, W)
    shown, bytes_in = [], []
    real_imshow, real_error = matplotlib.axes.Axes.imshow, V.create_error_visualization

    def imshow(self, X, *a, **k):
        shown.append(np.array(X))
        return real_imshow(self, X, *a, **k)

    def create_error_visualization(pred_mask, gt_mask, original_img):
        bytes_in.append(np.array(original_img))
        return real_error(pred_mask, gt_mask, original_img)

    matplotlib.axes.Axes.imshow = imshow
    V.create_error_visualization = create_error_visualization
    try:
        batch = {"image": torch.from_numpy(image), "mask": torch.from_numpy(mask)}
        V.visualize_error_analysis_batch(Stub(torch.from_numpy(logits)), batch, torch.device("cpu"))
    finally:
        matplotlib.axes.Axes.imshow = real_imshow
        V.create_error_visualization = real_error
        plt.close("all")
    assert len(shown) == 4 * B and len(bytes_in) == B
    tiles = [np.stack(shown[k::4]) for k in range(4)]           # image, gt, pred, error
    assert tiles[0].dtype == np.float64 and all(t.dtype == np.uint8 for t in tiles[1:])
    out = {"seed": np.int64(SEED), "image": image, "logits": logits, "mask": mask,
           "ref_image_float": tiles[0], "ref_image_u8": np.stack(bytes_in), "ref_gt": tiles[1],
           "ref_pred": tiles[2], "ref_error": tiles[3]}
    assert out["ref_image_u8"].dtype == np.uint8
    # the restatement reproduces every recorded array
    assert np.array_equal(R.seg_panel("image", image), out["ref_image_u8"])
    assert np.array_equal(R.seg_panel("gt", image, logits, mask), out["ref_gt"])
    assert np.array_equal(R.seg_panel("pred", image, logits, mask), out["ref_pred"])
    assert np.array_equal(R.seg_panel("error", image, logits, mask), out["ref_error"])
    with open(args.out, "wb") as f:
        np.savez_compressed(f, **dict(sorted(out.items())))
    print(os.path.basename(args.out), "written,", os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
