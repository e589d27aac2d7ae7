"""Record tests/golden/clip_extractor.npz through the reference's own ClipPatchExtractor
(CLIP_UNet/models/unet.py of the reference checkout, which needs only torch), wrapped around the
stand-in clip_model of clip_vit_ref.py with the seeded weights of the "fixture" geometry:

    python tests/tools/make_golden_clip_extractor.py --reference /path/to/UNet-Implementations

Recorded: the uint8 NHWC inputs (one 224 x 224 batch, one 96 x 128 batch that takes the resize
branch), the [N, 512] values of the output (grid position (0, 0), where the reference's interpolation
is an exact copy), whether all 256 grid positions were bitwise equal and how far they were apart,
and the pins of the rebuilt weights."""
import argparse
import contextlib
import importlib.util
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import clip_vit_ref as R  # noqa: E402

CASES = {"224": (31, 2, 224, 224), "96x128": (32, 2, 96, 128)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout")
    ap.add_argument("--out", default=os.path.join(HERE, "..", "golden", "clip_extractor.npz"))
    args = ap.parse_args()
    path = os.path.join(args.reference, "CLIP_UNet", "models", "unet.py")
    spec = importlib.util.spec_from_file_location("reference_clip_unet", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    geometry = R.GEOMETRIES["fixture"]
    sd = R.seeded_state_dict(geometry)
    clip_model = R.StandInClip(R.build(geometry))
    with contextlib.redirect_stdout(io.StringIO()):
        extractor = mod.ClipPatchExtractor(clip_model, device="cpu")
    out = {"seed_w": np.int64(R.SEED_W), "feature_dim": np.int64(extractor.feature_dim),
           "grid_size": np.asarray(extractor.grid_size, dtype=np.int64)}
    for tag, (seed, n, h, w) in CASES.items():
        u8 = R.images_u8(seed, n, h, w)
        with contextlib.redirect_stdout(io.StringIO()):
            y = extractor(R.normalise_u8(u8))
        assert tuple(y.shape) == (n, geometry["output_dim"], 16, 16), y.shape
        out[f"u8_{tag}"] = u8
        out[f"embed_{tag}"] = y[:, :, 0, 0].contiguous().numpy()
        # (the reference's interpolation from 1 x 1 blends the one value with itself: w0 v + w1 v
        # is v only up to an fp32 rounding wherever the source coordinate is not clamped)
        out[f"grid_equal_{tag}"] = np.bool_((y == y[:, :, :1, :1]).all().item())
        out[f"grid_max_dev_{tag}"] = np.float64(((y - y[:, :, :1, :1]).abs().max()
                                                 / y.abs().max()).item())
    out.update(R.pin_weights(sd))
    np.savez_compressed(args.out, **out)
    print(args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
