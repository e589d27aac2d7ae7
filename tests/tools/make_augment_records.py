#!/usr/bin/env python3
"""Generates tests/golden/augment_records.npz: the records the four samplers of
`unet_implementations_amd.augment` draw, recorded so that a change to the host side of the
augmentation can be held against the draws of the commit the fixture was made at.

For each seed of SEEDS one CPU generator feeds, in this order, `sample_params(...,
return_groups=True)`, `sample_warp`, `sample_post` and `sample_light` at N = 32, H = 48, W = 64,
two configurations selected by `which = arange(N) % 2`, every transform of `AugmentConfig` on.
The fp32 / int64 tensors and the `applied` and `groups` masks of every call are stored under
"s<seed>/<call>/<name>".  tests/test_augment_records_cpu.py draws the same calls (`records`) and
asserts exact equality.

Usage: python tests/tools/make_augment_records.py [--out PATH]
"""
import argparse
import dataclasses
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SEEDS, N, H, W = (0, 1), 32, 48, 64


def configs(A):
    """The two configurations: the second differs in the flip, the CLAHE grid and the grid steps."""
    c0 = A.AugmentConfig(
        horizontal_flip_prob=0.5,
        shift_scale_rotate_prob=0.7, shift_limit=(-0.1, 0.1), scale_limit=(-0.15, 0.15),
        rotate_limit=(-15.0, 15.0),
        crop_prob=0.5, crop_scale=(0.8, 1.0), crop_ratio=(0.9, 1.1),
        perspective_prob=0.5, perspective_scale=(0.05, 0.1),
        dropout_prob=0.5, dropout_height=(4, 9), dropout_width=(4, 9),
        color_prob=0.9,
        brightness_contrast_prob=0.4, brightness_limit=(-0.2, 0.2), contrast_limit=(-0.5, 0.25),
        rgb_shift_prob=0.3, rgb_shift_limit=(10.0, 12.0, 14.0),
        hsv_prob=0.3, hue_shift_limit=20.0, sat_shift_limit=30.0, val_shift_limit=20.0,
        gray_group_prob=0.9, to_gray_prob=0.3,
        clahe_prob=0.4, clahe_clip_limit=4.0, clahe_tile_grid=(4, 4), equalize_prob=0.3,
        noise_group_prob=0.9, gauss_noise_prob=0.3, gauss_var_limit=(4.0, 18.0),
        gaussian_blur_prob=0.4, gaussian_blur_limit=(3, 7),
        motion_blur_prob=0.3, motion_blur_limit=(3, 7),
        salt_pepper_prob=0.5, salt_p=(0.01, 0.05), pepper_p=(0.01, 0.05),
        distort_group_prob=0.9,
        elastic_prob=0.4, elastic_alpha=3.0, elastic_sigma=2.0, elastic_alpha_affine=2.0,
        grid_distortion_prob=0.3, grid_num_steps=5, grid_distort_limit=0.3,
        optical_distortion_prob=0.3, optical_distort_limit=0.05, optical_shift_limit=0.05,
        iso_noise_prob=0.5, iso_color_shift=(0.01, 0.05), iso_intensity=(0.1, 0.5),
        lighting_group_prob=0.9, shadow_prob=0.3,
        sunflare_prob=0.3, sunflare_src_radius=100,
        fog_prob=0.4, fog_coef=(0.3, 0.8), fog_alpha_coef=0.08)
    c1 = dataclasses.replace(c0, horizontal_flip_prob=1.0, clahe_tile_grid=(2, 8),
                             grid_num_steps=3)
    return [c0, c1]


def records(A, seed):
    """{"<call>/<name>": array} of the four sampler calls from one generator seeded `seed`."""
    cfg, which = configs(A), torch.arange(N) % 2
    gen = torch.Generator()
    gen.manual_seed(seed)
    out = {}

    def put(call, **arrays):
        for name, a in arrays.items():
            out[f"{call}/{name}"] = a.numpy() if torch.is_tensor(a) else np.asarray(a)

    p, r, applied, groups = A.sample_params(cfg, N, H, W, gen, which=which, return_applied=True,
                                            return_groups=True)
    put("params", params=p, rng=r, **{"applied_" + k: v for k, v in applied.items()},
        **{"group_" + k: v for k, v in groups.items()})
    w, applied = A.sample_warp(cfg, N, H, W, gen, which=which, return_applied=True)
    put("warp", warp=w, **{"applied_" + k: v for k, v in applied.items()})
    p2, r2, q, applied = A.sample_post(cfg, N, H, W, gen, p, r, groups, which=which,
                                       return_applied=True)
    put("post", params=p2, rng=r2, post=q, **{"applied_" + k: v for k, v in applied.items()})
    lt, applied = A.sample_light(cfg, N, H, W, gen, which=which, return_applied=True)
    put("light", light=lt, **{"applied_" + k: v for k, v in applied.items()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "augment_records.npz"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import unet_implementations_amd as ua
    blob = {}
    for seed in SEEDS:
        for key, a in records(ua.augment, seed).items():
            blob[f"s{seed}/{key}"] = a
    fired = {k: int(a.sum()) for k, a in blob.items() if "/applied_" in k}
    print(f"{len(blob)} arrays; fewest samples a member fires for: {min(fired.values())} "
          f"({min(fired, key=fired.get)})")
    np.savez_compressed(args.out, **blob)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
