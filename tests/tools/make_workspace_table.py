"""Writes tests/data/workspace_bytes.json: what every `unet_*_workspace_bytes` export of a library
answers over a grid of arguments.  No GPU needed.

The table pins the workspace sizes of csrc/: each multi-region workspace is described by one
layout function that both measures and carves it (csrc/ws_layout.h), and
tests/test_workspace_layout_cpu.py asserts that the library under test answers every row alike.
Callers size their buffers by these numbers, so a changed row is a changed layout.  Regenerate it
only from a library whose sizes are the ones to keep, e.g. a build of the parent commit:

    make -C unet-implementations_amd/csrc BUILD=build_parent OUT=../libunet_parent.so   (in a worktree)
    UNET_HIP_LIB=<that library> python tests/tools/make_workspace_table.py

One list of rows per export, each row the export's arguments followed by the bytes it returned.
Every grid holds the bench shapes (N = 8, 512 x 512 and each stage resolution down to 16 x 16,
32..512 channels, 2..32 classes), the smallest accepted arguments and arguments one off the edge of
what the export accepts, which answer 0.  (The weight-gradient exports have a table of their own,
tests/data/wgrad_workspace_bytes.json; here they ride along at the bench shapes, which is where the
fold workspaces sit on top of them.)"""
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TABLE = os.path.join(ROOT, "tests", "data", "workspace_bytes.json")

BATCHES = (1, 2, 8)
SIDES = (512, 256, 128, 64, 32, 16)              # the stage resolutions of the 512 x 512 net
STAGES = ((512, 32), (256, 64), (128, 128), (64, 256), (32, 512), (16, 512))   # (side, channels)
CHANNELS = (32, 64, 128, 256, 512)
CLASSES = (2, 3, 4, 5, 21, 32)
ODD = ((1, 1), (4, 4), (3, 5), (17, 23), (100, 60))      # (H, W) off the tile sizes


def _hw():
    return [(s, s) for s in SIDES] + list(ODD)


def _product(*axes):
    return [list(t) for t in itertools.product(*axes)]


def _flat(rows):
    """[(a, (h, w), c)] -> [[a, h, w, c]]"""
    return [[x for part in r for x in (part if isinstance(part, tuple) else (part,))] for r in rows]


def grids():
    """{export: [argument lists]} in table order."""
    hw = _hw()
    g = {}
    # (N, HW, C): C a multiple of 4 (the InstanceNorm kernels hold four channels a lane)
    g["unet_instnorm_workspace_bytes"] = (
        _product(BATCHES, [h * w for h, w in hw], (4, 8) + CHANNELS + (1024,)) +
        [[0, 64, 32], [-1, 64, 32], [1, 0, 32], [1, 64, 0], [1, 64, -4]])
    g["unet_conv_in_fwd_workspace_bytes"] = (
        _flat(itertools.product(BATCHES, hw, CHANNELS, (1, 2))) +
        [[0, 16, 16, 32, 1], [1, 0, 16, 32, 1], [1, 16, 0, 32, 1], [1, 16, 16, 0, 1],
         [1, 16, 16, 32, 0], [1, 16, 16, -32, 1]])
    g["unet_head1x1_bwd_workspace_bytes"] = (
        _product(BATCHES, [h * w for h, w in hw], (32,), (1,) + CLASSES) +
        [[0, 64, 32, 3], [1, 0, 32, 3], [-1, 64, 32, 3]])
    g["unet_head1x1_in_bwd_fold_workspace_bytes"] = (
        _product(BATCHES, [h * w for h, w in hw], (1,) + CLASSES) +
        [[0, 64, 3], [1, 0, 3], [1, -64, 3]])
    g["unet_stem_in_bwd_weight_fold_workspace_bytes"] = (
        _flat(itertools.product(BATCHES, [(s, s) for s in SIDES] + [(4, 128), (24, 40)],
                                (32, 64))) +
        [[0, 16, 128, 32], [1, 0, 128, 32], [1, 16, 0, 32], [1, 16, 128, 0]])
    g["unet_conv_in_bwd_weight_fold32_workspace_bytes"] = (
        _flat(itertools.product(BATCHES, [(s, s) for s in SIDES] + [(4, 4), (24, 40)])) +
        [[0, 16, 16], [1, 0, 16], [1, 16, 0]])
    g["unet_conv3x3_bwd_weight_workspace_bytes"] = (
        [[8, 512, 512, 3, 32, 1]] +
        [[8, s, s, c, c, 1] for s, c in STAGES] +
        [[8, s, s, c // 2, c, 2] for s, c in STAGES[:-1] if c >= 64] +
        [[1, 4, 4, 32, 32, 1], [0, 4, 4, 32, 32, 1], [1, 4, 4, 0, 32, 1], [1, 4, 4, 32, 0, 1]])
    g["unet_conv3x3_up_bwd_weight_workspace_bytes"] = (
        [[8, s, s, 2 * c if c < 512 else c, c] for s, c in STAGES[1:]] +
        [[1, 4, 4, 32, 32], [0, 4, 4, 32, 32], [1, 0, 4, 32, 32], [1, 4, 4, 0, 32]])
    g["unet_dice_wce_loss_workspace_bytes"] = (
        _flat(itertools.product(BATCHES + (4096,), hw)) + [[0, 16, 16], [-1, 16, 16]])
    g["unet_dice_wce_lossk_workspace_bytes"] = (
        _flat(itertools.product(BATCHES, CLASSES, ((512, 512), (16, 16), (1, 1), (17, 23)))) +
        [[0, 3, 16, 16], [1, 1, 16, 16], [1, 33, 16, 16], [1, 0, 16, 16]])
    g["unet_cc_workspace_bytes"] = (
        _flat(itertools.product(BATCHES + (65535,), hw)) +
        [[1, 16384, 16384], [0, 16, 16], [65536, 16, 16], [1, 0, 16], [1, 16, 0],
         [1, 16385, 16], [1, 16, 16385], [1, 16384, 16384 * 4 + 1]])
    g["unet_mask_cleanup_workspace_bytes"] = (
        _flat(itertools.product(BATCHES, CLASSES, ((512, 512), (16, 16), (1, 1), (17, 23)))) +
        [[65535, 3, 4, 4], [0, 3, 16, 16], [65536, 3, 16, 16], [1, 1, 16, 16], [1, 33, 16, 16],
         [1, 3, 0, 16], [1, 3, 16, 16385]])
    g["unet_augment_post_workspace_bytes"] = [[n] for n in (1, 2, 8, 32, 1000, 0, -1)]
    g["unet_augment_light_workspace_bytes"] = [[n] for n in (1, 2, 8, 32, 1000, 0, -1)]
    g["unet_gradcam_workspace_bytes"] = (
        _product(BATCHES + (65535,), [h * w for h, w in hw], (4, 8) + CHANNELS + (1024,)) +
        [[0, 64, 32], [65536, 64, 32], [1, 0, 32], [1, 64, 0], [1, 64, 2], [1, 64, 48],
         [1, 64, 96], [1, 64, 2048], [1, (1 << 30) + 1, 32]])
    g["unet_recon3x3_bwd_workspace_bytes"] = (
        _flat(itertools.product(BATCHES, hw)) + [[0, 16, 16], [1, 0, 16], [1, 16, 0]])
    g["unet_mse_loss_workspace_bytes"] = (
        _flat(itertools.product(BATCHES, (1, 3), hw)) +
        [[0, 3, 16, 16], [1, 0, 16, 16], [1, 3, 0, 16], [1, 3, 16, 0]])
    g["unet_ssim_workspace_bytes"] = (
        _flat(itertools.product(BATCHES, (1, 3), hw)) +
        [[0, 3, 16, 16], [1, 0, 16, 16], [1, 3, 0, 16], [1, 3, 16, 0]])
    g["unet_feature_mse_workspace_bytes"] = (
        _flat(itertools.product(BATCHES, [(s, s) for s in SIDES[1:]] + [(14, 14), (7, 9)],
                                (64, 128, 256, 512))) +
        [[0, 16, 16, 64], [1, 0, 16, 64], [1, 16, 0, 64], [1, 16, 16, 0], [1, 16, 16, 62]])
    g["unet_latent_colsum_workspace_bytes"] = (
        _product((2, 3, 64, 1000, 65536), (4, 32, 512, 2048)) +
        [[1, 32], [0, 32], [65537, 32], [64, 0], [64, 6]])
    g["unet_latent_gram_workspace_bytes"] = (
        _product((2, 3, 64, 1000, 65536), (4, 32, 512, 2048)) +
        [[1, 32], [0, 32], [65537, 32], [64, 0], [64, 6]])
    return g


def rows(lib):
    """{export: [[args..., bytes]]} as `lib` answers now."""
    return {name: [args + [int(getattr(lib, name)(*args))] for args in grid]
            for name, grid in grids().items()}


def main():
    import unet_implementations_amd as ua
    tab = rows(ua.lib())
    os.makedirs(os.path.dirname(TABLE), exist_ok=True)
    with open(TABLE, "w") as f:
        f.write("{\n")
        f.write(",\n".join(
            f' "{name}": [\n' + ",\n".join("  " + json.dumps(r) for r in tab[name]) + "\n ]"
            for name in tab))
        f.write("\n}\n")
    print(f"{TABLE}: " + ", ".join(f"{len(v)} {k[5:-16]}" for k, v in tab.items()))


if __name__ == "__main__":
    main()
