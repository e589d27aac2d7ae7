"""Writes tests/data/wgrad_workspace_bytes.json: what the weight-gradient workspace queries and
`unet_conv3x3_bwd_weight_is_winograd` of a library answer over a grid of shapes.  No GPU needed.

The table pins the host-side plan selection of csrc/conv_wgrad.hip: tests/test_wgrad_plan_cpu.py
asserts that the library under test answers every row alike.  Regenerate it only from a library
whose selection is the one to keep, e.g. a build of the parent commit beside the product one:

    make -C unet-implementations_amd/csrc BUILD=build_parent OUT=../libunet_parent.so   (in a worktree)
    UNET_HIP_LIB=<that library> python tests/tools/make_wgrad_workspace_table.py

Rows, each shape once with the default 2 GiB chunk limit ("limit": 0) and once with
`unet_debug_set_chunk_limit` lowered to three images' worth, so that N = 8 runs as 3 + 3 + 2:
  conv3x3: [N, H, W, Cx, Cout, stride, limit, bytes, wino] - wino: bit k set when is_winograd
           answers 1 with the thread's c32 switch (unet_set_c32_winograd) at k = 0, 1, 2
  up:      [N, h, w, Cx, Cout, limit, bytes] (Cx = 3 is no operand of the up-sampled form)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TABLE = os.path.join(ROOT, "tests", "data", "wgrad_workspace_bytes.json")

BATCHES = (1, 2, 8, 32)
SIZES = ((4, 4), (8, 16), (16, 24), (24, 40), (64, 64), (256, 192), (512, 512))
CX = (3, 32, 64, 96, 256, 512)
COUT = (32, 64, 96, 128, 512)
STRIDES = (1, 2)


def conv3x3_limit(H, W, Cx, Cout, stride):
    """Chunk limit at which the 3x3 weight gradient takes three images a launch."""
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    return 3 * max(H * W * Cx * 4, Ho * Wo * Cout * 4)


def up_limit(h, w, Cx, Cout):
    return 3 * max(h * w * Cx * 4, h * w * 9 * Cout * 4)


class chunk_limit:
    """`with chunk_limit(lib, nbytes):` - the debug chunk limit lowered (0: left at its default)
    for the block and restored afterwards."""

    def __init__(self, lib, nbytes):
        self.lib, self.nbytes = lib, nbytes

    def __enter__(self):
        if self.nbytes:
            self.lib.unet_debug_set_chunk_limit(self.nbytes)

    def __exit__(self, *exc):
        self.lib.unet_debug_set_chunk_limit(0)
        return False


def conv3x3_rows(lib):
    """Yields ([N, H, W, Cx, Cout, stride, limit], bytes, wino) in table order."""
    for H, W in SIZES:
        for Cx in CX:
            for Cout in COUT:
                for stride in STRIDES:
                    for limit in (0, conv3x3_limit(H, W, Cx, Cout, stride)):
                        with chunk_limit(lib, limit):
                            for N in BATCHES:
                                nbytes = lib.unet_conv3x3_bwd_weight_workspace_bytes(
                                    N, H, W, Cx, Cout, stride)
                                wino = 0
                                for k in (0, 1, 2):
                                    prev = lib.unet_set_c32_winograd(k)
                                    wino |= lib.unet_conv3x3_bwd_weight_is_winograd(
                                        N, H, W, Cx, Cout, stride) << k
                                    lib.unet_set_c32_winograd(prev)
                                yield [N, H, W, Cx, Cout, stride, limit], nbytes, wino


def up_rows(lib):
    """Yields ([N, h, w, Cx, Cout, limit], bytes) in table order."""
    for h, w in SIZES:
        for Cx in CX[1:]:
            for Cout in COUT:
                for limit in (0, up_limit(h, w, Cx, Cout)):
                    with chunk_limit(lib, limit):
                        for N in BATCHES:
                            yield [N, h, w, Cx, Cout, limit], \
                                lib.unet_conv3x3_up_bwd_weight_workspace_bytes(N, h, w, Cx, Cout)


def main():
    import unet_implementations_amd as ua
    lib = ua.lib()
    conv = [key + [nbytes, wino] for key, nbytes, wino in conv3x3_rows(lib)]
    up = [key + [nbytes] for key, nbytes in up_rows(lib)]
    os.makedirs(os.path.dirname(TABLE), exist_ok=True)
    with open(TABLE, "w") as f:
        f.write('{"conv3x3": [\n')
        f.write(",\n".join("  " + json.dumps(r) for r in conv))
        f.write('\n ],\n "up": [\n')
        f.write(",\n".join("  " + json.dumps(r) for r in up))
        f.write("\n ]\n}\n")
    print(f"{TABLE}: {len(conv)} conv3x3 rows, {len(up)} up rows")


if __name__ == "__main__":
    main()
