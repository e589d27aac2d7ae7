"""Writes tests/data/conv_host_gpu.json: what the convolution forward / data-gradient entry
points of csrc/conv_igemm.hip do on the GPU over a small grid of calls - per row the demangled
launch list (ops.record_launches), the reported stats_px / tiles_out and a CRC32 of the bytes of
every output the call writes (y / dx / g, the statistics or BSTATS summaries up to the reported
tile count, dx after an accumulate call onto a seeded non-zero dx).
tests/test_conv_host_gpu.py holds the library under test to all three columns, exactly;
tests/test_conv_host_fp64_gpu.py makes the same calls (build_row with coherent weight planes,
call_row) and holds their outputs to the float64 references of tests/tools/conv_host_refs.py.

Inputs come from a seeded CPU generator and these kernels use no atomics, so the outputs are
bit-reproducible: every row runs twice and no table is written when any row differs between its
two runs.  Regenerate it only on an MI355X from a library whose behaviour is the one to keep,
e.g. a build of the parent commit beside the product one:

    make -C unet-implementations_amd/csrc BUILD=build_parent OUT=../libunet_parent.so
    UNET_HIP_LIB=<that library> python tests/tools/make_conv_host_gpu_table.py

A row is a dict: "fn" the export, "fam" the test it belongs to, the shape, and
  lim   chunk limit in images of the chunked tensor (N = 8 then runs as 3 + 3 + 2)
  c32   setting of unet_set_c32_winograd for the call
  bs    "ok" (a complete unet_bwd_stats), "short" (partial_bytes one byte short) or absent
  act   which sources carry activation coefficients ("01", "0", "1", "")
  w3    0: the optional bf16 weight plane is null
Shapes are the smallest that select each form (thresholds of 256 / 512 tiles are crossed with
wide outputs of few input channels, not with the 512 x 512 workload)."""
import ctypes
import importlib.util
import json
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TABLE = os.path.join(ROOT, "tests", "data", "conv_host_gpu.json")


def _load(name):
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(ROOT, "tests", "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


T = _load("make_conv_host_table")
B16 = set(T.ES) | {"unet_conv_up_in_fwd_b16", "unet_stem_u8_fwd_b16",
                   "unet_conv_in_stats_finalize_b16"}
ONE_PLANE = {"unet_conv3x3_bwd_data_bs_b16_wb", "unet_conv_in_fwd_b16_wb",
             "unet_conv3x3_up_bwd_data_bs_b16_wb", "unet_conv_up_in_fwd_b16"}


def R(fam, fn, **kw):
    return dict(fam=fam, fn="unet_" + fn, **kw)


def _rows():
    rows = []
    # ---- plain forward: stem in its three width classes, row-fused, patch, gather-GEMM forms
    for fn in ("conv3x3_fwd", "conv3x3_fwd_bf16", "conv3x3_fwd_bf16x3"):
        rows += [R("fwd", fn, N=2, H=6, W=40, C0=3, Cout=32),
                 R("fwd", fn, N=2, H=6, W=128, C0=3, Cout=32),
                 R("fwd", fn, N=2, H=8, W=128, C0=3, Cout=64),
                 R("fwd", fn, N=2, H=5, W=7, C0=32, Cout=32),
                 R("fwd", fn, N=2, H=9, W=7, C0=32, C1=32, Cout=32, stride=2),
                 R("fwd", fn, N=2, H=8, W=8, C0=64, Cout=64),
                 R("fwd", fn, N=1, H=94, W=100, C0=32, Cout=512),
                 R("fwd", fn, N=1, H=94, W=124, C0=32, Cout=192),
                 R("fwd", fn, N=8, H=5, W=7, C0=32, C1=64, Cout=32, lim=3),
                 R("fwd", fn, N=8, H=6, W=8, C0=32, Cout=32, stride=2, lim=3)]
    rows += [R("fwd", "conv3x3_fwd", N=1, H=4, W=128, C0=32, Cout=32),
             R("fwd", "conv3x3_fwd", N=1, H=6, W=128, C0=64, Cout=32),
             R("fwd", "conv3x3_fwd", N=2, H=64, W=128, C0=32, C1=32, Cout=512),
             R("fwd", "conv3x3_fwd", N=2, H=8, W=8, C0=32, Cout=64),
             R("fwd", "conv3x3_fwd", N=2, H=8, W=8, C0=128, Cout=64),
             # split-bf16: narrow image (fp32 kernels), the split patch kernel, the 64-column forms
             R("fwd", "conv3x3_fwd_bf16x3", N=1, H=4, W=32, C0=32, Cout=32),
             R("fwd", "conv3x3_fwd_bf16x3", N=1, H=5, W=33, C0=32, Cout=64),
             R("fwd", "conv3x3_fwd_bf16x3", N=1, H=5, W=33, C0=32, Cout=32)]
    # ---- data gradient, stride 1
    for fn in ("conv3x3_bwd_data", "conv3x3_bwd_data_bf16", "conv3x3_bwd_data_bf16x3",
               "conv3x3_bwd_data_b16"):
        rows += [R("bwd", fn, N=2, H=5, W=7, Cout=32, Ccols=32),
                 R("bwd", fn, N=2, H=8, W=8, Cout=64, Ccols=32, Cin_total=96, ci_offset=64, acc=1),
                 R("bwd", fn, N=2, H=8, W=8, Cout=64, Ccols=64),
                 R("bwd", fn, N=2, H=8, W=12, Cout=32, Ccols=32, stride=2),
                 R("bwd", fn, N=8, H=5, W=7, Cout=64, Ccols=32, Cin_total=64, ci_offset=32, acc=1,
                   lim=3),
                 R("bwd", fn, N=8, H=8, W=12, Cout=32, Ccols=32, stride=2, lim=3)]
    rows += [R("bwd", "conv3x3_bwd_data_bf16", N=1, H=94, W=100, Cout=32, Ccols=512),
             R("bwd", "conv3x3_bwd_data_bf16", N=1, H=94, W=124, Cout=32, Ccols=192),
             R("bwd", "conv3x3_bwd_data_bf16x3", N=1, H=94, W=100, Cout=32, Ccols=512),
             R("bwd", "conv3x3_bwd_data_bf16x3", N=1, H=94, W=124, Cout=32, Ccols=192),
             R("bwd", "conv3x3_bwd_data_bf16x3", N=1, H=4, W=32, Cout=32, Ccols=32),
             R("bwd", "conv3x3_bwd_data_bf16x3", N=1, H=5, W=33, Cout=32, Ccols=64),
             R("bwd", "conv3x3_bwd_data_bf16x3", N=1, H=5, W=33, Cout=32, Ccols=32),
             R("bwd", "conv3x3_bwd_data", N=1, H=94, W=100, Cout=32, Ccols=512),
             R("bwd", "conv3x3_bwd_data", N=1, H=94, W=124, Cout=32, Ccols=192),
             R("bwd", "conv3x3_bwd_data", N=2, H=8, W=8, Cout=32, Ccols=64),
             R("bwd", "conv3x3_bwd_data", N=2, H=8, W=8, Cout=128, Ccols=64),
             R("bwd", "conv3x3_bwd_data", N=2, H=4, W=128, Cout=32, Ccols=32),
             R("bwd", "conv3x3_bwd_data", N=1, H=6, W=128, Cout=64, Ccols=32)]
    # ---- data gradient with the BSTATS epilogue
    for fn in ("conv3x3_bwd_data_bs", "conv3x3_bwd_data_bs_bf16x3", "conv3x3_bwd_data_bs_b16",
               "conv3x3_bwd_data_bs_b16_wb"):
        rows += [
            # gather-GEMM forms: tiles that do not / do lie inside one image
            R("bs", fn, N=2, H=5, W=7, Cout=32, Ccols=32, bs="ok"),
            R("bs", fn, N=2, H=8, W=16, Cout=32, Ccols=32, bs="ok"),
            R("bs", fn, N=2, H=8, W=16, Cout=32, Ccols=32, bs="short"),
            R("bs", fn, N=2, H=8, W=16, Cout=32, Ccols=32),
            R("bs", fn, N=2, H=8, W=8, Cout=64, Ccols=64, bs="ok", acc=1, Cin_total=128,
              ci_offset=64),
            R("bs", fn, N=2, H=8, W=8, Cout=256, Ccols=64, bs="ok"),
            R("bs", fn, N=1, H=576, W=16, Cout=32, Ccols=512, bs="ok"),
            R("bs", fn, N=1, H=688, W=16, Cout=32, Ccols=192, bs="ok"),
            # patch forms (stride 1: 64 and 128 columns; the split kernel's 256-tile floor)
            R("bs", fn, N=2, H=64, W=128, Cout=32, Ccols=512, bs="ok"),
            R("bs", fn, N=1, H=32, W=128, Cout=32, Ccols=512, bs="ok"),
            # 32 -> 32: direct / Winograd by the c32 switch, row-fused where 8 rows do not tile
            R("bs", fn, N=2, H=16, W=64, Cout=32, Ccols=32, bs="ok", c32=0),
            R("bs", fn, N=2, H=16, W=64, Cout=32, Ccols=32, bs="ok", c32=1),
            R("bs", fn, N=2, H=16, W=64, Cout=32, Ccols=32, bs="ok", c32=2),
            R("bs", fn, N=2, H=4, W=128, Cout=32, Ccols=32, bs="ok"),
            R("bs", fn, N=1, H=6, W=128, Cout=64, Ccols=32, bs="ok"),
            R("bs", fn, N=8, H=8, W=16, Cout=32, Ccols=32, bs="ok", lim=3),
            # stride 2: patch, the single-launch four-class form, the four per-class launches
            # (reduction tiles inside / not inside one image)
            R("bs2", fn, N=2, H=64, W=128, Cout=32, Ccols=512, stride=2, bs="ok"),
            R("bs2", fn, N=2, H=64, W=128, Cout=32, Ccols=512, stride=2),
            R("bs2", fn, N=2, H=96, W=96, Cout=32, Ccols=512, stride=2, bs="ok"),
            R("bs2", fn, N=2, H=16, W=32, Cout=32, Ccols=32, stride=2, bs="ok"),
            R("bs2", fn, N=2, H=8, W=12, Cout=32, Ccols=32, stride=2, bs="ok"),
            R("bs2", fn, N=2, H=8, W=12, Cout=32, Ccols=32, stride=2, bs="short", acc=1),
            R("bs2", fn, N=8, H=16, W=32, Cout=32, Ccols=32, stride=2, bs="ok", lim=3)]
    rows += [R("bs", "conv3x3_bwd_data_bs", N=2, H=128, W=512, Cout=32, Ccols=32, bs="ok", c32=1),
             R("bs", "conv3x3_bwd_data_bs_b16_wb", N=2, H=8, W=8, Cout=256, Ccols=64, bs="ok", w3=0),
             R("bs2", "conv3x3_bwd_data_bs_b16_wb", N=2, H=64, W=128, Cout=32, Ccols=512, stride=2,
               bs="ok", w3=0)]
    # ---- 1x1
    rows += [R("c1x1", "conv1x1_fwd", N=2, H=5, W=7, C0=32, C1=32, Cout=32),
             R("c1x1", "conv1x1_fwd", N=2, H=8, W=8, C0=64, Cout=64),
             R("c1x1", "conv1x1_fwd", N=8, H=5, W=7, C0=32, C1=64, Cout=32, lim=3),
             R("c1x1", "conv1x1_bwd_data", N=2, H=5, W=7, Cout=32, Ccols=32),
             R("c1x1", "conv1x1_bwd_data", N=2, H=8, W=8, Cout=64, Ccols=64, Cin_total=128,
               ci_offset=64, acc=1),
             R("c1x1", "conv1x1_bwd_data", N=8, H=5, W=7, Cout=64, Ccols=32, Cin_total=64,
               ci_offset=32, acc=1, lim=3)]
    # ---- fused forward
    for fn in ("conv_in_fwd", "conv_in_fwd_bf16x3", "conv_in_fwd_b16", "conv_in_fwd_b16_wb"):
        rows += [R("in", fn, N=2, H=6, W=40, C0=3, Cout=32, act=""),
                 R("in", fn, N=2, H=6, W=128, C0=3, Cout=32, act=""),
                 R("in", fn, N=2, H=8, W=128, C0=3, Cout=64, act=""),
                 R("in", fn, N=2, H=5, W=7, C0=32, Cout=32),
                 R("in", fn, N=2, H=8, W=8, C0=32, C1=32, Cout=64, act="1"),
                 R("in", fn, N=2, H=8, W=8, C0=32, Cout=64, act=""),
                 R("in", fn, N=2, H=8, W=8, C0=128, Cout=64),
                 R("in", fn, N=2, H=8, W=8, C0=256, Cout=64),
                 R("in", fn, N=2, H=8, W=8, C0=128, Cout=64, stride=2),
                 R("in", fn, N=2, H=16, W=16, C0=32, Cout=64, stride=2),
                 R("in", fn, N=1, H=576, W=16, C0=32, Cout=512),
                 R("in", fn, N=1, H=688, W=16, C0=32, Cout=192),
                 R("in", fn, N=2, H=8, W=16, C0=32, C1=32, Cout=32, ksize=1),
                 R("in", fn, N=2, H=64, W=64, C0=32, Cout=512, ksize=1),
                 R("in", fn, N=1, H=96, W=120, C0=32, Cout=192, ksize=1),
                 R("in", fn, N=2, H=16, W=64, C0=32, Cout=32, c32=0),
                 R("in", fn, N=2, H=16, W=64, C0=32, Cout=32, c32=1),
                 R("in", fn, N=2, H=16, W=64, C0=32, Cout=32, c32=2),
                 R("in", fn, N=1, H=4, W=128, C0=32, Cout=32),
                 R("in", fn, N=1, H=6, W=128, C0=64, Cout=32),
                 R("inp", fn, N=2, H=64, W=128, C0=32, C1=32, Cout=512),
                 R("inp", fn, N=1, H=32, W=128, C0=32, Cout=512),
                 R("inp", fn, N=2, H=64, W=256, C0=32, Cout=512, stride=2),
                 R("inp", fn, N=2, H=128, W=256, C0=32, Cout=512, stride=2),
                 R("in", fn, N=8, H=8, W=16, C0=32, C1=64, Cout=32, lim=3),
                 R("in", fn, N=8, H=16, W=16, C0=64, Cout=64, stride=2, lim=3),
                 R("in", fn, N=8, H=8, W=16, C0=32, Cout=32, ksize=1, lim=3)]
    rows += [R("in", "conv_in_fwd", N=2, H=128, W=512, C0=32, Cout=32, c32=1),
             R("in", "conv_in_fwd_b16_wb", N=2, H=8, W=8, C0=256, Cout=64, w3=0),
             R("inp", "conv_in_fwd_b16_wb", N=2, H=64, W=128, C0=32, C1=32, Cout=512, w3=0)]
    for fn in ("conv_in_stats_finalize", "conv_in_stats_finalize_b16"):
        rows += [R("fin", fn, N=2, H=8, W=16, Cout=32, stats_px=64),
                 R("fin", fn, N=2, H=8, W=16, Cout=32, stats_px=0),
                 R("fin", fn, N=2, H=8, W=16, Cout=64, stats_px=128, mask=1),
                 R("fin", fn, N=2, H=5, W=7, Cout=32, stats_px=0, mask=1)]
    # ---- low-resolution data gradient of the up-sampled operand
    for fn in ("conv3x3_up_bwd_data", "conv3x3_up_bwd_data_b16", "conv3x3_up_bwd_data_bs",
               "conv3x3_up_bwd_data_bs_b16", "conv3x3_up_bwd_data_bs_b16_wb"):
        bs = dict(bs="ok") if "_bs" in fn else {}
        rows += [R("upb", fn, N=2, H=5, W=7, Cout=32, Ccols=32, **bs),
                 R("upb", fn, N=2, H=8, W=16, Cout=32, Ccols=32, **bs),
                 R("upb", fn, N=2, H=8, W=8, Cout=32, Ccols=64, Cin_total=96, ci_offset=32, acc=1,
                   **bs),
                 R("upb", fn, N=2, H=8, W=8, Cout=256, Ccols=64, **bs),
                 R("upb", fn, N=1, H=64, W=64, Cout=32, Ccols=512, **bs),
                 R("upb", fn, N=1, H=128, W=128, Cout=32, Ccols=512, **bs),
                 R("upb", fn, N=8, H=8, W=16, Cout=32, Ccols=32, Cin_total=64, ci_offset=32, acc=1,
                   lim=3, **bs)]
    rows += [R("upb", "conv3x3_up_bwd_data_bs", N=2, H=8, W=16, Cout=32, Ccols=32, bs="short"),
             R("upb", "conv3x3_up_bwd_data_bs", N=2, H=8, W=16, Cout=32, Ccols=32),
             R("upb", "conv3x3_up_bwd_data_bs_b16_wb", N=2, H=8, W=8, Cout=256, Ccols=64, bs="ok",
               w3=0)]
    # ---- fused forward with the up-sampling in the loader
    rows += [R("upf", "conv_up_in_fwd", N=1, H=128, W=128, C0=32, C1=32, Cout=512),
             R("upf", "conv_up_in_fwd", N=1, H=128, W=192, C0=32, Cout=192, act=""),
             R("upf", "conv_up_in_fwd", N=1, H=256, W=512, C0=32, C1=32, Cout=32, act="0"),
             R("upf", "conv_up_in_fwd", N=1, H=8, W=32, C0=64, C1=32, Cout=32, c32=2),
             R("upf", "conv_up_in_fwd", N=1, H=256, W=512, C0=64, C1=32, Cout=32, c32=1),
             R("upf", "conv_up_in_fwd", N=1, H=256, W=512, C0=64, C1=32, Cout=32, c32=0),
             R("upf", "conv_up_in_fwd_b16", N=1, H=128, W=128, C0=32, C1=32, Cout=512),
             R("upf", "conv_up_in_fwd_b16", N=1, H=32, W=128, C0=32, Cout=512),
             R("upf", "conv_up_in_fwd_b16", N=1, H=256, W=256, C0=32, C1=32, Cout=32)]
    # ---- RGB stem from uint8
    for fn in ("stem_u8_fwd", "stem_u8_fwd_b16"):
        rows += [R("u8", fn, N=2, H=6, W=128, Cout=32), R("u8", fn, N=2, H=8, W=128, Cout=64)]
    # ---- a chunked split-mode gradient with reductions asked for: the chunks take the plain split
    # kernels (no layer is bound to a chunk), not the fused pipeline's
    rows += [R("bs", "conv3x3_bwd_data_bs_bf16x3", N=8, H=4, W=32, Cout=32, Ccols=32, bs="ok", lim=3),
             R("bs", "conv3x3_bwd_data_bs_bf16x3", N=2, H=4, W=32, Cout=32, Ccols=32, bs="ok")]
    # ---- the remaining rungs of the patch ladders (csrc/conv_tiles.h), each in every role its
    # family has: plain, fused forward, BSTATS gradient.  One image; 128 x 512 or 256 x 512 pixels
    # reach a floor of 256 or 512 tiles of 4 x 32 or 8 x 32 pixels at 64 or 32 columns, H = 68
    # keeps the 8-row tile of the bf16 weight plane out.
    wide, tall = dict(N=1, H=128, W=512), dict(N=1, H=256, W=512)
    odd, odd512 = dict(N=1, H=68, W=512), dict(N=2, H=68, W=128)
    rows += [   # fp32 <64, 64, 32, 4> and <32, 64, 32, 8>
        R("fwd", "conv3x3_fwd", **wide, C0=32, Cout=64),
        R("inp", "conv_in_fwd", **wide, C0=32, Cout=64),
        R("bs", "conv3x3_bwd_data_bs", **wide, Cout=32, Ccols=64, bs="ok"),
        R("fwd", "conv3x3_fwd", **tall, C0=64, Cout=32),
        R("inp", "conv_in_fwd", **tall, C0=64, Cout=32),
        R("bs", "conv3x3_bwd_data_bs", **tall, Cout=64, Ccols=32, bs="ok"),
        # split <64, 128, 32, 8> and <32, 64, 32, 8>; the plain <128, 64, 64, 4> and <64, 64, 32, 4>
        R("fwd", "conv3x3_fwd_bf16x3", **tall, C0=32, Cout=64),
        R("inp", "conv_in_fwd_bf16x3", **tall, C0=32, Cout=64),
        R("bs", "conv3x3_bwd_data_bs_bf16x3", **tall, Cout=32, Ccols=64, bs="ok"),
        R("fwd", "conv3x3_fwd_bf16x3", **tall, C0=32, Cout=32),
        R("inp", "conv_in_fwd_bf16x3", **tall, C0=32, Cout=32),
        R("bs", "conv3x3_bwd_data_bs_bf16x3", **tall, Cout=32, Ccols=32, bs="ok"),
        R("fwd", "conv3x3_fwd_bf16x3", N=2, H=64, W=128, C0=32, Cout=512),
        R("fwd", "conv3x3_fwd_bf16x3", N=1, H=4, W=32, C0=32, Cout=64),
        # bf16 tensors, no epilogue: every tile, fp32 weight panels and (_wb) the bf16 plane
        R("bwd", "conv3x3_bwd_data_b16", N=2, H=64, W=128, Cout=32, Ccols=512),
        R("bwd", "conv3x3_bwd_data_b16", **odd, Cout=32, Ccols=64),
        R("bwd", "conv3x3_bwd_data_b16", **wide, Cout=32, Ccols=32),
        R("bs", "conv3x3_bwd_data_bs_b16_wb", **tall, Cout=32, Ccols=64),
        R("bs", "conv3x3_bwd_data_bs_b16_wb", **odd512, Cout=32, Ccols=512),
        R("bs", "conv3x3_bwd_data_bs_b16_wb", **odd, Cout=32, Ccols=64),
        R("bs", "conv3x3_bwd_data_bs_b16_wb", **wide, Cout=32, Ccols=32),
        # ... <128, 64, 64, 4> with the bf16 plane, <32, 64, 32, 8> with and without it
        R("bs", "conv3x3_bwd_data_bs_b16_wb", **odd512, Cout=32, Ccols=512, bs="ok"),
        R("inp", "conv_in_fwd_b16_wb", **odd512, C0=32, Cout=512),
        R("inp", "conv_in_fwd_b16", **wide, C0=32, Cout=32),
        R("inp", "conv_in_fwd_b16_wb", **wide, C0=32, Cout=32),
        R("bs", "conv3x3_bwd_data_bs_b16", **wide, Cout=32, Ccols=32, bs="ok"),
        R("bs", "conv3x3_bwd_data_bs_b16_wb", **wide, Cout=32, Ccols=32, bs="ok"),
        # stride-2 data gradient <32, 64, 32, 8>: fp32, bf16 with fp32 panels / the bf16 plane
        R("bs2", "conv3x3_bwd_data_bs", N=1, H=512, W=512, Cout=32, Ccols=32, stride=2, bs="ok"),
        R("bs2", "conv3x3_bwd_data_bs_b16", N=1, H=512, W=512, Cout=32, Ccols=32, stride=2, bs="ok"),
        R("bs2", "conv3x3_bwd_data_bs_b16_wb", N=1, H=512, W=512, Cout=32, Ccols=32, stride=2,
          bs="ok")]
    for i, r in enumerate(rows):
        r["id"] = i
    return rows


ROWS = _rows()
FAMILIES = sorted({r["fam"] for r in ROWS})


# ---- running a row -----------------------------------------------------------------------------
def _crc(t):
    import torch
    return zlib.crc32(t.contiguous().view(-1).view(torch.uint8).cpu().numpy().tobytes())


def coherent_planes(w, planes):
    """The bf16 weight planes a kernel may read in place of the fp32 weight `w` [taps, A, B], from
    torch alone: [planes, 9, A, B] with h = bf16(w), m = bf16(w - h), l = bf16(w - h - m) (both
    differences are exact in fp32) - or only h, round to nearest even, for a one-plane form.  A
    1x1 weight is repeated over the nine taps (no 1x1 call reads its planes)."""
    import torch
    w = w.float().expand(9, *w.shape[1:])
    h = w.to(torch.bfloat16)
    if planes == 1:
        return h[None].contiguous()
    m = (w - h.float()).to(torch.bfloat16)
    lo = (w - h.float() - m.float()).to(torch.bfloat16)
    return torch.stack([h, m, lo]).contiguous()


def build_row(ua, row, coherent=False):
    """The operands of the call of `row` on seeded inputs -> a record (dict) with
      args       the ctypes argument list (without the stream)
      t          the named torch tensors the call reads: x0 x1 wf w3 bias (plain forward), dy wd w3
                 base (the seeded dx of an accumulate row, a copy) by mean rstd gamma beta mask (the
                 unet_bwd_stats operands), s0 a0 b0 s1 a1 b1 w w3 bias (fused forward; s0 = low and
                 s1 = skip of the up-sampling one; a / b = activation coefficients or absent),
                 image mean3 std3 wf bias (uint8 stem), y gamma beta mask tiles (finalize; tiles =
                 the [N, tiles, Cout, 2] (mean, M2) pairs it merges when stats_px > 0)
      out        the tensors the call writes: y / dx, or mean rstd alpha beta
    and what call_row needs (the chunked tensor's bytes per image, the report cells, workspace).
    coherent: the weight planes w3 are those of the row's fp32 weight (coherent_planes) instead of
    an independent draw, so that the right answer does not depend on which kernel reads what;
    every other operand, and the order of the draws, is the same."""
    import torch
    from unet_implementations_amd._lib import ActSrc, BwdStats
    lib = ua.lib()
    fn = row["fn"]
    keys = T.EXPORTS[fn]
    g = torch.Generator().manual_seed(1000 + row["id"])
    dev = torch.device("cuda")
    tt = torch.bfloat16 if fn in B16 else torch.float32
    es = 2 if fn in B16 else 4

    def rnd(shape, dtype=torch.float32, scale=1.0):
        return (torch.randn(shape, generator=g, dtype=torch.float32) * scale).to(dtype).to(dev)

    N, H, W = row["N"], row["H"], row["W"]
    stride, ksize = row.get("stride", 1), row.get("ksize", 3)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    Cout = row["Cout"]
    keep, out, t = [], {}, {}
    v = dict(N=N, H=H, W=W, Cout=Cout, stride=stride, ksize=ksize, slope=0.01, eps=1e-5,
             accumulate=row.get("acc", 0))
    planes = 1 if fn in ONE_PLANE else 3
    built = dict(t=t, out=out, keep=keep, per_image=0, px=None, bs=None, ws=None, partial=None,
                 Ho=Ho, Wo=Wo)

    def src(C, h, w, act, dtype, name):
        x = rnd((N, h, w, C), dtype)
        a = rnd((N, C), scale=0.5) + 1.0 if act else None
        b = rnd((N, C), scale=0.1) if act else None
        t["s" + name] = x
        if act:
            t["a" + name], t["b" + name] = a, b
        s = ActSrc(x.data_ptr(), C, a.data_ptr() if act else None, b.data_ptr() if act else None)
        keep.append(s)
        return ctypes.byref(s)

    if "x0" in keys:                                   # plain forward, 3x3 and 1x1
        C0, C1 = row["C0"], row.get("C1", 0)
        taps = 9 if "stride" in keys else 1
        x0, x1 = rnd((N, H, W, C0)), rnd((N, H, W, C1)) if C1 else None
        wf = rnd((taps, Cout, C0 + C1), scale=0.05)
        w3 = rnd((3, 9, Cout, C0 + C1), torch.bfloat16, 0.05)
        if coherent:
            w3 = coherent_planes(wf, 3)
        y = torch.zeros((N, Ho, Wo, Cout), device=dev)
        bias = rnd((Cout,))
        t.update(x0=x0, wf=wf, w3=w3, bias=bias)
        if C1:
            t["x1"] = x1
        v.update(x0=x0.data_ptr(), C0=C0, x1=x1.data_ptr() if C1 else None, C1=C1,
                 wf=wf.data_ptr(), w3=w3.data_ptr(), bias=bias.data_ptr(), y=y.data_ptr())
        out["y"] = y
        built["per_image"] = H * W * max(C0, C1) * 4
    elif "dy" in keys:                                 # data gradients
        Ccols = row["Ccols"]
        Cin_total = row.get("Cin_total", Ccols)
        up = fn.startswith("unet_conv3x3_up_")
        taps = 9 if (up or "stride" in keys) else 1
        dy = rnd((N, Ho, Wo, (9 if up else 1) * Cout), tt)
        wd = rnd((taps, Cin_total, Cout), scale=0.05)
        w3 = rnd((planes, 9, Cin_total, Cout), torch.bfloat16, 0.05) if row.get("w3", 1) else None
        if coherent and w3 is not None:
            w3 = coherent_planes(wd, planes)
        dx = rnd((N, H, W, Ccols), tt) if row.get("acc") else torch.zeros((N, H, W, Ccols),
                                                                          dtype=tt, device=dev)
        t.update(dy=dy, wd=wd)
        if w3 is not None:
            t["w3"] = w3
        if row.get("acc"):
            t["base"] = dx.clone()
        v.update(dy=dy.data_ptr(), wd=wd.data_ptr(), w3=w3.data_ptr() if w3 is not None else None,
                 Cin_total=Cin_total, ci_offset=row.get("ci_offset", 0), dx=dx.data_ptr(),
                 Ccols=Ccols, bs=None)
        out["dx"] = dx
        built["per_image"] = Ho * Wo * (9 if up else 1) * Cout * es
        if row.get("bs"):
            by = rnd((N, H, W, Ccols), tt)
            st = [rnd((N, Ccols)), rnd((N, Ccols)).abs() + 0.5, rnd((Ccols,)), rnd((Ccols,)),
                  (rnd((N, Ccols)) > 0).float() * 2.0]
            nb = N * ((H * W + 63) // 64) * Ccols * 8
            partial = torch.zeros(nb, dtype=torch.uint8, device=dev)
            bs = BwdStats(by.data_ptr(), *[x.data_ptr() for x in st], 0.01, partial.data_ptr(),
                          nb - (1 if row["bs"] == "short" else 0), -7)
            t.update(by=by, mean=st[0], rstd=st[1], gamma=st[2], beta=st[3], mask=st[4])
            built.update(bs=bs, partial=partial)
            v["bs"] = ctypes.byref(bs)
    elif "s0" in keys or "low" in keys:                # fused forward
        C0, C1 = row["C0"], row.get("C1", 0)
        act = row.get("act", "01")
        upf = "low" in keys
        a, b = ("low", "skip") if upf else ("s0", "s1")
        v[a] = src(C0, H // 2 if upf else H, W // 2 if upf else W, "0" in act,
                   torch.float32 if C0 == 3 else tt, "0")
        v[b] = src(C1, H, W, "1" in act, tt, "1") if C1 else None
        w = rnd((ksize * ksize, Cout, C0 + C1), scale=0.05)
        w3 = rnd((planes, 9, Cout, C0 + C1), torch.bfloat16, 0.05) if row.get("w3", 1) else None
        if coherent and w3 is not None:
            w3 = coherent_planes(w, planes)
        bias = rnd((Cout,))
        y = torch.zeros((N, Ho, Wo, Cout), dtype=tt, device=dev)
        t.update(w=w, bias=bias)
        if w3 is not None:
            t["w3"] = w3
        v.update(w=w.data_ptr(), wf=w.data_ptr(), w3=w3.data_ptr() if w3 is not None else None,
                 bias=bias.data_ptr(), y=y.data_ptr())
        out["y"] = y
        built["per_image"] = H * W * max(C0, C1) * es
    elif "image" in keys:                              # RGB stem from uint8
        img = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
        wf, bias = rnd((9, Cout, 3), scale=0.05), rnd((Cout,))
        y = torch.zeros((N, H, W, Cout), dtype=tt, device=dev)
        mean3, std3 = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
        t.update(image=img, wf=wf, bias=bias, mean3=torch.tensor(mean3, device=dev),
                 std3=torch.tensor(std3, device=dev))
        v.update(image=img.data_ptr(), mean3=(ctypes.c_float * 3)(*mean3),
                 std3=(ctypes.c_float * 3)(*std3), wf=wf.data_ptr(),
                 bias=bias.data_ptr(), y=y.data_ptr())
        out["y"] = y
    else:                                              # statistics finalize
        y = rnd((N, H * W, Cout), tt)
        res = [torch.zeros((N, Cout), device=dev) for _ in range(4)]
        gamma, beta = rnd((Cout,)), rnd((Cout,))
        mask = (rnd((N, Cout)) > 0).float() * 2.0 if row.get("mask") else None
        t.update(y=y, gamma=gamma, beta=beta)
        if mask is not None:
            t["mask"] = mask
        v.update(y=y.data_ptr(), stats_px=row["stats_px"], gamma=gamma.data_ptr(),
                 beta=beta.data_ptr(), mask=mask.data_ptr() if mask is not None else None,
                 mean=res[0].data_ptr(), rstd=res[1].data_ptr(), alpha_out=res[2].data_ptr(),
                 beta_out=res[3].data_ptr(), HoWo=H * W)
        out.update(mean=res[0], rstd=res[1], alpha=res[2], beta=res[3])
    if "ws" in keys:
        nws = lib.unet_conv_in_fwd_workspace_bytes(N, H, W, Cout, stride)
        if "stats_px" in keys:       # the producer's summaries: (mean, M2 >= 0) per tile
            ws = torch.zeros(nws, dtype=torch.uint8, device=dev)
            ws[:nws // 4 * 4] = rnd((nws // 4,)).abs().view(torch.uint8)
            if row["stats_px"]:
                tiles = H * W // row["stats_px"]
                t["tiles"] = ws[:N * tiles * Cout * 8].view(torch.float32).view(
                    N, tiles, Cout, 2).clone()
        else:
            ws = torch.zeros(nws, dtype=torch.uint8, device=dev)
        built["ws"] = ws
        if "px" in keys:
            built["px"] = ctypes.c_int(-7)
        v.update(ws=ws.data_ptr(), ws_bytes=nws,
                 px=ctypes.byref(built["px"]) if "px" in keys else None)
    built["args"] = [v[k] for k in keys]
    return built


def call_row(ua, row, built):
    """Makes the call of `row` on the operands of build_row under the row's chunk limit and c32
    switch; returns (launches, report, {output: tensor}) - the outputs of build_row plus, where the
    call reports them, `stats` / `partial` cut to the reported tile count (raw bytes)."""
    import torch
    lib = ua.lib()
    fn = row["fn"]
    keys = T.EXPORTS[fn]
    out = dict(built["out"])
    prev = lib.unet_set_c32_winograd(row["c32"]) if "c32" in row else None
    torch.cuda.synchronize()
    try:
        with T.chunk_limit(lib, row.get("lim", 0) * built["per_image"]), \
                ua.ops.record_launches() as rec:
            rc = getattr(lib, fn)(*built["args"], ua.ops._stream())
    finally:
        if prev is not None:
            lib.unet_set_c32_winograd(prev)
    ua.ops.check(rc)
    torch.cuda.synchronize()
    report = -1
    if "px" in keys:
        report = built["px"].value
        if report > 0:
            out["stats"] = built["ws"][:row["N"] * (built["Ho"] * built["Wo"] // report) *
                                       row["Cout"] * 8]
    if built["bs"] is not None:
        report = built["bs"].tiles_out
        if report > 0:
            out["partial"] = built["partial"][:row["N"] * report * row["Ccols"] * 8]
    return rec.names, report, out


def run_row(ua, row):
    """Makes the call of `row` on seeded inputs; returns (launches, report, {output: crc32})."""
    names, report, out = call_row(ua, row, build_row(ua, row))
    return names, report, {k: _crc(t) for k, t in out.items()}


# ---- coverage ------------------------------------------------------------------------------------
def assert_coverage(rec):
    """`rec`: the recorded rows ({"id", "launches", "report", "crc"}), aligned with ROWS."""
    assert [r["id"] for r in rec] == [r["id"] for r in ROWS], "the table is of another grid"
    both = [dict(r, **x) for r, x in zip(ROWS, rec)]

    def some(cond, what):
        assert any(cond(r) for r in both), "no row with " + what

    def kern(r, s):
        return any(s in k for k in r["launches"])

    launching = [n for n in T.EXPORTS]
    assert {r["fn"] for r in both} == set(launching), "an export that launches is missing"
    assert all(r["launches"] for r in both)
    for s in (1, 2):
        some(lambda r: r.get("stride", 1) == s and "stride" in T.EXPORTS[r["fn"]], f"stride {s}")
    some(lambda r: r.get("C1", 0) > 0 and "x0" in T.EXPORTS[r["fn"]], "a two-source forward")
    some(lambda r: r.get("ci_offset", 0) > 0, "a channel slice")
    for a in (0, 1):
        some(lambda r: "dy" in T.EXPORTS[r["fn"]] and r.get("acc", 0) == a, f"accumulate {a}")
    for fn in ("unet_conv3x3_fwd", "unet_conv_in_fwd", "unet_conv_in_fwd_b16"):
        some(lambda r: r["fn"] == fn and r["C0"] == 3 and r["W"] % 128, fn + ": stem, generic")
        some(lambda r: r["fn"] == fn and r["C0"] == 3 and r["W"] % 128 == 0 and r["H"] % 8,
             fn + ": stem, rows")
        some(lambda r: r["fn"] == fn and r["C0"] == 3 and r["W"] % 128 == 0 and r["H"] % 8 == 0,
             fn + ": stem, walk")
    for fn in ("unet_stem_u8_fwd", "unet_stem_u8_fwd_b16"):
        some(lambda r: r["fn"] == fn and r["H"] % 8, fn + ": rows")
        some(lambda r: r["fn"] == fn and r["H"] % 8 == 0, fn + ": walk")
    for k in ("conv_stem_fwd_kernel", "conv_stem_fwd_rows_kernel", "conv_stem_fwd_walk_kernel"):
        some(lambda r: kern(r, k), k)
    # the six chunk sites: N = 8 as 3 + 3 + 2, nothing reported
    for site in ("unet_conv3x3_fwd", "unet_conv3x3_bwd_data_bs", "unet_conv1x1_fwd",
                 "unet_conv1x1_bwd_data", "unet_conv_in_fwd", "unet_conv3x3_up_bwd_data_bs"):
        ch = [r for r in both if r["fn"] == site and r.get("lim")]
        assert ch and all(r["N"] == 8 and r["lim"] == 3 for r in ch), site
        assert all(len(r["launches"]) % 3 == 0 for r in ch), site
        assert all(r["report"] in (0, -1) for r in ch), site
    assert all(r["report"] <= 0 for r in both if r.get("lim"))
    for what, cond in (
            ("stride-1", lambda r: r["fam"] == "bs"),
            ("stride-2", lambda r: r["fam"] == "bs2"),
            ("up-sampled", lambda r: r["fam"] == "upb")):
        some(lambda r: cond(r) and r.get("bs") and r["report"] > 0, what + " dgrad, tiles_out > 0")
        some(lambda r: cond(r) and r.get("bs") and r["report"] == 0, what + " dgrad, tiles_out 0")
    some(lambda r: r["fam"] in ("in", "inp") and r["report"] > 0, "fused forward, stats_px > 0")
    some(lambda r: r["fam"] in ("in", "inp") and r["report"] == 0, "fused forward, stats_px 0")
    s2 = [r for r in both if r["fam"] == "bs2"]
    assert any(kern(r, "conv_dgrad_s2_patch_kernel") for r in s2), "stride-2 dgrad: patch fp32"
    assert any(kern(r, "conv_dgrad_s2_patch_b16_kernel") for r in s2), "stride-2 dgrad: patch bf16"
    assert any(kern(r, "conv_dgrad_s2_kernel") for r in s2), "stride-2 dgrad: single launch"
    assert any(len(r["launches"]) == 4 for r in s2), "stride-2 dgrad: per-class launches"
    for k in (0, 1, 2):
        some(lambda r: r.get("c32") == k and r.get("C0", r["Cout"]) == 32 and
             r.get("Ccols", r["Cout"]) == 32, f"32 -> 32 with the c32 switch at {k}")
    some(lambda r: kern(r, "conv_c32_kernel"), "conv_c32_kernel")
    some(lambda r: kern(r, "conv_wino32q_kernel"), "conv_wino32q_kernel")
    some(lambda r: kern(r, "conv_wino_up32_kernel"), "conv_wino_up32_kernel")
    for fn in ("unet_conv_in_fwd_bf16x3", "unet_conv3x3_bwd_data_bs_bf16x3"):
        some(lambda r: r["fn"] == fn and kern(r, "conv_patch_split_kernel"), fn + ": split patch")
        some(lambda r: r["fn"] == fn and "stride" not in r and r.get("ksize", 3) == 3 and
             not kern(r, "split"), fn + ": falls through to fp32")
    # every distinct return of the four dispatchers shows as a kernel instantiation
    for k in ("conv_patch_f32_kernel<", "conv_patch_up_kernel<", "conv_patch_s2_kernel<", "conv_patch_b16_kernel<",
              "conv_igemm_rf_kernel<",
              "conv_igemm_kernel<128, 128, 64, 64, 32, true, 1>",
              "conv_igemm_kernel<128, 64, 64, 32, 32, true, 1>",
              "conv_igemm_kernel<64, 64, 32, 32, 32, true, 1>",
              "conv_igemm_kernel<64, 64, 32, 32, 32, true, 2>",
              "conv_igemm_kernel<64, 64, 32, 32, 32, true, 4>",
              "conv_igemm_kernel<128, 32, 32, 32, 32, true, 1>",
              "conv_igemm_kernel<128, 128, 64, 64, 32, false, 1>",
              "conv_igemm_kernel<128, 64, 64, 32, 32, false, 1>",
              "conv_igemm_kernel<64, 64, 32, 32, 32, false, 1>",
              "conv_igemm_kernel<64, 64, 32, 32, 32, false, 2>",
              "conv_igemm_kernel<64, 64, 32, 32, 32, false, 4>",
              "conv_igemm_kernel<128, 32, 32, 32, 32, false, 1>",
              "conv_igemm_split_kernel<128, 128, 64, 64>", "conv_igemm_split_kernel<128, 64, 64, 32>",
              "conv_igemm_split_kernel<64, 64, 32, 32>", "conv_igemm_split_kernel<128, 32, 32, 32>",
              "conv_patch_split_kernel<"):
        some(lambda r: kern(r, k), k)
    # bf16 matrix cores on fp32 tensors (4 forms) and on bf16 tensors (gather, WIDE, DENSE)
    # (the instantiations on bf16 tensors are reported mangled)
    lowp = {k for r in both for k in r["launches"] if "conv_igemm_bf16_kernel" in k}
    assert len(lowp) >= 13, sorted(lowp)
    # chunked bf16-storage calls (element size 2 in the chunk walk's byte offsets)
    some(lambda r: r.get("lim") and r["fn"] in B16 and "dy" in T.EXPORTS[r["fn"]], "chunked bf16 dgrad")
    some(lambda r: r.get("lim") and r["fn"] in B16 and "s0" in T.EXPORTS[r["fn"]], "chunked bf16 fwd")


def record(ua, fams=None):
    """Runs every row (of the families `fams`) once; returns the table rows."""
    rec = []
    for row in ROWS:
        if fams is not None and row["fam"] not in fams:
            continue
        names, report, crc = run_row(ua, row)
        rec.append(dict(id=row["id"], launches=names, report=report, crc=crc))
    return rec


def write_table(rec):
    """Stores the rows as [id, [kernel indices], report, crcs] beside the list of kernel names."""
    kernels = sorted({k for r in rec for k in r["launches"]})
    os.makedirs(os.path.dirname(TABLE), exist_ok=True)
    with open(TABLE, "w") as f:
        f.write('{"kernels": [\n')
        f.write(",\n".join("  " + json.dumps(k) for k in kernels))
        f.write('\n ],\n "rows": [\n')
        f.write(",\n".join("  " + json.dumps(
            [r["id"], [kernels.index(k) for k in r["launches"]], r["report"], r["crc"]])
            for r in rec))
        f.write("\n ]\n}\n")


def load_table():
    """The committed table as `record` returns it."""
    with open(TABLE) as f:
        tab = json.load(f)
    return [dict(id=i, launches=[tab["kernels"][k] for k in ks], report=report, crc=crc)
            for i, ks, report, crc in tab["rows"]]


def main():
    import unet_implementations_amd as ua
    first = record(ua)
    second = record(ua)
    diff = [(a, b) for a, b in zip(first, second) if a != b]
    if diff:
        raise SystemExit(f"{len(diff)} rows differ between their two runs, first: {diff[0]}")
    try:
        assert_coverage(first)
    except AssertionError:
        with open(TABLE + ".rejected", "w") as f:    # (for diagnosis: not a table)
            json.dump(first, f, indent=0)
        raise
    write_table(first)
    print(f"{TABLE}: {len(first)} rows, each identical in two runs")


if __name__ == "__main__":
    main()
