"""Every kernel of the split-bf16 ("bf16x3") train step against fp64, launch asserted (-m gpu).

matmul_precision = "bf16x3" keeps fp32 tensors and splits every operand of a stride-1 3x3
multiply into three bf16 terms on chip (six bf16 MFMA products per multiply).  Its selectors
switch on tile counts, and a shape without a split tile silently runs an fp32 kernel behind
the same entry, so a small test shape says nothing about the kernel the step runs unless the
launch is asserted.  This file is the third of its kind, after tests/test_fp32_step_kernels_gpu.py
and tests/test_bf16_bench_layers_gpu.py; like the first it runs its table through the runners of
tests/tools/step_kernel_harness.py and holds only its operand mode (MODE): each row of LAYERS is one
call of the step - the same `ops` function with the operand mode unet.py uses in this mode (the
planes w3 / wd3 of a PackTable(convs, 3, None), x3=True on conv_in_bwd_weight, bf16="bf16x3" with
wd3 and a NextNorm where layer_bwd passes one, a PLAIN first source + activated skip for the
decoder's first convolutions - this mode materialises the activated up-sampling -, ci_offset /
accumulate where the walk uses them, the c32 switch as _UNetFunction.forward sets it) - at N = 2
and the smallest H != W grid for which (a) the call launches the very instantiations it launches
inside the step, finalizers and reduce stages included, and (b) every loop the workload shape
runs more than once still runs more than once; (b) is the comment over the row.  As in the fp32
file a weight-gradient row is made undeferred, so its names end with that layer's own 1 - 3
wgrad_reduce_batched_kernel stages.  Each case
  * records the launches of the call and asserts they are the row's names;
  * holds the result to a float64 evaluation of the SAME fp32 operands, one image at a time on
    the GPU (tests/tools/fp64_layer_refs.py), within the bound the existing x3 test of the same
    entry point uses (TOL_* of the harness: one set of values for both modes);
  * forward rows check mean, rstd, alpha, beta; BSTATS rows check that the gradient is bit-equal
    to the call without the epilogue and drive the InstanceNorm backward from the summaries;
    accumulating rows start from a non-zero buffer; column-slice rows fill dw with a sentinel;
  * kind "x3" (a split kernel runs): THE TERM CHECK.  The bounds above are the fp32 bounds and
    have 6 - 8 x headroom over one missing 2^-16 product (h l, m m or l h), so a kernel that
    forms five products instead of six passes them.  R.term_check evaluates the row's reference
    in fp64 on the six-product expansion of its two operands (the ACTIVATED operand is split:
    the loaders activate first) with one third-order product left out; e_drop is the smallest of
    the three relative L2 errors, e_kernel the kernel's relative L2 error, and the row asserts
    e_kernel <= e_drop / 2 and, on the reference alone, that the full six-product evaluation is
    100 x below e_drop (measured 5.7e-9 .. 7.0e-9 against 2.2e-6 .. 2.5e-6);
  * kind "same32" / "fp32" (the x3 entry lands on an fp32 kernel: the stride-2 layers, the 16 x 16
    layers - W % 32 != 0 has no split tile -, the stem, taps, the low-resolution GEMMs, head,
    InstanceNorm backward): the fp64 bounds all the same, every name must be one a row of the fp32
    file expects (looked up, not re-run), and "same32" rows are bit-equal to the same call through
    the fp32 entry.  Three rows cannot be: the stride-2 weight gradients with >= 4 channel tiles
    (128->256, 256->512, 512->512) - the fp32 entry takes the eight-wave conv_wgrad_kernel for
    them, the x3 entry (prec = 3 in wgrad_select) stays on the four-wave instantiation, whose
    name the fp32 file holds through its 64->128 row.  A stride-2 BSTATS row compares with the
    epilogue-free call of the FP32 entry: the x3 entry without the epilogue runs other kernels.
test_check_sees_one_missing_row: one forward, one BSTATS data-gradient and one weight-gradient
x3 row must be REJECTED against a reference with one row of one image zeroed;
test_term_check_sees_one_missing_product: each five-product evaluation is rejected by the
criterion the rows apply.  The closure: test_every_bf16x3_step_kernel_is_held records one whole
eager step at N = 8, 512 x 512 (oracle.unet_ref.synthetic_batch(1234, ...), the fp32 fixture's
optimizer and loss) and requires every kernel it launches to be a row's or an ALLOWED entry's,
test_every_row_kernel_runs_in_the_step is the converse, ALLOWED names per non-convolution kernel
the existing test that holds it and that test's smallest call (run by test_allowed_kernel_is_
launched_by_its_test).  The record shows 46 distinct kernels in 171 launches: the four split
tiles each as fused forward, BSTATS data gradient and PLAIN data gradient (twelve conv_patch_
split_kernel instantiations), two split weight gradients, and 32 fp32 / utility kernels.  The
plain forms are launch_patch_split_auto's: the skip halves of the decoder's first convolutions
take no NextNorm, and unet_conv3x3_bwd_data_bf16x3 without one goes through dispatch_igemm_split
- so they have rows here ("dgrad skip ...").  conv_igemm_split_kernel itself is not launched by
the step (every skip grid has W % 32 == 0) and stays with test_kernels_gpu.py::*bf16x3*.

MEASURED on an MI355X (profiles/bf16x3_step_kernels_error.txt has every row):
  * every launch list equals the row's; both closure tests pass; the controls reject;
  * largest share of each bound: y 0.08 (1.6e-6 of 2e-5, up fwd 512+512->512), dx 0.05 (1.1e-6,
    dgrad 512<-512 bstats), dw 0.011 (3.4e-7 of 3e-5), low-resolution g 0.063, taps 0.12,
    statistics 0.003, summaries 0.025, InstanceNorm backward 0.003;
  * term check, e_kernel / e_drop (bound 0.5): weight gradients 0.05 .. 0.12 on their dense
    operands - NO row needed the sparse dy the issue provides for them -; forward and data
    gradients 0.04 (K = 288) .. 0.26 (K = 9216), growing like sqrt(K).
THE BUG THE TERM CHECK FOUND: with conv_patch_split_kernel as it was, two rows failed it -
        up fwd 512+512->512 (K = 9216)   e_kernel 1.46e-6   e_drop 2.37e-6   ratio 0.62
        up fwd 512+256->256 (K = 6912)   e_kernel 1.27e-6   e_drop 2.37e-6   ratio 0.54
and fwd 512->512 32 / dgrad 512<-512 (K = 4608) sat at 0.42.  No product was missing: the kernel
chained the six MFMAs of a 16-channel chunk into ONE fp32 accumulator, so the large running sum
was rounded 6 K / 16 times (3456 at K = 9216), not K / 16 times; the random-walk estimate
2^-24 / sqrt(3) x sqrt(n / 2) gives 1.4e-6 for n = 3456 and 1.25e-6 for n = 2592, the measured
figures, 3 x the plain fp32 accumulation.  The kernel now keeps the five correction products
(2^-8 .. 2^-16 of the sum) in a second accumulator that is added once at the end: the same two
rows measure 6.1e-7 (0.26) and 5.2e-7 (0.22), every row passes, no register spills, and the eager
bf16x3 step at 8 x 512^2 takes 20.09 ms against 20.05 ms before.
Rows are kept within 2 x 256 x 256 pixels at up to 64 channels and 65,536 pixels above that,
counted on the grid the kernel tiles.  The rows above those caps, and why:
  * "fwd 32->32", "up fwd 64+32->32" (2 x 264 x 512): the step's finalizer pair in_stats_finalize_
    grp / _comb needs >= 512 statistics tiles of 256 pixels PER IMAGE, and N >= 2;
  * "fwd 32->64 s2" (input 2 x 256 x 1024, output at the cap): the same, 128-pixel tiles;
  * "dgrad s2 32<-64 bstats acc" (dx 2 x 256 x 512): the 32-column stride-2 form needs >= 256
    tiles of 8 x 32 on the dy grid;
  * "wgrad s2 32->64", "stem wgrad 3->32" (2 x 136 x 512): a third REDUCE stage needs > 256 slabs.
At the caps: the <32,64,32,8> and <64,128,32,8> tiles need M / 256 >= 512 (2 x 128 x 512), the
<128,64,64,4> tile M / 128 x columns / 128 >= 512 (2 x 128 x 256 at 128 columns).  Below the caps
but short of (b): the taps rows at C = 32 and C = 64, as in the fp32 file.

Kernel -> row (shape N x H x W of the row's input grid; regime notes in LAYERS):
  conv_patch_split_kernel<32, 64, 32, 8, fwd>     fwd 32->32, up fwd 64+32->32        2 x 264 x 512
  conv_patch_split_kernel<64, 128, 32, 8, fwd>    fwd 64->64, up fwd 128+64->64       2 x 128 x 512
  conv_patch_split_kernel<128, 64, 64, 4, fwd>    fwd 128->128, 256->256, up fwd 256+128->128, 512+256->256
                                                                                      2 x 128 x 256, 2 x 64 x 256
  conv_patch_split_kernel<64, 64, 32, 4, fwd>     fwd 512->512 32, up fwd 512+512->512  2 x 32 x 64
  conv_patch_split_kernel<.., bs>                 dgrad 32<-32 .. 512<-512 bstats     (the forward tiles' floors)
  conv_patch_split_kernel<.., plain>              dgrad skip 32<-32 .. 512<-512       (the same shapes)
  conv_wgrad_bf16_kernel<32, 32, 64, 3, ..>       wgrad 32->32, skip                  2 x 136 x 256
  conv_wgrad_bf16_kernel<64, 64, 16, 3, ..>       wgrad 64->64 .. 512->512 16, skips  2 x 72 x 128 .. 2 x 8 x 16
  conv_stem_fwd_walk_kernel, conv_patch_s2_kernel<..>, conv_igemm_kernel<64, 64, .., true, 4>
                                                  stem fwd, fwd .. s2, fwd 512->512 16 (the fp32 file's shapes)
  conv_dgrad_s2_patch_kernel<..>, conv_igemm_kernel<64, 64, .., false, 4>
                                                  dgrad s2 .. bstats acc, dgrad 512<-512 16 bstats
  conv_wgrad_kernel<64, 64, 16, 2, .., 4>, <32, 64, 32, 2, .., 4>, conv_stem_wgrad_rows_kernel
                                                  wgrad s2 .., stem wgrad 3->32
  upsample2x_bwd_taps_kernel, conv_wgrad_taps_kernel<..>, conv_igemm_kernel<.., false, 1 | 4>
                                                  taps .., up wgrad .., up dgrad .. bstats
  head_fwd / head_bwd / head_bwd_finalize, in_bwd_finalize1 / in_bwd_apply, in_stats_finalize_*
                                                  head fwd / bwd, in bwd .. fed, the forward rows
  nchw_to_nhwc, pack_w_batched, upsample2x_fwd_kernel<float>, loss_*, sgd_nesterov
                                                  ALLOWED (the test named next to each)

Wall time on an MI355X: the whole file 4.6 s for its 84 cases (1.1 s of it the recorded 8 x
512^2 step, the only launch at the workload size), its slowest case 0.84 s ("in bwd 32 fed", the
first fp64 autograd call), every other case at most 0.22 s; the fp32 file runs 85 cases in 4.9 s,
its slowest 0.83 s.
"""
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("step_kernel_harness", os.path.join(
    os.path.dirname(os.path.abspath(__file__)), "tools", "step_kernel_harness.py"))
HS = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(HS)
R = HS.R

# The term check: a kernel's relative L2 error must stay below half the error of a six-product
# evaluation that lacks one 2^-16 product, and the full six-product evaluation must sit at least
# 100 x below that error (both from the float64 reference alone).
TERM_MARGIN = 2.0
TERM_FLOOR = 100.0


def term(fn, a, b, got, exact, extra=None):
    """e_kernel, e_drop, e_six of one x3 result (see R.term_check): relative L2 against `exact`."""
    e_drop, e_six = R.term_check(fn, a, b, exact, extra)
    return dict(e_kernel=R.rel_l2(got, exact), e_drop=e_drop, e_six=e_six)


def term_failures(t):
    bad = []
    if not t["e_six"] * TERM_FLOOR <= t["e_drop"]:
        bad.append(f"the operands collapse the term check: six products {t['e_six']:.2e}, one "
                   f"dropped {t['e_drop']:.2e}")
    if not t["e_kernel"] * TERM_MARGIN <= t["e_drop"]:
        bad.append(f"term check: e_kernel {t['e_kernel']:.3e} > e_drop / 2 = {t['e_drop'] / 2:.3e}")
    return bad


# --------------------------------------------------------------------------- the operand mode
def pack(ua, w, stride):
    """The PackTable of one 3x3 layer as _Walk builds it in this mode: the packed fp32 layouts
    plus the three bf16 planes of both (none for the RGB stem), no Winograd form."""
    return HS.pack_one(ua, w, 3)


def forms(ua, op, table, grid=None, held=True):
    """The planes w3 / wd3, bf16 = "bf16x3" on the data gradient, x3 = True on the weight gradient
    (as the walk passes it for every layer of this mode); the low-resolution data gradient reads
    fp32 D, so the walk passes no planes.  No "up_fwd": this mode materialises the up-sampling."""
    return {"fwd": lambda: dict(w3=table.wf3[0]),
            "dgrad": lambda: dict(bf16="bf16x3", wd3=table.wd3[0]),
            "wgrad": lambda: dict(x3=True),
            "up_dgrad": lambda: dict(wd3=None)}[op]()


# The rows' x3 argument: True (the default) = the split kernel runs and the runner returns the
# term check's figures; False = an fp32 kernel behind the same entry, and the runner compares
# the result bit for bit with the same call through the fp32 entry (HS.FP32_ENTRY).
MODE = HS.Mode("bf16x3", 3, pack, forms, term)

# --------------------------------------------------------------------------- the table
# The runners and the kernel names more than one table uses: tests/tools/step_kernel_harness.py.
run_fwd, run_stem_fwd, run_dgrad, run_wgrad = HS.run_fwd, HS.run_stem_fwd, HS.run_dgrad, HS.run_wgrad
run_stem_wgrad, run_taps, run_up_wgrad = HS.run_stem_wgrad, HS.run_taps, HS.run_up_wgrad
run_up_dgrad, run_head_fwd, run_head_bwd, run_in_bwd = \
    HS.run_up_dgrad, HS.run_head_fwd, HS.run_head_bwd, HS.run_in_bwd
patch_s2, dgrad_s2, igemm, wgrad, wtaps = HS.patch_s2, HS.dgrad_s2, HS.igemm, HS.wgrad, HS.wtaps
REDUCE, FIN_GRP, FIN_COMB, FIN_EQ, TAPS = HS.REDUCE, HS.FIN_GRP, HS.FIN_COMB, HS.FIN_EQ, HS.TAPS
STEM_FWD, STEM_WGRAD, HEAD_FWD, HEAD_BWD = HS.STEM_FWD, HS.STEM_WGRAD, HS.HEAD_FWD, HS.HEAD_BWD
HEAD_BWD_FIN, IN_FIN1, IN_APPLY = HS.HEAD_BWD_FIN, HS.IN_FIN1, HS.IN_APPLY
_NS, _AN = HS._NS, HS._AN


# The split kernels of this mode.
def split(tile, form):
    """conv_patch_split_kernel<BN, WM, WN, TH, ACT, STATS, BSTATS>: form "fwd" = the fused forward
    (activation on load, statistics epilogue), "bs" = the data gradient of the fused pipeline
    (BSTATS epilogue), "plain" = the stand-alone data gradient (no epilogue)."""
    flags = {"fwd": "true, true, false", "bs": "false, false, true", "plain": "false, false, false"}
    return f"void {_NS}conv_patch_split_kernel<{tile}, {flags[form]}>(unet_conv::IgemmParams)"


T128, T64T, T64, T32T = "128, 64, 64, 4", "64, 128, 32, 8", "64, 64, 32, 4", "32, 64, 32, 8"


def wgrad3(targs):
    """conv_wgrad_bf16_kernel<CI_T, CO_T, S, 3 planes, single buffer, float, float, ACT>"""
    return f"void {_AN}conv_wgrad_bf16_kernel<{targs}>({_AN}WgradParams)"


WG3_32 = wgrad3("32, 32, 64, 3, true, float, float, true, 1")
WG3_64 = wgrad3("64, 64, 16, 3, false, float, float, true, 1")

# (id, the layers of UNet() it stands for, runner, arguments, expected kernel names in launch
# order, kind).  Encoder stage e, conv k: "e<e>.<k>"; decoder stage d: "d<d>.<k>".  Layers with the
# same call and channel geometry share a row.  The comment over a row is its regime note (b): what
# the workload shape (8 x 512^2) loops over, and what is left of it at the row's shape.  kind:
#   "x3"     a split-bf16 kernel runs: fp64 bounds and the term check;
#   "same32" the x3 entry lands on an fp32 kernel: fp64 bounds, torch.equal with the same call in
#            the fp32 operand mode, and every name must be one a row of the fp32 file holds;
#   "fp32"   an fp32 kernel as well (fp64 bounds and the lookup), but either the call has no operand
#            of this mode at all (stem forward, taps, low-resolution GEMMs, head, InstanceNorm
#            backward: the walk makes the fp32 mode's call) or the fp32 mode's call selects
#            another instantiation (the stride-2 weight gradients with >= 4 channel tiles: the x3
#            entry keeps them on the four-wave kernel, the fp32 entry takes the eight-wave one).
X3, SAME32, FP32 = "x3", "same32", "fp32"
LAYERS = [
    # ---- forward
    # walk over 8-row strips, 512 statistics tiles per image (the floor of the two-level
    # finalizer); workload: 2048 per image
    ("stem fwd 3->32", "e0.0", run_stem_fwd, dict(N=2, H=128, W=512),
     [STEM_FWD, FIN_GRP, FIN_COMB], FP32),
    # conv_patch_split rows: one TH x 32 pixel tile x BN columns per workgroup (no walk); K =
    # C0 + C1 in chunks of 16, nine taps per chunk, the source switch at chunk C0 / 16; grid =
    # images x tile rows x tile columns x column tiles, each > 1 unless the note says otherwise.
    # <32,64,32,8>: 8 x 32 tiles, 1 column tile (as the workload), K = 32 in 2 chunks; 1056 tiles
    # (the selector's floor is 512); 528 statistics tiles per image -> two-level finalizer (>= 512;
    # workload 1024)
    ("fwd 32->32", "e0.1 d4.1", run_fwd, dict(N=2, H=264, W=512, C0=32, C1=0, Cout=32, stride=1),
     [split(T32T, "fwd"), FIN_GRP, FIN_COMB], X3),
    # one 4 x 32 output tile per workgroup, K = 32 in one chunk per tap (as the workload);
    # 512 statistics tiles per image -> two-level finalizer
    ("fwd 32->64 s2", "e1.0", run_fwd,
     dict(N=2, H=256, W=1024, C0=32, C1=0, Cout=64, stride=2, x3=False),
     [patch_s2("64, 64, 32, 4"), FIN_GRP, FIN_COMB], SAME32),
    # <64,128,32,8>: 512 tiles of 8 x 32 (the floor), 1 column tile (as the workload), K = 64 in 4
    # chunks; 256 statistics tiles per image, one-level finalizer (workload: 256)
    ("fwd 64->64", "e1.1 d3.1", run_fwd, dict(N=2, H=128, W=512, C0=64, C1=0, Cout=64, stride=1),
     [split(T64T, "fwd"), FIN_EQ], X3),
    # 512 tiles x 1 column tile of 128 (the floor), K = 64 in two 32-channel chunks per tap
    ("fwd 64->128 s2", "e2.0", run_fwd,
     dict(N=2, H=256, W=512, C0=64, C1=0, Cout=128, stride=2, x3=False),
     [patch_s2("128, 64, 64, 4"), FIN_EQ], SAME32),
    # <128,64,64,4>: 512 tiles of 4 x 32 x 1 column tile of 128 (the floor; as the workload's 1),
    # K = 128 in 8 chunks
    ("fwd 128->128", "e2.1 d2.1", run_fwd, dict(N=2, H=128, W=256, C0=128, C1=0, Cout=128, stride=1),
     [split(T128, "fwd"), FIN_EQ], X3),
    # 256 tiles x 2 column tiles of 128, K = 128 in four chunks per tap
    ("fwd 128->256 s2", "e3.0", run_fwd,
     dict(N=2, H=128, W=512, C0=128, C1=0, Cout=256, stride=2, x3=False),
     [patch_s2("128, 64, 64, 4"), FIN_EQ], SAME32),
    # <128,64,64,4>: 256 tiles x 2 column tiles (the floor, = the workload's count), K = 256 in 16
    ("fwd 256->256", "e3.1 d1.1", run_fwd, dict(N=2, H=64, W=256, C0=256, C1=0, Cout=256, stride=1),
     [split(T128, "fwd"), FIN_EQ], X3),
    # 64 tiles x 8 column tiles of 64 (the floor; the workload has 128 x 8), K = 256 in 8 chunks
    ("fwd 256->512 s2", "e4.0", run_fwd,
     dict(N=2, H=64, W=256, C0=256, C1=0, Cout=512, stride=2, x3=False),
     [patch_s2("64, 64, 32, 4"), FIN_EQ], SAME32),
    # <64,64,32,4>: 32 tiles x 8 column tiles of 64 (the floor of this tile is 256; the workload
    # has 64 x 8), K = 512 in 32 chunks; 16 statistics tiles per image (workload: 8)
    ("fwd 512->512 32", "e4.1 d0.1", run_fwd, dict(N=2, H=32, W=64, C0=512, C1=0, Cout=512, stride=1),
     [split(T64, "fwd"), FIN_EQ], X3),
    # gather-GEMM 64 x 64, M = 256 output pixels in 4 tiles (2 per image) x 8 column tiles,
    # K = 9 x 512 in four K groups
    ("fwd 512->512 s2", "e5.0", run_fwd,
     dict(N=2, H=16, W=32, C0=512, C1=0, Cout=512, stride=2, x3=False),
     [igemm(64, 64, 32, 32, True, 4), FIN_EQ], SAME32),
    # the 16 x 16 layer (W % 32 != 0: no split tile): the same kernel at stride 1, M = 256 in 4
    # tiles (2 per image), four K groups
    ("fwd 512->512 16", "e5.1", run_fwd,
     dict(N=2, H=8, W=16, C0=512, C1=0, Cout=512, stride=1, x3=False),
     [igemm(64, 64, 32, 32, True, 4), FIN_EQ], SAME32),
    # the decoder's first convolutions: plain first source (the materialised activated
    # up-sampling) + activated skip, on the output grid
    # <64,64,32,4>: K = 1024 in 64 chunks (switch at 32), 32 tiles x 8 column tiles
    ("up fwd 512+512->512", "d0.0", run_fwd,
     dict(N=2, H=32, W=64, C0=512, C1=512, Cout=512, stride=1, plain0=True),
     [split(T64, "fwd"), FIN_EQ], X3),
    # <128,64,64,4>: K = 768 in 48 chunks (switch at 32), 256 tiles x 2 column tiles
    ("up fwd 512+256->256", "d1.0", run_fwd,
     dict(N=2, H=64, W=256, C0=512, C1=256, Cout=256, stride=1, plain0=True),
     [split(T128, "fwd"), FIN_EQ], X3),
    # <128,64,64,4>: K = 384 in 24 chunks (switch at 16), 512 tiles x 1 column tile
    ("up fwd 256+128->128", "d2.0", run_fwd,
     dict(N=2, H=128, W=256, C0=256, C1=128, Cout=128, stride=1, plain0=True),
     [split(T128, "fwd"), FIN_EQ], X3),
    # <64,128,32,8>: K = 192 in 12 chunks (switch at 8), 512 tiles
    ("up fwd 128+64->64", "d3.0", run_fwd,
     dict(N=2, H=128, W=512, C0=128, C1=64, Cout=64, stride=1, plain0=True),
     [split(T64T, "fwd"), FIN_EQ], X3),
    # <32,64,32,8>: K = 96 in 6 chunks (switch at 4), 1056 tiles; 528 statistics tiles per image
    # -> two-level finalizer
    ("up fwd 64+32->32", "d4.0", run_fwd,
     dict(N=2, H=264, W=512, C0=64, C1=32, Cout=32, stride=1, plain0=True),
     [split(T32T, "fwd"), FIN_GRP, FIN_COMB], X3),
    # a grid-stride loop over pixels; several workgroups per image
    ("head fwd 32->3", "head", run_head_fwd, dict(N=2, H=32, W=64), [HEAD_FWD], FP32),
    # ---- backward: head, InstanceNorm, then per layer kind
    # 2048 tiles of 64 pixels on 1024 workgroups (the grid's cap): 2 tiles per workgroup, dw / db
    # accumulated over them and ONE summary per 128-pixel range, 512 ranges per image (workload:
    # 32 tiles per workgroup, 128 ranges per image)
    ("head bwd 32->3", "head", run_head_bwd, dict(N=2, H=128, W=512), [HEAD_BWD, HEAD_BWD_FIN], FP32),
    # InstanceNorm backward fed by BSTATS summaries (every one of the step's 22 calls): 8
    # summaries of 64 pixels per (image, channel) merged by the finalizer, then the apply pass
    ("in bwd 32 fed", "every layer", run_in_bwd, dict(N=2, H=16, W=32, C=32, fed=True),
     [IN_FIN1, IN_APPLY], FP32),
    # 512 channels: 2 summaries per (image, channel)
    ("in bwd 512 fed", "every layer", run_in_bwd, dict(N=2, H=8, W=16, C=512, fed=True),
     [IN_FIN1, IN_APPLY], FP32),
    # split data gradients: the forward's tiles with K = Cout; "bs" rows leave one summary per
    # tile (256 pixels on the 8-row tiles, 128 on the 4-row ones), several per image
    # <32,64,32,8>: 512 tiles (the floor), K = 32 in 2 chunks, 256 reduction tiles per image
    ("dgrad 32<-32 bstats", "e0.1 d4.1", run_dgrad,
     dict(N=2, H=128, W=512, Cin=32, Cout=32, stride=1, nxt=True),
     [split(T32T, "bs")], X3),
    # the stand-alone form of the same tile (no epilogue): columns 64..95 of the 96-channel weight
    ("dgrad skip 32<-32", "d4.0", run_dgrad,
     dict(N=2, H=128, W=512, Cin=32, Cout=32, stride=1, ci_off=64, cin_total=96),
     [split(T32T, "plain")], X3),
    # segments of 64 pixels (Wo >= 64), 1088 of them in 272 splits of 4 (workload: 512 splits of
    # 64); 272 slabs -> 3 REDUCE stages, as the workload's 512
    ("wgrad 32->32", "e0.1 d4.1", run_wgrad, dict(N=2, H=136, W=256, Cx=32, Cout=32, stride=1),
     [WG3_32, REDUCE, REDUCE, REDUCE], X3),
    ("wgrad skip 32->32", "d4.0", run_wgrad,
     dict(N=2, H=136, W=256, Cx=32, Cout=32, stride=1, ci_off=64, cin_total=96),
     [WG3_32, REDUCE, REDUCE, REDUCE], X3),
    # taps: one thread per (low-resolution pixel, channel quad) in a grid-stride loop over a grid
    # capped at 4096 x 256 threads.  The workload makes 4 passes at C = 32 and 2 at C = 64, one
    # at C >= 128; the small rows make one pass, "taps 512 two passes" makes two, the second
    # partial (2 x 72 x 64 x 128 = 1179648 quads), within the cap of 65,536 dy pixels
    ("taps 32", "d4.0", run_taps, dict(N=2, h=16, w=32, C=32), [TAPS], FP32),
    ("taps 64", "d3.0", run_taps, dict(N=2, h=16, w=32, C=64), [TAPS], FP32),
    ("taps 128", "d2.0", run_taps, dict(N=2, h=16, w=32, C=128), [TAPS], FP32),
    ("taps 256", "d1.0", run_taps, dict(N=2, h=8, w=16, C=256), [TAPS], FP32),
    ("taps 512", "d0.0", run_taps, dict(N=2, h=8, w=16, C=512), [TAPS], FP32),
    ("taps 512 two passes", "d4.0 d3.0 (the loop)", run_taps, dict(N=2, h=72, w=64, C=512), [TAPS],
     FP32),
    # 128 segments of 32 pixels in 32 splits of 4 (workload: 256 splits of 64); 32 slabs -> 2
    # REDUCE stages, as the workload's 256
    ("up wgrad 64->32", "d4.0", run_up_wgrad, dict(N=2, h=32, w=64, Cx=64, Cout=32, cin_total=96),
     [wtaps("32, 32, 32, true, float, float, 4"), REDUCE, REDUCE], FP32),
    # plain GEMM, K = 288 in 9 chunks, M = 1024 in 16 tiles, 8 reduction tiles per image
    ("up dgrad 64<-32 bstats", "d4.0", run_up_dgrad, dict(N=2, h=16, w=32, C0=64, Cout=32, cin_total=96),
     [igemm(64, 64, 32, 32, False, 1)], FP32),
    # <64,128,32,8>: 512 tiles (the floor), K = 64 in 4 chunks, 256 reduction tiles per image
    ("dgrad 64<-64 bstats", "e1.1 d3.1", run_dgrad,
     dict(N=2, H=128, W=512, Cin=64, Cout=64, stride=1, nxt=True),
     [split(T64T, "bs")], X3),
    # segments of 16 pixels (three planes in LDS), 1152 of them in 288 splits of 4 (workload: 512
    # splits of 64); 288 slabs -> 3 REDUCE stages, as the workload's 512
    ("wgrad 64->64", "e1.1 d3.1", run_wgrad, dict(N=2, H=72, W=128, Cx=64, Cout=64, stride=1),
     [WG3_64, REDUCE, REDUCE, REDUCE], X3),
    # 128 segments of 16 pixels in 32 splits of 4 (workload: 256 splits of 32); 2 REDUCE stages
    ("up wgrad 128->64", "d3.0", run_up_wgrad, dict(N=2, h=16, w=64, Cx=128, Cout=64, cin_total=192),
     [wtaps("64, 64, 16, true, float, float, 4"), REDUCE, REDUCE], FP32),
    ("wgrad skip 64->64", "d3.0", run_wgrad,
     dict(N=2, H=72, W=128, Cx=64, Cout=64, stride=1, ci_off=128, cin_total=192),
     [WG3_64, REDUCE, REDUCE, REDUCE], X3),
    # the 128 x 128 GEMM tile needs M >= 65536 (the selector's floor): 512 M tiles, K = 576 in
    # 18 chunks, 128 columns in one tile
    ("up dgrad 128<-64 bstats", "d3.0", run_up_dgrad,
     dict(N=2, h=128, w=256, C0=128, Cout=64, cin_total=192),
     [igemm(128, 128, 64, 64, False, 1)], FP32),
    ("dgrad skip 64<-64", "d3.0", run_dgrad,
     dict(N=2, H=128, W=512, Cin=64, Cout=64, stride=1, ci_off=128, cin_total=192),
     [split(T64T, "plain")], X3),
    # <128,64,64,4>: 512 tiles x 1 column tile (the floor), K = 128 in 8 chunks
    ("dgrad 128<-128 bstats", "e2.1 d2.1", run_dgrad,
     dict(N=2, H=128, W=256, Cin=128, Cout=128, stride=1, nxt=True),
     [split(T128, "bs")], X3),
    # 4 channel tiles x 128 splits of 4 segments (workload: 128 splits of 64); 128 slabs -> 2
    # REDUCE stages, as the workload
    ("wgrad 128->128", "e2.1 d2.1", run_wgrad, dict(N=2, H=32, W=128, Cx=128, Cout=128, stride=1),
     [WG3_64, REDUCE, REDUCE], X3),
    # eight-wave form: 8 channel tiles x 32 splits of 4 segments of 32 pixels (workload: 32 splits
    # of 32); 2 REDUCE stages
    ("up wgrad 256->128", "d2.0", run_up_wgrad, dict(N=2, h=32, w=64, Cx=256, Cout=128, cin_total=384),
     [wtaps("64, 64, 32, true, float, float, 8"), REDUCE, REDUCE], FP32),
    ("wgrad skip 128->128", "d2.0", run_wgrad,
     dict(N=2, H=32, W=128, Cx=128, Cout=128, stride=1, ci_off=256, cin_total=384),
     [WG3_64, REDUCE, REDUCE], X3),
    # M = 32768 (the floor of the 128 x 128 tile): 256 M tiles x 2 column tiles, K = 1152
    ("up dgrad 256<-128 bstats", "d2.0", run_up_dgrad,
     dict(N=2, h=64, w=256, C0=256, Cout=128, cin_total=384),
     [igemm(128, 128, 64, 64, False, 1)], FP32),
    ("dgrad skip 128<-128", "d2.0", run_dgrad,
     dict(N=2, H=128, W=256, Cin=128, Cout=128, stride=1, ci_off=256, cin_total=384),
     [split(T128, "plain")], X3),
    # <128,64,64,4>: 256 tiles x 2 column tiles (the floor), K = 256 in 16 chunks
    ("dgrad 256<-256 bstats", "e3.1 d1.1", run_dgrad,
     dict(N=2, H=64, W=256, Cin=256, Cout=256, stride=1, nxt=True),
     [split(T128, "bs")], X3),
    # 16 channel tiles x 32 splits of 8 segments (workload: 32 splits of 64); 32 slabs -> 2
    # REDUCE stages, as the workload
    ("wgrad 256->256", "e3.1 d1.1", run_wgrad, dict(N=2, H=32, W=64, Cx=256, Cout=256, stride=1),
     [WG3_64, REDUCE, REDUCE], X3),
    # 32 channel tiles x 8 splits of 4 segments (workload: 8 splits of 32); 1 REDUCE
    ("up wgrad 512->256", "d1.0", run_up_wgrad, dict(N=2, h=16, w=32, Cx=512, Cout=256, cin_total=768),
     [wtaps("64, 64, 32, true, float, float, 8"), REDUCE], FP32),
    ("wgrad skip 256->256", "d1.0", run_wgrad,
     dict(N=2, H=32, W=64, Cx=256, Cout=256, stride=1, ci_off=512, cin_total=768),
     [WG3_64, REDUCE, REDUCE], X3),
    # 64 x 64 GEMM tiles without K groups: M = 4096 in 64 tiles x 8 column tiles, K = 2304 in 72
    # chunks (smaller M takes the K-group form)
    ("up dgrad 512<-256 bstats", "d1.0", run_up_dgrad,
     dict(N=2, h=32, w=64, C0=512, Cout=256, cin_total=768),
     [igemm(64, 64, 32, 32, False, 1)], FP32),
    ("dgrad skip 256<-256", "d1.0", run_dgrad,
     dict(N=2, H=64, W=256, Cin=256, Cout=256, stride=1, ci_off=512, cin_total=768),
     [split(T128, "plain")], X3),
    # <64,64,32,4>: 32 tiles x 8 column tiles (the floor), K = 512 in 32 chunks, 16 reduction
    # tiles per image (workload: 8)
    ("dgrad 512<-512 bstats", "e4.1 d0.1", run_dgrad,
     dict(N=2, H=32, W=64, Cin=512, Cout=512, stride=1, nxt=True),
     [split(T64, "bs")], X3),
    # 64 channel tiles x 8 splits of 16 segments (workload: 8 splits of 64); 8 slabs -> 1 REDUCE
    ("wgrad 512->512 32", "e4.1 d0.1", run_wgrad, dict(N=2, H=16, W=64, Cx=512, Cout=512, stride=1),
     [WG3_64, REDUCE], X3),
    # 64 channel tiles x 2 splits of 4 segments (workload: 4 splits of 16); 1 REDUCE
    ("up wgrad 512->512", "d0.0", run_up_wgrad, dict(N=2, h=8, w=16, Cx=512, Cout=512, cin_total=1024),
     [wtaps("64, 64, 32, true, float, float, 8"), REDUCE], FP32),
    ("wgrad skip 512->512", "d0.0", run_wgrad,
     dict(N=2, H=16, W=64, Cx=512, Cout=512, stride=1, ci_off=512, cin_total=1024),
     [WG3_64, REDUCE], X3),
    # four K groups over K = 4608, M = 256 in 4 tiles, 2 reduction tiles per image
    ("up dgrad 512<-512 bstats", "d0.0", run_up_dgrad,
     dict(N=2, h=8, w=16, C0=512, Cout=512, cin_total=1024),
     [igemm(64, 64, 32, 32, False, 4)], FP32),
    ("dgrad skip 512<-512", "d0.0", run_dgrad,
     dict(N=2, H=32, W=64, Cin=512, Cout=512, stride=1, ci_off=512, cin_total=1024),
     [split(T64, "plain")], X3),
    # the 16 x 16 layer: gather-GEMM with four K groups, M = 256 in 4 tiles, 2 reduction tiles
    # of 64 per image
    ("dgrad 512<-512 16 bstats", "e5.1", run_dgrad,
     dict(N=2, H=8, W=16, Cin=512, Cout=512, stride=1, nxt=True, x3=False),
     [igemm(64, 64, 32, 32, False, 4)], SAME32),
    # Wo <= 16: segments of 16 = one image row; 64 channel tiles x 4 splits of 4 (workload: 8 of 16)
    ("wgrad 512->512 16", "e5.1", run_wgrad, dict(N=2, H=8, W=16, Cx=512, Cout=512, stride=1),
     [WG3_64, REDUCE], X3),
    # stride 2: the entry drops the split mode (data gradient with reductions: fp32 kernels; weight
    # gradient: the bf16 operand modes are for stride 1)
    # one launch per output parity class (4 / 2 / 2 / 1 taps), four K groups, accumulating into
    # the skip gradient; 8 reduction tiles of 64 per image
    ("dgrad s2 512<-512 bstats acc", "e5.0", run_dgrad,
     dict(N=2, H=16, W=32, Cin=512, Cout=512, stride=2, nxt=True, acc=True, x3=False),
     [igemm(64, 64, 32, 32, False, 4)] * 4, SAME32),
    # four-wave direct form (the x3 entry never takes the eight-wave one), segments of 16: 64
    # channel tiles x 4 splits of 4 (workload: 8 of 16)
    ("wgrad s2 512->512", "e5.0", run_wgrad,
     dict(N=2, H=16, W=32, Cx=512, Cout=512, stride=2, x3=False),
     [wgrad("64, 64, 16, 2, true, float, float, 4"), REDUCE], FP32),
    # dy grid 2 x 32 x 128: 64 tiles of 4 x 32 x 4 column tiles = 256 (the floor), K = 512 in 16
    # chunks per tap class; 64 reduction tiles per image; accumulating
    ("dgrad s2 256<-512 bstats acc", "e4.0", run_dgrad,
     dict(N=2, H=64, W=256, Cin=256, Cout=512, stride=2, nxt=True, acc=True, x3=False),
     [dgrad_s2("64, 32, 64, 4")], SAME32),
    # segments of 16: 32 channel tiles x 8 splits of 4 (workload: 16 splits of 32); 1 REDUCE
    ("wgrad s2 256->512", "e4.0", run_wgrad,
     dict(N=2, H=16, W=64, Cx=256, Cout=512, stride=2, x3=False),
     [wgrad("64, 64, 16, 2, true, float, float, 4"), REDUCE], FP32),
    ("dgrad s2 128<-256 bstats acc", "e3.0", run_dgrad,
     dict(N=2, H=128, W=256, Cin=128, Cout=256, stride=2, nxt=True, acc=True, x3=False),
     [dgrad_s2("64, 32, 64, 4")], SAME32),
    # 8 channel tiles x 64 splits of 4 segments (workload: 64 splits of 32); 64 slabs -> 2 REDUCE
    ("wgrad s2 128->256", "e3.0", run_wgrad,
     dict(N=2, H=64, W=128, Cx=128, Cout=256, stride=2, x3=False),
     [wgrad("64, 64, 16, 2, true, float, float, 4"), REDUCE, REDUCE], FP32),
    ("dgrad s2 64<-128 bstats acc", "e2.0", run_dgrad,
     dict(N=2, H=128, W=512, Cin=64, Cout=128, stride=2, nxt=True, acc=True, x3=False),
     [dgrad_s2("64, 32, 64, 4")], SAME32),
    # 2 channel tiles x 32 splits of 4 (workload: 256 splits of 32); 32 slabs -> 2 REDUCE, as the
    # workload's 256.  Two channel tiles: the fp32 entry stays on the four-wave kernel too
    ("wgrad s2 64->128", "e2.0", run_wgrad,
     dict(N=2, H=32, W=128, Cx=64, Cout=128, stride=2, x3=False),
     [wgrad("64, 64, 16, 2, true, float, float, 4"), REDUCE, REDUCE], SAME32),
    # dy grid 2 x 128 x 256 in 256 tiles of 8 x 32 (the floor), 32 columns; 128 reduction tiles per
    # image; accumulating
    ("dgrad s2 32<-64 bstats acc", "e1.0", run_dgrad,
     dict(N=2, H=256, W=512, Cin=32, Cout=64, stride=2, nxt=True, acc=True, x3=False),
     [dgrad_s2("32, 64, 32, 8")], SAME32),
    # 1088 segments of 32 pixels in 272 splits of 4 (workload: 512 splits of 32); 272 slabs -> 3
    # REDUCE stages, as the workload's 512
    ("wgrad s2 32->64", "e1.0", run_wgrad,
     dict(N=2, H=136, W=512, Cx=32, Cout=64, stride=2, x3=False),
     [wgrad("32, 64, 32, 2, true, float, float, 4"), REDUCE, REDUCE, REDUCE], SAME32),
    # 1088 stages of 128 pixels on 544 workgroups, 2 each (workload: 1024 x 16); 544 slabs -> 3
    # REDUCE stages, as the workload's 1024
    ("stem wgrad 3->32", "e0.0", run_stem_wgrad, dict(N=2, H=136, W=512),
     [STEM_WGRAD, REDUCE, REDUCE, REDUCE], SAME32),
]


def _row(ident):
    return next(r for r in LAYERS if r[0] == ident)


def _run(ua, row, **extra):
    return row[2](ua, MODE, **row[3], **extra)


def line(row, out):
    """One line of profiles/bf16x3_step_kernels_error.txt."""
    ident, layers, runner, kw, expected, kind = row
    shape = " ".join(f"{k}={v}" for k, v in kw.items() if k not in ("x3",))
    kernels = " + ".join(dict.fromkeys(HS.short(n) for n in out["names"]))
    s = f"{ident} | {shape} | {kernels} | {R.report(out['metrics'])}"
    if "term" in out:
        t = out["term"]
        s += f" | e_kernel {t['e_kernel']:.2e} e_drop {t['e_drop']:.2e} e_six {t['e_six']:.1e}"
    if "eq32" in out:
        s += f" | bit-equal to the fp32 entry: {out['eq32']}"
    return s


@pytest.fixture(scope="module")
def fp32_names():
    """Every kernel name a row of tests/test_fp32_step_kernels_gpu.py expects (by lookup: nothing
    of that file runs here)."""
    F = HS.load("test_fp32_step_kernels_gpu")
    return set().union(*(r[4] for r in F.LAYERS))


@pytest.mark.parametrize("row", LAYERS, ids=[r[0] for r in LAYERS])
def test_step_layer_bf16x3(ua, fp32_names, row):
    ident, layers, runner, kw, expected, kind = row
    out = _run(ua, row)
    print(line(row, out))
    assert out["names"] == list(expected), f"{ident} ({layers}) launched {out['names']}"
    bad = R.failures(out["metrics"])
    if kind == X3:
        assert any("split" in n or "bf16_kernel<" in n for n in expected)
        bad += term_failures(out["term"])
    else:
        assert "term" not in out
        stray = [n for n in expected if n not in fp32_names]
        assert not stray, f"{ident}: no row of the fp32 file holds {stray}"
        if kind == SAME32:
            assert out["eq32"], f"{ident}: the x3 entry and the fp32 entry differ"
    assert not bad, f"{ident} ({layers}):\n" + "\n".join(bad)


# --------------------------------------------------------------------------- the check can fail
# One x3 row of each kind against a reference evaluated with one row of one image zeroed (the
# input row for the forward, a dy row for the gradients): 1 / 128 .. 1 / 72 of an image's rows,
# the size of error a mis-indexed tile row or a dropped slab would make.
MISSING_ROW = [("fwd 64->64", (1, 77)), ("dgrad 64<-64 bstats", (1, 77)), ("wgrad 64->64", (1, 21))]


@pytest.mark.parametrize("ident,drop_row", MISSING_ROW, ids=[m[0] for m in MISSING_ROW])
def test_check_sees_one_missing_row(ua, ident, drop_row):
    row = _row(ident)
    assert row[5] == X3
    out = _run(ua, row, drop_row=drop_row)
    assert not R.failures(out["metrics"]), R.failures(out["metrics"])
    assert R.failures(out["bad"]), f"the check cannot see a missing row: {out['bad']}"


def test_term_check_sees_one_missing_product():
    """The term check on the reference alone: a six-product evaluation without one 2^-16
    product is rejected by the criterion the rows apply to the kernel (at e_drop by construction),
    the full one passes it with the 100 x floor to spare - for the K of the smallest row."""
    a = torch.nn.functional.leaky_relu(HS.grand((2, 32, 16, 32), 1).double(), HS.SLOPE)
    w = R.he_weight(32, 32, 2, 9 * 32).double()

    def fn(p, q):
        return R.ref_conv(p, q, None, 1)

    exact = fn(a, w)
    e_drop, e_six = R.term_check(fn, a, w, exact)
    assert e_six * TERM_FLOOR <= e_drop
    for k in R.THIRD_ORDER:
        t = dict(e_kernel=R.rel_l2(R.six_products(fn, a, w, leave_out=k), exact), e_drop=e_drop,
                 e_six=e_six)
        assert term_failures(t), f"a kernel without the product {k} would pass: {t}"
    assert not term_failures(dict(e_kernel=e_six, e_drop=e_drop, e_six=e_six))


# --------------------------------------------------------------------------- the other kernels
# HS.ALLOWED (name -> the test that holds it, that test's smallest call) plus this mode's own.
def _call_upsample(ua, mode):
    ua.ops.upsample2x_in_fwd(ua.ops.Act(HS.grand((1, 1, 1, 32), 1), *HS.coeffs(1, 32, 40)), HS.SLOPE)


ALLOWED = dict(HS.ALLOWED)
# the activated up-sampling this mode materialises for the decoder's first convolutions
ALLOWED[f"void {_AN}upsample2x_fwd_kernel<float>(float const*, float*, int, int, int, long long, "
        "float const*, float const*, float)"] = \
    ("test_fused_gpu.py::test_upsample2x_in_fwd", _call_upsample)


@pytest.mark.parametrize("name", sorted(ALLOWED), ids=HS.allowed_ids(ALLOWED))
def test_allowed_kernel_is_launched_by_its_test(ua, name):
    HS.check_allowed(ua, MODE, ALLOWED, name)


# --------------------------------------------------------------------------- closure
@pytest.fixture(scope="module")
def step_names(ua):
    """The launches of one eager bf16x3 training step of UNet() at N = 8, 512 x 512."""
    return HS.record_step(ua, MODE.name)


def test_every_bf16x3_step_kernel_is_held(step_names):
    """Every kernel of the step is one a row of LAYERS or an entry of ALLOWED holds: a dispatch
    change that sends a layer to another tile, or to the fp32 fallback, fails here or in its row."""
    HS.check_step_is_held(step_names, MODE.name, LAYERS, ALLOWED)


def test_every_row_kernel_runs_in_the_step(step_names):
    """The converse: a row (or an ALLOWED entry) for a kernel the step no longer launches is dead
    weight that still looks like coverage."""
    HS.check_rows_run_in_the_step(step_names, MODE.name, LAYERS, ALLOWED)


def test_the_step_runs_all_twelve_split_forms(step_names):
    """The four split tiles, each as fused forward, BSTATS data gradient and plain data gradient,
    and the two split weight-gradient instantiations: the kernels this mode exists for."""
    want = {split(t, f) for t in (T128, T64T, T64, T32T) for f in ("fwd", "bs", "plain")}
    want |= {WG3_32, WG3_64}
    assert want <= set(step_names), sorted(want - set(step_names))
    assert not any("igemm_split" in n for n in step_names)
