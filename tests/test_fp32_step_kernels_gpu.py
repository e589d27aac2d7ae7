"""Every fp32 kernel of the train step against fp64, at the smallest shape that selects it (-m gpu).

The benchmark's default mode is the fp32 step (N = 8, 512 x 512).  Its selectors switch on tile
counts as well as on shape, so a small test shape says nothing about the kernel the step runs
unless the launch is asserted.  The runners, bounds and shared kernel names are those of
tests/tools/step_kernel_harness.py; this file holds the fp32 operand mode (MODE) and its table.
Each row of LAYERS is one call of that step - the same `ops`
function with the operand mode unet.py uses for the layer (activation on load with per-image
coefficients, two sources where the layer has two, the Winograd weight forms of the PackTable
the network builds, a NextNorm where the network passes one, ci_offset / accumulate where it
uses them, the c32 switch as UNet.forward sets it) - at N = 2 and the smallest H != W grid for
which (a) the call launches the very instantiations it launches inside the step, the statistics
finalizer included, and (b) every loop the
workload shape runs more than once (K chunks, K groups, the persistent tile walk, slabs,
reduction stages, source switches) still runs more than once; (b) is the comment over the row.
The weight-gradient rows differ from the step in one way: the step's backward runs under
ops.wgrad_deferral(), where a layer call only queues its slabs and two or three batched launches
over a many-entry table reduce them at the end (tests/test_wgrad_defer_gpu.py holds that path).
A row makes the call undeferred, so its names end with that layer's own 1 - 3
wgrad_reduce_batched_kernel stages over a one-entry table; the stage counts in the notes are per
layer at the workload shape, not counts of the step.
Layers with the same call and channel geometry share a row; layers that only share kernel names
(the Winograd kernels of the 64..512-channel layers) keep a row per channel count, because the
chunk and column-tile counts differ.  Each case
  * records the launches of the call (ops.record_launches) and asserts they are the row's names;
  * holds the result to a float64 evaluation of the SAME fp32 operands, one image at a time on
    the GPU (tests/tools/fp64_layer_refs.py), within the bound the existing small-shape test of
    the same entry point uses (TOL_* of the harness: 2e-5 on y and dx, 5e-5 on rstd / alpha / beta,
    3e-5 on dw and the low-resolution gradients, 1e-5..2e-5 on the head, 5e-5 on the
    InstanceNorm backward);
  * forward rows check mean, rstd, alpha, beta; BSTATS rows check that the gradient is bit-equal
    to the call without the epilogue and drive the InstanceNorm backward from the summaries as
    test_fused_gpu.py::_in_bwd_both_ways does; accumulating rows start from a non-zero buffer;
    column-slice rows fill dw with a sentinel that the other columns must keep.
No row needed a bound of its own: every measured error is at most 0.12 of its bound (the
largest: taps D 1.2e-7 of 1e-6, fwd 256->512 s2 y 2.4e-6 of 2e-5); each case prints its figures.
test_check_sees_one_missing_row: one row of each kind must be REJECTED by the same comparison
against a reference with one row of one image zeroed.
test_every_fp32_step_kernel_is_held records one whole step at N = 8, 512 x 512 and requires
every kernel it launches to be a row's or an ALLOWED entry's; test_every_row_kernel_runs_in_the_
step is the converse.  ALLOWED names, per non-convolution kernel, the existing test that holds it
and that test's smallest call, which test_allowed_kernel_is_launched_by_its_test runs.

Rows are kept within 2 x 256 x 256 pixels at up to 64 channels and 65,536 pixels above that,
counted on the grid the kernel tiles.  The rows above those caps, and why:
  * "fwd 32->32" (2 x 264 x 512) and "up fwd 64+32->32" (output 2 x 264 x 512): the step's
    finalizer pair in_stats_finalize_grp / _comb needs >= 512 statistics tiles of 256 pixels PER
    IMAGE, i.e. >= 131072 pixels per image, and N >= 2;
  * "fwd 32->64 s2" (input 2 x 256 x 1024, output 2 x 128 x 512 = the cap): the same, 128-pixel
    tiles;
  * "dgrad 32<-32 bstats", "dgrad skip 32<-32" (2 x 136 x 512): conv_wino32q needs >= 512 tiles
    (= the cap) and runs on 512 persistent workgroups, so a second round needs more than the cap;
  * "dgrad s2 32<-64 bstats acc" (dx 2 x 256 x 512): the 32-column stride-2 form needs >= 256
    tiles of 8 x 32 on the dy grid;
  * "wgrad s2 32->64", "stem wgrad 3->32" (2 x 136 x 512): a third REDUCE stage needs > 256 slabs.
Below the caps but short of (b): the taps rows at C = 32 and C = 64.  The step's second pass of
the grid-stride loop needs more than 1,048,576 channel quads, i.e. dy above 2 x 256 x 512 at
C = 64 and four times that at C = 32; the loop is the same code for every C, so "taps 512 two
passes" reaches it within the cap and the per-C rows stay small.

Kernel -> row (shape N x H x W of the row's input grid; regime notes in LAYERS):
  conv_stem_fwd_walk_kernel<float, float, 8>        stem fwd 3->32             2 x 128 x 512
  conv_wino32q_kernel<true>                         fwd 32->32                 2 x 264 x 512
  conv_wino32q_kernel<false>                        dgrad 32<-32 bstats, skip  2 x 136 x 512
  conv_wino_up32_kernel                             up fwd 64+32->32           2 x 132 x 256 (low)
  conv_wino_kernel<true, true, false, false>        fwd 64->64 .. 512->512 32  2 x 128 x 256 .. 2 x 32 x 128
  conv_wino_kernel<true, true, false, true>         up fwd 512+512 .. 128+64   2 x 16 x 64 .. 2 x 64 x 128 (low)
  conv_wino_kernel<false, false, true, false>       dgrad 64<-64 .. 512<-512 bstats   (the forward shapes)
  conv_wino_kernel<false, false, false, false>      dgrad skip 64 .. 512              (the forward shapes)
  conv_patch_s2_kernel<64, 64, 32, 4>               fwd 32->64 s2, 256->512 s2 2 x 256 x 1024, 2 x 64 x 256
  conv_patch_s2_kernel<128, 64, 64, 4>              fwd 64->128 s2, 128->256 s2  2 x 256 x 512, 2 x 128 x 512
  conv_igemm_kernel<64, 64, 32, 32, 32, true, 4>    fwd 512->512 s2, 512->512 16  2 x 16 x 32, 2 x 8 x 16
  conv_igemm_kernel<64, 64, 32, 32, 32, false, 4>   up dgrad 512<-512, dgrad 512<-512 16, dgrad s2 512<-512
                                                                               2 x 8 x 16, 2 x 8 x 16, 2 x 16 x 32
  conv_igemm_kernel<64, 64, 32, 32, 32, false, 1>   up dgrad 64<-32, 512<-256  2 x 16 x 32, 2 x 32 x 64
  conv_igemm_kernel<128, 128, 64, 64, 32, false, 1> up dgrad 128<-64, 256<-128 2 x 128 x 256, 2 x 64 x 256
  conv_dgrad_s2_patch_kernel<64, 32, 64, 4>         dgrad s2 256<-512, 128<-256, 64<-128
                                                                               2 x 64 x 256, 2 x 128 x 256, 2 x 128 x 512
  conv_dgrad_s2_patch_kernel<32, 64, 32, 8>         dgrad s2 32<-64            2 x 256 x 512
  conv_wgrad_wino32_kernel<true>                    wgrad 32->32, skip         2 x 136 x 256
  conv_wgrad_wino_kernel<true>                      wgrad 64->64 .. 512->512 16, skips  2 x 32 x 128 .. 2 x 16 x 32
  conv_wgrad_kernel<64, 64, 16, 2, true, .., 8>     wgrad s2 512->512          2 x 16 x 32
  conv_wgrad_kernel<64, 64, 32, 2, true, .., 8>     wgrad s2 256->512, 128->256  2 x 16 x 64, 2 x 64 x 128
  conv_wgrad_kernel<64, 64, 16, 2, true, .., 4>     wgrad s2 64->128           2 x 32 x 128
  conv_wgrad_kernel<32, 64, 32, 2, true, .., 4>     wgrad s2 32->64            2 x 136 x 512
  conv_wgrad_taps_kernel<32, 32, 32, true, .., 4>   up wgrad 64->32            2 x 32 x 64
  conv_wgrad_taps_kernel<64, 64, 16, true, .., 4>   up wgrad 128->64           2 x 16 x 64
  conv_wgrad_taps_kernel<64, 64, 32, true, .., 8>   up wgrad 256->128, 512->256, 512->512
                                                                               2 x 32 x 64, 2 x 16 x 32, 2 x 8 x 16
  conv_stem_wgrad_rows_kernel<float, float>         stem wgrad 3->32           2 x 136 x 512
  wgrad_reduce_batched_kernel                       every wgrad row (1, 2 or 3 stages)
  upsample2x_bwd_taps_kernel<float, 1>              taps 32 .. 512, two passes 2 x 16 x 32, 2 x 8 x 16, 2 x 72 x 64 (low)
  in_stats_finalize_grp / _comb_kernel              stem fwd, fwd 32->32, fwd 32->64 s2, up fwd 64+32->32
  in_stats_finalize_eq_kernel                       every other forward row
  head_fwd_kernel<float>                            head fwd 32->3             2 x 32 x 64
  head_bwd_kernel<float>, head_bwd_finalize_kernel  head bwd 32->3             2 x 128 x 512
  in_bwd_finalize1_kernel, in_bwd_apply_kernel<float>  in bwd 32 fed, 512 fed  2 x 16 x 32, 2 x 8 x 16
  in_bwd_reduce_kernel<float> (not in the step)     EXTRA: in bwd 32 / 512 reduce
  nchw_to_nhwc, pack_w_batched, wino_pack_batched, loss_reduce / _finalize / _grad, sgd_nesterov
                                                    ALLOWED (the test named next to each)

Measured on an MI355X: the whole file 4.9 s for its 85 cases (1.0 s of it the recorded 8 x 512^2
step), its slowest row 0.83 s ("in bwd 32 fed", the first fp64 autograd call), every other row
at most 0.52 s - inside a few seconds per row and two minutes for the file.
"""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("step_kernel_harness", os.path.join(
    os.path.dirname(os.path.abspath(__file__)), "tools", "step_kernel_harness.py"))
HS = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(HS)
R = HS.R


# --------------------------------------------------------------------------- the operand mode
def pack(ua, w, stride):
    """The PackTable of one 3x3 layer as _Walk builds it in the fp32 mode: the packed layouts plus
    the Winograd forms of a stride-1 layer with >= 64 channels on both sides."""
    co, ci = w.shape[0], w.shape[1]
    s1 = stride == 1 and min(co, ci) >= 64
    return HS.pack_one(ua, w, False, [(s1 and co % 64 == 0 and ci % 8 == 0,
                                      s1 and ci % 64 == 0 and co % 8 == 0)])


def forms(ua, op, table, grid=None, held=True):
    """wu / ud: the Winograd form where the PackTable holds one, the walk holds it for this source
    and the Winograd kernel tiles the grid; bf16 = "fp32" on the data gradient."""
    def form(u, supported):
        return u if u is not None and held and supported(*grid) else None

    if op == "fwd":
        return dict(wu=form(table.uf[0], ua.ops.conv_wino_supported))
    if op == "up_fwd":
        return dict(wu=form(table.uf[0], ua.ops.conv_up_wino_supported))
    if op == "dgrad":
        return dict(bf16="fp32", ud=form(table.ud[0], ua.ops.conv_wino_supported))
    return {}


MODE = HS.Mode("fp32", False, pack, forms)

# --------------------------------------------------------------------------- the table
# The runners and the kernel names more than one table uses: tests/tools/step_kernel_harness.py.
run_fwd, run_stem_fwd, run_up_fwd, run_dgrad = HS.run_fwd, HS.run_stem_fwd, HS.run_up_fwd, HS.run_dgrad
run_wgrad, run_stem_wgrad, run_taps, run_up_wgrad = \
    HS.run_wgrad, HS.run_stem_wgrad, HS.run_taps, HS.run_up_wgrad
run_up_dgrad, run_head_fwd, run_head_bwd, run_in_bwd = \
    HS.run_up_dgrad, HS.run_head_fwd, HS.run_head_bwd, HS.run_in_bwd
patch_s2, dgrad_s2, igemm, wgrad, wtaps = HS.patch_s2, HS.dgrad_s2, HS.igemm, HS.wgrad, HS.wtaps
REDUCE, FIN_GRP, FIN_COMB, FIN_EQ, TAPS = HS.REDUCE, HS.FIN_GRP, HS.FIN_COMB, HS.FIN_EQ, HS.TAPS
STEM_FWD, STEM_WGRAD, HEAD_FWD, HEAD_BWD = HS.STEM_FWD, HS.STEM_WGRAD, HS.HEAD_FWD, HS.HEAD_BWD
HEAD_BWD_FIN, IN_FIN1, IN_APPLY, IN_REDUCE = HS.HEAD_BWD_FIN, HS.IN_FIN1, HS.IN_APPLY, HS.IN_REDUCE
_NS, _AN = HS._NS, HS._AN


# The Winograd kernels of this mode.
def wino(act, stats, bstats, up):
    """conv_wino_kernel<ACT, STATS, BSTATS, UP>"""
    t = ", ".join("true" if f else "false" for f in (act, stats, bstats, up))
    return f"void {_NS}conv_wino_kernel<{t}>({_NS}WinoParams)"


def wino32q(fused):
    return f"void {_NS}conv_wino32q_kernel<{'true' if fused else 'false'}>(unet_conv::IgemmParams, int)"


WINO_UP32 = f"{_NS}conv_wino_up32_kernel(unet_conv::IgemmParams, int)"
WGRAD_WINO = f"void {_AN}conv_wgrad_wino_kernel<true>({_AN}WgradParams)"
WGRAD_WINO32 = f"void {_AN}conv_wgrad_wino32_kernel<true>({_AN}WgradParams, int)"

# (id, the layers of UNet() it stands for, runner, arguments, expected kernel names in launch
# order).  Encoder stage e, conv k: "e<e>.<k>"; decoder stage d: "d<d>.<k>".  Layers with the same
# call and channel geometry share a row.  The comment over a row is its regime note (b): what
# the workload shape (8 x 512^2) loops over, and what is left of it at the row's shape.
LAYERS = [
    # ---- forward
    # walk over 8-row strips, 512 statistics tiles per image (the floor of the two-level
    # finalizer); workload: 2048 per image
    ("stem fwd 3->32", "e0.0", run_stem_fwd, dict(N=2, H=128, W=512),
     [STEM_FWD, FIN_GRP, FIN_COMB]),
    # 1056 tiles of 8 x 32 on 512 persistent workgroups: 3 rounds, the last partial (workload: 8);
    # 528 statistics tiles per image -> two-level finalizer (>= 512; workload 1024)
    ("fwd 32->32", "e0.1 d4.1", run_fwd, dict(N=2, H=264, W=512, C0=32, C1=0, Cout=32, stride=1),
     [wino32q(True), FIN_GRP, FIN_COMB]),
    # one 4 x 32 output tile per workgroup, K = 32 in one chunk per tap (as the workload);
    # 512 statistics tiles per image -> two-level finalizer
    ("fwd 32->64 s2", "e1.0", run_fwd, dict(N=2, H=256, W=1024, C0=32, C1=0, Cout=64, stride=2),
     [patch_s2("64, 64, 32, 4"), FIN_GRP, FIN_COMB]),
    # conv_wino rows: one 8 x 32 tile x 64 columns per workgroup (no walk), K = C in C / 8
    # chunks, Cout / 64 column tiles, >= 256 tiles (the selector's floor); an image holds several
    # tiles, so the one-level finalizer merges several summaries per (n, c)
    # K = 64 in 8 chunks, 1 column tile, 256 tiles, 128 per image
    ("fwd 64->64", "e1.1 d3.1", run_fwd, dict(N=2, H=128, W=256, C0=64, C1=0, Cout=64, stride=1),
     [wino(1, 1, 0, 0), FIN_EQ]),
    # 512 tiles x 1 column tile of 128 (the floor), K = 64 in two 32-channel chunks per tap
    ("fwd 64->128 s2", "e2.0", run_fwd, dict(N=2, H=256, W=512, C0=64, C1=0, Cout=128, stride=2),
     [patch_s2("128, 64, 64, 4"), FIN_EQ]),
    # K = 128 in 16 chunks, 2 column tiles, 128 x 2 tiles
    ("fwd 128->128", "e2.1 d2.1", run_fwd, dict(N=2, H=64, W=256, C0=128, C1=0, Cout=128, stride=1),
     [wino(1, 1, 0, 0), FIN_EQ]),
    # 256 tiles x 2 column tiles of 128, K = 128 in four chunks per tap
    ("fwd 128->256 s2", "e3.0", run_fwd, dict(N=2, H=128, W=512, C0=128, C1=0, Cout=256, stride=2),
     [patch_s2("128, 64, 64, 4"), FIN_EQ]),
    # K = 256 in 32 chunks, 4 column tiles, 64 x 4 tiles
    ("fwd 256->256", "e3.1 d1.1", run_fwd, dict(N=2, H=64, W=128, C0=256, C1=0, Cout=256, stride=1),
     [wino(1, 1, 0, 0), FIN_EQ]),
    # 64 tiles x 8 column tiles of 64 (the floor; the workload has 128 x 8), K = 256 in 8 chunks
    ("fwd 256->512 s2", "e4.0", run_fwd, dict(N=2, H=64, W=256, C0=256, C1=0, Cout=512, stride=2),
     [patch_s2("64, 64, 32, 4"), FIN_EQ]),
    # K = 512 in 64 chunks, 8 column tiles, 32 x 8 tiles, 16 per image (workload: 4)
    ("fwd 512->512 32", "e4.1 d0.1", run_fwd, dict(N=2, H=32, W=128, C0=512, C1=0, Cout=512, stride=1),
     [wino(1, 1, 0, 0), FIN_EQ]),
    # gather-GEMM 64 x 64, M = 256 output pixels in 4 tiles (2 per image) x 8 column tiles,
    # K = 9 x 512 in four K groups
    ("fwd 512->512 s2", "e5.0", run_fwd, dict(N=2, H=16, W=32, C0=512, C1=0, Cout=512, stride=2),
     [igemm(64, 64, 32, 32, True, 4), FIN_EQ]),
    # the same kernel at stride 1: M = 256 in 4 tiles (2 per image), four K groups
    ("fwd 512->512 16", "e5.1", run_fwd, dict(N=2, H=8, W=16, C0=512, C1=0, Cout=512, stride=1),
     [igemm(64, 64, 32, 32, True, 4), FIN_EQ]),
    # conv_wino with the up-sampling loader: K = C0 + C1 in chunks of 8, the source switch at
    # chunk C0 / 8; output grids of 2h x 2w
    # K = 1024 in 128 chunks (switch at 64), 8 column tiles, 32 x 8 tiles
    ("up fwd 512+512->512", "d0.0", run_up_fwd, dict(N=2, h=16, w=64, C0=512, C1=512, Cout=512),
     [wino(1, 1, 0, 1), FIN_EQ]),
    # K = 768 in 96 chunks (switch at 64), 4 column tiles, 64 x 4 tiles
    ("up fwd 512+256->256", "d1.0", run_up_fwd, dict(N=2, h=32, w=64, C0=512, C1=256, Cout=256),
     [wino(1, 1, 0, 1), FIN_EQ]),
    # K = 384 in 48 chunks (switch at 32), 2 column tiles, 128 x 2 tiles
    ("up fwd 256+128->128", "d2.0", run_up_fwd, dict(N=2, h=32, w=128, C0=256, C1=128, Cout=128),
     [wino(1, 1, 0, 1), FIN_EQ]),
    # K = 192 in 24 chunks (switch at 16), 1 column tile, 256 tiles
    ("up fwd 128+64->64", "d3.0", run_up_fwd, dict(N=2, h=64, w=128, C0=128, C1=64, Cout=64),
     [wino(1, 1, 0, 1), FIN_EQ]),
    # K = 96 in three register-resident chunks; 1056 tiles on 256 persistent workgroups: 5
    # rounds, the last partial (workload: 16); 528 statistics tiles per image -> two-level finalizer
    ("up fwd 64+32->32", "d4.0", run_up_fwd, dict(N=2, h=132, w=256, C0=64, C1=32, Cout=32),
     [WINO_UP32, FIN_GRP, FIN_COMB]),
    # a grid-stride loop over pixels; several workgroups per image
    ("head fwd 32->3", "head", run_head_fwd, dict(N=2, H=32, W=64),
     [HEAD_FWD]),
    # ---- backward: head, InstanceNorm, then per layer kind
    # 2048 tiles of 64 pixels on 1024 workgroups (the grid's cap): 2 tiles per workgroup, dw / db
    # accumulated over them and ONE summary per 128-pixel range, 512 ranges per image (workload:
    # 32 tiles per workgroup, 128 ranges per image)
    ("head bwd 32->3", "head", run_head_bwd, dict(N=2, H=128, W=512),
     [HEAD_BWD, HEAD_BWD_FIN]),
    # InstanceNorm backward fed by BSTATS summaries (every one of the step's 22 calls): 8
    # summaries of 64 pixels per (image, channel) merged by the finalizer, then the apply pass
    ("in bwd 32 fed", "every layer", run_in_bwd, dict(N=2, H=16, W=32, C=32, fed=True),
     [IN_FIN1, IN_APPLY]),
    # 512 channels: 2 summaries per (image, channel)
    ("in bwd 512 fed", "every layer", run_in_bwd, dict(N=2, H=8, W=16, C=512, fed=True),
     [IN_FIN1, IN_APPLY]),
    # 544 tiles on 512 persistent workgroups: 2 rounds, the last partial (workload: 8); 272
    # reduction tiles per image
    ("dgrad 32<-32 bstats", "e0.1 d4.1", run_dgrad,
     dict(N=2, H=136, W=512, Cin=32, Cout=32, stride=1, nxt=True),
     [wino32q(False)]),
    # the same walk; columns 64..95 of the 96-channel weight, no epilogue
    ("dgrad skip 32<-32", "d4.0", run_dgrad,
     dict(N=2, H=136, W=512, Cin=32, Cout=32, stride=1, ci_off=64, cin_total=96),
     [wino32q(False)]),
    # 272 tiles on 256 persistent workgroups: 2 rounds, the last partial (workload: 16); 256
    # slabs -> 2 REDUCE stages (16 x per stage), as the workload
    ("wgrad 32->32", "e0.1 d4.1", run_wgrad, dict(N=2, H=136, W=256, Cx=32, Cout=32, stride=1),
     [WGRAD_WINO32, REDUCE, REDUCE]),
    ("wgrad skip 32->32", "d4.0", run_wgrad,
     dict(N=2, H=136, W=256, Cx=32, Cout=32, stride=1, ci_off=64, cin_total=96),
     [WGRAD_WINO32, REDUCE, REDUCE]),
    # taps: one thread per (low-resolution pixel, channel quad) in a grid-stride loop over a grid
    # capped at 4096 x 256 threads.  The workload makes 4 passes at C = 32 and 2 at C = 64, one
    # at C >= 128; the small rows make one pass, "taps 512 two passes" makes two, the second
    # partial (2 x 72 x 64 x 128 = 1179648 quads), within the cap of 65,536 dy pixels
    ("taps 32", "d4.0", run_taps, dict(N=2, h=16, w=32, C=32), [TAPS]),
    ("taps 64", "d3.0", run_taps, dict(N=2, h=16, w=32, C=64), [TAPS]),
    ("taps 128", "d2.0", run_taps, dict(N=2, h=16, w=32, C=128), [TAPS]),
    ("taps 256", "d1.0", run_taps, dict(N=2, h=8, w=16, C=256), [TAPS]),
    ("taps 512", "d0.0", run_taps, dict(N=2, h=8, w=16, C=512), [TAPS]),
    ("taps 512 two passes", "d4.0 d3.0 (the loop)", run_taps, dict(N=2, h=72, w=64, C=512), [TAPS]),
    # 128 segments of 32 pixels in 32 splits of 4 (workload: 256 splits of 64); 32 slabs -> 2
    # REDUCE stages, as the workload's 256
    ("up wgrad 64->32", "d4.0", run_up_wgrad, dict(N=2, h=32, w=64, Cx=64, Cout=32, cin_total=96),
     [wtaps("32, 32, 32, true, float, float, 4"), REDUCE, REDUCE]),
    # plain GEMM, K = 288 in 9 chunks, M = 1024 in 16 tiles, 8 reduction tiles per image
    ("up dgrad 64<-32 bstats", "d4.0", run_up_dgrad, dict(N=2, h=16, w=32, C0=64, Cout=32, cin_total=96),
     [igemm(64, 64, 32, 32, False, 1)]),
    # conv_wino data gradients: as the forward rows (K = Cout in chunks of 8, Cin / 64 column
    # tiles), 256-pixel reduction tiles, several per image
    ("dgrad 64<-64 bstats", "e1.1 d3.1", run_dgrad,
     dict(N=2, H=128, W=256, Cin=64, Cout=64, stride=1, nxt=True),
     [wino(0, 0, 1, 0)]),
    # 256 chunks of 16 x 2 pixels in 32 splits of 8 (workload: 256 splits of 64); 32 slabs -> 2
    # REDUCE stages, as the workload's 256
    ("wgrad 64->64", "e1.1 d3.1", run_wgrad, dict(N=2, H=32, W=128, Cx=64, Cout=64, stride=1),
     [WGRAD_WINO, REDUCE, REDUCE]),
    # 128 segments of 16 pixels in 32 splits of 4 (workload: 256 splits of 32); 2 REDUCE stages
    ("up wgrad 128->64", "d3.0", run_up_wgrad, dict(N=2, h=16, w=64, Cx=128, Cout=64, cin_total=192),
     [wtaps("64, 64, 16, true, float, float, 4"), REDUCE, REDUCE]),
    ("wgrad skip 64->64", "d3.0", run_wgrad,
     dict(N=2, H=32, W=128, Cx=64, Cout=64, stride=1, ci_off=128, cin_total=192),
     [WGRAD_WINO, REDUCE, REDUCE]),
    # the 128 x 128 GEMM tile needs M >= 65536 (the selector's floor): 512 M tiles, K = 576 in
    # 18 chunks, 128 columns in one tile
    ("up dgrad 128<-64 bstats", "d3.0", run_up_dgrad, dict(N=2, h=128, w=256, C0=128, Cout=64, cin_total=192),
     [igemm(128, 128, 64, 64, False, 1)]),
    ("dgrad skip 64<-64", "d3.0", run_dgrad,
     dict(N=2, H=128, W=256, Cin=64, Cout=64, stride=1, ci_off=128, cin_total=192),
     [wino(0, 0, 0, 0)]),
    ("dgrad 128<-128 bstats", "e2.1 d2.1", run_dgrad,
     dict(N=2, H=64, W=256, Cin=128, Cout=128, stride=1, nxt=True),
     [wino(0, 0, 1, 0)]),
    # 4 channel tiles x 32 splits of 8 chunks (workload: 64 splits of 64); 2 REDUCE stages
    ("wgrad 128->128", "e2.1 d2.1", run_wgrad, dict(N=2, H=32, W=128, Cx=128, Cout=128, stride=1),
     [WGRAD_WINO, REDUCE, REDUCE]),
    # eight-wave form: 8 channel tiles x 32 splits of 4 segments of 32 pixels (workload: 32 splits
    # of 32); 2 REDUCE stages
    ("up wgrad 256->128", "d2.0", run_up_wgrad, dict(N=2, h=32, w=64, Cx=256, Cout=128, cin_total=384),
     [wtaps("64, 64, 32, true, float, float, 8"), REDUCE, REDUCE]),
    ("wgrad skip 128->128", "d2.0", run_wgrad,
     dict(N=2, H=32, W=128, Cx=128, Cout=128, stride=1, ci_off=256, cin_total=384),
     [WGRAD_WINO, REDUCE, REDUCE]),
    # M = 32768 (the floor of the 128 x 128 tile): 256 M tiles x 2 column tiles, K = 1152
    ("up dgrad 256<-128 bstats", "d2.0", run_up_dgrad, dict(N=2, h=64, w=256, C0=256, Cout=128, cin_total=384),
     [igemm(128, 128, 64, 64, False, 1)]),
    ("dgrad skip 128<-128", "d2.0", run_dgrad,
     dict(N=2, H=64, W=256, Cin=128, Cout=128, stride=1, ci_off=256, cin_total=384),
     [wino(0, 0, 0, 0)]),
    ("dgrad 256<-256 bstats", "e3.1 d1.1", run_dgrad,
     dict(N=2, H=64, W=128, Cin=256, Cout=256, stride=1, nxt=True),
     [wino(0, 0, 1, 0)]),
    # 16 channel tiles x 8 splits of 8 chunks (workload: 16 splits of 64); <= 16 slabs -> 1 REDUCE
    ("wgrad 256->256", "e3.1 d1.1", run_wgrad, dict(N=2, H=16, W=64, Cx=256, Cout=256, stride=1),
     [WGRAD_WINO, REDUCE]),
    # 32 channel tiles x 8 splits of 4 segments (workload: 8 splits of 32); 1 REDUCE
    ("up wgrad 512->256", "d1.0", run_up_wgrad, dict(N=2, h=16, w=32, Cx=512, Cout=256, cin_total=768),
     [wtaps("64, 64, 32, true, float, float, 8"), REDUCE]),
    ("wgrad skip 256->256", "d1.0", run_wgrad,
     dict(N=2, H=16, W=64, Cx=256, Cout=256, stride=1, ci_off=512, cin_total=768),
     [WGRAD_WINO, REDUCE]),
    # 64 x 64 GEMM tiles without K groups: M = 4096 in 64 tiles x 8 column tiles, K = 2304 in 72
    # chunks (smaller M takes the K-group form)
    ("up dgrad 512<-256 bstats", "d1.0", run_up_dgrad, dict(N=2, h=32, w=64, C0=512, Cout=256, cin_total=768),
     [igemm(64, 64, 32, 32, False, 1)]),
    ("dgrad skip 256<-256", "d1.0", run_dgrad,
     dict(N=2, H=64, W=128, Cin=256, Cout=256, stride=1, ci_off=512, cin_total=768),
     [wino(0, 0, 0, 0)]),
    ("dgrad 512<-512 bstats", "e4.1 d0.1", run_dgrad,
     dict(N=2, H=32, W=128, Cin=512, Cout=512, stride=1, nxt=True),
     [wino(0, 0, 1, 0)]),
    # 64 channel tiles x 4 splits of 16 chunks (workload: 4 splits of 64); 1 REDUCE
    ("wgrad 512->512 32", "e4.1 d0.1", run_wgrad, dict(N=2, H=16, W=64, Cx=512, Cout=512, stride=1),
     [WGRAD_WINO, REDUCE]),
    # 64 channel tiles x 2 splits of 4 segments (workload: 4 splits of 16); 1 REDUCE
    ("up wgrad 512->512", "d0.0", run_up_wgrad, dict(N=2, h=8, w=16, Cx=512, Cout=512, cin_total=1024),
     [wtaps("64, 64, 32, true, float, float, 8"), REDUCE]),
    ("wgrad skip 512->512", "d0.0", run_wgrad,
     dict(N=2, H=16, W=64, Cx=512, Cout=512, stride=1, ci_off=512, cin_total=1024),
     [WGRAD_WINO, REDUCE]),
    # four K groups over K = 4608, M = 256 in 4 tiles, 2 reduction tiles per image
    ("up dgrad 512<-512 bstats", "d0.0", run_up_dgrad, dict(N=2, h=8, w=16, C0=512, Cout=512, cin_total=1024),
     [igemm(64, 64, 32, 32, False, 4)]),
    ("dgrad skip 512<-512", "d0.0", run_dgrad,
     dict(N=2, H=32, W=128, Cin=512, Cout=512, stride=1, ci_off=512, cin_total=1024),
     [wino(0, 0, 0, 0)]),
    # gather-GEMM with four K groups, M = 256 in 4 tiles, 2 reduction tiles of 64 per image
    ("dgrad 512<-512 16 bstats", "e5.1", run_dgrad,
     dict(N=2, H=8, W=16, Cin=512, Cout=512, stride=1, nxt=True),
     [igemm(64, 64, 32, 32, False, 4)]),
    # the smallest grid the Winograd form takes (32 chunks): 64 channel tiles x 4 splits of 8
    ("wgrad 512->512 16", "e5.1", run_wgrad, dict(N=2, H=16, W=32, Cx=512, Cout=512, stride=1),
     [WGRAD_WINO, REDUCE]),
    # one launch per output parity class (4 / 2 / 2 / 1 taps), four K groups, accumulating into
    # the skip gradient; 8 reduction tiles of 64 per image
    ("dgrad s2 512<-512 bstats acc", "e5.0", run_dgrad,
     dict(N=2, H=16, W=32, Cin=512, Cout=512, stride=2, nxt=True, acc=True),
     [igemm(64, 64, 32, 32, False, 4)] * 4),
    # eight-wave direct form, segments of 16: 64 channel tiles x 4 splits of 4 (workload: 4 of 32)
    ("wgrad s2 512->512", "e5.0", run_wgrad, dict(N=2, H=16, W=32, Cx=512, Cout=512, stride=2),
     [wgrad("64, 64, 16, 2, true, float, float, 8"), REDUCE]),
    # dy grid 2 x 32 x 128: 64 tiles of 4 x 32 x 4 column tiles = 256 (the floor), K = 512 in 16
    # chunks per tap class; 64 reduction tiles per image; accumulating
    ("dgrad s2 256<-512 bstats acc", "e4.0", run_dgrad,
     dict(N=2, H=64, W=256, Cin=256, Cout=512, stride=2, nxt=True, acc=True),
     [dgrad_s2("64, 32, 64, 4")]),
    # segments of 32: 32 channel tiles x 4 splits of 4 (workload: 8 splits of 32); 1 REDUCE
    ("wgrad s2 256->512", "e4.0", run_wgrad, dict(N=2, H=16, W=64, Cx=256, Cout=512, stride=2),
     [wgrad("64, 64, 32, 2, true, float, float, 8"), REDUCE]),
    ("dgrad s2 128<-256 bstats acc", "e3.0", run_dgrad,
     dict(N=2, H=128, W=256, Cin=128, Cout=256, stride=2, nxt=True, acc=True),
     [dgrad_s2("64, 32, 64, 4")]),
    # 8 channel tiles x 32 splits of 4 segments (workload: 32 splits of 32); 32 slabs -> 2 REDUCE
    ("wgrad s2 128->256", "e3.0", run_wgrad, dict(N=2, H=64, W=128, Cx=128, Cout=256, stride=2),
     [wgrad("64, 64, 32, 2, true, float, float, 8"), REDUCE, REDUCE]),
    ("dgrad s2 64<-128 bstats acc", "e2.0", run_dgrad,
     dict(N=2, H=128, W=512, Cin=64, Cout=128, stride=2, nxt=True, acc=True),
     [dgrad_s2("64, 32, 64, 4")]),
    # four-wave form, segments of 16: 2 channel tiles x 32 splits of 4 (workload: 256 splits of
    # 32); 32 slabs -> 2 REDUCE, as the workload's 256
    ("wgrad s2 64->128", "e2.0", run_wgrad, dict(N=2, H=32, W=128, Cx=64, Cout=128, stride=2),
     [wgrad("64, 64, 16, 2, true, float, float, 4"), REDUCE, REDUCE]),
    # dy grid 2 x 128 x 256 in 256 tiles of 8 x 32 (the floor), 32 columns; 128 reduction tiles per
    # image; accumulating
    ("dgrad s2 32<-64 bstats acc", "e1.0", run_dgrad,
     dict(N=2, H=256, W=512, Cin=32, Cout=64, stride=2, nxt=True, acc=True),
     [dgrad_s2("32, 64, 32, 8")]),
    # 1088 segments of 32 pixels in 272 splits of 4 (workload: 512 splits of 32); 272 slabs -> 3
    # REDUCE stages, as the workload's 512
    ("wgrad s2 32->64", "e1.0", run_wgrad, dict(N=2, H=136, W=512, Cx=32, Cout=64, stride=2),
     [wgrad("32, 64, 32, 2, true, float, float, 4"), REDUCE, REDUCE, REDUCE]),
    # 1088 stages of 128 pixels on 544 workgroups, 2 each (workload: 1024 x 16); 544 slabs -> 3
    # REDUCE stages, as the workload's 1024
    ("stem wgrad 3->32", "e0.0", run_stem_wgrad, dict(N=2, H=136, W=512),
     [STEM_WGRAD, REDUCE, REDUCE, REDUCE]),
]

# The stand-alone reduction pass of the InstanceNorm backward: the fp32 step never launches it
# (every gradient comes with BSTATS summaries), the stand-alone pipeline and odd shapes do, and
# HS.summaries compares against it - so it is held against fp64 here too, outside LAYERS.
EXTRA = [
    ("in bwd 32 reduce", "stand-alone pipeline", run_in_bwd, dict(N=2, H=16, W=32, C=32, fed=False)),
    ("in bwd 512 reduce", "stand-alone pipeline", run_in_bwd, dict(N=2, H=8, W=16, C=512, fed=False)),
]


@pytest.mark.parametrize("row", LAYERS, ids=[r[0] for r in LAYERS])
def test_step_layer_fp32(ua, row):
    ident, layers, runner, kw, expected = row
    out = runner(ua, MODE, **kw)
    print(f"{ident}: {R.report(out['metrics'])}")
    assert out["names"] == list(expected), f"{ident} ({layers}) launched {out['names']}"
    bad = R.failures(out["metrics"])
    assert not bad, f"{ident} ({layers}):\n" + "\n".join(bad)


@pytest.mark.parametrize("row", EXTRA, ids=[r[0] for r in EXTRA])
def test_instnorm_backward_reduction_pass(ua, row):
    ident, layers, runner, kw = row
    out = runner(ua, MODE, **kw)
    names = out["names"]
    print(f"{ident}: {R.report(out['metrics'])}")
    assert IN_REDUCE in names and names[-1] == IN_APPLY, f"{ident} launched {names}"
    bad = R.failures(out["metrics"])
    assert not bad, f"{ident} ({layers}):\n" + "\n".join(bad)


# --------------------------------------------------------------------------- the check can fail
# One row of each kind against a reference evaluated with one row of one image zeroed (the
# input row for the forward, a dy row for the gradients): 1 / 128 .. 1 / 16 of an image's rows,
# the size of error a mis-indexed tile row or a dropped slab would make.
MISSING_ROW = [("fwd 64->64", (1, 77)), ("dgrad 64<-64 bstats", (1, 77)), ("wgrad 64->64", (1, 21)),
               ("taps 64", (1, 21))]


@pytest.mark.parametrize("ident,drop_row", MISSING_ROW, ids=[m[0] for m in MISSING_ROW])
def test_check_sees_one_missing_row(ua, ident, drop_row):
    row = next(r for r in LAYERS if r[0] == ident)
    out = row[2](ua, MODE, drop_row=drop_row, **row[3])
    assert not R.failures(out["metrics"]), R.failures(out["metrics"])
    assert R.failures(out["bad"]), f"the check cannot see a missing row: {out['bad']}"


# --------------------------------------------------------------------------- the other kernels
# HS.ALLOWED (name -> the test that holds it, that test's smallest call) plus this mode's own.
def _call_wino_pack(ua, mode):
    ua.ops.PackTable([HS.grand((64, 64, 3, 3), 1), HS.grand((32, 32, 3, 3), 4)], False,
                     [(True, True), (False, False)]).run()


ALLOWED = dict(HS.ALLOWED)
ALLOWED[f"{_NS}wino_pack_batched_kernel(unet_wino_pack_entry const*, int)"] = \
    ("test_fused_gpu.py::test_winograd_weight_packing_in_one_launch", _call_wino_pack)


@pytest.mark.parametrize("name", sorted(ALLOWED), ids=HS.allowed_ids(ALLOWED))
def test_allowed_kernel_is_launched_by_its_test(ua, name):
    HS.check_allowed(ua, MODE, ALLOWED, name)


# --------------------------------------------------------------------------- closure
@pytest.fixture(scope="module")
def step_names(ua):
    """The launches of one eager fp32 training step of UNet() at N = 8, 512 x 512."""
    return HS.record_step(ua, MODE.name)


def test_every_fp32_step_kernel_is_held(step_names):
    """Every kernel of the step is one a row of LAYERS or an entry of ALLOWED holds: a dispatch
    change that brings in another fp32 kernel fails here until a case holds it."""
    HS.check_step_is_held(step_names, MODE.name, LAYERS, ALLOWED)


def test_every_row_kernel_runs_in_the_step(step_names):
    """The converse: a row (or an ALLOWED entry) for a kernel the step no longer launches is dead
    weight that still looks like coverage."""
    HS.check_rows_run_in_the_step(step_names, MODE.name, LAYERS, ALLOWED)


