"""Every weight-gradient instantiation the plan rule of csrc/conv_wgrad.hip can reach, held to
float64 with its launch asserted (-m gpu).

One table, one case per row.  A row states the entry point, the operand mode, the shape, the
column slice (off, extra), the chunk size, the edge it is there for, and - written out by hand -
the compute launches the call must make.  A case
  * asserts the recorded compute launches equal the row's (reduction launches filtered out as
    tests/test_wgrad_defer_gpu.py does);
  * asserts the columns of dw outside the slice keep the sentinel;
  * compares dw with the row's float64 reference (tests/tools/wgrad_refs.py: it rounds what the
    row's kernel rounds, see there), max |dw - ref| / max |ref| <= the bound;
  * compares again with the reference whose dy lacks the pixel (N - 1, Ho - 1, Wo - 1): that
    comparison must FAIL the same bound (the check of the check);
  * where the row asks for db, compares db as well;
  * on a split-bf16 kernel, applies the term check of tests/test_bf16x3_step_kernels_gpu.py; where
    the bf16 / split entry lands on an fp32 kernel, requires the result bit-equal to the fp32
    entry's (the harness's eq32 rule).

The bounds are those of the existing small-shape tests (tests/tools/step_kernel_harness.py):
TOL_DW = 3e-5, 2e-5 for the 32-channel Winograd form as tests/test_wgrad_defer_gpu.py has it,
TOL_UP = 3e-5 for the tap entries, TOL_DW for db (tests/test_kernels_gpu.py's bias gradient).
The bf16-tensor rows take the same bounds: their references round as the loaders round.  No
bound was calibrated from a kernel's error.

WHICH ROWS.  tests/tools/wgrad_plan_model.py restates the plan rule; over its grid (storage x
cores, activation, stride, Cx and Cout in {32 .. 256}, N in {1, 2, 3}, H in {4 .. 64}, W in
{8 .. 136}, c32 "always", the tap entries, the stem) it reaches 138 instantiations, and the
first row of each here is the cheapest request of the grid that selects it.  The rows after
those are the edges, one row each on at least one instantiation of every family the edge can
occur in: a ragged last segment, a short last workgroup, N = 3, a column slice, a chunked batch
with activation on load, odd H and W at stride 2, more than one ring strip, db on both paths of
bias_grad_kernel, the centre-tap forms.  tests/test_wgrad_plan_model_cpu.py asserts, without a
GPU, that the model gives every row the launches the row states, that the table's name set
equals the grid's, and each edge from the model's plan fields.  (The model finds no request at
or below 2 x 128 x 128 that queues three reduction stages - that takes more than 256 slabs,
2 x 256 x 256 - so the one large row here is the two-stage 128-slab one; the three-stage
reduction stays with tests/test_wgrad_defer_gpu.py.)

NOT REACHABLE.  The launchers compile 22 instantiations no request selects (UNREACHABLE below,
each with the rule that excludes it); they are listed, not searched for.

Measured on an MI355X: profiles/wgrad_fp64_errors.txt."""
import collections
import importlib.util
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 7.0
BF = torch.bfloat16

TESTS = os.path.dirname(os.path.abspath(__file__))


def _load(name, *where):
    spec = importlib.util.spec_from_file_location(name, os.path.join(TESTS, *where, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


WR = _load("wgrad_refs", "tools")
M = _load("wgrad_plan_model", "tools")                  # the row's request: its chunk limit
DEFER = _load("test_wgrad_defer_gpu")                   # short_name, compute_launches
X3 = _load("test_bf16x3_step_kernels_gpu")              # the term check's criterion
R = WR.R
SLOPE = WR.SLOPE
short_name, compute_launches, term_failures = DEFER.short_name, DEFER.compute_launches, \
    X3.term_failures
TOL_DW, TOL_UP, TOL_C32 = 3e-5, 3e-5, 2e-5     # step_kernel_harness's two; the defer test's


def B(cpp):
    """The recorded (mangled) name of an instantiation with __bf16 template arguments, from its
    C++ spelling: the demangler gives up on those, so such launches are recorded as
    _ZN12_GLOBAL__N_1<len><kernel>I<arguments>EEvNS_11WgradParamsE."""
    kernel, args = re.fullmatch(r"(\w+)<(.*)>", cpp).groups()
    enc = "".join("DF16b" if a == "__bf16" else f"Lb{int(a == 'true')}E" if a in ("true", "false")
                  else f"Li{int(a)}E" for a in args.split(", "))
    return f"_ZN12_GLOBAL__N_1{len(kernel)}{kernel}I{enc}EEvNS_11WgradParamsE"


# the stem kernels take pointers: their mangled names spell the parameter list
STEM_B16 = "_ZN12_GLOBAL__N_122conv_stem_wgrad_kernelIDF16bEEvPKfPKT_Pfiiiiix"
STEM_ROWS_B16 = ("_ZN12_GLOBAL__N_127conv_stem_wgrad_rows_kernelIfDF16bEEvPKT_PKT0_Pfiiiiix"
                 "NS_9StemNormWE")
STEM_ROWS_U8_B16 = ("_ZN12_GLOBAL__N_127conv_stem_wgrad_rows_kernelIhDF16bEEvPKT_PKT0_Pfiiiiix"
                    "NS_9StemNormWE")

# entry: conv3x3 (ops.conv3x3_bwd_weight, plain operand), in (ops.conv_in_bwd_weight), 1x1
# (ops.conv1x1_bwd_weight), stem (the fp32 RGB image through conv_in_bwd_weight), u8 (a U8Image),
# up (ops.conv3x3_up_bwd_weight; H, W = the low-resolution size).
# mode: fp32, bf16 (bf16 matrix cores on fp32 tensors whose values are bf16 numbers), x3 (split
# bf16 on fp32 tensors), b16 (bf16 tensors).  act: activation on load (else Act(x) without
# coefficients, the plain form).  dw has off + Cx + extra input channels, the call writes
# [off, off + Cx).  chunk: images per launch, forced with the debug chunk limit (0: the whole
# batch).  c32: the c32 Winograd switch of the call.  kernel: the compute launches of the call,
# in order, as test_wgrad_defer_gpu.short_name spells them (one per chunk; db adds the
# bias_grad_kernel launches).
Row = collections.namedtuple(
    "Row", "entry mode act N H W Cx Cout stride ks off extra chunk c32 db seed edge kernel",
    defaults=(1, 3, 0, 0, 0, "always", False, 1, "", ()))

ROWS = {
    # ---- fp32-4wave
    "fp32-4wave:conv3x3-fp32-32to32-s1-1x4x8":
        Row("conv3x3", "fp32", False, 1, 4, 8, 32, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 32, 16, 1, false, float, float, 4>",)),
    "fp32-4wave:in-fp32-act-32to32-s1-1x4x8":
        Row("in", "fp32", True, 1, 4, 8, 32, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 32, 16, 1, true, float, float, 4>",)),
    "fp32-4wave:conv3x3-fp32-32to32-s2-1x4x8":
        Row("conv3x3", "fp32", False, 1, 4, 8, 32, 32, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 32, 16, 2, false, float, float, 4>",)),
    "fp32-4wave:in-fp32-act-32to32-s2-1x4x8":
        Row("in", "fp32", True, 1, 4, 8, 32, 32, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 32, 16, 2, true, float, float, 4>",)),
    "fp32-4wave:conv3x3-fp32-32to32-s1-1x4x24":
        Row("conv3x3", "fp32", False, 1, 4, 24, 32, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 32, 32, 1, false, float, float, 4>",)),
    "fp32-4wave:in-fp32-act-32to32-s1-1x4x24":
        Row("in", "fp32", True, 1, 4, 24, 32, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 32, 32, 1, true, float, float, 4>",)),
    "fp32-4wave:conv3x3-fp32-32to32-s2-1x4x40":
        Row("conv3x3", "fp32", False, 1, 4, 40, 32, 32, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 32, 32, 2, false, float, float, 4>",)),
    "fp32-4wave:in-fp32-act-32to32-s2-1x4x40":
        Row("in", "fp32", True, 1, 4, 40, 32, 32, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 32, 32, 2, true, float, float, 4>",)),
    "fp32-4wave:conv3x3-fp32-32to32-s1-1x4x64":
        Row("conv3x3", "fp32", False, 1, 4, 64, 32, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 32, 64, 1, false, float, float, 4>",)),
    "fp32-4wave:in-fp32-act-32to32-s1-1x4x64":
        Row("in", "fp32", True, 1, 4, 64, 32, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 32, 64, 1, true, float, float, 4>",)),
    "fp32-4wave:conv3x3-fp32-32to64-s1-1x4x8":
        Row("conv3x3", "fp32", False, 1, 4, 8, 32, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 64, 16, 1, false, float, float, 4>",)),
    "fp32-4wave:in-fp32-act-32to64-s1-1x4x8":
        Row("in", "fp32", True, 1, 4, 8, 32, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 64, 16, 1, true, float, float, 4>",)),
    "fp32-4wave:conv3x3-fp32-32to64-s2-1x4x8":
        Row("conv3x3", "fp32", False, 1, 4, 8, 32, 64, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 64, 16, 2, false, float, float, 4>",)),
    "fp32-4wave:in-fp32-act-32to64-s2-1x4x8":
        Row("in", "fp32", True, 1, 4, 8, 32, 64, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 64, 16, 2, true, float, float, 4>",)),
    "fp32-4wave:conv3x3-fp32-32to64-s1-1x4x24":
        Row("conv3x3", "fp32", False, 1, 4, 24, 32, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 64, 32, 1, false, float, float, 4>",)),
    "fp32-4wave:in-fp32-act-32to64-s1-1x4x24":
        Row("in", "fp32", True, 1, 4, 24, 32, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 64, 32, 1, true, float, float, 4>",)),
    "fp32-4wave:conv3x3-fp32-32to64-s2-1x4x40":
        Row("conv3x3", "fp32", False, 1, 4, 40, 32, 64, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 64, 32, 2, false, float, float, 4>",)),
    "fp32-4wave:in-fp32-act-32to64-s2-1x4x40":
        Row("in", "fp32", True, 1, 4, 40, 32, 64, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 64, 32, 2, true, float, float, 4>",)),
    "fp32-4wave:conv3x3-fp32-64to64-s1-1x4x8":
        Row("conv3x3", "fp32", False, 1, 4, 8, 64, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<64, 64, 16, 1, false, float, float, 4>",)),
    "fp32-4wave:in-fp32-act-64to64-s1-1x4x8":
        Row("in", "fp32", True, 1, 4, 8, 64, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<64, 64, 16, 1, true, float, float, 4>",)),
    "fp32-4wave:conv3x3-fp32-64to64-s2-1x4x8":
        Row("conv3x3", "fp32", False, 1, 4, 8, 64, 64, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<64, 64, 16, 2, false, float, float, 4>",)),
    "fp32-4wave:in-fp32-act-64to64-s2-1x4x8":
        Row("in", "fp32", True, 1, 4, 8, 64, 64, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<64, 64, 16, 2, true, float, float, 4>",)),
    "fp32-4wave:conv3x3-fp32-64to64-s1-1x4x24":
        Row("conv3x3", "fp32", False, 1, 4, 24, 64, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<64, 64, 32, 1, false, float, float, 4>",)),
    "fp32-4wave:in-fp32-act-64to64-s1-1x4x24":
        Row("in", "fp32", True, 1, 4, 24, 64, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<64, 64, 32, 1, true, float, float, 4>",)),
    "fp32-4wave:in-fp32-act-32to32-s1-1x4x40":
        Row("in", "fp32", True, 1, 4, 40, 32, 32,
            edge="a ragged last segment",
            kernel=("conv_wgrad_kernel<32, 32, 32, 1, true, float, float, 4>",)),
    "fp32-4wave:in-fp32-act-32to32-s1-1x5x8":
        Row("in", "fp32", True, 1, 5, 8, 32, 32,
            edge="a short last workgroup",
            kernel=("conv_wgrad_kernel<32, 32, 16, 1, true, float, float, 4>",)),
    "fp32-4wave:in-fp32-act-32to32-s1-3x4x8":
        Row("in", "fp32", True, 3, 4, 8, 32, 32,
            edge="N = 3",
            kernel=("conv_wgrad_kernel<32, 32, 16, 1, true, float, float, 4>",)),
    "fp32-4wave:in-fp32-act-32to32-s1-1x4x8-slice":
        Row("in", "fp32", True, 1, 4, 8, 32, 32, off=32, extra=64,
            edge="a column slice with off > 0 and extra > 0",
            kernel=("conv_wgrad_kernel<32, 32, 16, 1, true, float, float, 4>",)),
    "fp32-4wave:in-fp32-act-32to32-s1-3x4x8-chunk":
        Row("in", "fp32", True, 3, 4, 8, 32, 32, chunk=2,
            edge="a chunked batch, 2 + 1 images, activation on load",
            kernel=("conv_wgrad_kernel<32, 32, 16, 1, true, float, float, 4>",) * 2),
    "fp32-4wave:in-fp32-act-32to32-s2-1x25x41":
        Row("in", "fp32", True, 1, 25, 41, 32, 32, stride=2,
            edge="odd H and W at stride 2: Ho = 13, Wo = 21",
            kernel=("conv_wgrad_kernel<32, 32, 32, 2, true, float, float, 4>",)),
    "fp32-4wave:in-x3-act-32to32-s1-1x4x8":
        Row("in", "x3", True, 1, 4, 8, 32, 32,
            edge="eq32: the split entry lands on an fp32 kernel (S = 16)",
            kernel=("conv_wgrad_kernel<32, 32, 16, 1, true, float, float, 4>",)),
    "fp32-4wave:in-x3-act-32to64-s2-1x4x40":
        Row("in", "x3", True, 1, 4, 40, 32, 64, stride=2,
            edge="eq32: the split entry at stride 2",
            kernel=("conv_wgrad_kernel<32, 64, 32, 2, true, float, float, 4>",)),
    "fp32-4wave:conv3x3-bf16-32to64-s1-1x4x8":
        Row("conv3x3", "bf16", False, 1, 4, 8, 32, 64,
            edge="eq32: the bf16 entry lands on an fp32 kernel (S = 16)",
            kernel=("conv_wgrad_kernel<32, 64, 16, 1, false, float, float, 4>",)),
    "fp32-4wave:conv3x3-bf16-32to64-s2-1x4x40":
        Row("conv3x3", "bf16", False, 1, 4, 40, 32, 64, stride=2,
            edge="eq32: the bf16 entry at stride 2",
            kernel=("conv_wgrad_kernel<32, 64, 32, 2, false, float, float, 4>",)),
    "fp32-4wave:conv3x3-fp32-32to64-s1-2x12x24-db":
        Row("conv3x3", "fp32", False, 2, 12, 24, 32, 64, db=True,
            edge="db, M < 4096: one bias_grad launch",
            kernel=("conv_wgrad_kernel<32, 64, 32, 1, false, float, float, 4>",
                    "bias_grad_kernel")),
    "fp32-4wave:conv3x3-fp32-32to32-s1-2x128x128-db":
        Row("conv3x3", "fp32", False, 2, 128, 128, 32, 32, c32=False, db=True,
            edge="db, M >= 4096: two bias_grad launches; 128 slabs, the largest reduction here",
            kernel=("conv_wgrad_kernel<32, 32, 64, 1, false, float, float, 4>",
                    "bias_grad_kernel", "bias_grad_kernel")),
    "fp32-4wave:1x1-fp32-64to64-s1-2x4x8-k1-slice":
        Row("1x1", "fp32", False, 2, 4, 8, 64, 64, ks=1, off=64, extra=32,
            edge="conv1x1_bwd_weight: the centre tap",
            kernel=("conv_wgrad_kernel<64, 64, 16, 1, false, float, float, 4>",)),
    "fp32-4wave:in-fp32-act-64to64-s1-1x8x128-k1":
        Row("in", "fp32", True, 1, 8, 128, 64, 64, ks=1,
            edge="ksize = 1 keeps the direct kernel where 3x3 takes Winograd",
            kernel=("conv_wgrad_kernel<64, 64, 32, 1, true, float, float, 4>",)),
    "fp32-4wave:in-x3-act-32to32-s1-2x4x64-k1":
        Row("in", "x3", True, 2, 4, 64, 32, 32, ks=1,
            edge="ksize = 1 through the split entry: an fp32 kernel",
            kernel=("conv_wgrad_kernel<32, 32, 64, 1, true, float, float, 4>",)),
    # ---- fp32-8wave
    "fp32-8wave:conv3x3-fp32-128to32-s1-1x4x80":
        Row("conv3x3", "fp32", False, 1, 4, 80, 128, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 32, 128, 1, false, float, float, 8>",)),
    "fp32-8wave:in-fp32-act-128to32-s1-1x4x80":
        Row("in", "fp32", True, 1, 4, 80, 128, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 32, 128, 1, true, float, float, 8>",)),
    "fp32-8wave:conv3x3-fp32-128to32-s1-1x4x8":
        Row("conv3x3", "fp32", False, 1, 4, 8, 128, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 32, 16, 1, false, float, float, 8>",)),
    "fp32-8wave:in-fp32-act-128to32-s1-1x4x8":
        Row("in", "fp32", True, 1, 4, 8, 128, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 32, 16, 1, true, float, float, 8>",)),
    "fp32-8wave:conv3x3-fp32-128to32-s2-1x4x8":
        Row("conv3x3", "fp32", False, 1, 4, 8, 128, 32, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 32, 16, 2, false, float, float, 8>",)),
    "fp32-8wave:in-fp32-act-128to32-s2-1x4x8":
        Row("in", "fp32", True, 1, 4, 8, 128, 32, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 32, 16, 2, true, float, float, 8>",)),
    "fp32-8wave:conv3x3-fp32-128to32-s1-1x4x24":
        Row("conv3x3", "fp32", False, 1, 4, 24, 128, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 32, 32, 1, false, float, float, 8>",)),
    "fp32-8wave:in-fp32-act-128to32-s1-1x4x24":
        Row("in", "fp32", True, 1, 4, 24, 128, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 32, 32, 1, true, float, float, 8>",)),
    "fp32-8wave:conv3x3-fp32-128to32-s2-1x4x40":
        Row("conv3x3", "fp32", False, 1, 4, 40, 128, 32, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 32, 32, 2, false, float, float, 8>",)),
    "fp32-8wave:in-fp32-act-128to32-s2-1x4x40":
        Row("in", "fp32", True, 1, 4, 40, 128, 32, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 32, 32, 2, true, float, float, 8>",)),
    "fp32-8wave:conv3x3-fp32-128to32-s1-1x4x40":
        Row("conv3x3", "fp32", False, 1, 4, 40, 128, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 32, 64, 1, false, float, float, 8>",)),
    "fp32-8wave:in-fp32-act-128to32-s1-1x4x40":
        Row("in", "fp32", True, 1, 4, 40, 128, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 32, 64, 1, true, float, float, 8>",)),
    "fp32-8wave:conv3x3-fp32-32to256-s1-1x4x8":
        Row("conv3x3", "fp32", False, 1, 4, 8, 32, 256,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 64, 16, 1, false, float, float, 8>",)),
    "fp32-8wave:in-fp32-act-32to256-s1-1x4x8":
        Row("in", "fp32", True, 1, 4, 8, 32, 256,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 64, 16, 1, true, float, float, 8>",)),
    "fp32-8wave:conv3x3-fp32-32to256-s2-1x4x8":
        Row("conv3x3", "fp32", False, 1, 4, 8, 32, 256, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 64, 16, 2, false, float, float, 8>",)),
    "fp32-8wave:in-fp32-act-32to256-s2-1x4x8":
        Row("in", "fp32", True, 1, 4, 8, 32, 256, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 64, 16, 2, true, float, float, 8>",)),
    "fp32-8wave:conv3x3-fp32-32to256-s1-1x4x24":
        Row("conv3x3", "fp32", False, 1, 4, 24, 32, 256,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 64, 32, 1, false, float, float, 8>",)),
    "fp32-8wave:in-fp32-act-32to256-s1-1x4x24":
        Row("in", "fp32", True, 1, 4, 24, 32, 256,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 64, 32, 1, true, float, float, 8>",)),
    "fp32-8wave:conv3x3-fp32-32to256-s2-1x4x40":
        Row("conv3x3", "fp32", False, 1, 4, 40, 32, 256, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 64, 32, 2, false, float, float, 8>",)),
    "fp32-8wave:in-fp32-act-32to256-s2-1x4x40":
        Row("in", "fp32", True, 1, 4, 40, 32, 256, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 64, 32, 2, true, float, float, 8>",)),
    "fp32-8wave:conv3x3-fp32-32to256-s1-1x4x40":
        Row("conv3x3", "fp32", False, 1, 4, 40, 32, 256,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 64, 64, 1, false, float, float, 8>",)),
    "fp32-8wave:in-fp32-act-32to256-s1-1x4x40":
        Row("in", "fp32", True, 1, 4, 40, 32, 256,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 64, 64, 1, true, float, float, 8>",)),
    "fp32-8wave:conv3x3-fp32-32to256-s2-1x4x80":
        Row("conv3x3", "fp32", False, 1, 4, 80, 32, 256, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 64, 64, 2, false, float, float, 8>",)),
    "fp32-8wave:in-fp32-act-32to256-s2-1x4x80":
        Row("in", "fp32", True, 1, 4, 80, 32, 256, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<32, 64, 64, 2, true, float, float, 8>",)),
    "fp32-8wave:conv3x3-fp32-64to256-s1-1x4x8":
        Row("conv3x3", "fp32", False, 1, 4, 8, 64, 256,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<64, 64, 16, 1, false, float, float, 8>",)),
    "fp32-8wave:in-fp32-act-64to256-s1-1x4x8":
        Row("in", "fp32", True, 1, 4, 8, 64, 256,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<64, 64, 16, 1, true, float, float, 8>",)),
    "fp32-8wave:conv3x3-fp32-64to256-s2-1x4x8":
        Row("conv3x3", "fp32", False, 1, 4, 8, 64, 256, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<64, 64, 16, 2, false, float, float, 8>",)),
    "fp32-8wave:in-fp32-act-64to256-s2-1x4x8":
        Row("in", "fp32", True, 1, 4, 8, 64, 256, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<64, 64, 16, 2, true, float, float, 8>",)),
    "fp32-8wave:conv3x3-fp32-64to256-s1-1x4x24":
        Row("conv3x3", "fp32", False, 1, 4, 24, 64, 256,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<64, 64, 32, 1, false, float, float, 8>",)),
    "fp32-8wave:in-fp32-act-64to256-s1-1x4x24":
        Row("in", "fp32", True, 1, 4, 24, 64, 256,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<64, 64, 32, 1, true, float, float, 8>",)),
    "fp32-8wave:conv3x3-fp32-64to256-s2-1x4x40":
        Row("conv3x3", "fp32", False, 1, 4, 40, 64, 256, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<64, 64, 32, 2, false, float, float, 8>",)),
    "fp32-8wave:in-fp32-act-64to256-s2-1x4x40":
        Row("in", "fp32", True, 1, 4, 40, 64, 256, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<64, 64, 32, 2, true, float, float, 8>",)),
    "fp32-8wave:conv3x3-fp32-64to256-s1-1x4x40":
        Row("conv3x3", "fp32", False, 1, 4, 40, 64, 256,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<64, 64, 64, 1, false, float, float, 8>",)),
    "fp32-8wave:in-fp32-act-64to256-s1-1x4x40":
        Row("in", "fp32", True, 1, 4, 40, 64, 256,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_kernel<64, 64, 64, 1, true, float, float, 8>",)),
    "fp32-8wave:in-fp32-act-128to32-s1-1x4x136":
        Row("in", "fp32", True, 1, 4, 136, 128, 32,
            edge="a ragged last segment",
            kernel=("conv_wgrad_kernel<32, 32, 128, 1, true, float, float, 8>",)),
    "fp32-8wave:in-fp32-act-128to32-s1-1x5x8":
        Row("in", "fp32", True, 1, 5, 8, 128, 32,
            edge="a short last workgroup",
            kernel=("conv_wgrad_kernel<32, 32, 16, 1, true, float, float, 8>",)),
    "fp32-8wave:in-fp32-act-128to32-s1-3x4x8":
        Row("in", "fp32", True, 3, 4, 8, 128, 32,
            edge="N = 3",
            kernel=("conv_wgrad_kernel<32, 32, 16, 1, true, float, float, 8>",)),
    "fp32-8wave:in-fp32-act-128to32-s1-1x4x80-slice":
        Row("in", "fp32", True, 1, 4, 80, 128, 32, off=32, extra=64,
            edge="a column slice with off > 0 and extra > 0",
            kernel=("conv_wgrad_kernel<32, 32, 128, 1, true, float, float, 8>",)),
    "fp32-8wave:in-fp32-act-128to32-s1-3x4x8-chunk":
        Row("in", "fp32", True, 3, 4, 8, 128, 32, chunk=2,
            edge="a chunked batch, 2 + 1 images, activation on load",
            kernel=("conv_wgrad_kernel<32, 32, 16, 1, true, float, float, 8>",) * 2),
    "fp32-8wave:in-fp32-act-128to32-s2-1x25x41":
        Row("in", "fp32", True, 1, 25, 41, 128, 32, stride=2,
            edge="odd H and W at stride 2: Ho = 13, Wo = 21",
            kernel=("conv_wgrad_kernel<32, 32, 32, 2, true, float, float, 8>",)),
    "fp32-8wave:in-fp32-act-256to64-s1-2x4x8-k1-slice":
        Row("in", "fp32", True, 2, 4, 8, 256, 64, ks=1, off=64,
            edge="ksize = 1 through conv_in_bwd_weight (8 waves)",
            kernel=("conv_wgrad_kernel<64, 64, 16, 1, true, float, float, 8>",)),
    # ---- wino
    "wino:conv3x3-fp32-64to64-s1-1x8x128":
        Row("conv3x3", "fp32", False, 1, 8, 128, 64, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_wino_kernel<false>",)),
    "wino:in-fp32-act-64to64-s1-1x8x128":
        Row("in", "fp32", True, 1, 8, 128, 64, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_wino_kernel<true>",)),
    "wino:in-fp32-act-64to64-s1-1x8x144":
        Row("in", "fp32", True, 1, 8, 144, 64, 64,
            edge="a short last workgroup",
            kernel=("conv_wgrad_wino_kernel<true>",)),
    "wino:in-fp32-act-64to64-s1-3x4x96":
        Row("in", "fp32", True, 3, 4, 96, 64, 64,
            edge="N = 3",
            kernel=("conv_wgrad_wino_kernel<true>",)),
    "wino:in-fp32-act-64to64-s1-1x8x128-slice":
        Row("in", "fp32", True, 1, 8, 128, 64, 64, off=32, extra=64,
            edge="a column slice with off > 0 and extra > 0",
            kernel=("conv_wgrad_wino_kernel<true>",)),
    # ---- wino32
    "wino32:conv3x3-fp32-32to32-s1-1x8x32":
        Row("conv3x3", "fp32", False, 1, 8, 32, 32, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_wino32_kernel<false>",)),
    "wino32:in-fp32-act-32to32-s1-1x8x32":
        Row("in", "fp32", True, 1, 8, 32, 32, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_wino32_kernel<true>",)),
    "wino32:in-fp32-act-32to32-s1-3x8x32":
        Row("in", "fp32", True, 3, 8, 32, 32, 32,
            edge="N = 3",
            kernel=("conv_wgrad_wino32_kernel<true>",)),
    "wino32:in-fp32-act-32to32-s1-1x8x32-slice":
        Row("in", "fp32", True, 1, 8, 32, 32, 32, off=32, extra=64,
            edge="a column slice with off > 0 and extra > 0",
            kernel=("conv_wgrad_wino32_kernel<true>",)),
    # ---- bf16x3
    "bf16x3:conv3x3-x3-32to32-s1-1x4x64":
        Row("conv3x3", "x3", False, 1, 4, 64, 32, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_bf16_kernel<32, 32, 64, 3, true, float, float, false, 1>",)),
    "bf16x3:in-x3-act-32to32-s1-1x4x64":
        Row("in", "x3", True, 1, 4, 64, 32, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_bf16_kernel<32, 32, 64, 3, true, float, float, true, 1>",)),
    "bf16x3:conv3x3-x3-32to64-s1-1x4x24":
        Row("conv3x3", "x3", False, 1, 4, 24, 32, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_bf16_kernel<32, 64, 32, 3, false, float, float, false, 1>",)),
    "bf16x3:in-x3-act-32to64-s1-1x4x24":
        Row("in", "x3", True, 1, 4, 24, 32, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_bf16_kernel<32, 64, 32, 3, false, float, float, true, 1>",)),
    "bf16x3:conv3x3-x3-64to64-s1-1x4x8":
        Row("conv3x3", "x3", False, 1, 4, 8, 64, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_bf16_kernel<64, 64, 16, 3, false, float, float, false, 1>",)),
    "bf16x3:in-x3-act-64to64-s1-1x4x8":
        Row("in", "x3", True, 1, 4, 8, 64, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_bf16_kernel<64, 64, 16, 3, false, float, float, true, 1>",)),
    "bf16x3:in-x3-act-32to32-s1-1x4x80":
        Row("in", "x3", True, 1, 4, 80, 32, 32,
            edge="a ragged last segment",
            kernel=("conv_wgrad_bf16_kernel<32, 32, 64, 3, true, float, float, true, 1>",)),
    "bf16x3:in-x3-act-32to32-s1-1x5x64":
        Row("in", "x3", True, 1, 5, 64, 32, 32,
            edge="a short last workgroup",
            kernel=("conv_wgrad_bf16_kernel<32, 32, 64, 3, true, float, float, true, 1>",)),
    "bf16x3:in-x3-act-32to32-s1-3x4x64":
        Row("in", "x3", True, 3, 4, 64, 32, 32,
            edge="N = 3",
            kernel=("conv_wgrad_bf16_kernel<32, 32, 64, 3, true, float, float, true, 1>",)),
    "bf16x3:in-x3-act-32to32-s1-1x4x64-slice":
        Row("in", "x3", True, 1, 4, 64, 32, 32, off=32, extra=64,
            edge="a column slice with off > 0 and extra > 0",
            kernel=("conv_wgrad_bf16_kernel<32, 32, 64, 3, true, float, float, true, 1>",)),
    "bf16x3:in-x3-act-32to32-s1-3x4x64-chunk":
        Row("in", "x3", True, 3, 4, 64, 32, 32, chunk=2,
            edge="a chunked batch, 2 + 1 images, activation on load",
            kernel=("conv_wgrad_bf16_kernel<32, 32, 64, 3, true, float, float, true, 1>",) * 2),
    "bf16x3:conv3x3-x3-32to64-s1-2x12x24-db":
        Row("conv3x3", "x3", False, 2, 12, 24, 32, 64, db=True,
            edge="db behind a split kernel",
            kernel=("conv_wgrad_bf16_kernel<32, 64, 32, 3, false, float, float, false, 1>",
                    "bias_grad_kernel")),
    # ---- bf16-cores
    "bf16-cores:conv3x3-bf16-32to32-s1-1x4x64":
        Row("conv3x3", "bf16", False, 1, 4, 64, 32, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_bf16_kernel<32, 32, 64, 1, false, float, float, false, 1>",)),
    "bf16-cores:conv3x3-bf16-32to64-s1-1x4x24":
        Row("conv3x3", "bf16", False, 1, 4, 24, 32, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_bf16_kernel<32, 64, 32, 1, false, float, float, false, 1>",)),
    "bf16-cores:conv3x3-bf16-64to64-s1-1x4x8":
        Row("conv3x3", "bf16", False, 1, 4, 8, 64, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_bf16_kernel<64, 64, 16, 1, false, float, float, false, 1>",)),
    "bf16-cores:conv3x3-bf16-64to64-s1-1x4x24":
        Row("conv3x3", "bf16", False, 1, 4, 24, 64, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_bf16_kernel<64, 64, 32, 1, false, float, float, false, 1>",)),
    "bf16-cores:conv3x3-bf16-32to32-s1-1x4x80":
        Row("conv3x3", "bf16", False, 1, 4, 80, 32, 32,
            edge="a ragged last segment",
            kernel=("conv_wgrad_bf16_kernel<32, 32, 64, 1, false, float, float, false, 1>",)),
    "bf16-cores:conv3x3-bf16-32to32-s1-1x5x64":
        Row("conv3x3", "bf16", False, 1, 5, 64, 32, 32,
            edge="a short last workgroup",
            kernel=("conv_wgrad_bf16_kernel<32, 32, 64, 1, false, float, float, false, 1>",)),
    "bf16-cores:conv3x3-bf16-32to32-s1-3x4x64":
        Row("conv3x3", "bf16", False, 3, 4, 64, 32, 32,
            edge="N = 3",
            kernel=("conv_wgrad_bf16_kernel<32, 32, 64, 1, false, float, float, false, 1>",)),
    "bf16-cores:conv3x3-bf16-32to32-s1-1x4x64-slice":
        Row("conv3x3", "bf16", False, 1, 4, 64, 32, 32, off=32, extra=64,
            edge="a column slice with off > 0 and extra > 0",
            kernel=("conv_wgrad_bf16_kernel<32, 32, 64, 1, false, float, float, false, 1>",)),
    # ---- b16-ring
    "b16-ring:in-b16-32to32-s1-1x4x64":
        Row("in", "b16", False, 1, 4, 64, 32, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_b16_ring_kernel<32, 32, 64, false, 2, 1, 1>",)),
    "b16-ring:in-b16-act-32to32-s1-1x4x64":
        Row("in", "b16", True, 1, 4, 64, 32, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_b16_ring_kernel<32, 32, 64, true, 2, 1, 1>",)),
    "b16-ring:in-b16-32to64-s1-1x4x24":
        Row("in", "b16", False, 1, 4, 24, 32, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_b16_ring_kernel<32, 64, 32, false, 2, 1, 1>",)),
    "b16-ring:in-b16-32to64-s2-1x4x40":
        Row("in", "b16", False, 1, 4, 40, 32, 64, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_b16_ring_kernel<32, 64, 32, false, 2, 1, 2>",)),
    "b16-ring:in-b16-act-32to64-s1-1x4x24":
        Row("in", "b16", True, 1, 4, 24, 32, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_b16_ring_kernel<32, 64, 32, true, 2, 1, 1>",)),
    "b16-ring:in-b16-act-32to64-s2-1x4x40":
        Row("in", "b16", True, 1, 4, 40, 32, 64, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_b16_ring_kernel<32, 64, 32, true, 2, 1, 2>",)),
    "b16-ring:in-b16-64to64-s1-1x6x8":
        Row("in", "b16", False, 1, 6, 8, 64, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_b16_ring_kernel<64, 64, 16, false, 2, 1, 1>",)),
    "b16-ring:in-b16-64to64-s2-1x4x8":
        Row("in", "b16", False, 1, 4, 8, 64, 64, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_b16_ring_kernel<64, 64, 16, false, 2, 1, 2>",)),
    "b16-ring:in-b16-64to64-s1-1x4x8":
        Row("in", "b16", False, 1, 4, 8, 64, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_b16_ring_kernel<64, 64, 16, false, 2, 2, 1>",)),
    "b16-ring:in-b16-64to64-s2-1x8x8":
        Row("in", "b16", False, 1, 8, 8, 64, 64, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_b16_ring_kernel<64, 64, 16, false, 2, 2, 2>",)),
    "b16-ring:in-b16-act-64to64-s1-1x6x8":
        Row("in", "b16", True, 1, 6, 8, 64, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_b16_ring_kernel<64, 64, 16, true, 2, 1, 1>",)),
    "b16-ring:in-b16-act-64to64-s2-1x4x8":
        Row("in", "b16", True, 1, 4, 8, 64, 64, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_b16_ring_kernel<64, 64, 16, true, 2, 1, 2>",)),
    "b16-ring:in-b16-act-64to64-s1-1x4x8":
        Row("in", "b16", True, 1, 4, 8, 64, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_b16_ring_kernel<64, 64, 16, true, 2, 2, 1>",)),
    "b16-ring:in-b16-act-64to64-s2-1x8x8":
        Row("in", "b16", True, 1, 8, 8, 64, 64, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_b16_ring_kernel<64, 64, 16, true, 2, 2, 2>",)),
    "b16-ring:in-b16-64to64-s1-1x6x24":
        Row("in", "b16", False, 1, 6, 24, 64, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_b16_ring_kernel<64, 64, 32, false, 2, 1, 1>",)),
    "b16-ring:in-b16-64to64-s1-1x4x24":
        Row("in", "b16", False, 1, 4, 24, 64, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_b16_ring_kernel<64, 64, 32, false, 2, 2, 1>",)),
    "b16-ring:in-b16-act-64to64-s1-1x6x24":
        Row("in", "b16", True, 1, 6, 24, 64, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_b16_ring_kernel<64, 64, 32, true, 2, 1, 1>",)),
    "b16-ring:in-b16-act-64to64-s1-1x4x24":
        Row("in", "b16", True, 1, 4, 24, 64, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_b16_ring_kernel<64, 64, 32, true, 2, 2, 1>",)),
    "b16-ring:in-b16-act-32to32-s1-1x4x80":
        Row("in", "b16", True, 1, 4, 80, 32, 32,
            edge="a ragged last segment",
            kernel=("conv_wgrad_b16_ring_kernel<32, 32, 64, true, 2, 1, 1>",)),
    "b16-ring:in-b16-act-32to32-s1-3x4x64":
        Row("in", "b16", True, 3, 4, 64, 32, 32,
            edge="N = 3",
            kernel=("conv_wgrad_b16_ring_kernel<32, 32, 64, true, 2, 1, 1>",)),
    "b16-ring:in-b16-act-32to32-s1-1x4x64-slice":
        Row("in", "b16", True, 1, 4, 64, 32, 32, off=32, extra=64,
            edge="a column slice with off > 0 and extra > 0",
            kernel=("conv_wgrad_b16_ring_kernel<32, 32, 64, true, 2, 1, 1>",)),
    "b16-ring:in-b16-act-64to64-s1-1x6x40":
        Row("in", "b16", True, 1, 6, 40, 64, 64,
            edge="more than one column strip, the last one ragged",
            kernel=("conv_wgrad_b16_ring_kernel<64, 64, 32, true, 2, 1, 1>",)),
    "b16-ring:in-b16-act-64to64-s1-1x4x40":
        Row("in", "b16", True, 1, 4, 40, 64, 64,
            edge="more than one column strip, the last one ragged",
            kernel=("conv_wgrad_b16_ring_kernel<64, 64, 32, true, 2, 2, 1>",)),
    "b16-ring:in-b16-act-32to32-s1-3x4x64-chunk":
        Row("in", "b16", True, 3, 4, 64, 32, 32, chunk=2,
            edge="a chunked batch, 2 + 1 images, activation on load",
            kernel=("conv_wgrad_b16_ring_kernel<32, 32, 64, true, 2, 1, 1>",) * 2),
    "b16-ring:in-b16-act-64to64-s2-1x8x41":
        Row("in", "b16", True, 1, 8, 41, 64, 64, stride=2,
            edge="odd W at stride 2, Wo = 21 (an odd Ho has no whole ring rounds)",
            kernel=("conv_wgrad_b16_ring_kernel<64, 64, 16, true, 2, 2, 2>",)),
    "b16-ring:in-b16-act-64to64-s1-2x4x8-k1":
        Row("in", "b16", True, 2, 4, 8, 64, 64, ks=1,
            edge="ksize = 1 on bf16 tensors",
            kernel=("conv_wgrad_b16_ring_kernel<64, 64, 16, true, 2, 2, 1>",)),
    # ---- b16-segments
    "b16-segments:in-b16-32to32-s1-1x25x64":
        Row("in", "b16", False, 1, 25, 64, 32, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=(B("conv_wgrad_bf16_kernel<32, 32, 64, 1, false, __bf16, __bf16, false, 1>"),)),
    "b16-segments:in-b16-act-32to32-s1-1x25x64":
        Row("in", "b16", True, 1, 25, 64, 32, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=(B("conv_wgrad_bf16_kernel<32, 32, 64, 1, false, __bf16, __bf16, true, 1>"),)),
    "b16-segments:in-b16-32to64-s1-1x25x24":
        Row("in", "b16", False, 1, 25, 24, 32, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=(B("conv_wgrad_bf16_kernel<32, 64, 32, 1, false, __bf16, __bf16, false, 1>"),)),
    "b16-segments:in-b16-32to64-s2-1x6x40":
        Row("in", "b16", False, 1, 6, 40, 32, 64, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=(B("conv_wgrad_bf16_kernel<32, 64, 32, 1, false, __bf16, __bf16, false, 2>"),)),
    "b16-segments:in-b16-act-32to64-s1-1x25x24":
        Row("in", "b16", True, 1, 25, 24, 32, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=(B("conv_wgrad_bf16_kernel<32, 64, 32, 1, false, __bf16, __bf16, true, 1>"),)),
    "b16-segments:in-b16-act-32to64-s2-1x6x40":
        Row("in", "b16", True, 1, 6, 40, 32, 64, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=(B("conv_wgrad_bf16_kernel<32, 64, 32, 1, false, __bf16, __bf16, true, 2>"),)),
    "b16-segments:in-b16-64to64-s1-1x25x8":
        Row("in", "b16", False, 1, 25, 8, 64, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=(B("conv_wgrad_bf16_kernel<64, 64, 16, 1, false, __bf16, __bf16, false, 1>"),)),
    "b16-segments:in-b16-64to64-s2-1x6x8":
        Row("in", "b16", False, 1, 6, 8, 64, 64, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=(B("conv_wgrad_bf16_kernel<64, 64, 16, 1, false, __bf16, __bf16, false, 2>"),)),
    "b16-segments:in-b16-act-64to64-s1-1x25x8":
        Row("in", "b16", True, 1, 25, 8, 64, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=(B("conv_wgrad_bf16_kernel<64, 64, 16, 1, false, __bf16, __bf16, true, 1>"),)),
    "b16-segments:in-b16-act-64to64-s2-1x6x8":
        Row("in", "b16", True, 1, 6, 8, 64, 64, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=(B("conv_wgrad_bf16_kernel<64, 64, 16, 1, false, __bf16, __bf16, true, 2>"),)),
    "b16-segments:in-b16-64to64-s1-1x25x24":
        Row("in", "b16", False, 1, 25, 24, 64, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=(B("conv_wgrad_bf16_kernel<64, 64, 32, 1, false, __bf16, __bf16, false, 1>"),)),
    "b16-segments:in-b16-act-64to64-s1-1x25x24":
        Row("in", "b16", True, 1, 25, 24, 64, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=(B("conv_wgrad_bf16_kernel<64, 64, 32, 1, false, __bf16, __bf16, true, 1>"),)),
    "b16-segments:in-b16-act-32to32-s1-1x5x80":
        Row("in", "b16", True, 1, 5, 80, 32, 32,
            edge="a ragged last segment",
            kernel=(B("conv_wgrad_bf16_kernel<32, 32, 64, 1, false, __bf16, __bf16, true, 1>"),)),
    "b16-segments:in-b16-act-32to32-s1-1x5x64":
        Row("in", "b16", True, 1, 5, 64, 32, 32,
            edge="a short last workgroup",
            kernel=(B("conv_wgrad_bf16_kernel<32, 32, 64, 1, false, __bf16, __bf16, true, 1>"),)),
    "b16-segments:in-b16-act-32to32-s1-3x5x64":
        Row("in", "b16", True, 3, 5, 64, 32, 32,
            edge="N = 3",
            kernel=(B("conv_wgrad_bf16_kernel<32, 32, 64, 1, false, __bf16, __bf16, true, 1>"),)),
    "b16-segments:in-b16-act-32to32-s1-1x25x64-slice":
        Row("in", "b16", True, 1, 25, 64, 32, 32, off=32, extra=64,
            edge="a column slice with off > 0 and extra > 0",
            kernel=(B("conv_wgrad_bf16_kernel<32, 32, 64, 1, false, __bf16, __bf16, true, 1>"),)),
    "b16-segments:in-b16-act-32to32-s1-3x5x64-chunk":
        Row("in", "b16", True, 3, 5, 64, 32, 32, chunk=2,
            edge="a chunked batch, 2 + 1 images, activation on load",
            kernel=(B("conv_wgrad_bf16_kernel<32, 32, 64, 1, false, "
                      "__bf16, __bf16, true, 1>"),) * 2),
    "b16-segments:in-b16-act-32to64-s2-1x25x41":
        Row("in", "b16", True, 1, 25, 41, 32, 64, stride=2,
            edge="odd H and W at stride 2: Ho = 13, Wo = 21",
            kernel=(B("conv_wgrad_bf16_kernel<32, 64, 32, 1, false, __bf16, __bf16, true, 2>"),)),
    # ---- b16-fp32cores
    "b16-fp32cores:in-b16-32to32-s1-1x4x8":
        Row("in", "b16", False, 1, 4, 8, 32, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=(B("conv_wgrad_kernel<32, 32, 16, 1, false, __bf16, __bf16, 4>"),)),
    "b16-fp32cores:in-b16-act-32to32-s1-1x4x8":
        Row("in", "b16", True, 1, 4, 8, 32, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=(B("conv_wgrad_kernel<32, 32, 16, 1, true, __bf16, __bf16, 4>"),)),
    "b16-fp32cores:in-b16-32to32-s2-1x4x8":
        Row("in", "b16", False, 1, 4, 8, 32, 32, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=(B("conv_wgrad_kernel<32, 32, 16, 2, false, __bf16, __bf16, 4>"),)),
    "b16-fp32cores:in-b16-act-32to32-s2-1x4x8":
        Row("in", "b16", True, 1, 4, 8, 32, 32, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=(B("conv_wgrad_kernel<32, 32, 16, 2, true, __bf16, __bf16, 4>"),)),
    "b16-fp32cores:in-b16-32to32-s1-1x4x24":
        Row("in", "b16", False, 1, 4, 24, 32, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=(B("conv_wgrad_kernel<32, 32, 32, 1, false, __bf16, __bf16, 4>"),)),
    "b16-fp32cores:in-b16-act-32to32-s1-1x4x24":
        Row("in", "b16", True, 1, 4, 24, 32, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=(B("conv_wgrad_kernel<32, 32, 32, 1, true, __bf16, __bf16, 4>"),)),
    "b16-fp32cores:in-b16-32to32-s2-1x4x40":
        Row("in", "b16", False, 1, 4, 40, 32, 32, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=(B("conv_wgrad_kernel<32, 32, 32, 2, false, __bf16, __bf16, 4>"),)),
    "b16-fp32cores:in-b16-act-32to32-s2-1x4x40":
        Row("in", "b16", True, 1, 4, 40, 32, 32, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=(B("conv_wgrad_kernel<32, 32, 32, 2, true, __bf16, __bf16, 4>"),)),
    "b16-fp32cores:in-b16-32to64-s1-1x4x8":
        Row("in", "b16", False, 1, 4, 8, 32, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=(B("conv_wgrad_kernel<32, 64, 16, 1, false, __bf16, __bf16, 4>"),)),
    "b16-fp32cores:in-b16-act-32to64-s1-1x4x8":
        Row("in", "b16", True, 1, 4, 8, 32, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=(B("conv_wgrad_kernel<32, 64, 16, 1, true, __bf16, __bf16, 4>"),)),
    "b16-fp32cores:in-b16-32to64-s2-1x4x8":
        Row("in", "b16", False, 1, 4, 8, 32, 64, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=(B("conv_wgrad_kernel<32, 64, 16, 2, false, __bf16, __bf16, 4>"),)),
    "b16-fp32cores:in-b16-act-32to64-s2-1x4x8":
        Row("in", "b16", True, 1, 4, 8, 32, 64, stride=2,
            edge="the smallest shape of the grid that selects it",
            kernel=(B("conv_wgrad_kernel<32, 64, 16, 2, true, __bf16, __bf16, 4>"),)),
    "b16-fp32cores:in-b16-act-32to32-s1-1x4x40":
        Row("in", "b16", True, 1, 4, 40, 32, 32,
            edge="a ragged last segment",
            kernel=(B("conv_wgrad_kernel<32, 32, 32, 1, true, __bf16, __bf16, 4>"),)),
    "b16-fp32cores:in-b16-act-32to32-s1-1x5x8":
        Row("in", "b16", True, 1, 5, 8, 32, 32,
            edge="a short last workgroup",
            kernel=(B("conv_wgrad_kernel<32, 32, 16, 1, true, __bf16, __bf16, 4>"),)),
    "b16-fp32cores:in-b16-act-32to32-s1-3x4x8":
        Row("in", "b16", True, 3, 4, 8, 32, 32,
            edge="N = 3",
            kernel=(B("conv_wgrad_kernel<32, 32, 16, 1, true, __bf16, __bf16, 4>"),)),
    "b16-fp32cores:in-b16-act-32to32-s1-1x4x8-slice":
        Row("in", "b16", True, 1, 4, 8, 32, 32, off=32, extra=64,
            edge="a column slice with off > 0 and extra > 0",
            kernel=(B("conv_wgrad_kernel<32, 32, 16, 1, true, __bf16, __bf16, 4>"),)),
    "b16-fp32cores:in-b16-act-32to32-s1-3x4x8-chunk":
        Row("in", "b16", True, 3, 4, 8, 32, 32, chunk=2,
            edge="a chunked batch, 2 + 1 images, activation on load",
            kernel=(B("conv_wgrad_kernel<32, 32, 16, 1, true, __bf16, __bf16, 4>"),) * 2),
    "b16-fp32cores:in-b16-act-32to32-s2-1x25x41":
        Row("in", "b16", True, 1, 25, 41, 32, 32, stride=2,
            edge="odd H and W at stride 2: Ho = 13, Wo = 21",
            kernel=(B("conv_wgrad_kernel<32, 32, 32, 2, true, __bf16, __bf16, 4>"),)),
    # ---- taps-4wave
    "taps-4wave:up-fp32-32to32-s1-1x4x8":
        Row("up", "fp32", False, 1, 4, 8, 32, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_taps_kernel<32, 32, 32, false, float, float, 4>",)),
    "taps-4wave:up-fp32-act-32to32-s1-1x4x8":
        Row("up", "fp32", True, 1, 4, 8, 32, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_taps_kernel<32, 32, 32, true, float, float, 4>",)),
    "taps-4wave:up-fp32-32to64-s1-1x4x8":
        Row("up", "fp32", False, 1, 4, 8, 32, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_taps_kernel<32, 64, 16, false, float, float, 4>",)),
    "taps-4wave:up-fp32-act-32to64-s1-1x4x8":
        Row("up", "fp32", True, 1, 4, 8, 32, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_taps_kernel<32, 64, 16, true, float, float, 4>",)),
    "taps-4wave:up-fp32-64to64-s1-1x4x8":
        Row("up", "fp32", False, 1, 4, 8, 64, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_taps_kernel<64, 64, 16, false, float, float, 4>",)),
    "taps-4wave:up-fp32-act-64to64-s1-1x4x8":
        Row("up", "fp32", True, 1, 4, 8, 64, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_taps_kernel<64, 64, 16, true, float, float, 4>",)),
    "taps-4wave:up-fp32-act-32to32-s1-1x5x8":
        Row("up", "fp32", True, 1, 5, 8, 32, 32,
            edge="a ragged last segment",
            kernel=("conv_wgrad_taps_kernel<32, 32, 32, true, float, float, 4>",)),
    "taps-4wave:up-fp32-act-32to32-s1-1x6x24":
        Row("up", "fp32", True, 1, 6, 24, 32, 32,
            edge="a short last workgroup",
            kernel=("conv_wgrad_taps_kernel<32, 32, 32, true, float, float, 4>",)),
    "taps-4wave:up-fp32-act-32to32-s1-3x4x8":
        Row("up", "fp32", True, 3, 4, 8, 32, 32,
            edge="N = 3",
            kernel=("conv_wgrad_taps_kernel<32, 32, 32, true, float, float, 4>",)),
    "taps-4wave:up-fp32-act-32to32-s1-1x4x8-slice":
        Row("up", "fp32", True, 1, 4, 8, 32, 32, off=32, extra=64,
            edge="a column slice with off > 0 and extra > 0",
            kernel=("conv_wgrad_taps_kernel<32, 32, 32, true, float, float, 4>",)),
    "taps-4wave:up-fp32-act-32to32-s1-3x4x8-chunk":
        Row("up", "fp32", True, 3, 4, 8, 32, 32, chunk=2,
            edge="a chunked batch, 2 + 1 images, activation on load",
            kernel=("conv_wgrad_taps_kernel<32, 32, 32, true, float, float, 4>",) * 2),
    # ---- taps-8wave
    "taps-8wave:up-fp32-128to32-s1-1x4x8":
        Row("up", "fp32", False, 1, 4, 8, 128, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_taps_kernel<32, 32, 64, false, float, float, 8>",)),
    "taps-8wave:up-fp32-act-128to32-s1-1x4x8":
        Row("up", "fp32", True, 1, 4, 8, 128, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_taps_kernel<32, 32, 64, true, float, float, 8>",)),
    "taps-8wave:up-fp32-32to256-s1-1x4x8":
        Row("up", "fp32", False, 1, 4, 8, 32, 256,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_taps_kernel<32, 64, 32, false, float, float, 8>",)),
    "taps-8wave:up-fp32-act-32to256-s1-1x4x8":
        Row("up", "fp32", True, 1, 4, 8, 32, 256,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_taps_kernel<32, 64, 32, true, float, float, 8>",)),
    "taps-8wave:up-fp32-64to256-s1-1x4x8":
        Row("up", "fp32", False, 1, 4, 8, 64, 256,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_taps_kernel<64, 64, 32, false, float, float, 8>",)),
    "taps-8wave:up-fp32-act-64to256-s1-1x4x8":
        Row("up", "fp32", True, 1, 4, 8, 64, 256,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_taps_kernel<64, 64, 32, true, float, float, 8>",)),
    "taps-8wave:up-fp32-act-128to32-s1-1x9x8":
        Row("up", "fp32", True, 1, 9, 8, 128, 32,
            edge="a ragged last segment",
            kernel=("conv_wgrad_taps_kernel<32, 32, 64, true, float, float, 8>",)),
    "taps-8wave:up-fp32-act-128to32-s1-1x6x48":
        Row("up", "fp32", True, 1, 6, 48, 128, 32,
            edge="a short last workgroup",
            kernel=("conv_wgrad_taps_kernel<32, 32, 64, true, float, float, 8>",)),
    "taps-8wave:up-fp32-act-128to32-s1-3x4x8":
        Row("up", "fp32", True, 3, 4, 8, 128, 32,
            edge="N = 3",
            kernel=("conv_wgrad_taps_kernel<32, 32, 64, true, float, float, 8>",)),
    "taps-8wave:up-fp32-act-128to32-s1-1x4x8-slice":
        Row("up", "fp32", True, 1, 4, 8, 128, 32, off=32, extra=64,
            edge="a column slice with off > 0 and extra > 0",
            kernel=("conv_wgrad_taps_kernel<32, 32, 64, true, float, float, 8>",)),
    "taps-8wave:up-fp32-act-128to32-s1-3x4x8-chunk":
        Row("up", "fp32", True, 3, 4, 8, 128, 32, chunk=2,
            edge="a chunked batch, 2 + 1 images, activation on load",
            kernel=("conv_wgrad_taps_kernel<32, 32, 64, true, float, float, 8>",) * 2),
    # ---- taps-b16
    "taps-b16:up-b16-32to32-s1-1x4x8":
        Row("up", "b16", False, 1, 4, 8, 32, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_taps_b16_kernel<32, 32, 64, false>",)),
    "taps-b16:up-b16-act-32to32-s1-1x4x8":
        Row("up", "b16", True, 1, 4, 8, 32, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_taps_b16_kernel<32, 32, 64, true>",)),
    "taps-b16:up-b16-64to64-s1-1x4x8":
        Row("up", "b16", False, 1, 4, 8, 64, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_taps_b16_kernel<64, 64, 16, false>",)),
    "taps-b16:up-b16-act-64to64-s1-1x4x8":
        Row("up", "b16", True, 1, 4, 8, 64, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_wgrad_taps_b16_kernel<64, 64, 16, true>",)),
    "taps-b16:up-b16-act-32to32-s1-1x9x8":
        Row("up", "b16", True, 1, 9, 8, 32, 32,
            edge="a ragged last segment",
            kernel=("conv_wgrad_taps_b16_kernel<32, 32, 64, true>",)),
    "taps-b16:up-b16-act-32to32-s1-1x6x48":
        Row("up", "b16", True, 1, 6, 48, 32, 32,
            edge="a short last workgroup",
            kernel=("conv_wgrad_taps_b16_kernel<32, 32, 64, true>",)),
    "taps-b16:up-b16-act-32to32-s1-3x4x8":
        Row("up", "b16", True, 3, 4, 8, 32, 32,
            edge="N = 3",
            kernel=("conv_wgrad_taps_b16_kernel<32, 32, 64, true>",)),
    "taps-b16:up-b16-act-32to32-s1-1x4x8-slice":
        Row("up", "b16", True, 1, 4, 8, 32, 32, off=32, extra=64,
            edge="a column slice with off > 0 and extra > 0",
            kernel=("conv_wgrad_taps_b16_kernel<32, 32, 64, true>",)),
    "taps-b16:up-b16-act-32to32-s1-3x4x8-chunk":
        Row("up", "b16", True, 3, 4, 8, 32, 32, chunk=2,
            edge="a chunked batch, 2 + 1 images, activation on load",
            kernel=("conv_wgrad_taps_b16_kernel<32, 32, 64, true>",) * 2),
    # ---- taps-b16-fp32cores
    "taps-b16-fp32cores:up-b16-32to64-s1-1x4x8":
        Row("up", "b16", False, 1, 4, 8, 32, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=(B("conv_wgrad_taps_kernel<32, 64, 16, false, __bf16, __bf16, 4>"),)),
    "taps-b16-fp32cores:up-b16-act-32to64-s1-1x4x8":
        Row("up", "b16", True, 1, 4, 8, 32, 64,
            edge="the smallest shape of the grid that selects it",
            kernel=(B("conv_wgrad_taps_kernel<32, 64, 16, true, __bf16, __bf16, 4>"),)),
    "taps-b16-fp32cores:up-b16-act-32to64-s1-1x5x8":
        Row("up", "b16", True, 1, 5, 8, 32, 64,
            edge="a ragged last segment",
            kernel=(B("conv_wgrad_taps_kernel<32, 64, 16, true, __bf16, __bf16, 4>"),)),
    "taps-b16-fp32cores:up-b16-act-32to64-s1-1x9x8":
        Row("up", "b16", True, 1, 9, 8, 32, 64,
            edge="a short last workgroup",
            kernel=(B("conv_wgrad_taps_kernel<32, 64, 16, true, __bf16, __bf16, 4>"),)),
    "taps-b16-fp32cores:up-b16-act-32to64-s1-3x4x8":
        Row("up", "b16", True, 3, 4, 8, 32, 64,
            edge="N = 3",
            kernel=(B("conv_wgrad_taps_kernel<32, 64, 16, true, __bf16, __bf16, 4>"),)),
    "taps-b16-fp32cores:up-b16-act-32to64-s1-1x4x8-slice":
        Row("up", "b16", True, 1, 4, 8, 32, 64, off=32, extra=64,
            edge="a column slice with off > 0 and extra > 0",
            kernel=(B("conv_wgrad_taps_kernel<32, 64, 16, true, __bf16, __bf16, 4>"),)),
    "taps-b16-fp32cores:up-b16-act-32to64-s1-3x4x8-chunk":
        Row("up", "b16", True, 3, 4, 8, 32, 64, chunk=2,
            edge="a chunked batch, 2 + 1 images, activation on load",
            kernel=(B("conv_wgrad_taps_kernel<32, 64, 16, true, __bf16, __bf16, 4>"),) * 2),
    # ---- stem
    "stem:stem-b16-3to32-s1-1x4x24":
        Row("stem", "b16", False, 1, 4, 24, 3, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=(STEM_B16,)),
    "stem:stem-b16-3to32-s1-1x4x128":
        Row("stem", "b16", False, 1, 4, 128, 3, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=(STEM_ROWS_B16,)),
    "stem:u8-b16-3to32-s1-1x4x128":
        Row("u8", "b16", False, 1, 4, 128, 3, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=(STEM_ROWS_U8_B16,)),
    "stem:stem-fp32-3to32-s1-1x4x24":
        Row("stem", "fp32", False, 1, 4, 24, 3, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_stem_wgrad_kernel<float>",)),
    "stem:stem-fp32-3to32-s1-1x4x128":
        Row("stem", "fp32", False, 1, 4, 128, 3, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_stem_wgrad_rows_kernel<float, float>",)),
    "stem:u8-fp32-3to32-s1-1x4x128":
        Row("u8", "fp32", False, 1, 4, 128, 3, 32,
            edge="the smallest shape of the grid that selects it",
            kernel=("conv_stem_wgrad_rows_kernel<unsigned char, float>",)),
    "stem:stem-b16-3to32-s1-1x6x24":
        Row("stem", "b16", False, 1, 6, 24, 3, 32,
            edge="a ragged last segment",
            kernel=(STEM_B16,)),
    "stem:stem-b16-3to32-s1-3x4x8":
        Row("stem", "b16", False, 3, 4, 8, 3, 32,
            edge="N = 3",
            kernel=(STEM_B16,)),
}

# Instantiations the launchers compile and no request reaches, with the line of the rule that
# excludes each (csrc/conv_wgrad.hip).  launch_wgrad<> instantiates every fp32-core tile for
# both storages (with_bools(p.b16, ..)) and launch_wgrad_b16_ring<> both ring forms of every tile.
UNREACHABLE = {
    # bf16 tensors ask for the bf16 matrix cores; launch_wgrad_plan falls through to the
    # fp32-core kernels only when `(pl.S / 16) % pl.npp != 0`.  These segments split into whole
    # k-groups (npp = 4, 2, 1 on the 32x32, 32x64, 64x64 tile), so `use_bf16` - at stride 2
    # `p.b16 && prec == 1 && stride == 2 && (pl.S / 16) % pl.npp == 0` - takes them first.
    "whole k-groups": tuple(
        B(f"conv_wgrad_kernel<{t}, {act}, __bf16, __bf16, 4>")
        for t in ("32, 32, 64, 1", "32, 64, 32, 1", "32, 64, 32, 2", "64, 64, 16, 1",
                  "64, 64, 16, 2", "64, 64, 32, 1") for act in ("false", "true")),
    # launch_wgrad_taps_plan tests `pl.ci_t == 64 && p.b16` and `pl.ci_t == 32 && pl.co_t == 32
    # && p.b16` (conv_wgrad_taps_b16_kernel) before the fp32-core forms of those tiles.
    "taps_b16 first": tuple(
        B(f"conv_wgrad_taps_kernel<{t}, {act}, __bf16, __bf16, 4>")
        for t in ("32, 32, 32", "64, 64, 16") for act in ("false", "true")),
    # rg = 2 needs PlanOpts::ring8, which wgrad_select sets only where `c.Cx % 64 == 0 &&
    # c.Cout % 64 == 0`: the 64x64 tile.
    "ring8 is for 64x64 tiles": tuple(
        f"conv_wgrad_b16_ring_kernel<{t}, {act}, 2, 2, {s}>"
        for t, s in (("32, 32, 64", 1), ("32, 64, 32", 1), ("32, 64, 32", 2))
        for act in ("false", "true")),
}


def family(name):
    """The kernel family of a recorded compute launch: the unit of the error record and of -k."""
    b16 = "DF16b" in name
    if "stem" in name:
        return "stem"
    if "wino32" in name:
        return "wino32"
    if "wino" in name:
        return "wino"
    if "ring" in name:
        return "b16-ring"
    if "taps_b16" in name:
        return "taps-b16"
    if "taps" in name:
        if b16:
            return "taps-b16-fp32cores"
        return "taps-8wave" if name.endswith("8>") else "taps-4wave"
    if "conv_wgrad_bf16_kernel" in name:
        if b16:
            return "b16-segments"
        return "bf16x3" if name.split(", ")[3] == "3" else "bf16-cores"
    if b16:
        return "b16-fp32cores"
    return "fp32-8wave" if name.endswith("8>") else "fp32-4wave"


def tol(row):
    if row.entry == "up":
        return TOL_UP
    return TOL_C32 if "wino32" in row.kernel[0] else TOL_DW


CORES = {"fp32": 0, "bf16": 1, "x3": 3, "b16": 1}


def request(row):
    """The request of tests/tools/wgrad_plan_model.py a row makes"""
    return M.Request(row.entry, "bf16" if row.mode == "b16" else "fp32", CORES[row.mode], row.act,
                     row.N, row.H, row.W, row.Cx, row.Cout, row.stride, row.ks == 1,
                     {"always": 2, True: 1, False: 0}[row.c32], row.chunk)


class Call:
    """One row's call on its seeded operands (tests/tools/wgrad_refs.py::Operands, moved to the
    device in the row's storage type)."""

    def __init__(self, ua, row):
        self.ua, self.row, self.ops = ua, row, WR.Operands(row)
        b16 = row.mode == "b16"
        x = self.ops.x.to(DEV)
        self.x = x.to(BF) if b16 and x.dtype == torch.float32 and row.Cx != 3 else x
        self.dy = self.ops.dy.to(DEV).to(BF) if b16 else self.ops.dy.to(DEV)
        self.coef = None if self.ops.coef is None else tuple(c.to(DEV) for c in self.ops.coef)

    def new_dw(self):
        s = self.row
        total = s.off + s.Cx + s.extra
        shape = (s.Cout, total) if s.entry == "1x1" else (s.Cout, total, s.ks, s.ks)
        return torch.full(shape, SENTINEL, device=DEV)

    def __call__(self, dw, db=None, fp32_entry=False):
        s, ops, lib = self.row, self.ua.ops, self.ua._lib.lib()
        mode = "fp32" if fp32_entry else s.mode
        if s.chunk:
            lib.unet_debug_set_chunk_limit(M.chunk_limit_bytes(request(s)))
        try:
            with ops.c32_winograd_scope(s.c32):
                if s.entry == "conv3x3":
                    ops.conv3x3_bwd_weight(self.x, self.dy, dw, s.off, s.stride, db=db,
                                           bf16="bf16x3" if mode == "x3" else mode)
                elif s.entry == "1x1":
                    ops.conv1x1_bwd_weight(self.x, self.dy, dw, s.off)
                elif s.entry == "up":
                    ops.conv3x3_up_bwd_weight(self.source(), SLOPE, self.dy, dw, s.off)
                else:   # in, stem, u8
                    ops.conv_in_bwd_weight(self.source(), SLOPE, self.dy, dw, s.off, s.ks, s.stride,
                                           x3=mode == "x3")
        finally:
            if s.chunk:
                lib.unet_debug_set_chunk_limit(0)      # (0: back to the default)
        return dw

    def source(self):
        ops = self.ua.ops
        if self.row.entry == "u8":
            return ops.U8Image(self.x)
        return ops.Act(self.x) if self.coef is None else ops.Act(self.x, *self.coef)

    def cols(self, dw):
        return dw[:, self.row.off:self.row.off + self.row.Cx]


@pytest.mark.parametrize("name", list(ROWS))
def test_wgrad_against_fp64(ua, name):
    row = ROWS[name]
    call = Call(ua, row)
    db = torch.full((row.Cout,), SENTINEL, device=DEV) if row.db else None
    with ua.ops.record_launches() as rec:
        dw = call(call.new_dw(), db=db)
    assert compute_launches(rec.names) == row.kernel, f"{name}: launched {rec.names}"
    s = row
    outside = torch.cat([dw[:, :s.off], dw[:, s.off + s.Cx:]], 1)
    assert bool((outside == SENTINEL).all()), \
        f"{name}: the weight gradient wrote outside its input-channel slice"
    got = call.cols(dw)
    a, dy = call.ops.a64(dev=DEV), call.ops.dy64(DEV)
    ref = WR.reference(row, a, dy)
    bound = tol(row)
    err = WR.rel(got, ref)
    # the check of the check: the same comparison against a reference without one dy pixel
    err_drop = WR.rel(got, WR.reference(row, a, call.ops.dy64(DEV, drop_pixel=True)))
    line = f"WGRAD | {family(row.kernel[0])} | {name} | {err:.3e} | {bound:.1e} | {err_drop:.3e}"
    bad = []
    if not err <= bound:
        bad.append(f"dw vs fp64: {err:.3e} > {bound:.1e}")
    if not err_drop > bound:
        bad.append(f"the reference without one dy pixel passes: {err_drop:.3e} <= {bound:.1e}")
    if row.db:
        e = WR.rel(db, WR.bias_reference(call.ops, DEV))
        line += f" | db {e:.3e}"
        if not e <= TOL_DW:
            bad.append(f"db vs fp64: {e:.3e} > {TOL_DW:.1e}")
    fam = family(row.kernel[0])
    if fam == "bf16x3":
        e_drop, e_six = R.term_check(lambda p, q: WR.reference(row, p, q), a, dy, ref)
        t = dict(e_kernel=R.rel_l2(got, ref), e_drop=e_drop, e_six=e_six)
        line += f" | e_kernel {t['e_kernel']:.2e} e_drop {e_drop:.2e} e_six {e_six:.1e}"
        bad += term_failures(t)
    elif row.mode in ("x3", "bf16") and fam.startswith("fp32"):
        # the entry lands on an fp32 kernel: bit-equal to the fp32 entry's result
        same = torch.equal(dw, call(call.new_dw(), fp32_entry=True))
        line += f" | bit-equal to the fp32 entry: {same}"
        if not same:
            bad.append("the result differs from the fp32 entry's")
    print(line)
    assert not bad, f"{name} ({row.edge}):\n" + "\n".join(bad)
