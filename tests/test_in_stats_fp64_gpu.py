"""The InstanceNorm statistics against fp64 on planes that are not noise (-m gpu).

Every layer reads the per-(image, channel) mean and rstd, folded into alpha = gamma rstd mask and
beta = (beta - mean gamma rstd) mask.  The older tests hold the code that produces them on
stationary Gaussian planes only, where every tile mean lies within sigma / sqrt(px) of every
other: a merge with a wrong count, a tile in the wrong slot of its image and a reformulation that
cancels all stay inside the bounds there.  Here the planes have structure (tests/tools/
in_stats_refs.py: offset, corner, ramp, halves, constant, and noise as the control), the
comparison is per element (rstd and alpha relative to their own value, mean on the scale max |y|
of its own plane, beta on the scale (|beta_c| + |mean gamma rstd|) mask, alpha = beta = 0 exactly
where the mask is 0), and the bounds are the project's own: 5e-5 on rstd, alpha, beta, 2e-5 on
mean, 1e-6 on the rstd of a constant plane against 1 / sqrt(eps).  tests/test_in_stats_refs_cpu.py
shows that a well-conditioned fp32 evaluation meets a quarter of each bound on every family and
shape used here.  Three layers, launches asserted (ops.record_launches):
  (a) test_merge: the merges alone.  (mean_t, M2_t) summaries of a plane's tiles, formed in fp64
      and rounded to fp32, are written into the convolution workspace and finalized with
      stats_px = px (ops._conv_stats_finalize); reference: the fp64 merge of the rounded
      summaries.  N = 2, C in {32, 64, 96}; 2 x 64, 48 x 256, 511 x 128 tiles x pixels take
      in_stats_finalize_eq_kernel, 512 x 128, 1024 x 256, 2048 x 128, 4096 x 64 the pair
      in_stats_finalize_grp / _comb_kernel; with and without gamma, beta and mask; every call is
      made twice and must repeat bit for bit.
  (b) test_stand_alone_pass: in_stats_kernel<float> through ops.instnorm_stats, and
      in_stats_kernel<__bf16> through unet_conv_in_stats_finalize_b16 with stats_px = 0 on
      bf16-rounded planes (reference from the rounded values), + in_stats_finalize_kernel.
  (c) test_epilogue_fp32 / _bf16x3: every forward row of the fp32 and bf16x3 step-kernel tables at
      the row's own shape and launch names, on structured operands (the harness's `structured`:
      corner / ramp / halves sources, a bias of up to +-30 per channel); reference: the fp64
      statistics of the y the call returned.  y stays held to the fp64 convolution.
Each case prints its worst figure with the family and (n, c) it came from.
test_check_sees_*: one case of each layer must be REJECTED against a reference with the first
tile replaced by its neighbour, and against one with an image's first 8 rows zeroed.

Measured on an MI355X: the worst error over all cases that reach the kernel, and the family it
came from (bounds: rstd, alpha, beta 5e-5; mean 2e-5; constant 1e-6):
  kernel                              rstd              beta              mean              constant
  in_stats_finalize_eq_kernel         2.4e-7 corner     3.0e-7 corner     1.2e-7 halves     5.4e-8
  in_stats_finalize_grp / _comb       1.0e-6 ramp       9.2e-7 ramp       7.6e-8 halves     5.4e-8
  in_stats_kernel<float> + finalize   5.9e-6 offset     5.8e-6 offset     2.1e-7 offset     5.4e-8
  in_stats_kernel<__bf16> + finalize  1.1e-5 offset     1.1e-5 offset     2.5e-7 offset     5.4e-8
  epilogues, fp32 table, eq rows      1.5e-6            1.1e-6            1.3e-7            (fwd 512->512 s2)
  epilogues, fp32 table, grp rows     2.0e-6            2.1e-6            9.0e-8            (up fwd 64+32->32, stem)
  epilogues, bf16x3 table, eq rows    1.5e-6            7.6e-6            1.3e-7            (up fwd 512+512->512)
  epilogues, bf16x3 table, grp rows   1.3e-6            2.1e-6            1.0e-7            (stem fwd 3->32)
(alpha follows rstd.)  grp / _comb: every `corner` plane takes the combine kernel's second merge
(at most 3e-7 there), the figures of the row come from the planes that keep the shifted sums.
in_stats_kernel: the worst is 33 x 7 pixels in blocks of 77, above the 64 pixels up to which a
block is formed again; 2 x 2 pixels now 2.7e-6.  The whole file: 76 cases in 3.9 s, the slowest
1.3 s (the first case, which loads the library), every other at most 0.03 s.

What the file found.  Before it, in_stats_finalize_grp / _comb trusted the sums shifted by the
mean of tile 0 (S1 = sum(mean_t - K), S2 = sum(M2_t + per (mean_t - K)^2), M2 = S2 - tiles per
(S1 / tiles)^2) on every plane, and in_stats_kernel its Chan merges.  The same cases on that code,
next to the fp32 emulation of the shifted sums that prompted the file (worst rstd error):
  tiles x px      emulated (A, sigma)        measured, `corner`
  512 x 128       -                          5.4e-5
  1024 x 256      1.4e-4 (3, 0.01)           2.7e-4
  2048 x 128      2.3e-4 (100, 0.01)         2.1e-4
  4096 x 64       8.5e-4 (3, 0.01)           2.4e-4
  every other family, every count: at most 9e-7; in_stats_finalize_eq_kernel on `corner`: 2.4e-7
  through the epilogues: fwd 32->32 8.2e-5, up fwd 64+32->32 (bf16x3 table) 8.4e-5
  in_stats_kernel<float> on `offset` at 2 x 2 pixels: 1.7e-4 (chunk means round at the size of
  the level, and four pixels do not average that away); 3.5e-5 at 5 x 3 pixels
Both kernels now test the conditioning of what they have formed and form it again where the test
fails (csrc/instnorm.hip); planes that pass it keep their results bit for bit.  The figures of
the table above are theirs.  A form of the two-level merge without the shift (per-group (mean,
M2) in two passes, 16-way Chan merge) was measured as well: 8e-7 at worst, but it moves every
statistic of the 512^2 and 256^2 layers by an ulp, after which
test_net_gpu.py::test_clip_unet_full_size_batch_split misses its 1e-4 by 3 % and the benchmark's
8-step loss differs from before in the fourth digit; profiles/in_stats_bench.json has the cost of
both paths of the guarded form.
"""
import ctypes
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def _load(name, *where):
    spec = importlib.util.spec_from_file_location(name, os.path.join(
        os.path.dirname(os.path.abspath(__file__)), *where, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


HS = _load("step_kernel_harness", "tools")
S, DEV, EPS = HS.S, HS.DEV, HS.EPS
T32 = _load("test_fp32_step_kernels_gpu")
TX3 = _load("test_bf16x3_step_kernels_gpu")
assert EPS == S.EPS and HS.TOL_STAT == S.TOL_STAT and HS.TOL_Y == S.TOL_Y

FAMILIES = list(S.FAMILIES)


def _affines(N, C):
    """without, and with, gamma / beta / mask"""
    return [(None, None, None), S.affine(N, C, 5, DEV)]


def _show(ident, per_family):
    """per_family: [(family, metrics)] -> prints the worst figure of the case and where it is"""
    fam, m = max(((f, S.worst_of(ms)) for f, ms in per_family), key=lambda p: p[1]["err"] / p[1]["tol"])
    print(f"{ident}: worst {m['what']} {m['err']:.2e} of {m['tol']:.0e} on `{fam}` at (n, c) = {m['at']}")
    for f, ms in per_family:
        print(f"    {f:9s} {S.report(ms)}")


def _assert_held(ident, per_family):
    _show(ident, per_family)
    bad = [f"{f}: {line}" for f, ms in per_family for line in S.failures(ms)]
    assert not bad, f"{ident}:\n" + "\n".join(bad)


# --------------------------------------------------------------------------- (a) the merges
def _finalize(ua, y, mean32, m232, px, gamma, beta, mask):
    """The finalizer of the convolutions' statistics epilogue on the summaries [N, tiles, C]
    -> (st [4, N, C], launched names)"""
    N, H, W, C = y.shape
    ws = ua.ops._ws(ua.lib().unet_conv_in_fwd_workspace_bytes(N, H, W, C, 1), y)
    part = torch.stack([mean32, m232], dim=-1).contiguous()          # float2 [N][tiles][C]
    raw = part.view(torch.uint8).reshape(-1)
    assert raw.numel() <= ws.numel()
    ws[:raw.numel()] = raw
    st = torch.full((4, N, C), float("nan"), device=DEV)
    with ua.ops.record_launches() as rec:
        ua.ops._conv_stats_finalize(False, y, st, ws, ctypes.c_int(px), gamma, beta, EPS, mask)
    return st, rec.names


def _merge_case(ua, merge, C, family, perturb=None):
    """-> [(metrics, names)] for both affine settings of one family.  perturb(y, mean_t, m2_t) ->
    the summaries the REFERENCE merges (the check of the check)."""
    tiles, px, H, W, th, tw = merge
    y = S.FAMILIES[family](2, H, W, C, 3, DEV)
    mean_t, m2_t = S.tile_summaries(y, th, tw)
    mean32, m232 = mean_t.float(), m2_t.float()
    ymax = S.plane_max(y)
    ref_in = (mean32, m232) if perturb is None else perturb(y, mean32, m232)
    out = []
    for gamma, beta, mask in _affines(2, C):
        st, names = _finalize(ua, y, mean32, m232, px, gamma, beta, mask)
        again, _ = _finalize(ua, y, mean32, m232, px, gamma, beta, mask)
        assert torch.equal(st, again), "the finalizer does not repeat bit for bit"
        ref = S.merge_exact(*ref_in, px, gamma, beta, mask)
        out.append((S.compare(st, ref, ymax, const=family == "constant"), names))
    return out


MERGES = [(m, [HS.FIN_EQ]) for m in S.MERGE_ONE_LEVEL] + \
    [(m, [HS.FIN_GRP, HS.FIN_COMB]) for m in S.MERGE_TWO_LEVEL]


@pytest.mark.parametrize("C", S.MERGE_CHANNELS)
@pytest.mark.parametrize("merge,expected", MERGES, ids=[f"{m[0][0]}x{m[0][1]}" for m in MERGES])
def test_merge(ua, merge, expected, C):
    per_family = []
    for family in FAMILIES:
        for k, (metrics, names) in enumerate(_merge_case(ua, merge, C, family)):
            assert names == expected, f"{merge[0]} tiles launched {names}"
            per_family.append((family + ("+affine" if k else ""), metrics))
    _assert_held(f"merge {merge[0]} x {merge[1]}, C = {C}", per_family)


def _tile_replaced(y, mean32, m232):
    return S.tile_replaced(mean32, m232, 0, 1)


def _rows_zeroed_summaries(th, tw):
    def perturb(y, mean32, m232):
        mean_t, m2_t = S.tile_summaries(S.rows_zeroed(y), th, tw)
        return mean_t.float(), m2_t.float()
    return perturb


@pytest.mark.parametrize("merge", [S.MERGE_ONE_LEVEL[1], S.MERGE_TWO_LEVEL[1]],
                         ids=lambda m: f"{m[0]}x{m[1]}")
def test_check_sees_a_wrong_merge(ua, merge):
    for perturb in (_tile_replaced, _rows_zeroed_summaries(*merge[4:])):
        for metrics, _ in _merge_case(ua, merge, 32, "corner", perturb):
            assert S.failures(metrics), f"the check cannot see {perturb}: {S.report(metrics)}"


# --------------------------------------------------------------------------- (b) stand-alone pass
def _is_stats_kernel(name, b16):
    """in_stats_kernel<float>; the demangler gives up on __bf16, that name stays mangled"""
    if b16:
        return "in_stats_kernel" in name and "DF16b" in name
    return HS.short(name) == "in_stats_kernel<float>"


def _pass_case(ua, shape, b16, family, perturb=None):
    N, H, W, C = shape
    y = S.FAMILIES[family](N, H, W, C, 3, DEV)
    gamma, beta, mask = S.affine(N, C, 5, DEV)
    if b16:
        y = y.to(torch.bfloat16).contiguous()
        ws = ua.ops._ws(ua.lib().unet_conv_in_fwd_workspace_bytes(N, H, W, C, 1), y)
        st = torch.full((4, N, C), float("nan"), device=DEV)
        with ua.ops.record_launches() as rec:
            ua.ops._conv_stats_finalize(True, y, st, ws, ctypes.c_int(0), gamma, beta, EPS, mask)
    else:
        mask = None     # (the stand-alone entry folds no mask)
        with ua.ops.record_launches() as rec:
            st = ua.ops.instnorm_stats(y, gamma, beta, EPS)
    names = rec.names
    assert len(names) == 2 and _is_stats_kernel(names[0], b16) and \
        HS.short(names[1]) == "in_stats_finalize_kernel", f"{shape} launched {names}"
    ref = S.plane_stats(y if perturb is None else perturb(y), gamma, beta, mask)
    return S.compare(st, ref, S.plane_max(y), const=family == "constant")


@pytest.mark.parametrize("b16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", S.PASS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stand_alone_pass(ua, shape, b16):
    _assert_held(f"in_stats_kernel<{'__bf16' if b16 else 'float'}> {shape}",
                 [(f, _pass_case(ua, shape, b16, f)) for f in FAMILIES])


@pytest.mark.parametrize("b16", [False, True], ids=["fp32", "bf16"])
def test_check_sees_a_wrong_plane(ua, b16):
    for perturb in (S.first_tile_replaced, S.rows_zeroed):
        metrics = _pass_case(ua, (2, 64, 64, 64), b16, "corner", perturb)
        assert S.failures(metrics), f"the check cannot see {perturb.__name__}: {S.report(metrics)}"


# --------------------------------------------------------------------------- (c) the epilogues
def _forward_rows(table):
    return [r for r in table.LAYERS if any(r[2] is f for f in (table.run_fwd, table.run_stem_fwd,
                                                                getattr(table, "run_up_fwd", None)))]


def _runner(row):
    return getattr(HS, row[2].__name__)


def _epilogue(ua, mode, row):
    ident, layers, _, kw, expected = row[:5]
    # (no term check and no second call through the fp32 entry: the tables' own cases make them)
    out = _runner(row)(ua, mode._replace(term=None), gen=HS.structured, **kw)
    assert out["names"] == list(expected), f"{ident} ({layers}) launched {out['names']}"
    y_held = [m for m in out["metrics"] if m["what"] == "y"]
    assert len(y_held) == 1 and not HS.R.failures(y_held), HS.R.failures(y_held)
    return out


@pytest.mark.parametrize("row", _forward_rows(T32), ids=lambda r: r[0])
def test_epilogue_fp32(ua, row):
    out = _epilogue(ua, T32.MODE, row)
    _assert_held(f"fp32 {row[0]}", [("structured", out["stats"])])


@pytest.mark.parametrize("row", _forward_rows(TX3), ids=lambda r: r[0])
def test_epilogue_bf16x3(ua, row):
    out = _epilogue(ua, TX3.MODE, row)
    _assert_held(f"bf16x3 {row[0]}", [("structured", out["stats"])])


@pytest.mark.parametrize("table,ident", [(T32, "fwd 64->64"), (T32, "fwd 32->32"), (TX3, "fwd 64->64")],
                         ids=["fp32 fwd 64->64", "fp32 fwd 32->32", "bf16x3 fwd 64->64"])
def test_check_sees_wrong_epilogue_statistics(ua, table, ident):
    out = _epilogue(ua, table.MODE, next(r for r in table.LAYERS if r[0] == ident))
    assert not S.failures(out["stats"]), S.failures(out["stats"])
    for bad in out["stats_bad"]:
        assert S.failures(bad), f"the check cannot see an altered plane: {S.report(bad)}"
