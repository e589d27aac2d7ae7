"""The check of the check for tests/test_in_stats_fp64_gpu.py, without a GPU: the references,
plane families and metric of tests/tools/in_stats_refs.py.
  * fairness: on every plane family, at every shape the GPU file uses, a well-conditioned fp32
    evaluation (chunked two-pass + Chan merge) stays within ONE QUARTER of every bound the GPU
    file sets, so a bound missed on the device is a finding about the kernel and not about the
    inputs;
  * sensitivity: the naive E[x^2] - E[x]^2 exceeds ten times the rstd bound on `offset`; the
    shifted-sum two-level merge (what in_stats_finalize_grp / _comb computed before the GPU file
    existed) exceeds the rstd bound on `corner` at 1024 tiles x 256 pixels and stays within it on
    `noise`; with the combine kernel's conditioning test it stays within a quarter of every
    bound on every family;
  * the exact merge of tile summaries equals the plane statistics, and each reference rejects its
    own perturbations (one tile's summary replaced by its neighbour's, one merge count halved,
    one image's first 8 rows zeroed).
The merge shapes run at C = 4 here (N = 2: 8 planes, which the families' (n, c) cycles cover): every
restatement treats an (image, channel) plane on its own, so the channel count of the GPU cases
(32, 64, 96, a matter of the kernels' blocks) changes nothing here but the time.  The stand-alone
pass's shapes run as they are.  Measured (the worst over families, shapes, fp32 and bf16 planes,
with and without affine, against the full bound): well-conditioned fp32 rstd 6.0e-6 of 5e-5
(`offset`, 33 x 7 pixels), beta 6.0e-6 of 5e-5, mean 2.3e-7 of 2e-5; naive on `offset` rstd 0.1 to
0.27; shifted sums at 1024 x 256 rstd 1.4e-4 on `corner`, 8.5e-8 on `noise`; with the conditioning
test at most 4.6e-7 (`ramp`, 4096 x 64), every `corner` plane and no other merged again."""
import importlib.util
import os

import pytest
import torch

_spec = importlib.util.spec_from_file_location("in_stats_refs", os.path.join(
    os.path.dirname(os.path.abspath(__file__)), "tools", "in_stats_refs.py"))
S = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(S)

CPU_C = 4
MERGES = S.MERGE_ONE_LEVEL + S.MERGE_TWO_LEVEL
PLANES = [(2, m[2], m[3], CPU_C) for m in MERGES if (m[2], m[3]) != (512, 512)] + \
    [(2, 512, 512, CPU_C)] + S.PASS_SHAPES
FAMILY_SHAPE = [(f, s) for f in S.FAMILIES for s in PLANES]
_ids = [f"{f}-{'x'.join(map(str, s))}" for f, s in FAMILY_SHAPE]


def _err(metrics, what):
    return next(m["err"] for m in metrics if m["what"] == what)


@pytest.mark.parametrize("family,shape", FAMILY_SHAPE, ids=_ids)
def test_inputs_are_fair_to_an_fp32_kernel(family, shape):
    N, H, W, C = shape
    y = S.FAMILIES[family](N, H, W, C, 3)
    const = family == "constant"
    # without and with gamma / beta / mask; then the bf16 reader's inputs: the same planes
    # rounded to bf16, reference from the rounded values
    for gamma, beta, mask in ((None, None, None), S.affine(N, C, 5)):
        for x in (y, y.to(torch.bfloat16)):
            m = S.compare(S.well_conditioned32(x, gamma, beta, mask),
                          S.plane_stats(x, gamma, beta, mask), S.plane_max(x), const=const)
            print(f"{family} {shape} {x.dtype} affine={gamma is not None}: {S.report(m)}")
            assert not S.failures(m, scale=0.25), S.failures(m, scale=0.25)


def test_offset_spreads_over_three_decades():
    y = S.offset(2, 64, 64, 32, 3)
    ref = S.plane_stats(y)
    ratio = ref["mean"].abs() * ref["rstd"]
    assert ratio.min() < 3 and ratio.max() > 300 and y.abs().max() < 60
    assert ((ratio > 10) & (ratio < 100)).any()


@pytest.mark.parametrize("shape", [(2, 64, 64, 64), (2, 33, 7, 128), (2, 512, 512, CPU_C)],
                         ids=lambda s: "x".join(map(str, s)))
def test_naive_form_is_rejected_on_offset(shape):
    y = S.offset(*shape, 3)
    m = S.compare(S.naive32(y), S.plane_stats(y), S.plane_max(y))
    print(S.report(m))
    assert _err(m, "rstd") > 10 * S.TOL_STAT


HS = importlib.util.module_from_spec(importlib.util.spec_from_file_location(
    "step_kernel_harness", os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools",
                                        "step_kernel_harness.py")))
HS.__spec__.loader.exec_module(HS)


@pytest.mark.parametrize("N,H,W,C0,Cout,stride", [(2, 32, 64, 32, 32, 1), (2, 32, 64, 64, 32, 2),
                                                  (2, 16, 32, 3, 32, 1)],
                         ids=["32->32", "64->32 s2", "stem 3->32"])
def test_structured_epilogue_outputs_are_fair_to_an_fp32_kernel(N, H, W, C0, Cout, stride):
    """The planes the epilogue cases of the GPU file see: y = conv3x3(structured sources, He
    weights) + a bias of up to +-30, from the fp64 reference convolution, rounded to fp32."""
    g = torch.Generator().manual_seed(4)
    x = HS.structured("source", (N, H, W, C0), 1, "cpu")
    w = torch.randn((Cout, C0, 3, 3), generator=g, dtype=torch.double) * (2.0 / (9 * C0)) ** 0.5
    b = HS.structured("bias", (Cout,), 4, "cpu")
    y = HS.R.ref_conv(HS.R.nchw64(x), w, b.double(), stride).permute(0, 2, 3, 1).float().contiguous()
    ref = S.plane_stats(y)
    ratio = (ref["mean"].abs() * ref["rstd"]).max().item()
    gamma, beta, mask = S.affine(N, Cout, 5)
    for aff in ((None, None, None), (gamma, beta, mask)):
        m = S.compare(S.well_conditioned32(y, *aff), S.plane_stats(y, *aff), S.plane_max(y))
        print(f"max |mean| / std {ratio:.0f}: {S.report(m)}")
        assert not S.failures(m, scale=0.25), S.failures(m, scale=0.25)


def _summaries(family, merge, C=CPU_C, seed=3):
    tiles, px, H, W, th, tw = merge
    y = S.FAMILIES[family](2, H, W, C, seed)
    mean_t, m2_t = S.tile_summaries(y, th, tw)
    assert mean_t.shape[1] == tiles and th * tw == px
    return y, mean_t, m2_t


def test_shifted_sums_are_rejected_on_corner_and_pass_on_noise():
    merge = S.MERGE_TWO_LEVEL[1]
    assert merge[:2] == (1024, 256)
    for family, rejected in (("corner", True), ("noise", False)):
        y, mean_t, m2_t = _summaries(family, merge)
        mean32, m232 = mean_t.float(), m2_t.float()
        m = S.compare(S.shifted32(mean32, m232, 256), S.merge_exact(mean32, m232, 256), S.plane_max(y))
        print(f"{family}: {S.report(m)}")
        assert (_err(m, "rstd") > S.TOL_STAT) == rejected, (family, S.report(m))


@pytest.mark.parametrize("merge", S.MERGE_TWO_LEVEL, ids=lambda m: f"{m[0]}x{m[1]}")
@pytest.mark.parametrize("family", list(S.FAMILIES))
def test_guarded_shifted_sums_hold_on_every_family(family, merge):
    """The two-level finalizer as it is now: the shifted sums stand only where S2 <= 16 M2, and
    within a quarter of every bound there; the other planes (corner: all of them; noise: none)
    are merged again around their own mean."""
    y, mean_t, m2_t = _summaries(family, merge)
    mean32, m232 = mean_t.float(), m2_t.float()
    taken = []
    m = S.compare(S.shifted32(mean32, m232, merge[1], guard=S.GUARD, taken=taken),
                  S.merge_exact(mean32, m232, merge[1]), S.plane_max(y), const=family == "constant")
    print(f"{family} {merge[:2]}: {int(taken[0].sum())} of {taken[0].numel()} planes merged again; "
          f"{S.report(m)}")
    assert not S.failures(m, scale=0.25), S.failures(m, scale=0.25)
    if family == "corner":
        assert bool(taken[0].all())
    if family in ("noise", "constant"):
        assert not bool(taken[0].any())


@pytest.mark.parametrize("merge", MERGES, ids=lambda m: f"{m[0]}x{m[1]}")
@pytest.mark.parametrize("family", list(S.FAMILIES))
def test_exact_merge_equals_plane_statistics(family, merge):
    y, mean_t, m2_t = _summaries(family, merge)
    gamma, beta, mask = S.affine(2, CPU_C, 5)
    ref = S.plane_stats(y, gamma, beta, mask)
    got = S.merge_exact(mean_t, m2_t, merge[1], gamma, beta, mask)
    for k in ("mean", "rstd", "alpha", "beta"):
        assert torch.allclose(got[k], ref[k], rtol=1e-11, atol=1e-11), k
    # the summaries rounded to fp32 (what the GPU file writes) still give the plane's statistics
    # within a quarter of the bounds
    got = S.merge_exact(mean_t.float(), m2_t.float(), merge[1], gamma, beta, mask)
    st = torch.stack([got[k] for k in ("mean", "rstd", "alpha", "beta")])
    m = S.compare(st, ref, S.plane_max(y), const=family == "constant")
    assert not S.failures(m, scale=0.25), S.failures(m, scale=0.25)


def _as_st(ref):
    return torch.stack([ref[k] for k in ("mean", "rstd", "alpha", "beta")]).float()


@pytest.mark.parametrize("merge", [S.MERGE_ONE_LEVEL[1], S.MERGE_TWO_LEVEL[1]],
                         ids=lambda m: f"{m[0]}x{m[1]}")
@pytest.mark.parametrize("family", ["corner", "ramp", "halves", "offset", "noise"])
def test_references_reject_their_own_perturbations(family, merge):
    tiles, px = merge[:2]
    y, mean_t, m2_t = _summaries(family, merge)
    ymax = S.plane_max(y)
    good = S.merge_exact(mean_t, m2_t, px)
    assert not S.failures(S.compare(_as_st(good), good, ymax))
    # tile 0's summary replaced by tile 1's; the last tile's by its neighbour's on the planes
    # whose first two tiles are alike (halves, noise: the merge cannot tell them apart there)
    dst, src = (0, 1) if family in ("corner", "ramp", "offset") else (tiles - 1, tiles // 2 - 1)
    swapped = S.merge_exact(*S.tile_replaced(mean_t, m2_t, dst, src), px)
    halved = S.merge_exact(mean_t, m2_t, S.count_halved(tiles, px, 0))
    zeroed = S.plane_stats(S.rows_zeroed(y))
    for what, bad in (("tile replaced", swapped), ("count halved", halved), ("rows zeroed", zeroed)):
        assert S.failures(S.compare(_as_st(good), bad, ymax)), (family, what)
