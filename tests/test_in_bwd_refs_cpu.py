"""The check of the check for tests/test_in_bwd_fp64_gpu.py, without a GPU: the reference, the
families and the metric of tests/tools/in_bwd_refs.py.
  * fairness: on every (gradient, plane) pair of B.CASES, at every shape of the stand-alone pass,
    on fp32 and on bf16-rounded tensors, a plain fp32 evaluation (running sums per tile of 64 and
    of 256 pixels, fp64 merge, fp32 c1, c2, dz) stays within ONE QUARTER of every bound the GPU
    file sets, and the share of tie elements stays under the 0.1 % cap; the same for the operands
    the epilogue cases see (the harness's `structured_bwd`);
  * the new reference (fp64 from the fp32 values given) and the one the suite already trusts
    (fp64 autograd through recomputed statistics, fp64_layer_refs.ref_in_bwd) agree to 1e-6 of
    the maximum on `noise`;
  * sensitivity: each altered reference (lrelu'(z) ignored, the mask of image 1 on image 0, the
    last image's first 8 rows of g zeroed) is rejected by the restatement's own comparison."""
import importlib.util
import os

import pytest
import torch


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(
        os.path.dirname(os.path.abspath(__file__)), "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


B = _load("in_bwd_refs")
HS = _load("step_kernel_harness")
S = B.S
N = 2


def _restated(c, tile, b16):
    return B.restate32(c["g"], c["y"], c["mean"], c["rstd"], c["gamma"], c["beta"], c["mask"],
                       B.SLOPE, tile, b16_store=b16)


def _reference(c):
    return B.reference(c["g"], c["y"], c["mean"], c["rstd"], c["gamma"], c["beta"], c["mask"], B.SLOPE)


@pytest.mark.parametrize("b16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", B.PASS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_inputs_are_fair_to_an_fp32_kernel(shape, b16):
    worst = None
    for gfam, yfam in B.CASES:
        c = B.make_case(gfam, yfam, N, *shape, b16=b16)
        ref = _reference(c)
        for tile in (64, 256):
            m = B.compare(_restated(c, tile, b16), ref, b16=b16)
            bad = B.failures(m, scale=0.25)
            assert not bad, f"{gfam} x {yfam} {shape} tile {tile}: " + "; ".join(bad)
            w = B.worst_of(m)
            if worst is None or w["err"] / w["tol"] > worst[1]["err"] / worst[1]["tol"]:
                worst = (f"{gfam} x {yfam} tile {tile}", w)
        print(f"{gfam:12s} x {yfam:8s} ties {B.tie_count(ref):4d}  {B.report(m)}")
    print(f"{shape} {'bf16' if b16 else 'fp32'}: worst {worst[1]['what']} {worst[1]['err']:.2e} of "
          f"{worst[1]['tol']:.0e} on {worst[0]} at {worst[1]['at']}")


@pytest.mark.parametrize("shape", [(32, 64, 32), (8, 16, 512)], ids=lambda s: "x".join(map(str, s)))
def test_structured_epilogue_operands_are_fair_to_an_fp32_kernel(shape):
    """The operands of the epilogue cases: the NextNorm of HS.structured_bwd and a g with the
    structure a data gradient of structured dy has (a level per plane, a corner, noise)."""
    H, W, C = shape
    nn = HS.structured_norm(N, H, W, C, 10, "cpu")
    g = HS.structured_bwd("grad", (N, H, W, C), 1, "cpu")
    ref = B.reference(g, nn["y"], nn["st"][0], nn["st"][1], nn["gamma"], nn["beta"], nn["mask"], B.SLOPE)
    for tile in (64, 256):
        m = B.compare(B.restate32(g, nn["y"], nn["st"][0], nn["st"][1], nn["gamma"], nn["beta"],
                                  nn["mask"], B.SLOPE, tile), ref)
        print(f"tile {tile}: ties {B.tie_count(ref)}  {B.report(m)}")
        assert not B.failures(m, scale=0.25), B.failures(m, scale=0.25)


def test_every_family_appears_twice_and_the_named_pairs_are_there():
    for fam in B.G_FAMILIES:
        assert sum(g == fam for g, _ in B.CASES) >= 2, fam
    for fam in S.FAMILIES:
        assert sum(y == fam for _, y in B.CASES) >= 2, fam
    for pair in (("level", "offset"), ("aligned", "offset"), ("corner", "corner"), ("aligned", "corner"),
                 ("signed_tiles", "ramp"), ("gauss", "noise"), ("zero", "halves")):
        assert pair in B.CASES, pair


def test_gradient_families_are_what_they_claim():
    H, W, C = 32, 128, 8
    c = B.make_case("level", "offset", N, H, W, C)
    m, s = c["g"].double().mean(dim=(1, 2)).abs(), c["g"].double().std(dim=(1, 2))
    assert (m / s).min() < 3 and (m / s).max() > 300
    c = B.make_case("signed_tiles", "ramp", N, H, W, C)
    t = c["g"].double().reshape(N, H // 8, 8, W // 32, 32, C).sum(dim=(2, 4))
    assert t.abs().min() > 500 and (c["g"].double().sum(dim=(1, 2)).abs() < 10).all()
    c = B.make_case("aligned", "offset", N, H, W, C)
    ref = _reference(c)
    assert (ref["S2"].abs() > 0.1 * ref["A2"])[ref["kept"]].all()      # S2 does not cancel
    c = B.make_case("corner", "corner", N, H, W, C)
    first = c["g"].double()[:, :8, :32].abs().sum(dim=(1, 2)) / c["g"].double().abs().sum(dim=(1, 2))
    assert first.max() > 0.9
    assert not B.make_case("zero", "halves", N, H, W, C)["g"].any()


@pytest.mark.parametrize("shape", [(12, 20, 32), (33, 7, 128)], ids=lambda s: "x".join(map(str, s)))
def test_the_two_references_agree_on_noise(shape):
    """fp64 autograd through statistics recomputed in fp64 against the formulas on the statistics
    rounded to fp32: on `noise` (|mean| / std < 1) the rounding of the statistics is worth ~1e-7."""
    c = B.make_case("gauss", "noise", N, *shape)
    ref = _reference(c)
    assert B.tie_count(ref) == 0
    dz, dg, db = HS.R.ref_in_bwd(c["g"], c["y"], c["gamma"], c["beta"], c["mask"])
    for what, a, b in (("dz", dz, ref["dz"]), ("dgamma", dg, ref["dgamma"]), ("dbeta", db, ref["dbeta"])):
        e = (a - b).abs().max().item() / a.abs().max().item()
        print(f"{what}: {e:.2e}")
        assert e <= 1e-6, (what, e)


@pytest.mark.parametrize("kind", B.ALTERED)
@pytest.mark.parametrize("gfam,yfam", [("level", "offset"), ("corner", "corner"), ("gauss", "noise"),
                                       ("aligned", "corner"), ("signed_tiles", "ramp")])
def test_altered_references_are_rejected(gfam, yfam, kind):
    c = B.make_case(gfam, yfam, N, 16, 64, 32)
    got = _restated(c, 64, False)
    assert not B.failures(B.compare(got, _reference(c)))
    m = B.compare(got, B.altered(kind, c))
    print(B.report(m))
    rejected = {x.split(":")[0] for x in B.failures(m)}
    assert rejected & {"S1", "S2", "dz", "dgamma", "dbeta", "nonzero"}, (gfam, yfam, kind, B.report(m))


def test_forward_comparison_sees_a_wrong_selection():
    c = B.make_case("gauss", "offset", N, 12, 20, 32)
    ref = _reference(c)
    a = ref["a"].float()
    assert not B.failures(B.compare_forward(a, ref))
    assert B.failures(B.compare_forward(a.abs(), ref))
