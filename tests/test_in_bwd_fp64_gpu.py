"""The InstanceNorm backward and its fused reductions against fp64, per plane (-m gpu).

The backward of every layer forms S1 = sum gz and S2 = sum gz xhat per (image, channel), gz =
g mask lrelu'(z), in the stand-alone reduction pass or in the BSTATS epilogue of the data gradient
that produced g, and dz = gamma rstd (gz - S1 / HW - xhat S2 / HW) from them.  The older tests see
S1 and S2 only through dz, dgamma and dbeta on the tensors' maximum, with zero-mean Gaussian g:
there the sums cancel to sqrt(HW) sigma, and a dropped mask factor, an ignored lrelu'(z) or a tile
of the neighbouring image stay inside the bounds.  Here (tests/tools/in_bwd_refs.py, B):
  * the reference is fp64 on exactly the fp32 (or bf16) values the kernel is given;
  * S1, S2 are held per plane on A1 = sum |gz|, A2 = sum |gz xhat| at 2e-5 (TOL_BS); dgamma, dbeta
    per channel on the same sums over the images; dz per element on |al| (|gz| + A1 / HW + |xhat|
    A2 / HW) at 5e-5 (TOL_IN); dbias on sum_n |al| A1; a plane whose mask is 0, and everything for
    g = 0, must be exactly 0;
  * the gradients have a level per plane, a corner, alignment with xhat, tiles that cancel (B.CASES
    crosses them with the plane families of in_stats_refs.py);
  * elements whose z = y al + be no fp32 expression decides (ties, at most 0.1 % of a case) are
    left out of dz, and what they could contribute is added to the permitted error of the sums
    and of the dz of their own plane.
tests/test_in_bwd_refs_cpu.py shows that a plain fp32 evaluation meets a quarter of each bound on
every case and shape used here.  Launches are asserted (ops.record_launches):
  (a) test_stand_alone_pass: ops.instnorm_lrelu_drop_bwd without partials on fp32 and on bf16
      tensors, B.CASES at each of B.PASS_SHAPES, N = 2 and N = 1 (at N = 1 dbeta and dgamma ARE S1
      and S2 of the plane: the reduction pass keeps its sums in its workspace); in_bwd_reduce,
      in_bwd_finalize1, in_bwd_apply; every call twice, bit-equal.  C = 96 raises before a launch.
  (b) test_forward_agrees: ops.instnorm_lrelu_drop_fwd with the folded alpha, beta2 of
      ops.instnorm_stats: outside the ties sign(a) is the reference's selection, a holds 5e-5 on
      |y al| + |mean al| + |beta|.
  (c) test_epilogue_fp32 / _bf16x3: every row of the two step-kernel tables whose runner ends in
      the InstanceNorm backward, at the row's shape and launch names, on structured operands
      (HS.structured_bwd); the reference on the g the call returned; held: the epilogue's
      summaries summed in fp64 (`partial`), the backward fed by them (`fed`), and the backward
      through the reduction pass (`reduce`).
  (d) test_check_sees_*: one case of (a) and of (c) must be REJECTED against the references with
      lrelu'(z) ignored, with image 1's mask on image 0, with the last image's first 8 rows zeroed.
  (e) test_chunked_data_gradient_leaves_no_summaries: a data gradient that runs in several chunks
      leaves nn.tiles == 0 and the unchunked bits, and the reduction pass then holds the layer.
Each case prints its worst figure with the family and position.

Measured on an MI355X: the worst error over all cases that reach the kernel, and the case it came
from (bounds: S1, S2, dgamma 2e-5; dz 5e-5); ties = tie elements summed over the cases (the cap is
0.1 % of each case; the largest share was 4.9e-4, in a case of the shape 16 x 32 x 4):
  kernel / route                        S1                       S2                         dz                       dgamma                     ties
  in_bwd_reduce / apply <float>         6.0e-7 corner x ramp     4.3e-7 signed_tiles x halves  6.7e-7 corner x ramp   4.3e-7 signed_tiles x halves  254
  in_bwd_reduce / apply <__bf16>        2.0e-6 level x constant  3.5e-7 signed_tiles x ramp  8.9e-7 level x constant  5.3e-7 signed_tiles x ramp  140
  head_bwd_kernel (both tables)         5.9e-8                   5.6e-8                     1.8e-7                   5.0e-8                     105
  conv_wino32q (dgrad 32<-32), fp32     4.3e-8                   6.5e-8                     2.0e-7                   6.5e-8                     106
  conv_wino BSTATS (dgrad 64..512)      1.2e-7 512<-512          1.3e-7 64<-64              2.1e-7 256<-256          1.7e-7 64<-64              329
  conv_igemm, up dgrad (5 rows)         1.6e-7 512<-512          2.0e-7 128<-64             2.3e-7 512<-512          1.9e-7 512<-512            343
  conv_igemm, dgrad 512<-512 16         1.9e-7                   1.7e-7                     2.3e-7                   1.5e-7                     0
  stride 2 (igemm x 4, dgrad_s2_patch)  1.3e-7 128<-256          2.2e-7 32<-64              2.2e-7 256<-512          1.3e-7 32<-64              731
  in bwd fed (32, 512 channels)         2.6e-7 512               2.0e-7 512                 3.2e-7 512               1.8e-7 512                 3
  conv_patch_split BSTATS (bf16x3)      1.1e-7 512<-512          2.1e-7 64<-64              2.7e-7 64<-64            2.2e-7 64<-64              581
  bf16x3 dgrad 32<-32                   5.9e-8                   1.1e-7                     1.7e-7                   1.1e-7                     100
  chunked -> reduction pass             -                        -                          2.6e-7                   2.5e-7                     105
  in_apply_fwd_kernel                   a 2.3e-7 (`noise`); 0 selections differ outside the ties on all 42 cases
(the rows of an epilogue give the worst of its three routes; profiles/in_bwd_fp64_errors.txt has
them apart.)  The whole file: 67 cases in 5.7 s, the slowest 2.1 s (the first case, which loads the
library), every other at most 0.08 s.

What the file found: nothing to fix.  Every reduction is within 2e-6 of its plane's own sum of
magnitudes and every dz within 1e-6 of its own scale, on planes 1000 standard deviations from 0,
on gradients with a level, a corner, alignment with xhat and tiles that cancel; the four codings
of z = y al + be select alike outside the ties.  That the check can fail was shown on three
libraries with one line reverted each (none committed): without the mask factor of
in_bwd_reduce_kernel 53 of the 67 cases fail, with sel = 1 in the conv_igemm epilogue 18 (every
row that kernel serves), without p.bs_tile0 at conv_igemm's store site the two `dgrad s2 512<-512
bstats acc` rows.
"""
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
B, S, DEV, SLOPE, EPS = HS.B, HS.S, HS.DEV, HS.SLOPE, HS.EPS
T32 = _load("test_fp32_step_kernels_gpu")
TX3 = _load("test_bf16x3_step_kernels_gpu")
assert SLOPE == B.SLOPE and HS.TOL_BS == B.TOL_BS and HS.TOL_IN == B.TOL_IN and HS.TOL_STAT == B.TOL_STAT

_KEYS = ("g", "y", "mean", "rstd", "gamma", "beta", "mask")


def _show(ident, per_case):
    """per_case: [(label, metrics)] -> prints the worst figure of the case and where it is"""
    lab, m = max(((f, B.worst_of(ms)) for f, ms in per_case), key=lambda p: p[1]["err"] / p[1]["tol"])
    print(f"{ident}: worst {m['what']} {m['err']:.2e} of {m['tol']:.0e} on `{lab}` at {m['at']}")
    for f, ms in per_case:
        print(f"    {f:32s} {B.report(ms)}")


def _assert_held(ident, per_case):
    _show(ident, per_case)
    bad = [f"{f}: {line}" for f, ms in per_case for line in B.failures(ms)]
    assert not bad, f"{ident}:\n" + "\n".join(bad)


# --------------------------------------------------------------------------- (a) stand-alone pass
def _is(name, kernel, b16):
    """in_bwd_reduce_kernel<float> / in_bwd_apply_kernel<float>; the demangler gives up on __bf16,
    that name stays mangled"""
    if b16:
        return kernel in name and "DF16b" in name
    return HS.short(name) == kernel + "<float>"


def _pass_call(ua, c):
    C = c["y"].shape[3]
    dg, db, dbias = (torch.full((C,), float("nan"), device=DEV) for _ in range(3))
    with ua.ops.record_launches() as rec:
        dz = ua.ops.instnorm_lrelu_drop_bwd(c["g"].clone(), c["y"], c["mean"], c["rstd"], c["gamma"],
                                            c["beta"], c["mask"], SLOPE, dg, db, dbias)
    return dict(dz=dz, dgamma=dg, dbeta=db, dbias=dbias), rec.names


def _pass_case(ua, gfam, yfam, n, shape, b16, ref_of=None):
    c = B.make_case(gfam, yfam, n, *shape, device=DEV, b16=b16)
    got, names = _pass_call(ua, c)
    again, _ = _pass_call(ua, c)
    for k in got:
        assert torch.equal(got[k], again[k]), f"{k} does not repeat bit for bit"
    assert len(names) == 3 and _is(names[0], "in_bwd_reduce_kernel", b16) and names[1] == HS.IN_FIN1 \
        and _is(names[2], "in_bwd_apply_kernel", b16), f"{shape} launched {names}"
    if not b16:
        assert names == [HS.IN_REDUCE, HS.IN_FIN1, HS.IN_APPLY], names
    assert got["dz"].dtype == c["g"].dtype
    if n == 1:      # one image: dbeta, dgamma are the plane's S1, S2
        got["sums"] = torch.stack([got["dbeta"], got["dgamma"]], dim=-1)[None]
    ref = B.reference(*(c[k] for k in _KEYS), SLOPE) if ref_of is None else ref_of(c)
    return B.compare(got, ref, b16=b16), B.tie_count(ref)


@pytest.mark.parametrize("b16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", B.PASS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stand_alone_pass(ua, shape, b16):
    per_case, ties = [], 0
    for gfam, yfam in B.CASES:
        for n in (2, 1):
            m, t = _pass_case(ua, gfam, yfam, n, shape, b16)
            per_case.append((f"{gfam} x {yfam} N={n}", m))
            ties += t
    print(f"ties: {ties}")
    _assert_held(f"in_bwd_reduce / apply <{'__bf16' if b16 else 'float'}> {shape}", per_case)


def test_96_channels_are_refused_before_any_launch(ua):
    c = B.make_case("gauss", "noise", 2, 4, 4, 96, device=DEV)
    with ua.ops.record_launches() as rec:
        with pytest.raises(Exception):
            _pass_call(ua, c)
        torch.cuda.synchronize()
    assert rec.names == [], rec.names


@pytest.mark.parametrize("b16", [False, True], ids=["fp32", "bf16"])
def test_check_sees_a_wrong_stand_alone_pass(ua, b16):
    for gfam, yfam in (("level", "offset"), ("corner", "corner")):
        for kind in B.ALTERED:
            m, _ = _pass_case(ua, gfam, yfam, 2, (12, 20, 32), b16, ref_of=lambda c: B.altered(kind, c, SLOPE))
            assert B.failures(m), f"the check cannot see `{kind}` on {gfam} x {yfam}: {B.report(m)}"


# --------------------------------------------------------------------------- (b) the forward
@pytest.mark.parametrize("shape", B.PASS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_agrees(ua, shape):
    per_case = []
    for yfam in S.FAMILIES:
        y = S.FAMILIES[yfam](2, *shape, 3, DEV)
        gamma, beta, mask = B.affine(2, shape[2], 5, DEV)
        st = ua.ops.instnorm_stats(y, gamma, beta, EPS)
        with ua.ops.record_launches() as rec:
            a = ua.ops.instnorm_lrelu_drop_fwd(y, st[2].contiguous(), st[3].contiguous(), mask, SLOPE)
        assert [HS.short(n) for n in rec.names] == ["in_apply_fwd_kernel"], rec.names
        ref = B.reference(torch.zeros_like(y), y, st[0].contiguous(), st[1].contiguous(), gamma, beta,
                          mask, SLOPE)
        per_case.append((yfam, B.compare_forward(a, ref)))
    _show(f"in_apply_fwd_kernel {shape}", per_case)
    bad = [f"{f}: {line}" for f, ms in per_case for line in B.failures(ms)]
    assert not bad, "\n".join(bad)


# --------------------------------------------------------------------------- (c) the epilogues
def _bwd_rows(table):
    def ends_in_the_backward(r):
        runner, kw = r[2], r[3]
        return (runner is table.run_dgrad and kw.get("nxt")) or runner is table.run_up_dgrad or \
            runner is table.run_head_bwd or (runner is table.run_in_bwd and kw.get("fed"))
    return [r for r in table.LAYERS if ends_in_the_backward(r)]


def _epilogue(ua, mode, row):
    ident, layers, _, kw, expected = row[:5]
    # (no term check: the tables' own cases make it.  The hook stays set, so that a row whose
    # split entry lands on an fp32 kernel keeps comparing with the fp32 entry's plain call)
    if mode.term is not None:
        mode = mode._replace(term=lambda *a, **k: None)
    out = getattr(HS, row[2].__name__)(ua, mode, gen=HS.structured_bwd, **kw)
    assert out["names"] == list(expected), f"{ident} ({layers}) launched {out['names']}"
    # g (and the head's dw, db) stay held to the fp64 evaluation by the row's own metric
    own = [m for m in out["metrics"] if "via summaries" not in m["what"]]
    assert not HS.R.failures(own), HS.R.failures(own)
    print(f"ties: {out['ties']}")
    return out


def _routes(out):
    return [(route, m) for route, m in out["bwd"].items()]


@pytest.mark.parametrize("row", _bwd_rows(T32), ids=lambda r: r[0])
def test_epilogue_fp32(ua, row):
    _assert_held(f"fp32 {row[0]}", _routes(_epilogue(ua, T32.MODE, row)))


@pytest.mark.parametrize("row", _bwd_rows(TX3), ids=lambda r: r[0])
def test_epilogue_bf16x3(ua, row):
    _assert_held(f"bf16x3 {row[0]}", _routes(_epilogue(ua, TX3.MODE, row)))


@pytest.mark.parametrize("table,ident", [(T32, "dgrad 64<-64 bstats"), (T32, "dgrad s2 64<-128 bstats acc"),
                                         (TX3, "dgrad 64<-64 bstats"), (T32, "head bwd 32->3")],
                         ids=["fp32 dgrad 64<-64", "fp32 dgrad s2 64<-128", "bf16x3 dgrad 64<-64",
                              "head bwd"])
def test_check_sees_wrong_epilogue_reductions(ua, table, ident):
    out = _epilogue(ua, table.MODE, next(r for r in table.LAYERS if r[0] == ident))
    for route, m in _routes(out):
        assert not B.failures(m), (route, B.failures(m))
    for kind, m in out["bwd_bad"].items():
        assert B.failures(m), f"the check cannot see `{kind}`: {B.report(m)}"


# --------------------------------------------------------------------------- (e) chunking
@pytest.fixture
def small_chunks(ua):
    """Lower the buffer-range threshold so that a 4-image batch runs in several chunks."""
    def setter(per_image_bytes):
        ua.lib().unet_debug_set_chunk_limit(int(1.5 * per_image_bytes))
    yield setter
    ua.lib().unet_debug_set_chunk_limit(0)


def test_chunked_data_gradient_leaves_no_summaries(ua, small_chunks):
    """Batch::whole(bs) is null for a call that runs in chunks: no epilogue, nn.tiles == 0, and the
    caller (unet.py: partials = ... if nn.tiles > 0 else None) takes the reduction pass."""
    N, H, W, C = 4, 16, 32, 64
    w = HS.R.he_weight(C, C, 2, 9 * C)
    table = HS.pack_one(ua, w, False)
    dy = HS.structured_bwd("grad", (N, H, W, C), 1)
    D = HS.structured_bwd("grad", (N, H // 2, W // 2, 9 * C), 5)

    def run():
        nn = HS.next_norm_of(ua, HS.structured_bwd, N, H, W, C, 10)
        dx = ua.ops.conv3x3_bwd_data(dy, table.wd[0], 0, C, H, W, 1, nxt=nn)
        nl = HS.next_norm_of(ua, HS.structured_bwd, N, H // 2, W // 2, C, 20)
        gl = ua.ops.conv3x3_up_bwd_data(D, table.wd[0], 0, C, nxt=nl)
        return (dx, nn), (gl, nl)

    whole = run()
    for g, nn in whole:
        assert nn.tiles > 0, "the unchunked call has no epilogue: the case shows nothing"
    small_chunks((H // 2) * (W // 2) * 9 * C * 4)     # D: one image per chunk; dy: two
    small = run()
    per_case = []
    for what, (g, nn), (g0, _) in zip(("conv3x3_bwd_data", "conv3x3_up_bwd_data"), small, whole):
        assert nn.tiles == 0, f"{what}: a chunked call left {nn.tiles} tiles of summaries"
        assert torch.equal(g, g0), f"{what}: chunking changed the gradient"
        partials = (nn.partial, nn.tiles) if nn.tiles > 0 else None
        assert partials is None
        with ua.ops.record_launches() as rec:
            got = HS.bwd_results(ua, g, nn, ("reduce",))["reduce"]
        assert rec.names == [HS.IN_REDUCE, HS.IN_FIN1, HS.IN_APPLY], rec.names
        ref = B.reference(g, nn.y, nn.st[0], nn.st[1], nn.gamma, nn.beta, nn.mask, SLOPE)
        per_case.append((what, B.compare(got, ref)))
    _assert_held("chunked, through the reduction pass", per_case)
