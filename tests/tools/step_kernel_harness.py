"""The harness of the per-layer "held against fp64, launch asserted" suites: everything that is
the same for every operand mode of the train step.  tests/test_fp32_step_kernels_gpu.py and
tests/test_bf16x3_step_kernels_gpu.py run their LAYERS tables through the runners below;
tests/test_bf16_bench_layers_gpu.py (bench shape, bf16 operands, bounds of its own) takes the
mode-independent kernel names and the step recorder.  Loaded by path like fp64_layer_refs.py
(`load` below), which it loads in turn as R.  Here:
  * the TOL_* bounds;
  * one runner per operation of the step.  run_x(ua, mode, **row arguments) makes the call as the
    network's walk makes it in that operand mode and returns a dict: names (the recorded kernel
    names), metrics (against a float64 evaluation of the same fp32 operands) and, where they
    apply, bad (metrics against an altered reference - the check of the check), term and eq32
    (the split mode's verdicts); the forward runners take an operand generator (`gen`) for
    tests/test_in_stats_fp64_gpu.py and then also return stats / stats_bad, the statistics
    against those of the returned y per element (tests/tools/in_stats_refs.py, loaded as S);
    the runners whose call ends in the InstanceNorm backward (run_dgrad with nxt, run_up_dgrad,
    run_head_bwd, run_in_bwd) take one for tests/test_in_bwd_fp64_gpu.py and then also return
    bwd / bwd_bad, the reductions and dz per plane and per element against the fp64 formulas on
    the g the call returned (tests/tools/in_bwd_refs.py, loaded as B);
  * Mode, the record a table hands to the runners: how one layer's weights are packed and which
    forms and keywords carry the mode into each entry point;
  * the kernel names and name builders more than one table uses;
  * ALLOWED, the non-convolution kernels of every step with the test that holds each, and the
    bodies of the closure tests (the test functions stay in the test files)."""
import collections
import importlib.util
import os

import torch

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load(name, *where):
    """The module tests/<where...>/<name>.py by path (no package import)."""
    spec = importlib.util.spec_from_file_location(name, os.path.join(TESTS, *where, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = load("fp64_layer_refs", "tools")
S = load("in_stats_refs", "tools")
B = load("in_bwd_refs", "tools")
DEV, SLOPE, EPS = R.DEV, R.SLOPE, R.EPS
grand, coeffs, nchw64, act64, metric = R.grand, R.coeffs, R.nchw64, R.act64, R.metric

# The bounds of the existing small-shape tests of the same entry points (relative to the
# tensor's max magnitude unless a scale is given); where two tests are named, the second is the
# test of the split-bf16 operand mode, which holds the same value.
TOL_Y = 2e-5         # test_fused_gpu.py::test_conv_in_fwd, ::test_conv_in_fwd_split_bf16: y, and
#                      mean on the scale max |y| + 1
TOL_STAT = 5e-5      # ... rstd, alpha, and beta on its own scale (as test_conv_in_fwd has them)
TOL_DX = 2e-5        # test_kernels_gpu.py::test_conv3x3_bwd_data,
#                      test_fused_gpu.py::test_data_gradient_split_bf16_emits_reductions
TOL_DW = 3e-5        # test_fused_gpu.py::test_conv_in_bwd_weight (also [bf16x3]),
#                      test_kernels_gpu.py (dw)
TOL_UP = 3e-5        # test_fused_gpu.py::test_conv3x3_up_backward_at_low_resolution (dw and g)
TOL_TAPS = 1e-6      # test_kernels_gpu.py::test_upsample2x (the same stencil, 4-term sums)
TOL_BS = 2e-5        # test_fused_gpu.py::_in_bwd_both_ways (summaries vs reduction pass)
TOL_IN = 5e-5        # test_kernels_gpu.py::test_instnorm_lrelu_drop (dy, dgamma, dbeta)
TOL_HEAD = 2e-5      # test_kernels_gpu.py::test_head1x1: 1e-5 (logits, da) .. 2e-5 (dw, db)
TOL_HEAD_X = 1e-5

# --------------------------------------------------------------------------- the operand mode
# name:  the matmul_precision of the step ("fp32", "bf16x3");
# planes: the `planes` argument of the step's PackTable in this mode;
# pack(ua, w, stride) -> the PackTable of one 3x3 layer as _Walk builds it in this mode, run;
# forms(ua, op, table, grid=None, held=True) -> the keyword arguments that carry the mode into
#        op = "fwd" (conv_in_fwd), "up_fwd" (conv_up_in_fwd), "dgrad" (conv3x3_bwd_data), "wgrad"
#        (conv_in_bwd_weight, table = None) or "up_dgrad" (conv3x3_up_bwd_data).  grid: the six
#        arguments of conv_wino_supported / conv_up_wino_supported for the call; held: the walk
#        holds a Winograd form for this source (it holds none for the up-sampled half);
# term(fn, a, b, got, exact, extra=None): the split mode's hook.  Where it is set, a row with
#        x3=True (a split kernel runs) gets out["term"] = term(...), the figures of the term
#        check, and a row with x3=False (the entry lands on an fp32 kernel) is called a second
#        time as FP32_ENTRY has it and gets out["eq32"] = the two results are bit-equal.
Mode = collections.namedtuple("Mode", "name planes pack forms term", defaults=(None,))
# the same call through the fp32 entry (no Winograd form): what eq32 compares with
FP32_ENTRY = dict(fwd=dict(w3=None), dgrad=dict(bf16="fp32", wd3=None), wgrad=dict(x3=False))


def pack_one(ua, w, planes, wino=None):
    table = ua.ops.PackTable([w], planes, wino)
    table.run()
    return table


def summaries(ua, g, nn):
    """The BSTATS summaries drive the InstanceNorm backward like the stand-alone reduction pass
    over the same gradient does (test_fused_gpu.py::_in_bwd_both_ways)."""
    assert nn.tiles > 0, "no BSTATS epilogue ran"
    C = nn.y.shape[3]
    outs = []
    for partials in ((nn.partial, nn.tiles), None):
        dg, db, dbias = (torch.empty(C, device=DEV) for _ in range(3))
        dz = ua.ops.instnorm_lrelu_drop_bwd(g.clone(), nn.y, nn.st[0], nn.st[1], nn.gamma, nn.beta,
                                            nn.mask, SLOPE, dg, db, dbias, partials=partials)
        outs.append((dz, dg, db))
    return [metric(what + " via summaries", a, b, TOL_BS)
            for a, b, what in zip(outs[0], outs[1], ("dz", "dgamma", "dbeta"))]


def next_norm(ua, n, H, W, C, seed):
    return ua.ops.NextNorm(*R.norm_layer(n, H, W, C, seed), SLOPE)


def fused_stats(y_ref, st, gamma, beta, mask):
    """mean, rstd, alpha, beta of the fused forward against fp64 (test_conv_in_fwd's rules)"""
    mean = y_ref.mean(dim=(2, 3))
    rstd = 1.0 / torch.sqrt(y_ref.var(dim=(2, 3), unbiased=False) + EPS)
    gm, mk = gamma.double()[None], mask.double()
    scale = (beta.abs().max() + (mean * gm * rstd).abs().max()).item() / 0.7
    return [metric("mean", st[0], mean, TOL_Y, scale=y_ref.abs().max().item() + 1),
            metric("rstd", st[1], rstd, TOL_STAT),
            metric("alpha", st[2], gm * rstd * mk, TOL_STAT),
            metric("beta", st[3], (beta.double()[None] - mean * gm * rstd) * mk, TOL_STAT,
                   scale=scale)]


def operand(gen, kind, shape, seed, scale=1.0):
    """A forward runner's operand: grand(shape, seed, scale) for the rows of the tables; with an
    operand generator (tests/test_in_stats_fp64_gpu.py) gen(kind, shape, seed), kind = "source"
    (an NHWC layer tensor) or "bias"."""
    return grand(shape, seed, scale) if gen is None else gen(kind, shape, seed)


def structured(kind, shape, seed, dev=None):
    """The operand generator of the statistics tests: sources whose channels cycle over the plane
    families corner, ramp and halves (low noise, levels that differ per image and channel), and a
    bias with per-channel offsets up to +-30, which puts every plane of y far from 0.  (The
    runners' y metric is relative to max |y_ref|, ~30 here: y is held ~30 x looser in absolute
    terms than by the tables' own rows, which still hold it; these cases are about the
    statistics.)  dev: "cpu" for tests/test_in_stats_refs_cpu.py."""
    dev = DEV if dev is None else dev
    if kind == "bias":
        g = torch.Generator(device=dev).manual_seed(seed)
        return (torch.rand(shape, generator=g, device=dev) * 60.0 - 30.0).contiguous()
    c = torch.arange(shape[3], device=dev) % 3
    planes = [S.FAMILIES[f](*shape, seed, dev) for f in ("corner", "ramp", "halves")]
    return torch.where(c == 0, planes[0], torch.where(c == 1, planes[1], planes[2])).contiguous()


def returned_stats(y, st, gamma, beta, mask, perturb=None):
    """The statistics st against the fp64 statistics of THE y THE CALL RETURNED (so that the
    convolution's rounding does not enter), element by element (in_stats_refs.compare).
    perturb: the check of the check - the reference from perturb(y)."""
    ref = S.plane_stats(y if perturb is None else perturb(y), gamma, beta, mask)
    return S.compare(st, ref, S.plane_max(y))


def structured_norm(n, H, W, C, seed, dev=None):
    """The layer a BSTATS epilogue reduces for, on structured planes: y whose channels cycle over
    corner / ramp / halves / offset, its fp64 statistics rounded once (st [4, n, C] like
    R.norm_layer's), gamma, beta and a dropout mask with a 0 entry and a keep scale of 1 / 0.7
    (B.affine) -> dict(y, st, gamma, beta, mask)."""
    dev = DEV if dev is None else dev
    c = torch.arange(C, device=dev) % 4
    planes = [S.FAMILIES[f](n, H, W, C, seed, dev) for f in ("corner", "ramp", "halves", "offset")]
    y = torch.where(c == 0, planes[0], torch.where(c == 1, planes[1],
                                                   torch.where(c == 2, planes[2], planes[3]))).contiguous()
    gamma, beta, mask = B.affine(n, C, seed + 1, dev)
    ref = S.plane_stats(y)
    al = gamma.double()[None] * ref["rstd"]
    st = torch.stack([ref["mean"], ref["rstd"], al, beta.double()[None] - ref["mean"] * al])
    return dict(y=y, st=st.float().contiguous(), gamma=gamma, beta=beta, mask=mask)


def structured_bwd(kind, shape, seed, dev=None):
    """The operand generator of the InstanceNorm-backward tests: kind = "norm" -> structured_norm
    (shape = (n, H, W, C)); kind = "grad" -> an NHWC gradient whose channels cycle over the
    families level / corner / signed_tiles / gauss of in_bwd_refs.py, so that the data gradient
    formed from it has a level per plane, a corner and tiles that cancel.  dev: "cpu" for
    tests/test_in_bwd_refs_cpu.py."""
    dev = DEV if dev is None else dev
    if kind == "norm":
        return structured_norm(*shape, seed, dev)
    c = torch.arange(shape[3], device=dev) % 4
    planes = [B.G_FAMILIES[f](*shape, seed, dev) for f in ("level", "corner", "signed_tiles", "gauss")]
    return torch.where(c == 0, planes[0], torch.where(c == 1, planes[1],
                                                      torch.where(c == 2, planes[2], planes[3]))).contiguous()


def next_norm_of(ua, gen, n, H, W, C, seed):
    """The NextNorm of a backward runner: R.norm_layer's for the rows of the tables, gen("norm",
    ...)'s with an operand generator"""
    if gen is None:
        return next_norm(ua, n, H, W, C, seed)
    d = gen("norm", (n, H, W, C), seed)
    return ua.ops.NextNorm(d["y"], d["st"], d["gamma"], d["beta"], d["mask"], SLOPE)


def _in_bwd_call(ua, g, nn, partials):
    C = nn.y.shape[3]
    dg, db, dbias = (torch.empty(C, device=g.device) for _ in range(3))
    dz = ua.ops.instnorm_lrelu_drop_bwd(g.clone(), nn.y, nn.st[0], nn.st[1], nn.gamma, nn.beta,
                                        nn.mask, SLOPE, dg, db, dbias, partials=partials)
    return dict(dz=dz, dgamma=dg, dbeta=db, dbias=dbias)


def bwd_results(ua, g, nn, routes=("partial", "fed", "reduce")):
    """What the InstanceNorm backward of the layer nn makes of the gradient g, by route:
      partial  the per-tile summaries the producer's epilogue left, summed over the tiles in fp64;
      fed      instnorm_lrelu_drop_bwd(partials=...): dz, dgamma, dbeta, dbias, and the merged
               (S1, S2) of instnorm_bwd_merge_partials;
      reduce   the same from the stand-alone reduction pass (no S1, S2: the call keeps them in
               its workspace)."""
    N, H, W, C = nn.y.shape
    out = {}
    if "partial" in routes or "fed" in routes:
        assert nn.tiles > 0, "no BSTATS epilogue ran"
    if "partial" in routes:
        part = nn.partial.view(torch.float32)[:N * nn.tiles * C * 2].reshape(N, nn.tiles, C, 2)
        out["partial"] = dict(sums=part.double().sum(dim=1))
    if "fed" in routes:
        out["fed"] = _in_bwd_call(ua, g, nn, (nn.partial, nn.tiles))
        out["fed"]["sums"] = ua.ops.instnorm_bwd_merge_partials(nn.partial, nn.tiles, N, H * W, C)[1]
    if "reduce" in routes:
        out["reduce"] = _in_bwd_call(ua, g, nn, None)
    return out


def _with_bwd(out, gen, ua, g, nn, routes=("partial", "fed", "reduce"), results=None):
    """out["bwd"] = {route: metrics of in_bwd_refs.compare} against the fp64 formulas on THE g THE
    CALL RETURNED (so that the convolution's rounding does not enter) and nn's y and statistics;
    out["bwd_bad"] = {altered reference: the metrics of the first route against it}."""
    if gen is None:
        return out
    c = dict(g=g, y=nn.y, mean=nn.st[0], rstd=nn.st[1], gamma=nn.gamma, beta=nn.beta, mask=nn.mask)
    got = bwd_results(ua, g, nn, routes) if results is None else results
    ref = B.reference(g, nn.y, nn.st[0], nn.st[1], nn.gamma, nn.beta, nn.mask, SLOPE)
    out["bwd"] = {route: B.compare(r, ref) for route, r in got.items()}
    out["ties"] = B.tie_count(ref)
    del ref
    first = got["fed" if "fed" in got else next(iter(got))]
    out["bwd_bad"] = {kind: B.compare(first, B.altered(kind, c, SLOPE)) for kind in B.ALTERED}
    return out


# --------------------------------------------------------------------------- one runner per call
# N, H, W: the layer's input grid.  drop_row = (image, row): the check of the check - the
# reference is evaluated a second time with that row zeroed (input row for a forward, dy row for
# gradients) and the metrics against it come back as out["bad"].  x3 (read where mode.term is
# set): the split kernel runs; else an fp32 kernel behind the same entry.
# gen (forward runners): an operand generator (`operand` above) instead of the tables' Gaussian
# operands; the result then also carries out["stats"], the statistics against those of the
# returned y per element, and out["stats_bad"], the same against two altered references: the last
# image's first 8 x 32 tile of y replaced by the tile next to it, and its first 8 rows zeroed.
def _with_returned_stats(out, gen, y, st, gamma, beta, mask):
    if gen is not None:
        out["stats"] = returned_stats(y, st, gamma, beta, mask)
        out["stats_bad"] = [returned_stats(y, st, gamma, beta, mask, perturb=f)
                            for f in (S.first_tile_replaced, S.rows_zeroed)]
    return out


# gen (the runners that end in the InstanceNorm backward): an operand generator of kinds "norm"
# and "grad" (structured_bwd).  The NextNorm then comes from gen("norm", ...), dy / D / dlogits
# from gen("grad", ...), and the result also carries out["bwd"], out["bwd_bad"] and out["ties"]
# (_with_bwd above).  With gen=None nothing changes.


def run_fwd(ua, mode, N, H, W, C0, C1, Cout, stride, plain0=False, x3=True, drop_row=None,
            gen=None):
    """unet_conv_in_fwd[_wino | _bf16x3] as _Walk.run_layer_fused calls it: sources activated on
    load with per-image coefficients, the mode's weight form, dropout mask folded into alpha /
    beta.  plain0: the first source is a plain tensor (the materialised activated up-sampling of
    a decoder stage's first convolution in the split mode), the second the activated skip."""
    x0, c0 = operand(gen, "source", (N, H, W, C0), 1), (() if plain0 else coeffs(N, C0, 10))
    x1, c1 = (operand(gen, "source", (N, H, W, C1), 2), coeffs(N, C1, 20)) if C1 else (None, None)
    w = R.he_weight(Cout, C0 + C1, 3, 9 * (C0 + C1))
    b, gamma, beta = operand(gen, "bias", (Cout,), 4, 0.3), grand((Cout,), 5) * 0.2 + 1.0, grand((Cout,), 6) * 0.2
    mask = R.keep_mask(N, Cout, 7, 0.7)
    table = mode.pack(ua, w, stride)
    own = mode.forms(ua, "fwd", table, (N, H, W, C0, C1, Cout))
    same32 = mode.term is not None and not x3
    s0 = ua.ops.Act(x0, *c0)
    s1 = ua.ops.Act(x1, *c1) if C1 else None

    def call(kw):
        return ua.ops.conv_in_fwd(s0, s1, SLOPE, table.wf[0], b, 3, stride, gamma, beta, EPS, mask,
                                  **kw)

    with ua.ops.c32_winograd_scope(True):
        with ua.ops.record_launches() as rec:
            y, st = call(own)
        y32 = call(FP32_ENTRY["fwd"])[0] if same32 else None
    a = nchw64(x0) if plain0 else act64(x0, *c0)
    if C1:
        a = torch.cat([a, act64(x1, *c1)], 1)
    wd_, bd = w.double(), b.double()
    y_ref = R.ref_conv(a, wd_, bd, stride)
    out = dict(names=rec.names,
               metrics=[metric("y", nchw64(y), y_ref, TOL_Y)] + fused_stats(y_ref, st, gamma, beta, mask))
    if same32:
        out["eq32"] = torch.equal(y, y32)
    elif mode.term is not None:
        out["term"] = mode.term(lambda p, q: R.ref_conv(p, q, None, stride), a, wd_, nchw64(y), y_ref,
                                extra=bd[None, :, None, None])
    if drop_row is not None:
        a[drop_row[0], :, drop_row[1], :] = 0
        out["bad"] = [metric("y against the reference without one input row", nchw64(y),
                             R.ref_conv(a, wd_, bd, stride), TOL_Y)]
    return _with_returned_stats(out, gen, y, st, gamma, beta, mask)


def run_stem_fwd(ua, mode, N, H, W, gen=None):
    """unet_conv_in_fwd on the plain RGB image (3 -> 32): no mode has a weight form for it (no
    Winograd form, no planes in the PackTable), so the walk makes the fp32 mode's call."""
    x = operand(gen, "source", (N, H, W, 3), 1)
    w = R.he_weight(32, 3, 2, 27)
    b, gamma, beta = operand(gen, "bias", (32,), 3, 0.1), grand((32,), 5) * 0.2 + 1.0, grand((32,), 6) * 0.2
    mask = torch.ones(N, 32, device=DEV)
    table = mode.pack(ua, w, 1)
    own = mode.forms(ua, "fwd", table, (N, H, W, 3, 0, 32))
    assert all(v is None for v in own.values()), own
    with ua.ops.c32_winograd_scope(True), ua.ops.record_launches() as rec:
        y, st = ua.ops.conv_in_fwd(ua.ops.Act(x), None, SLOPE, table.wf[0], b, 3, 1, gamma, beta,
                                   EPS, None, **own)
    y_ref = R.ref_conv(nchw64(x), w.double(), b.double(), 1)
    out = dict(names=rec.names, metrics=[metric("y", nchw64(y), y_ref, TOL_Y)] +
               fused_stats(y_ref, st, gamma, beta, mask))
    return _with_returned_stats(out, gen, y, st, gamma, beta, mask)


def run_up_fwd(ua, mode, N, h, w, C0, C1, Cout, gen=None):
    """unet_conv_up_in_fwd / _wino as _Walk.run_up_layer calls it: bilinear 2x up-sampling of the
    activated low-resolution source [N, h, w, C0] in the loader, activated skip [N, 2h, 2w, C1]."""
    low, cl = operand(gen, "source", (N, h, w, C0), 1), coeffs(N, C0, 10)
    skip, cs = operand(gen, "source", (N, 2 * h, 2 * w, C1), 2), coeffs(N, C1, 20)
    wt = R.he_weight(Cout, C0 + C1, 3, 9 * (C0 + C1))
    b, gamma, beta = operand(gen, "bias", (Cout,), 4, 0.3), grand((Cout,), 5) * 0.2 + 1.0, grand((Cout,), 6) * 0.2
    mask = R.keep_mask(N, Cout, 7, 0.7)
    table = mode.pack(ua, wt, 1)
    s_low, s_skip = ua.ops.Act(low, *cl), ua.ops.Act(skip, *cs)
    with ua.ops.c32_winograd_scope(True):
        assert ua.ops.conv_up_in_fwd_supported(s_low, s_skip, Cout)    # what run_up_layer asks
        own = mode.forms(ua, "up_fwd", table, (N, 2 * h, 2 * w, C0, C1, Cout))
        with ua.ops.record_launches() as rec:
            y, st = ua.ops.conv_up_in_fwd(s_low, s_skip, SLOPE, table.wf[0], b, gamma, beta, EPS,
                                          mask, **own)
    a = torch.cat([R.upsample64(act64(low, *cl)), act64(skip, *cs)], 1)
    y_ref = R.ref_conv(a, wt.double(), b.double(), 1)
    out = dict(names=rec.names, metrics=[metric("y", nchw64(y), y_ref, TOL_Y)] +
               fused_stats(y_ref, st, gamma, beta, mask))
    return _with_returned_stats(out, gen, y, st, gamma, beta, mask)


def run_dgrad(ua, mode, N, H, W, Cin, Cout, stride, nxt=False, acc=False, ci_off=0, cin_total=None,
              x3=True, drop_row=None, gen=None):
    """unet_conv3x3_bwd_data[_bs][_wino | _bf16x3] as _Walk.layer_bwd calls it: dx[N, H, W, Cin]
    (+)= the data gradient of dy for input channels [ci_off, ci_off + Cin) of a layer with
    cin_total inputs; nxt = with the BSTATS epilogue; acc = accumulate into the gradient the
    decoder left in the skip.  The walk holds a Winograd form for a lone source and for the skip
    half of a decoder stage's first convolution (weight_forms: ud, ud1 - the same test on
    (Cout, Cin))."""
    cin_total = cin_total or Cin
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    dy = grand((N, Ho, Wo, Cout), 1) if gen is None else gen("grad", (N, Ho, Wo, Cout), 1)
    w = R.he_weight(Cout, cin_total, 2, 9 * Cout)
    base = grand((N, H, W, Cin), 3) if acc else None
    nn = next_norm_of(ua, gen, N, H, W, Cin, 10) if nxt else None
    table = mode.pack(ua, w, stride)
    own = mode.forms(ua, "dgrad", table, (N, H, W, Cout, 0, Cin), bool(cin_total == Cin or ci_off))
    same32 = mode.term is not None and not x3

    def call(nxt_, kw):
        return ua.ops.conv3x3_bwd_data(dy, table.wd[0], ci_off, Cin, H, W, stride,
                                       out=base.clone() if acc else None, accumulate=acc,
                                       nxt=nxt_, **kw)

    with ua.ops.c32_winograd_scope(True):
        with ua.ops.record_launches() as rec:
            dx = call(nn, own)
        # (without the epilogue: the same entry where the mode's own kernel runs; where the split
        # entry lands on an fp32 kernel - which at stride 2 it does only WITH the epilogue - the
        # fp32 entry)
        plain = call(None, FP32_ENTRY["dgrad"] if same32 else own) if nxt else None
        dx32 = call(next_norm(ua, N, H, W, Cin, 10) if nxt else None, FP32_ENTRY["dgrad"]) \
            if same32 else None
    wsl = w.double()[:, ci_off:ci_off + Cin]
    dyd = nchw64(dy)
    ref = R.ref_dgrad(dyd, wsl, stride, H, W)
    if acc:
        ref += nchw64(base)
    out = dict(names=rec.names, metrics=[metric("dx", nchw64(dx), ref, TOL_DX)])
    if nxt:
        assert torch.equal(plain, dx), "the BSTATS epilogue changed the gradient"
        out["metrics"] += summaries(ua, dx, nn)
    if same32:
        out["eq32"] = torch.equal(dx, dx32)
    elif mode.term is not None:
        out["term"] = mode.term(lambda p, q: R.ref_dgrad(p, q, stride, H, W), dyd, wsl, nchw64(dx),
                                ref, extra=nchw64(base) if acc else None)
    if drop_row is not None:
        dyd = dyd.clone()
        dyd[drop_row[0], :, drop_row[1], :] = 0
        bad = R.ref_dgrad(dyd, wsl, stride, H, W) + (nchw64(base) if acc else 0)
        out["bad"] = [metric("dx against the reference without one dy row", nchw64(dx), bad, TOL_DX)]
    return _with_bwd(out, gen if nxt else None, ua, dx, nn)


def run_wgrad(ua, mode, N, H, W, Cx, Cout, stride, ci_off=0, cin_total=None, x3=True, drop_row=None):
    """unet_conv_in_bwd_weight[_bf16x3]: dw[:, ci_off : ci_off + Cx] of a layer with cin_total
    inputs, operand x [N, H, W, Cx] activated on load; the other columns keep a sentinel.  x3 in
    the split mode: the split kernel runs (stride 1); else the entry's fp32 kernel."""
    cin_total = cin_total or Cx
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x, coef = grand((N, H, W, Cx), 1), coeffs(N, Cx, 30)
    dy = grand((N, Ho, Wo, Cout), 2)
    src = ua.ops.Act(x, *coef)

    def call(kw):
        dw = torch.full((Cout, cin_total, 3, 3), 7.0, device=DEV)
        with ua.ops.c32_winograd_scope(True), ua.ops.record_launches() as rec:
            ua.ops.conv_in_bwd_weight(src, SLOPE, dy, dw, ci_off, 3, stride, **kw)
        outside = torch.cat([dw[:, :ci_off], dw[:, ci_off + Cx:]], 1)
        assert bool((outside == 7.0).all()), "the weight gradient wrote outside its input-channel slice"
        return rec.names, dw[:, ci_off:ci_off + Cx]

    names, got = call(mode.forms(ua, "wgrad", None))
    a, dyd = act64(x, *coef), nchw64(dy)
    ref = R.ref_wgrad(a, dyd, stride)
    out = dict(names=names, metrics=[metric("dw", got, ref, TOL_DW)])
    if mode.term is not None and not x3:
        out["eq32"] = torch.equal(got, call(FP32_ENTRY["wgrad"])[1])
    elif mode.term is not None:
        out["term"] = mode.term(lambda p, q: R.ref_wgrad(p, q, stride), a, dyd, got, ref)
    if drop_row is not None:
        dyd = dyd.clone()
        dyd[drop_row[0], :, drop_row[1], :] = 0
        out["bad"] = [metric("dw against the reference without one dy row", got,
                             R.ref_wgrad(a, dyd, stride), TOL_DW)]
    return out


def run_stem_wgrad(ua, mode, N, H, W):
    """unet_conv_in_bwd_weight[_bf16x3] of the stem: the plain RGB image (no split form: K = 27,
    so the split mode's row is always compared with the fp32 entry)."""
    x = grand((N, H, W, 3), 1)
    dy = grand((N, H, W, 32), 2)

    def call(kw):
        dw = torch.zeros(32, 3, 3, 3, device=DEV)
        with ua.ops.c32_winograd_scope(True), ua.ops.record_launches() as rec:
            ua.ops.conv_in_bwd_weight(ua.ops.Act(x), SLOPE, dy, dw, 0, 3, 1, **kw)
        return rec.names, dw

    names, dw = call(mode.forms(ua, "wgrad", None))
    out = dict(names=names, metrics=[metric("dw", dw, R.ref_wgrad(nchw64(x), nchw64(dy), 1), TOL_DW)])
    if mode.term is not None:
        out["eq32"] = torch.equal(dw, call(FP32_ENTRY["wgrad"])[1])
    return out


def run_taps(ua, mode, N, h, w, C, drop_row=None):
    """unet_upsample2x_bwd_taps: D[N, h, w, 9 C] from dy[N, 2h, 2w, C]."""
    dy = grand((N, 2 * h, 2 * w, C), 1)
    with ua.ops.record_launches() as rec:
        D = ua.ops.upsample2x_bwd_taps(dy)
    dyd = nchw64(dy)
    out = dict(names=rec.names, metrics=[metric("D", D, R.ref_taps(dyd), TOL_TAPS)])
    if drop_row is not None:
        dyd = dyd.clone()
        dyd[drop_row[0], :, drop_row[1], :] = 0
        out["bad"] = [metric("D against the reference without one dy row", D, R.ref_taps(dyd),
                             TOL_TAPS)]
    return out


def run_up_wgrad(ua, mode, N, h, w, Cx, Cout, cin_total):
    """unet_conv3x3_up_bwd_weight: dw[:, 0:Cx] of conv3x3(upsample2x(act(low))) as a GEMM over the
    low-resolution pixels; the skip's columns keep a sentinel."""
    low, coef = grand((N, h, w, Cx), 1), coeffs(N, Cx, 40)
    D = grand((N, h, w, 9 * Cout), 2)
    dw = torch.full((Cout, cin_total, 3, 3), 7.0, device=DEV)
    with ua.ops.record_launches() as rec:
        ua.ops.conv3x3_up_bwd_weight(ua.ops.Act(low, *coef), SLOPE, D, dw, 0)
    assert bool((dw[:, Cx:] == 7.0).all()), "the weight gradient wrote outside its input-channel slice"
    ref = R.ref_up_wgrad(act64(low, *coef), D.double())
    return dict(names=rec.names, metrics=[metric("dw", dw[:, :Cx], ref, TOL_UP)])


def run_up_dgrad(ua, mode, N, h, w, C0, Cout, cin_total, gen=None):
    """unet_conv3x3_up_bwd_data_bs: the low-resolution data gradient of the up-sampled operand as a
    GEMM g = D B (fp32 D: no mode passes a weight form), with the BSTATS epilogue of the layer
    that produced the low-resolution tensor."""
    wt = R.he_weight(Cout, cin_total, 3, 9 * Cout)
    table = mode.pack(ua, wt, 1)
    D = grand((N, h, w, 9 * Cout), 5) if gen is None else gen("grad", (N, h, w, 9 * Cout), 5)
    nn = next_norm_of(ua, gen, N, h, w, C0, 20)
    with ua.ops.record_launches() as rec:
        g = ua.ops.conv3x3_up_bwd_data(D, table.wd[0], 0, C0, nxt=nn,
                                       **mode.forms(ua, "up_dgrad", table))
    ref = R.ref_up_dgrad(D.double(), wt.double()[:, :C0])
    plain = ua.ops.conv3x3_up_bwd_data(D, table.wd[0], 0, C0)
    assert torch.equal(plain, g), "the BSTATS epilogue changed the gradient"
    out = dict(names=rec.names, metrics=[metric("g", g, ref, TOL_UP)] + summaries(ua, g, nn))
    return _with_bwd(out, gen, ua, g, nn)


def run_head_fwd(ua, mode, N, H, W):
    """unet_head1x1_in_fwd: logits (NCHW) of the 1x1 head over the activated last decoder output."""
    y, coef = grand((N, H, W, 32), 1), coeffs(N, 32, 50)
    w, b = grand((3, 32), 2, 0.2), grand((3,), 3, 0.1)
    with ua.ops.record_launches() as rec:
        logits = ua.ops.head1x1_in_fwd(ua.ops.Act(y, *coef), SLOPE, w, b)
    ref = torch.einsum("nchw,kc->nkhw", act64(y, *coef), w.double()) + b.double()[None, :, None, None]
    return dict(names=rec.names, metrics=[metric("logits", logits, ref, TOL_HEAD_X)])


def run_head_bwd(ua, mode, N, H, W, gen=None):
    """unet_head1x1_in_bwd_bs: da = W^T dlogits, dW, db and the InstanceNorm-backward reductions
    of the last decoder layer (whose raw output the head reads)."""
    nn = next_norm_of(ua, gen, N, H, W, 32, 60)
    al, be = (nn.st[2] * nn.mask).contiguous(), (nn.st[3] * nn.mask).contiguous()
    x = ua.ops.Act(nn.y, al, be)
    dl = grand((N, 3, H, W), 2) if gen is None else \
        gen("grad", (N, H, W, 3), 2).permute(0, 3, 1, 2).contiguous()
    w = grand((3, 32), 3, 0.2)
    dw, db = torch.empty(3, 32, device=DEV), torch.empty(3, device=DEV)
    with ua.ops.record_launches() as rec:
        da = ua.ops.head1x1_in_bwd(x, SLOPE, dl, w, dw, db, nxt=nn)
    a, dld = act64(nn.y, al, be), dl.double()
    metrics = [metric("da", nchw64(da), torch.einsum("nkhw,kc->nchw", dld, w.double()), TOL_HEAD_X),
               metric("dw", dw, torch.einsum("nkhw,nchw->kc", dld, a), TOL_HEAD),
               metric("db", db, dld.sum(dim=(0, 2, 3)), TOL_HEAD)]
    return _with_bwd(dict(names=rec.names, metrics=metrics + summaries(ua, da, nn)), gen, ua, da, nn)


def run_in_bwd(ua, mode, N, H, W, C, fed, gen=None):
    """unet_instnorm_lrelu_drop_bwd[_partials]: InstanceNorm + LeakyReLU + dropout backward
    against fp64 autograd.  fed: the reductions come as BSTATS summaries of the producer of g (here
    the stand-alone up data gradient with Cout = 32), as in the step; else the stand-alone
    reduction pass runs.  With gen the call is held by out["bwd"] alone (route "fed", with the
    epilogue's own summaries as "partial", or "reduce"): the max-norm comparison with autograd
    through recomputed statistics is not one structured planes can be held by."""
    if gen is None:
        y, st, gamma, beta, mask = R.norm_layer(N, H, W, C, 70)
        nn = ua.ops.NextNorm(y, st, gamma, beta, mask, SLOPE)
    else:
        nn = next_norm_of(ua, gen, N, H, W, C, 70)
        y, st, gamma, beta, mask = nn.y, nn.st, nn.gamma, nn.beta, nn.mask
    partials = None
    if fed:
        wt = R.he_weight(32, C, 3, 9 * 32)
        D = grand((N, H, W, 9 * 32), 5) if gen is None else gen("grad", (N, H, W, 9 * 32), 5)
        g = ua.ops.conv3x3_up_bwd_data(D, mode.pack(ua, wt, 1).wd[0], 0, C, nxt=nn)
        assert nn.tiles > 0, "no BSTATS epilogue ran"
        partials = (nn.partial, nn.tiles)
    else:
        g = grand((N, H, W, C), 71) if gen is None else gen("grad", (N, H, W, C), 71)
    dg, db, dbias = (torch.empty(C, device=DEV) for _ in range(3))
    with ua.ops.record_launches() as rec:
        dz = ua.ops.instnorm_lrelu_drop_bwd(g.clone(), y, st[0], st[1], gamma, beta, mask, SLOPE,
                                            dg, db, dbias, partials=partials)
    if gen is not None:
        route = dict(dz=dz, dgamma=dg, dbeta=db, dbias=dbias)
        results = {"fed": route} if fed else {"reduce": route}
        if fed:
            results["partial"] = bwd_results(ua, g, nn, ("partial",))["partial"]
            route["sums"] = ua.ops.instnorm_bwd_merge_partials(nn.partial, nn.tiles, N, H * W, C)[1]
        return _with_bwd(dict(names=rec.names, metrics=[]), gen, ua, g, nn, results=results)
    dz_ref, dg_ref, db_ref = R.ref_in_bwd(g, y, gamma, beta, mask)
    return dict(names=rec.names,
                metrics=[metric("dz", dz, dz_ref, TOL_IN), metric("dgamma", dg, dg_ref, TOL_IN),
                         metric("dbeta", db, db_ref, TOL_IN),
                         # the conv-bias gradient = sum of dz: mathematically 0 (test_kernels_gpu.py's rule)
                         metric("dbias", dbias, torch.zeros(C, dtype=torch.double, device=DEV), 1e-3,
                                scale=max(1.0, dz_ref.abs().sum().item() / C))])


# --------------------------------------------------------------------------- kernel names
# As ops.record_launches reports them (demangled).
_NS, _AN = "unet_conv::(anonymous namespace)::", "(anonymous namespace)::"
_F2 = "HIP_vector_type<float, 2u>"


def short(name):
    """conv_wino_kernel<true, ..> of a reported name: without namespaces, `void` and arguments"""
    return name.replace(_NS, "").replace(_AN, "").replace("void ", "").split("(")[0]


def patch_s2(targs):
    return f"void {_NS}conv_patch_s2_kernel<{targs}>(unet_conv::IgemmParams)"


def dgrad_s2(targs):
    return f"void {_NS}conv_dgrad_s2_patch_kernel<{targs}>(unet_conv::IgemmParams)"


def igemm(bm, bn, wm, wn, act, kg):
    """conv_igemm_kernel<BM, BN, WM, WN, 32, ACT, KG>: KG = K groups of a workgroup"""
    return (f"void {_NS}conv_igemm_kernel<{bm}, {bn}, {wm}, {wn}, 32, {'true' if act else 'false'}, "
            f"{kg}>(unet_conv::IgemmParams)")


def wgrad(targs):
    """conv_wgrad_kernel<CI_T, CO_T, S, STRIDE, ACT, float, float, waves>"""
    return f"void {_AN}conv_wgrad_kernel<{targs}>({_AN}WgradParams)"


def wtaps(targs):
    return f"void {_AN}conv_wgrad_taps_kernel<{targs}>({_AN}WgradParams)"


REDUCE = f"{_AN}wgrad_reduce_batched_kernel({_AN}ReduceTable)"
FIN_GRP = f"{_AN}in_stats_finalize_grp_kernel({_F2} const*, {_F2}*, int, int, float)"
FIN_COMB = (f"{_AN}in_stats_finalize_comb_kernel({_F2} const*, {_F2} const*, float const*, "
            "float const*, float, float const*, float*, float*, float*, float*, int, int, int, int, "
            "float)")
FIN_EQ = (f"{_AN}in_stats_finalize_eq_kernel({_F2} const*, float const*, float const*, float, "
          "float const*, float*, float*, float*, float*, int, int, int, float)")
STEM_FWD = (f"void {_NS}conv_stem_fwd_walk_kernel<float, float, 8>(float const*, float const*, "
            f"float const*, float*, int, int, int, int, {_F2}*, {_NS}StemNorm)")
STEM_WGRAD = (f"void {_AN}conv_stem_wgrad_rows_kernel<float, float>(float const*, float const*, "
              f"float*, int, int, int, int, int, long long, {_AN}StemNormW)")
HEAD_FWD = (f"void {_AN}head_fwd_kernel<float>(float const*, float const*, float const*, float*, "
            "long long, int, int, float const*, float const*, float)")
HEAD_BWD = (f"void {_AN}head_bwd_kernel<float>(float const*, float const*, float const*, float*, "
            f"float*, long long, int, int, long long, float const*, float const*, float, {_AN}HeadBs)")
HEAD_BWD_FIN = f"{_AN}head_bwd_finalize_kernel(float const*, float*, float*, int, int)"
TAPS = (f"void {_AN}upsample2x_bwd_taps_kernel<float, 1>(float const*, float*, int, int, int, "
        "long long)")
IN_FIN1 = f"{_AN}in_bwd_finalize1_kernel({_F2} const*, {_F2}*, {_F2}*, int, int, int)"
IN_APPLY = (f"void {_AN}in_bwd_apply_kernel<float>(float const*, float const*, float const*, "
            "float const*, float const*, float const*, float const*, float, "
            f"{_F2} const*, float*, float*, int, int, int, {_F2} const*, float*, float*, float*)")
IN_REDUCE = (f"void {_AN}in_bwd_reduce_kernel<float>(float const*, float const*, float const*, "
             f"float const*, float const*, float const*, float const*, float, {_F2}*, int, int, int)")
# the kernels every step launches outside its convolution, norm and head calls
NCHW_TO_NHWC = f"{_AN}nchw_to_nhwc_kernel(float const*, float*, int, long long, long long)"
PACK_W = f"{_AN}pack_w_batched_kernel(unet_pack_entry const*, int)"
LOSS_REDUCE = f"{_AN}loss_reduce_kernel(float const*, long long const*, float*, int, int)"
LOSS_FINALIZE = (f"{_AN}loss_finalize_kernel(float const*, int, int, float, float, float, int, "
                 f"float const*, float, float*, {_AN}LossCoef*, float*)")
LOSS_GRAD = (f"{_AN}loss_grad_kernel(float const*, long long const*, {_AN}LossCoef const*, "
             "float const*, float*, int, int, float const*)")
# (their uint8-target twins and the two kernels of the sharded loss: no step launches them, so
# they have no entry in ALLOWED; tests/test_loss_fp64_gpu.py asserts them)
LOSS_REDUCE_U8 = f"{_AN}loss_reduce_u8_kernel(float const*, unsigned char const*, float*, int, int)"
LOSS_GRAD_U8 = (f"{_AN}loss_grad_u8_kernel(float const*, unsigned char const*, {_AN}LossCoef const*, "
                "float const*, float*, int, int, float const*)")
LOSS_SHARD_STATS = f"{_AN}loss_shard_stats_kernel(float const*, int, int, float, double*, double*)"
LOSS_SHARD_APPLY = (f"{_AN}loss_shard_apply_kernel(double const*, int, double const*, int, float, float, "
                    f"float, int, float const*, float, float*, {_AN}LossCoef*, float*)")
SGD = (f"{_AN}sgd_nesterov_kernel(float*, float const*, float*, long long, float, float, float, int, "
       "float, float const*)")


# --------------------------------------------------------------------------- the other kernels
# The kernels of a step that are neither convolutions nor norm / head kernels with a row: name ->
# (the existing test that holds it against a reference, that test's smallest call as a function
# of (ua, mode)).  check_allowed runs the call and requires the name, so an entry is a checked
# claim.  A table adds the entries of its mode to a copy of ALLOWED.
def _call_layout(ua, mode):
    ua.ops.nchw_to_nhwc(grand((2, 3, 10, 14), 1))


def _call_pack(ua, mode):
    # (the bf16 planes of a mode that has them come from the same launch)
    ua.ops.PackTable([grand((32, 3, 3, 3), 1), grand((64, 32, 3, 3), 2)], mode.planes).run()


def _call_loss(ua, mode):
    g = torch.Generator(device=DEV).manual_seed(1)
    lg = torch.randn((2, 3, 24, 40), generator=g, device=DEV) * 2.0
    tg = torch.randint(0, 3, (2, 24, 40), generator=g, device=DEV)
    tg[:, :2, :] = 255
    ua.ops.dice_wce_loss_fwd_bwd(lg, tg, 1e-5, 1.0, 1.0, 255, True)


def _call_sgd(ua, mode):
    p, gr = grand((1003,), 30), grand((1003,), 31)
    ua.ops.sgd_nesterov_step(p, gr, torch.zeros_like(p), 0.005, 0.99, 1e-4, True)


_LOSS_TEST = "test_loss_fp64_gpu.py::test_loss_case"
ALLOWED = {
    NCHW_TO_NHWC: ("test_kernels_gpu.py::test_layout_roundtrip", _call_layout),
    PACK_W: ("test_kernels_gpu.py::test_pack_weights_batched_matches_per_layer", _call_pack),
    LOSS_REDUCE: (_LOSS_TEST, _call_loss),
    LOSS_FINALIZE: (_LOSS_TEST, _call_loss),
    LOSS_GRAD: (_LOSS_TEST, _call_loss),
    SGD: ("test_loss_fp64_gpu.py::test_sgd_case", _call_sgd),
}
_CONV_WORDS = ("conv", "wgrad", "taps", "wino_up", "wino32", "igemm", "patch")


def allowed_ids(allowed):
    return [n.replace(_NS, "").replace(_AN, "").split("(")[0] for n in sorted(allowed)]


def check_allowed(ua, mode, allowed, name):
    """The body of test_allowed_kernel_is_launched_by_its_test."""
    held_by, call = allowed[name]
    assert not any(w in short(name) for w in _CONV_WORDS), \
        f"{name}: a convolution kernel needs a row of LAYERS"
    with ua.ops.record_launches() as rec:
        call(ua, mode)
    assert name in rec.names, f"the call of {held_by} launched {rec.names}"


# --------------------------------------------------------------------------- closure
def record_step(ua, precision):
    """The launches of one eager training step of UNet() at N = 8, 512 x 512 in the operand mode
    `precision` (forward, loss, backward, SGD), c32 switch as the network sets it: the authority
    for the name set of that mode."""
    from oracle import unet_ref as O
    torch.manual_seed(0)
    model = ua.UNet().to(DEV).train()
    model.matmul_precision = precision
    opt = ua.create_optimizer(model)
    lossf = ua.get_loss_function()
    img, tgt = O.synthetic_batch(1234, 8, 512, 512)
    img, tgt = img.to(DEV), tgt.to(DEV)
    with ua.ops.record_launches() as rec:
        loss = ua.train_step(model, opt, lossf, img, tgt)
        torch.cuda.synchronize()
    assert torch.isfinite(loss)
    return rec.names


def check_step_is_held(step_names, precision, layers, allowed):
    """Every kernel of the step is one a row of `layers` (names in column 4) or an entry of
    `allowed` holds."""
    assert len(step_names) > 100
    held = set(allowed).union(*(r[4] for r in layers))
    stray = sorted(set(step_names) - held)
    assert not stray, f"kernels of the {precision} step no case holds:\n" + "\n".join(stray)


def check_rows_run_in_the_step(step_names, precision, layers, allowed):
    """The converse: no row, and no entry of `allowed`, for a kernel the step does not launch."""
    step = set(step_names)
    dead = sorted((r[0], n) for r in layers for n in set(r[4]) if n not in step)
    dead += sorted(("ALLOWED", n) for n in allowed if n not in step)
    assert not dead, f"rows for kernels the {precision} step does not launch:\n" + \
        "\n".join(f"{i}: {n}" for i, n in dead)
