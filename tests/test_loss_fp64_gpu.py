"""The loss and optimizer kernels of the train step held to float64 across their argument space,
launches asserted (-m gpu), with the head at K != 3 and exact argmax ties beside them.

LOSS.  One table (tests/tools/loss_refs.py: LOSS_CASES), one case per row: shapes from a single
pixel to a ragged ninth sweep of the 128-block reduction (520 x 520) and the admitted batch limit
(1024 images; 631 is the first batch whose finalize kernel needs more than 64 KiB of dynamic LDS),
every scalar argument varied around 2 x 24 x 40 and 2 x 17 x 9, four kinds of logits, four kinds of
targets, and the forms: the one-call form (every case), forward + separate gradient pass, the
sharded pair with one and with three uneven shards, and the uint8-target twins.  Every form is
compared with the same float64 evaluation (simple_loss64); where unet_hip.h promises identical bits
the forms are also bit-equal to each other.  Bounds: the floor is what
tests/test_kernels_gpu.py::test_loss_vs_oracle holds against the fp32 oracle (loss, ce, dice 2e-6
relative; class weights 1e-6; dlogits 2e-5 of max |dlogits|); a case's bound is max(floor, 3 x the
fp32 oracle's own error against the same float64 reference), computed here.
tests/test_loss_refs_cpu.py shows, on these cases, that altering any one argument moves the
reference by at least 10x the bound.

SGD.  unet_sgd_nesterov_step and the device-hyper form a graph-captured step launches, three steps
from a first step whose momentum buffer holds garbage, against sgd_nesterov64 at
tests/test_kernels_gpu.py::test_sgd_golden's bound (1e-6 of max, parameters and momentum); the two
forms bit-equal.

Measured on an MI355X: profiles/loss_fp64_errors.txt (each test prints its figures before it
asserts)."""
import importlib.util
import json
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16

_spec = importlib.util.spec_from_file_location("step_kernel_harness", os.path.join(
    os.path.dirname(os.path.abspath(__file__)), "tools", "step_kernel_harness.py"))
HS = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(HS)
L = HS.load("loss_refs", "tools")
SLOPE = HS.SLOPE


def show(kind, name, **figures):
    print(f"\n{kind} {name} " + json.dumps(figures, sort_keys=True))


# --------------------------------------------------------------------------- loss
def _names(u8):
    return (HS.LOSS_REDUCE_U8, HS.LOSS_GRAD_U8) if u8 else (HS.LOSS_REDUCE, HS.LOSS_GRAD)


class _Calls:
    """The library calls of one case on one target tensor, each with its launches asserted."""

    def __init__(self, ua, case, lgd, tgd):
        self.ops, self.case, self.lg, self.tg = ua.ops, case, lgd, tgd
        cw = L.fixed_weights_of(case)
        self.args = (case.w_dice, case.w_ce, case.ignore, case.weights == "dynamic")
        self.kw = dict(class_weights=None if cw is None else cw.to(DEV), grad_scale=case.grad_scale)
        self.reduce, self.grad = _names(tgd.dtype == torch.uint8)

    def _rec(self, fn, expect):
        with self.ops.record_launches() as rec:
            out = fn()
        assert rec.names == expect, f"launched {rec.names}"
        return out

    def one_call(self):
        return self._rec(lambda: self.ops.dice_wce_loss_fwd_bwd(
            self.lg, self.tg, self.case.smooth, *self.args, **self.kw),
            [self.reduce, HS.LOSS_FINALIZE, self.grad])

    def forward_only(self, ws):
        out, none = self._rec(lambda: self.ops.dice_wce_loss_fwd_bwd(
            self.lg, self.tg, self.case.smooth, *self.args, want_grad=False, ws=ws, **self.kw),
            [self.reduce, HS.LOSS_FINALIZE])
        assert none is None
        return out

    def gradient(self, ws, upstream):
        return self._rec(lambda: self.ops.dice_wce_loss_grad(self.lg, self.tg, ws, upstream,
                                                             self.case.ignore), [self.grad])

    def shards(self, sizes):
        """shard_stats per shard, the statistics summed on the host in double, shard_apply per
        shard -> [(loss_out, dlogits)]"""
        parts, n0 = [], 0
        for n in sizes:
            parts.append((self.lg[n0:n0 + n].contiguous(), self.tg[n0:n0 + n].contiguous()))
            n0 += n
        assert n0 == self.lg.shape[0]
        phase1 = [self._rec(lambda lg=lg, tg=tg: self.ops.dice_wce_loss_shard_stats(
            lg, tg, self.case.smooth, self.case.ignore), [self.reduce, HS.LOSS_SHARD_STATS])
            for lg, tg in parts]
        total = sum(st.cpu() for st, _ in phase1)
        assert total.dtype == torch.float64
        total = total.to(DEV)
        return [self._rec(lambda lg=lg, tg=tg, ws=ws: self.ops.dice_wce_loss_shard_apply(
            lg, tg, total, n0, ws, self.case.smooth, *self.args, **self.kw),
            [HS.LOSS_SHARD_APPLY, self.grad]) for (lg, tg), (_, ws) in zip(parts, phase1)]


def _errors(out, dl, ref):
    out = out.cpu()
    return L.errors(out[0], out[1], out[2], out[3:6], dl, ref)


def _failures(what, err, bound):
    return [f"{what} {k}: {err[k]:.3e} > {bound[k]:.1e}" for k in err if not err[k] <= bound[k]]


@pytest.mark.parametrize("name", list(L.LOSS_CASES))
def test_loss_case(ua, name):
    case = L.LOSS_CASES[name]
    lg, tg = L.make_loss_case(case, L.case_seed(name))
    N = case.shape[0]
    ref = L.reference(case, lg, tg)
    bound, oracle = L.bounds(case, lg, tg, ref)
    lgd = lg.to(DEV)
    calls = _Calls(ua, case, lgd, tg.to(DEV))
    out, dl = calls.one_call()
    torch.cuda.synchronize()
    err = {"one-call": _errors(out, dl, ref)}
    equal = {}
    if case.targets == "image_ignored":
        equal["an ignored image has dlogits == 0"] = bool((dl[-1] == 0).all())
    if case.form == "grad":
        ws = ua.ops.dice_wce_loss_workspace(lgd)
        out2 = calls.forward_only(ws)
        equal["forward-only loss_out"] = torch.equal(out2[:6], out[:6])
        equal["gradient pass, no upstream"] = torch.equal(calls.gradient(ws, None), dl)
        up = torch.tensor(case.upstream, device=DEV)
        err["upstream"] = _errors(out2, calls.gradient(ws, up),
                                  L.reference(case, lg, tg, upstream=case.upstream))
    if case.form == "shard1":
        (out_s, dl_s), = calls.shards((N,))
        equal["one shard loss_out"] = torch.equal(out_s[:6], out[:6])
        equal["one shard dlogits"] = torch.equal(dl_s, dl)
    shard3 = None
    if case.form == "shard3":
        shard3, n0 = calls.shards(L.SHARDS), 0
        for k, (out_s, dl_s) in enumerate(shard3):
            n = L.SHARDS[k]
            part = ref._replace(dlogits=ref.dlogits[n0:n0 + n])
            err[f"shard {k}"] = _errors(out_s, dl_s, part)
            equal[f"shard {k} loss_out as shard 0"] = torch.equal(out_s[:6], shard3[0][0][:6])
            n0 += n
    if case.tdtype == "u8":       # the int64 forms on the cleaned mask: the same bits
        twin = _Calls(ua, case, lgd, L.clean_mask(tg).to(DEV))
        out_t, dl_t = twin.one_call()
        equal["u8 one-call loss_out"] = torch.equal(out[:6], out_t[:6])
        equal["u8 one-call dlogits"] = torch.equal(dl, dl_t)
        ws, ws_t = ua.ops.dice_wce_loss_workspace(lgd), ua.ops.dice_wce_loss_workspace(lgd)
        equal["u8 forward-only"] = torch.equal(calls.forward_only(ws)[:6], twin.forward_only(ws_t)[:6])
        up = torch.tensor(-2.75, device=DEV)
        equal["u8 gradient pass"] = torch.equal(calls.gradient(ws, up), twin.gradient(ws_t, up))
        sizes = L.SHARDS if case.form == "shard3" else (N,)
        mine = shard3 if shard3 is not None else calls.shards(sizes)
        for k, ((oa, da), (ob, db)) in enumerate(zip(mine, twin.shards(sizes))):
            equal[f"u8 shard {k}"] = torch.equal(oa[:6], ob[:6]) and torch.equal(da, db)
    show("LOSS", name, errors=err, bounds=bound, oracle=oracle, equal=equal)
    bad = [m for what, e in err.items() for m in _failures(what, e, bound)]
    bad += [f"not bit-equal: {k}" for k, v in equal.items() if not v]
    assert not bad, f"{name}: " + "; ".join(bad)


def test_loss_refuses_a_batch_past_the_limit(ua):
    """1025 images: UNET_E_INVALID from all four entry points, before any launch."""
    lg = torch.zeros((1025, 3, 2, 2), device=DEV)
    tg = torch.zeros((1025, 2, 2), dtype=torch.int64, device=DEV)
    ws = torch.empty(1 << 22, dtype=torch.uint8, device=DEV)
    stats = torch.zeros(10, dtype=torch.float64, device=DEV)
    calls = [lambda: ua.ops.dice_wce_loss_fwd_bwd(lg, tg, 1e-5, 1.0, 1.0, 255, True, ws=ws),
             lambda: ua.ops.dice_wce_loss_grad(lg, tg, ws, None, 255),
             lambda: ua.ops.dice_wce_loss_shard_stats(lg, tg, 1e-5, 255),
             lambda: ua.ops.dice_wce_loss_shard_apply(lg, tg, stats, 1025, ws, 1e-5, 1.0, 1.0, 255,
                                                      True)]
    with ua.ops.record_launches() as rec:
        for call in calls:
            with pytest.raises(RuntimeError, match="bad shape"):
                call()
    assert rec.names == []


# --------------------------------------------------------------------------- SGD
@pytest.mark.parametrize("gs", L.SGD_GRAD_SCALES)
@pytest.mark.parametrize("args", list(L.SGD_ARGS))
@pytest.mark.parametrize("n", L.SGD_SIZES)
def test_sgd_case(ua, n, args, gs):
    lr, mu, wd = L.SGD_ARGS[args]
    p0, junk, grads = L.make_sgd_case(n, 100 + n)
    traj = L.sgd_trajectory64(p0, junk, grads, lr, mu, wd, gs)
    p, buf = p0.to(DEV), junk.to(DEV)
    p_dev, buf_dev = p.clone(), buf.clone()
    hyper = torch.tensor([lr, mu, wd, gs], dtype=torch.float32, device=DEV)
    worst, bad = 0.0, []
    for s, g in enumerate(grads):
        gd = g.to(DEV)
        with ua.ops.record_launches() as rec:
            ua.ops.sgd_nesterov_step(p, gd, buf, lr, mu, wd, s == 0, gs)
            ua.ops.sgd_nesterov_step_dev(p_dev, gd, buf_dev, hyper, s == 0)
        assert rec.names == [HS.SGD, HS.SGD]
        if not (torch.equal(p, p_dev) and torch.equal(buf, buf_dev)):
            bad.append(f"step {s}: the device-hyper form differs from the host-argument form")
        if lr == 0.0 and not torch.equal(p.cpu(), p0):
            bad.append(f"step {s}: lr = 0 changed the parameters")
        for what, got, ref in (("p", p, traj[s][0]), ("momentum", buf, traj[s][1])):
            e = L.of_max(got, ref)
            worst = max(worst, e)
            if not e <= L.TOL_SGD:
                bad.append(f"step {s} {what}: {e:.3e} > {L.TOL_SGD:.0e}")
    show("SGD", f"{args}-gs{gs}-n{n}", worst=worst, bound=L.TOL_SGD)
    assert not bad, "; ".join(bad)


# --------------------------------------------------------------------------- head, K != 3
def _head_operands(N, H, W, K):
    y = HS.grand((N, H, W, 32), 1)
    al, be = HS.coeffs(N, 32, 50)
    w, b = HS.grand((K, 32), 2, 0.2), HS.grand((K,), 3, 0.1)
    dl = HS.grand((N, K, H, W), 4)
    return y, al, be, w, b, dl


def _head_ref(a64_nchw, w, b, dl):
    """fp64 conv2d (1 x 1) and its autograd on the CPU -> logits, da, dw, db"""
    a = a64_nchw.cpu().clone().requires_grad_(True)
    wr = w.double().cpu()[:, :, None, None].clone().requires_grad_(True)
    br = b.double().cpu().clone().requires_grad_(True)
    logits = F.conv2d(a, wr, br)
    da, dw, db = torch.autograd.grad(logits, (a, wr, br), dl.double().cpu())
    return logits.detach(), da, dw[:, :, 0, 0], db


@pytest.mark.parametrize("shape", [(2, 12, 20), (3, 17, 9)])
@pytest.mark.parametrize("K", [1, 2, 4])
def test_head_other_class_counts(ua, K, shape):
    """head1x1_fwd / _bwd (plain operand), head1x1_in_fwd / _in_bwd (activation on load; with and
    without the next layer's reductions) on fp32 tensors at the harness's bounds, and on bf16
    tensors at the bounds tests/test_bf16_gpu.py holds K = 3 to.  3 x 17 x 9: M = 459 is no
    multiple of either tile and tiles straddle images."""
    N, H, W = shape
    y, al, be, w, b, dl = _head_operands(N, H, W, K)
    metrics = []

    def held(tag, logits, da, dw, db, ref, tx, tw):
        metrics.extend([HS.metric(f"{tag} logits", logits.cpu(), ref[0], tx),
                        HS.metric(f"{tag} da", HS.nchw64(da).cpu(), ref[1], tx),
                        HS.metric(f"{tag} dw", dw.cpu(), ref[2], tw),
                        HS.metric(f"{tag} db", db.cpu(), ref[3], tw)])

    def grads():
        return torch.empty(K, 32, device=DEV), torch.empty(K, device=DEV)

    # plain operand
    ref = _head_ref(HS.nchw64(y), w, b, dl)
    with ua.ops.record_launches() as rec:
        logits = ua.ops.head1x1_fwd(y, w, b)
        dw, db = grads()
        da = ua.ops.head1x1_bwd(y, dl, w, dw, db)
    assert rec.names == [HS.HEAD_FWD, HS.HEAD_BWD, HS.HEAD_BWD_FIN], rec.names
    held("plain", logits, da, dw, db, ref, HS.TOL_HEAD_X, HS.TOL_HEAD)
    # activated on load
    ref = _head_ref(HS.act64(y, al, be), w, b, dl)
    with ua.ops.record_launches() as rec:
        logits = ua.ops.head1x1_in_fwd(ua.ops.Act(y, al, be), SLOPE, w, b)
        dw, db = grads()
        da = ua.ops.head1x1_in_bwd(ua.ops.Act(y, al, be), SLOPE, dl, w, dw, db)
    assert rec.names == [HS.HEAD_FWD, HS.HEAD_BWD, HS.HEAD_BWD_FIN], rec.names
    held("act", logits, da, dw, db, ref, HS.TOL_HEAD_X, HS.TOL_HEAD)
    # ... with the reductions of the layer in front asked for
    nn = HS.next_norm(ua, N, H, W, 32, 60)
    al2, be2 = (nn.st[2] * nn.mask).contiguous(), (nn.st[3] * nn.mask).contiguous()
    ref = _head_ref(HS.act64(nn.y, al2, be2), w, b, dl)
    dw, db = grads()
    dw0, db0 = grads()
    with ua.ops.record_launches() as rec:
        da = ua.ops.head1x1_in_bwd(ua.ops.Act(nn.y, al2, be2), SLOPE, dl, w, dw, db, nxt=nn)
    assert rec.names == [HS.HEAD_BWD, HS.HEAD_BWD_FIN], rec.names
    da0 = ua.ops.head1x1_in_bwd(ua.ops.Act(nn.y, al2, be2), SLOPE, dl, w, dw0, db0)
    assert torch.equal(da, da0) and torch.equal(dw, dw0) and torch.equal(db, db0), \
        "asking for the reductions changed the gradients"
    held("nxt", ua.ops.head1x1_in_fwd(ua.ops.Act(nn.y, al2, be2), SLOPE, w, b), da, dw, db, ref,
         HS.TOL_HEAD_X, HS.TOL_HEAD)
    if nn.tiles > 0:
        metrics.extend(HS.summaries(ua, da, nn))
    # bf16 tensors: fp32 arithmetic on bf16 storage, da stored as bf16
    yb = y.to(BF)
    ref = _head_ref(HS.act64(yb, al, be), w, b, dl)
    with ua.ops.record_launches() as rec:
        logits = ua.ops.head1x1_in_fwd(ua.ops.Act(yb, al, be), SLOPE, w, b)
        dw, db = grads()
        da = ua.ops.head1x1_in_bwd(ua.ops.Act(yb, al, be), SLOPE, dl, w, dw, db)
    assert len(rec.names) == 3 and "head_fwd_kernel" in rec.names[0] and \
        "head_bwd_kernel" in rec.names[1] and rec.names[2] == HS.HEAD_BWD_FIN, rec.names
    assert logits.dtype == torch.float32 and da.dtype == BF
    metrics.extend([HS.metric("b16 logits", logits.cpu(), ref[0], 1e-4),
                    HS.metric("b16 da", HS.nchw64(da).cpu(), ref[1], 5e-3),
                    HS.metric("b16 dw", dw.cpu(), ref[2], 1e-4),
                    HS.metric("b16 db", db.cpu(), ref[3], 1e-4)])
    show("HEAD", f"K{K}-{N}x{H}x{W}", **{m["what"]: m["err"] for m in metrics})
    assert not HS.R.failures(metrics), HS.R.failures(metrics)


# --------------------------------------------------------------------------- argmax ties
@pytest.mark.parametrize("tdtype", [torch.int64, torch.uint8])
@pytest.mark.parametrize("shape", [(2, 5, 7), (2, 8, 8), (1, 33, 65)])
def test_argmax_dice_counts_exact_ties(ua, shape, tdtype):
    """Exact ties between planes (0,1), (1,2), (0,2) and all three, as the largest value and not:
    the first maximum wins like torch.argmax on the CPU; the counts are exact integers.  5 x 7
    and 33 x 65: HW % 4 != 0, the one-pixel-per-lane form for a uint8 target as well; 8 x 8: its
    four-pixel form."""
    N, H, W = shape
    g = torch.Generator().manual_seed(H * W)
    z = torch.randn(N, 3, H, W, generator=g)
    kind = torch.randint(0, 5, (N, H, W), generator=g)
    for k, (a, b) in {1: (0, 1), 2: (1, 2), 3: (0, 2)}.items():
        z[:, b] = torch.where(kind == k, z[:, a], z[:, b])
    z[:, 1] = torch.where(kind == 4, z[:, 0], z[:, 1])
    z[:, 2] = torch.where(kind == 4, z[:, 0], z[:, 2])
    tg = torch.randint(0, 3, (N, H, W), generator=g)
    tg[torch.rand(N, H, W, generator=g) < 0.15] = 255
    ref_p = z.argmax(dim=1)
    tied_max = sum(int(((z[:, a] == z[:, b]) & (z[:, a] == z.max(dim=1).values)).sum())
                   for a, b in ((0, 1), (1, 2), (0, 2)))
    assert tied_max > 0
    preds, counts = ua.ops.argmax_dice_counts(z.to(DEV), tg.to(tdtype).to(DEV))
    assert torch.equal(preds.cpu().long(), ref_p)
    valid = tg != 255
    for c in range(3):
        pc, mc = (ref_p == c) & valid, (tg == c) & valid
        assert counts[c].tolist() == [int((pc & mc).sum()), int(pc.sum()), int(mc.sum())]
