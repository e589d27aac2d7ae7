"""tests/tools/loss_refs.py without a GPU: the float64 references of SimpleLoss and of the
Nesterov SGD step agree with the fp32 oracle (to fp32 rounding) and with torch.optim.SGD run in
double, and - the check of the check - on the very cases tests/test_loss_fp64_gpu.py runs, altering
any one scalar argument moves the reference by at least 10x the bound the GPU test holds the
kernels to, so a kernel that ignored or mixed up the argument cannot pass."""
import importlib.util
import os

import pytest
import torch

from oracle import unet_ref as O

TESTS = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("loss_refs", os.path.join(TESTS, "tools", "loss_refs.py"))
L = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(L)


seed_of = L.case_seed


# --------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("name", ["shape-2x17x9", "shape-2x24x40", "shape-32x8x8"])
def test_simple_loss64_agrees_with_the_fp32_oracle(name):
    """Default arguments: the oracle is the same arithmetic in fp32 - a few fp32 roundings apart
    (1e-6 of the value, 2e-6 of the largest gradient: a tenth of the GPU test's floors)."""
    case = L.LOSS_CASES[name]
    lg, tg = L.make_loss_case(case, seed_of(name))
    ref = L.reference(case, lg, tg)
    oe = L.oracle_errors(case, lg, tg, ref)
    assert oe["loss"] <= 1e-6 and oe["ce"] <= 1e-6 and oe["dice"] <= 1e-6, oe
    assert oe["weights"] <= 1e-6 and oe["dlogits"] <= 2e-6, oe
    assert abs(ref.class_weights.sum().item() - 3.0) <= 1e-12
    assert L.of_max(L.class_weights64(tg, 255), O.class_weights(tg)) <= 1e-6


def test_simple_loss64_static_and_unweighted_agree_with_the_fp32_oracle():
    for name in ("weights-static-24x40", "weights-none-24x40", "form-grad-17x9-static"):
        case = L.LOSS_CASES[name]
        lg, tg = L.make_loss_case(case, seed_of(name))
        ref = L.reference(case, lg, tg)
        oe = L.oracle_errors(case, lg, tg, ref)
        assert max(oe["loss"], oe["ce"], oe["dice"]) <= 1e-6 and oe["dlogits"] <= 2e-6, (name, oe)
    assert torch.equal(ref.class_weights, torch.tensor(L.STATIC).double())


def test_shards_add_up_to_the_concatenated_batch():
    for name in ("form-shard3", "cross-shard3-static-third", "cross-shard3-u8-ignore7"):
        case = L.LOSS_CASES[name]
        lg, tg = L.make_loss_case(case, seed_of(name))
        whole = L.reference(case, lg, tg)
        labels = L.labels_of(case, tg)
        parts, n0 = [], 0
        for n in L.SHARDS:
            part = L.simple_loss64(lg[n0:n0 + n], labels[n0:n0 + n], n_global=case.shape[0],
                                   global_target=labels, **L.ref_kwargs(case))
            assert L.of_max(part.dlogits, whole.dlogits[n0:n0 + n]) <= 1e-12
            assert L.of_max(part.class_weights, whole.class_weights) <= 1e-15
            parts.append(part)
            n0 += n
        for k in ("loss", "ce", "dice"):
            assert L.rel(sum(getattr(p, k) for p in parts), getattr(whole, k)) <= 1e-12


def test_an_ignored_image_has_no_gradient_and_unit_dice():
    case = L.LOSS_CASES["targets-image-ignored"]
    lg, tg = L.make_loss_case(case, 3)
    ref = L.reference(case, lg, tg)
    assert bool((ref.dlogits[-1] == 0).all()) and bool((ref.dlogits[0] != 0).any())


def test_sgd_nesterov64_agrees_with_the_oracle_and_torch_sgd():
  for n in (1, 2, 3, 4, 5, 1003):          # (the seeds of tests/test_loss_fp64_gpu.py::test_sgd_case)
    p0, junk, grads = L.make_sgd_case(n, 100 + n)
    for lr, mu, wd in L.SGD_ARGS.values():
        traj = L.sgd_trajectory64(p0, junk, grads, lr, mu, wd, 1.0)
        # the fp32 oracle
        ps, bufs = [p0.clone()], [None]
        for s, g in enumerate(grads):
            O.sgd_nesterov_(ps, [g], bufs, lr, mu, wd)
            assert L.of_max(ps[0], traj[s][0]) <= L.TOL_SGD
            assert L.of_max(bufs[0], traj[s][1]) <= L.TOL_SGD
        # torch.optim.SGD in double
        p = p0.double().clone().requires_grad_(True)
        opt = torch.optim.SGD([p], lr=lr, momentum=mu, weight_decay=wd, nesterov=mu > 0)
        for s, g in enumerate(grads):
            p.grad = g.double().clone()
            opt.step()
            assert L.of_max(p.detach(), traj[s][0]) <= 1e-13, (lr, mu, wd, s)
    # grad_scale multiplies the gradient
    a = L.sgd_trajectory64(p0, junk, grads, 0.005, 0.99, 1e-4, 0.5)
    b = L.sgd_trajectory64(p0, junk, [g * 0.5 for g in grads], 0.005, 0.99, 1e-4, 1.0)
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a, b))


def test_loss_batch_limit_is_checked_before_any_launch(ua):
    """The four entry points that share the limit (and their uint8 twins) take 1024 images - they
    stop at the workspace size, still before a launch - and refuse 1025 with UNET_E_INVALID."""
    lib = ua.lib()

    def fwd_bwd(sfx, n, ws):
        return getattr(lib, "unet_dice_wce_loss_fwd_bwd" + sfx)(
            1, 1, 1, None, 1, ws, n, 4, 4, 1e-5, 1.0, 1.0, 255, 1, None, 1.0, None)

    def grad(sfx, n, ws):
        return getattr(lib, "unet_dice_wce_loss_grad" + sfx)(1, 1, 1, ws, None, 1, n, 4, 4, 255, None)

    def stats(sfx, n, ws):
        return getattr(lib, "unet_dice_wce_loss_shard_stats" + sfx)(
            1, 1, 1, 1, ws, n, 4, 4, 1e-5, 255, None)

    def apply(sfx, n, ws):
        return getattr(lib, "unet_dice_wce_loss_shard_apply" + sfx)(
            1, 1, 1, n, 1, None, 1, ws, n, 4, 4, 1e-5, 1.0, 1.0, 255, 1, None, 1.0, None)

    for fn in (fwd_bwd, grad, stats, apply):
        for sfx in ("", "_u8"):
            assert fn(sfx, 1025, 1 << 30) == -1 and b"bad shape" in lib.unet_last_error(), fn.__name__
            assert fn(sfx, 1024, 16) == -3, fn.__name__
    assert lib.unet_dice_wce_loss_workspace_bytes(1024, 4, 4) > 1024 * 128 * 13 * 4


# --------------------------------------------------------------------------- the check of the check
LOSS_ARGUMENTS = ("w_dice", "w_ce", "smooth", "ignore_index", "grad_scale", "upstream",
                  "static weights", "n_global")


@pytest.mark.parametrize("name", list(L.LOSS_CASES))
def test_every_loss_argument_moves_the_reference(name):
    case = L.LOSS_CASES[name]
    lg, tg = L.make_loss_case(case, seed_of(name))
    labels = L.labels_of(case, tg)
    ref = L.reference(case, lg, tg, upstream=case.upstream)
    bound, _ = L.bounds(case, lg, tg, L.reference(case, lg, tg))
    alts = L.alterations(case)
    assert set(case.hides) <= set(alts), "hides names an argument the case does not have"
    for arg, over in alts.items():
        if arg in case.hides:
            continue
        if arg == "n_global":       # the last shard of the concatenated batch
            n0 = case.shape[0] - L.SHARDS[-1]
            kw = dict(L.ref_kwargs(case), global_target=labels)
            base = L.simple_loss64(lg[n0:], labels[n0:], n_global=case.shape[0], **kw)
            alt = L.simple_loss64(lg[n0:], labels[n0:], **{**kw, **over})
        else:
            base, alt = ref, L.reference(case, lg, tg, **{"upstream": case.upstream, **over})
        move = L.moved(alt, base)
        shown = {k: v / bound[k] for k, v in move.items()}
        assert any(v >= 10.0 for v in shown.values()), \
            f"{name}: altering {arg} moves the reference by {move}, bounds {bound}"


def test_every_loss_argument_is_shown_by_its_sweep():
    """No argument is hidden where it is swept, and each is shown by at least four cases."""
    shown = {a: 0 for a in LOSS_ARGUMENTS}
    for name, case in L.LOSS_CASES.items():
        for a in L.alterations(case):
            shown[a] += a not in case.hides
        if case.shape in ((2, 17, 9), (2, 24, 40), (6, 17, 9), (6, 24, 40)):
            assert not case.hides, name
    assert all(v >= 2 for v in shown.values()) and shown["w_dice"] >= 4, shown


@pytest.mark.parametrize("args", list(L.SGD_ARGS))
@pytest.mark.parametrize("n", [1, 5, 1003])
def test_every_sgd_argument_moves_the_reference(n, args):
    """(the sizes share their arithmetic: 1, 5 and 1003 elements stand for all of SGD_SIZES)"""
    lr, mu, wd = L.SGD_ARGS[args]
    p0, junk, grads = L.make_sgd_case(n, 100 + n)
    for gs in L.SGD_GRAD_SCALES:
        kw = dict(lr=lr, mu=mu, wd=wd, grad_scale=gs)
        ref = L.sgd_trajectory64(p0, junk, grads, **kw)
        for arg, over in L.sgd_alterations(**kw).items():
            if (args, arg) in L.SGD_HIDES:
                continue
            alt = L.sgd_trajectory64(p0, junk, grads, **{**kw, **over})
            move = max(max(L.of_max(a[0], r[0]), L.of_max(a[1], r[1])) for a, r in zip(alt, ref))
            assert move >= 10.0 * L.TOL_SGD, f"n={n} {args} grad_scale={gs}: {arg} moves {move:.2e}"
