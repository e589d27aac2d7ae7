"""The K-class tail on the GPU (-m gpu): the matrix-core head for 5..32 classes, the K-class
SimpleLoss, argmax / counts / confusion, and UNet / CLIPUNet with 5 classes end to end.

Every comparison is against a float64 evaluation written from the oracle's K-generic pieces
(tests/tools/kclass_refs.py; tests/test_kclass_cpu.py ties it to oracle.simple_loss at K = 3),
never against the code under test.  Launches are asserted with ops.record_launches(): the new
kernels for the new path, today's kernels at K = 3 (loss, counts) and K <= 4 (head).

Bounds.  Head: the ones tests/test_loss_fp64_gpu.py::test_head_other_class_counts holds K <= 4
to (the dot length is still 32, the pixel reduction the same).  Loss: max(floor, 3 x the fp32
torch evaluation's own error against the same float64 reference), the floor being what
test_kernels_gpu.py::test_loss_vs_oracle holds; computed per case and printed before asserting.
Integers are exact.  Whole model: the bounds tests/test_net_gpu.py applies at 64 x 64."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import unet_ref as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16

_spec = importlib.util.spec_from_file_location("step_kernel_harness", os.path.join(
    os.path.dirname(os.path.abspath(__file__)), "tools", "step_kernel_harness.py"))
HS = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(HS)
KR = HS.load("kclass_refs", "tools")
SLOPE = HS.SLOPE


def show(kind, name, **figures):
    print(f"\n{kind} {name} " + json.dumps(figures, sort_keys=True))


def kp_of(K):
    return 4 if K <= 4 else 8 if K <= 8 else 16 if K <= 16 else 32


def launched(names, *fragments):
    """The recorded launches are exactly one kernel per fragment, in order."""
    assert len(names) == len(fragments) and all(f in n for f, n in zip(fragments, names)), \
        f"launched {names}, expected {fragments}"


# --------------------------------------------------------------------------- head
def _head_ref(a64_nchw, w, b, dl):
    """fp64 conv2d (1 x 1) and its autograd on the CPU -> logits, da, dw, db"""
    a = a64_nchw.cpu().clone().requires_grad_(True)
    wr = w.double().cpu()[:, :, None, None].clone().requires_grad_(True)
    br = b.double().cpu().clone().requires_grad_(True)
    logits = F.conv2d(a, wr, br)
    da, dw, db = torch.autograd.grad(logits, (a, wr, br), dl.double().cpu())
    return logits.detach(), da, dw[:, :, 0, 0], db


@pytest.mark.parametrize("shape", [(2, 24, 40), (2, 17, 9), (1, 64, 64)])
@pytest.mark.parametrize("K", [5, 8, 21, 32])
def test_head_5_to_32_classes(ua, K, shape):
    """2 x 17 x 9: 306 pixels are no multiple of the 32-pixel tile and tiles straddle the two
    images; 2 x 24 x 40 and 1 x 64 x 64 take several workgroups."""
    N, H, W = shape
    y = HS.grand((N, H, W, 32), 1)
    al, be = HS.coeffs(N, 32, 50)
    w, b = HS.grand((K, 32), 2, 0.2), HS.grand((K,), 3, 0.1)
    dl = HS.grand((N, K, H, W), 4)
    metrics = []

    def held(tag, logits, da, dw, db, ref, tx, tw, tda=None):
        metrics.extend([HS.metric(f"{tag} logits", logits.cpu(), ref[0], tx),
                        HS.metric(f"{tag} da", HS.nchw64(da).cpu(), ref[1], tx if tda is None else tda),
                        HS.metric(f"{tag} dw", dw.cpu(), ref[2], tw),
                        HS.metric(f"{tag} db", db.cpu(), ref[3], tw)])

    def grads():
        return torch.empty(K, 32, device=DEV), torch.empty(K, device=DEV)

    fwd, bwd, fin = "headk_fwd_kernel<float>", "headk_bwd_kernel<float>", "headk_bwd_finalize_kernel"
    # plain operand
    ref = _head_ref(HS.nchw64(y), w, b, dl)
    with ua.ops.record_launches() as rec:
        logits = ua.ops.head1x1_fwd(y, w, b)
        dw, db = grads()
        da = ua.ops.head1x1_bwd(y, dl, w, dw, db)
    launched(rec.names, fwd, bwd, fin)
    held("plain", logits, da, dw, db, ref, HS.TOL_HEAD_X, HS.TOL_HEAD)
    dw2, db2 = grads()
    da2 = ua.ops.head1x1_bwd(y, dl, w, dw2, db2)
    assert torch.equal(da, da2) and torch.equal(dw, dw2) and torch.equal(db, db2) and \
        torch.equal(logits, ua.ops.head1x1_fwd(y, w, b)), "two runs differ"
    # activated on load, without and with the next layer's reductions asked for (K > 4 leaves none)
    ref = _head_ref(HS.act64(y, al, be), w, b, dl)
    with ua.ops.record_launches() as rec:
        logits = ua.ops.head1x1_in_fwd(ua.ops.Act(y, al, be), SLOPE, w, b)
        dw, db = grads()
        da = ua.ops.head1x1_in_bwd(ua.ops.Act(y, al, be), SLOPE, dl, w, dw, db)
    launched(rec.names, fwd, bwd, fin)
    held("act", logits, da, dw, db, ref, HS.TOL_HEAD_X, HS.TOL_HEAD)
    nn = HS.next_norm(ua, N, H, W, 32, 60)
    al2, be2 = (nn.st[2] * nn.mask).contiguous(), (nn.st[3] * nn.mask).contiguous()
    ref = _head_ref(HS.act64(nn.y, al2, be2), w, b, dl)
    dw, db = grads()
    with ua.ops.record_launches() as rec:
        da = ua.ops.head1x1_in_bwd(ua.ops.Act(nn.y, al2, be2), SLOPE, dl, w, dw, db, nxt=nn)
    launched(rec.names, bwd, fin)
    assert nn.tiles == 0
    held("nxt", ua.ops.head1x1_in_fwd(ua.ops.Act(nn.y, al2, be2), SLOPE, w, b), da, dw, db, ref,
         HS.TOL_HEAD_X, HS.TOL_HEAD)
    # bf16 tensors: fp32 arithmetic on bf16 storage, da stored as bf16 (the bounds of K <= 4)
    yb = y.to(BF)
    for tag, act, a64 in (("b16 plain", ua.ops.Act(yb, None, None), HS.nchw64(yb)),
                          ("b16 act", ua.ops.Act(yb, al, be), HS.act64(yb, al, be))):
        ref = _head_ref(a64, w, b, dl)
        with ua.ops.record_launches() as rec:
            logits = ua.ops.head1x1_in_fwd(act, SLOPE, w, b)
            dw, db = grads()
            da = ua.ops.head1x1_in_bwd(act, SLOPE, dl, w, dw, db)
        # (the demangler gives up on __bf16: these two names stay mangled)
        launched(rec.names, "headk_fwd_kernelIDF16b", "headk_bwd_kernelIDF16b", fin)
        assert logits.dtype == torch.float32 and da.dtype == BF
        held(tag, logits, da, dw, db, ref, 1e-4, 1e-4, tda=5e-3)
    show("HEADK", f"K{K}-{N}x{H}x{W}", **{m["what"]: m["err"] for m in metrics})
    assert not HS.R.failures(metrics), HS.R.failures(metrics)


@pytest.mark.parametrize("K", [5, 32])
def test_head_writes_nothing_outside_its_tensors(ua, K):
    """logits [N, K, HW] and da [M, 32] inside poisoned buffers (153 pixels: the last tile is
    ragged): the planes beyond K and the rows beyond M keep their poison."""
    N, H, W, PAD = 1, 17, 9, 4096
    M = N * H * W
    y = HS.grand((N, H, W, 32), 1)
    w, b = HS.grand((K, 32), 2, 0.2), HS.grand((K,), 3, 0.1)
    dl = HS.grand((N, K, H, W), 4)
    ops, L = ua.ops, ua.lib()
    lbuf = torch.full((PAD + M * K + PAD,), 7.25, device=DEV)
    dbuf = torch.full((PAD + M * 32 + PAD,), 7.25, device=DEV)
    lg, da = lbuf[PAD:PAD + M * K], dbuf[PAD:PAD + M * 32]
    dw, db = torch.empty(K, 32, device=DEV), torch.empty(K, device=DEV)
    ws = torch.empty(L.unet_head1x1_bwd_workspace_bytes(N, H * W, 32, K), dtype=torch.uint8,
                     device=DEV)
    ops.check(L.unet_head1x1_fwd(y.data_ptr(), w.data_ptr(), b.data_ptr(), lg.data_ptr(), N, H * W,
                                 32, K, ops._stream()))
    ops.check(L.unet_head1x1_bwd(y.data_ptr(), dl.data_ptr(), w.data_ptr(), da.data_ptr(),
                                 dw.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), N, H * W,
                                 32, K, ops._stream()))
    torch.cuda.synchronize()
    for buf, n in ((lbuf, M * K), (dbuf, M * 32)):
        assert bool((buf[:PAD] == 7.25).all()) and bool((buf[PAD + n:] == 7.25).all())
    assert torch.equal(lg.view(N, K, H, W), ops.head1x1_fwd(y, w, b))
    assert bool((da != 7.25).all())


def test_head_up_to_4_classes_keeps_its_kernels(ua):
    y, w, b = HS.grand((1, 8, 8, 32), 1), HS.grand((4, 32), 2, 0.2), HS.grand((4,), 3, 0.1)
    dw, db = torch.empty(4, 32, device=DEV), torch.empty(4, device=DEV)
    with ua.ops.record_launches() as rec:
        ua.ops.head1x1_fwd(y, w, b)
        ua.ops.head1x1_bwd(y, HS.grand((1, 4, 8, 8), 4), w, dw, db)
    assert rec.names == [HS.HEAD_FWD, HS.HEAD_BWD, HS.HEAD_BWD_FIN], rec.names


# --------------------------------------------------------------------------- loss
def _loss_errors(out, dl, ref, K):
    out = out.cpu()
    assert out.numel() == 3 + K
    return KR.errors(out[0], out[1], out[2], out[3:3 + K], dl, ref)


def _run_loss_case(ua, K, shape, weights, kind, seed, upstream=-2.75, grad_scale=0.5):
    """One problem through every form: one call (int64 and raw uint8 targets), forward plus
    separate gradient, upstream scale.  -> (error figures, bounds, bit-equalities)"""
    lg, labels, raw = KR.make_loss_case(K, shape, kind, seed)
    fixed = KR.fixed_weights(K) if weights == "fixed" else None
    kw = dict(w_dice=0.7, w_ce=1.3, smooth=1e-5, ignore_index=255, dynamic=weights == "dynamic",
              fixed_weights=fixed, grad_scale=grad_scale)
    ref = KR.simple_loss_k(lg, labels, **kw)
    bound, oracle = KR.bounds(lg, labels, ref, **kw)
    lgd = lg.to(DEV)
    cw = None if fixed is None else fixed.to(DEV)
    args = (1e-5, 0.7, 1.3, 255, weights == "dynamic")
    kp = kp_of(K)
    err, equal, outs = {}, {}, {}
    for tag, tgd, tt in (("i64", labels.to(DEV), "long long"), ("u8", raw.to(DEV), "unsigned char")):
        red, grad = f"lossk_reduce_kernel<{kp}, {tt}>", f"lossk_grad_kernel<{kp}, {tt}>"
        with ua.ops.record_launches() as rec:
            out, dl = ua.ops.dice_wce_loss_fwd_bwd(lgd, tgd, *args, class_weights=cw,
                                                   grad_scale=grad_scale)
        launched(rec.names, red, "lossk_finalize_kernel", grad)
        err[f"{tag} one-call"] = _loss_errors(out, dl, ref, K)
        ws = ua.ops.dice_wce_loss_workspace(lgd)
        with ua.ops.record_launches() as rec:
            out2, none = ua.ops.dice_wce_loss_fwd_bwd(lgd, tgd, *args, class_weights=cw,
                                                      grad_scale=grad_scale, want_grad=False, ws=ws)
            dl2 = ua.ops.dice_wce_loss_grad(lgd, tgd, ws, None, 255)
        launched(rec.names, red, "lossk_finalize_kernel", grad)
        assert none is None
        equal[f"{tag} forward-only loss_out"] = torch.equal(out2, out)
        equal[f"{tag} separate gradient"] = torch.equal(dl2, dl)
        up = torch.tensor(upstream, device=DEV)
        err[f"{tag} upstream"] = _loss_errors(
            out2, ua.ops.dice_wce_loss_grad(lgd, tgd, ws, up, 255),
            KR.simple_loss_k(lg, labels, upstream=upstream, **kw), K)
        if kind == "image_ignored":
            equal[f"{tag} an ignored image has dlogits == 0"] = bool((dl[-1] == 0).all())
        outs[tag] = (out, dl)
    equal["u8 loss_out as int64 on the cleaned mask"] = torch.equal(outs["u8"][0], outs["i64"][0])
    equal["u8 dlogits as int64 on the cleaned mask"] = torch.equal(outs["u8"][1], outs["i64"][1])
    return err, bound, oracle, equal


def _assert_loss(name, err, bound, oracle, equal):
    show("LOSSK", name, errors=err, bounds=bound, torch_fp32=oracle, equal=equal)
    bad = [f"{what} {k}: {e[k]:.3e} > {bound[k]:.1e}" for what, e in err.items() for k in e
           if not e[k] <= bound[k]]
    bad += [f"not bit-equal: {k}" for k, v in equal.items() if not v]
    assert not bad, f"{name}: " + "; ".join(bad)


@pytest.mark.parametrize("kind", ["missing", "image_ignored", "large"])
@pytest.mark.parametrize("weights", ["dynamic", "fixed", "none"])
@pytest.mark.parametrize("shape", [(2, 24, 40), (2, 17, 9)])
@pytest.mark.parametrize("K", [2, 4, 5, 21, 32])
def test_loss_k_classes(ua, K, shape, weights, kind):
    """Every case has an ignored band and, in its uint8 form, stray labels >= K the rule cleans."""
    name = f"K{K}-{'x'.join(map(str, shape))}-{weights}-{kind}"
    _assert_loss(name, *_run_loss_case(ua, K, shape, weights, kind, 100 + K))


def test_loss_5_classes_at_520x520(ua):
    """270 400 pixels: the 128 slabs of an image each sweep it raggedly."""
    _assert_loss("K5-1x520x520", *_run_loss_case(ua, 5, (1, 520, 520), "dynamic", "missing", 7))


def test_loss_and_counts_at_3_classes_keep_their_kernels(ua):
    lg, labels, _ = KR.make_loss_case(3, (2, 24, 40), "missing", 3)
    with ua.ops.record_launches() as rec:
        out, _ = ua.ops.dice_wce_loss_fwd_bwd(lg.to(DEV), labels.to(DEV), 1e-5, 1.0, 1.0, 255, True)
        ua.ops.argmax_dice_counts(lg.to(DEV), labels.to(DEV))
        ua.ops.eval_confusion(lg.to(DEV), labels.to(DEV))
    assert rec.names[:3] == [HS.LOSS_REDUCE, HS.LOSS_FINALIZE, HS.LOSS_GRAD], rec.names
    assert "argmax_counts_kernel<" in rec.names[3] and "eval_confusion_kernel<" in rec.names[4]
    assert out.numel() == 8


@pytest.mark.parametrize("shape", [(2, 17, 9), (2, 24, 40), (1, 48, 48)])
def test_the_k_form_at_3_classes_is_the_3_class_call(ua, shape):
    """The exports themselves, K-form with K = 3 against the 3-class export: the same launches
    and the same bits.  2 x 17 x 9: 153 pixels are no multiple of 4 (the one-pixel counts kernel,
    the non-vector confusion kernel); 2 x 24 x 40: aligned (four pixels per lane with uint8
    targets, the vector confusion kernel); 1 x 48 x 48: 2304 pixels, two reduce slabs an image."""
    L, ptr, stream = ua.lib(), ua.ops._ptr, ua.ops._stream()
    N, H, W = shape
    aligned = (H * W) % 4 == 0

    def both(base, kform, u8):
        """(export, its class argument) of the 3-class form and of the K-form"""
        sfx = "_u8" if u8 else ""
        return (getattr(L, base + sfx), ()), (getattr(L, kform + sfx), (3,))

    def workspaces(dev):
        n3 = L.unet_dice_wce_loss_workspace_bytes(N, H, W)
        assert n3 == L.unet_dice_wce_lossk_workspace_bytes(N, 3, H, W) > 0
        return [torch.zeros(n3, dtype=torch.uint8, device=dev) for _ in range(2)]

    up = torch.tensor(-2.75, device=DEV)
    for kind in ("missing", "image_ignored"):
        lg, labels, raw = KR.make_loss_case(3, shape, kind, 31)
        lgd = lg.to(DEV)
        for u8, tgd in ((False, labels.to(DEV)), (True, raw.to(DEV))):
            names = [HS.LOSS_REDUCE_U8 if u8 else HS.LOSS_REDUCE, HS.LOSS_FINALIZE,
                     HS.LOSS_GRAD_U8 if u8 else HS.LOSS_GRAD]
            for weights in ("dynamic", "fixed", "none"):
                cw = KR.fixed_weights(3).to(DEV) if weights == "fixed" else None
                got = []
                for (fwd, k), (grad, _), ws in zip(
                        both("unet_dice_wce_loss_fwd_bwd", "unet_dice_wce_lossk_fwd_bwd", u8),
                        both("unet_dice_wce_loss_grad", "unet_dice_wce_lossk_grad", u8),
                        workspaces(DEV)):
                    out, out2 = torch.zeros(8, device=DEV), torch.zeros(8, device=DEV)
                    dl, dl2 = torch.empty_like(lgd), torch.empty_like(lgd)
                    tail = (1e-5, 0.7, 1.3, 255, 1 if weights == "dynamic" else 0, ptr(cw), 0.5,
                            stream)
                    with ua.ops.record_launches() as rec:
                        ua._lib.check(fwd(ptr(lgd), ptr(tgd), ptr(out), ptr(dl), ptr(ws),
                                          ws.numel(), N, *k, H, W, *tail))
                    assert rec.names == names, rec.names
                    # forward only, then the gradient on its own with an upstream scale
                    with ua.ops.record_launches() as rec:
                        ua._lib.check(fwd(ptr(lgd), ptr(tgd), ptr(out2), None, ptr(ws),
                                          ws.numel(), N, *k, H, W, *tail))
                        ua._lib.check(grad(ptr(lgd), ptr(tgd), ptr(ws), ws.numel(), ptr(up),
                                           ptr(dl2), N, *k, H, W, 255, stream))
                    assert rec.names == names, rec.names
                    got.append((out[:6], dl, out2[:6], dl2))
                # (bits, not values: the one image of 1 x 48 x 48, wholly ignored, has a NaN loss)
                for a, b in zip(*got):
                    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), \
                        (kind, u8, weights)
            # argmax and counts
            got = []
            for fn, k in both("unet_argmax_dice_counts", "unet_argmax_countsk", u8):
                preds = torch.full((N, H, W), 77, dtype=torch.uint8, device=DEV)
                counts = torch.full((3, 3), -1, dtype=torch.int64, device=DEV)
                with ua.ops.record_launches() as rec:
                    ua._lib.check(fn(ptr(lgd), ptr(tgd), ptr(preds), counts.data_ptr(), N, *k, H,
                                     W, 255, stream))
                tt = "unsigned char" if u8 else "long long"
                launched(rec.names, f"argmax_counts_kernel<{tt}, {4 if u8 and aligned else 1}>")
                got.append((rec.names, preds, counts))
            assert got[0][0] == got[1][0]
            assert torch.equal(got[0][1], got[1][1]) and torch.equal(got[0][2], got[1][2])
            assert torch.equal(got[0][1].cpu().long(), lg.argmax(1))
        # confusion (int64 targets only): at network size, and with one image upscaled and - where
        # there is a second one - that one given a zero size
        tgd = labels.to(DEV)
        some = torch.tensor([(2 * H + 1, 3 * W), (0, W)][:N], dtype=torch.int64, device=DEV)
        for dims in (None, some):
            got = []
            for fn, k in both("unet_eval_confusion", "unet_eval_confusionk", False):
                cm = torch.full((N, 3, 3), -1, dtype=torch.int64, device=DEV)
                with ua.ops.record_launches() as rec:
                    ua._lib.check(fn(ptr(lgd), ptr(tgd), ptr(dims), cm.data_ptr(), N, *k, H, W,
                                     255, stream))
                launched(rec.names, "eval_confusion_kernel<")
                got.append((rec.names, cm))
            assert got[0][0] == got[1][0] and torch.equal(got[0][1], got[1][1])
            assert ("<true" in got[0][0][0]) == (W % 4 == 0), got[0][0]
            if dims is None:
                want = np.stack([KR.confusion(p, t, 3) for p, t in
                                 zip(lg.argmax(1).numpy(), labels.numpy())])
            else:
                want = KR.resized_confusion(lg.argmax(1).numpy(), labels.numpy(),
                                            some.cpu().tolist(), 3)
            assert np.array_equal(got[0][1].cpu().numpy(), want)


# --------------------------------------------------------------------------- counts, confusion
@pytest.mark.parametrize("K", [2, 5, 32])
def test_counts_and_confusion_are_exact(ua, K):
    N, H, W = 3, 33, 47
    lg = KR.gapped_logits(N, K, H, W, 40 + K)
    # one constructed exact tie: every plane equal on a block, and a two-way tie of the last two
    # classes above the rest - the first maximum wins
    lg[:, :, :4, :8] = 0.5
    lg[:, K - 2:, 4:8, :8] = 9.0
    untied = lg.clone()
    untied[:, 0, :4, :8] += 1.0
    untied[:, K - 2, 4:8, :8] += 1.0
    assert KR.top2_gap(untied) >= 1e-3
    pred = untied.argmax(1)
    assert bool((pred[:, :4, :8] == 0).all()) and bool((pred[:, 4:8, :8] == K - 2).all())
    g = torch.Generator().manual_seed(K)
    tgt = torch.randint(0, K, (N, H, W), generator=g)
    tgt[:, -2:, :] = 255
    tgt[-1, :, :5] = 255
    raw = tgt.to(torch.uint8).clone()
    raw[:, 10, ::3] = 200          # stray bytes: cleaned to class 0
    cleaned = KR.clean_mask_k(raw, K, 255)
    kp = kp_of(K)
    for tag, t_dev, t_ref, tt in (("i64", tgt.to(DEV), tgt, "long long"),
                                  ("u8", raw.to(DEV), cleaned, "unsigned char")):
        with ua.ops.record_launches() as rec:
            preds, counts = ua.ops.argmax_dice_counts(lg.to(DEV), t_dev)
        launched(rec.names, f"argmax_countsk_kernel<{kp}, {tt}>")
        assert preds.dtype == torch.uint8 and torch.equal(preds.cpu().long(), pred), tag
        m = O.segmentation_metrics([pred.numpy()], [t_ref.numpy()], num_classes=K)
        assert counts.shape == (K, 3) and counts.dtype == torch.int64
        c = counts.cpu().numpy()
        assert c[:, 0].tolist() == m["intersections"].tolist(), tag
        assert (c[:, 1] - c[:, 0]).tolist() == m["false_positives"].tolist(), tag
        assert (c[:, 2] - c[:, 0]).tolist() == m["false_negatives"].tolist(), tag
    with ua.ops.record_launches() as rec:
        assert torch.equal(ua.ops.argmax_classes(lg.to(DEV)).cpu().long(), pred)
    launched(rec.names, f"argmax_countsk_kernel<{kp}, long long>")
    none, only = ua.ops.argmax_dice_counts(lg.to(DEV), tgt.to(DEV), want_preds=False)
    assert none is None and torch.equal(only, ua.ops.argmax_dice_counts(lg.to(DEV), tgt.to(DEV))[1])
    # confusion: at network size, up- and down-scaled, and one out-of-range size (zero counts)
    with ua.ops.record_launches() as rec:
        cm = ua.ops.eval_confusion(lg.to(DEV), tgt.to(DEV))
    launched(rec.names, "eval_confusionk_kernel<")
    want = np.stack([KR.confusion(p, t, K) for p, t in zip(pred.numpy(), tgt.numpy())])
    assert cm.shape == (N, K, K) and np.array_equal(cm.cpu().numpy(), want)
    for dims in ([(66, 141), (20, 31), (33, 47)], [(500, 375), (0, 47), (7, 200)],
                 [(16385, 3), (33, 47), (100, 20)]):
        cm = ua.ops.eval_confusion(lg.to(DEV), tgt.to(DEV),
                                   torch.tensor(dims, dtype=torch.int64, device=DEV))
        want = KR.resized_confusion(pred.numpy(), tgt.numpy(), dims, K)
        assert np.array_equal(cm.cpu().numpy(), want), dims
    met = ua.SegmentationMetrics(num_classes=K)
    met.update_from_logits(lg.to(DEV), tgt.to(DEV), torch.tensor([(33, 47)] * N))
    m = O.segmentation_metrics([pred.numpy()], [tgt.numpy()], num_classes=K)
    assert met.total_pixels == m["total_pixels"] and met.correct_pixels == m["correct_pixels"]
    assert met.compute_pixel_accuracy() == m["pixel_accuracy"]
    assert np.array_equal(met.confusion_matrix, want_sum(pred, tgt, K))


def want_sum(pred, tgt, K):
    return sum(KR.confusion(p, t, K) for p, t in zip(pred.numpy(), tgt.numpy()))


# --------------------------------------------------------------------------- whole model
def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def sample_idx(numel, k=64, seed=5):
    rng = np.random.Generator(np.random.PCG64(seed + numel))
    return rng.integers(0, numel, size=min(k, numel))


_REF = {}
STEP_LOSS_TOL = (2e-4, 2e-3, 5e-2)     # tests/test_net_gpu.py::run_golden, steps 0 / 1 / 2


def model_reference(clip):
    """The float64 run of the oracle with a 5-class head, computed once per variant and shared
    (read-only) by the operand modes."""
    if clip not in _REF:
        clip_dim = 32 if clip else None
        sd = KR.state_dict_k(31, 5, clip_dim=clip_dim)
        img, tgt = KR.batch_k(9, 1, 64, 64, 5)
        feats = None
        if clip:
            feats = torch.randn(1, clip_dim, 2, 2, generator=torch.Generator().manual_seed(4))
        masks = [O.draw_dropout_masks(50 + s, 1) for s in range(3)]
        ref = KR.train_steps64(sd, img, tgt, masks, clip=feats)
        # the oracle with the bf16 pipeline's rounding points, in fp32: what sizes the bf16 bounds
        osd = O.leaf_state_dict(sd)
        lem = O.unet_forward(osd, img, masks[0], clip_features=feats, bf16_storage=True)
        lossem = F.cross_entropy(lem, tgt, weight=KR.class_weights_k(tgt, 255, 5, torch.float32),
                                 ignore_index=255) + O.dice_loss(lem, tgt)
        lossem.backward()
        ref["emulation"] = (lem.detach(), lossem.item(), {k: v.grad for k, v in osd.items()})
        _REF[clip] = (sd, img, tgt, feats, masks, ref)
    return _REF[clip]


@pytest.mark.parametrize("mode", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("clip", [False, True], ids=["unet", "clipunet"])
def test_model_with_5_classes_against_the_float64_oracle(ua, clip, mode):
    """Logits, loss and every parameter gradient of one step and the parameters after three
    FusedSGD steps, at the bounds tests/test_net_gpu.py applies at 64 x 64.
    fp32 and bf16x3, those of its golden run: logits 1e-4, gradient norms 5e-3, sampled gradients
    1e-2 with its outlier rule, the first update's length 5e-3 per tensor, the losses of the
    three steps 2e-4 / 2e-3 / 5e-2 of the float64 trajectory.
    bf16: that file's only bf16 bounds (test_bf16_matmul_mode_tracks_fp32: logits rms below 0.1,
    loss 1e-2, gradient cosine above 0.9) were measured at 256 x 256; at 64 x 64 the oracle's own
    bf16 evaluation does not meet the cosine (tests/test_bf16_gpu.py explains why: the
    1/32-resolution layers normalise over four pixels).  So bf16 is held as
    test_bf16_pipeline_vs_oracle_with_the_same_rounding_points holds it: no further from the
    exact result than the oracle evaluated with the same rounding points - logits rms 1.5 x + 1e-3,
    loss 1.5 x + 5e-3, gradient 1 - cos 1.3 x + 1e-2.
    Parameters after three steps.  That test holds no parameter bound past the first update: the
    trajectory is chaotic (its comment: the reference's own fp32 run leaves its fp64 run by 1.9e-2
    of the loss at step 2).  Measured here, as the relative error of the whole three-step update
    against the float64 trajectory: the fp32 oracle on the CPU 3e-5 / 9e-3 / 0.12 after one / two /
    three steps, the HIP fp32 step 0.45 after three, with every step-0 figure above held.  So the
    figure is printed, and what is held is what does not depend on the trajectory: the three
    FusedSGD steps on the K-class parameter set (the 5 x 32 head in the flat arena) equal the
    oracle's Nesterov recurrence in float64 on the gradients of those steps, to the 1e-6 of
    max |p| that tests/test_kernels_gpu.py::test_sgd_golden holds the kernel to."""
    sd, img, tgt, feats, masks, ref = model_reference(clip)
    l64, g64 = ref["logits"], ref["grads"]
    model = ua.CLIPUNet(with_clip_features=True, clip_dim=32, num_classes=5) if clip \
        else ua.UNet(num_classes=5)
    model.load_state_dict(sd)
    model = model.to(DEV).train()
    model.matmul_precision = mode
    imgd, tgtd = img.to(DEV), tgt.to(DEV)
    extra = (feats.to(DEV),) if clip else ()
    lossf = ua.SimpleLoss()
    opt = ua.create_optimizer(model)
    figures, bad, losses, step_grads = {}, [], [], []
    live = [k for k in g64 if g64[k].norm().item() >= 1e-4]   # (not: conv biases under InstanceNorm)
    for s in range(3):
        model.dropout_mask_override = masks[s]
        opt.zero_grad()
        with ua.ops.record_launches() as rec:
            logits = model(imgd, *extra)
            loss = lossf(logits, tgtd)
            loss.backward()
        losses.append(loss.item())
        step_grads.append([p.grad.detach().cpu().double().clone() for p in model.parameters()])
        if s == 0:
            names = " ".join(rec.names)
            for kernel in ("headk_fwd_kernel", "headk_bwd_kernel",
                           "lossk_reduce_kernel<8, long long>", "lossk_finalize_kernel",
                           "lossk_grad_kernel<8, long long>"):
                assert kernel in names, kernel
            assert logits.shape == (1, 5, 64, 64) and lossf.last_terms.numel() == 8
            figures["logits"] = relerr(logits, l64)
            ga = torch.cat([p.grad.reshape(-1) for _, p in model.named_parameters()]).double().cpu()
            gb = torch.cat([g64[k].reshape(-1) for k, _ in model.named_parameters()])
            figures["gradient cosine"] = (ga @ gb / (ga.norm() * gb.norm())).item()
            d = logits.detach().cpu().double() - l64
            figures["logits rms"] = (d.norm() / l64.norm()).item()
            if mode != "bf16":
                for k, p in model.named_parameters():
                    gk, gr = p.grad.reshape(-1).cpu().double(), g64[k].reshape(-1)
                    ref_norm = gr.norm().item()
                    if k not in live:
                        if gk.norm().item() >= 1e-3:
                            bad.append(f"{k}: |grad| should be ~0")
                        continue
                    if abs(gk.norm().item() - ref_norm) > 5e-3 * ref_norm:
                        bad.append(f"{k}: grad norm {gk.norm().item()} vs {ref_norm}")
                    idx = torch.from_numpy(sample_idx(gk.numel()))
                    err = (gk[idx] - gr[idx]).abs()
                    tol = 1e-2 * max(gr[idx].abs().max().item(), ref_norm / gk.numel() ** 0.5)
                    n_out = int((err > tol).sum().item())
                    if n_out > 3 + 0.01 * err.numel() or err.max().item() > 5 * tol:
                        bad.append(f"{k}: {n_out} of {err.numel()} sampled grads beyond tol")
        opt.step()
        if s == 0 and mode != "bf16":
            for k, p in model.named_parameters():
                if k in live:
                    dp = (p.detach().cpu().double() - sd[k].double()).norm().item()
                    ref_d = (ref["after"][0][k] - sd[k].double()).norm().item()
                    if abs(dp - ref_d) > 5e-3 * ref_d + 1e-7:
                        bad.append(f"{k}: first update |dp| {dp} vs {ref_d}")
    figures["losses"] = [abs(a - b) / abs(b) for a, b in zip(losses, ref["losses"])]
    num = den = 0.0
    for k, p in model.named_parameters():
        if k in live:
            num += ((p.detach().cpu().double() - ref["after"][2][k]) ** 2).sum().item()
            den += ((ref["after"][2][k] - sd[k].double()) ** 2).sum().item()
    figures["3-step update"] = (num / den) ** 0.5
    hyper = opt.param_groups[0]
    p64 = [sd[k].double().clone() for k, _ in model.named_parameters()]
    bufs = [None] * len(p64)
    for grads in step_grads:
        O.sgd_nesterov_(p64, grads, bufs, hyper["lr"], hyper["momentum"], hyper["weight_decay"])
    figures["sgd recurrence"] = max(
        ((p.detach().cpu().double() - q).abs().max() / q.abs().max()).item()
        for p, q in zip(model.parameters(), p64))
    show("MODELK", f"{'clipunet' if clip else 'unet'}-{mode}", **figures)
    if mode == "bf16":
        lem, lossem, gem = ref["emulation"]
        gm = torch.cat([gem[k].reshape(-1) for k, _ in model.named_parameters()]).double()
        e_emu = ((lem.double() - l64).norm() / l64.norm()).item()
        loss_emu = abs(lossem - ref["losses"][0]) / abs(ref["losses"][0])
        d_emu = 1.0 - (gm @ gb / (gm.norm() * gb.norm())).item()
        print("emulation: logits rms", e_emu, "loss", loss_emu, "1 - cos", d_emu)
        held = [("logits rms", figures["logits rms"] <= 1.5 * e_emu + 1e-3),
                ("loss", figures["losses"][0] <= 1.5 * loss_emu + 5e-3),
                ("gradient cosine", 1.0 - figures["gradient cosine"] <= 1.3 * d_emu + 1e-2)]
    else:
        held = [("logits", figures["logits"] <= 1e-4)]
        held += [(f"loss of step {s}", figures["losses"][s] <= STEP_LOSS_TOL[s]) for s in range(3)]
    held.append(("sgd recurrence", figures["sgd recurrence"] <= 1e-6))
    bad += [what for what, ok in held if not ok]
    assert not bad, f"{bad} {figures}"


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_graph_captured_5_class_step_equals_the_eager_one(ua, mode):
    sd = KR.state_dict_k(23, 5)
    img, tgt = KR.batch_k(6, 2, 64, 64, 5)
    masks = [m.to(DEV) if m is not None else None for m in O.draw_dropout_masks(5, 2)]
    outs = []
    for graphed in (False, True):
        model = ua.UNet(num_classes=5)
        model.load_state_dict(sd)
        model = model.to(DEV).train()
        model.matmul_precision = mode
        model.dropout_mask_override = masks
        opt = ua.create_optimizer(model)
        lossf = ua.SimpleLoss()
        a = (img.to(DEV), tgt.to(DEV))
        if graphed:
            step = ua.GraphedTrainStep(model, opt, lossf, *a)
        else:
            def step(x, y, model=model, opt=opt, lossf=lossf):
                return ua.train_step(model, opt, lossf, x, y)
        losses = [step(*a).item() for _ in range(3)]
        torch.cuda.synchronize()
        arena, _ = model.flat_parameters()
        outs.append((losses, arena.detach().cpu().clone()))
        del model, opt
    assert outs[0][0] == outs[1][0], f"losses differ: {outs[0][0]} vs {outs[1][0]}"
    assert torch.equal(outs[0][1], outs[1][1]), "parameters differ after three steps"


def _same(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def test_validate_and_evaluate_model_with_5_classes(ua):
    """A two-batch loader: validate's scores and evaluate_model's numbers against the oracle's
    metrics on torch.argmax of the same logits - integers exact, floats equal as in
    tests/test_eval_gpu.py (the same integers through the same formulas)."""
    K = 5
    model = ua.UNet(num_classes=K)
    model.load_state_dict(KR.state_dict_k(7, K))
    model = model.to(DEV).eval()
    img, tgt = KR.batch_k(3, 4, 64, 64, K)
    dims = [(64, 64), (100, 150), (40, 50), (82, 94)]
    loader = [{"image": img[i:i + 2], "mask": tgt[i:i + 2],
               "original_dims": torch.tensor(dims[i:i + 2], dtype=torch.int64)} for i in (0, 2)]
    with torch.no_grad():
        logits = [model(b["image"].to(DEV)).cpu() for b in loader]
    for lg in logits:      # (a near-tie would make torch.argmax on the host a coin toss)
        assert KR.top2_gap(lg) > 0
    preds = [lg.argmax(1).numpy() for lg in logits]
    # evaluate_model: every image at its original size
    want = sum(KR.resized_confusion(p, b["mask"].numpy(), b["original_dims"].tolist(), K).sum(0)
               for p, b in zip(preds, loader))
    res = ua.evaluate.evaluate_model(model, loader, DEV)
    assert np.array_equal(res["confusion_matrix"], want)
    resized = [([p[KR.nearest_index(64, h)][:, KR.nearest_index(64, w)]],
                [t[KR.nearest_index(64, h)][:, KR.nearest_index(64, w)]])
               for pb, b in zip(preds, loader)
               for p, t, (h, w) in zip(pb, b["mask"].numpy(), b["original_dims"].tolist())]
    m = O.segmentation_metrics([r[0] for r in resized], [r[1] for r in resized], num_classes=K)
    assert _same(res["pixel_accuracy"], m["pixel_accuracy"]) and _same(res["mean_iou"], m["mean_iou"])
    for c in range(K):
        assert _same(res[f"class_{c}"]["dice"], float(m["dice"][c]))
        assert _same(res[f"class_{c}"]["iou"], float(m["iou"][c]))
    fg = [d for d in m["dice"][1:] if not np.isnan(d)]
    assert _same(res["mean_foreground_dice"], float(np.mean(fg)))
    # validate: per-batch Dice of the argmax maps, averaged over the batches, and the mean loss
    vloss, scores = ua.validate(model, loader, ua.SimpleLoss(), DEV)
    per = []
    for p, b in zip(preds, loader):
        t = b["mask"].numpy()
        valid = t != 255
        row = []
        for c in range(K):
            pc, tc = (p == c) & valid, (t == c) & valid
            inter, union = float((pc & tc).sum()), float(pc.sum() + tc.sum())
            row.append(2.0 * inter / (union + 1e-5) if union > 0 else 1.0)
        per.append(row)
    d = [(per[0][c] + per[1][c]) / 2 for c in range(K)]
    assert [scores[f"class_{c}"] for c in range(K)] == pytest.approx(d, rel=1e-12)
    assert scores["mean_foreground"] == pytest.approx(sum(d[1:]) / (K - 1), rel=1e-12)
    ref = np.mean([KR.simple_loss_k(lg, b["mask"]).loss.item() for lg, b in zip(logits, loader)])
    assert abs(vloss - ref) <= 2e-6 * abs(ref) * 4, (vloss, ref)
    maps = ua.predict_masks(model, loader[0]["image"].to(DEV))
    assert torch.equal(maps.cpu().long(), torch.from_numpy(preds[0]))
