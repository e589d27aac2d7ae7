"""dL/dz of the two 512 x 512 layers with 32 -> 32 channels whose gradient has several readers
(the second convolution of the first encoder stage, the first convolution of the last decoder
stage) is formed inside their weight gradient: the dy side of conv_wgrad_wino32_kernel<true>
reads g = dL/da and the raw output y, evaluates in_bwd_dz4 and stores dz over g in place
(ops.conv_in_bwd_weight_fold32) - the layers' apply launch is gone.

The fold keeps the BITS of the sequence it replaces (instnorm_lrelu_drop_bwd(partials=...) then
conv_in_bwd_weight), so every comparison is torch.equal and no bound is needed; the launch list
is asserted.

Shapes:
  operation  (2, 136, 256): the smallest shape at which tests/test_fp32_step_kernels_gpu.py
             reaches conv_wgrad_wino32_kernel<true> - 272 tiles of 8 x 32 pixels on 256
             workgroups, 16 of them with two tiles; the two images differ.
             (3, 96, 256): 288 tiles, 96 per image, 36 per eighth of the walk: the workgroups of
             the third eighth (tiles 72 .. 107) step from image 0 into image 1 - the coefficient
             rows change INSIDE a workgroup's walk, which no workgroup of the first shape does
             (its eighths of 34 tiles end on the image boundary at tile 136).
  whole step (2, 160, 256): the network takes sizes that are multiples of 32 only (five
             halvings, each decoder stage doubles exactly), so 136 rows cannot run a step;
             160 x 256 is the next size above it that can: 320 tiles, workgroups of one and of
             two tiles, the fold taken by both layers (asserted through the launch counts).
"""
import importlib.util
import os

import pytest
import torch

from oracle import unet_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _load(name):
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(ROOT, "tests", "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load("fp64_layer_refs")
DEV, SLOPE = R.DEV, R.SLOPE
WINO32 = "conv_wgrad_wino32_kernel<true>"


def tile_summaries(g, y, st, mask, tiles):
    """(S1, S2) = (sum gz, sum gz xhat) over each of `tiles` equal pixel ranges per image, as a
    data gradient's epilogue leaves them: float pairs [N, tiles, C, 2], fp64 values rounded once."""
    N, H, W, C = y.shape
    yd, gd = y.double().reshape(N, H * W, C), g.double().reshape(N, H * W, C)
    mean, rstd, al, be = (st[k].double()[:, None, :] for k in range(4))
    mk = 1.0 if mask is None else mask.double()[:, None, :]
    z = yd * al + be
    gz = gd * mk * torch.where(z > 0, 1.0, SLOPE)
    xh = (yd - mean) * rstd
    s1 = gz.reshape(N, tiles, -1, C).sum(2)
    s2 = (gz * xh).reshape(N, tiles, -1, C).sum(2)
    return torch.stack([s1, s2], -1).float().contiguous()


def count(names, what):
    return sum(what in n for n in names)


# --------------------------------------------------------------------------- operation
def _operands(ua, N, H, W, with_mask):
    al, be = R.coeffs(N, 32, 40)
    x = ua.ops.Act(R.grand((N, H, W, 32), 1), al, be)
    y, st, gamma, beta, mask = R.norm_layer(N, H, W, 32, 80)
    if not with_mask:
        mask = None
    g = R.grand((N, H, W, 32), 2)
    part = tile_summaries(g, y, st, mask, H)
    return dict(x=x, y=y, mean=st[0], rstd=st[1], gamma=gamma, beta=beta, mask=mask, g=g,
                part=part, tiles=H)


def _stored(ua, o, ci_off, cin_total):
    """the sequence the fold replaces -> (dz, dw, dgamma, dbeta, dbias), launches"""
    ops = ua.ops
    dw = torch.zeros(32, cin_total, 3, 3, device=DEV)
    dg, db, dbias = (torch.empty(32, device=DEV) for _ in range(3))
    with ops.c32_winograd_scope(True), ops.record_launches() as rec:
        dz = ops.instnorm_lrelu_drop_bwd(o["g"].clone(), o["y"], o["mean"], o["rstd"], o["gamma"],
                                         o["beta"], o["mask"], SLOPE, dg, db, dbias,
                                         partials=(o["part"], o["tiles"]))
        ops.conv_in_bwd_weight(o["x"], SLOPE, dz, dw, ci_off, 3, 1)
    return (dz, dw, dg, db, dbias), rec.names


def _folded(ua, o, ci_off, cin_total):
    ops = ua.ops
    dw = torch.zeros(32, cin_total, 3, 3, device=DEV)
    dg, db, dbias = (torch.full((32,), 7.0, device=DEV) for _ in range(3))
    g = o["g"].clone()
    with ops.c32_winograd_scope(True), ops.record_launches() as rec:
        assert ops.conv_in_bwd_weight_fold32_supported(o["x"], g)
        dz = ops.conv_in_bwd_weight_fold32(o["x"], SLOPE, g, o["y"], o["mean"], o["rstd"],
                                           o["gamma"], o["beta"], o["mask"], SLOPE,
                                           (o["part"], o["tiles"]), dw, ci_off, dg, db, dbias)
    assert dz.data_ptr() == g.data_ptr()        # dz is read back from the g buffer
    return (g, dw, dg, db, dbias), rec.names


NAMES = ("dz", "dw", "dgamma", "dbeta", "dbias")


@pytest.mark.parametrize("ci_off,cin_total", [(0, 32), (64, 96)], ids=["whole", "skip_slice"])
@pytest.mark.parametrize("with_mask", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("N,H,W", [(2, 136, 256), (3, 96, 256)])
def test_fold_equals_apply_then_wgrad(ua, N, H, W, with_mask, ci_off, cin_total):
    o = _operands(ua, N, H, W, with_mask)
    ref, names0 = _stored(ua, o, ci_off, cin_total)
    assert count(names0, WINO32) == 1 and count(names0, "in_bwd_apply") == 1, names0
    got, names = _folded(ua, o, ci_off, cin_total)
    assert count(names, "in_bwd_apply") == 0 and count(names, WINO32) == 1, names
    assert count(names, "in_bwd_finalize1") == 1, names
    assert set(names) <= set(names0), sorted(set(names) - set(names0))
    assert not torch.equal(got[0], o["g"])
    for name, a, b in zip(NAMES, got, ref):
        assert torch.equal(a, b), f"{name} differs by {(a - b).abs().max().item():.3e}"


def test_fold_is_refused_where_the_winograd_kernel_does_not_run(ua):
    """64 tiles: conv_in_bwd_weight takes the direct kernel there, and the fold says so"""
    o = _operands(ua, 2, 64, 128, True)
    with ua.ops.c32_winograd_scope(True):
        assert not ua.ops.conv_in_bwd_weight_fold32_supported(o["x"], o["g"])
        g = o["g"].clone()
        with pytest.raises(RuntimeError), ua.ops.record_launches() as rec:
            ua.ops.conv_in_bwd_weight_fold32(
                o["x"], SLOPE, g, o["y"], o["mean"], o["rstd"], o["gamma"], o["beta"], o["mask"],
                SLOPE, (o["part"], o["tiles"]), torch.zeros(32, 32, 3, 3, device=DEV), 0, None,
                None, None)
        assert rec.names == [] and torch.equal(g, o["g"])      # refused before anything ran


# --------------------------------------------------------------------------- rejection
@pytest.mark.parametrize("row", ["mean", "rstd", "gamma", "beta", "mask", "c1", "c2"])
def test_a_zeroed_coefficient_row_in_the_reference_is_seen(ua, row):
    """The comparison is not vacuous: the stored sequence with ONE coefficient row zeroed (c1 / c2
    through the summaries they are merged from) differs from the fold in dz and in dw."""
    o = _operands(ua, 2, 136, 256, True)
    got, _ = _folded(ua, o, 0, 32)
    bad = dict(o)
    if row in ("c1", "c2"):
        bad["part"] = o["part"].clone()
        bad["part"][..., 0 if row == "c1" else 1] = 0.0
    else:
        bad[row] = torch.zeros_like(o[row])
    ref, _ = _stored(ua, bad, 0, 32)
    assert not torch.equal(got[0], ref[0]), f"dz does not depend on {row}"
    assert not torch.equal(got[1], ref[1]), f"dw does not depend on {row}"


# --------------------------------------------------------------------------- whole step
STEP_H, STEP_W = 160, 256


def _model(ua, folds):
    model = ua.UNet()
    model.load_state_dict(O.fill_state_dict(7))
    model = model.to(DEV).train()
    model.dropout_mask_override = [m.to(DEV) if m is not None else None
                                   for m in O.draw_dropout_masks(5, 2)]
    model.wgrad32_folds = folds
    return model


def _eager_step(ua, folds, img, tgt):
    model = _model(ua, folds)
    lossf = ua.get_loss_function()
    with ua.ops.record_launches() as rec:
        loss = lossf(model(img), tgt)
        loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    return loss.detach().clone(), grads, rec.names


def test_whole_step_with_and_without_the_folds(ua):
    img, tgt = O.synthetic_batch(11, 2, STEP_H, STEP_W)
    img, tgt = img.to(DEV), tgt.to(DEV)
    loss1, g1, names1 = _eager_step(ua, True, img, tgt)
    loss0, g0, names0 = _eager_step(ua, False, img, tgt)
    assert count(names0, "in_bwd_apply") - count(names1, "in_bwd_apply") == 2
    assert count(names1, WINO32) == count(names0, WINO32) >= 2
    assert set(names1) == set(names0), sorted(set(names1) ^ set(names0))
    assert torch.equal(loss1, loss0)
    for k in g0:
        assert torch.equal(g1[k], g0[k]), f"{k} differs by {(g1[k] - g0[k]).abs().max().item():.3e}"


def test_graph_replayed_step_with_the_folds_equals_the_eager_one(ua):
    img, tgt = O.synthetic_batch(11, 2, STEP_H, STEP_W)
    img, tgt = img.to(DEV), tgt.to(DEV)
    outs = []
    for graphed in (False, True):
        model = _model(ua, True)
        opt = ua.create_optimizer(model)
        lossf = ua.get_loss_function()
        if graphed:
            loss = ua.GraphedTrainStep(model, opt, lossf, img, tgt)(img, tgt)
        else:
            loss = ua.train_step(model, opt, lossf, img, tgt)
        torch.cuda.synchronize()
        arena, _ = model.flat_parameters()
        outs.append((loss.detach().clone(), arena.detach().clone()))
    assert torch.equal(outs[0][0], outs[1][0]), "losses differ"
    assert torch.equal(outs[0][1], outs[1][1]), "parameters differ after the step"
