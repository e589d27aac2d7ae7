"""Two full-resolution gradients of the fp32 step are formed inside their consumers instead of
being stored, and the merge of the InstanceNorm-backward summaries keeps its loads in flight:

  * stem: dL/dz of the first layer is formed by the loader of its weight gradient
    (ops.stem_in_bwd_weight_fold) - no apply pass, no dz tensor;
  * head: dL/da of the last decoder layer is never stored; a second launch of the head's
    backward kernel forms it again on the way to that layer's dL/dz (ops.head1x1_in_bwd_fold);
  * ops.instnorm_bwd_merge_partials (in_bwd_finalize1_kernel): same sums, same order.

Every fold is held to the BITS of the sequence it replaces (torch.equal), its launch list is
asserted, and the stem's dw also to the fp64 reference of tests/tools/fp64_layer_refs.py at the
bound of the stem row of tests/test_fp32_step_kernels_gpu.py (TOL_DW = 3e-5 of max |dw|, from
test_fused_gpu.py::test_conv_in_bwd_weight).

Shapes (the smallest that take each path):
  stem   W = 128, the narrowest width of the raw-row kernel (one 128-pixel stage per image row).
         (2, 8): 16 stages, one per workgroup; (1, 8): one image; (3, 343): 1029 stages = 515
         workgroups of 2 stages, the last one with a single stage, workgroups 171 and 343
         straddling two images (the coefficient rows change inside a workgroup).
  head   (2, 8, 8): 2 tiles of 64 pixels, one summary per image - the smallest shape with the
         reductions epilogue; (2, 256, 256): 2048 tiles on 1024 workgroups, two tiles per
         workgroup, 512 summaries per image (the batched loads of the merge); (2, 6, 6): 72 pixels
         are no whole number of tiles - no epilogue, the fallback.
"""
import importlib.util
import math
import os
import re

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
TOL_DW = 3e-5     # the stem row of test_fp32_step_kernels_gpu.py


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


# --------------------------------------------------------------------------- stem
@pytest.mark.parametrize("u8", [False, True], ids=["float", "uint8"])
@pytest.mark.parametrize("with_mask", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("N,H", [(2, 8), (3, 343), (1, 8)])
def test_stem_fold_equals_apply_then_wgrad(ua, N, H, with_mask, u8):
    W, C = 128, 32
    ops = ua.ops
    if u8:
        gen = torch.Generator(device=DEV).manual_seed(1)
        img = torch.randint(0, 256, (N, H, W, 3), generator=gen, device=DEV, dtype=torch.uint8)
        x = ops.U8Image(img)
        mean, std = (torch.tensor(v, dtype=torch.double, device=DEV) for v in (x.mean, x.std))
        x64 = ((img.double() / 255.0 - mean) / std).permute(0, 3, 1, 2)
    else:
        img = R.grand((N, H, W, 3), 1)
        x = ops.Act(img)
        x64 = R.nchw64(img)
    y, st, gamma, beta, mask = R.norm_layer(N, H, W, C, 80)
    if not with_mask:
        mask = None
    g = R.grand((N, H, W, C), 2)
    partials = (tile_summaries(g, y, st, mask, H), H)

    dw0 = torch.zeros(C, 3, 3, 3, device=DEV)
    dg0, db0, dbias0 = (torch.empty(C, device=DEV) for _ in range(3))
    dz = ops.instnorm_lrelu_drop_bwd(g.clone(), y, st[0], st[1], gamma, beta, mask, SLOPE, dg0, db0,
                                     dbias0, partials=partials)
    ops.conv_in_bwd_weight(x, SLOPE, dz, dw0, 0, 3, 1)

    dw = torch.zeros(C, 3, 3, 3, device=DEV)
    dg, db, dbias = (torch.full((C,), 7.0, device=DEV) for _ in range(3))
    assert ops.stem_in_bwd_weight_fold_supported(x, g)
    with ops.record_launches() as rec:
        ops.stem_in_bwd_weight_fold(x, g, y, st[0], st[1], gamma, beta, mask, SLOPE, partials, dw,
                                    dg, db, dbias)
    assert count(rec.names, "conv_stem_wgrad_rows_kernel") == 1, rec.names
    assert count(rec.names, "in_bwd_apply") == 0 and count(rec.names, "in_bwd_finalize1") == 1, \
        rec.names
    assert torch.equal(dw, dw0), f"dw differs by {(dw - dw0).abs().max().item():.3e}"
    assert torch.equal(dg, dg0) and torch.equal(db, db0) and torch.equal(dbias, dbias0)

    dz_ref = R.ref_in_bwd(g, y, gamma, beta, mask)[0]
    m = R.metric("dw", dw, R.ref_wgrad(x64, R.nchw64(dz_ref), 1), TOL_DW)
    print(R.report([m]))
    assert not R.failures([m]), R.failures([m])


# --------------------------------------------------------------------------- head
def _head_operands(ua, N, H, W):
    nn = ua.ops.NextNorm(*R.norm_layer(N, H, W, 32, 60), SLOPE)
    al, be = (nn.st[2] * nn.mask).contiguous(), (nn.st[3] * nn.mask).contiguous()
    return nn, ua.ops.Act(nn.y, al, be), R.grand((N, 3, H, W), 2), R.grand((3, 32), 3, 0.2)


def _head_three_steps(ua, N, H, W):
    """head_bwd -> (in_bwd_finalize1 | reduction pass) -> apply: the sequence the fold replaces"""
    ops = ua.ops
    nn, x, dl, w = _head_operands(ua, N, H, W)
    dw, db = torch.empty(3, 32, device=DEV), torch.empty(3, device=DEV)
    dg, dbt, dbias = (torch.empty(32, device=DEV) for _ in range(3))
    da = ops.head1x1_in_bwd(x, SLOPE, dl, w, dw, db, nxt=nn)
    dz = ops.instnorm_lrelu_drop_bwd(da, nn.y, nn.st[0], nn.st[1], nn.gamma, nn.beta, nn.mask,
                                     SLOPE, dg, dbt, dbias,
                                     partials=(nn.partial, nn.tiles) if nn.tiles > 0 else None)
    return nn.tiles, (dz, dw, db, dg, dbt, dbias)


@pytest.mark.parametrize("N,H,W,tiles", [(2, 8, 8, 1), (2, 256, 256, 512), (2, 6, 6, 0)])
def test_head_fold_equals_the_three_step_sequence(ua, N, H, W, tiles):
    ops = ua.ops
    tiles0, ref = _head_three_steps(ua, N, H, W)
    assert tiles0 == tiles
    nn, x, dl, w = _head_operands(ua, N, H, W)
    dw, db = torch.empty(3, 32, device=DEV), torch.empty(3, device=DEV)
    dg, dbt, dbias = (torch.full((32,), 7.0, device=DEV) for _ in range(3))
    with ops.record_launches() as rec:
        dz = ops.head1x1_in_bwd_fold(x, SLOPE, dl, w, dw, db, nn, dg, dbt, dbias)
    short = [re.search(r"\w+_kernel", n).group(0) for n in rec.names]
    assert nn.tiles == tiles and nn.applied == (tiles > 0)
    if tiles > 0:
        assert short == ["head_bwd_kernel", "head_bwd_finalize_kernel", "in_bwd_finalize1_kernel",
                         "head_bwd_kernel"], rec.names
    else:       # the fallback: the head's backward as it was, then the stand-alone passes
        assert short == ["head_bwd_kernel", "head_bwd_finalize_kernel"], rec.names
        dz = ops.instnorm_lrelu_drop_bwd(dz, nn.y, nn.st[0], nn.st[1], nn.gamma, nn.beta, nn.mask,
                                         SLOPE, dg, dbt, dbias)
    for name, a, b in zip(("dz", "dw", "db", "dgamma", "dbeta", "dbias"),
                          (dz, dw, db, dg, dbt, dbias), ref):
        assert torch.equal(a, b), f"{name} differs by {(a - b).abs().max().item():.3e}"


# --------------------------------------------------------------------------- the merge
MERGE_HW = 1 << 18      # 512 x 512: 1 / HW is a power of two, so coef = sums / HW exactly


@pytest.fixture(scope="module")
def merge_cases():
    """partial[N, split, C, 2] per (C, split): signed summaries of magnitude ~1e3 whose sum per
    (image, channel, component) is ~1 - below 1e-6 of the sum of their magnitudes at 4096 - and the
    exact (math.fsum) totals."""
    cases = {}
    for C in (32, 40):
        for split in (1, 7, 8, 9, 511, 512, 513, 4096):
            gen = torch.Generator().manual_seed(1000 * C + split)
            p = torch.randn((2, split, C, 2), generator=gen, dtype=torch.double) * 1e3
            p[:, 0] -= p.sum(1) - 1.0
            p = p.float()
            flat = p.double().permute(0, 2, 3, 1).reshape(-1, split).tolist()
            exact = torch.tensor([math.fsum(r) for r in flat], dtype=torch.double).reshape(2, C, 2)
            cases[(C, split)] = (p.contiguous(), exact)
    return cases


@pytest.mark.parametrize("split", [1, 7, 8, 9, 511, 512, 513, 4096])
@pytest.mark.parametrize("C", [32, 40])
def test_merge_of_summaries_is_the_double_sum(ua, merge_cases, C, split):
    p, exact = merge_cases[(C, split)]
    pd = p.to(DEV)
    coef, sums = ua.ops.instnorm_bwd_merge_partials(pd, split, 2, MERGE_HW, C)
    coef2, sums2 = ua.ops.instnorm_bwd_merge_partials(pd, split, 2, MERGE_HW, C)
    assert torch.equal(coef, coef2) and torch.equal(sums, sums2), "two runs differ"
    for name, got, ref in (("sums", sums, exact), ("coef", coef, exact / MERGE_HW)):
        ref32 = ref.float()
        ulp = torch.nextafter(ref32.abs(), torch.full_like(ref32, float("inf"))) - ref32.abs()
        err = ((got.cpu().double() - ref).abs() / ulp.double()).max().item()
        print(f"{name}: {err:.3f} ulp")
        assert err <= 1.0, f"{name}: {err:.3f} ulp from the exact sum"


# --------------------------------------------------------------------------- whole step
def _model(ua, folds):
    model = ua.UNet()
    model.load_state_dict(O.fill_state_dict(7))
    model = model.to(DEV).train()
    model.dropout_mask_override = [m.to(DEV) if m is not None else None
                                   for m in O.draw_dropout_masks(5, 2)]
    model.fullres_folds = folds
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


# (64, 64): the head's fold alone - the stem takes its stored form at a width the raw-row kernel
# does not run; (64, 128): both folds
@pytest.mark.parametrize("H,W,fewer_applies", [(64, 64, 1), (64, 128, 2)])
def test_whole_step_with_and_without_the_folds(ua, H, W, fewer_applies):
    """Every fold keeps the bits of what it replaces (the merge keeps its order of additions), so
    the loss and every gradient of one step are equal - no bound is needed."""
    img, tgt = O.synthetic_batch(11, 2, H, W)
    img, tgt = img.to(DEV), tgt.to(DEV)
    loss1, g1, names1 = _eager_step(ua, True, img, tgt)
    loss0, g0, names0 = _eager_step(ua, False, img, tgt)
    assert count(names0, "in_bwd_apply") - count(names1, "in_bwd_apply") == fewer_applies
    assert count(names1, "head_bwd_kernel") == 2 and count(names0, "head_bwd_kernel") == 1
    assert set(names1) <= set(names0), sorted(set(names1) - set(names0))
    assert torch.equal(loss1, loss0)
    for k in g0:
        assert torch.equal(g1[k], g0[k]), f"{k} differs by {(g1[k] - g0[k]).abs().max().item():.3e}"


def test_graph_replayed_step_with_the_folds_equals_the_eager_one(ua):
    img, tgt = O.synthetic_batch(11, 2, 64, 128)
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
