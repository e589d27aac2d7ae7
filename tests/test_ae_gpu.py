"""GPU (-m gpu): the autoencoder pretraining step on the MI355X - the recon head, MSE and Adam
kernels against fp64 restatements on the same operands, the whole network against the
reference's own autoencoder (tests/golden/ae64.npz), bf16, batch split, determinism, graph
capture and the pretrain -> transfer loop."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import importlib.util
import os

from oracle import unet_ref as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
SLOPE = 0.01
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location(
        "make_golden_ae", os.path.join(ROOT, "tests", "tools", "make_golden_ae.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def conv3x3_f64(a_nchw, w, b=None):
    """3x3 / pad 1 convolution in fp64 on the device as nine shifted contractions."""
    N, C, H, W = a_nchw.shape
    ap = F.pad(a_nchw, (1, 1, 1, 1))
    out = None
    for ky in range(3):
        for kx in range(3):
            t = torch.einsum("nchw,kc->nkhw", ap[:, :, ky:ky + H, kx:kx + W], w[:, :, ky, kx])
            out = t if out is None else out + t
    if b is not None:
        out = out + b.view(1, -1, 1, 1)
    return out


def _operand(ua, N, H, W, fused, b16, seed):
    """(ops.Act source, fp64 NCHW activated operand) of a 32-channel last decoder layer."""
    y = (rnd(N, H, W, 32, seed=seed) * 1.5 + 0.3).to(DEV)
    if b16:
        y = y.bfloat16()
    yf = y.double()
    if not fused:
        a = F.leaky_relu(yf, SLOPE)
        src = ua.ops.Act(a.to(y.dtype).contiguous())
        return src, src.x.double().permute(0, 3, 1, 2)
    al = (rnd(N, 32, seed=seed + 1) * 0.5 + 1.0)
    be = rnd(N, 32, seed=seed + 2) * 0.7
    drop = torch.rand(N, 32, generator=torch.Generator().manual_seed(seed + 3)) < 0.15
    al, be = torch.where(drop, 0.0, al).to(DEV), torch.where(drop, 0.0, be).to(DEV)
    a = F.leaky_relu(yf * al.double()[:, None, None, :] + be.double()[:, None, None, :], SLOPE)
    return ua.ops.Act(y, al.contiguous(), be.contiguous()), a.permute(0, 3, 1, 2)


HEAD_CASES = [(2, 13, 37), (1, 8, 32), (3, 33, 70), (8, 512, 512)]


@pytest.mark.parametrize("case", HEAD_CASES)
@pytest.mark.parametrize("mode", ["fused", "unfused", "bf16"])
def test_recon_head_forward_and_backward_vs_fp64(ua, case, mode):
    N, H, W = case
    fused, b16 = mode != "unfused", mode == "bf16"
    src, a64 = _operand(ua, N, H, W, fused, b16, seed=11)
    w = (rnd(3, 32, 3, 3, seed=2) * 0.1).to(DEV)
    b = (rnd(3, seed=3) * 0.1).to(DEV)
    out = ua.ops.recon3x3_fwd(src, SLOPE, w, b)
    a64 = a64.detach().requires_grad_(True)
    w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = torch.sigmoid(conv3x3_f64(a64, w64, b64))
    assert out.shape == (N, 3, H, W) and out.dtype == torch.float32
    e = (out.double() - ref.detach()).abs().max().item()
    assert e <= 1e-5, f"head forward abs err {e:.3e}"
    dout = (rnd(N, 3, H, W, seed=4) * 1e-3).to(DEV)
    dw, db = torch.empty(3, 32, 3, 3, device=DEV), torch.empty(3, device=DEV)
    da = ua.ops.recon3x3_bwd(src, SLOPE, dout, out, w, dw, db)
    # fp64 backward through the kernel's own sigmoid output (dz formed from `out`)
    ref.backward(dout.double())
    assert da.dtype == src.x.dtype and da.shape == (N, H, W, 32)
    e_da = relerr(da.permute(0, 3, 1, 2), a64.grad)
    assert e_da <= (4e-3 if b16 else 1e-4), f"da rel err {e_da:.3e}"
    assert relerr(dw, w64.grad) <= 1e-4, relerr(dw, w64.grad)
    assert relerr(db, b64.grad) <= 1e-4, relerr(db, b64.grad)
    if N * H * W < 1 << 16:     # bit-reproducible
        dw2, db2 = torch.empty_like(dw), torch.empty_like(db)
        da2 = ua.ops.recon3x3_bwd(src, SLOPE, dout, out, w, dw2, db2)
        assert torch.equal(da, da2) and torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.parametrize("case", [(2, 64, 64), (1, 40, 96), (8, 512, 512)])
@pytest.mark.parametrize("b16", [False, True])
def test_recon_head_backward_emits_next_norm_reductions(ua, case, b16):
    """With NextNorm the head's backward also sums gz and gz * xhat per workgroup: da keeps its
    bits, and the summaries drive the InstanceNorm backward to the reduction pass's results."""
    N, H, W = case
    C = 32
    y = (rnd(N, C, H, W, seed=30) * 1.5 + 0.3).permute(0, 2, 3, 1).contiguous().to(DEV)
    if b16:
        y = y.bfloat16()
    gamma, beta = (rnd(C, seed=31) * 0.2 + 1.0).to(DEV), (rnd(C, seed=32) * 0.2).to(DEV)
    st = ua.ops.instnorm_stats(y.float(), gamma, beta, 1e-5).clone() if b16 else \
        ua.ops.instnorm_stats(y, gamma, beta, 1e-5).clone()
    mask = ((torch.rand(N, C, generator=torch.Generator().manual_seed(33)) < 0.8).float()
            / 0.8).to(DEV)
    st[2] *= mask
    st[3] *= mask
    x = ua.ops.Act(y, st[2].contiguous(), st[3].contiguous())
    w = (rnd(3, C, 3, 3, seed=6) * 0.1).to(DEV)
    b = (rnd(3, seed=7) * 0.1).to(DEV)
    out = ua.ops.recon3x3_fwd(x, SLOPE, w, b)
    dout = (rnd(N, 3, H, W, seed=5) * 1e-2).to(DEV)
    dw0, db0, dw1, db1 = (torch.empty(3, C, 3, 3, device=DEV), torch.empty(3, device=DEV),
                          torch.empty(3, C, 3, 3, device=DEV), torch.empty(3, device=DEV))
    ref = ua.ops.recon3x3_bwd(x, SLOPE, dout, out, w, dw0, db0)
    nn_ = ua.ops.NextNorm(y, st, gamma, beta, mask, SLOPE)
    g = ua.ops.recon3x3_bwd(x, SLOPE, dout, out, w, dw1, db1, nxt=nn_)
    assert torch.equal(g, ref)
    assert torch.equal(dw1, dw0) and torch.equal(db1, db0)
    assert nn_.tiles > 0
    outs = []
    for partials in ((nn_.partial, nn_.tiles), None):
        dg, dbt, dbias = (torch.empty(C, device=DEV) for _ in range(3))
        dy = ua.ops.instnorm_lrelu_drop_bwd(g.clone(), y, st[0], st[1], gamma, beta, mask, SLOPE,
                                            dg, dbt, dbias, partials=partials)
        outs.append((dy, dg, dbt))
    for a, r, what in zip(outs[0], outs[1], ("dy", "dgamma", "dbeta")):
        e = relerr(a.float(), r.float())
        assert e <= (1e-2 if b16 else 2e-5), f"{what}: {e:.3e}"


@pytest.mark.parametrize("shape", [(2, 3, 13, 37), (8, 3, 512, 512)])
def test_mse_loss_kernels(ua, shape):
    N, C, H, W = shape
    out = torch.rand(N, C, H, W, generator=torch.Generator().manual_seed(1)).to(DEV)
    u8 = torch.randint(0, 256, (N, H, W, C), generator=torch.Generator().manual_seed(2),
                       dtype=torch.uint8)
    # the dataset's fp32 division, on the CPU as the reference's Dataset does it
    t = (u8.permute(0, 3, 1, 2).float().contiguous() / 255.0).to(DEV)
    u8 = u8.to(DEV)
    loss, per = ua.ops.mse_loss_fwd(out, t)
    loss8, per8 = ua.ops.mse_loss_fwd(out, u8, target_u8=True)
    assert torch.equal(loss, loss8) and torch.equal(per, per8)
    d = out.double() - t.double()
    ref_per = (d * d).sum(dim=(1, 2, 3))
    assert relerr(per, ref_per) <= 1e-6
    assert abs(loss.item() - ref_per.sum().item() / d.numel()) <= 1e-6 * loss.item()
    up = torch.tensor(0.75, device=DEV)
    g = ua.ops.mse_loss_grad(out, t, up)
    g8 = ua.ops.mse_loss_grad(out, u8, up, target_u8=True)
    assert torch.equal(g, g8)
    assert relerr(g, 0.75 * 2 * d / d.numel()) <= 1e-6
    g1 = ua.ops.mse_loss_grad(out, t)
    assert relerr(g1, 2 * d / d.numel()) <= 1e-6
    # the module against nn.MSELoss, forward and backward
    o = out.clone().requires_grad_(True)
    l_ = ua.MSELoss()(o, t)
    l_.backward()
    o2 = out.double().clone().requires_grad_(True)
    r = torch.nn.MSELoss()(o2, t.double())
    r.backward()
    assert abs(l_.item() - r.item()) <= 1e-6 * r.item()
    assert relerr(o.grad, o2.grad) <= 1e-6
    o3 = out.clone().requires_grad_(True)
    l8 = ua.MSELoss(target_layout="nhwc_u8")(o3, u8)
    assert torch.equal(l8.detach(), l_.detach())


def _arena_model(ua, seed):
    torch.manual_seed(seed)
    model = ua.Autoencoder().to(DEV)
    arena, garena = model.flat_parameters()
    params = list(model.parameters())
    for p, off in zip(params, model._offsets):
        p.grad = garena[off:off + p.numel()].view_as(p)
    return model, params, garena


def test_adam_over_the_arena_and_a_foreign_tensor_vs_torch(ua):
    k, lr, wd = 5, 1e-3, 1e-5
    model, params, garena = _arena_model(ua, 0)
    with torch.no_grad():
        for p in params:     # |p| ~ 1e-3: its fp32 ulp stays far below the 1e-5 * lr * k bound
            p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(p.numel())) * 1e-3)
    odd = torch.nn.Parameter(
        (torch.randn(1001, generator=torch.Generator().manual_seed(9)) * 1e-3).to(DEV))
    opt = ua.FusedAdam(params, lr=lr, weight_decay=wd, model=model)
    opt_odd = ua.FusedAdam([odd], lr=lr, weight_decay=wd)
    cpu = [torch.nn.Parameter(p.detach().cpu().clone()) for p in params]
    cpu_odd = torch.nn.Parameter(odd.detach().cpu().clone())
    ref = torch.optim.Adam(cpu, lr=lr, weight_decay=wd, foreach=False)
    ref_odd = torch.optim.Adam([cpu_odd], lr=lr, weight_decay=wd, foreach=False)
    gen = torch.Generator().manual_seed(3)
    for s in range(k):
        g = torch.randn(garena.numel(), generator=gen)
        garena.copy_(g.to(DEV))
        for c, p in zip(cpu, params):
            c.grad = p.grad.detach().cpu().clone()
        go = torch.randn(1001, generator=gen)
        odd.grad = go.to(DEV)
        cpu_odd.grad = go.clone()
        assert opt._flat_ready()
        opt.step()
        opt_odd.step()
        ref.step()
        ref_odd.step()
    tol = 1e-5 * lr * k
    for c, p in zip(cpu + [cpu_odd], params + [odd]):
        assert (p.detach().cpu() - c.detach()).abs().max().item() <= tol
    for o, r, ps, cs in ((opt, ref, params, cpu), (opt_odd, ref_odd, [odd], [cpu_odd])):
        for p, c in zip(ps, cs):
            for key in ("exp_avg", "exp_avg_sq"):
                a, b = o.state[p][key].cpu(), r.state[c][key]
                assert (a - b).abs().max().item() <= 1e-6 * b.abs().max().item() + 1e-30
    # state_dict both ways: FusedAdam -> torch.optim.Adam -> FusedAdam, one more step each
    sd = opt.state_dict()
    assert float(sd["state"][0]["step"]) == k
    back = torch.optim.Adam([torch.nn.Parameter(p.detach().cpu().clone()) for p in params],
                            lr=lr, weight_decay=wd, foreach=False)
    back.load_state_dict(sd)
    model2, params2, garena2 = _arena_model(ua, 1)
    with torch.no_grad():
        for p2, p in zip(params2, params):
            p2.copy_(p)
    opt2 = ua.FusedAdam(params2, lr=lr, weight_decay=wd, model=model2)
    opt2.load_state_dict(back.state_dict())
    g = torch.randn(garena.numel(), generator=gen)
    garena2.copy_(g.to(DEV))
    garena.copy_(g.to(DEV))
    for c, p in zip(back.param_groups[0]["params"], params):
        c.grad = p.grad.detach().cpu().clone()
    opt.step()
    opt2.step()
    back.step()
    for p, p2, c in zip(params, params2, back.param_groups[0]["params"]):
        assert torch.equal(p, p2)
        assert (p.detach().cpu() - c.detach()).abs().max().item() <= 1e-5 * lr * 2


def test_adam_grad_scale_equals_halved_gradients(ua):
    outs = []
    for scale in (0.5, 1.0):
        model, params, garena = _arena_model(ua, 0)
        g = torch.randn(garena.numel(), generator=torch.Generator().manual_seed(4)).to(DEV)
        opt = ua.FusedAdam(params, lr=1e-3, weight_decay=1e-5, model=model)
        opt.grad_scale = scale
        for _ in range(3):
            garena.copy_(g if scale == 0.5 else g * 0.5)
            opt.step()
        outs.append(model.flat_parameters()[0].clone())
    assert torch.equal(outs[0], outs[1])


def _golden_model(ua, g, slope, fused=True):
    kw = {"inplace": True} if slope is None else {"negative_slope": slope, "inplace": True}
    model = ua.Autoencoder(encoder_dropout_rates=[0.0, 0.0, 0.05, 0.1, 0.15, 0.15],
                           decoder_dropout_rates=[0.15, 0.1, 0.1, 0.05, 0.0], nonlin_kwargs=kw)
    model.load_state_dict(_recorder().ae_state_dict())
    model = model.to(DEV)
    model.fused_pipeline = fused
    return model


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("slope", [None, 1.0])
def test_ae64_golden(ua, golden, fused, slope):
    """The whole autoencoder against the reference's (ae64.npz): eval and train outputs, 3 Adam +
    cosine steps (loss, parameter deltas, Adam state); at slope 1 every sampled gradient entry."""
    g = golden("ae64")
    tag = "" if slope is None else "_s1"
    model = _golden_model(ua, g, slope, fused)
    img = torch.from_numpy(g["image_u8"]).to(DEV).permute(0, 3, 1, 2).float().contiguous() / 255.0
    model.eval()
    with torch.no_grad():
        out = model(img)
    assert relerr(out, torch.from_numpy(g[f"eval_out{tag}"])) <= 1e-4
    model.train()
    opt = ua.ae.create_optimizer(model)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=int(g["t_max"]), eta_min=1e-6)
    lossf = ua.ae.get_loss_function()
    names = [str(k) for k in g["param_names"]]
    p0 = {k: p.detach().clone() for k, p in model.named_parameters()}
    nmask = len([k for k in g.files if k.startswith(f"mask{tag}_0_")])
    for s in range(int(g["steps"])):
        model.dropout_mask_override = [torch.from_numpy(g[f"mask{tag}_{s}_{j}"]) for j in range(nmask)]
        assert opt.param_groups[0]["lr"] == float(g[f"lr{tag}_{s}"])
        opt.zero_grad()
        out = model(img)
        loss = lossf(out, img)
        loss.backward()
        ref_loss = float(g[f"loss{tag}_{s}"])
        # later steps compound tie flips of the default slope through the Adam normalisation
        tol = (2e-4, 2e-3, 5e-2)[s]
        assert abs(loss.item() - ref_loss) <= tol * ref_loss, (s, loss.item(), ref_loss)
        if s == 0:
            assert relerr(out, torch.from_numpy(g[f"train_out{tag}"])) <= 1e-4
            for i, (k, p) in enumerate(model.named_parameters()):
                assert k == names[i]
                gn = float(g[f"gnorm{tag}_{i}"])
                got = p.grad.double().norm().item()
                if gn < 1e-4:     # conv biases under InstanceNorm: exact 0 up to rounding
                    assert got < 1e-3, k
                    continue
                # default slope: LeakyReLU tie flips (the bound test_net_gpu uses); slope 1: tight
                assert abs(got - gn) <= (5e-3 if slope is None else 1e-3) * gn, (k, got, gn)
                if slope == 1.0:    # tie-free: every sampled entry to 1e-4 of the tensor's max
                    gk = p.grad.detach().reshape(-1).cpu()
                    idx = torch.from_numpy(_recorder().sample_idx(gk.numel(), k=256))
                    ref = torch.from_numpy(g[f"gsamp{tag}_{i}"])
                    e = (gk[idx] - ref).abs().max().item()
                    assert e <= 1e-4 * gk.abs().max().item() + 1e-12, (k, e)
        opt.step()
        sched.step()
        for i, (k, p) in enumerate(model.named_parameters()):
            if float(g[f"gnorm{tag}_{i}"]) < 1e-4:
                continue   # Adam normalises the rounding noise of a ~0 gradient to full-size steps
            dn = float(g[f"dnorm{tag}_{s}_{i}"])
            d = (p.detach() - p0[k]).double().norm().item()
            assert abs(d - dn) <= (5e-3, 2e-2, 5e-2)[s] * dn, (s, k, d, dn)
    assert opt._steps == float(g[f"adam_step{tag}"])
    # the Adam state after step 3 (tie-free network: at the default slope the steps-2/3 gradients
    # carry the tie flips that the 5e-2 loss bound of step 3 admits)
    for i, (k, p) in enumerate(model.named_parameters()):
        if slope is None or float(g[f"gnorm{tag}_{i}"]) < 1e-4:
            continue
        for key, ref in (("exp_avg", f"mnorm{tag}_{i}"), ("exp_avg_sq", f"vnorm{tag}_{i}")):
            got = opt.state[p][key].double().norm().item()
            assert abs(got - float(g[ref])) <= 5e-2 * float(g[ref]), (k, key, got, float(g[ref]))


def _ae_step(ua, model, img, masks, opt=None):
    model.dropout_mask_override = masks
    if opt is not None:
        opt.zero_grad()
    else:
        model.zero_grad(set_to_none=True)
    out = model(img)
    loss = ua.MSELoss()(out, img)
    loss.backward()
    if opt is not None:
        opt.step()
    return out, loss


def _masks(model, n, seed):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.rand(n, m.conv.out_channels, generator=gen) >= m.drop.drop_prob).float()
            / (1 - m.drop.drop_prob)
            for blk in [b for part in model._build_plan() for b in part] for m in blk
            if m.drop is not None and m.drop.drop_prob > 0]


def _image(n, hw, seed):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 256, (n, 3, hw, hw), generator=gen).float() / 255.0).to(DEV)


def test_bf16_autoencoder_tracks_fp32(ua):
    """matmul_precision="bf16" (bf16 layer tensors) against the fp32 AE on the same weights,
    image and masks, at the bf16 UNet test's size (256x256) and with its output and loss bounds.
    The whole-network gradient cosine measured 0.877 here (0.853 at 128x128) against the
    UNet's 0.95, so it is held to 0.85 rather than the UNet's 0.9 (not investigated further:
    DESIGN.md §8); the head's own gradient, one bf16 rounding of its operand away, is held
    tightly."""
    img = _image(2, 256, 5)
    outs = {}
    for mode in ("fp32", "bf16"):
        model = ua.ae.create_model(DEV).train()
        torch.manual_seed(0)
        model.load_state_dict(_recorder().ae_state_dict())
        model.matmul_precision = mode
        out, loss = _ae_step(ua, model, img, _masks(model, 2, 6))
        gr = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).double().cpu()
        gh = model.reconstruction_output[0].weight.grad.reshape(-1).double().cpu()
        outs[mode] = (out.detach().double().cpu(), loss.item(), gr, gh)
    d = outs["bf16"][0] - outs["fp32"][0]
    e = (d.norm() / outs["fp32"][0].norm()).item()
    assert 1e-6 < e < 0.1, f"bf16 output rms rel err {e:.3e}"
    assert abs(outs["bf16"][1] - outs["fp32"][1]) < 1e-2 * abs(outs["fp32"][1])
    ga, gb = outs["bf16"][2], outs["fp32"][2]
    cos = (ga @ gb / (ga.norm() * gb.norm())).item()
    assert cos > 0.85, f"bf16 gradient cosine {cos:.3f}"
    ha, hb = outs["bf16"][3], outs["fp32"][3]
    hcos = (ha @ hb / (ha.norm() * hb.norm())).item()
    assert hcos > 0.99, f"bf16 head weight-gradient cosine {hcos:.4f}"


def test_batch_split_at_bench_size(ua):
    """An 8 x 512^2 AE step against four 2 x 512^2 steps with the same dropout masks: the MSE
    mean normalises over the batch, so the bs-8 gradient is the mean of the four bs-2 ones.
    Tie-free network (negative_slope = 1): at the default slope the two tilings' different
    summation orders flip a fraction of the LeakyReLU branches (norm-wise ~1e-3 measured here;
    test_net_gpu.test_full_size_batch_split_invariance sizes that effect for the UNet)."""
    model = ua.Autoencoder(encoder_dropout_rates=[0.0, 0.0, 0.05, 0.1, 0.15, 0.15],
                           decoder_dropout_rates=[0.15, 0.1, 0.1, 0.05, 0.0],
                           nonlin_kwargs={"negative_slope": 1.0, "inplace": True}).to(DEV).train()
    model.load_state_dict(_recorder().ae_state_dict())
    img = _image(8, 512, 7)
    masks = _masks(model, 8, 8)
    _ae_step(ua, model, img, masks)
    full = [p.grad.detach().double().clone() for p in model.parameters()]
    acc = [torch.zeros_like(g) for g in full]
    for q in range(4):
        sl = slice(2 * q, 2 * q + 2)
        _ae_step(ua, model, img[sl].contiguous(), [m[sl] for m in masks])
        for a, p in zip(acc, model.parameters()):
            a += p.grad.detach().double() / 4
    for (k, _), a, f in zip(model.named_parameters(), acc, full):
        if f.norm().item() < 1e-6 * max(x.norm().item() for x in full):
            continue           # conv biases under InstanceNorm: rounding noise of a zero gradient
        e = ((a - f).norm() / (f.norm() + 1e-30)).item()
        assert e <= 1e-4, f"{k}: batch-split gradient rel L2 {e:.3e}"


def test_two_identical_steps_are_bit_identical(ua):
    img = _image(2, 128, 9)
    res = []
    for _ in range(2):
        model = ua.ae.create_model(DEV).train()
        model.load_state_dict(_recorder().ae_state_dict())
        opt = ua.ae.create_optimizer(model)
        masks = _masks(model, 2, 10)
        _ae_step(ua, model, img, masks, opt)
        _ae_step(ua, model, img, masks, opt)
        res.append(model.flat_parameters()[0].clone())
    assert torch.equal(res[0], res[1])


def test_graphed_step_with_fused_adam_replays_eager_steps(ua):
    """GraphedTrainStep with FusedAdam: 3 replays equal 3 eager steps bit for bit, with an LR
    change between replays (the device step count and lr follow without re-capture)."""
    img = _image(2, 64, 11)
    results = []
    for graphed in (False, True):
        model = ua.ae.create_model(DEV).train()
        model.load_state_dict(_recorder().ae_state_dict())
        model.dropout_mask_override = [m.to(DEV) for m in _masks(model, 2, 12)]
        opt = ua.ae.create_optimizer(model)
        lossf = ua.ae.get_loss_function()
        step = ua.GraphedTrainStep(model, opt, lossf, img, img) if graphed else None
        losses = []
        for s in range(3):
            opt.param_groups[0]["lr"] = 1e-3 * (1.0 - 0.3 * s)
            loss = step(img, img) if graphed else ua.train_step(model, opt, lossf, img, img)
            losses.append(loss.item())
        results.append((model.flat_parameters()[0].clone(), losses, opt._steps,
                        opt._flat_m.clone(), opt._flat_v.clone()))
    (pa, la, sa, ma, va), (pb, lb, sb, mb, vb) = results
    assert sa == sb == 3
    assert la == lb
    assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb)


def test_pretrain_then_transfer(ua, tmp_path):
    """2 AE steps, ua.ae.save_checkpoint, UNet.load_pretrained_encoder(path): no missing keys, the
    encoder equals the AE's, and one frozen-encoder segmentation step runs."""
    ae = ua.ae.create_model(DEV).train()
    opt = ua.ae.create_optimizer(ae)
    lossf = ua.ae.get_loss_function()
    img = _image(2, 64, 13)
    for _ in range(2):
        ua.train_step(ae, opt, lossf, img, img)
    sched = ua.ae.create_lr_scheduler(opt, 10)
    path = ua.ae.save_checkpoint(ae, opt, sched, 0, 0.5, tmp_path, is_best=True)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert ck["best_loss"] == 0.5 and ck["config"]["out_channels"] == 3
    ae2 = ua.ae.create_model(DEV)
    opt2 = ua.ae.create_optimizer(ae2)
    start, best = ua.ae.load_checkpoint(path, ae2, opt2, device=DEV)
    assert start == 1 and best == 0.5 and opt2._steps == 2
    unet = ua.create_model(DEV)
    missing = unet.load_pretrained_encoder(path)
    assert missing == []
    for (k, a), (k2, b) in zip(ae.encoder_stages.state_dict().items(),
                               unet.encoder_stages.state_dict().items()):
        assert k == k2 and torch.equal(a, b)
    enc0 = [p.detach().clone() for p in unet.encoder_stages.parameters()]
    sgd = ua.create_optimizer(unet)
    _, tgt = O.synthetic_batch(1, 2, 64, 64)
    loss = ua.train_step(unet.train(), sgd, ua.get_loss_function(), img, tgt.to(DEV))
    assert math.isfinite(loss.item())
    assert all(torch.equal(a, p) for a, p in zip(enc0, unet.encoder_stages.parameters()))


def test_encode_and_u8_input(ua):
    model = ua.ae.create_model(DEV).eval()
    g = torch.Generator().manual_seed(14)
    u8 = torch.randint(0, 256, (2, 128, 128, 3), generator=g, dtype=torch.uint8).to(DEV)
    img = u8.permute(0, 3, 1, 2).float().contiguous() / 255.0
    with torch.no_grad():
        a = model(img)
        b = model(u8, input_layout="nhwc_u8")
    assert relerr(b, a) <= 1e-4      # the stem's normalisation vs the device's own v / 255
    z = model.encode(img)
    assert z.shape == (2, 512 * 4 * 4)


def test_validate_metrics(ua):
    model = ua.ae.create_model(DEV)
    imgs = [_image(2, 64, 20 + i) for i in range(3)]

    class DS(list):
        pass

    class Loader:
        dataset = DS([0] * 6)

        def __iter__(self):
            return iter([{"image": x, "target": x} for x in imgs])

        def __len__(self):
            return 3

    loss, m = ua.ae.validate(model, Loader(), ua.ae.get_loss_function(), DEV)
    model.eval()
    with torch.no_grad():
        outs = [model(x).double() for x in imgs]
    mse = torch.cat([((o - x.double()) ** 2).mean(dim=(1, 2, 3)) for o, x in zip(outs, imgs)])
    ref_loss = sum(((o - x.double()) ** 2).mean().item() for o, x in zip(outs, imgs)) / 3
    assert abs(loss - ref_loss) <= 1e-5 * ref_loss and m["loss"] == loss
    assert abs(m["mse"] - mse.sum().item() / 6) <= 1e-5 * m["mse"]
    assert abs(m["psnr"] - (10 * torch.log10(1 / mse)).sum().item() / 6) <= 1e-4
