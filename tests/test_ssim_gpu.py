"""GPU (-m gpu): the fused SSIM kernels on the MI355X - metrics and loss gradients against the
reference's own values (tests/golden/ssim.npz) and the fp64 restatement of tests/test_ssim_cpu.py,
the uint8 target, determinism and batch invariance, the MSE-only ReconstructionLoss, the AE
trajectory under MSE + SSIM, graph capture and the evaluation loop."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load("ssim_restatement", ["test_ssim_cpu.py"])


def _ae_recorder():
    return _load("make_golden_ae", ["tools", "make_golden_ae.py"])


def dev(a):
    return torch.from_numpy(np.asarray(a)).to(DEV).contiguous()


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def noisy_pair(shape, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(shape, generator=g)
    p = (t + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1)
    return p.to(DEV), t.to(DEV)


def test_metrics_against_the_reference(ua, golden):
    g = golden("ssim")
    for tag in [str(c) for c in g["cases"]]:
        p, t = (v.to(DEV) for v in R.case_inputs(g, tag))
        ev = ua.evaluate_reconstructions(p, t)
        ssim = ua.calculate_ssim(p, t)
        assert torch.equal(ssim, ev["ssim"])
        ref = torch.from_numpy(g[f"ssim_{tag}"]).double()
        assert (ssim.double().cpu() - ref).abs().max().item() <= 2e-5, tag
        exact = R.ssim_per_image(p.double(), t.double()).cpu()
        # measured 1.2e-6 (the fixture's own fp32 values sit up to 1.25e-5 from fp64)
        assert (ssim.double().cpu() - exact).abs().max().item() <= 5e-6, tag
        mse = torch.from_numpy(g[f"eval_mse_{tag}"]).double()
        assert ((ev["mse"].double().cpu() - mse).abs() / mse).max().item() <= 1e-6, tag
        psnr = torch.from_numpy(g[f"psnr_{tag}"]).double()
        for got in (ev["psnr"], ua.calculate_psnr(p, t)):
            assert (got.double().cpu() - psnr).abs().max().item() <= 2e-5, tag   # measured 3.8e-6
        assert torch.equal(ua.calculate_ssim(p, t, reduction="mean"), ssim.mean())
        assert torch.equal(ua.calculate_ssim(p, t, kernel_size=10, reduction="sum"), ssim.sum())


@pytest.mark.parametrize("shape", [(8, 3, 512, 512), (2, 3, 1, 1), (1, 3, 3, 200), (1, 1, 45, 33)])
def test_ssim_against_fp64(ua, shape):
    """The bench size, and sizes below the window / not tile multiples."""
    p, t = noisy_pair(shape, 3)
    _, ssim, sq = ua.ops.ssim_fwd(p, t, want_loss=False)
    exact = R.ssim_per_image(p.double(), t.double())
    assert (ssim - exact).abs().max().item() <= 1e-5
    esq = ((p.double() - t.double()) ** 2).sum(dim=(1, 2, 3))
    assert ((sq - esq).abs() / esq).max().item() <= 1e-6


# against the fixture a gradient may differ by its own error against fp64 (held to 1e-4 below, on
# the full tensor) plus the reference's fp32 error (test_ssim_cpu.REF_FP32_GRAD)
GRAD_VS_FIXTURE = 1e-4 + R.REF_FP32_GRAD


def _grad(lossf, p, t, upstream=None):
    x = p.clone().requires_grad_(True)
    loss = lossf(x, t)
    if upstream is None:
        loss.sum().backward()
    else:
        (loss * upstream).sum().backward()
    return loss.detach(), x.grad


def test_loss_gradients_against_the_reference_and_fp64(ua, golden):
    g = golden("ssim")
    for tag in [str(c) for c in g["cases"]]:
        p, t = (v.to(DEV) for v in R.case_inputs(g, tag))
        N = p.shape[0]
        for sa in (True, False):
            loss, gr = _grad(ua.SSIMLoss(size_average=sa), p, t)
            ref = torch.from_numpy(g[f"ssimloss_{int(sa)}_{tag}"]).double()
            assert (loss.double().cpu() - ref).abs().max().item() <= 2e-5, (tag, sa)
            e = R.grad_errors(gr, g, f"ssimloss_grad_{int(sa)}_{tag}", tag)
            assert max(e) <= GRAD_VS_FIXTURE, (tag, sa, e)
            # a non-unit upstream (per image for size_average=False) against fp64 autograd
            up = torch.tensor(0.7) if sa else torch.linspace(0.5, 2.0, N)
            _, gu = _grad(ua.SSIMLoss(size_average=sa), p, t, up.to(DEV))
            x = p.double().clone().requires_grad_(True)
            s = R.ssim_map(x, t.double())
            lx = 1 - (s.mean() if sa else s.mean(dim=(1, 2, 3)))
            (lx * up.to(DEV).double()).sum().backward()
            assert rel_l2(gu, x.grad) <= 1e-4, (tag, sa)
        loss, gr = _grad(ua.ReconstructionLoss(1.0, 0.0, 0.1), p, t)
        ref = float(g[f"reconloss_{tag}"])
        assert abs(loss.item() - ref) <= 2e-6 + 1e-5 * ref, tag
        e = R.grad_errors(gr, g, f"reconloss_grad_{tag}", tag)
        assert max(e) <= GRAD_VS_FIXTURE, (tag, e)
        x = p.double().clone().requires_grad_(True)
        (((x - t.double()) ** 2).mean() + 0.1 * (1 - R.ssim_map(x, t.double()).mean())).backward()
        assert rel_l2(gr, x.grad) <= 1e-4, tag


def test_gradient_at_bench_size_against_fp64(ua):
    p, t = noisy_pair((8, 3, 512, 512), 4)
    _, gr = _grad(ua.ReconstructionLoss(1.0, 0.0, 0.1), p, t)
    x = p.double().clone().requires_grad_(True)
    (((x - t.double()) ** 2).mean() + 0.1 * (1 - R.ssim_map(x, t.double()).mean())).backward()
    assert rel_l2(gr, x.grad) <= 1e-4


def test_uint8_target_is_bit_identical(ua):
    gen = torch.Generator().manual_seed(5)
    u8 = torch.randint(0, 256, (2, 37, 50, 3), generator=gen, dtype=torch.uint8).to(DEV)
    t = (u8.permute(0, 3, 1, 2).double() / 255.0).float().contiguous()
    p = (t + 0.05 * torch.randn(t.shape, generator=gen).to(DEV)).clamp(0, 1)
    for mk in (lambda lay: ua.SSIMLoss(target_layout=lay),
               lambda lay: ua.SSIMLoss(size_average=False, target_layout=lay),
               lambda lay: ua.ReconstructionLoss(1.0, 0.0, 0.1, target_layout=lay)):
        la, ga = _grad(mk("nchw"), p, t)
        lb, gb = _grad(mk("nhwc_u8"), p, u8)
        assert torch.equal(la, lb) and torch.equal(ga, gb)
    assert torch.equal(ua.calculate_ssim(p, t), ua.calculate_ssim(p, u8))


def test_deterministic_and_batch_invariant(ua):
    p, t = noisy_pair((8, 3, 96, 80), 6)
    a = ua.ops.ssim_fwd(p, t)
    b = ua.ops.ssim_fwd(p, t)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    up = torch.linspace(0.5, 2.0, 8, device=DEV)
    ga = ua.ops.ssim_grad(p, t, up, upstream_per_image=True)
    assert torch.equal(ga, ua.ops.ssim_grad(p, t, up, upstream_per_image=True))
    for i in range(8):
        _, s1, q1 = ua.ops.ssim_fwd(p[i:i + 1].contiguous(), t[i:i + 1].contiguous())
        assert torch.equal(s1[0], a[1][i]) and torch.equal(q1[0], a[2][i]), i
        g1 = ua.ops.ssim_grad(p[i:i + 1].contiguous(), t[i:i + 1].contiguous(), up[i:i + 1],
                              upstream_per_image=True)
        assert torch.equal(g1[0], ga[i]), i


def test_ssim_of_an_image_with_itself_is_one(ua):
    p, _ = noisy_pair((2, 3, 64, 48), 7)
    s = ua.calculate_ssim(p, p)
    assert (s.double() - 1).abs().max().item() <= 1e-6


def test_mse_only_reconstruction_loss_is_mse_loss(ua):
    p, t = noisy_pair((2, 3, 64, 64), 8)
    la, ga = _grad(ua.MSELoss(), p, t)
    lb, gb = _grad(ua.ReconstructionLoss(1.0, 0.0, 0.0), p, t)
    assert torch.equal(la, lb) and torch.equal(ga, gb)


def test_ae_trajectory_under_reconstruction_loss(ua, golden):
    """3 Adam + cosine steps of the tie-free (negative_slope 1) autoencoder under
    ReconstructionLoss(1, 0, 0.1) against the reference's (the bounds of test_ae64_golden)."""
    g = golden("ssim")
    rec = _ae_recorder()
    model = ua.Autoencoder(encoder_dropout_rates=rec.ENC_DROPOUT, decoder_dropout_rates=rec.DEC_DROPOUT,
                           nonlin_kwargs={"negative_slope": 1.0, "inplace": True})
    model.load_state_dict(rec.ae_state_dict())
    model = model.to(DEV).train()
    img = dev(g["ae_image_u8"]).permute(0, 3, 1, 2).float().contiguous() / 255.0
    opt = ua.ae.create_optimizer(model)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=int(g["ae_t_max"]), eta_min=1e-6)
    lossf = ua.ReconstructionLoss(1.0, 0.0, 0.1)
    p0 = {k: p.detach().clone() for k, p in model.named_parameters()}
    for s in range(int(g["ae_steps"])):
        model.dropout_mask_override = rec.draw_masks(rec.SEED_DROP + s)
        assert opt.param_groups[0]["lr"] == float(g[f"ae_lr_{s}"])
        opt.zero_grad()
        loss = lossf(model(img), img)
        loss.backward()
        ref = float(g[f"ae_loss_{s}"])
        assert abs(loss.item() - ref) <= (2e-4, 2e-3, 5e-2)[s] * ref, (s, loss.item(), ref)
        for i, (k, p) in enumerate(model.named_parameters()):
            gn = float(g[f"ae_gnorm_{s}_{i}"])
            if gn < 1e-4:        # conv biases under InstanceNorm: exact 0 up to rounding
                continue
            got = p.grad.double().norm().item()
            assert abs(got - gn) <= (1e-3, 2e-2, 5e-2)[s] * gn, (s, k, got, gn)
        opt.step()
        sched.step()
        for i, (k, p) in enumerate(model.named_parameters()):
            if float(g[f"ae_gnorm_0_{i}"]) < 1e-4:
                continue
            dn = float(g[f"ae_dnorm_{s}_{i}"])
            d = (p.detach() - p0[k]).double().norm().item()
            assert abs(d - dn) <= (5e-3, 2e-2, 5e-2)[s] * dn, (s, k, d, dn)


def test_graphed_step_with_reconstruction_loss_replays_eager_steps(ua):
    rec = _ae_recorder()
    gen = torch.Generator().manual_seed(11)
    img = (torch.randint(0, 256, (2, 3, 64, 64), generator=gen).float() / 255.0).to(DEV)
    results = []
    for graphed in (False, True):
        model = ua.ae.create_model(DEV).train()
        model.load_state_dict(rec.ae_state_dict())
        model.dropout_mask_override = [m.to(DEV) for m in rec.draw_masks(12)]
        opt = ua.ae.create_optimizer(model)
        lossf = ua.ReconstructionLoss(1.0, 0.0, 0.1)
        step = ua.GraphedTrainStep(model, opt, lossf, img, img) if graphed else None
        losses = []
        for s in range(3):
            opt.param_groups[0]["lr"] = 1e-3 * (1.0 - 0.3 * s)
            loss = step(img, img) if graphed else ua.train_step(model, opt, lossf, img, img)
            losses.append(loss.item())
        results.append((model.flat_parameters()[0].clone(), losses, opt._flat_m.clone()))
    (pa, la, ma), (pb, lb, mb) = results
    assert la == lb
    assert torch.equal(pa, pb) and torch.equal(ma, mb)


def test_evaluate_reconstruction_quality(ua):
    """A 5-image loader with a partial last batch against the reference's loop
    (src/evaluate.py:268-377) restated in fp64."""
    model = ua.ae.create_model(DEV)
    gen = torch.Generator().manual_seed(21)
    imgs = [(torch.randint(0, 256, (n, 3, 64, 64), generator=gen).float() / 255.0).to(DEV)
            for n in (2, 2, 1)]
    loader = [{"image": x, "target": x} for x in imgs]
    m = ua.ae.evaluate_reconstruction_quality(model, loader, DEV)
    assert m["num_samples"] == 5
    model.eval()
    mse = psnr = ssim = 0.0
    with torch.no_grad():
        for x in imgs:
            o = model(x).double()
            e = ((o - x.double()) ** 2).mean(dim=(1, 2, 3))
            mse += e.sum().item()
            psnr += (10 * torch.log10(1 / e)).sum().item()
            ssim += R.ssim_per_image(o, x.double()).sum().item()
    assert abs(m["mse"] - mse / 5) <= 1e-5 * mse / 5
    assert abs(m["psnr"] - psnr / 5) <= 1e-4
    assert abs(m["ssim"] - ssim / 5) <= 1e-5
