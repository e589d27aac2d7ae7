#!/usr/bin/env python3
"""Generates tests/golden/ssim.npz by running the REFERENCE's SSIM code on CPU.

Runs only in the build container (needs the reference checkout).  Loads
`AE_pretrained/reconstruction/utils/metrics.py` and `models/losses.py` by file path (the packages'
`__init__` import cv2, and losses.py imports torchvision, which gets a stub: only PerceptualLoss
uses it).  The reference's `SSIMLoss.__init__` raises (its window builder calls torch.exp on a
Python float), so the loss is built with `__new__` + `nn.Module.__init__` and given the window it
intends, `gaussian_kernel(11, 1.5, 3)`; `ReconstructionLoss(1.0, 0, 0.1)` is built with
ssim_weight 0 and then handed that loss.

Records, for seeded random and structured (smooth, flat regions, edges) inputs at 2x3x64x64,
1x3x37x50, 2x3x8x8 and 2x3x128x96: calculate_psnr, calculate_ssim (reduction none), the
evaluate_reconstructions dictionary, SSIMLoss for both size_average settings with the autograd
gradient with respect to pred, and ReconstructionLoss(1.0, 0, 0.1) with its gradient.  Inputs are
8-bit images (stored as uint8 NCHW; the operands are v / 255 in fp32, `load_case`).  Gradients are
kept as their fp64 L2 norm and GRAD_SAMPLES entries at seeded positions (`grad_idx_<case>`), which
keeps the fixture small.  Also 3 Adam
+ cosine steps of the reference Autoencoder under that ReconstructionLoss at 2 x 64^2 with
negative_slope = 1.0 (make_golden_ae.py's weights, image and dropout masks).
Data only: nothing from the reference's source travels.

Usage: python tests/tools/make_golden_ssim.py [--out PATH] [--reference DIR]
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SHAPES = [(2, 3, 64, 64), (1, 3, 37, 50), (2, 3, 8, 8), (2, 3, 128, 96)]
SEED = 31
GRAD_SAMPLES = 1024


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _recorder_ae():
    return _load("make_golden_ae", os.path.join(ROOT, "tests", "tools", "make_golden_ae.py"))


def case_inputs(shape, kind, seed):
    """(pred, target) fp32 in [0, 1].  random: independent uniform images, pred a noisy copy of
    target.  structured: smooth gradients, flat blocks and sharp edges, pred a blurred, offset and
    lightly noised version."""
    g = torch.Generator().manual_seed(seed)
    N, C, H, W = shape
    if kind == "random":
        t = torch.rand(shape, generator=g)
        p = (t + 0.15 * torch.randn(shape, generator=g)).clamp(0, 1)
        return p.contiguous(), t.contiguous()
    yy = torch.linspace(0, 1, H).view(1, 1, H, 1)
    xx = torch.linspace(0, 1, W).view(1, 1, 1, W)
    ph = torch.rand(N, C, 1, 1, generator=g) * 6.28
    t = 0.5 + 0.3 * torch.sin(6.0 * xx + 4.0 * yy + ph)
    t = t.expand(N, C, H, W).clone()
    t[:, :, : H // 3, : W // 2] = 0.8                     # a flat block
    t[:, :, H // 2:, W // 2:] = 0.1                       # another, meeting the first at edges
    t[:, 1, :, W // 3] = 1.0                              # a one-pixel line in one channel
    p = t.clone()
    p[:, :, 1:, 1:] = 0.6 * t[:, :, 1:, 1:] + 0.4 * t[:, :, :-1, :-1]   # blur + shift
    p = (p + 0.02 * torch.randn(shape, generator=g) + 0.03).clamp(0, 1)
    return p.contiguous(), t.contiguous()


def quantize(x):
    """An 8-bit image: uint8 values and the fp32 operand v / 255."""
    u8 = (x * 255).round().clamp(0, 255).to(torch.uint8)
    return u8, u8.float() / 255


def load_case(g, tag):
    """(pred, target) fp32 NCHW of a recorded case, as the recorder fed them to the reference."""
    return (torch.from_numpy(g[f"pred_u8_{tag}"]).float() / 255,
            torch.from_numpy(g[f"target_u8_{tag}"]).float() / 255)


def grad_idx(numel, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return np.sort(rng.choice(numel, size=min(GRAD_SAMPLES, numel), replace=False)).astype(np.int64)


def put_grad(out, key, grad, idx):
    flat = grad.detach().reshape(-1)
    out[key] = npf(flat[torch.from_numpy(idx)])
    out[f"{key}_norm"] = np.float64(flat.double().norm().item())


def make_ssim_loss(L, M, size_average):
    loss = L.SSIMLoss.__new__(L.SSIMLoss)
    torch.nn.Module.__init__(loss)
    loss.window_size = 11
    loss.size_average = size_average
    loss.channel = 3
    loss.window = M.gaussian_kernel(11, 1.5, 3)
    return loss


def make_recon_loss(L, M, mse_w, ssim_w):
    rl = L.ReconstructionLoss(mse_weight=mse_w, perceptual_weight=0.0, ssim_weight=0.0)
    rl.ssim_weight = ssim_w
    rl.ssim_loss = make_ssim_loss(L, M, True)
    return rl


def npf(t):
    return t.detach().cpu().numpy()


def record_cases(L, M, out):
    names = []
    for si, shape in enumerate(SHAPES):
        for kind in ("random", "structured"):
            tag = f"{kind}_{'x'.join(map(str, shape))}"
            names.append(tag)
            p, t = case_inputs(shape, kind, SEED + 10 * si + (kind == "structured"))
            pu, p = quantize(p)
            tu, t = quantize(t)
            out[f"pred_u8_{tag}"] = npf(pu)
            out[f"target_u8_{tag}"] = npf(tu)
            idx = grad_idx(p.numel(), SEED + si)
            out[f"grad_idx_{tag}"] = idx
            out[f"psnr_{tag}"] = npf(M.calculate_psnr(p, t))
            out[f"ssim_{tag}"] = npf(M.calculate_ssim(p, t))
            for k, v in M.evaluate_reconstructions(p, t).items():
                out[f"eval_{k}_{tag}"] = npf(v)
            for sa in (True, False):
                x = p.clone().requires_grad_(True)
                loss = make_ssim_loss(L, M, sa)(x, t)
                loss.sum().backward()       # size_average=False: unit upstream per image
                out[f"ssimloss_{int(sa)}_{tag}"] = npf(loss)
                put_grad(out, f"ssimloss_grad_{int(sa)}_{tag}", x.grad, idx)
            x = p.clone().requires_grad_(True)
            loss = make_recon_loss(L, M, 1.0, 0.1)(x, t)
            loss.backward()
            out[f"reconloss_{tag}"] = npf(loss)
            put_grad(out, f"reconloss_grad_{tag}", x.grad, idx)
            print(f"  {tag}: ssim {out[f'ssim_{tag}']}")
    out["cases"] = np.array(names)


def record_ae(L, M, reference, out):
    """3 Adam + cosine steps at 2 x 64^2, negative_slope 1 (make_golden_ae's setup), under
    ReconstructionLoss(1.0, 0, 0.1)."""
    R = _recorder_ae()
    sys.path.insert(0, os.path.join(reference, "AE_pretrained", "reconstruction", "models"))
    import autoencoder as mod     # the reference's model file (torch only)
    sd0 = R.ae_state_dict()
    u8, img = R.synthetic_image()
    model = mod.Autoencoder(in_channels=3, out_channels=3, encoder_dropout_rates=R.ENC_DROPOUT,
                            decoder_dropout_rates=R.DEC_DROPOUT,
                            nonlin_kwargs={"negative_slope": 1.0, "inplace": True})
    model.load_state_dict(sd0)
    drops = [m for m in model.modules() if type(m).__name__ == "SpatialDropout2d" and m.drop_prob > 0]
    feed = []

    def injected(self, x):
        if not self.training or self.drop_prob == 0:
            return x
        return x * feed.pop(0).view(x.size(0), x.size(1), 1, 1).expand_as(x)

    for m in drops:
        m.forward = injected.__get__(m)
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-5)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=R.T_MAX, eta_min=1e-6)
    lossf = make_recon_loss(L, M, 1.0, 0.1)
    for s in range(R.STEPS):
        feed[:] = list(R.draw_masks(R.SEED_DROP + s))
        out[f"ae_lr_{s}"] = np.float64(opt.param_groups[0]["lr"])
        opt.zero_grad()
        o = model(img)
        assert not feed, "every injected mask is consumed"
        loss = lossf(o, img)
        loss.backward()
        out[f"ae_loss_{s}"] = npf(loss)
        for i, (k, p) in enumerate(model.named_parameters()):
            out[f"ae_gnorm_{s}_{i}"] = np.float64(p.grad.double().norm().item())
        opt.step()
        sched.step()
        for i, (k, p) in enumerate(model.named_parameters()):
            out[f"ae_dnorm_{s}_{i}"] = np.float64((p.detach() - sd0[k]).double().norm().item())
        print(f"  AE step {s}: loss {loss.item():.6f}")
    out["ae_image_u8"] = u8
    out["ae_steps"] = np.int64(R.STEPS)
    out["ae_t_max"] = np.int64(R.T_MAX)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ssim.npz"))
    ap.add_argument("--reference", default="/root/reference")
    args = ap.parse_args()
    rec = os.path.join(args.reference, "AE_pretrained", "reconstruction")
    if "torchvision" not in sys.modules:      # losses.py: `from torchvision import models`
        tv = types.ModuleType("torchvision")
        tv.models = types.ModuleType("torchvision.models")
        sys.modules["torchvision"] = tv
        sys.modules["torchvision.models"] = tv.models
    M = _load("ref_recon_metrics", os.path.join(rec, "utils", "metrics.py"))
    L = _load("ref_recon_losses", os.path.join(rec, "models", "losses.py"))
    torch.use_deterministic_algorithms(True)
    torch.set_num_threads(1)
    out = {"seed": np.int64(SEED), "window": npf(M.gaussian_kernel(11, 1.5, 1)[0, 0])}
    record_cases(L, M, out)
    record_ae(L, M, args.reference, out)
    with open(args.out, "wb") as f:
        np.savez_compressed(f, **dict(sorted(out.items())))
    print(os.path.basename(args.out), "written")


if __name__ == "__main__":
    main()
