#!/usr/bin/env python3
"""Generates tests/golden/ae64.npz by running the REFERENCE's autoencoder on CPU.

Runs only in the build container (needs the reference checkout).  Imports the reference's
`AE_pretrained/reconstruction/models/autoencoder.py` (torch only), loads deterministic weights -
`oracle.unet_ref.fill_state_dict` for the body shared with the UNet plus a seeded draw for
`reconstruction_output.0.*` - injects seeded dropout masks at the autoencoder's rates, and
records, at 2 x 64x64, for the default LeakyReLU slope and for negative_slope = 1.0 (the tie-free
network): eval and train outputs, the loss of 3 `torch.optim.Adam(lr=1e-3, weight_decay=1e-5)`
steps with a `CosineAnnealingLR` step between them under `nn.MSELoss`, per-tensor gradient norms
and 256 sampled entries per tensor, parameter-delta norms per step and the Adam state after step 3.
Data only: nothing from the reference's source travels.

Usage: python tests/tools/make_golden_ae.py [--out PATH] [--reference DIR]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import unet_ref as O  # noqa: E402

SEED_W, SEED_HEAD, SEED_X, SEED_DROP = 2024, 4242, 1234, 77
N, HW, STEPS, T_MAX = 2, 64, 3, 4
ENC_DROPOUT = [0.0, 0.0, 0.05, 0.1, 0.15, 0.15]   # the AE's create_model
DEC_DROPOUT = [0.15, 0.1, 0.1, 0.05, 0.0]


def sample_idx(numel, k=64, seed=5):
    rng = np.random.Generator(np.random.PCG64(seed + numel))
    return np.sort(rng.choice(numel, size=min(k, numel), replace=False))


def npf(t):
    return t.detach().cpu().numpy()


def ae_state_dict():
    """The UNet body of fill_state_dict (the AE's zero-rate stages are the UNet's, so the
    module indices agree) and a seeded 3x3 head."""
    sd = {k: v for k, v in O.fill_state_dict(SEED_W).items()
          if not k.startswith("segmentation_output")}
    rng = np.random.Generator(np.random.PCG64(SEED_HEAD))
    std = np.sqrt(2.0 / (3 * 9))
    sd["reconstruction_output.0.weight"] = torch.from_numpy(
        (rng.standard_normal((3, 32, 3, 3)) * std).astype(np.float32))
    sd["reconstruction_output.0.bias"] = torch.from_numpy(
        (rng.standard_normal(3) * 0.1).astype(np.float32))
    return sd


def dropout_channels():
    """(channels, rate) of every SpatialDropout2d of the AE in forward order."""
    feats = O.FEATURES
    out = [(f, p) for f, p in zip(feats, ENC_DROPOUT) if p > 0 for _ in range(2)]
    for d, p in enumerate(DEC_DROPOUT):
        if p > 0:
            out += [(feats[len(feats) - 2 - d], p)] * 2
    return out


def draw_masks(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.empty(N, c, 1, 1).bernoulli_(1 - p, generator=g).div_(1 - p).view(N, c)
            for c, p in dropout_channels()]


def synthetic_image():
    rng = np.random.Generator(np.random.PCG64(SEED_X))
    u8 = rng.integers(0, 256, size=(N, HW, HW, 3), dtype=np.uint8)
    img = torch.from_numpy(u8).float().permute(0, 3, 1, 2).contiguous() / 255.0
    return u8, img


def run(mod, slope, out, tag):
    sd0 = ae_state_dict()
    u8, img = synthetic_image()
    kw = {"inplace": True} if slope is None else {"negative_slope": slope, "inplace": True}
    model = mod.Autoencoder(in_channels=3, out_channels=3, encoder_dropout_rates=ENC_DROPOUT,
                            decoder_dropout_rates=DEC_DROPOUT, nonlin_kwargs=kw)
    model.load_state_dict(sd0)
    assert list(model.state_dict()) == list(sd0), "state_dict keys differ from the reference's"
    drops = [m for m in model.modules() if type(m).__name__ == "SpatialDropout2d" and m.drop_prob > 0]
    assert len(drops) == len(dropout_channels())
    feed = []

    def injected(self, x):          # the reference's channel dropout with a recorded mask
        if not self.training or self.drop_prob == 0:
            return x
        return x * feed.pop(0).view(x.size(0), x.size(1), 1, 1).expand_as(x)

    for m in drops:
        m.forward = injected.__get__(m)
    model.eval()
    with torch.no_grad():
        out[f"eval_out{tag}"] = npf(model(img))
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-5)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=T_MAX, eta_min=1e-6)
    lossf = torch.nn.MSELoss()
    names = [k for k, _ in model.named_parameters()]
    for s in range(STEPS):
        masks = draw_masks(SEED_DROP + s)
        for j, m in enumerate(masks):
            out[f"mask{tag}_{s}_{j}"] = npf(m)
        feed[:] = list(masks)
        out[f"lr{tag}_{s}"] = np.float64(opt.param_groups[0]["lr"])
        opt.zero_grad()
        o = model(img)
        assert not feed, "every injected mask is consumed"
        loss = lossf(o, img)
        loss.backward()
        out[f"loss{tag}_{s}"] = npf(loss)
        if s == 0:
            out[f"train_out{tag}"] = npf(o)
            for i, (k, p) in enumerate(model.named_parameters()):
                gk = p.grad.reshape(-1)
                out[f"gnorm{tag}_{i}"] = np.float64(gk.double().norm().item())
                out[f"gsamp{tag}_{i}"] = npf(gk[torch.from_numpy(sample_idx(gk.numel(), k=256))])
        opt.step()
        sched.step()
        for i, (k, p) in enumerate(model.named_parameters()):
            d = (p.detach() - sd0[k]).reshape(-1)
            out[f"dnorm{tag}_{s}_{i}"] = np.float64(d.double().norm().item())
        print(f"  slope {slope or 0.01} step {s}: loss {loss.item():.6f}")
    for i, (k, p) in enumerate(model.named_parameters()):
        st = opt.state[p]
        idx = torch.from_numpy(sample_idx(p.numel()))
        out[f"psamp{tag}_{i}"] = npf(p.detach().reshape(-1)[idx])
        out[f"msamp{tag}_{i}"] = npf(st["exp_avg"].reshape(-1)[idx])
        out[f"vsamp{tag}_{i}"] = npf(st["exp_avg_sq"].reshape(-1)[idx])
        out[f"mnorm{tag}_{i}"] = np.float64(st["exp_avg"].double().norm().item())
        out[f"vnorm{tag}_{i}"] = np.float64(st["exp_avg_sq"].double().norm().item())
    out[f"adam_step{tag}"] = np.float64(float(opt.state[model.encoder_stages[0].block[0].weight]["step"]))
    return names, u8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ae64.npz"))
    ap.add_argument("--reference", default="/root/reference")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.reference, "AE_pretrained", "reconstruction", "models"))
    import autoencoder as mod     # the reference's model file (torch only)
    torch.use_deterministic_algorithms(True)
    torch.set_num_threads(1)
    out = dict(seed_w=SEED_W, seed_head=SEED_HEAD, seed_x=SEED_X, seed_drop=SEED_DROP, n=N, hw=HW,
               t_max=T_MAX, steps=STEPS)
    names, u8 = run(mod, None, out, "")
    run(mod, 1.0, out, "_s1")
    out["image_u8"] = u8
    out["param_names"] = np.array(names)
    # fixed member order and no timestamps: the same seeds give the same bytes
    with open(args.out, "wb") as f:
        np.savez_compressed(f, **dict(sorted(out.items())))
    print(os.path.basename(args.out), "written")


if __name__ == "__main__":
    main()
