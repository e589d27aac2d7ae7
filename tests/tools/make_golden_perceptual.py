#!/usr/bin/env python3
"""Generates tests/golden/perceptual.npz by running the REFERENCE's PerceptualLoss on CPU.

Runs only in the build container (needs the reference checkout).  Loads
`AE_pretrained/reconstruction/models/losses.py` by file path with a stand-in for
`torchvision.models.vgg16(weights=None)` (torchvision is not installed): an object whose
`.features` is the stock-torch nn.Sequential of configuration "D" (tests/tools/vgg_inputs.py), so
the reference's own PerceptualLoss / ReconstructionLoss run unchanged.  The trunk's weights are
the seeded ones of vgg_inputs.trunk_weights (7.6 M floats cannot be committed; the fixture pins
them with per-tensor norms and sampled entries).

Records, for the cases of vgg_inputs.CASES (8-bit inputs, stored as uint8 NCHW): the per-layer
feature MSEs, the loss, the fp64 norm and GRAD_SAMPLES sampled entries of dL/doutput, and the
reference's own fp32-vs-fp64 distance measured by running the same modules in double
(`ref_loss_err_<case>`, `ref_grad_err_<case>`); the reference's state_dict key list for the
default layers; and 3 Adam + cosine steps of the reference Autoencoder under
ReconstructionLoss(1.0, 0.1, 0.0) at 2 x 64^2 with negative_slope = 1.0 (make_golden_ae.py's
weights, image and dropout masks): learning rate, loss and output of every step.
Data only: nothing from the reference's source travels.

Usage: python tests/tools/make_golden_perceptual.py [--out PATH] [--reference DIR]
"""
import argparse
import copy
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

import vgg_inputs as V  # noqa: E402


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def npf(t):
    return t.detach().cpu().numpy()


def run(loss_module, p, t):
    """(loss, per-layer MSEs in `features` order, dL/dp) of the reference module."""
    x = p.clone().requires_grad_(True)
    loss = loss_module(x, t)
    loss.backward()
    with torch.no_grad():
        pn, tn = loss_module._normalize(p), loss_module._normalize(t)
        per_layer = [torch.nn.functional.mse_loss(layer(pn.clone()), layer(tn.clone()))
                     for layer in loss_module.features.values()]
    return loss.detach(), torch.stack(per_layer), x.grad.detach()


def record_cases(L, weights, out):
    for si, (tag, (shape, layers, kind, seed)) in enumerate(V.CASES.items()):
        pu, tu = V.case_inputs(shape, kind, seed)
        p, t = pu.float() / 255, tu.float() / 255
        ref = V.load_trunk(L.PerceptualLoss(layers=layers), weights)
        loss, per_layer, grad = run(ref, p, t)
        ref64 = copy.deepcopy(ref).double()
        loss64, per64, grad64 = run(ref64, p.double(), t.double())
        idx = V.grad_idx(p.numel(), seed)
        flat = grad.reshape(-1)
        out[f"pred_u8_{tag}"] = npf(pu)
        out[f"target_u8_{tag}"] = npf(tu)
        out[f"layers_{tag}"] = np.array(list(ref.features.keys()))
        out[f"loss_{tag}"] = npf(loss)
        out[f"layer_mse_{tag}"] = npf(per_layer)
        out[f"grad_idx_{tag}"] = idx
        out[f"grad_{tag}"] = npf(flat[torch.from_numpy(idx)])
        out[f"grad_norm_{tag}"] = np.float64(flat.double().norm().item())
        # the reference's own distance from fp64: the loss, and the gradient as the largest of the
        # relative L2 over all entries, over the sampled entries and of the norm
        e_s, e_n = V.grad_errors(grad, npf(grad64.reshape(-1)[torch.from_numpy(idx)]), idx,
                                 grad64.norm().item())
        e_full = ((grad.double() - grad64).norm() / grad64.norm()).item()
        out[f"ref_loss_err_{tag}"] = np.float64(abs(loss.item() - loss64.item()) / loss64.item())
        out[f"ref_grad_err_{tag}"] = np.float64(max(e_s, e_n, e_full))
        print(f"  {tag}: loss {loss.item():.6f} layers {npf(per_layer)} "
              f"ref err {out[f'ref_loss_err_{tag}']:.2e} / {out[f'ref_grad_err_{tag}']:.2e}")
    out["cases"] = np.array(list(V.CASES))


def record_ae(L, reference, weights, out):
    """3 Adam + cosine steps at 2 x 64^2, negative_slope 1 (make_golden_ae's setup), under
    ReconstructionLoss(1.0, 0.1, 0.0) with the seeded trunk."""
    R = _load("make_golden_ae", os.path.join(ROOT, "tests", "tools", "make_golden_ae.py"))
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
    lossf = L.ReconstructionLoss(mse_weight=1.0, perceptual_weight=0.1, ssim_weight=0.0)
    V.load_trunk(lossf.perceptual_loss, weights)
    for s in range(R.STEPS):
        feed[:] = list(R.draw_masks(R.SEED_DROP + s))
        out[f"ae_lr_{s}"] = np.float64(opt.param_groups[0]["lr"])
        opt.zero_grad()
        o = model(img)
        assert not feed, "every injected mask is consumed"
        loss = lossf(o, img)
        loss.backward()
        out[f"ae_loss_{s}"] = npf(loss)
        out[f"ae_out_{s}"] = npf(o)
        opt.step()
        sched.step()
        print(f"  AE step {s}: loss {loss.item():.6f}")
    out["ae_image_u8"] = u8
    out["ae_steps"] = np.int64(R.STEPS)
    out["ae_t_max"] = np.int64(R.T_MAX)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "perceptual.npz"))
    ap.add_argument("--reference", default="/root/reference")
    args = ap.parse_args()
    V.install_torchvision_stub()
    L = _load("ref_recon_losses", os.path.join(args.reference, "AE_pretrained", "reconstruction",
                                               "models", "losses.py"))
    torch.use_deterministic_algorithms(True)
    torch.set_num_threads(1)
    weights = V.trunk_weights(V.convs_needed(None))
    out = {"seed_w": np.int64(V.SEED_W)}
    out.update(V.pin_weights(weights))
    torch.manual_seed(0)
    out["state_dict_keys"] = np.array(list(L.PerceptualLoss().state_dict().keys()))
    record_cases(L, weights, out)
    record_ae(L, args.reference, weights, out)
    with open(args.out, "wb") as f:
        np.savez_compressed(f, **dict(sorted(out.items())))
    print(os.path.basename(args.out), "written")


if __name__ == "__main__":
    main()
