"""Shared by tests/tools/make_golden_perceptual.py and the perceptual-loss tests: the VGG16 trunk's
seeded weights, the stand-in for `torchvision.models.vgg16(weights=None)`, the recorded cases and
their inputs.

The trunk's 7.6 M floats (to relu4_3) cannot be committed, so the recorder and the tests both
rebuild them from a numpy PCG64 stream: Kaiming-normal (fan_out) weights and small non-zero biases
(so that the bias path is exercised), drawn convolution by convolution, so a shallower trunk is a
prefix of a deeper one.  The fixture pins them with per-tensor norms and 64 sampled entries."""
import sys
import types

import numpy as np
import torch
import torch.nn as nn

# torchvision's configuration "D" and the reference's layer map (models/losses.py:103-109)
CFG = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M")
LAYER_MAP = {"relu1_1": 1, "relu1_2": 3, "relu2_1": 6, "relu2_2": 8, "relu3_1": 11, "relu3_2": 13,
             "relu3_3": 15, "relu4_1": 18, "relu4_2": 20, "relu4_3": 22, "relu5_1": 25,
             "relu5_2": 27, "relu5_3": 29}
DEFAULT_LAYERS = ["relu1_2", "relu2_2", "relu3_3", "relu4_3"]
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SEED_W = 1616
PIN_SAMPLES = 64
GRAD_SAMPLES = 1024

# name -> (shape, layers (None = default), kind of input, seed)
CASES = {
    "random_32": ((2, 3, 32, 32), None, "random", 41),
    "structured_32": ((2, 3, 32, 32), None, "structured", 42),
    "random_64": ((2, 3, 64, 64), None, "random", 43),
    "floor_37x50": ((1, 3, 37, 50), ["relu1_2", "relu2_2", "relu3_3"], "random", 44),
    "relu2_2_only": ((2, 3, 32, 32), ["relu2_2"], "random", 45),
    "relu1_1_only": ((2, 3, 32, 32), ["relu1_1"], "structured", 46),
    "relu3_1_only": ((2, 3, 32, 32), ["relu3_1"], "random", 47),
}


def conv_channels():
    """(feature index, Cin, Cout) of the 13 convolutions in order."""
    out, idx, cin = [], 0, 3
    for v in CFG:
        if v == "M":
            idx += 1
        else:
            out.append((idx, cin, v))
            cin = v
            idx += 2
    return out


def convs_needed(layers):
    names = [n for n in (DEFAULT_LAYERS if layers is None else layers) if n in LAYER_MAP]
    deepest = max(LAYER_MAP[n] for n in names)
    return sum(1 for idx, _, _ in conv_channels() if idx < deepest)


def trunk_weights(nconv=13, seed=SEED_W):
    """[(feature index, weight OIHW fp32, bias fp32)] of the first `nconv` convolutions."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for idx, cin, cout in conv_channels()[:nconv]:
        w = (rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (cout * 9))).astype(np.float32)
        b = (rng.standard_normal(cout) * 0.05).astype(np.float32)
        out.append((idx, torch.from_numpy(w), torch.from_numpy(b)))
    return out


def load_trunk(loss_module, weights):
    """Copy the seeded weights into a PerceptualLoss (the reference's or this project's: both hold
    `features`, a ModuleDict of prefix Sequentials sharing their modules)."""
    by_idx = {idx: (w, b) for idx, w, b in weights}
    sd = loss_module.state_dict()
    for key in list(sd):
        parts = key.split(".")
        if parts[0] == "features":
            w, b = by_idx[int(parts[2])]
            sd[key] = (w if parts[3] == "weight" else b).clone()
    loss_module.load_state_dict(sd)
    return loss_module


def pin_weights(weights):
    """{key: value} that pins the rebuilt weights: fp64 norms and PIN_SAMPLES entries a tensor."""
    out = {}
    for idx, w, b in weights:
        for name, t in (("w", w), ("b", b)):
            flat = t.reshape(-1)
            rng = np.random.Generator(np.random.PCG64(idx * 2 + (name == "b")))
            pos = np.sort(rng.choice(flat.numel(), size=min(PIN_SAMPLES, flat.numel()),
                                     replace=False)).astype(np.int64)
            out[f"pin_{name}{idx}_norm"] = np.float64(flat.double().norm().item())
            out[f"pin_{name}{idx}_idx"] = pos
            out[f"pin_{name}{idx}_val"] = flat[torch.from_numpy(pos)].numpy()
    return out


def stub_features():
    """The stock-torch nn.Sequential of configuration "D" with torchvision's initialisation:
    13 x (Conv2d, ReLU(inplace=True)) and 5 x MaxPool2d(2, 2), 31 modules."""
    mods, cin = [], 3
    for v in CFG:
        if v == "M":
            mods.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            mods += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    for m in mods:
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            nn.init.constant_(m.bias, 0)
    return nn.Sequential(*mods)


def install_torchvision_stub():
    """`from torchvision import models; models.vgg16(weights=None)` without torchvision: an object
    whose `.features` is `stub_features()`."""
    if "torchvision" in sys.modules and hasattr(sys.modules["torchvision"].models, "vgg16"):
        return
    tv = types.ModuleType("torchvision")
    tv.models = types.ModuleType("torchvision.models")

    def vgg16(weights=None):
        assert weights is None
        return types.SimpleNamespace(features=stub_features())

    tv.models.vgg16 = vgg16
    sys.modules["torchvision"] = tv
    sys.modules["torchvision.models"] = tv.models


def case_inputs(shape, kind, seed):
    """(pred, target) as 8-bit images: uint8 NCHW tensors (the operands are v / 255 in fp32)."""
    g = torch.Generator().manual_seed(seed)
    N, C, H, W = shape
    if kind == "random":
        t = torch.rand(shape, generator=g)
        p = (t + 0.15 * torch.randn(shape, generator=g)).clamp(0, 1)
    else:   # smooth gradients, flat blocks and sharp edges; pred blurred, shifted, lightly noised
        yy = torch.linspace(0, 1, H).view(1, 1, H, 1)
        xx = torch.linspace(0, 1, W).view(1, 1, 1, W)
        ph = torch.rand(N, C, 1, 1, generator=g) * 6.28
        t = (0.5 + 0.3 * torch.sin(6.0 * xx + 4.0 * yy + ph)).expand(N, C, H, W).clone()
        t[:, :, : H // 3, : W // 2] = 0.8
        t[:, :, H // 2:, W // 2:] = 0.1
        t[:, 1, :, W // 3] = 1.0
        p = t.clone()
        p[:, :, 1:, 1:] = 0.6 * t[:, :, 1:, 1:] + 0.4 * t[:, :, :-1, :-1]
        p = (p + 0.02 * torch.randn(shape, generator=g) + 0.03).clamp(0, 1)

    def q(x):
        return (x * 255).round().clamp(0, 255).to(torch.uint8).contiguous()

    return q(p), q(t)


def operands(g, tag):
    """(pred, target) fp32 NCHW of a recorded case, as the recorder fed them to the reference."""
    return (torch.from_numpy(g[f"pred_u8_{tag}"]).float() / 255,
            torch.from_numpy(g[f"target_u8_{tag}"]).float() / 255)


def grad_idx(numel, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return np.sort(rng.choice(numel, size=min(GRAD_SAMPLES, numel), replace=False)).astype(np.int64)


def grad_errors(grad, ref_samples, idx, ref_norm):
    """(relative L2 error over the sampled entries, relative error of the L2 norm)."""
    flat = grad.detach().reshape(-1).double().cpu()
    ref = torch.from_numpy(np.asarray(ref_samples)).double()
    got = flat[torch.from_numpy(np.asarray(idx))]
    return (((got - ref).norm() / ref.norm()).item(),
            abs(flat.norm().item() - float(ref_norm)) / float(ref_norm))
