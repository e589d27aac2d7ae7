"""CPU (-m "not gpu"): Grad-CAM without a device - the ABI surface of unet_gradcam_*, the host-side
argument checks, the fixture's bit-stable inputs, the target / class validation of
`evaluate.gradcam`, and the zero-mean argument its ValueError text rests on.  Nothing here reads
the reference (tests/golden/gradcam.npz was recorded from its own generate_gradcam_heatmap by
tests/tools/make_golden_gradcam.py)."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "unet_hip.h")


def _load(name):
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(ROOT, "tests", "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GI = _load("gradcam_inputs")
ENTRY_POINTS = ("unet_gradcam_weights", "unet_gradcam_map", "unet_gradcam_heatmap")


def test_entry_points_declared_exported_and_bound(ua):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    handle = ctypes.CDLL(ua.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), f"{name} not declared in unet_hip.h"
        assert hasattr(handle, name), f"{name} not exported"
        assert name in ua._lib.SIGNATURES
    for name in ("gradcam_weights", "gradcam_map", "gradcam_heatmap"):
        assert callable(getattr(ua.ops, name))
    for name in ("gradcam", "gradcam_batch", "generate_gradcam_heatmap"):
        assert callable(getattr(ua.evaluate, name)) and getattr(ua, name) is getattr(ua.evaluate, name)


def test_abi_version_is_unchanged(ua):
    header = int(re.search(r"#define\s+UNET_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert header == ua._lib.ABI_VERSION == ua.lib().unet_abi_version() == 11


def test_host_arguments_are_rejected_before_any_launch(ua):
    lib = ua.lib()
    assert lib.unet_gradcam_workspace_bytes(8, 512 * 512, 32) > 0
    assert lib.unet_gradcam_workspace_bytes(3, 4, 512) > 0
    assert lib.unet_gradcam_workspace_bytes(3, 4, 48) == 0          # 12 lanes do not tile a wave
    rc = lib.unet_gradcam_weights(None, 0, 16, 16, 1 << 20, 1, 64, 32, None)
    assert rc == -1 and b"null" in lib.unet_last_error()
    rc = lib.unet_gradcam_weights(16, 0, 16, 16, 1 << 20, 1, 64, 48, None)
    assert rc == -1 and b"bad shape" in lib.unet_last_error()
    rc = lib.unet_gradcam_weights(16, 0, 16, 16, 1 << 20, 0, 64, 32, None)
    assert rc == -1 and b"bad shape" in lib.unet_last_error()
    rc = lib.unet_gradcam_weights(16, 0, 16, 16, 8, 1, 64, 32, None)
    assert rc == -3 and b"workspace" in lib.unet_last_error()
    rc = lib.unet_gradcam_weights(8, 0, 16, 16, 1 << 20, 1, 64, 32, None)
    assert rc == -1 and b"aligned" in lib.unet_last_error()
    src = ua._lib.ActSrc(16, 32, None, None)
    rc = lib.unet_gradcam_map(None, 0, 0.01, 16, 16, 16, 1 << 20, 1, 64, None)
    assert rc == -1 and b"null" in lib.unet_last_error()
    rc = lib.unet_gradcam_map(ctypes.byref(src), 0, 1.5, 16, 16, 16, 1 << 20, 1, 64, None)
    assert rc == -1 and b"slope" in lib.unet_last_error()
    rc = lib.unet_gradcam_map(ctypes.byref(src), 0, 0.01, 16, 16, 16, 8, 1, 64, None)
    assert rc == -3 and b"workspace" in lib.unet_last_error()
    rc = lib.unet_gradcam_heatmap(16, 16, 1 << 20, None, 1, 8, 8, 64, 64, None)
    assert rc == -1 and b"null" in lib.unet_last_error()
    rc = lib.unet_gradcam_heatmap(16, 16, 1 << 20, 16, 1, 0, 8, 64, 64, None)
    assert rc == -1 and b"bad shape" in lib.unet_last_error()
    rc = lib.unet_gradcam_heatmap(16, 16, 8, 16, 1, 8, 8, 64, 64, None)
    assert rc == -3 and b"workspace" in lib.unet_last_error()


def test_fixture_inputs_regenerate_bit_identically(golden):
    g = golden("gradcam")
    assert [str(c) for c in g["cases"]] == [c[0] for c in GI.CASES]
    assert int(g["weight_seed"]) == GI.WEIGHT_SEED
    for name, spec in GI.BATCHES.items():
        assert list(g[f"batch_{name}"]) == list(spec)
    sd = GI.state_dict()
    imgs = {name: GI.images(name) for name in GI.BATCHES}
    assert np.array_equal(GI.digest(sd, imgs), g["sha256_inputs"])
    for name, batch, layer, cls in GI.CASES:
        n, h, w = GI.BATCHES[batch][1:]
        heat = g[f"heat_{name}"]
        assert heat.shape == (n, h, w) and heat.dtype == np.float32
        assert heat.min() >= 0.0 and heat.max() <= 1.0
    # the case behind the per-image normalisation and the zero guard keeps its shape
    z = g[f"heat_{GI.ZERO_CASE}"]
    zero = [not z[b].any() for b in range(z.shape[0])]
    assert any(zero) and not all(zero)
    pmin, pmax = g[f"premin_{GI.ZERO_CASE}"], g[f"premax_{GI.ZERO_CASE}"]
    for b, is_zero in enumerate(zero):
        if is_zero:
            assert pmax[b] < -0.1 * (pmax[b] - pmin[b])
    # the yardstick: shallow target at the logits tolerance, deep targets at 4 x the reference's
    # own fp32 distance from fp64
    bounds = GI.layer_bounds(g)
    assert bounds["decoder_stages[-1]"] == 1e-4
    assert all(1e-4 <= b < 0.1 for b in bounds.values())


def test_inner_targets_and_bad_classes_raise_value_error(ua):
    model = ua.UNet()
    x = torch.zeros(1, 3, 64, 64)
    conv = model.decoder_stages[0].conv_block.block[0]          # the reference's code default
    with pytest.raises(ValueError, match="never holds that tensor") as e:
        ua.evaluate.gradcam(model, x, 1, conv)
    assert "identically zero" in str(e.value) and "decoder_stages.0.conv_block.block.0" in str(e.value)
    norm = model.encoder_stages[2].block[1]
    assert isinstance(norm, nn.InstanceNorm2d)
    with pytest.raises(ValueError, match="never holds that tensor") as e:
        ua.evaluate.gradcam(model, x, 1, norm)
    assert "identically zero" not in str(e.value)
    with pytest.raises(ValueError, match="never holds that tensor"):
        ua.evaluate.gradcam(model, x, 1, model.encoder_stages[0].block)
    with pytest.raises(ValueError, match="not a module of this model"):
        ua.evaluate.gradcam(model, x, 1, nn.Conv2d(3, 3, 3))
    for bad in (-1, 3, 7):
        with pytest.raises(ValueError, match="target_class"):
            ua.evaluate.gradcam(model, x, bad)
    with pytest.raises(ValueError, match="precision"):
        ua.evaluate.gradcam(model, x, 1, precision="bf16")
    # valid arguments on a CPU tensor: the package's usual answer
    for target in (None, model.encoder_stages[3], model.decoder_stages[1],
                   model.decoder_stages[1].conv_block):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ua.evaluate.gradcam(model, x, 1, target)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ua.evaluate.gradcam_batch(model, {"image": x, "mask": torch.zeros(1, 64, 64).long()}, "cpu")
    with pytest.raises(NotImplementedError, match="gradcam"):
        ua.evaluate.evaluate_model(None, [], "cpu", visualize_samples=1)


def test_gradient_at_a_pre_norm_convolution_has_zero_spatial_mean():
    """Conv2d -> InstanceNorm2d(affine) -> LeakyReLU -> mean in fp64: InstanceNorm's backward
    removes the per-(image, channel) mean of its input gradient, so the spatial mean of dL/dy at
    the convolution's output - the Grad-CAM channel weight of that target - is zero up to
    rounding: <= 1e-12 of the mean |gradient|."""
    torch.manual_seed(0)
    conv = nn.Conv2d(5, 8, 3, padding=1).double()
    norm = nn.InstanceNorm2d(8, affine=True).double()
    with torch.no_grad():
        norm.weight.uniform_(0.5, 1.5)
        norm.bias.uniform_(-0.5, 0.5)
    x = torch.randn(3, 5, 12, 9, dtype=torch.float64)
    y = conv(x)
    y.retain_grad()
    out = nn.functional.leaky_relu(norm(y), 0.01)
    (out * torch.randn_like(out)).mean().backward()       # any downstream gradient
    weights = y.grad.mean(dim=(2, 3))
    scale = y.grad.abs().mean(dim=(2, 3))
    assert (scale > 0).all()
    assert (weights.abs() <= 1e-12 * scale).all(), (weights.abs() / scale).max()
