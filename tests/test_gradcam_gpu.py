"""GPU: Grad-CAM on the HIP path.  The three kernels against fp64 torch on the same, already
rounded, inputs; `evaluate.gradcam` on whole batches against tests/golden/gradcam.npz (the
reference's own generate_gradcam_heatmap in float64, recorded by
tests/tools/make_golden_gradcam.py); the equivalence with the stage-level hooks; and everything the
pass must leave alone (gradients, arena, modes).

Error bounds.  Kernels: worst cases of fp32 sums (see each test).  End to end: per target layer
max(1e-4, 4 x the largest distance the reference's OWN fp32 run keeps from its fp64 run over that
layer's cases) - Grad-CAM through many InstanceNorms is ill-conditioned, and this path differs
from the reference's fp32 one only in summation order and the Winograd transforms."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
U = 2.0 ** -24
SLOPE = 0.01


def _load(name):
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(ROOT, "tests", "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GI = _load("gradcam_inputs")
MAPS = [(2, 2), (5, 7), (64, 64)]


def _rand(shape, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(DEV).to(dtype)


# ---- kernels -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [32, 512])
@pytest.mark.parametrize("hw", MAPS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_weights_are_the_spatial_mean(ua, hw, C, dtype):
    """|w - mean_p g| <= K 2^-24 mean_p |g| per (image, channel), K = H W: the worst case of a
    sequential fp32 sum of K terms and one division, which any summation order meets."""
    h, w = hw
    g = _rand((3, h, w, C), 1000 + h * C, dtype)
    got = ua.ops.gradcam_weights(g)
    assert got.shape == (3, C) and got.dtype == torch.float32
    g64 = g.double()
    want, bound = g64.mean(dim=(1, 2)), h * w * U * g64.abs().mean(dim=(1, 2))
    err = (got.double() - want).abs()
    print(f"weights {h}x{w} C={C} {dtype}: max err / bound = {(err / bound).max().item():.3f}")
    assert (err <= bound).all()
    assert torch.equal(got, ua.ops.gradcam_weights(g))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [32, 512])
@pytest.mark.parametrize("hw", MAPS, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("activated", [True, False], ids=["act", "plain"])
def test_map_is_the_rectified_weighted_sum(ua, activated, hw, C, dtype):
    """|cam - relu(sum_c w_c a_c)| <= (C + 1) 2^-24 sum_c |w_c a_c| per pixel (C products and
    sums, the activation's roundings); a = lrelu(x alpha + beta) formed on load, or x itself."""
    h, w = hw
    x = _rand((3, h, w, C), 2000 + h * C, dtype)
    wts = _rand((3, C), 2001 + h * C)
    x64, w64 = x.double(), wts.double()
    if activated:
        alpha = 1.0 + 0.3 * _rand((3, C), 2002 + C)
        beta = 0.5 * _rand((3, C), 2003 + C)
        src = ua.ops.Act(x, alpha.contiguous(), beta.contiguous())
        z = x64 * alpha.double()[:, None, None, :] + beta.double()[:, None, None, :]
        a64 = torch.where(z > 0, z, z * float(np.float32(SLOPE)))
    else:
        src, a64 = x, x64
    cam, _ = ua.ops.gradcam_map(src, SLOPE, wts)
    assert cam.shape == (3, h, w) and cam.dtype == torch.float32
    terms = w64[:, None, None, :] * a64
    want, bound = terms.sum(dim=3).clamp_min(0), (C + 1) * U * terms.abs().sum(dim=3)
    err = (cam.double() - want).abs()
    print(f"map {h}x{w} C={C} {dtype} act={activated}: max err / bound = "
          f"{(err / bound).max().item():.3f}")
    assert (err <= bound).all()
    assert (cam >= 0).all()
    assert torch.equal(cam, ua.ops.gradcam_map(src, SLOPE, wts)[0])


def _heatmap_of(ua, cam, size):
    """unet_gradcam_heatmap of a given non-negative map [N, h, w]: the map travels through
    unet_gradcam_map as channel 0 of a plain 4-channel tensor with weights (1, 0, 0, 0), which
    reproduces it exactly and leaves its minima / maxima in the workspace."""
    N, h, w = cam.shape
    x = torch.zeros((N, h, w, 4), device=DEV)
    x[..., 0] = cam
    wts = torch.zeros((N, 4), device=DEV)
    wts[:, 0] = 1.0
    got, ws = ua.ops.gradcam_map(x, SLOPE, wts)
    assert torch.equal(got, cam)
    return ua.ops.gradcam_heatmap(got, ws, size)


def _reference_heatmap(cam, size):
    """utils/visualize.py:431-437 per image, in fp64."""
    cam = cam.double()
    cam = cam - cam.amin(dim=(1, 2), keepdim=True)
    mx = cam.amax(dim=(1, 2), keepdim=True)
    cam = torch.where(mx != 0, cam / torch.where(mx != 0, mx, torch.ones_like(mx)), cam)
    return F.interpolate(cam.unsqueeze(1), size=size, mode="bilinear", align_corners=False)[:, 0]


@pytest.mark.parametrize("hw,size", [((2, 2), (64, 64)), ((5, 7), (40, 56)), ((64, 64), (64, 64))],
                         ids=["2x2to64x64", "5x7to40x56", "64x64same"])
def test_heatmap_normalises_per_image_and_resizes(ua, hw, size):
    cam = _rand((3,) + hw, 3000 + hw[0]).abs() * torch.tensor([0.01, 1.0, 300.0], device=DEV).view(3, 1, 1)
    got = _heatmap_of(ua, cam, size)
    assert got.shape == (3,) + size and got.dtype == torch.float32
    err = (got.double() - _reference_heatmap(cam, size)).abs().max().item()
    print(f"heatmap {hw} -> {size}: max err {err:.2e}")
    assert err <= 1e-6
    assert got.min().item() >= 0.0 and got.max().item() <= 1.0


@pytest.mark.parametrize("hw,size", [((2, 2), (64, 64)), ((5, 7), (40, 56)), ((64, 64), (64, 64))],
                         ids=["2x2to64x64", "5x7to40x56", "64x64same"])
def test_heatmap_zero_guard_and_exact_one(ua, hw, size):
    """An all-zero map and a constant positive map give all zeros (no NaN, nothing divided); a map
    with one positive pixel reaches exactly 1 at that pixel - all in ONE batch, so the minima and
    maxima are per image."""
    cam = torch.zeros((3,) + hw, device=DEV)
    cam[1] = 0.7
    cam[2, 0, 0] = 3e-5          # output pixel (0, 0) samples source pixel (0, 0) alone
    got = _heatmap_of(ua, cam, size)
    assert torch.isfinite(got).all()
    assert not got[0].any() and not got[1].any()
    assert got[2, 0, 0].item() == 1.0 and got[2].max().item() == 1.0


# ---- end to end ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold(golden):
    g = golden("gradcam")
    return g, GI.layer_bounds(g)


@pytest.fixture(scope="module")
def inputs():
    return {name: GI.images(name).to(DEV) for name in GI.BATCHES}


def _model(ua, precision="fp32"):
    model = ua.UNet()
    model.load_state_dict(GI.state_dict())
    model = model.to(DEV).eval()
    model.matmul_precision = precision
    return model


@pytest.fixture(scope="module")
def model(ua):
    return _model(ua)


@pytest.fixture(scope="module")
def model_x3(ua):
    return _model(ua, "bf16x3")


def _case_error(ua, m, inputs, g, case, **kw):
    name, batch, layer, cls = case
    heat = ua.evaluate.gradcam(m, inputs[batch], cls, GI.target_module(m, layer), **kw)
    want = torch.from_numpy(g[f"heat_{name}"]).to(DEV)
    assert heat.shape == want.shape and heat.dtype == torch.float32 and heat.is_cuda
    return heat, (heat.double() - want.double()).abs().amax(dim=(1, 2))


@pytest.mark.parametrize("case", GI.CASES, ids=[c[0] for c in GI.CASES])
def test_fixture_cases_fp32(ua, model, inputs, gold, case):
    g, bounds = gold
    heat, err = _case_error(ua, model, inputs, g, case)
    bound = bounds[GI.layer_key(case[2])]
    print(f"gradcam fp32 {case[0]}: per-image max err {[f'{e:.2e}' for e in err.tolist()]}, "
          f"bound {bound:.2e}, reference fp32 {float(g['ref32_err_' + case[0]]):.2e}")
    assert err.max().item() <= bound
    assert heat.min().item() >= 0.0 and heat.max().item() <= 1.0


@pytest.mark.parametrize("case", GI.CASES, ids=[c[0] for c in GI.CASES])
def test_fixture_cases_bf16x3(ua, model_x3, inputs, gold, case):
    """The split-bf16 operand mode (precision=None: the model's own mode) at the fp32 bounds."""
    g, bounds = gold
    heat, err = _case_error(ua, model_x3, inputs, g, case, precision=None)
    bound = bounds[GI.layer_key(case[2])]
    print(f"gradcam bf16x3 {case[0]}: per-image max err {[f'{e:.2e}' for e in err.tolist()]}, "
          f"bound {bound:.2e}")
    assert model_x3.matmul_precision == "bf16x3"
    assert err.max().item() <= bound


def test_zero_maps_are_exactly_zero_beside_a_live_one(ua, model, inputs, gold):
    g, bounds = gold
    case = next(c for c in GI.CASES if c[0] == GI.ZERO_CASE)
    heat, err = _case_error(ua, model, inputs, g, case)
    want = g[f"heat_{GI.ZERO_CASE}"]
    zero = [not want[b].any() for b in range(want.shape[0])]
    assert any(zero) and not all(zero)
    for b, z in enumerate(zero):
        if z:
            assert not heat[b].any(), f"image {b} must be exactly zero"
        else:
            assert heat[b].max().item() == 1.0
            assert err[b].item() <= bounds[GI.layer_key(case[2])]
    assert torch.isfinite(heat).all()


@pytest.mark.parametrize("case", [GI.CASES[0], GI.CASES[7], GI.CASES[9]],
                         ids=lambda c: c[0])
def test_two_calls_are_bit_identical(ua, model, inputs, case):
    name, batch, layer, cls = case
    t = GI.target_module(model, layer)
    a = ua.evaluate.gradcam(model, inputs[batch], cls, t)
    b = ua.evaluate.gradcam(model, inputs[batch], cls, t)
    assert torch.equal(a, b)


def test_default_target_and_conv_block_alias(ua, model, inputs):
    x = inputs["sq"]
    a = ua.evaluate.gradcam(model, x, 2)
    assert torch.equal(a, ua.evaluate.gradcam(model, x, 2, model.decoder_stages[0]))
    assert torch.equal(a, ua.evaluate.gradcam(model, x, 2, model.decoder_stages[0].conv_block))


def test_generate_gradcam_heatmap_has_the_references_contract(ua, model, inputs, gold):
    g, bounds = gold
    x = inputs["wide"]
    t = model.decoder_stages[2]
    one = ua.evaluate.generate_gradcam_heatmap(model, x[1:2].cpu(), 2, t, DEV)
    assert isinstance(one, np.ndarray) and one.shape == (64, 128) and one.dtype == np.float32
    batched = ua.evaluate.gradcam(model, x, 2, t)[1].cpu().numpy()
    bound = bounds["decoder_stages[2]"]
    assert np.abs(one.astype(np.float64) - batched).max() <= bound
    assert np.abs(one.astype(np.float64) - g["heat_wide_dec2_c2"][1]).max() <= bound


@pytest.mark.parametrize("layer", [("decoder", 0), ("encoder", 3), ("decoder", -1)],
                         ids=GI.layer_key)
def test_equals_the_formula_on_the_stage_level_hook_tensors(ua, model, inputs, gold, layer):
    """The feature map and gradient the existing stage-level hooks hand out, one image at a time
    with out[0, c].mean().backward(), through the reference's formula in torch."""
    _, bounds = gold
    x, cls = inputs["sq"], 1
    t = GI.target_module(model, layer)
    got = {}
    h1 = t.register_forward_hook(lambda m, i, o: got.__setitem__("a", o.detach()))
    h2 = t.register_full_backward_hook(lambda m, gi, go: got.__setitem__("g", go[0].detach()))
    want = []
    try:
        for b in range(x.shape[0]):
            out = model(x[b:b + 1])
            out[0, cls].mean().backward()
            cam = F.relu((got["g"].mean(dim=(2, 3), keepdim=True) * got["a"]).sum(dim=1))
            cam = cam - cam.min()
            if cam.max() != 0:
                cam = cam / cam.max()
            want.append(F.interpolate(cam.unsqueeze(1), size=x.shape[2:], mode="bilinear",
                                      align_corners=False)[0, 0])
    finally:
        h1.remove()
        h2.remove()
        model.zero_grad()
    heat = ua.evaluate.gradcam(model, x, cls, t)
    err = (heat - torch.stack(want)).abs().max().item()
    print(f"gradcam vs hook formulation {GI.layer_key(layer)}: max err {err:.2e}")
    assert err <= bounds[GI.layer_key(layer)]


def test_leaves_gradients_arena_and_modes_alone(ua, inputs):
    """Sentinel in every .grad and in the arena, train mode, a dropout-mask override: all as they
    were after the call, and the next two train_steps (gradients, momentum) are bit-identical to
    a twin's that never called gradcam."""
    from oracle import unet_ref as O
    img, tgt = O.synthetic_batch(11, 2, 64, 64)
    img, tgt = img.to(DEV), tgt.to(DEV)
    masks = O.draw_dropout_masks(5, 2)
    losses = []
    for call in (True, False):
        m = _model(ua).train()
        m.dropout_mask_override = masks
        opt, lossf = ua.create_optimizer(m), ua.get_loss_function()
        first = ua.train_step(m, opt, lossf, img, tgt)       # arena, momentum and .grad exist
        _, grad_arena = m.flat_parameters()
        grad_arena.fill_(1.25)
        for p in m.parameters():
            p.grad.fill_(1.25)
        grads = [p.grad for p in m.parameters()]
        if call:
            for target in (None, m.encoder_stages[2], m.decoder_stages[-1]):
                heat = ua.evaluate.gradcam(m, inputs["sq"], 1, target)
                assert torch.isfinite(heat).all()
            assert m.training and all(s.training for s in m.modules())
            assert m.dropout_mask_override is masks and m.matmul_precision == "fp32"
            assert (m.flat_parameters()[1] == 1.25).all()
            for p, gp in zip(m.parameters(), grads):
                assert p.grad is gp and (p.grad == 1.25).all()
        losses.append((first, ua.train_step(m, opt, lossf, img, tgt),
                       ua.train_step(m, opt, lossf, img, tgt)))
    for a, b in zip(*losses):
        assert torch.equal(a, b)


def test_bf16_model_runs_fp32_by_default_and_its_own_mode_on_request(ua, inputs, gold):
    g, bounds = gold
    m = _model(ua, "bf16")
    for case in (GI.CASES[1], GI.CASES[6]):
        heat, err = _case_error(ua, m, inputs, g, case)
        assert m.matmul_precision == "bf16"
        assert err.max().item() <= bounds[GI.layer_key(case[2])]
        own, err16 = _case_error(ua, m, inputs, g, case, precision=None)
        assert m.matmul_precision == "bf16"
        assert torch.isfinite(own).all() and own.min().item() >= 0.0 and own.max().item() <= 1.0
        print(f"gradcam bf16 pipeline {case[0]}: per-image max err vs fp64 "
              f"{[f'{e:.2e}' for e in err16.tolist()]} (reported, not bounded)")
    # the model still steps in its own mode afterwards
    assert torch.isfinite(m(inputs["sq"])).all()


def test_gradcam_batch_reports_the_images_that_hold_the_class(ua, model):
    from oracle import unet_ref as O
    seed, n, h, w = GI.BATCHES["sq"]
    img, mask = O.synthetic_batch(seed, n, h, w)
    for cls in (1, 2):
        heat, present = ua.evaluate.gradcam_batch(model, {"image": img, "mask": mask}, DEV,
                                                  target_class=cls)
        assert present.is_cuda and present.dtype == torch.bool
        assert present.tolist() == [bool((mask[b] == cls).any()) for b in range(n)]
        assert torch.equal(heat, ua.evaluate.gradcam(model, img.to(DEV), cls))
    assert 0 < sum((mask[b] == 1).any().item() for b in range(n)) < n or \
        0 < sum((mask[b] == 2).any().item() for b in range(n)) < n
