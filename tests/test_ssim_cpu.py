"""CPU (-m "not gpu"): the SSIM feature without a device - an fp64 restatement of the reference's
SSIM against tests/golden/ssim.npz, the blur form of the SSIM gradient that unet_ssim_grad
implements against autograd of that restatement, argument validation and the ABI surface."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

C1, C2 = 0.01 ** 2, 0.03 ** 2


def window1d(size=11, sigma=1.5):
    coords = torch.arange(size, dtype=torch.float64) - (size - 1) / 2
    g = torch.exp(-(coords ** 2) / (2 * sigma ** 2))
    return g / g.sum()


def blur(x, g):
    """Zero-padded 11 x 11 Gaussian blur of [..., H, W] as conv2d(padding=5) (fp64 if x is)."""
    sh = x.shape
    k = (g.view(-1, 1) * g.view(1, -1)).to(x).view(1, 1, 11, 11)
    return F.conv2d(x.reshape(-1, 1, sh[-2], sh[-1]), k, padding=5).reshape(sh)


def moments(x, y, g):
    return blur(x, g), blur(y, g), blur(x * x, g), blur(y * y, g), blur(x * y, g)


def ssim_map(x, y, g=None, c1=C1, c2=C2):
    """The reference's SSIM map (utils/metrics.py calculate_ssim) restated."""
    g = window1d() if g is None else g
    mx, my, exx, eyy, exy = moments(x, y, g)
    sxx, syy, sxy = exx - mx * mx, eyy - my * my, exy - mx * my
    return ((2 * mx * my + c1) * (2 * sxy + c2)) / ((mx * mx + my * my + c1) * (sxx + syy + c2))


def ssim_per_image(x, y, g=None):
    return ssim_map(x, y, g).mean(dim=(1, 2, 3))


def ssim_grad_blur_form(x, y, g=None, c1=C1, c2=C2):
    """d mean(SSIM map over all elements) / dx in the form the kernel computes:
    (G*A + 2x G*B + y G*C) / K with A, B, C the map's derivatives w.r.t. mu_x, E[x^2], E[xy]."""
    g = window1d() if g is None else g
    mx, my, exx, eyy, exy = moments(x, y, g)
    sxx, syy, sxy = exx - mx * mx, eyy - my * my, exy - mx * my
    N1, N2 = 2 * mx * my + c1, 2 * sxy + c2
    D1, D2 = mx * mx + my * my + c1, sxx + syy + c2
    S = N1 * N2 / (D1 * D2)
    A = 2 * my * (N2 - N1) / (D1 * D2) - 2 * mx * S / D1 + 2 * mx * S / D2
    B = -S / D2
    Cc = 2 * N1 / (D1 * D2)
    return (blur(A, g) + 2 * x * blur(B, g) + y * blur(Cc, g)) / x.numel()


def cases(golden):
    g = golden("ssim")
    return g, [str(c) for c in g["cases"]]


def t64(a):
    return torch.from_numpy(np.asarray(a)).double()


def case_inputs(g, tag):
    """(pred, target) fp32 NCHW of a recorded case: the stored 8-bit images as v / 255."""
    return (torch.from_numpy(g[f"pred_u8_{tag}"]).float() / 255,
            torch.from_numpy(g[f"target_u8_{tag}"]).float() / 255)


def grad_errors(grad, g, key, tag):
    """(relative L2 error over the recorded sample of entries, relative error of the L2 norm) of a
    gradient against the fixture's `key` (GRAD_SAMPLES entries at grad_idx_<tag>, and its norm)."""
    flat = grad.detach().reshape(-1).double().cpu()
    ref = t64(g[key])
    got = flat[torch.from_numpy(g[f"grad_idx_{tag}"])]
    norm = float(g[f"{key}_norm"])
    return ((got - ref).norm() / ref.norm()).item(), abs(flat.norm().item() - norm) / norm


def test_window_is_the_references_gaussian_kernel(ua, golden):
    """The 11 taps the kernels receive: their outer product is gaussian_kernel(11, 1.5)."""
    ref = torch.from_numpy(golden("ssim")["window"])
    w = torch.tensor(ua.ops.gaussian_window(11, 1.5), dtype=torch.float32)
    assert torch.equal(w.view(-1, 1) * w.view(1, -1), ref)
    assert torch.allclose(window1d(), w.double(), atol=1e-8, rtol=0)


# the reference's fp32 SSIM itself sits up to 1.24e-5 from fp64 on the structured inputs (the
# cancellation E[x^2] - mu^2 over flat regions; 1.2e-7 on the random ones), so the fixture
# pins the restatement to 2e-5
REF_FP32_SSIM = 2e-5
# likewise its fp32 SSIM gradient: up to 1.78e-4 relative L2 over the sampled entries (1.0e-4 on
# the norm) from fp64 on the structured 8-bit inputs, 1.4e-6 on the random ones
REF_FP32_GRAD = 2e-4


def test_fp64_restatement_matches_the_reference(golden):
    g, names = cases(golden)
    for tag in names:
        x, y = (v.double() for v in case_inputs(g, tag))
        s = ssim_per_image(x, y)
        assert (s - t64(g[f"ssim_{tag}"])).abs().max().item() <= REF_FP32_SSIM, tag
        assert (s - t64(g[f"eval_ssim_{tag}"])).abs().max().item() <= REF_FP32_SSIM, tag
        mse = ((x - y) ** 2).mean(dim=(1, 2, 3))
        assert ((mse - t64(g[f"eval_mse_{tag}"])).abs() / mse).max().item() <= 1e-6, tag
        psnr = 10 * torch.log10(1 / mse)
        assert (psnr - t64(g[f"psnr_{tag}"])).abs().max().item() <= 1e-4, tag
        assert abs(1 - s.mean().item() - float(g[f"ssimloss_1_{tag}"])) <= REF_FP32_SSIM, tag
        assert (1 - s - t64(g[f"ssimloss_0_{tag}"])).abs().max().item() <= REF_FP32_SSIM, tag
        rl = mse.mean() + 0.1 * (1 - s.mean())
        assert abs(rl.item() - float(g[f"reconloss_{tag}"])) <= 0.1 * REF_FP32_SSIM, tag


def test_fp64_autograd_matches_the_reference_gradients(golden):
    g, names = cases(golden)
    for tag in names:
        p, t = case_inputs(g, tag)
        x, y = p.double().requires_grad_(True), t.double()
        (1 - ssim_map(x, y).mean()).backward()
        e_samp, e_norm = grad_errors(x.grad, g, f"ssimloss_grad_1_{tag}", tag)
        assert e_samp <= REF_FP32_GRAD and e_norm <= REF_FP32_GRAD, (tag, e_samp, e_norm)


@pytest.mark.parametrize("shape", [(1, 3, 37, 50), (2, 3, 8, 8)])
def test_blur_form_gradient_equals_autograd(shape):
    """Pins the derivation unet_ssim_grad implements (zero-padded borders included)."""
    gen = torch.Generator().manual_seed(3)
    y = torch.rand(shape, generator=gen, dtype=torch.float64)
    x = (y + 0.2 * torch.randn(shape, generator=gen, dtype=torch.float64)).clamp(0, 1)
    xa = x.clone().requires_grad_(True)
    ssim_map(xa, y).mean().backward()
    got = ssim_grad_blur_form(x, y)
    e = ((got - xa.grad).abs().max() / xa.grad.abs().max()).item()
    assert e <= 1e-10, e


def test_argument_validation(ua):
    x = torch.rand(1, 3, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ua.calculate_ssim(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ua.calculate_psnr(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ua.evaluate_reconstructions(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ua.SSIMLoss()(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ua.ReconstructionLoss(ssim_weight=0.1)(x, x)
    with pytest.raises(NotImplementedError):
        ua.calculate_ssim(x, x, kernel_size=7)
    with pytest.raises(NotImplementedError):
        ua.SSIMLoss(window_size=7)
    with pytest.raises(NotImplementedError):
        ua.ReconstructionLoss(perceptual_weight=0.5)
    with pytest.raises(NotImplementedError):
        ua.ae.evaluate_reconstruction_quality(None, [], "cpu", visualize_samples=4)
    with pytest.raises(ValueError):
        ua.SSIMLoss(target_layout="nhwc")
    assert ua.ReconstructionLoss(ssim_weight=0.0).ssim_loss is None
    assert isinstance(ua.ReconstructionLoss(ssim_weight=0.1).ssim_loss, ua.SSIMLoss)


def test_ssim_symbols_abi_version_and_host_checks(ua):
    handle = ctypes.CDLL(ua.LIB_PATH)
    for name in ("unet_ssim_workspace_bytes", "unet_ssim_fwd", "unet_ssim_grad"):
        assert hasattr(handle, name) and name in ua._lib.SIGNATURES
    lib = ua.lib()
    assert lib.unet_abi_version() == ua._lib.ABI_VERSION == 11
    # 2 doubles per (image, channel, 32 x 32 tile)
    assert lib.unet_ssim_workspace_bytes(8, 3, 512, 512) == 8 * 3 * 256 * 16
    assert lib.unet_ssim_workspace_bytes(1, 3, 37, 50) == 3 * 4 * 16
    assert lib.unet_ssim_workspace_bytes(0, 3, 8, 8) == 0
    g = (ctypes.c_float * 11)(*([1.0 / 11] * 11))
    rc = lib.unet_ssim_fwd(None, None, 0, g, 1e-4, 9e-4, None, None, None, 1.0, 0.0, None, 0,
                           1, 3, 8, 8, None)
    assert rc == -1 and b"null" in lib.unet_last_error()
    rc = lib.unet_ssim_fwd(1, 1, 1, g, 1e-4, 9e-4, 1, 1, None, 1.0, 0.0, 1, 1 << 20, 1, 4, 8, 8,
                           None)
    assert rc == -1 and b"C == 3" in lib.unet_last_error()
    rc = lib.unet_ssim_fwd(1, 1, 0, g, 1e-4, 9e-4, 1, 1, None, 1.0, 0.0, 1, 8, 1, 3, 64, 64, None)
    assert rc == -3 and b"workspace" in lib.unet_last_error()
    rc = lib.unet_ssim_grad(1, 1, 0, g, 1e-4, 9e-4, None, 1, 1.0, 0.0, 1, 1, 3, 8, 8, None)
    assert rc == -1 and b"per-image" in lib.unet_last_error()
