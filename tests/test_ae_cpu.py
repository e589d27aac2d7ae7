"""CPU (-m "not gpu"): the autoencoder pretraining surface - model structure, configuration
checks, FusedAdam argument validation, the LR schedule, the recon / MSE / Adam ABI's argument
checks and the reproducibility of the ae64 fixture's seeded inputs."""
import importlib.util
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location(
        "make_golden_ae", os.path.join(ROOT, "tests", "tools", "make_golden_ae.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_autoencoder_state_dict_matches_fixture_keys(ua, golden):
    g = golden("ae64")
    model = ua.Autoencoder()
    sd = model.state_dict()
    assert list(sd) == [str(k) for k in g["param_names"]]
    assert "segmentation_output.weight" not in sd
    assert tuple(sd["reconstruction_output.0.weight"].shape) == (3, 32, 3, 3)
    assert tuple(sd["reconstruction_output.0.bias"].shape) == (3,)
    # the shapes are the recorder's (reference) weights'
    ref = _recorder().ae_state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in ref.items()}
    model.load_state_dict(ref)
    # parameter registration order = state_dict order = arena order
    assert [n for n, _ in model.named_parameters()] == list(sd)
    assert model.out_channels == 3 and not hasattr(model, "num_classes")
    assert model.input_mean == (0.0, 0.0, 0.0) and model.input_std == (1.0, 1.0, 1.0)


def test_autoencoder_reference_api(ua):
    model = ua.ae.create_model("cpu")
    assert model.get_encoder() is model.encoder_stages
    dec, head = model.get_decoder()
    assert dec is model.decoder_stages and head is model.reconstruction_output
    rates = [m.drop_prob for m in model.modules() if isinstance(m, ua.SpatialDropout2d)]
    assert rates == [0.05] * 2 + [0.1] * 2 + [0.15] * 4 + [0.15] * 2 + [0.1] * 4 + [0.05] * 2
    # initialize_weights: Kaiming conv weights, zero biases, unit / zero InstanceNorm affine
    assert torch.all(model.reconstruction_output[0].bias == 0)
    assert torch.all(model.encoder_stages[0].block[1].weight == 1)


def test_check_supported(ua):
    assert ua.Autoencoder().check_supported()
    m = ua.Autoencoder()
    m.reconstruction_output[0] = torch.nn.Conv2d(32, 3, 1)
    with pytest.raises(NotImplementedError, match="32 -> 3 3x3"):
        m.check_supported()
    m = ua.Autoencoder()
    m.reconstruction_output[1] = torch.nn.Tanh()
    with pytest.raises(NotImplementedError, match="Sigmoid"):
        m.check_supported()
    m = ua.Autoencoder(out_channels=4)
    with pytest.raises(NotImplementedError):
        m.check_supported()
    # the segmentation UNet keeps its own head check
    assert ua.UNet().check_supported()


def test_hook_on_inner_head_module_is_rejected(ua):
    m = ua.Autoencoder()
    m.reconstruction_output[0].register_forward_hook(lambda *a: None)
    with pytest.raises(NotImplementedError, match="reconstruction_output.0"):
        m._check_hooks()
    m = ua.Autoencoder()
    m.reconstruction_output.register_forward_hook(lambda *a: None)
    m._check_hooks()      # the head module itself is a stage-level module


def test_fused_adam_argument_validation(ua):
    ps = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(NotImplementedError, match="amsgrad"):
        ua.FusedAdam(ps, amsgrad=True)
    with pytest.raises(NotImplementedError, match="maximize"):
        ua.FusedAdam(ps, maximize=True)
    with pytest.raises(NotImplementedError, match="decoupled"):
        ua.FusedAdam(ps, decoupled_weight_decay=True)
    with pytest.raises(ValueError):
        ua.FusedAdam(ps, lr=-1.0)
    with pytest.raises(ValueError):
        ua.FusedAdam(ps, betas=(1.0, 0.999))
    with pytest.raises(ValueError):
        ua.FusedAdam(ps, eps=-1e-8)
    with pytest.raises(ValueError):
        ua.FusedAdam(ps, weight_decay=-1e-5)
    with pytest.raises(NotImplementedError, match="one parameter group"):
        ua.FusedAdam([{"params": ps}, {"params": [torch.nn.Parameter(torch.zeros(2))]}])
    opt = ua.FusedAdam(ps, lr=2e-3, betas=(0.8, 0.99), eps=1e-7, weight_decay=1e-5)
    ref = torch.optim.Adam([torch.nn.Parameter(torch.zeros(3))], lr=2e-3, betas=(0.8, 0.99),
                           eps=1e-7, weight_decay=1e-5)
    # torch's param_groups layout: checkpoints interchange
    assert opt.state_dict()["param_groups"] == ref.state_dict()["param_groups"]


def test_fused_adam_state_dict_loads_torch_adam_layout(ua):
    p = torch.nn.Parameter(torch.randn(5))
    ref = torch.optim.Adam([p], lr=1e-3, weight_decay=1e-5)
    p.grad = torch.randn(5)
    ref.step()
    ref.step()
    opt = ua.FusedAdam([torch.nn.Parameter(p.detach().clone())], lr=1e-3, weight_decay=1e-5)
    opt.load_state_dict(ref.state_dict())
    assert opt._steps == 2
    sd = opt.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    assert float(sd["state"][0]["step"]) == 2.0
    back = torch.optim.Adam([torch.nn.Parameter(torch.zeros(5))], lr=1e-3, weight_decay=1e-5)
    back.load_state_dict(sd)
    assert torch.equal(back.state_dict()["state"][0]["exp_avg"], ref.state_dict()["state"][0]["exp_avg"])


def test_ae_lr_schedule_is_the_references(ua):
    p = [torch.nn.Parameter(torch.zeros(4))]
    opt = ua.FusedAdam(p, lr=1e-3, weight_decay=1e-5)
    sched = ua.ae.create_lr_scheduler(opt, 10)
    assert isinstance(sched, torch.optim.lr_scheduler.CosineAnnealingLR)
    ref_opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(4))], lr=1e-3, weight_decay=1e-5)
    ref = torch.optim.lr_scheduler.CosineAnnealingLR(ref_opt, T_max=10, eta_min=1e-6)
    got, want = [], []
    for _ in range(12):
        got.append(opt.param_groups[0]["lr"])
        want.append(ref_opt.param_groups[0]["lr"])
        sched.step()
        ref.step()
    assert got == want
    assert abs(min(got) - 1e-6) < 1e-12 and got[0] == 1e-3


def test_ae_optimizer_and_loss_factories(ua):
    model = ua.ae.create_model("cpu")
    opt = ua.ae.create_optimizer(model)
    g = opt.param_groups[0]
    assert isinstance(opt, ua.FusedAdam) and g["lr"] == 1e-3 and g["weight_decay"] == 1e-5
    assert g["betas"] == (0.9, 0.999) and g["eps"] == 1e-8
    lossf = ua.ae.get_loss_function()
    assert isinstance(lossf, ua.MSELoss) and lossf.reduction == "mean"
    for bad in ({"reduction": "sum"}, {"reduction": "none"}):
        with pytest.raises(NotImplementedError):
            ua.MSELoss(**bad)
    with pytest.raises(RuntimeError, match="MI355X"):
        lossf(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4))


def test_recon_abi_argument_validation_without_gpu(ua):
    lib = ua.lib()
    rc = lib.unet_recon3x3_fwd(None, 0, 0.01, None, None, None, 1, 8, 8, 3, None)
    assert rc == -1 and b"null" in lib.unet_last_error()
    src = ua._lib.ActSrc(1, 16, None, None)
    rc = lib.unet_recon3x3_fwd(src, 0, 0.01, 1, 1, 1, 1, 8, 8, 3, None)
    assert rc == -1 and b"C == 32" in lib.unet_last_error()
    src = ua._lib.ActSrc(1, 32, None, None)
    rc = lib.unet_recon3x3_fwd(src, 0, 0.01, 1, 1, 1, 1, 8, 8, 4, None)
    assert rc == -1 and b"K == 3" in lib.unet_last_error()
    rc = lib.unet_recon3x3_bwd(src, 0, 0.01, 1, 1, 1, 1, 1, 1, 1, 16, 2, 64, 64, 3, None, None)
    assert rc == -3 and b"workspace" in lib.unet_last_error()
    assert lib.unet_recon3x3_bwd_workspace_bytes(8, 512, 512) == 1024 * 867 * 4
    assert lib.unet_recon3x3_bwd_workspace_bytes(2, 64, 64) == 32 * 867 * 4
    assert lib.unet_recon3x3_bwd_workspace_bytes(0, 64, 64) == 0
    rc = lib.unet_mse_loss_fwd(1, 1, 1, 1, 1, 1, 1 << 20, 2, 4, 8, 8, None)
    assert rc == -1 and b"uint8" in lib.unet_last_error()
    rc = lib.unet_mse_loss_fwd(1, 1, 0, 1, 1, 1, 0, 2, 3, 8, 8, None)
    assert rc == -3 and b"workspace" in lib.unet_last_error()
    assert lib.unet_mse_loss_workspace_bytes(8, 3, 512, 512) > 0
    rc = lib.unet_mse_loss_grad(None, 1, 0, None, 1, 2, 3, 8, 8, None)
    assert rc == -1 and b"null" in lib.unet_last_error()
    rc = lib.unet_adam_step(1, 1, 1, 1, 0, 1, 1, None)
    assert rc == -1 and b"adam_step" in lib.unet_last_error()


def test_ae_fixture_inputs_are_reproducible_from_their_seeds(golden):
    """make_golden_ae.py's seeded inputs: the same seeds give the same bytes as the stored
    fixture (image, every dropout mask of every step), and the weights are deterministic."""
    g = golden("ae64")
    rec = _recorder()
    u8, img = rec.synthetic_image()
    assert np.array_equal(u8, g["image_u8"])
    for tag in ("", "_s1"):
        for s in range(int(g["steps"])):
            masks = rec.draw_masks(int(g["seed_drop"]) + s)
            for j, m in enumerate(masks):
                assert np.array_equal(m.numpy(), g[f"mask{tag}_{s}_{j}"])
    a, b = rec.ae_state_dict(), rec.ae_state_dict()
    assert list(a) == [str(k) for k in g["param_names"]]
    assert all(torch.equal(a[k], b[k]) for k in a)
