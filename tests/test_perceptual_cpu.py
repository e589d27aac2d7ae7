"""CPU (-m "not gpu"): the perceptual (VGG16 feature) loss without a device - the ABI surface, the
module tree and its initialisation against the stand-in trunk, every host-side refusal, and an fp64
restatement of the reference's PerceptualLoss (one pass with taps) against
tests/golden/perceptual.npz with the trunk weights rebuilt from their seed."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


V = _load("vgg_inputs", ["tools", "vgg_inputs.py"])

SYMBOLS = ("unet_perceptual_prep", "unet_relu_maxpool2x2_fwd", "unet_feature_mse_fwd",
           "unet_perceptual_relu_bwd", "unet_perceptual_stem_bwd_data")
# the restatement is the reference's arithmetic in fp64 up to the order of its sums (one pass with
# taps instead of four prefix passes): its distance from the recorded fp32 values is the recorded
# fp32-vs-fp64 distance up to fp64 rounding
FP64_SLACK = 1e-9


def restatement(p, t, weights, layers):
    """PerceptualLoss.forward (models/losses.py:138-168) restated as ONE pass over the trunk with
    taps, in the dtype of p: (loss, [per-layer MSE in the order of `layers`])."""
    mean = torch.tensor(V.MEAN, dtype=torch.float32).to(p.dtype).view(1, 3, 1, 1)
    std = torch.tensor(V.STD, dtype=torch.float32).to(p.dtype).view(1, 3, 1, 1)
    names = [n for n in (V.DEFAULT_LAYERS if layers is None else layers) if n in V.LAYER_MAP]
    names = list(dict.fromkeys(names))
    taps = {V.LAYER_MAP[n]: n for n in names}
    by_idx = {idx: (w.to(p.dtype), b.to(p.dtype)) for idx, w, b in weights}
    x = torch.cat([(p - mean) / std, (t - mean) / std])
    N = p.shape[0]
    mse, idx = {}, 0
    for v in V.CFG:
        if v == "M":
            x = F.max_pool2d(x, 2, 2)
            idx += 1
            continue
        w, b = by_idx[idx]
        x = F.relu(F.conv2d(x, w, b, padding=1))
        if idx + 1 in taps:
            mse[taps[idx + 1]] = ((x[:N] - x[N:].detach()) ** 2).mean()
        idx += 2
        if len(mse) == len(names):
            break
    per_layer = [mse[n] for n in names]
    return sum(per_layer) / len(per_layer), per_layer


@pytest.fixture(scope="module")
def weights():
    return V.trunk_weights(V.convs_needed(None))


def test_symbols_header_bindings_and_abi_version(ua):
    handle = ctypes.CDLL(ua.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    for name in SYMBOLS + ("unet_feature_mse_workspace_bytes",):
        assert hasattr(handle, name), name
        assert name in ua._lib.SIGNATURES, name
        assert name + "(" in header, name
    lib = ua.lib()
    assert lib.unet_abi_version() == ua._lib.ABI_VERSION == 11
    # one double per (image pair, workgroup): at most 256 workgroups an image, one per 2048 float4
    assert lib.unet_feature_mse_workspace_bytes(8, 512, 512, 64) == 8 * 256 * 8
    assert lib.unet_feature_mse_workspace_bytes(2, 4, 4, 32) == 2 * 8
    assert lib.unet_feature_mse_workspace_bytes(0, 4, 4, 32) == 0


def test_entry_points_refuse_bad_arguments(ua):
    lib = ua.lib()
    m = (ctypes.c_float * 3)(*V.MEAN)
    s = (ctypes.c_float * 3)(*V.STD)
    assert lib.unet_perceptual_prep(None, None, 0, m, s, None, 1, 8, 8, None) == -1
    assert b"null" in lib.unet_last_error()
    assert lib.unet_relu_maxpool2x2_fwd(1, 1, 2, 1, 8, 32, None) == -1
    assert lib.unet_relu_maxpool2x2_fwd(1, 1, 2, 8, 8, 48, None) == -1
    assert b"C % 32" in lib.unet_last_error()
    assert lib.unet_feature_mse_fwd(1, 1, 1, 8, 2, 64, 64, 64, None) == -3
    assert b"workspace" in lib.unet_last_error()
    assert lib.unet_perceptual_relu_bwd(1, None, 0.0, 1, 1, 1, 1, 8, 8, 32, None) == -1
    assert b"exclusive" in lib.unet_last_error()
    assert lib.unet_perceptual_relu_bwd(1, None, 0.0, None, None, 1, 1, 8, 8, 32, None) == -1
    assert lib.unet_perceptual_stem_bwd_data(1, 1, s, 1, 1, 8, 8, 3, None) == -1
    assert b"Cout % 32" in lib.unet_last_error()


def test_module_tree_matches_the_reference(ua, golden):
    g = golden("perceptual")
    pl = ua.PerceptualLoss()
    assert list(pl.state_dict().keys()) == [str(k) for k in g["state_dict_keys"]]
    assert all(not p.requires_grad for p in pl.parameters())
    assert not pl.training
    assert list(pl.features.keys()) == V.DEFAULT_LAYERS
    # prefixes share one set of stock modules
    assert pl.features["relu1_2"][0] is pl.features["relu4_3"][0]
    assert len(pl.features["relu4_3"]) == 23
    assert torch.equal(pl.mean.flatten(), torch.tensor(V.MEAN))
    assert torch.equal(pl.std.flatten(), torch.tensor(V.STD))
    assert ua.PerceptualLoss is ua.losses.PerceptualLoss and "PerceptualLoss" in ua.__all__


def test_initialisation_is_the_stand_in_trunks_draw(ua):
    """torch.manual_seed(s); ua.PerceptualLoss() draws what the stand-in for
    torchvision.models.vgg16(weights=None) draws under the same seed."""
    torch.manual_seed(5)
    pl = ua.PerceptualLoss()
    torch.manual_seed(5)
    stub = V.stub_features()
    sd = pl.state_dict()
    for idx in (0, 2, 5, 7, 10, 12, 14, 17, 19, 21):
        assert torch.equal(sd[f"features.relu4_3.{idx}.weight"], stub[idx].weight), idx
        assert torch.count_nonzero(sd[f"features.relu4_3.{idx}.bias"]) == 0
    torch.manual_seed(5)
    shallow = ua.PerceptualLoss(layers=["relu1_1"])
    assert torch.equal(shallow.state_dict()["features.relu1_1.0.weight"], stub[0].weight)
    assert list(shallow.state_dict().keys()) == ["mean", "std", "features.relu1_1.0.weight",
                                                 "features.relu1_1.0.bias"]


def test_layer_selection(ua):
    pl = ua.PerceptualLoss(layers=["relu2_2", "nonsense", "relu1_1"])
    assert list(pl.features.keys()) == ["relu2_2", "relu1_1"]     # unknown names are skipped
    assert len(pl._trunk) == 4 and pl._pools == 1
    assert [t for _, t, _ in pl._trunk] == [1, None, None, 0]
    deep = ua.PerceptualLoss(layers=["relu5_3"])
    assert len(deep._trunk) == 13 and deep._pools == 4
    with pytest.raises(ValueError, match="no valid"):
        ua.PerceptualLoss(layers=["conv1_1"])
    with pytest.raises(ValueError, match="no valid"):
        ua.PerceptualLoss(layers=[])


def test_host_side_refusals(ua):
    x = torch.rand(1, 3, 16, 16)
    pl = ua.PerceptualLoss()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pl(x, x)
    with pytest.raises(ValueError, match="poolings"):      # relu4_3 sits behind 3 pools: >= 8
        pl(x[:, :, :7, :], x[:, :, :7, :])
    with pytest.raises(ValueError, match="poolings"):
        pl(x[:, :, :, :4], x[:, :, :, :4])
    with pytest.raises(RuntimeError, match="no CPU fallback"):   # 8 x 8 passes the size check
        pl(x[:, :, :8, :8], x[:, :, :8, :8])
    for prec in ("bf16", "bf16x3", True, 3):
        with pytest.raises(NotImplementedError):
            ua.PerceptualLoss(precision=prec)
    with pytest.raises(ValueError):
        ua.PerceptualLoss(target_layout="nhwc")
    with pytest.raises(ValueError):
        ua.PerceptualLoss(chunk=0)


def test_reconstruction_loss_takes_the_callers_network(ua):
    with pytest.raises(NotImplementedError, match="perceptual=ua.PerceptualLoss"):
        ua.ReconstructionLoss(perceptual_weight=0.5)
    pl = ua.PerceptualLoss(layers=["relu1_2"])
    rl = ua.ReconstructionLoss(perceptual_weight=0.5, perceptual=pl)
    assert rl.perceptual_loss is pl and rl.perceptual_weight == 0.5
    assert "perceptual_loss.features.relu1_2.0.weight" in rl.state_dict()
    assert ua.ReconstructionLoss(perceptual_weight=0.0, perceptual=pl).perceptual_loss is None
    with pytest.raises(TypeError):
        ua.ReconstructionLoss(perceptual_weight=0.5, perceptual=torch.nn.Identity())
    with pytest.raises(ValueError):
        ua.ReconstructionLoss(perceptual_weight=0.5, perceptual=pl, target_layout="nhwc_u8")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rl(torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 16))
    full = ua.ae.get_reconstruction_loss(1.0, 0.1, 0.1, perceptual_layers=["relu1_1"])
    assert isinstance(full.perceptual_loss, ua.PerceptualLoss)
    assert list(full.perceptual_loss.features.keys()) == ["relu1_1"]
    assert isinstance(full.ssim_loss, ua.SSIMLoss)
    assert ua.ae.get_reconstruction_loss(1.0, 0.0, 0.0).perceptual_loss is None
    assert isinstance(ua.ae.get_loss_function(), ua.MSELoss)     # unchanged


def test_seeded_weights_match_the_pinned_samples(golden, weights):
    g = golden("perceptual")
    assert int(g["seed_w"]) == V.SEED_W
    pins = V.pin_weights(weights)
    assert len(pins) == 10 * 2 * 3
    for key, val in pins.items():
        assert np.array_equal(np.asarray(val), g[key]), key
    # loading them into the module puts them where the kernels read them
    import unet_implementations_amd as ua
    pl = V.load_trunk(ua.PerceptualLoss(), weights)
    assert torch.equal(pl._trunk[3][0].weight, weights[3][1])
    assert torch.equal(pl._trunk[9][0].bias, weights[9][2])


def test_fp64_restatement_reproduces_the_fixture(golden, weights):
    g = golden("perceptual")
    tags = [str(c) for c in g["cases"]]
    assert tags == list(V.CASES)
    for tag in tags:
        shape, layers, kind, seed = V.CASES[tag]
        pu, tu = V.case_inputs(shape, kind, seed)
        assert np.array_equal(pu.numpy(), g[f"pred_u8_{tag}"]), tag
        assert np.array_equal(tu.numpy(), g[f"target_u8_{tag}"]), tag
        p, t = V.operands(g, tag)
        x = p.double().requires_grad_(True)
        loss, per_layer = restatement(x, t.double(), weights, layers)
        loss.backward()
        e_loss = float(g[f"ref_loss_err_{tag}"])
        e_grad = float(g[f"ref_grad_err_{tag}"])
        ref = float(g[f"loss_{tag}"])
        print(tag, "loss err", abs(loss.item() - ref) / ref, "recorded", e_loss)
        assert abs(loss.item() - ref) <= (e_loss + FP64_SLACK) * ref, tag
        assert [str(n) for n in g[f"layers_{tag}"]] == \
            [n for n in (layers or V.DEFAULT_LAYERS) if n in V.LAYER_MAP]
        for got, want in zip(per_layer, g[f"layer_mse_{tag}"]):
            assert abs(got.item() - float(want)) <= 1e-6 * float(want), tag
        e_s, e_n = V.grad_errors(x.grad, g[f"grad_{tag}"], g[f"grad_idx_{tag}"],
                                 g[f"grad_norm_{tag}"])
        print(tag, "grad err", e_s, e_n, "recorded", e_grad)
        assert e_s <= e_grad + FP64_SLACK and e_n <= e_grad + FP64_SLACK, (tag, e_s, e_n)


def test_one_pass_with_taps_equals_the_prefix_passes(weights):
    """The reference evaluates four prefix Sequentials; one pass with taps has the same value and
    gradient (fp64, to rounding).  A check of the oracle only: it runs the restatement of this file
    against the stand-in trunk, no product code, and holds on any commit."""
    pu, tu = V.case_inputs((1, 3, 16, 16), "random", 3)
    p, t = pu.double() / 255, tu.double() / 255
    mean = torch.tensor(V.MEAN).double().view(1, 3, 1, 1)
    std = torch.tensor(V.STD).double().view(1, 3, 1, 1)
    stub = V.stub_features().double()
    for idx, w, b in weights:
        stub[idx].weight.data.copy_(w)
        stub[idx].bias.data.copy_(b)
    x = p.clone().requires_grad_(True)
    total = 0.0
    for name in V.DEFAULT_LAYERS:
        prefix = stub[: V.LAYER_MAP[name] + 1]
        with torch.no_grad():
            ft = prefix((t - mean) / std)
        total = total + F.mse_loss(prefix((x - mean) / std), ft)
    (total / 4).backward()
    y = p.clone().requires_grad_(True)
    loss, _ = restatement(y, t, weights, None)
    loss.backward()
    assert abs(loss.item() - (total / 4).item()) <= 1e-13 * loss.item()
    assert ((x.grad - y.grad).norm() / x.grad.norm()).item() <= 1e-12
