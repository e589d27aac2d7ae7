"""GPU (-m gpu): the perceptual (VGG16 feature) loss on the MI355X - each new kernel alone against
torch / numpy / fp64, the loss and its gradient against the reference's own values
(tests/golden/perceptual.npz) and the fp64 restatement of tests/test_perceptual_cpu.py, kernel
selection, chunking, determinism, the no-grad path, ReconstructionLoss with the term, the AE
trajectory under MSE + 0.1 perceptual and graph capture."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load("perceptual_restatement", ["test_perceptual_cpu.py"])
V = R.V
WINO_FWD = "conv_wino_kernel<true, true, false, false>"
WINO_DGRAD = "conv_wino_kernel<false, false, false, false>"
BWD_KERNELS = ("perceptual_relu_bwd", "perceptual_relu_pool_bwd", "stem_bwd_data")


def _ae_recorder():
    return _load("make_golden_ae", ["tools", "make_golden_ae.py"])


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def randn(shape, seed, dtype=torch.float32):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=dtype)


@pytest.fixture(scope="module")
def weights():
    return V.trunk_weights(V.convs_needed(None))


@pytest.fixture(scope="module")
def losses(ua, weights):
    """PerceptualLoss modules with the seeded trunk on the device, one per layer selection (the
    weights are packed once each)."""
    made = {}

    def get(layers=None, **kw):
        key = (tuple(layers) if layers else None, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = V.load_trunk(ua.PerceptualLoss(layers=layers, **kw), weights).to(DEV)
        return made[key]
    return get


def loss_and_grad(lossf, p, t, scale=None):
    x = p.clone().requires_grad_(True)
    loss = lossf(x, t)
    (loss if scale is None else scale * loss).backward()
    return loss.detach(), x.grad.detach()


# ---------------------------------------------------------------- kernels alone
@pytest.mark.parametrize("shape", [(2, 3, 8, 8), (1, 3, 37, 50)])
@pytest.mark.parametrize("u8", [False, True])
def test_prep_is_bit_equal_to_torch(ua, shape, u8):
    N, _, H, W = shape
    gen = torch.Generator().manual_seed(H)
    out = torch.rand(shape, generator=gen)
    if u8:
        tu = torch.randint(0, 256, (N, H, W, 3), generator=gen, dtype=torch.uint8)
        t_arg, t = tu, (tu.float() / 255).permute(0, 3, 1, 2)
    else:
        t_arg = t = torch.rand(shape, generator=gen)
    mean = torch.tensor(V.MEAN).view(1, 3, 1, 1)
    std = torch.tensor(V.STD).view(1, 3, 1, 1)
    want = torch.cat([(out - mean) / std, (t - mean) / std]).permute(0, 2, 3, 1).contiguous()
    got = ua.ops.perceptual_prep(out.to(DEV), t_arg.to(DEV), u8)
    assert got.shape == (2 * N, H, W, 3)
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("shape", [(3, 6, 10, 32), (2, 7, 9, 64), (2, 64, 64, 64)])
def test_relu_maxpool_is_bit_equal_to_torch(ua, shape):
    y = randn(shape, 1)
    y[0, :2, :2, :] = -1.0         # an all-negative window pools to 0
    want = F.max_pool2d(F.relu(y.permute(0, 3, 1, 2)), 2).permute(0, 2, 3, 1).contiguous()
    got = ua.ops.relu_maxpool2x2_fwd(y.to(DEV))
    assert got.shape == want.shape
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("shape", [(4, 6, 10, 32), (6, 37, 25, 64), (4, 64, 64, 64)])
def test_feature_mse_against_fp64_and_batch_permutation(ua, shape):
    """Each term is two fp32 roundings (the difference of two non-negative values, its square)
    summed in double: relative error <= (1 + 2^-24)^3 - 1 < 2e-7 per term, all terms >= 0."""
    M = shape[0]
    N = M // 2
    y = randn(shape, 2)
    a = F.relu(y.double())
    want = ((a[:N] - a[N:]) ** 2).sum(dim=(1, 2, 3))
    sums = torch.empty(N, dtype=torch.float64, device=DEV)
    ua.ops.feature_mse_fwd(y.to(DEV), sums)
    err = ((sums.cpu() - want).abs() / want).max().item()
    print("feature_mse rel err", shape, err)
    assert err <= 1e-6
    perm = list(range(N))[::-1]
    yp = torch.cat([y[:N][perm], y[N:][perm]])
    sums_p = torch.empty(N, dtype=torch.float64, device=DEV)
    ua.ops.feature_mse_fwd(yp.to(DEV), sums_p)
    assert torch.equal(sums_p.cpu(), sums.cpu()[perm])


def relu_bwd_numpy(yo, yt, coef, g, gp):
    """dz = y_o > 0 ? g_in + coef (relu(y_o) - relu(y_t)) : 0 with gp routed to the first maximum
    of each 2x2 window (row-major), in fp64."""
    yo = yo.astype(np.float64)
    N, H, W, C = yo.shape
    gin = np.zeros_like(yo)
    if g is not None:
        gin += g.astype(np.float64)
    if gp is not None:
        a = np.maximum(yo, 0)
        for yw in range(H // 2):
            for xw in range(W // 2):
                win = a[:, 2 * yw:2 * yw + 2, 2 * xw:2 * xw + 2, :].reshape(N, 4, C)
                first = win.argmax(axis=1)          # numpy: the first maximum
                for q in range(4):
                    gin[:, 2 * yw + q // 2, 2 * xw + q % 2, :] += \
                        np.where(first == q, gp[:, yw, xw, :].astype(np.float64), 0.0)
    if yt is not None:
        gin += coef * (np.maximum(yo, 0) - np.maximum(yt.astype(np.float64), 0))
    return np.where(yo > 0, gin, 0.0)


# (no incoming gradient and no tap is not a layer of the trunk: the entry point refuses it)
@pytest.mark.parametrize("shape", [(2, 6, 10, 32), (2, 7, 9, 64)])
@pytest.mark.parametrize("form,tap", [("same", True), ("same", False), ("pool", True),
                                      ("pool", False), ("none", True)])
def test_relu_bwd_against_numpy_and_autograd(ua, shape, form, tap):
    N, H, W, C = shape
    yo, yt = randn(shape, 3), randn(shape, 4)
    # planted positive ties inside windows (first-maximum routing) and exact zeros
    yo[:, 0, 0, :] = yo[:, 0, 1, :] = 3.0
    yo[:, 2, 3, :] = yo[:, 3, 2, :] = 2.5
    yo[:, 4, 4:6, : C // 2] = 0.0
    yo[:, 4:6, 6:8, C // 2:] = 0.0          # a window of zeros: the gradient goes nowhere
    g = randn(shape, 5) if form == "same" else None
    gp = randn((N, H // 2, W // 2, C), 6) if form == "pool" else None
    coef = 0.37
    got = ua.ops.perceptual_relu_bwd(yo.to(DEV), yt.to(DEV) if tap else None, coef,
                                     g=None if g is None else g.to(DEV),
                                     gp=None if gp is None else gp.to(DEV)).cpu().double()
    want = torch.from_numpy(relu_bwd_numpy(yo.numpy(), yt.numpy() if tap else None, coef,
                                           None if g is None else g.numpy(),
                                           None if gp is None else gp.numpy()))
    scale = want.abs().max().item()
    assert (got - want).abs().max().item() <= 1e-6 * scale
    # CPU autograd of max_pool2d o relu (+ the tap's MSE term) in fp64
    x = yo.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    a = F.relu(x)
    obj = 0.0
    if g is not None:
        obj = obj + (a * g.double().permute(0, 3, 1, 2)).sum()
    if gp is not None:
        obj = obj + (F.max_pool2d(a, 2) * gp.double().permute(0, 3, 1, 2)).sum()
    if tap:
        obj = obj + 0.5 * coef * ((a - F.relu(yt.double().permute(0, 3, 1, 2))) ** 2).sum()
    obj.backward()
    auto = x.grad.permute(0, 2, 3, 1)
    assert (got - auto).abs().max().item() <= 1e-6 * scale
    if gp is not None and not tap:   # an ignored odd row / column receives nothing from the pool
        if H % 2:
            assert torch.count_nonzero(got[:, H - 1]) == 0
        if W % 2:
            assert torch.count_nonzero(got[:, :, W - 1]) == 0


@pytest.mark.parametrize("shape", [(2, 8, 8), (1, 37, 50), (2, 64, 128)])
@pytest.mark.parametrize("cout", [32, 64])
def test_stem_bwd_data_against_fp64(ua, shape, cout):
    """Bound: 4 x the error of torch's own fp32 conv_transpose2d against fp64 on the same inputs
    (floor 1e-6), relative to max |dx|."""
    N, H, W = shape
    dz = randn((N, H, W, cout), 7)
    w = randn((cout, 3, 3, 3), 8) * 0.1
    std = torch.tensor(V.STD)
    dz_nchw = dz.permute(0, 3, 1, 2).contiguous()
    want = F.conv_transpose2d(dz_nchw.double(), w.double(), padding=1) / std.double().view(1, 3, 1, 1)
    own = F.conv_transpose2d(dz_nchw, w, padding=1) / std.view(1, 3, 1, 1)
    scale = want.abs().max().item()
    e_torch = (own.double() - want).abs().max().item() / scale
    got = ua.ops.perceptual_stem_bwd_data(dz.to(DEV), w.to(DEV)).cpu().double()
    e = (got - want).abs().max().item() / scale
    print("stem_bwd_data", shape, cout, "err", e, "torch fp32", e_torch)
    assert got.shape == (N, 3, H, W)
    assert e <= max(4 * e_torch, 1e-6)


# ---------------------------------------------------------------- the loss
@pytest.mark.parametrize("tag", list(V.CASES))
def test_fixture_cases(ua, golden, losses, tag):
    """Loss within max(4 x the reference's own fp32 error, 2e-6); gradient (sampled entries'
    relative L2, and the norm) within max(4 x its own error, 2e-5)."""
    g = golden("perceptual")
    _, layers, _, _ = V.CASES[tag]
    p, t = (v.to(DEV) for v in V.operands(g, tag))
    lossf = losses(layers)
    loss, grad = loss_and_grad(lossf, p, t)
    ref = float(g[f"loss_{tag}"])
    e_loss = abs(loss.item() - ref) / ref
    e_s, e_n = V.grad_errors(grad, g[f"grad_{tag}"], g[f"grad_idx_{tag}"], g[f"grad_norm_{tag}"])
    e_layers = (lossf.last_layer_mse.cpu() - torch.from_numpy(g[f"layer_mse_{tag}"]).double()).abs() \
        / torch.from_numpy(g[f"layer_mse_{tag}"]).double()
    print(tag, "loss err", e_loss, "grad err", e_s, e_n, "layers", e_layers.tolist())
    assert e_loss <= max(4 * float(g[f"ref_loss_err_{tag}"]), 2e-6)
    assert e_layers.max().item() <= 1e-5
    bound = max(4 * float(g[f"ref_grad_err_{tag}"]), 2e-5)
    assert e_s <= bound and e_n <= bound


@pytest.mark.parametrize("n,layers", [(2, ["relu1_2", "relu2_2"]), (4, ["relu1_2"])])
def test_128_against_fp64_and_kernel_selection(ua, weights, losses, n, layers):
    """conv1_2 (64 -> 64 at 128^2) runs the Winograd forward on the 2n stacked images and the
    Winograd data gradient on the n output images exactly when conv_wino_supported says so."""
    pu, tu = V.case_inputs((n, 3, 128, 128), "random", 50 + n)
    p, t = pu.float() / 255, tu.float() / 255
    x = p.double().requires_grad_(True)
    ref, _ = R.restatement(x, t.double(), weights, layers)
    ref.backward()
    lossf = losses(layers)
    with ua.ops.record_launches() as rec:
        loss, grad = loss_and_grad(lossf, p.to(DEV), t.to(DEV))
    e_loss = abs(loss.item() - ref.item()) / ref.item()
    e_grad = rel_l2(grad, x.grad)
    print("128", n, layers, "loss err", e_loss, "grad err", e_grad)
    assert e_loss <= 2e-6 and e_grad <= 2e-5
    fwd = ua.ops.conv_wino_supported(2 * n, 128, 128, 64, 0, 64)
    dgrad = ua.ops.conv_wino_supported(n, 128, 128, 64, 0, 64)
    # conv1_2 is the trunk's largest Winograd-shaped layer (every deeper one has fewer tiles), so
    # a Winograd launch appears in the record exactly when conv1_2's shape is supported; deeper
    # layers may add launches of their own
    assert (sum(WINO_FWD in k for k in rec.names) >= 1) == fwd
    assert (sum(WINO_DGRAD in k for k in rec.names) >= 1) == dgrad
    assert fwd and dgrad == (n == 4)       # the two cases cover both answers of the data gradient
    assert sum("perceptual_stem_bwd_data" in k for k in rec.names) == 1


def test_chunks_agree_with_fp64(ua, weights, losses):
    pu, tu = V.case_inputs((3, 3, 32, 32), "random", 60)
    p, t = pu.float() / 255, tu.float() / 255
    x = p.double().requires_grad_(True)
    ref, _ = R.restatement(x, t.double(), weights, None)
    ref.backward()
    for chunk in (1, 3):
        loss, grad = loss_and_grad(losses(None, chunk=chunk), p.to(DEV), t.to(DEV))
        e_loss = abs(loss.item() - ref.item()) / ref.item()
        e_grad = rel_l2(grad, x.grad)
        print("chunk", chunk, "loss err", e_loss, "grad err", e_grad)
        assert e_loss <= 2e-6 and e_grad <= 2e-5


def test_deterministic_no_grad_path_and_upstream_scale(ua, losses):
    pu, tu = V.case_inputs((2, 3, 32, 32), "random", 61)
    p, t = (pu.float() / 255).to(DEV), (tu.float() / 255).to(DEV)
    lossf = losses(None)
    l1, g1 = loss_and_grad(lossf, p, t)
    l2, g2 = loss_and_grad(lossf, p, t)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    def backward_launches(names):
        return [k for k in names if any(b in k for b in BWD_KERNELS) or "bwd_data" in k]

    # under torch.no_grad() an output that requires grad launches no backward kernel ...
    with ua.ops.record_launches() as rec, torch.no_grad():
        l3 = lossf(p.clone().requires_grad_(True), t)
    assert rec.names and not backward_launches(rec.names), backward_launches(rec.names)
    assert torch.equal(l3, l1) and not l3.requires_grad
    # ... and neither does one that does not require grad, with autograd on
    with ua.ops.record_launches() as rec:
        l5 = lossf(p, t)
    assert rec.names and not backward_launches(rec.names), backward_launches(rec.names)
    assert torch.equal(l5, l1) and not l5.requires_grad
    with ua.ops.record_launches() as rec:
        loss_and_grad(lossf, p, t)
    assert [k for k in rec.names if "perceptual_relu_bwd" in k or "perceptual_relu_pool_bwd" in k]
    assert [k for k in rec.names if "stem_bwd_data" in k]
    _, g4 = loss_and_grad(lossf, p, t, scale=0.25)
    assert torch.equal(g4, 0.25 * g1)
    # a second backward through a retained graph scales the kept gradient again
    x = p.clone().requires_grad_(True)
    loss = lossf(x, t)
    loss.backward(retain_graph=True)
    loss.backward()
    assert torch.equal(x.grad, 2 * g1)


@pytest.mark.parametrize("u8", [False, True])
def test_reconstruction_loss_is_the_sum_of_its_terms(ua, weights, u8):
    layout = "nhwc_u8" if u8 else "nchw"
    pu, tu = V.case_inputs((2, 3, 64, 64), "structured", 62)
    p = (pu.float() / 255).to(DEV)
    t = tu.permute(0, 2, 3, 1).contiguous().to(DEV) if u8 else (tu.float() / 255).to(DEV)
    pl = V.load_trunk(ua.PerceptualLoss(target_layout=layout), weights).to(DEV)
    full, g_full = loss_and_grad(ua.ReconstructionLoss(1.0, 0.1, 0.1, target_layout=layout,
                                                       perceptual=pl), p, t)
    parts = [(1.0, ua.MSELoss(target_layout=layout)), (0.1, pl),
             (0.1, ua.SSIMLoss(target_layout=layout))]
    loss, grad = 0.0, 0.0
    for w, f in parts:
        l, gr = loss_and_grad(f, p, t)
        loss, grad = loss + w * l.double(), grad + w * gr.double()
    assert abs(full.item() - loss.item()) <= 1e-6 * loss.item()
    assert rel_l2(g_full, grad) <= 1e-6
    if u8:      # the uint8 target is the fp32 target's bits
        same, g_same = loss_and_grad(
            ua.ReconstructionLoss(1.0, 0.1, 0.1, perceptual=V.load_trunk(
                ua.PerceptualLoss(), weights).to(DEV)), p, (tu.float() / 255).to(DEV))
        assert torch.equal(same, full) and torch.equal(g_same, g_full)


def _ae_loss(ua, weights):
    return ua.ReconstructionLoss(1.0, 0.1, 0.0,
                                 perceptual=V.load_trunk(ua.PerceptualLoss(), weights)).to(DEV)


def test_ae_trajectory_under_mse_plus_perceptual(ua, golden, weights):
    """3 Adam + cosine steps of the tie-free (negative_slope 1) autoencoder under
    ReconstructionLoss(1.0, 0.1, 0.0) against the reference's: loss within 2e-4, outputs 1e-4."""
    g = golden("perceptual")
    rec = _ae_recorder()
    model = ua.Autoencoder(encoder_dropout_rates=rec.ENC_DROPOUT, decoder_dropout_rates=rec.DEC_DROPOUT,
                           nonlin_kwargs={"negative_slope": 1.0, "inplace": True})
    model.load_state_dict(rec.ae_state_dict())
    model = model.to(DEV).train()
    img = torch.from_numpy(g["ae_image_u8"]).to(DEV).permute(0, 3, 1, 2).float().contiguous() / 255.0
    opt = ua.ae.create_optimizer(model)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=int(g["ae_t_max"]), eta_min=1e-6)
    lossf = _ae_loss(ua, weights)
    errs = []
    for s in range(int(g["ae_steps"])):
        model.dropout_mask_override = rec.draw_masks(rec.SEED_DROP + s)
        assert opt.param_groups[0]["lr"] == float(g[f"ae_lr_{s}"])
        opt.zero_grad()
        out = model(img)
        loss = lossf(out, img)
        loss.backward()
        ref = float(g[f"ae_loss_{s}"])
        errs.append((abs(loss.item() - ref) / ref, rel_l2(out, torch.from_numpy(g[f"ae_out_{s}"]))))
        opt.step()
        sched.step()
    print("AE steps (loss err, output err)", errs)
    for e_loss, e_out in errs:
        assert e_loss <= 2e-4 and e_out <= 1e-4


def test_graphed_step_replays_eager_steps(ua, weights):
    rec = _ae_recorder()
    gen = torch.Generator().manual_seed(13)
    imgs = [(torch.randint(0, 256, (2, 3, 64, 64), generator=gen).float() / 255.0).to(DEV)
            for _ in range(3)]
    results = []
    for graphed in (False, True):
        model = ua.ae.create_model(DEV).train()
        model.load_state_dict(rec.ae_state_dict())
        model.dropout_mask_override = [m.to(DEV) for m in rec.draw_masks(12)]
        opt = ua.ae.create_optimizer(model)
        lossf = _ae_loss(ua, weights)
        step = ua.GraphedTrainStep(model, opt, lossf, imgs[0], imgs[0]) if graphed else None
        ls = []
        for s in range(3):
            opt.param_groups[0]["lr"] = 1e-3 * (1.0 - 0.3 * s)
            loss = step(imgs[s], imgs[s]) if graphed else \
                ua.train_step(model, opt, lossf, imgs[s], imgs[s])
            ls.append(loss.item())
        results.append((model.flat_parameters()[0].clone(), ls, opt._flat_m.clone()))
    (pa, la, ma), (pb, lb, mb) = results
    assert la == lb
    assert torch.equal(pa, pb) and torch.equal(ma, mb)
