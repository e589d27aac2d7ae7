"""uint8 batches in every operand mode (-m gpu): the dataset's uint8 [N,H,W,3] image through the
`_b16` stems and the whole net in the bf16 / split-bf16 modes, its uint8 [N,H,W] mask through the
uint8-target loss and metric kernels, and both through `train_step`, `GraphedTrainStep` and
`validate`.

The stem loaders compute the very floats `ops.preprocess_u8` writes and the uint8 target changes
only a load (the kernels are the int64 forms' templates, the reduction keeps their pixel-to-lane
map), so the yardstick everywhere is BIT EQUALITY with the existing path on converted inputs -
`torch.equal`, no tolerance."""
import numpy as np
import pytest
import torch

from oracle import unet_ref as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
SLOPE, EPS = 0.01, 1e-5


def u8_images(seed, n, h, w):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)


def raw_masks(seed, n, h, w, case="plain"):
    """A raw dataset mask: classes 0, 1, 2, the 255 border and stray values 3, 7, 254 the
    dataset's rule maps to 0.  case "absent": no pixel of class 2; "ignored": image 0 is all 255."""
    rng = np.random.Generator(np.random.PCG64(seed))
    vals = np.array([0, 1, 2, 255, 3, 7, 254], dtype=np.uint8)
    p = np.array([0.4, 0.2, 0.15, 0.1, 0.05, 0.05, 0.05])
    if case == "absent":
        p[2] = 0.0
        p /= p.sum()
    m = rng.choice(vals, size=(n, h, w), p=p)
    if case == "ignored":
        m[0] = 255
    return m


def cleaned(m):
    return np.where((m > 2) & (m != 255), 0, m)


def to_dev(m_u8):
    return torch.from_numpy(m_u8).to(DEV), torch.from_numpy(cleaned(m_u8)).long().to(DEV)


# ------------------------------------------------------------------------------------ stems
@pytest.fixture(scope="module")
def stem_case(ua):
    """(x_u8, fp32 image, {Cout: (packed weight, bias, gamma, beta)}) per H; computed once"""
    out = {}
    for H in (8, 6):      # H % 8 == 0: the walking kernel; else the rows kernel
        x = u8_images(10 + H, 2, H, 128).to(DEV)
        g = torch.Generator().manual_seed(20 + H)
        par = {}
        for cout in (32, 64):
            w = (torch.randn(cout, 3, 3, 3, generator=g) * 0.2).to(DEV)
            par[cout] = (ua.ops.pack_conv3x3_weights(w, want_wd=False)[0],
                         (torch.randn(cout, generator=g) * 0.1).to(DEV),
                         (1 + 0.1 * torch.randn(cout, generator=g)).to(DEV),
                         (0.1 * torch.randn(cout, generator=g)).to(DEV))
        out[H] = (x, ua.ops.preprocess_u8(x)[0], par)
    return out


@pytest.mark.parametrize("H", [8, 6])
@pytest.mark.parametrize("cout", [32, 64])
def test_stem_forward_on_bf16_tensors(ua, stem_case, H, cout):
    """ops.conv_in_fwd(U8Image, b16=True) (unet_stem_u8_fwd_b16) against the same call on the
    preprocessed fp32 image: y and all four statistics planes, bit for bit.  (Raised
    NotImplementedError before the `_b16` stem existed.)"""
    ops = ua.ops
    x, xf, par = stem_case[H]
    wf, b, gamma, beta = par[cout]
    y_u8, st_u8 = ops.conv_in_fwd(ops.U8Image(x), None, SLOPE, wf, b, 3, 1, gamma, beta, EPS, None,
                                  b16=True)
    y, st = ops.conv_in_fwd(ops.Act(xf), None, SLOPE, wf, b, 3, 1, gamma, beta, EPS, None, b16=True)
    assert y_u8.dtype == torch.bfloat16 and y_u8.shape == (2, H, 128, cout)
    assert torch.equal(y_u8, y)
    for k in range(4):
        assert torch.equal(st_u8[k], st[k]), f"statistics plane {k}"
    assert float(y.float().abs().max()) > 0


@pytest.mark.parametrize("H", [8, 6])
@pytest.mark.parametrize("cout", [32, 64])
def test_stem_weight_gradient_from_a_bf16_dy(ua, stem_case, H, cout):
    """ops.conv_in_bwd_weight(U8Image, bf16 dy) (unet_stem_u8_bwd_weight_b16) against the
    fp32-image call."""
    ops = ua.ops
    x, xf, _ = stem_case[H]
    g = torch.Generator().manual_seed(30 + H + cout)
    dy = torch.randn(2, H, 128, cout, generator=g).to(DEV).bfloat16()
    dw_u8 = torch.zeros(cout, 3, 3, 3, device=DEV)
    dw = torch.zeros(cout, 3, 3, 3, device=DEV)
    ops.conv_in_bwd_weight(ops.U8Image(x), SLOPE, dy, dw_u8, 0, 3, 1)
    ops.conv_in_bwd_weight(ops.Act(xf), SLOPE, dy, dw, 0, 3, 1)
    assert torch.equal(dw_u8, dw)
    assert float(dw.abs().max()) > 0


# ------------------------------------------------------------------------------------ whole net
@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
def test_uint8_batch_through_the_fused_stem_in_the_bf16_modes(ua, mode, monkeypatch):
    """forward(x_u8, input_layout="nhwc_u8") in the bf16 and split-bf16 modes: logits and every
    parameter gradient equal the run on the preprocessed tensor, and the fused stem really ran -
    `ops.preprocess_u8` is made to raise during the uint8 run, so the former fallback (which
    would pass the equality) fails."""
    x_u8 = u8_images(5, 2, 128, 128).to(DEV)
    tgt = torch.randint(0, 3, (2, 128, 128), generator=torch.Generator().manual_seed(6)).to(DEV)
    model = ua.UNet()
    model.load_state_dict(O.fill_state_dict(3))
    model = model.to(DEV).train()
    model.matmul_precision = mode
    model.dropout_mask_override = O.draw_dropout_masks(4, 2)
    lossf = ua.get_loss_function()
    x_f32 = ua.ops.preprocess_u8(x_u8)[0]

    def run(inp, layout):
        for p in model.parameters():
            p.grad = None
        logits = model(inp, input_layout=layout)
        lossf(logits, tgt).backward()
        return logits.detach().clone(), [p.grad.detach().clone() for p in model.parameters()]

    l_ref, g_ref = run(x_f32, "nhwc")

    def no_fallback(*a, **k):
        raise AssertionError("the uint8 batch went through preprocess_u8, not the fused stem")
    monkeypatch.setattr(ua.ops, "preprocess_u8", no_fallback)
    l_u8, g_u8 = run(x_u8, "nhwc_u8")
    assert torch.equal(l_u8, l_ref)
    assert len(g_u8) == len(g_ref) and len(g_ref) > 0
    for a, b in zip(g_u8, g_ref):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------ loss
LOSS_SHAPES = [(32, 48), (32, 50), (31, 50)]   # whole 4-pixel groups per row / per image only /
                                               # not at all (H*W % 4 == 2: one pixel per lane)


@pytest.fixture(scope="module")
def loss_logits():
    g = torch.Generator().manual_seed(40)
    return {hw: (torch.randn(2, 3, *hw, generator=g) * 2).to(DEV) for hw in LOSS_SHAPES}


def _loss_run(lossf, logits, target, up):
    z = logits.clone().requires_grad_(True)
    loss = lossf(z, target)
    (loss * up).backward()
    # (last_terms: [total, ce, dice, w0, w1, w2] - the two slots behind them are never written)
    return loss.detach().clone(), lossf.last_terms[:6].clone(), z.grad.clone()


@pytest.mark.parametrize("hw", LOSS_SHAPES)
@pytest.mark.parametrize("case", ["plain", "absent", "ignored"])
@pytest.mark.parametrize("dynamic", [True, False])
def test_loss_on_the_raw_uint8_mask(ua, loss_logits, hw, case, dynamic):
    """SimpleLoss(target_layout="u8") on the raw mask against SimpleLoss() on the np.where-cleaned
    int64 mask: loss, last_terms and dlogits for upstream gradients 1 and 0.5."""
    raw, clean = to_dev(raw_masks(50, 2, *hw, case=case))
    kw = dict(dynamic_weights=dynamic, class_weights=None if dynamic else [0.5, 1.5, 1.0])
    for up in (1.0, 0.5):
        l8, t8, d8 = _loss_run(ua.SimpleLoss(target_layout="u8", **kw), loss_logits[hw], raw, up)
        l, t, d = _loss_run(ua.SimpleLoss(**kw), loss_logits[hw], clean, up)
        assert torch.equal(l8, l) and torch.isfinite(l)
        assert torch.equal(t8, t)
        assert torch.equal(d8, d)
        assert float(d.abs().max()) > 0


def test_loss_on_a_mask_view_that_is_not_word_aligned(ua, loss_logits):
    """A contiguous mask at an odd byte offset: the four-pixel form must not be chosen."""
    hw = (32, 48)
    m = raw_masks(51, 2, *hw)
    buf = torch.zeros(m.size + 1, dtype=torch.uint8, device=DEV)
    raw = buf[1:].view(2, *hw)
    raw.copy_(torch.from_numpy(m))
    assert raw.is_contiguous() and raw.data_ptr() % 4 == 1
    clean = torch.from_numpy(cleaned(m)).long().to(DEV)
    l8, t8, d8 = _loss_run(ua.SimpleLoss(target_layout="u8"), loss_logits[hw], raw, 1.0)
    l, t, d = _loss_run(ua.SimpleLoss(), loss_logits[hw], clean, 1.0)
    assert torch.equal(l8, l) and torch.equal(t8, t) and torch.equal(d8, d)
    _, c8 = ua.ops.argmax_dice_counts(loss_logits[hw], raw)
    _, c = ua.ops.argmax_dice_counts(loss_logits[hw], clean)
    assert torch.equal(c8, c)


def test_u8_loss_takes_only_contiguous_uint8_device_masks(ua, loss_logits):
    hw = (32, 48)
    raw, clean = to_dev(raw_masks(52, 2, *hw))
    lossf = ua.SimpleLoss(target_layout="u8")
    with pytest.raises(TypeError):
        lossf(loss_logits[hw], clean)                       # int64
    with pytest.raises(TypeError):
        lossf(loss_logits[hw], raw.cpu())                   # host tensor
    wide = torch.zeros(2, hw[0], 2 * hw[1], dtype=torch.uint8, device=DEV)
    with pytest.raises(TypeError):
        lossf(loss_logits[hw], wide[:, :, ::2])             # not contiguous
    with pytest.raises(ua._lib.UNetHipError, match="ignore_index"):
        ua.SimpleLoss(target_layout="u8", ignore_index=-100)(loss_logits[hw], raw)


@pytest.mark.parametrize("hw", LOSS_SHAPES)
def test_shard_pair_on_the_raw_uint8_mask(ua, loss_logits, hw):
    """unet_dice_wce_loss_shard_stats_u8 / _shard_apply_u8 in one process, `apply` fed its own
    `stats` (a world of one shard), against the int64 pair run the same way."""
    ops = ua.ops
    z = loss_logits[hw]
    raw, clean = to_dev(raw_masks(53, 2, *hw))
    res = []
    for tgt in (raw, clean):
        stats, ws = ops.dice_wce_loss_shard_stats(z, tgt, 1e-5, 255)
        out, dl = ops.dice_wce_loss_shard_apply(z, tgt, stats, 2, ws, 1e-5, 1.0, 1.0, 255, True)
        res.append((stats.clone(), out[:6].clone(), dl.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    # ... and a world of one shard is the one-call loss
    one, dl1 = ops.dice_wce_loss_fwd_bwd(z, raw, 1e-5, 1.0, 1.0, 255, True)
    assert torch.equal(one[:6], res[0][1]) and torch.equal(dl1, res[0][2])


@pytest.mark.parametrize("hw", LOSS_SHAPES)
def test_argmax_dice_counts_on_the_raw_uint8_mask(ua, loss_logits, hw):
    z = loss_logits[hw]
    raw, clean = to_dev(raw_masks(54, 2, *hw))
    p8, c8 = ua.ops.argmax_dice_counts(z, raw)
    p, c = ua.ops.argmax_dice_counts(z, clean)
    assert torch.equal(p8, p) and torch.equal(p.long(), z.argmax(1))
    assert torch.equal(c8, c) and int(c.sum()) > 0
    _, c8n = ua.ops.argmax_dice_counts(z, raw, want_preds=False)
    assert torch.equal(c8n, c)


# ------------------------------------------------------------------------------------ steps
def _u8_batches(k):
    return [(u8_images(60 + i, 2, 128, 128).to(DEV),
             torch.from_numpy(raw_masks(70 + i, 2, 128, 128)).to(DEV)) for i in range(k)]


def _converted(ua, batches):
    """the batches as the fp32 / int64 path takes them: NCHW fp32 images, cleaned int64 masks"""
    out = []
    for x, m in batches:
        xf, t = ua.ops.preprocess_u8(x, m)
        out.append((xf.permute(0, 3, 1, 2).contiguous(), t))
    return out


def _bf16_model(ua, masks):
    model = ua.UNet()
    model.load_state_dict(O.fill_state_dict(23))
    model = model.to(DEV).train()
    model.matmul_precision = "bf16"
    model.dropout_mask_override = masks
    return model


def test_graph_captured_step_on_uint8_batches(ua):
    """GraphedTrainStep(..., input_layout="nhwc_u8") with a "u8" loss, bf16 mode: three replays on
    three different uint8 batches leave the losses and the parameters of three eager train_step
    calls on the preprocessed fp32 / int64 tensors; the static buffers stay uint8 and a batch of
    another dtype is refused."""
    masks = [m.to(DEV) if m is not None else None for m in O.draw_dropout_masks(5, 2)]
    batches = _u8_batches(3)
    conv = _converted(ua, batches)

    model = _bf16_model(ua, masks)
    opt = ua.create_optimizer(model)
    lossf = ua.get_loss_function()
    eager = [ua.train_step(model, opt, lossf, x, t).clone() for x, t in conv]
    p_eager = model.flat_parameters()[0].detach().clone()
    del model, opt

    model = _bf16_model(ua, masks)
    opt = ua.create_optimizer(model)
    lossf = ua.SimpleLoss(target_layout="u8")
    step = ua.GraphedTrainStep(model, opt, lossf, *batches[0], input_layout="nhwc_u8")
    assert step.images.dtype == torch.uint8 and step.masks.dtype == torch.uint8
    with pytest.raises(ValueError, match="dtype"):
        step(conv[0][0].permute(0, 2, 3, 1).contiguous(), batches[0][1])
    with pytest.raises(ValueError, match="dtype"):
        step(batches[0][0], conv[0][1])
    graph = [step(x, m).clone() for x, m in batches]
    torch.cuda.synchronize()
    for a, b in zip(graph, eager):
        assert torch.equal(a, b)
    assert torch.equal(model.flat_parameters()[0].detach(), p_eager)
    assert len({float(v) for v in eager}) == 3


def test_eager_step_on_uint8_batches(ua):
    """train_step(..., input_layout="nhwc_u8") with a "u8" loss against the converted batch."""
    masks = [m.to(DEV) if m is not None else None for m in O.draw_dropout_masks(5, 2)]
    batches = _u8_batches(1)
    conv = _converted(ua, batches)
    res = []
    for u8 in (False, True):
        model = _bf16_model(ua, masks)
        opt = ua.create_optimizer(model)
        if u8:
            loss = ua.train_step(model, opt, ua.SimpleLoss(target_layout="u8"), *batches[0],
                                 input_layout="nhwc_u8")
        else:
            loss = ua.train_step(model, opt, ua.get_loss_function(), *conv[0])
        res.append((loss.clone(), model.flat_parameters()[0].detach().clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_validate_on_uint8_batches(ua):
    """A two-batch list loader of uint8 dicts returns the loss and Dice of the converted loader."""
    batches = _u8_batches(2)
    conv = _converted(ua, batches)
    model = ua.UNet()
    model.load_state_dict(O.fill_state_dict(23))
    model = model.to(DEV)
    model.matmul_precision = "bf16"
    loss8, dice8 = ua.validate(model, [{"image": x, "mask": m} for x, m in batches],
                               ua.SimpleLoss(target_layout="u8"), DEV, input_layout="nhwc_u8")
    loss, dice = ua.validate(model, [{"image": x, "mask": t} for x, t in conv],
                             ua.get_loss_function(), DEV)
    assert loss8 == loss and np.isfinite(loss)
    assert dice8 == dice
