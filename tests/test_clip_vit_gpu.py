"""GPU: the CLIP image tower of csrc/vit.hip - every kernel against fp64 with a bound derived from
the rounding model (inputs are pre-rounded to bf16 wherever the kernel's inputs are bf16, so the
reference has no rounding ambiguity), the whole model against the fp64 restatement with the bf16
emulation's error on the same inputs as the budget, the reference extractor's golden, and the
CLIP_UNet train step fed by the extractor."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import unet_ref as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load("clip_vit_ref", ["tools", "clip_vit_ref.py"])


def gen(seed):
    return torch.Generator().manual_seed(seed)


def b16(t):
    return t.to(torch.bfloat16)


# ------------------------------------------------------------------------------------ GEMM
# the issue's four shapes, and two with K = 64 that select the 128 x 64 and 128 x 128 tiles
# (the four all take the 64 x 64 one: fewer than 128 workgroups otherwise)
GEMM_SHAPES = [(17, 64, 64), (197, 2304, 768), (3 * 197, 768, 3072), (2 * 50, 128, 592),
               (1576, 768, 64), (1576, 2304, 64)]
_gemm_cache = {}


def gemm_case(shape):
    """bf16 operands, fp64 product and sum of |a||w| - computed once a shape."""
    if shape not in _gemm_cache:
        M, Nout, K = shape
        g = gen(M + Nout + K)
        a = b16(torch.randn(M, K, generator=g))
        w = b16(torch.randn(Nout, K, generator=g) / K ** 0.5)
        if K == 592:        # P = 14: 588 real columns, 4 of padding
            a[:, 588:] = 0
            w[:, 588:] = 0
        bias = torch.randn(Nout, generator=g)
        resid = torch.randn(M, Nout, generator=g)
        prod = a.double() @ w.double().T
        absprod = a.double().abs() @ w.double().abs().T
        _gemm_cache[shape] = (a, w, bias, resid, prod, absprod)
    return _gemm_cache[shape]


@pytest.mark.parametrize("epilogue", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", GEMM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gemm_against_fp64(ua, shape, epilogue):
    """|err| <= K 2^-24 (|A| |W|^T)_ij + 2^-23 |y| for fp32 outputs (fp32 accumulation of exact
    bf16 products, then the epilogue's roundings); bf16 outputs add 2^-8 |y| (one rounding to
    nearest).  QuickGELU: the pre-activation's error passes through a slope within [-0.1, 1.1]
    (factor 1.13 with the product's own rounding) and the fast exponential adds 2^-20 |y|.
    Rows >= M of a poisoned, over-allocated output stay untouched."""
    M, Nout, K = shape
    a, w, bias, resid, prod, absprod = gemm_case(shape)
    POISON, EXTRA = 12345.0, 5
    fp32_out = epilogue in (0, 3)
    out = torch.full((M + EXTRA, Nout), POISON, dtype=torch.float32 if fp32_out else torch.bfloat16,
                     device=DEV)
    if epilogue == 3:
        out[:M] = resid.to(DEV)
    got = ua.ops.vit_gemm(a.to(DEV), w.to(DEV), None if epilogue == 0 else bias.to(DEV), epilogue,
                          out=out)
    assert got.data_ptr() == out.data_ptr()
    res = out.cpu()
    assert bool((res[M:] == POISON).all()), "rows >= M were written"
    pre = prod if epilogue == 0 else prod + bias.double()
    bound = K * 2.0 ** -24 * absprod
    if epilogue == 2:
        ref = pre * torch.sigmoid(1.702 * pre)
        bound = 1.13 * (bound + 2.0 ** -23 * pre.abs()) + (2.0 ** -8 + 2.0 ** -20) * ref.abs()
    else:
        ref = pre + resid.double() if epilogue == 3 else pre
        bound = bound + 2.0 ** -23 * ref.abs() + (0 if fp32_out else 2.0 ** -8 * ref.abs())
    err = (res[:M].double() - ref).abs()
    worst = (err / bound.clamp_min(1e-30)).max().item()
    print(f"gemm {shape} epilogue {epilogue}: max err / bound = {worst:.3f}, max err {err.max():.3e}")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("D", [128, 768, 1024])
@pytest.mark.parametrize("rows", [1, 197, 2 * 257])
def test_layernorm_against_fp64(ua, rows, D):
    """A mean of 3 against a spread of 1 (cancellation in a one-sum variance would show);
    |err| <= 2^-8 |y| + 1e-5: the bf16 rounding of the output and the fp32 arithmetic."""
    g = gen(rows * 7 + D)
    x = 3.0 + torch.randn(rows, D, generator=g)
    gamma = 1.0 + 0.1 * torch.randn(D, generator=g)
    beta = 0.05 * torch.randn(D, generator=g)
    got = ua.ops.vit_layernorm(x.to(DEV), gamma.to(DEV), beta.to(DEV)).cpu().double()
    ref = F.layer_norm(x.double(), (D,), gamma.double(), beta.double(), 1e-5)
    err = (got - ref).abs()
    worst = (err / (2.0 ** -8 * ref.abs() + 1e-5)).max().item()
    print(f"layernorm {rows} x {D}: max err / bound = {worst:.3f}")
    assert worst <= 1.0


def test_tokens_ln_pre_against_fp64(ua):
    N, T, D = 3, 50, 128
    g = gen(5)
    pe, cls, pos = torch.randn(N * (T - 1), D, generator=g), torch.randn(D, generator=g), \
        torch.randn(T, D, generator=g)
    gamma, beta = 1.0 + 0.1 * torch.randn(D, generator=g), 0.05 * torch.randn(D, generator=g)
    got = ua.ops.vit_tokens_ln(pe.to(DEV), cls.to(DEV), pos.to(DEV), gamma.to(DEV), beta.to(DEV),
                               N).cpu().double()
    tok = torch.cat([cls.double().expand(N, 1, D), pe.double().reshape(N, T - 1, D)], 1) + pos.double()
    ref = F.layer_norm(tok, (D,), gamma.double(), beta.double(), 1e-5).reshape(N * T, D)
    # fp32 throughout: a few ulps of the normalised value
    assert ((got - ref).abs() <= 2.0 ** -20 * ref.abs() + 1e-5).all()


# ------------------------------------------------------------------------------------ attention
def attention_inputs(N, T, heads, seed, huge=False):
    g = gen(seed)
    D = 64 * heads
    # q, k with a spread of 1.7: the logits q.k / 8 have a spread of 1.7^2 sqrt(64) / 8 = 2.9,
    # a softmax that is neither flat nor one-hot
    qkv = torch.randn(N * T, 3 * D, generator=g)
    qkv[:, :2 * D] *= 1.7
    if huge:
        qkv[3, D:2 * D] *= 40.0        # one key with huge logits (of either sign) for every query
    return b16(qkv)


@pytest.mark.parametrize("case", [(1, 17, 2), (2, 50, 2), (1, 197, 12), (2, 257, 16)],
                         ids=lambda c: "x".join(map(str, c)))
def test_attention_against_fp64(ua, case):
    """|err| <= 2^-7 max_j |v_j| per element: P and the output are each rounded once to bf16
    (2^-9 relative each, of values bounded by max_j |v_j| since the weights sum to 1); the fp32
    score and sum arithmetic is far below."""
    N, T, heads = case
    qkv = attention_inputs(N, T, heads, 100 + T)
    got = ua.ops.vit_attention(qkv.to(DEV), N, T, heads).cpu().double()
    ref = R.attention_ref(qkv.double(), N, T, heads, round_p=False)
    D = 64 * heads
    p = torch.softmax(qkv.double()[:, :64].reshape(N, T, 64)[0] @ qkv.double()[:, D:D + 64]
                      .reshape(N, T, 64)[0].T / 8, -1)
    assert 0.02 < p.max(-1).values.mean() < 0.9, "softmax flat or one-hot: rescale the inputs"
    vmax = qkv.double()[:, 2 * D:].abs().reshape(N, T, D).amax(dim=1, keepdim=True)
    bound = (2.0 ** -7 * vmax).expand(N, T, D).reshape(N * T, D)
    err = (got - ref).abs()
    worst = (err / bound).max().item()
    print(f"attention {case}: max err / bound = {worst:.3f}")
    assert worst <= 1.0


def test_attention_with_one_huge_logit_is_finite(ua):
    N, T, heads = 1, 50, 2
    qkv = attention_inputs(N, T, heads, 9, huge=True)
    got = ua.ops.vit_attention(qkv.to(DEV), N, T, heads).cpu().double()
    assert bool(torch.isfinite(got).all())
    ref = R.attention_ref(qkv.double(), N, T, heads, round_p=False)
    vmax = qkv.double()[:, 2 * 64 * heads:].abs().amax(dim=0, keepdim=True)
    assert ((got - ref).abs() <= 2.0 ** -7 * vmax).all()


# ------------------------------------------------------------------------------------ patch gather
def bf16_ulp(v):
    """The spacing of bf16 at |v| (8 significant bits)."""
    return torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126))) - 7)


@pytest.mark.parametrize("u8", [False, True], ids=["fp32", "u8"])
@pytest.mark.parametrize("P", [32, 16, 14])
@pytest.mark.parametrize("size", [(224, 224), (96, 128), (512, 512)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_patch_gather_against_fp64(ua, size, P, u8):
    """Reference: fp64 F.interpolate, then unfold.  Identity sampling (224 x 224) must be the
    correctly rounded bf16 of the fp32 value.  Resized: one bf16 ulp of the value, plus what fp32
    leaves of the sampling itself - the source coordinate (< in) carries 2 in 2^-24 of absolute
    error in fp32 (F.interpolate's own formula and precision), which moves the result by at most
    that times the largest difference of two neighbours (2 V, V = max |pixel|), and the blend's
    three fused operations add 4 2^-24 V.  The padded columns must be exactly 0."""
    H, W = size
    N = 2 if H < 512 else 1
    img = R.images_u8(H + P, N, H, W)
    x32 = R.normalise_u8(img)                      # fp32 NCHW: ToTensor + Normalize
    if u8:
        got = ua.ops.vit_patchify(torch.from_numpy(img).to(DEV), 224, P, "nhwc_u8")
    else:
        got = ua.ops.vit_patchify(x32.to(DEV), 224, P, "nchw")
    K, Kp = 3 * P * P, ua.ops.vit_k_padded(P)
    G = 224 // P
    assert tuple(got.shape) == (N * G * G, Kp) and got.dtype == torch.bfloat16
    got = got.cpu()
    assert bool((got[:, K:] == 0).all())
    ref = R.patch_matrix(x32, 224, P)
    if (H, W) == (224, 224):
        assert torch.equal(got[:, :K], ref.float().bfloat16())
        return
    V = x32.abs().max().item()
    bound = bf16_ulp(ref) + (2 * max(H, W) * 2.0 ** -24) * 2 * V + 4 * 2.0 ** -24 * V
    err = (got[:, :K].double() - ref).abs()
    worst = (err / bound).max().item()
    print(f"patch gather {size} P={P} u8={u8}: max err / bound = {worst:.3f}")
    assert worst <= 1.0


def test_u8_and_fp32_inputs_give_the_same_patch_matrix_and_features(ua):
    """The same pixels as uint8 NHWC and as normalised fp32 NCHW: the kernel normalises each tap
    with correctly rounded operations before it blends, so the patch matrices agree to one bf16 ulp
    (measured: bitwise) on the identity and on the resize path, and so do the features."""
    ext = extractor(ua, "fixture")
    for H, W in ((224, 224), (96, 128)):
        img = R.images_u8(3, 2, H, W)
        a_u8 = ua.ops.vit_patchify(torch.from_numpy(img).to(DEV), 224, 32, "nhwc_u8").float()
        a_f = ua.ops.vit_patchify(R.normalise_u8(img).to(DEV), 224, 32, "nchw").float()
        assert ((a_u8 - a_f).abs() <= bf16_ulp(a_f.double()).float()).all()
        f_u8 = ext(torch.from_numpy(img), input_layout="nhwc_u8")
        f_f = ext(R.normalise_u8(img))
        assert torch.equal(a_u8, a_f) and torch.equal(f_u8, f_f)


# ------------------------------------------------------------------------------------ whole model
_models, _cases = {}, {}


def extractor(ua, name):
    if name not in _models:
        clip_model = R.StandInClip(R.build(R.GEOMETRIES[name]))
        _models[name] = ua.ClipPatchExtractor(clip_model, device=DEV)
    return _models[name]


def model_case(name, u8_nhwc, tag):
    """(fp64 restatement, (rel L2, max rel) of the bf16 emulation) for these inputs, once."""
    if (name, tag) not in _cases:
        geometry = R.GEOMETRIES[name]
        x = R.normalise_u8(u8_nhwc)
        with torch.no_grad():
            ref = R.extractor_ref(R.build(geometry, dtype=torch.float64), x.double())[:, :, 0, 0]
        emu = R.emulate(R.seeded_state_dict(geometry), x, geometry["heads"])
        _cases[(name, tag)] = (ref, R.errors(emu, ref))
    return _cases[(name, tag)]


def check_budget(label, got, ref, emu_err, factor=2.0):
    l2, mx = R.errors(got, ref)
    print(f"{label}: rel L2 {l2:.3e} (emulation {emu_err[0]:.3e}), max rel {mx:.3e} "
          f"(emulation {emu_err[1]:.3e})")
    assert l2 <= factor * emu_err[0] and mx <= factor * emu_err[1]


@pytest.mark.parametrize("name,n", [("fixture", 2), ("p14_t257", 2), ("full_width", 3)])
def test_whole_model_within_twice_the_emulations_error(ua, name, n):
    """Relative L2 error of the embedding and maximum error relative to max |y|, against the fp64
    restatement, each at most 2 x the bf16 emulation's on the same inputs (the factor covers fp32
    accumulation order and the bf16 rounding flips it causes)."""
    img = R.images_u8(50 + n, n, 224, 224)
    ref, emu_err = model_case(name, img, "w")
    feats = extractor(ua, name)(torch.from_numpy(img), input_layout="nhwc_u8")
    assert tuple(feats.shape) == (n, 512, 16, 16) and feats.dtype == torch.float32
    check_budget(name, feats[:, :, 0, 0], ref, emu_err)
    # encode_image itself
    emb = extractor(ua, name).visual(R.normalise_u8(img).to(DEV))
    assert torch.equal(emb, feats[:, :, 0, 0])


@pytest.mark.parametrize("tag", ["224", "96x128"])
def test_golden_of_the_reference_extractor(ua, golden, tag):
    g = golden("clip_extractor")
    img = g[f"u8_{tag}"]
    ref, emu_err = model_case("fixture", img, tag)
    feats = extractor(ua, "fixture")(R.normalise_u8(img))
    check_budget(f"golden {tag} vs fp64", feats[:, :, 0, 0], ref, emu_err)
    check_budget(f"golden {tag} vs recorded", feats[:, :, 0, 0], torch.from_numpy(g[f"embed_{tag}"]),
                 emu_err)
    assert torch.equal(feats, feats[:, :, :1, :1].expand_as(feats)), "grid positions differ"


# ------------------------------------------------------------------------------------ robustness
def test_batch_sizes_determinism_and_weight_refresh(ua):
    ext = ua.ClipPatchExtractor(R.StandInClip(R.build(R.GEOMETRIES["fixture"])), device=DEV)
    img = R.images_u8(8, 5, 224, 224)
    ref, emu_err = model_case("fixture", img, "n5")
    f5 = ext(torch.from_numpy(img), input_layout="nhwc_u8")
    check_budget("N = 5", f5[:, :, 0, 0], ref, emu_err)
    f1 = ext(torch.from_numpy(img[:1]), input_layout="nhwc_u8")
    # every output element sums its products in the same order whatever M is
    assert torch.equal(f1, f5[:1])
    assert torch.equal(ext(torch.from_numpy(img), input_layout="nhwc_u8"), f5)     # no atomics
    # an in-place weight change is seen: the bf16 copies are remade
    w = ext.visual.transformer.resblocks[0].mlp.c_fc.weight
    with torch.no_grad():
        w.mul_(1.5)
    f5b = ext(torch.from_numpy(img), input_layout="nhwc_u8")
    assert not torch.equal(f5b, f5)
    fresh = ua.ClipVisionTransformer.from_state_dict(
        {k: v.cpu() for k, v in ext.visual.state_dict().items()}).to(DEV)
    assert torch.equal(fresh.feature_map(torch.from_numpy(img).to(DEV), 16, "nhwc_u8"), f5b)


# ------------------------------------------------------------------------------------ end to end
def test_clip_unet_train_step_fed_by_the_extractor(ua, golden):
    """ClipPatchExtractor -> CLIPUNet (64 x 64, the clip64 weights) -> SimpleLoss -> backward ->
    FusedSGD through ua.clip.train_step, against the same step fed the features of the fp64
    restatement.  Tolerances: those of test_clip_unet_golden (loss 2e-4, gradient norms 5e-3,
    relative), loosened by the feature error propagated through the fusion layer - which is zero:
    the features are constant over the grid, the 1 x 1 fusion convolution turns them into one
    constant per (image, output channel), and the InstanceNorm that follows removes a per-plane
    constant exactly (mean) and does not see it in the variance.  What is left of a feature error
    is the fp32 rounding of that cancellation, far inside the golden tolerances."""
    g = golden("clip64")
    n, hw, clip_dim = int(g["n"]), int(g["hw"]), int(g["clip_dim"])
    assert clip_dim == 512
    ext = extractor(ua, "fixture")
    img, tgt = O.synthetic_batch(int(g["seed_x"]), n, hw, hw)
    clip_u8 = R.images_u8(21, n, 96, 128)
    clip_images = R.normalise_u8(clip_u8)
    ref, emu_err = model_case("fixture", clip_u8, "e2e")
    ref_feats = ref.float()[:, :, None, None].expand(n, 512, 16, 16).contiguous().to(DEV)

    def run(clip_extractor):
        model = ua.CLIPUNet(with_clip_features=True, clip_dim=clip_dim)
        model.load_state_dict(O.fill_state_dict(int(g["seed_w"]), clip_dim=clip_dim))
        model = model.to(DEV).train()
        model.dropout_mask_override = O.draw_dropout_masks(int(g["seed_drop"]), n)
        opt = ua.create_optimizer(model)
        loss = ua.clip.train_step(model, opt, ua.SimpleLoss(), img.to(DEV), tgt.to(DEV),
                                  clip_extractor=clip_extractor, clip_images=clip_images)
        return loss.item(), {k: p.grad.double().norm().item() for k, p in model.named_parameters()}, \
            {k: p.detach().clone() for k, p in model.named_parameters()}

    seen = {}

    def recording(x, input_layout="nchw"):
        seen["f"] = ext(x, input_layout=input_layout)
        return seen["f"]

    loss_a, norms_a, params_a = run(recording)
    loss_b, norms_b, _ = run(lambda x, input_layout="nchw": ref_feats)
    check_budget("e2e features", seen["f"][:, :, 0, 0], ref, emu_err)
    print(f"loss {loss_a:.6f} vs {loss_b:.6f}")
    assert np.isfinite(loss_a) and abs(loss_a - loss_b) <= 2e-4 * abs(loss_b)
    for k, nb in norms_b.items():
        if nb < 1e-4:
            assert norms_a[k] < 1e-3, k
        else:
            assert abs(norms_a[k] - nb) <= 5e-3 * nb, (k, norms_a[k], nb)
    sd0 = O.fill_state_dict(int(g["seed_w"]), clip_dim=clip_dim)
    moved = [k for k, p in params_a.items() if not torch.equal(p.cpu(), sd0[k])]
    assert any("clip_fusion_conv" in k for k in moved) and len(moved) > 80   # the step was taken


def test_validate_with_and_without_an_extractor(ua, golden):
    g = golden("clip64")
    n, hw, clip_dim = int(g["n"]), int(g["hw"]), int(g["clip_dim"])
    model = ua.CLIPUNet(with_clip_features=True, clip_dim=clip_dim)
    model.load_state_dict(O.fill_state_dict(int(g["seed_w"]), clip_dim=clip_dim))
    model = model.to(DEV)
    img, tgt = O.synthetic_batch(int(g["seed_x"]), n, hw, hw)
    batch = {"image": img, "mask": tgt, "clip_image": R.normalise_u8(R.images_u8(22, n, 224, 224))}
    with_loss, with_scores = ua.clip.validate(model, [batch], ua.SimpleLoss(), DEV,
                                              clip_extractor=extractor(ua, "fixture"))
    no_loss, no_scores = ua.clip.validate(model, [batch], ua.SimpleLoss(), DEV)
    assert np.isfinite(with_loss) and np.isfinite(no_loss) and with_loss != no_loss
    assert set(with_scores) == set(no_scores) == {"background", "cat", "dog", "mean_foreground"}
    epoch_loss = ua.clip.train_one_epoch(model, [batch], ua.create_optimizer(model),
                                         ua.SimpleLoss(), DEV,
                                         clip_extractor=extractor(ua, "fixture"))
    assert np.isfinite(epoch_loss)
