"""Shared by tests/tools/make_golden_clip_extractor.py, tools/bench_clip_vit.py and the CLIP tower
tests: a stock-torch restatement of the published CLIP image tower (Radford et al. 2021, "Learning
Transferable Visual Models From Natural Language Supervision": ViT with a pre-LayerNorm, QuickGELU
MLPs and a linear projection of the class token), its seeded weights, a bf16 emulation of the HIP
path on the CPU, and a stand-in for the `clip_model` object the reference's extractor wraps.

Neither the `clip` package nor its weights are needed: the weights come from a numpy PCG64 stream,
drawn tensor by tensor in state-dict order (non-zero biases, gamma != 1, beta != 0, so that every
path is exercised); the fixture pins them with per-tensor norms and 64 sampled entries."""
import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
SEED_W = 2024
PIN_SAMPLES = 64
OUT_GRID = 16

# name -> dict(input_resolution, patch_size, width, layers, heads, output_dim)
GEOMETRIES = {
    "fixture": dict(input_resolution=224, patch_size=32, width=128, layers=2, heads=2,
                    output_dim=512),
    "p14_t257": dict(input_resolution=224, patch_size=14, width=128, layers=4, heads=2,
                     output_dim=512),
    "full_width": dict(input_resolution=224, patch_size=16, width=768, layers=2, heads=12,
                       output_dim=512),
    "vit_b16": dict(input_resolution=224, patch_size=16, width=768, layers=12, heads=12,
                    output_dim=512),
}


class QuickGELU(nn.Module):
    def forward(self, x):
        return x * torch.sigmoid(1.702 * x)


class ResidualAttentionBlock(nn.Module):
    def __init__(self, d_model, n_head):
        super().__init__()
        self.attn = nn.MultiheadAttention(d_model, n_head)
        self.ln_1 = nn.LayerNorm(d_model)
        self.mlp = nn.Sequential(OrderedDict([("c_fc", nn.Linear(d_model, d_model * 4)),
                                              ("gelu", QuickGELU()),
                                              ("c_proj", nn.Linear(d_model * 4, d_model))]))
        self.ln_2 = nn.LayerNorm(d_model)

    def forward(self, x):
        h = self.ln_1(x)
        x = x + self.attn(h, h, h, need_weights=False)[0]
        return x + self.mlp(self.ln_2(x))


class Transformer(nn.Module):
    def __init__(self, width, layers, heads):
        super().__init__()
        self.width, self.layers = width, layers
        self.resblocks = nn.Sequential(*[ResidualAttentionBlock(width, heads)
                                         for _ in range(layers)])

    def forward(self, x):
        return self.resblocks(x)


class VisionTransformer(nn.Module):
    """Parameter names and shapes of CLIP's image tower; forward(x [N,3,R,R]) -> [N, output_dim]."""

    def __init__(self, input_resolution, patch_size, width, layers, heads, output_dim):
        super().__init__()
        self.input_resolution, self.patch_size, self.output_dim = input_resolution, patch_size, output_dim
        self.conv1 = nn.Conv2d(3, width, kernel_size=patch_size, stride=patch_size, bias=False)
        tokens = (input_resolution // patch_size) ** 2 + 1
        self.class_embedding = nn.Parameter(torch.zeros(width))
        self.positional_embedding = nn.Parameter(torch.zeros(tokens, width))
        self.ln_pre = nn.LayerNorm(width)
        self.transformer = Transformer(width, layers, heads)
        self.ln_post = nn.LayerNorm(width)
        self.proj = nn.Parameter(torch.zeros(width, output_dim))

    def forward(self, x):
        x = self.conv1(x)
        x = x.reshape(x.shape[0], x.shape[1], -1).permute(0, 2, 1)          # [N, G^2, D]
        cls = self.class_embedding.to(x.dtype).expand(x.shape[0], 1, -1)
        x = torch.cat([cls, x], dim=1) + self.positional_embedding.to(x.dtype)
        x = self.ln_pre(x)
        x = self.transformer(x.permute(1, 0, 2)).permute(1, 0, 2)            # through [T, N, D]
        x = self.ln_post(x[:, 0, :])
        return x @ self.proj


def seeded_state_dict(geometry, seed=SEED_W):
    """OrderedDict of fp32 tensors in the state-dict order of VisionTransformer(**geometry)."""
    shapes = [(k, tuple(v.shape)) for k, v in VisionTransformer(**geometry).state_dict().items()]
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = OrderedDict()
    for name, shape in shapes:
        z = rng.standard_normal(shape)
        if name.endswith("ln_1.weight") or name.endswith("ln_2.weight") or \
                name in ("ln_pre.weight", "ln_post.weight"):
            t = 1.0 + 0.1 * z                       # gamma != 1
        elif name.endswith("bias"):
            t = 0.05 * z                            # every bias and beta non-zero
        elif name == "conv1.weight":
            t = z / math.sqrt(shape[1] * shape[2] * shape[3])
        elif name in ("class_embedding", "positional_embedding"):
            t = 0.5 * z
        elif name == "proj":
            t = z / math.sqrt(shape[0])
        elif name.endswith("in_proj_weight"):
            t = 2.0 * z / math.sqrt(shape[1])       # logits with a spread: softmax not flat
        else:
            t = z / math.sqrt(shape[1])
        sd[name] = torch.from_numpy(t.astype(np.float32))
    return sd


def build(geometry, seed=SEED_W, dtype=torch.float32):
    model = VisionTransformer(**geometry)
    model.load_state_dict(seeded_state_dict(geometry, seed))
    return model.to(dtype).eval()


def pin_weights(sd):
    """{key: value} that pins rebuilt weights: fp64 norms and PIN_SAMPLES entries a tensor."""
    out = {}
    for i, (name, t) in enumerate(sd.items()):
        flat = t.reshape(-1)
        rng = np.random.Generator(np.random.PCG64(1000 + i))
        pos = np.sort(rng.choice(flat.numel(), size=min(PIN_SAMPLES, flat.numel()),
                                 replace=False)).astype(np.int32)
        out[f"pin_{i}_norm"] = np.float64(flat.double().norm().item())
        out[f"pin_{i}_idx"] = pos
        out[f"pin_{i}_val"] = flat[torch.from_numpy(pos.astype(np.int64))].numpy()
    return out


class StandInClip:
    """What the reference's ClipPatchExtractor needs of `clip.load(...)[0]`."""

    def __init__(self, visual):
        self.visual = visual
        self.dtype = next(visual.parameters()).dtype

    def encode_image(self, x):
        return self.visual(x.to(self.dtype))


def images_u8(seed, n, h, w):
    """uint8 NHWC test images: 2 x 2 blocks of random values (compresses in the fixture)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    low = rng.integers(0, 256, size=(n, (h + 1) // 2, (w + 1) // 2, 3), dtype=np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(low, 2, axis=1), 2, axis=2)[:, :h, :w])


def normalise_u8(u8_nhwc):
    """fp32 NCHW (v / 255 - mean) / std of a uint8 NHWC batch: ToTensor + Normalize."""
    x = torch.as_tensor(u8_nhwc).permute(0, 3, 1, 2).float() / 255.0
    mean = torch.tensor(CLIP_MEAN, dtype=torch.float32).view(1, 3, 1, 1)
    std = torch.tensor(CLIP_STD, dtype=torch.float32).view(1, 3, 1, 1)
    return ((x - mean) / std).contiguous()


def extractor_ref(visual, images, grid=OUT_GRID):
    """ClipPatchExtractor.forward restated: resize to the tower's resolution, encode, broadcast."""
    r = visual.input_resolution
    x = images.to(next(visual.parameters()).dtype)
    if tuple(x.shape[2:]) != (r, r):
        x = F.interpolate(x, size=(r, r), mode="bilinear", align_corners=False)
    with torch.no_grad():
        e = visual(x)
    return F.interpolate(e[:, :, None, None], size=(grid, grid), mode="bilinear",
                         align_corners=False)


# ---- bf16 emulation of the HIP path ------------------------------------------------------------
def rb(t):
    """Round to bf16 (nearest even, from the fp32 value the kernel holds) and back to fp64."""
    return t.float().bfloat16().double()


def patch_matrix(x, resolution, patch):
    """fp64 [N G^2, 3 P^2] of the (resized) image, columns in the order of
    conv1.weight.reshape(D, -1)."""
    x = x.double()
    if tuple(x.shape[2:]) != (resolution, resolution):
        x = F.interpolate(x, size=(resolution, resolution), mode="bilinear", align_corners=False)
    cols = F.unfold(x, kernel_size=patch, stride=patch)                      # [N, 3 P^2, G^2]
    return cols.permute(0, 2, 1).reshape(-1, cols.shape[1])


def _ln(x, w, b, eps=1e-5):
    return F.layer_norm(x, (x.shape[-1],), w.double(), b.double(), eps)


def attention_ref(qkv, n, t, heads, round_p=True):
    """softmax(q k^T / 8) v of the packed [N T, 3 D] fp64 projection; round_p: the probabilities
    rounded to bf16 for the second product, the row sum taken of the unrounded ones."""
    d = qkv.shape[1] // 3
    q, k, v = (qkv[:, i * d:(i + 1) * d].reshape(n, t, heads, 64).permute(0, 2, 1, 3)
               for i in range(3))
    s = q @ k.transpose(-1, -2) / 8.0
    e = torch.exp(s - s.amax(dim=-1, keepdim=True))
    o = ((rb(e) if round_p else e) @ v) / e.sum(dim=-1, keepdim=True)
    return o.permute(0, 2, 1, 3).reshape(n * t, d)


def emulate(sd, x, heads, emulate_bf16=True):
    """The [N, E] embedding of fp32 NCHW images x (any size) in fp64 with the operands rounded to
    bf16 exactly where the HIP path rounds them: the patch matrix, the GEMM weights, the LayerNorm
    outputs, QKV, P, the attention output and the GELU output.  emulate_bf16=False: no rounding
    (the fp64 restatement, written as the same GEMMs)."""
    r_ = rb if emulate_bf16 else (lambda t: t.double())
    w = sd["conv1.weight"]
    D, patch = w.shape[0], w.shape[-1]
    pos = sd["positional_embedding"].double()
    T = pos.shape[0]
    res = int(round(math.sqrt(T - 1))) * patch
    n = x.shape[0]
    a = r_(patch_matrix(x, res, patch))
    pe = (a @ r_(w.reshape(D, -1)).T).reshape(n, T - 1, D)
    cls = sd["class_embedding"].double().expand(n, 1, D)
    s = _ln(torch.cat([cls, pe], dim=1) + pos, sd["ln_pre.weight"], sd["ln_pre.bias"])
    s = s.reshape(n * T, D)
    i = 0
    while f"transformer.resblocks.{i}.ln_1.weight" in sd:
        p = f"transformer.resblocks.{i}."
        h = r_(_ln(s, sd[p + "ln_1.weight"], sd[p + "ln_1.bias"]))
        qkv = r_(h @ r_(sd[p + "attn.in_proj_weight"]).T + sd[p + "attn.in_proj_bias"].double())
        o = r_(attention_ref(qkv, n, T, heads, round_p=emulate_bf16))
        s = s + (o @ r_(sd[p + "attn.out_proj.weight"]).T + sd[p + "attn.out_proj.bias"].double())
        h = r_(_ln(s, sd[p + "ln_2.weight"], sd[p + "ln_2.bias"]))
        f = h @ r_(sd[p + "mlp.c_fc.weight"]).T + sd[p + "mlp.c_fc.bias"].double()
        f = r_(f * torch.sigmoid(1.702 * f))
        s = s + (f @ r_(sd[p + "mlp.c_proj.weight"]).T + sd[p + "mlp.c_proj.bias"].double())
        i += 1
    c = _ln(s.reshape(n, T, D)[:, 0], sd["ln_post.weight"], sd["ln_post.bias"])
    return c @ sd["proj"].double()


def errors(got, ref):
    """(relative L2 error, maximum error relative to max |ref|)."""
    got, ref = got.double().cpu(), ref.double().cpu()
    return (((got - ref).norm() / ref.norm()).item(),
            ((got - ref).abs().max() / ref.abs().max()).item())
