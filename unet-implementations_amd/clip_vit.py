"""The frozen CLIP image tower of CLIP_UNet on the HIP path.

`ClipVisionTransformer` carries the parameters of OpenAI CLIP's `VisionTransformer` under the same
names and shapes (`load_state_dict(clip_model.visual.state_dict())` works) and runs `encode_image`
through csrc/vit.hip: a patch gather that resizes while it reads, bf16 matrix-core GEMMs with fp32
accumulators and epilogues, one attention launch for all (image, head) pairs, fp32 LayerNorm and
residual stream.  `ClipPatchExtractor` is the reference's module of that name
(CLIP_UNet/models/unet.py:486-618): resize to the tower's resolution, `encode_image`, broadcast of
the [N, E] embedding to [N, E, 16, 16] - the tensor `CLIPUNet.forward(x, clip_features)` takes.

Forward only and always under no_grad: the reference keeps CLIP frozen
(CLIP_UNet/src/train.py:718).  Supported: head dimension 64, width % 64 == 0 and <= 1024,
at most 257 tokens (ViT-B/32, B/16 and L/14 at 224).
"""
import math

import torch
import torch.nn as nn

from . import ops

MAX_TOKENS = 257
MAX_WIDTH = 1024


def _frozen(t):
    return nn.Parameter(t, requires_grad=False)


class _LayerNormParams(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.weight = _frozen(torch.ones(d))
        self.bias = _frozen(torch.zeros(d))


class _Linear(nn.Module):
    def __init__(self, d_in, d_out, std):
        super().__init__()
        self.weight = _frozen(torch.randn(d_out, d_in) * std)
        self.bias = _frozen(torch.zeros(d_out))


class _Attention(nn.Module):
    """The parameters of nn.MultiheadAttention(D, heads)."""

    def __init__(self, d, std, proj_std):
        super().__init__()
        self.in_proj_weight = _frozen(torch.randn(3 * d, d) * std)
        self.in_proj_bias = _frozen(torch.zeros(3 * d))
        self.out_proj = _Linear(d, d, proj_std)


class _MLP(nn.Module):
    def __init__(self, d, fc_std, proj_std):
        super().__init__()
        self.c_fc = _Linear(d, 4 * d, fc_std)
        self.c_proj = _Linear(4 * d, d, proj_std)


class _ResBlock(nn.Module):
    def __init__(self, d, layers):
        super().__init__()
        # CLIP's initialisation (clip/model.py, initialize_parameters)
        attn_std, proj_std, fc_std = d ** -0.5, (d ** -0.5) * ((2 * layers) ** -0.5), (2 * d) ** -0.5
        self.attn = _Attention(d, attn_std, proj_std)
        self.ln_1 = _LayerNormParams(d)
        self.mlp = _MLP(d, fc_std, proj_std)
        self.ln_2 = _LayerNormParams(d)


class _Transformer(nn.Module):
    def __init__(self, d, layers, heads):
        super().__init__()
        self.width, self.layers, self.heads = d, layers, heads
        self.resblocks = nn.Sequential(*[_ResBlock(d, layers) for _ in range(layers)])


def check_geometry(input_resolution, patch_size, width, heads):
    """Raises NotImplementedError naming the limit the geometry breaks."""
    if input_resolution % patch_size:
        raise NotImplementedError("input_resolution must be a multiple of patch_size")
    tokens = (input_resolution // patch_size) ** 2 + 1
    if tokens > MAX_TOKENS:
        raise NotImplementedError(
            f"{tokens} tokens: the HIP attention keeps a whole score row in registers and takes at "
            f"most {MAX_TOKENS} (ViT-B/32, B/16, L/14 at 224; not L/14@336)")
    if width % 64 or width > MAX_WIDTH:
        raise NotImplementedError(f"width {width}: must be a multiple of 64, at most {MAX_WIDTH}")
    if heads * 64 != width:
        raise NotImplementedError(f"width {width} with {heads} heads: the head dimension must be 64")
    return tokens


class ClipVisionTransformer(nn.Module):
    def __init__(self, input_resolution=224, patch_size=16, width=768, layers=12, heads=12,
                 output_dim=512):
        super().__init__()
        self.tokens = check_geometry(input_resolution, patch_size, width, heads)
        self.input_resolution, self.patch_size, self.output_dim = input_resolution, patch_size, output_dim
        self.width, self.layers, self.heads = width, layers, heads
        scale = width ** -0.5
        self.conv1 = nn.Conv2d(3, width, kernel_size=patch_size, stride=patch_size, bias=False)
        self.conv1.weight.requires_grad_(False)
        self.class_embedding = _frozen(scale * torch.randn(width))
        self.positional_embedding = _frozen(scale * torch.randn(self.tokens, width))
        self.ln_pre = _LayerNormParams(width)
        self.transformer = _Transformer(width, layers, heads)
        self.ln_post = _LayerNormParams(width)
        self.proj = _frozen(scale * torch.randn(width, output_dim))
        self._b16 = {}       # parameter name -> (tensor identity, _version, bf16 copy)

    @classmethod
    def from_state_dict(cls, sd):
        """The tower a CLIP state dict describes (keys with or without the `visual.` prefix)."""
        if any(k.startswith("visual.") for k in sd):
            sd = {k[len("visual."):]: v for k, v in sd.items() if k.startswith("visual.")}
        w = sd["conv1.weight"]
        width, patch = int(w.shape[0]), int(w.shape[-1])
        tokens = int(sd["positional_embedding"].shape[0])
        g = int(round(math.sqrt(tokens - 1)))
        if g * g != tokens - 1:
            raise NotImplementedError(f"{tokens} positional embeddings are not a square grid + 1")
        layers = len({k.split(".")[2] for k in sd if k.startswith("transformer.resblocks.")})
        model = cls(g * patch, patch, width, layers, width // 64, int(sd["proj"].shape[1]))
        model.load_state_dict({k: v.float() for k, v in sd.items()})
        return model

    def _apply(self, fn, *args, **kwargs):
        self._b16 = {}
        return super()._apply(fn, *args, **kwargs)

    def _bf16(self, name, p, make=None):
        """bf16 copy of a weight, remade only when the parameter was replaced or written in place
        (its `_version` moved) - what ops.PackTable does for the convolutions."""
        hit = self._b16.get(name)
        if hit is not None and hit[0] is p and hit[1] == p._version:
            return hit[2]
        w = (p if make is None else make(p)).to(torch.bfloat16).contiguous()
        self._b16[name] = (p, p._version, w)
        return w

    def _patch_weight(self, w):
        D = w.shape[0]
        k = 3 * self.patch_size ** 2
        out = torch.zeros(D, ops.vit_k_padded(self.patch_size), dtype=w.dtype, device=w.device)
        out[:, :k] = w.reshape(D, k)
        return out

    @torch.no_grad()
    def stream(self, x, input_layout="nchw"):
        """The fp32 residual stream [N T, D] after the last block (before ln_post)."""
        N = x.shape[0]
        T, heads = self.tokens, self.heads
        a = ops.vit_patchify(x, self.input_resolution, self.patch_size, input_layout)
        pe = ops.vit_gemm(a, self._bf16("conv1.weight", self.conv1.weight, self._patch_weight))
        s = ops.vit_tokens_ln(pe, self.class_embedding, self.positional_embedding,
                              self.ln_pre.weight, self.ln_pre.bias, N)
        for i, blk in enumerate(self.transformer.resblocks):
            key = f"transformer.resblocks.{i}."
            h = ops.vit_layernorm(s, blk.ln_1.weight, blk.ln_1.bias)
            qkv = ops.vit_gemm(h, self._bf16(key + "attn.in_proj_weight", blk.attn.in_proj_weight),
                               blk.attn.in_proj_bias, ops.VIT_BIAS)
            att = ops.vit_attention(qkv, N, T, heads)
            ops.vit_gemm(att, self._bf16(key + "attn.out_proj.weight", blk.attn.out_proj.weight),
                         blk.attn.out_proj.bias, ops.VIT_BIAS_RESIDUAL, out=s)
            h = ops.vit_layernorm(s, blk.ln_2.weight, blk.ln_2.bias)
            f = ops.vit_gemm(h, self._bf16(key + "mlp.c_fc.weight", blk.mlp.c_fc.weight),
                             blk.mlp.c_fc.bias, ops.VIT_BIAS_GELU)
            ops.vit_gemm(f, self._bf16(key + "mlp.c_proj.weight", blk.mlp.c_proj.weight),
                         blk.mlp.c_proj.bias, ops.VIT_BIAS_RESIDUAL, out=s)
        return s

    @torch.no_grad()
    def feature_map(self, x, grid=16, input_layout="nchw"):
        """[N, E, grid, grid] fp32: the embedding at every position of the grid."""
        s = self.stream(x, input_layout)
        return ops.vit_head(s, self.ln_post.weight, self.ln_post.bias, self.proj, x.shape[0],
                            self.tokens, grid)

    def forward(self, x, input_layout="nchw"):
        """The [N, E] embedding of `encode_image`."""
        return self.feature_map(x, 1, input_layout).flatten(1)


class ClipPatchExtractor(nn.Module):
    """Drop-in for the reference's ClipPatchExtractor(clip_model, device): `clip_model` is any
    object whose `.visual` carries CLIP's VisionTransformer parameters (clip.load(...)[0], loaded
    on the host), or a ClipVisionTransformer."""

    OUT_GRID = 16       # CLIP_UNet/models/unet.py:611-612

    def __init__(self, clip_model, device="cuda"):
        super().__init__()
        visual = clip_model if isinstance(clip_model, ClipVisionTransformer) else \
            getattr(clip_model, "visual", None)
        if visual is None:
            raise ValueError("CLIP model doesn't have a 'visual' attribute")
        if not isinstance(visual, ClipVisionTransformer):
            visual = ClipVisionTransformer.from_state_dict(visual.state_dict())
        self.visual = visual.to(device)
        self.device = torch.device(device)
        self.feature_dim = visual.output_dim
        g = visual.input_resolution // visual.patch_size
        self.grid_size = (g, g)

    @torch.no_grad()
    def forward(self, images, input_layout="nchw"):
        images = images.to(self.device)
        if input_layout == "nchw" and images.dtype != torch.float32:
            images = images.float()
        return self.visual.feature_map(images.contiguous(), self.OUT_GRID, input_layout)
