"""Drop-in `UNet` for the reference's Our_UNet (Our_UNet/models/unet.py:233-432).

Same constructor keywords, same module tree (`encoder_stages[i].block[j]`,
`decoder_stages[i].conv_block.block[j]`, `segmentation_output`) and therefore
the same 90 `state_dict()` keys/shapes, same `forward(x) -> logits` contract
(NCHW fp32 in, NCHW fp32 logits out).  The sub-modules only hold parameters:
`forward` runs the whole network as ONE autograd node whose forward/backward
launch the gfx950 kernels of libunet_hip.so through the C ABI.

Internal layout: activations NHWC fp32.  Default (`fused_pipeline`, fp32 operand mode): per
conv layer only the RAW output y and its per-(n,c) InstanceNorm statistics live in HBM; the
statistics come out of the convolution's epilogue and every consumer (next conv, its weight
gradient, the up-sampling, the head) applies a = dropout(leaky_relu(IN(y))) while it stages
the operand (`ops.Act`).  The stand-alone pipeline (bf16 / bf16x3 operand modes, or
`fused_pipeline = False`) also materialises a.
"""
from typing import Dict, List, Optional, Tuple, Type, Union

import torch
import torch.nn as nn

from . import ops


class SpatialDropout2d(nn.Module):
    """Channel dropout (reference: Our_UNet/models/unet.py:13-35).

    Only carries `drop_prob`.  On the fused path `UNet.forward` draws the masks [N, C]
    (already divided by 1-p) of ALL dropout modules with one Bernoulli launch
    (`_draw_masks`): the same distribution as the reference's per-module
    `new_empty(N, C, 1, 1).bernoulli_(1 - p).div_(1 - p)`, but not the same random stream,
    so parity tests inject masks through `UNet.dropout_mask_override`.
    """

    def __init__(self, drop_prob):
        super().__init__()
        self.drop_prob = drop_prob

    def extra_repr(self):
        return f"drop_prob={self.drop_prob}"

    def draw_mask(self, n, channels, device):
        mask = torch.empty(n, channels, 1, 1, device=device).bernoulli_(1 - self.drop_prob)
        return mask.div_(1 - self.drop_prob).view(n, channels)

    def forward(self, x):  # NCHW tensor, stock torch semantics (not on the fused path)
        if not self.training or self.drop_prob == 0:
            return x
        return x * self.draw_mask(x.size(0), x.size(1), x.device).view(x.size(0), x.size(1), 1, 1)


def _same_padding(kernel_size):
    if isinstance(kernel_size, int):
        return kernel_size // 2
    return (kernel_size[0] // 2, kernel_size[1] // 2)


class ConvBlock(nn.Module):
    """[Conv2d -> norm -> nonlin -> SpatialDropout2d?] x n_convs; stride on the first conv.

    Mirrors Our_UNet/models/unet.py:37-141 (module order inside `.block` decides the
    state_dict indices: 0/1 and 3/4, or 0/1 and 4/5 when dropout modules are present).
    """

    def __init__(self, in_channels, out_channels, kernel_size, stride, n_convs=2, padding=None,
                 norm_op=nn.InstanceNorm2d, norm_op_kwargs=None, dropout_op=None,
                 dropout_op_kwargs=None, nonlin=nn.LeakyReLU, nonlin_kwargs=None, conv_bias=True,
                 spatial_dropout_rate=0.0):
        super().__init__()
        norm_op_kwargs = {"eps": 1e-5, "affine": True} if norm_op_kwargs is None else norm_op_kwargs
        nonlin_kwargs = {"inplace": True} if nonlin_kwargs is None else nonlin_kwargs
        dropout_op_kwargs = {} if dropout_op_kwargs is None else dropout_op_kwargs
        if padding is None:
            padding = _same_padding(kernel_size)
        mods = []
        cin = in_channels
        for k in range(n_convs):
            mods.append(nn.Conv2d(cin, out_channels, kernel_size, stride if k == 0 else 1, padding,
                                  bias=conv_bias))
            if norm_op is not None:
                mods.append(norm_op(out_channels, **norm_op_kwargs))
            if nonlin is not None:
                mods.append(nonlin(**nonlin_kwargs))
            if spatial_dropout_rate > 0:
                mods.append(SpatialDropout2d(spatial_dropout_rate))
            if dropout_op is not None:
                mods.append(dropout_op(**dropout_op_kwargs))
            cin = out_channels
        self.block = nn.Sequential(*mods)

    def forward(self, x):
        """The block on its own (reference: Our_UNet/models/unet.py:136-141 `self.block(x)`):
        NCHW fp32 in, NCHW fp32 out, differentiable.  Inside `UNet.forward` the blocks are never
        called - the network runs as one fused walk; a stand-alone call runs the same HIP entry
        points layer by layer (conv -> statistics -> InstanceNorm + LeakyReLU + dropout)."""
        return _run_block_standalone(self, x, None)


class UpBlock(nn.Module):
    """Bilinear up-sample to the skip size, concat [up, skip], ConvBlock
    (Our_UNet/models/unet.py:143-231)."""

    def __init__(self, in_channels, skip_channels, out_channels, kernel_size, n_convs=2,
                 norm_op=nn.InstanceNorm2d, norm_op_kwargs=None, dropout_op=None,
                 dropout_op_kwargs=None, nonlin=nn.LeakyReLU, nonlin_kwargs=None, conv_bias=True,
                 spatial_dropout_rate=0.0):
        super().__init__()
        self.conv_block = ConvBlock(in_channels + skip_channels, out_channels, kernel_size,
                                    stride=1, n_convs=n_convs, padding=None, norm_op=norm_op,
                                    norm_op_kwargs=norm_op_kwargs, dropout_op=dropout_op,
                                    dropout_op_kwargs=dropout_op_kwargs, nonlin=nonlin,
                                    nonlin_kwargs=nonlin_kwargs, conv_bias=conv_bias,
                                    spatial_dropout_rate=spatial_dropout_rate)

    def forward(self, x, skip):
        """Bilinear 2x up-sampling of `x` to the skip's size, cat([up, skip]), conv block
        (reference: Our_UNet/models/unet.py:203-231), stand-alone and differentiable; NCHW fp32.
        The HIP up-sampling kernel is the exact-2x stencil the network uses."""
        return _run_block_standalone(self.conv_block, x, skip)


def _run_block_standalone(block, x, skip):
    if not x.is_cuda:
        raise RuntimeError("unet-implementations_amd blocks run on MI355X only: move the module "
                           "and the input to a ROCm device (no CPU fallback exists)")
    if x.dim() != 4 or (skip is not None and skip.dim() != 4):
        raise ValueError("expected NCHW tensors")
    if skip is not None and (skip.shape[2] != 2 * x.shape[2] or skip.shape[3] != 2 * x.shape[3]):
        raise NotImplementedError("UpBlock on the HIP path up-samples by exactly 2x")
    layers = _parse_block(block, False, type(block).__name__)
    params = [q for l in layers for q in (l.conv.weight, l.conv.bias, l.norm.weight, l.norm.bias)]
    return _BlockFunction.apply(block, layers, x, skip, *params)


class _BlockFunction(torch.autograd.Function):
    """One ConvBlock (optionally behind up-sample + concat) through the stand-alone entry points:
    what `UNet(fused_pipeline=False)` runs per layer."""

    @staticmethod
    def forward(ctx, block, layers, x, skip, *params):
        x0 = ops.nchw_to_nhwc(x.detach().contiguous().float())
        x1 = None
        if skip is not None:
            x0 = ops.upsample2x_fwd(x0)
            x1 = ops.nchw_to_nhwc(skip.detach().contiguous().float())
        override = getattr(block, "dropout_mask_override", None)
        masks = iter(override) if override is not None else None
        recs = []
        for l in layers:
            w = l.conv.weight.detach()
            if w.shape[0] % 32:
                raise NotImplementedError("the HIP convolution needs Cout % 32 == 0")
            wf, wd = ops.pack_conv3x3_weights(w.contiguous())
            y = ops.conv3x3_fwd(x0, x1, wf, l.conv.bias.detach(), l.stride)
            st = ops.instnorm_stats(y, l.norm.weight.detach(), l.norm.bias.detach(), l.norm.eps)
            m = None
            if l.drop is not None and l.drop.drop_prob > 0:
                if masks is not None:
                    m = next(masks).to(device=y.device, dtype=torch.float32).contiguous()
                elif block.training:
                    m = l.drop.draw_mask(y.shape[0], y.shape[3], y.device).contiguous()
            a = ops.instnorm_lrelu_drop_fwd(y, st[2], st[3], m, l.slope)
            recs.append((l, x0, x1, y, st, m, wd))
            x0, x1 = a, None
        ctx.recs, ctx.up = recs, skip is not None
        return ops.nhwc_to_nchw(x0)

    @staticmethod
    def backward(ctx, gout):
        g = ops.nchw_to_nhwc(gout.contiguous().float())
        grads = []
        dx1 = None
        for l, x0, x1, y, st, m, wd in reversed(ctx.recs):
            C = y.shape[3]
            dgm, dbt, dbias = (torch.empty(C, device=y.device) for _ in range(3))
            dy = ops.instnorm_lrelu_drop_bwd(g, y, st[0], st[1], l.norm.weight.detach(),
                                             l.norm.bias.detach(), m, l.slope, dgm, dbt, dbias)
            dw = torch.empty_like(l.conv.weight)
            ops.conv3x3_bwd_weight(x0, dy, dw, 0, l.stride)
            N, H, W, C0 = x0.shape
            if x1 is not None:
                ops.conv3x3_bwd_weight(x1, dy, dw, C0, l.stride)
                dx1 = ops.conv3x3_bwd_data(dy, wd, C0, x1.shape[3], H, W, l.stride)
            first = l is ctx.recs[0][0]
            if first and not ctx.needs_input_grad[2]:
                g = None
            elif C0 % 32:
                raise NotImplementedError("the HIP data gradient needs a multiple of 32 input "
                                          "channels (the RGB stem's input gets no gradient)")
            else:
                g = ops.conv3x3_bwd_data(dy, wd, 0, C0, H, W, l.stride)
            grads = [dw, dbias, dgm, dbt] + grads
        ctx.recs = None
        gx = None
        if g is not None:
            gx = ops.nhwc_to_nchw(ops.upsample2x_bwd(g) if ctx.up else g)
        gskip = ops.nhwc_to_nchw(dx1) if dx1 is not None else None
        return (None, None, gx, gskip, *grads)


def _parse_block(block, first_of_decoder, prefix):
    """[Conv2d -> InstanceNorm2d(affine) -> LeakyReLU -> SpatialDropout2d?] x n of a ConvBlock as
    `_Layer`s; raises NotImplementedError for anything the HIP path does not cover."""
    mods = list(block.block)
    layers, i = [], 0
    while i < len(mods):
        conv = mods[i]
        if not isinstance(conv, nn.Conv2d):
            raise NotImplementedError(f"{prefix}: unexpected module {type(conv).__name__}")
        ks, st = _as_int(conv.kernel_size), _as_int(conv.stride)
        if ks != 3 or st not in (1, 2) or _as_int(conv.padding) != 1 or conv.bias is None \
                or conv.groups != 1 or _as_int(conv.dilation) != 1:
            raise NotImplementedError(
                f"{prefix}.block.{i}: the HIP path covers 3x3/pad 1/stride 1|2 convs with bias")
        i += 1
        norm = mods[i] if i < len(mods) else None
        if not (isinstance(norm, nn.InstanceNorm2d) and norm.affine
                and not norm.track_running_stats):
            raise NotImplementedError(
                f"{prefix}: the HIP path needs InstanceNorm2d(affine=True) after each conv")
        i += 1
        act = mods[i] if i < len(mods) else None
        if not isinstance(act, nn.LeakyReLU):
            raise NotImplementedError(f"{prefix}: the HIP path needs LeakyReLU after the norm")
        i += 1
        drop = None
        if i < len(mods) and isinstance(mods[i], SpatialDropout2d):
            drop = mods[i]
            i += 1
        if i < len(mods) and not isinstance(mods[i], nn.Conv2d):
            raise NotImplementedError(
                f"{prefix}: dropout_op={type(mods[i]).__name__} is not on the HIP path")
        layers.append(_Layer(conv, norm, float(act.negative_slope), drop, st,
                             first_of_decoder and not layers, f"{prefix}.block.{len(layers)}"))
    return layers


class _Layer:
    """One conv3x3 + InstanceNorm + LeakyReLU (+ dropout) unit of the fused plan."""

    __slots__ = ("conv", "norm", "slope", "drop", "stride", "first_of_decoder", "name", "ksize")

    def __init__(self, conv, norm, slope, drop, stride, first_of_decoder, name, ksize=3):
        self.conv, self.norm, self.slope, self.drop = conv, norm, slope, drop
        self.stride, self.first_of_decoder, self.name = stride, first_of_decoder, name
        self.ksize = ksize


class _Rec:
    """What the forward of one layer leaves for its backward (`_Walk.saved`, forward order).
    Every field is set by the `_Walk.run_*` call that made the record; None = does not apply.

    Operands: `x0` / `x1` (tensors, or ops.Act on the fused pipeline); `low` replaces `x0` where
    the first operand was up-sampled while the convolution loaded it.  Results: raw output `y`,
    statistics `st`, dropout `mask`, and the activated output `a` (stand-alone pipeline only).
    Backward weight forms: `wd` / `wd3` (packed fp32 / bf16 planes), `ud` / `ud1` (Winograd form
    of the data gradient into x0 / into the skip half x1).
    Place in the backward schedule: `bwd_hooks` = the modules this layer is the last of (their
    backward hooks see its output gradient), `completes` = the module this layer is the first of
    (its gradients are final once this layer's backward ran), `skip_dst` = index of the record
    whose input x1 is (first convolution of a decoder stage: dx1 goes there).
    `nxt` alone is written later: by `next_norm()`, read by this layer's `_Walk.layer_bwd`."""

    __slots__ = ("layer", "x0", "x1", "low", "y", "st", "mask", "a", "wd", "wd3", "ud", "ud1",
                 "bwd_hooks", "completes", "skip_dst", "nxt")

    def __init__(self, layer, x0, x1, y, st, mask, bwd_forms, place, low=None, a=None):
        self.layer, self.x0, self.x1, self.low, self.a = layer, x0, x1, low, a
        self.y, self.st, self.mask = y, st, mask
        self.wd, self.wd3, self.ud, self.ud1 = bwd_forms
        self.bwd_hooks, self.completes, self.skip_dst = place
        self.nxt = None

    def next_norm(self):
        """For the kernel that produces the FINAL gradient of this layer's output: it also leaves
        the reductions of this layer's InstanceNorm backward in the returned ops.NextNorm."""
        l = self.layer
        self.nxt = ops.NextNorm(self.y, self.st, l.norm.weight.detach(), l.norm.bias.detach(),
                                self.mask, l.slope)
        return self.nxt

    def output(self):
        """This layer's output as its consumers take it."""
        return self.a if self.a is not None else ops.Act(self.y, self.st[2], self.st[3])


def _as_int(v):
    if isinstance(v, (tuple, list)):
        if len(set(v)) != 1:
            return None
        return int(v[0])
    return int(v)


class UNet(nn.Module):
    """6-stage encoder/decoder UNet with the reference's constructor surface."""

    def __init__(self, in_channels: int = 3, num_classes: int = 3, n_stages: int = 6,
                 features_per_stage: List[int] = None,
                 kernel_sizes: List[Tuple[int, int]] = None,
                 strides: List[Tuple[int, int]] = None, n_conv_per_stage: List[int] = None,
                 n_conv_per_stage_decoder: List[int] = None, conv_bias: bool = True,
                 norm_op: Type[nn.Module] = nn.InstanceNorm2d, norm_op_kwargs: Dict = None,
                 dropout_op: Optional[Type[nn.Module]] = None, dropout_op_kwargs: Dict = None,
                 nonlin: Type[nn.Module] = nn.LeakyReLU, nonlin_kwargs: Dict = None,
                 encoder_dropout_rates: List[float] = None,
                 decoder_dropout_rates: List[float] = None):
        super().__init__()
        if features_per_stage is None:
            features_per_stage = [32, 64, 128, 256, 512, 512]
        if kernel_sizes is None:
            kernel_sizes = [[3, 3]] * n_stages
        if strides is None:
            strides = [[1, 1]] + [[2, 2]] * (n_stages - 1)
        if n_conv_per_stage is None:
            n_conv_per_stage = [2] * n_stages
        if n_conv_per_stage_decoder is None:
            n_conv_per_stage_decoder = [2] * (n_stages - 1)
        if norm_op_kwargs is None:
            norm_op_kwargs = {"eps": 1e-5, "affine": True}
        if nonlin_kwargs is None:
            nonlin_kwargs = {"inplace": True}
        if encoder_dropout_rates is None:
            encoder_dropout_rates = [0.0, 0.0, 0.1, 0.2, 0.3, 0.3]
        if decoder_dropout_rates is None:
            decoder_dropout_rates = [0.3, 0.2, 0.2, 0.1, 0.0]

        self.in_channels = in_channels
        self.num_classes = num_classes
        self.n_stages = n_stages
        self.features_per_stage = features_per_stage

        common = dict(norm_op=norm_op, norm_op_kwargs=norm_op_kwargs, dropout_op=dropout_op,
                      dropout_op_kwargs=dropout_op_kwargs, nonlin=nonlin,
                      nonlin_kwargs=nonlin_kwargs, conv_bias=conv_bias)
        self.encoder_stages = nn.ModuleList()
        cin = in_channels
        for s in range(n_stages):
            self.encoder_stages.append(
                ConvBlock(cin, features_per_stage[s], kernel_sizes[s], strides[s],
                          n_convs=n_conv_per_stage[s],
                          spatial_dropout_rate=encoder_dropout_rates[s], **common))
            cin = features_per_stage[s]
        self._fusion_layer = None
        self._build_bottleneck(common)      # registration order = state_dict / arena order
        self.decoder_stages = nn.ModuleList()
        for s in range(n_stages - 1):
            lvl = n_stages - 2 - s
            self.decoder_stages.append(
                UpBlock(features_per_stage[lvl + 1], features_per_stage[lvl],
                        features_per_stage[lvl], kernel_sizes[lvl],
                        n_convs=n_conv_per_stage_decoder[lvl],
                        spatial_dropout_rate=decoder_dropout_rates[s], **common))
        self._build_head(features_per_stage[0], num_classes)
        self.initialize_weights()
        self._plan = None
        self._arena = None       # flat fp32 parameter arena (parameters are views into it)
        self._grad_arena = None  # flat fp32 gradient arena (p.grad are views into it)
        self._offsets = None
        self.dropout_mask_override = None  # test hook: list of [N, C] masks in forward order
        # data-parallel hook: called during backward as `hook(lo)` once every gradient at arena
        # offsets >= lo is final (backward completes the arena back to front)
        self.grad_ready_hook = None
        # "fp32" (default, the parity path) or "bf16": the conv operands (forward, data gradient,
        # stride-1 weight gradient) are rounded to bf16 on chip and contracted on the bf16 matrix
        # cores with fp32 accumulation (tensors, InstanceNorm statistics, master weights: fp32)
        self.matmul_precision = "fp32"
        # fp32 operand mode only: keep just the raw conv outputs in HBM (statistics from the
        # conv epilogue, InstanceNorm + LeakyReLU + dropout applied by the consumers on load)
        self.fused_pipeline = True
        # fp32 fused pipeline: run the stride-1 3x3 layers the Winograd F(2x2,3x3) kernel tiles
        # on it (2.25x fewer matrix-core FLOPs, a few extra fp32 roundings: csrc/conv_wino.hip)
        self.winograd = True
        # fp32 fused pipeline: two full-resolution gradients are formed inside their consumers
        # instead of being stored - dL/da of the last decoder layer (the head's backward goes on
        # to that layer's dL/dz) and dL/dz of the stem (formed by the loader of its weight
        # gradient).  Same bits either way; off = the stored forms
        self.fullres_folds = True
        # ... and two more whose dL/dz has several readers are formed inside the 32-channel
        # Winograd weight gradient, which stores dz over g in place (the layers' separate
        # InstanceNorm-backward pass is gone).  Same bits either way; off = the separate pass
        self.wgrad32_folds = True
        # normalisation constants of forward(..., input_layout="nhwc_u8") (ImageNet, as the
        # reference's dataset: Our_UNet/src/train.py:303-308)
        self.input_mean, self.input_std = ops.IMAGENET_MEAN, ops.IMAGENET_STD

    def _build_bottleneck(self, common):
        """Hook for variants that add modules between encoder and decoder (CLIPUNet)."""

    # -- the head: a model-level hook of the fused walk (the Autoencoder plugs in its own) -------
    def _build_head(self, in_features, out_channels):
        self.segmentation_output = nn.Conv2d(in_features, out_channels, kernel_size=1, stride=1,
                                             padding=0, bias=True)

    def _head_module(self):
        return self.segmentation_output

    def _check_head(self):
        head = self.segmentation_output
        if _as_int(head.kernel_size) != 1 or head.in_channels != 32 or \
                not 2 <= head.out_channels <= ops.MAX_CLASSES:
            raise NotImplementedError(
                "the HIP head kernels are the 32 -> K 1x1 convolution for 2 <= K <= "
                f"{ops.MAX_CLASSES} classes (got {head.in_channels} -> {head.out_channels}, "
                f"kernel {_as_int(head.kernel_size)})")

    def _head_fwd(self, walk, cur):
        """NCHW fp32 output of the head over the last decoder layer's output `cur` (ops.Act on the
        fused pipeline, the activated NHWC tensor otherwise)."""
        head = self.segmentation_output
        hw = head.weight.detach().view(head.out_channels, -1)
        if walk.fused:
            return ops.head1x1_in_fwd(cur, walk.slope, hw, head.bias.detach())
        return ops.head1x1_fwd(cur, hw, head.bias.detach())

    def _head_bwd(self, walk, rec, dout, grad_only=False):
        """dL/da of the last decoder layer's output (`rec`: its record); writes the head's weight
        gradients (grad_only: the data gradient alone, nothing is written but the result; `rec`
        is then also the last layer that gets one when it is the walk's `stop`)."""
        head = self.segmentation_output
        hw = head.weight.detach().view(head.out_channels, -1)
        dw = db = None
        if not grad_only:
            dw = self._grad_view(head.weight).view(head.out_channels, -1)
            db = self._grad_view(head.bias)
        if walk.fused:
            # g is the final gradient of the last decoder layer's output: the head's backward
            # also leaves the reductions of that layer's InstanceNorm backward (NextNorm)
            last = grad_only and rec is walk.saved[walk.stop_at]
            if self.fullres_folds and not grad_only and walk.mode == "fp32" and \
                    not _hooked(rec.bwd_hooks, "_backward_hooks") and \
                    getattr(self, "_debug_capture", None) is None:
                # nothing but that layer's InstanceNorm backward reads g: it runs inside the
                # head's backward and g is never stored (the NextNorm then says `applied`)
                l = rec.layer
                return ops.head1x1_in_bwd_fold(rec.output(), walk.slope, dout, hw, dw, db,
                                               rec.next_norm(), self._grad_view(l.norm.weight),
                                               self._grad_view(l.norm.bias),
                                               self._grad_view(l.conv.bias))
            return ops.head1x1_in_bwd(rec.output(), walk.slope, dout, hw, dw, db,
                                      nxt=None if last else rec.next_norm())
        return ops.head1x1_bwd(rec.a, dout, hw, dw, db)

    # -- reference: Our_UNet/models/unet.py:386-397 --------------------------------------
    def initialize_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="leaky_relu")
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.InstanceNorm2d):
                if m.weight is not None:
                    nn.init.constant_(m.weight, 1)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    # -- fused-plan construction -------------------------------------------------------------
    def _block_layers(self, block, first_of_decoder, prefix):
        return _parse_block(block, first_of_decoder, prefix)

    def _build_plan(self):
        enc = [self._block_layers(b, False, f"encoder_stages.{i}")
               for i, b in enumerate(self.encoder_stages)]
        dec = [self._block_layers(b.conv_block, True, f"decoder_stages.{i}.conv_block")
               for i, b in enumerate(self.decoder_stages)]
        self._check_head()
        if enc[0][0].stride != 1:
            raise NotImplementedError("first encoder conv must be stride 1")
        self._plan = (enc, dec)
        return self._plan

    def load_pretrained_encoder(self, pretrained, freeze=True):
        """Counterpart of AE_pretrained/transfer_learning/models/unet.py:409-454: load
        `encoder_stages.*` from a checkpoint (path, full checkpoint dict or state_dict) and
        freeze the encoder.  Files are read with `torch.load(..., weights_only=True)`."""
        ckpt = pretrained
        if isinstance(pretrained, (str, bytes)) or hasattr(pretrained, "__fspath__"):
            ckpt = torch.load(pretrained, map_location="cpu", weights_only=True)
        if "model_state_dict" in ckpt:
            ckpt = ckpt["model_state_dict"]
        if "encoder_stages" in ckpt and isinstance(ckpt["encoder_stages"], dict):
            enc_sd = ckpt["encoder_stages"]
        else:
            enc_sd = {k[len("encoder_stages."):]: v for k, v in ckpt.items()
                      if k.startswith("encoder_stages.")}
        own = self.encoder_stages.state_dict()
        matched = {k: v for k, v in enc_sd.items() if k in own and own[k].shape == v.shape}
        self.encoder_stages.load_state_dict(matched, strict=False)
        if freeze:
            for p in self.encoder_stages.parameters():
                p.requires_grad = False
        return sorted(set(own) - set(matched))     # keys that could not be loaded

    def check_supported(self):
        """Raise NotImplementedError unless this configuration is covered by the HIP path
        (3x3 / pad 1 / stride 1|2 convs with bias, InstanceNorm2d(affine), LeakyReLU,
        optional SpatialDropout2d, 32 -> 3 head).  Works without a GPU."""
        self._build_plan()
        return True

    # -- flat parameter / gradient arenas -------------------------------------------------------
    def _ensure_arena(self, params=None):
        # (a walk of the module tree - 182 modules - costs ~70 us of host time: callers that
        # already hold the parameter list pass it in)
        if params is None:
            params = list(self.parameters())
        dev = params[0].device
        ok = self._arena is not None and self._arena.device == dev
        if ok:
            base = self._arena.data_ptr()
            for p, off in zip(params, self._offsets):
                if p.data_ptr() != base + 4 * off:
                    ok = False
                    break
        if ok:
            return
        offsets, total = [], 0
        for p in params:
            if p.dtype != torch.float32 or p.device != dev:
                raise RuntimeError("all UNet parameters must be fp32 on one device")
            offsets.append(total)
            total += (p.numel() + 3) // 4 * 4
        arena = torch.zeros(total, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for p, off in zip(params, offsets):
                view = arena[off:off + p.numel()].view(p.shape)
                view.copy_(p.data)
                p.data = view
        self._arena, self._offsets = arena, offsets
        self._grad_arena = torch.zeros(total, dtype=torch.float32, device=dev)

    def flat_parameters(self):
        """(param_arena, grad_arena): flat fp32 views that alias every parameter / gradient."""
        self._ensure_arena()
        return self._arena, self._grad_arena

    def _grad_view(self, p):
        idx = self._param_index[id(p)]
        off = self._offsets[idx]
        return self._grad_arena[off:off + p.numel()].view(p.shape)

    # -- forward ----------------------------------------------------------------------------------
    def forward(self, x, extra=None, input_layout="nchw"):
        """`input_layout="nhwc"` takes the fp32 [N,H,W,3] tensor of `ops.preprocess_u8` directly;
        `"nhwc_u8"` takes the dataset's uint8 [N,H,W,3] batch itself: its normalisation
        ((v / 255) - input_mean) / input_std (Our_UNet/src/train.py:303-308) then runs inside the
        loaders of the first convolution and of its weight gradient, in every `matmul_precision`
        (fused pipeline, W % 128 == 0; other cases go through `ops.preprocess_u8`)."""
        u8 = None
        if input_layout == "nhwc_u8":
            if x.dtype != torch.uint8:
                raise TypeError("input_layout='nhwc_u8' takes a uint8 [N,H,W,3] tensor")
            # (bottleneck features in the bf16 mode run the stand-alone passes: _Walk.fused)
            fusable = self.fused_pipeline and x.is_cuda and x.dim() == 4 and \
                x.shape[2] % 128 == 0 and not (self.matmul_precision == "bf16" and extra is not None)
            if fusable:
                u8 = ops.U8Image(x.contiguous(), self.input_mean, self.input_std)
            else:
                x = ops.preprocess_u8(x.contiguous(), None, self.input_mean, self.input_std)[0]
            x = x.permute(0, 3, 1, 2)
        elif input_layout == "nhwc":
            x = x.permute(0, 3, 1, 2)      # a view: the shape checks below see NCHW sizes
        elif input_layout != "nchw":
            raise ValueError("input_layout must be 'nchw', 'nhwc' or 'nhwc_u8'")
        self._check_input(x)
        self._check_hooks()
        params = list(self.parameters())
        self._ensure_arena(params)
        self._param_index = {id(p): i for i, p in enumerate(params)}
        if u8 is not None:
            x_nhwc = u8
        elif input_layout != "nchw":
            x_nhwc = x.permute(0, 2, 3, 1).contiguous().float()     # already NHWC in memory
        else:
            x_nhwc = ops.nchw_to_nhwc(x.contiguous().float())
        return _UNetFunction.apply(self, x_nhwc, self._bottleneck_input(x, extra), *params)

    def _check_input(self, x):
        """The checks every walk starts with (x: NCHW sizes); builds the plan."""
        if not x.is_cuda:
            raise RuntimeError("unet-implementations_amd.UNet runs on MI355X only: move the model "
                               "and the input to a ROCm device (no CPU fallback exists)")
        if x.dim() != 4 or x.shape[1] != self.in_channels or self.in_channels != 3:
            raise ValueError("expected an NCHW batch with 3 channels")
        n_down = self.n_stages - 1
        if x.shape[2] % (1 << n_down) or x.shape[3] % (1 << n_down) or \
                min(x.shape[2], x.shape[3]) < (2 << n_down):
            raise ValueError(f"H and W must be multiples of {1 << n_down} and >= {2 << n_down}")
        if self._plan is None:
            self._build_plan()

    def _check_hooks(self):
        """The fused walk fires hooks of the stage-level modules only (encoder_stages[i],
        decoder_stages[i], its conv_block, segmentation_output, the model itself).  A hook on any
        other sub-module (an inner Conv2d / norm / activation, a `.block` Sequential - the
        reference's Grad-CAM helper accepts any target layer, Our_UNet/utils/visualize.py:
        401-402) would never fire: raise instead of letting the caller fail later on a missing
        feature map."""
        inner = self.__dict__.get("_inner_modules")
        if inner is None:
            ok = {id(self), id(self._head_module()), id(self.encoder_stages),
                  id(self.decoder_stages)}
            ok.update(id(m) for m in self.encoder_stages)
            for d in self.decoder_stages:
                ok.update((id(d), id(d.conv_block)))
            inner = self.__dict__["_inner_modules"] = [
                (n, m) for n, m in self.named_modules() if id(m) not in ok]
        for name, m in inner:
            if m._forward_hooks or m._forward_pre_hooks or m._backward_hooks or \
                    m._backward_pre_hooks:
                raise NotImplementedError(
                    f"a hook is registered on {name}: the fused HIP walk never calls inner "
                    "modules, so it would not fire.  Hook a stage-level module instead "
                    "(encoder_stages[i], decoder_stages[i], decoder_stages[i].conv_block, "
                    "segmentation_output).")

    def _bottleneck_input(self, x, extra):
        """Second source of the bottleneck fusion layer (NHWC) or None; CLIPUNet overrides."""
        if extra is not None:
            raise TypeError("this UNet takes no extra bottleneck features")
        return None


def _draw_masks(model, layers, n, device):
    """Dropout masks in forward order; mirrors the reference's per-module draws."""
    if model.dropout_mask_override is not None:
        it = iter(model.dropout_mask_override)
        return [next(it).to(device=device, dtype=torch.float32).contiguous()
                if (l.drop is not None and l.drop.drop_prob > 0) else None for l in layers]
    if not model.training:
        return [None] * len(layers)
    # every SpatialDropout2d's [N, C] mask from ONE bernoulli draw over a cached vector of keep
    # probabilities (2 launches instead of 2 per module; same distribution as the per-module
    # `new_empty(N, C, 1, 1).bernoulli_(1 - p).div_(1 - p)` of the reference)
    sizes = [n * l.conv.out_channels if (l.drop is not None and l.drop.drop_prob > 0) else 0
             for l in layers]
    total = sum(sizes)
    if total == 0:
        return [None] * len(layers)
    key = (n, str(device), tuple(sizes), tuple(l.drop.drop_prob if s else 0.0
                                               for l, s in zip(layers, sizes)))
    cache = model.__dict__.get("_keep_cache")
    if cache is None or cache[0] != key:
        keep = torch.cat([torch.full((s,), 1.0 - l.drop.drop_prob) for l, s in zip(layers, sizes)
                          if s]).to(device)
        cache = model.__dict__["_keep_cache"] = (key, keep)
    keep = cache[1]
    flat = torch.bernoulli(keep).div_(keep)
    out, pos = [], 0
    for l, s in zip(layers, sizes):
        out.append(flat[pos:pos + s].view(n, l.conv.out_channels) if s else None)
        pos += s
    return out


def _hooked(mods, attr):
    return [m for m in mods if getattr(m, attr, None)]


def _fire_forward_hooks(mods, make_output):
    """nn.Module forward hooks of stage-level sub-modules (encoder_stages[i], decoder_stages[i],
    its conv_block, segmentation_output), which the fused walk never calls: the stage output is
    materialised (NCHW fp32) only when such a hook exists and handed to it as `output` (the
    reference's Grad-CAM helper, Our_UNet/utils/visualize.py:392-402).  Hooks observe: a hook
    that returns a replacement output is not supported on this path."""
    mods = _hooked(mods, "_forward_hooks")
    if not mods:
        return
    out = make_output()
    for m in mods:
        for hook in list(m._forward_hooks.values()):
            if hook(m, (None,), out) is not None:
                raise NotImplementedError("forward hooks that replace the output of a sub-module "
                                          "are not supported on the HIP path")


def _fire_backward_hooks(mods, make_grad):
    """register_backward_hook / register_full_backward_hook of the same sub-modules: called with
    grad_output = (dL/d output,) when the backward walk reaches the stage (grad_input is not
    materialised: (None,))."""
    mods = _hooked(mods, "_backward_hooks")
    if not mods:
        return
    g = make_grad()
    for m in mods:
        for hook in list(m._backward_hooks.values()):
            hook(m, (None,), (g,))


class _Walk:
    """State of one walk over the plan: made by the forward and, where a gradient is needed, kept
    for its backward.  The methods run ONE layer; which layer runs when, and which hooks fire, is
    the schedule in `_UNetFunction._forward` / `._backward`."""

    def __init__(self, model, x, fusion, need_grad):
        mode = model.matmul_precision      # operand mode handed to every conv call
        if mode not in ("fp32", "bf16", "bf16x3"):
            raise ValueError("matmul_precision must be 'fp32', 'bf16' or 'bf16x3'")
        enc, dec = model._plan
        layers = [l for blk in enc for l in blk] + ([fusion] if fusion is not None else []) + \
            [l for blk in dec for l in blk]
        self.model, self.mode = model, mode
        self.need_grad = need_grad         # False under no_grad / frozen parameters: no records
        self.saved = []                    # one _Rec per layer, forward order
        self.head_out = None               # what a head keeps for its own backward (Autoencoder)
        self.stop_at = None                # gradient-only backward: index of the target's record
        # The fused pipeline serves the fp32 mode and the mixed-precision mode ("bf16": there the
        # layer tensors themselves are bf16 in HBM); 0 <= slope <= 1 (lrelu(z) = max(z, slope z)),
        # one slope for the whole net.  Anything else runs the stand-alone passes.
        self.slope = layers[0].slope
        self.fused = model.fused_pipeline and \
            len({l.slope for l in layers}) == 1 and 0.0 <= self.slope <= 1.0 and \
            not (mode == "bf16" and fusion is not None)
        self.b16 = self.fused and mode == "bf16"
        # split-bf16 mode on the fused pipeline: the stride-1 3x3 layers that tile as 4 x 32
        # pixels run the split patch kernel (forward + data gradient), the rest the fp32 kernels
        self.x3 = self.fused and mode == "bf16x3"
        # test hook: a list that receives (layer name, raw conv output y, statistics [4,N,C]) of
        # every fused layer in forward order (tests/test_net_gpu.py: the LeakyReLU branch pattern)
        self.dbg_fwd = getattr(model, "_debug_forward", None)

        dev = x.x.device if isinstance(x, ops.U8Image) else x.device
        use_masks = model.training or model.dropout_mask_override is not None
        masks = _draw_masks(model, layers, x.shape[0], dev) if use_masks else [None] * len(layers)
        self.mask_of = {id(l): m for l, m in zip(layers, masks)}

        # one launch packs every 3x3 weight into the kernels' layouts (persistent buffers); in
        # the fp32 mode the stride-1 layers with >= 64 channels also get their Winograd forms
        # U = G g G^T (forward, incl. the up-sampling loader of the decoder's first convolutions;
        # data gradient: the C -> C layers and the skip halves of the decoder's first
        # convolutions) - `weight_forms` picks per call
        convs = [l.conv.weight for l in layers if l.ksize == 3]
        wino = None
        if mode == "fp32" and model.fused_pipeline and model.winograd:
            wino = []
            for l in layers:
                if l.ksize != 3:
                    continue
                co, ci = l.conv.weight.shape[0], l.conv.weight.shape[1]
                s1 = l.stride == 1 and min(co, ci) >= 64
                wino.append((s1 and co % 64 == 0 and ci % 8 == 0,
                             s1 and ci % 64 == 0 and co % 8 == 0))
        # (the 32 -> 32 channel layers' Winograd form needs no weight form of its own: a switch)
        table = model.__dict__.get("_pack_table")
        # (the bf16 planes: all three terms in the split mode; in the mixed-precision mode their
        # first plane is the bf16-rounded weight the patch kernels stage without a conversion)
        planes = 3 if mode == "bf16x3" else (1 if (mode == "bf16" and model.fused_pipeline) else False)
        if table is None or not table.matches(convs, planes, wino):
            table = model.__dict__["_pack_table"] = ops.PackTable(convs, planes, wino)
        table.run()
        self.table = table
        self.row = {id(w): k for k, w in enumerate(convs)}    # weight -> its PackTable row

    def weight_forms(self, l, s0, s1, up=False):
        """THE place that picks a layer's weight forms -> ((w, w3, wu), (wd, wd3, ud, ud1)): what
        the forward call takes and what its record keeps for the backward (`_Rec`).  w / wd are
        the packed fp32 layouts (1x1: the matrix and its transpose), w3 / wd3 the PackTable's bf16
        planes (None in the fp32 mode), wu / ud / ud1 the Winograd forms where the table holds one
        AND the library tiles this call's shape.  s0, s1: the operands as the call gets them;
        up: s0 is the low-resolution operand that the convolution up-samples on load."""
        w = l.conv.weight
        if l.ksize == 1:
            w2d = w.detach().view(w.shape[0], w.shape[1])
            return (w2d, None, None), \
                (ops.transpose2d(w2d) if self.need_grad else None, None, None, None)
        t, k = self.table, self.row[id(w)]
        wu = ud = ud1 = None
        if self.fused and self.mode == "fp32":
            n, h, w_ = (s1 if up else s0).shape[:3]       # the convolution's output grid
            c0, c1, cout = s0.shape[3], 0 if s1 is None else s1.shape[3], w.shape[0]
            # forward: every source must be activated on load
            if t.uf[k] is not None and s0.alpha is not None and \
                    (s1 is None or s1.alpha is not None) and \
                    (ops.conv_up_wino_supported if up else ops.conv_wino_supported)(
                        n, h, w_, c0, c1, cout):
                wu = t.uf[k]
            # data gradient: into the skip half of an up-sampling layer, or into a lone source
            if t.ud[k] is not None:
                if up:
                    if self.need_grad and ops.conv_wino_supported(n, h, w_, cout, 0, c1):
                        ud1 = t.ud[k]
                elif c1 == 0 and ops.conv_wino_supported(n, h, w_, cout, 0, c0):
                    ud = t.ud[k]
        return (t.wf[k], t.wf3[k], wu), (t.wd[k], t.wd3[k], ud, ud1)

    def run_layer(self, l, x0, x1, place):
        """Stand-alone pipeline: convolution, statistics and activation as three passes over NHWC
        fp32 tensors; returns the activated output."""
        (w, w3, _), bwd_forms = self.weight_forms(l, x0, x1)
        if l.ksize == 1:
            y = ops.conv1x1_fwd(x0, x1, w, l.conv.bias.detach())
        else:
            y = ops.conv3x3_fwd(x0, x1, w, l.conv.bias.detach(), l.stride, bf16=self.mode, wf3=w3)
        st = ops.instnorm_stats(y, l.norm.weight.detach(), l.norm.bias.detach(), l.norm.eps)
        m = self.mask_of[id(l)]
        a = ops.instnorm_lrelu_drop_fwd(y, st[2], st[3], m, l.slope)
        if self.need_grad:
            self.saved.append(_Rec(l, x0, x1, y, st, m, bwd_forms, place, a=a))
        return a

    def run_layer_fused(self, l, s0, s1, place, low=None):
        """s0 / s1: ops.Act operands; returns the Act of this layer's output.  low: s0 is only the
        up-sampling of this Act - the backward works on `low` and s0 is not kept."""
        (w, w3, wu), bwd_forms = self.weight_forms(l, s0, s1)
        m = self.mask_of[id(l)]
        y, st = ops.conv_in_fwd(s0, s1, self.slope, w, l.conv.bias.detach(), l.ksize, l.stride,
                                l.norm.weight.detach(), l.norm.bias.detach(), l.norm.eps, m,
                                b16=self.b16, w3=w3, wu=wu)
        return self._fused_output(l, None if low is not None else s0, s1, low, y, st, m,
                                  bwd_forms, place)

    def run_up_layer(self, l, low, skip, place):
        """First conv of a decoder stage: conv3x3(cat(upsample2x(act(low)), act(skip)))."""
        if not self.fused:
            return self.run_layer(l, ops.upsample2x_fwd(low), skip, place)
        if self.x3 or l.ksize != 3 or \
                not ops.conv_up_in_fwd_supported(low, skip, l.conv.weight.shape[0]):
            return self.run_layer_fused(l, ops.Act(ops.upsample2x_in_fwd(low, self.slope)), skip,
                                        place, low=low)
        # the bilinear gather runs inside the conv's patch loader: the up-sampled tensor never
        # exists, and the backward works on `low` (ops.conv3x3_up_bwd_weight / _data)
        (w, w3, wu), bwd_forms = self.weight_forms(l, low, skip, up=True)
        m = self.mask_of[id(l)]
        y, st = ops.conv_up_in_fwd(low, skip, self.slope, w, l.conv.bias.detach(),
                                   l.norm.weight.detach(), l.norm.bias.detach(), l.norm.eps, m,
                                   wu=wu, w3=w3)
        return self._fused_output(l, None, skip, low, y, st, m, bwd_forms, place)

    def _fused_output(self, l, x0, x1, low, y, st, m, bwd_forms, place):
        if self.need_grad:
            self.saved.append(_Rec(l, x0, x1, y, st, m, bwd_forms, place, low=low))
        if self.dbg_fwd is not None:
            self.dbg_fwd.append((l.name, y, st))
        return ops.Act(y, st[2], st[3])

    def stage_output(self, v):
        """activated stage output as an NCHW fp32 tensor (only materialised for hooks)"""
        if isinstance(v, ops.Act):
            if v.x.dtype != torch.float32:
                raise NotImplementedError("sub-module hooks on the bf16 pipeline")
            a = v.x if v.alpha is None else ops.instnorm_lrelu_drop_fwd(v.x, v.alpha, v.beta,
                                                                        None, self.slope)
            return ops.nhwc_to_nchw(a)
        return ops.nhwc_to_nchw(v)

    def layer_bwd(self, i, g_a, stop, dx0_acc=None, grad_only=False):
        """Backward of layer `i` from g_a = dL/d(its activated output) -> (dx0, dx1): the gradients
        of its operands (dx0 on the low-resolution grid where the layer up-sampled on load).
        stop: index of the first trainable layer - the gradient into layer j's input is needed
        only for j > stop.  dx0_acc: the gradient another consumer of x0 already wrote (a skip):
        dx0 is accumulated into it.  grad_only: the data gradients and the InstanceNorm backward
        alone - no weight, bias or affine gradient is formed and the gradient arena is not
        touched; layer `stop` itself gets no backward (its output gradient is the result)."""
        rec = self.saved[i]
        l, st, x0, x1, low = rec.layer, rec.st, rec.x0, rec.x1, rec.low
        fused, slope = self.fused, self.slope
        gv = (lambda p: None) if grad_only else self.model._grad_view
        need_dx = i > stop
        need_dx1 = rec.skip_dst is not None and rec.skip_dst > stop
        dbg = getattr(self.model, "_debug_capture", None)
        if dbg is not None:
            dbg.append((l.name, "ga", g_a.clone()))
        nn_, rec.nxt = rec.nxt, None       # reductions left by the kernel that produced g_a
        # dx0 of this layer is the final gradient of the previous layer's output (the skip
        # halves dx1 are accumulated into later, by the encoder): its producer also emits
        # that layer's InstanceNorm-backward reductions
        nxt = self.saved[i - 1].next_norm() \
            if fused and need_dx and not (grad_only and i - 1 == stop) else None
        dw = gv(l.conv.weight)
        want_dw = l.conv.weight.requires_grad and not grad_only
        partials = (nn_.partial, nn_.tiles) if nn_ is not None and nn_.tiles > 0 else None
        if i == 0 and fused and want_dw and partials is not None and dbg is None and \
                self.mode == "fp32" and x1 is None and low is None and l.ksize == 3 and \
                self.model.fullres_folds and ops.stem_in_bwd_weight_fold_supported(x0, g_a):
            # the RGB stem: no gradient goes on to the image, so its dL/dz is read by the weight
            # gradient alone - whose loader forms it from g_a and y (never stored)
            ops.stem_in_bwd_weight_fold(x0, g_a, rec.y, st[0], st[1], l.norm.weight.detach(),
                                        l.norm.bias.detach(), rec.mask, l.slope, partials, dw,
                                        gv(l.norm.weight), gv(l.norm.bias), gv(l.conv.bias))
            return None, None
        # the 32 -> 32 channel layers at full resolution: the Winograd weight gradient (of the
        # skip half where the layer up-samples its first operand) forms dz itself and leaves it
        # in g_a for the gradients that follow
        xw = x1 if low is not None else x0
        fold32 = fused and want_dw and partials is not None and dbg is None and \
            self.mode == "fp32" and not self.x3 and l.ksize == 3 and l.stride == 1 and \
            self.model.wgrad32_folds and not (nn_ is not None and nn_.applied) and \
            (low is not None or x1 is None) and xw is not None and \
            not _hooked(rec.bwd_hooks, "_backward_hooks") and \
            ops.conv_in_bwd_weight_fold32_supported(xw, g_a)
        if nn_ is not None and nn_.applied:
            dy = g_a       # head1x1_in_bwd_fold: the producer already went on to dL/dz
        elif fold32:
            dy = ops.conv_in_bwd_weight_fold32(
                xw, slope, g_a, rec.y, st[0], st[1], l.norm.weight.detach(), l.norm.bias.detach(),
                rec.mask, l.slope, partials, dw, low.shape[3] if low is not None else 0,
                gv(l.norm.weight), gv(l.norm.bias), gv(l.conv.bias))
        else:
            dy = ops.instnorm_lrelu_drop_bwd(g_a, rec.y, st[0], st[1], l.norm.weight.detach(),
                                             l.norm.bias.detach(), rec.mask, l.slope,
                                             gv(l.norm.weight), gv(l.norm.bias), gv(l.conv.bias),
                                             partials=partials)
        if dbg is not None:
            dbg.append((l.name, "dy", dy.clone()))
        if low is not None:
            # conv3x3(upsample2x(act(low))): both gradients of the up-sampled operand are
            # GEMMs over the LOW-resolution pixels once dy is reduced to its nine D_tap
            C0 = low.shape[3]
            D = ops.upsample2x_bwd_taps(dy) if (want_dw or need_dx) else None
            if want_dw:
                ops.conv3x3_up_bwd_weight(low, slope, D, dw, 0)
                if not fold32:
                    ops.conv_in_bwd_weight(x1, slope, dy, dw, C0, 3, 1, x3=self.x3)
            g_low = ops.conv3x3_up_bwd_data(D, rec.wd, 0, C0, nxt=nxt,
                                            wd3=rec.wd3 if ops._is_b16(D) else None) \
                if need_dx else None
            dx1 = ops.conv3x3_bwd_data(dy, rec.wd, C0, x1.shape[3], x1.shape[1], x1.shape[2], 1,
                                       wd3=rec.wd3,
                                       bf16="bf16x3" if rec.wd3 is not None else False,
                                       ud=rec.ud1) if need_dx1 else None
            return g_low, dx1
        if want_dw and fused and fold32:
            want_dw = False
        elif want_dw and fused:      # the weight gradient activates its operand on load
            ops.conv_in_bwd_weight(x0, slope, dy, dw, 0, l.ksize, l.stride, x3=self.x3)
            if x1 is not None:
                ops.conv_in_bwd_weight(x1, slope, dy, dw, x0.shape[3], l.ksize, l.stride,
                                       x3=self.x3)
            want_dw = False
        if l.ksize == 1:
            if want_dw:
                dw2d = dw.view(dw.shape[0], dw.shape[1])
                ops.conv1x1_bwd_weight(x0, dy, dw2d, 0)
                if x1 is not None:
                    ops.conv1x1_bwd_weight(x1, dy, dw2d, x0.shape[3])
            dx0 = ops.conv1x1_bwd_data(dy, rec.wd, 0, x0.shape[3]) if need_dx else None
            return dx0, None      # the second source (frozen CLIP features) needs no gradient
        if want_dw:
            ops.conv3x3_bwd_weight(x0, dy, dw, 0, l.stride, bf16=self.mode)
            if x1 is not None:
                ops.conv3x3_bwd_weight(x1, dy, dw, x0.shape[3], l.stride, bf16=self.mode)
        dx0 = dx1 = None
        N, H, W, C0 = x0.shape
        if need_dx:
            dx0 = ops.conv3x3_bwd_data(dy, rec.wd, 0, C0, H, W, l.stride, out=dx0_acc,
                                       accumulate=dx0_acc is not None, bf16=self.mode,
                                       wd3=rec.wd3, nxt=nxt, ud=rec.ud)
        if x1 is not None and need_dx1:
            dx1 = ops.conv3x3_bwd_data(dy, rec.wd, C0, x1.shape[3], H, W, l.stride,
                                       bf16=self.mode, wd3=rec.wd3)
        return dx0, dx1


class _UNetFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, x, extra, *params):
        # The 32-channel layers' kernel choice is made HERE, applied to this walk's calls only and
        # saved for the backward walk (which may run on autograd's own thread, after other
        # models ran): the library's switch is per calling thread.
        c32_mode = "always" if ops.c32_winograd_override() == "always" else bool(model.winograd)
        with ops.c32_winograd_scope(c32_mode):
            logits = _UNetFunction._forward(ctx, model, x, extra, params)
        if any(ctx.needs_input_grad):
            ctx.c32_mode = c32_mode
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        # The slab reductions of the weight gradients (2-3 small launches per gradient, 44 per
        # step) are queued and launched together: at the end of the walk, or - with a
        # data-parallel hook - whenever a stage's gradients are handed to the exchange.
        with ops.c32_winograd_scope(ctx.c32_mode), ops.wgrad_deferral() as deferred:       # (the forward's decision)
            return _UNetFunction._backward(ctx, dlogits, deferred)

    @staticmethod
    def _forward(ctx, model, x, extra, params, fire_hooks=True):
        fire = _fire_forward_hooks if fire_hooks else (lambda mods, make_output: None)
        enc, dec = model._plan
        fusion = model._fusion_layer if extra is not None else None
        walk = _Walk(model, x, fusion, any(ctx.needs_input_grad))
        fused = walk.fused
        if isinstance(x, ops.U8Image) and not fused:
            raise RuntimeError("the uint8 stem needs the fused pipeline")
        run = walk.run_layer_fused if fused else walk.run_layer
        # (the image is a plain operand of the fused pipeline)
        cur = ops.Act(x) if fused and not isinstance(x, ops.U8Image) else x

        def place(blk, li, hooked, owner, skip_dst=None):
            """(bwd_hooks, completes, skip_dst) of layer li of a stage: see _Rec"""
            return (hooked if li == len(blk) - 1 else (), owner if li == 0 else None, skip_dst)

        skips = []      # (stage output, index of the record that will take it as x0)
        for bi, blk in enumerate(enc):
            stage = model.encoder_stages[bi]
            for li, l in enumerate(blk):
                cur = run(l, cur, None, place(blk, li, (stage,), stage))
            if bi < len(enc) - 1:
                skips.append((cur, len(walk.saved)))
            fire([stage], lambda: walk.stage_output(cur))
        if fusion is not None:
            if extra.shape[:3] != cur.shape[:3]:
                raise NotImplementedError("bottleneck features must match the 1/32-resolution "
                                          f"grid {tuple(cur.shape[1:3])} (got {tuple(extra.shape[1:3])})")
            cur = run(fusion, cur, ops.Act(extra) if fused else extra,
                      ((), model.clip_fusion_conv, None))
        for di, blk in enumerate(dec):
            stage = model.decoder_stages[di]
            hooked = (stage, stage.conv_block)
            skip, skip_dst = skips[len(skips) - 1 - di]
            if cur.shape[1] * 2 != skip.shape[1] or cur.shape[2] * 2 != skip.shape[2]:
                raise NotImplementedError("decoder up-sampling must be exactly 2x")
            cur = walk.run_up_layer(blk[0], cur, skip, place(blk, 0, hooked, stage, skip_dst))
            for li in range(1, len(blk)):
                cur = run(blk[li], cur, None, place(blk, li, hooked, stage))
            fire(hooked, lambda: walk.stage_output(cur))
        logits = model._head_fwd(walk, cur)
        fire([model._head_module()], lambda: logits)
        if walk.need_grad:
            ctx.walk, ctx.params = walk, params
        return logits

    @staticmethod
    def _backward(ctx, dlogits, deferred):
        walk, params = ctx.walk, ctx.params
        model, saved = walk.model, walk.saved
        gv = model._grad_view
        dlogits = dlogits.contiguous()
        # The kernels WRITE the gradient arena and the returned views normally become p.grad.
        # A gradient that already exists (a second backward before the step, or
        # zero_grad(set_to_none=False)) must be accumulated into instead: arena-aliased ones
        # are saved here and added back below (autograd gets None for them: adding the returned
        # view to itself would double it); foreign tensors are left to autograd's own `+=`.
        gbase = model._grad_arena.data_ptr()
        carried = {}
        for p, off in zip(params, model._offsets):
            if p.grad is not None and p.grad.data_ptr() == gbase + 4 * off:
                carried[id(p)] = p.grad.detach().clone()
        if carried and model.grad_ready_hook is not None:
            raise RuntimeError(
                "gradient accumulation (a parameter already has .grad) cannot be combined with "
                "the bucketed all-reduce hook: the buckets would ship before the old gradient is "
                "added.  Clear model.grad_ready_hook for the accumulation micro-steps, or call "
                "optimizer.zero_grad() (set_to_none=True) before each backward.")
        head = model._head_module()
        g = model._head_bwd(walk, saved[-1], dlogits)
        hook = model.grad_ready_hook

        def ready(module):
            if hook is not None:
                deferred.flush()      # the gradients handed over must be final
                first = next(module.parameters())     # (only with a data-parallel hook installed)
                hook(model._offsets[model._param_index[id(first)]])

        ready(head)
        _fire_backward_hooks([head], lambda: dlogits)

        def grad_nchw(t):
            if t.dtype != torch.float32:
                raise NotImplementedError("sub-module hooks on the bf16 pipeline")
            return ops.nhwc_to_nchw(t)

        def layer_params(l):
            return (l.conv.weight, l.conv.bias, l.norm.weight, l.norm.bias)

        # Frozen layers (AE-transfer freezes encoder_stages): nothing upstream of
        # the first trainable layer needs a backward pass, and frozen layers in between only
        # propagate the data gradient (no weight-gradient kernels).
        stop = min((i for i, r in enumerate(saved)
                    if any(q.requires_grad for q in layer_params(r.layer))), default=len(saved))
        skip_grads = {}      # index of a record -> the skip gradient its dx0 is accumulated into
        for i in range(len(saved) - 1, stop - 1, -1):
            rec = saved[i]
            _fire_backward_hooks(rec.bwd_hooks, lambda: grad_nchw(g))
            g, g_skip = walk.layer_bwd(i, g, stop, dx0_acc=skip_grads.pop(i, None))
            if g_skip is not None:
                skip_grads[rec.skip_dst] = g_skip
            if rec.layer.first_of_decoder and rec.low is None and g is not None:
                g = ops.upsample2x_bwd(g)     # the up-sampled operand was materialised
            if rec.completes is not None:
                ready(rec.completes)
        deferred.flush()
        if hook is not None:
            # everything below the first trainable parameter is a frozen prefix: no gradient,
            # nothing to exchange
            hook(next((off for p, off in zip(params, model._offsets) if p.requires_grad), 0))
        # ids of the parameters whose gradient this backward produced
        touched = {id(q) for q in head.parameters()}
        touched.update(id(q) for r in saved[stop:] for q in layer_params(r.layer))
        walk.saved = None
        grads = []
        for p in params:
            # no gradient for frozen parameters and for layers that did not run (e.g. the CLIP
            # fusion layer when no features were passed): like the reference, .grad stays None
            if not p.requires_grad or id(p) not in touched:
                grads.append(None)
            elif id(p) in carried:
                gv(p).add_(carried[id(p)])     # p.grad is this view: accumulated in place
                grads.append(None)
            else:
                grads.append(gv(p))
        return (None, None, None, *grads)


class _GradOnlyCtx:
    """What `_UNetFunction._forward` needs of an autograd context when the walk is run by hand."""
    needs_input_grad = (True,)


def stage_feature_and_gradient(model, x, target_class, target):
    """(A, G, slope) for Grad-CAM: A = the output of the stage module `target` in eval mode, as the
    walk holds it (ops.Act: raw convolution output + folded InstanceNorm coefficients; the
    activated NHWC tensor on the stand-alone pipeline), and G = d mean_hw(logits[b, target_class])
    / dA, an NHWC tensor of the walk's storage type - the tensors a forward hook and a backward
    hook on `target` see (for an encoder stage G includes the skip path's share).  The images of a
    batch are independent (InstanceNorm, no dropout), so one seed dlogits[b, c] = 1 / (H W) gives
    every image's own gradient.

    The backward walks from the head down to the target only, with the data-gradient and
    InstanceNorm-backward kernels alone: no weight, bias or affine gradient, no write to the
    gradient arena or to any .grad, no hook is fired or needed.  model.training and
    dropout_mask_override are put back."""
    if type(model)._head_bwd is not UNet._head_bwd or model._fusion_layer is not None:
        raise NotImplementedError("Grad-CAM on the HIP path covers UNet (not CLIPUNet / Autoencoder)")
    K = model._head_module().out_channels
    if K != 3:
        raise NotImplementedError(f"Grad-CAM on the HIP path covers the 3-class model (got {K} "
                                  "classes)")
    model._check_input(x)
    if not 0 <= int(target_class) < K:
        raise ValueError(f"target_class {target_class} is outside [0, {K})")
    was_training, override = model.training, model.dropout_mask_override
    # the mode of this pass may differ from the model's (evaluate.gradcam): keep the model's own
    # packed weights for its next step
    table = model.__dict__.get("_pack_table")
    model.eval()
    model.dropout_mask_override = None
    c32_mode = "always" if ops.c32_winograd_override() == "always" else bool(model.winograd)
    try:
        with torch.no_grad(), ops.c32_winograd_scope(c32_mode):
            ctx = _GradOnlyCtx()
            logits = _UNetFunction._forward(ctx, model, ops.nchw_to_nhwc(x.contiguous().float()),
                                            None, None, fire_hooks=False)
            walk, saved = ctx.walk, ctx.walk.saved
            t = next(i for i, r in enumerate(saved) if any(m is target for m in r.bwd_hooks))
            walk.stop_at = t
            dlogits = torch.zeros_like(logits)
            dlogits[:, int(target_class)] = 1.0 / (logits.shape[2] * logits.shape[3])
            g = model._head_bwd(walk, saved[-1], dlogits, grad_only=True)
            skip_grads = {}
            for i in range(len(saved) - 1, t, -1):
                rec = saved[i]
                g, g_skip = walk.layer_bwd(i, g, t, dx0_acc=skip_grads.pop(i, None),
                                           grad_only=True)
                if g_skip is not None:
                    skip_grads[rec.skip_dst] = g_skip
                if rec.layer.first_of_decoder and rec.low is None:
                    g = ops.upsample2x_bwd(g)     # the up-sampled operand was materialised
            feature = saved[t].output()
            walk.saved = None
            return feature, g, walk.slope
    finally:
        model.train(was_training)
        model.dropout_mask_override = override
        if table is not None:
            model.__dict__["_pack_table"] = table
