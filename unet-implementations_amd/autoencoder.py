"""Drop-in `Autoencoder` for the reference's reconstruction pretraining model
(AE_pretrained/reconstruction/models/autoencoder.py:240-466).

The body is `UNet`'s: the same `encoder_stages` / `decoder_stages` (ConvBlock / UpBlock,
InstanceNorm, LeakyReLU, spatial dropout, bilinear 2x concat) run by the same fused HIP walk.
Only the head differs: `reconstruction_output = Sequential(Conv2d(32, 3, 3, padding=1),
Sigmoid())`, run by the recon kernels (csrc/recon.hip) through `UNet`'s head hooks.  The
`state_dict` keys are the reference's: `encoder_stages.*`, `decoder_stages.*`,
`reconstruction_output.0.{weight,bias}`, so a checkpoint's encoder loads with
`UNet.load_pretrained_encoder`.

Operand modes: every mode of `UNet` (fp32 fused / unfused, `matmul_precision="bf16"` with bf16
layer tensors, "bf16x3" with fp32 layer tensors, Winograd on / off) - the head kernels read fp32
or bf16 layer tensors and compute in fp32.
"""
from typing import Dict, List, Optional, Tuple, Type

import torch
import torch.nn as nn

from . import ops
from .unet import UNet, _as_int


class Autoencoder(UNet):
    """6-stage encoder/decoder autoencoder with the reference's constructor surface."""

    def __init__(self, in_channels: int = 3, out_channels: int = 3, n_stages: int = 6,
                 features_per_stage: List[int] = None,
                 kernel_sizes: List[Tuple[int, int]] = None,
                 strides: List[Tuple[int, int]] = None, n_conv_per_stage: List[int] = None,
                 n_conv_per_stage_decoder: List[int] = None, conv_bias: bool = True,
                 norm_op: Type[nn.Module] = nn.InstanceNorm2d, norm_op_kwargs: Dict = None,
                 dropout_op: Optional[Type[nn.Module]] = None, dropout_op_kwargs: Dict = None,
                 nonlin: Type[nn.Module] = nn.LeakyReLU, nonlin_kwargs: Dict = None,
                 encoder_dropout_rates: List[float] = None,
                 decoder_dropout_rates: List[float] = None):
        # (UNet.__init__ builds the modules in the reference's order - the head through
        # _build_head - and then runs initialize_weights: the same RNG draws as the reference)
        super().__init__(in_channels=in_channels, num_classes=out_channels, n_stages=n_stages,
                         features_per_stage=features_per_stage, kernel_sizes=kernel_sizes,
                         strides=strides, n_conv_per_stage=n_conv_per_stage,
                         n_conv_per_stage_decoder=n_conv_per_stage_decoder, conv_bias=conv_bias,
                         norm_op=norm_op, norm_op_kwargs=norm_op_kwargs, dropout_op=dropout_op,
                         dropout_op_kwargs=dropout_op_kwargs, nonlin=nonlin,
                         nonlin_kwargs=nonlin_kwargs,
                         encoder_dropout_rates=encoder_dropout_rates,
                         decoder_dropout_rates=decoder_dropout_rates)
        del self.num_classes
        self.out_channels = out_channels
        # the reference's AE dataset does not normalise: image = uint8 / 255
        # (AE_pretrained/reconstruction/src/train.py:257-266)
        self.input_mean, self.input_std = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)

    # -- head hooks of the fused walk ------------------------------------------------------------
    def _build_head(self, in_features, out_channels):
        self.reconstruction_output = nn.Sequential(
            nn.Conv2d(in_features, out_channels, kernel_size=3, stride=1, padding=1, bias=True),
            nn.Sigmoid())

    def _head_module(self):
        return self.reconstruction_output

    def _check_head(self):
        mods = list(self.reconstruction_output)
        conv = mods[0] if mods else None
        if len(mods) != 2 or not isinstance(conv, nn.Conv2d) or not isinstance(mods[1], nn.Sigmoid):
            raise NotImplementedError("the HIP reconstruction head is Conv2d(32, 3, 3) + Sigmoid")
        if _as_int(conv.kernel_size) != 3 or _as_int(conv.padding) != 1 or \
                _as_int(conv.stride) != 1 or _as_int(conv.dilation) != 1 or conv.groups != 1 or \
                conv.bias is None or conv.in_channels != 32 or conv.out_channels != 3:
            raise NotImplementedError("the HIP reconstruction head is the 32 -> 3 3x3 convolution "
                                      "(pad 1, bias) followed by a sigmoid")

    def _head_fwd(self, walk, cur):
        conv = self.reconstruction_output[0]
        out = ops.recon3x3_fwd(cur if walk.fused else ops.Act(cur), walk.slope,
                               conv.weight.detach(), conv.bias.detach())
        if walk.need_grad:
            walk.head_out = out.detach()     # (an alias without grad_fn: no reference cycle)
        return out

    def _head_bwd(self, walk, rec, dout):
        conv = self.reconstruction_output[0]
        out, walk.head_out = walk.head_out, None
        # fused pipeline: da is the final gradient of the last decoder layer's output, so the
        # head's backward also leaves the reductions of that layer's InstanceNorm backward
        return ops.recon3x3_bwd(rec.output() if walk.fused else ops.Act(rec.a), walk.slope, dout,
                                out, conv.weight.detach(), self._grad_view(conv.weight),
                                self._grad_view(conv.bias),
                                nxt=rec.next_norm() if walk.fused else None)

    # -- reference API ---------------------------------------------------------------------------
    def get_encoder(self):
        return self.encoder_stages

    def get_decoder(self):
        return self.decoder_stages, self.reconstruction_output

    @torch.no_grad()
    def encode(self, x):
        """Bottleneck activations flattened to [N, C*H*W] (NCHW order), as the reference's
        `encode`.  Runs the fused walk with the bottleneck stage's output materialised; not
        differentiable (the pretrained encoder is consumed through its weights)."""
        got = []
        h = self.encoder_stages[-1].register_forward_hook(lambda m, i, o: got.append(o))
        try:
            self.forward(x)
        finally:
            h.remove()
        out = got[0]
        return out.reshape(out.shape[0], -1)
