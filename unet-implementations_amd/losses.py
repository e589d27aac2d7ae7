"""Drop-in `SimpleLoss` (reference: Our_UNet/models/losses.py:5-121).

Dice + cross-entropy with per-batch inverse-frequency class weights and
ignore_index handling.  `forward(logits[N,3,H,W] fp32, target[N,H,W] int64)`
returns a 0-dim fp32 tensor supporting `.backward()` / `.item()`; with
`target_layout="u8"` the target is the dataset's uint8 mask itself.  One fused
kernel sequence computes the loss AND dL/dlogits in the forward call; autograd's
backward only scales that stored gradient.
"""
import torch
import torch.nn as nn

from . import ops


class _LossFunction(torch.autograd.Function):
    """Forward: the loss value and, in the workspace, the class weights / Dice coefficients the
    gradient needs.  Backward: ONE launch of the gradient kernel with autograd's upstream scalar
    applied inside it (`unet_dice_wce_loss_grad`) - no stock-torch scaling pass over dlogits."""

    @staticmethod
    def forward(ctx, logits, target, mod, class_weights):
        want_grad = ctx.needs_input_grad[0]
        world = mod._world()
        if world > 1:
            import torch.distributed as dist
            stats, ws = ops.dice_wce_loss_shard_stats(logits, target, mod.smooth, mod.ignore_index)
            dist.all_reduce(stats, op=dist.ReduceOp.SUM, group=mod.process_group)
            out, _ = ops.dice_wce_loss_shard_apply(
                logits, target, stats, logits.shape[0] * world, ws, mod.smooth, mod.weight_dice,
                mod.weight_ce, mod.ignore_index, mod.dynamic_weights, class_weights=class_weights,
                grad_scale=mod.grad_scale, want_grad=False)
        else:
            ws = ops.dice_wce_loss_workspace(logits)
            out, _ = ops.dice_wce_loss_fwd_bwd(
                logits, target, mod.smooth, mod.weight_dice, mod.weight_ce, mod.ignore_index,
                mod.dynamic_weights, class_weights=class_weights, grad_scale=mod.grad_scale,
                want_grad=False, ws=ws)
        if want_grad:
            ctx.held = (logits, target, ws, mod.ignore_index)
        mod.last_terms = out  # [total, ce, dice, w0, w1, w2, -, -] on device (no sync)
        return out[0].clone()

    @staticmethod
    def backward(ctx, g):
        logits, target, ws, ignore_index = ctx.held
        ctx.held = None
        # g is the 0-dim upstream gradient (1 for loss.backward()), read on the device
        return ops.dice_wce_loss_grad(logits, target, ws, g, ignore_index), None, None, None


class SimpleLoss(nn.Module):
    def __init__(self, weight_dice=1.0, weight_ce=1.0, ignore_index=255, smooth=1e-5,
                 class_weights=None, dynamic_weights=True, batch_sync="local", process_group=None,
                 target_layout="int64"):
        """`target_layout="u8"`: the target is the dataset's uint8 [N,H,W] mask on the device,
        handed to the kernels untouched (1 byte a pixel instead of 8; a raw mask is cleaned on
        load with the dataset's rule v > 2 and v != 255 -> 0).  The loss, `last_terms` and the
        gradient equal those of the default layout on the cleaned mask bit for bit.

        `batch_sync="global"` (data parallel only; not in the reference, which is
        single-process): every rank evaluates the loss of the CONCATENATED batch - class weights,
        CE denominator and the Dice batch mean taken over all ranks' images (equal per-rank batch
        sizes) - so that N ranks x batch b reproduce one process at batch N*b.  Gradients must
        then be summed, not averaged: `ddp.GradBucketAllReduce(..., average=False)`."""
        super().__init__()
        if batch_sync not in ("local", "global"):
            raise ValueError("batch_sync must be 'local' or 'global'")
        if target_layout not in ("int64", "u8"):
            raise ValueError("target_layout must be 'int64' or 'u8'")
        self.target_layout = target_layout
        self.batch_sync = batch_sync
        self.process_group = process_group
        self.weight_dice = weight_dice
        self.weight_ce = weight_ce
        self.ignore_index = ignore_index
        self.smooth = smooth
        self.class_weights = class_weights
        self.dynamic_weights = dynamic_weights
        self.grad_scale = 1.0  # data-parallel training pre-scales the gradient by 1/world
        self.last_terms = None

    def _world(self):
        if self.batch_sync != "global":
            return 1
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return 1
        return dist.get_world_size(self.process_group)

    def forward(self, input, target):
        if not input.is_cuda:
            raise RuntimeError("unet-implementations_amd.SimpleLoss runs on MI355X only "
                               "(no CPU fallback exists)")
        if input.shape[-2:] != target.shape[-2:]:
            # the reference resizes the logits to the target (Our_UNet/models/losses.py:66-68)
            input = ops.resize_bilinear(input, target.shape[-2:])
        if self.target_layout == "u8":
            if target.dtype != torch.uint8 or not target.is_cuda or not target.is_contiguous():
                raise TypeError("target_layout='u8' takes a contiguous uint8 device tensor")
        elif target.dtype != torch.int64:
            target = target.long()
        cw = None
        dynamic = bool(self.dynamic_weights) and target.size(0) > 0
        if not dynamic and self.class_weights is not None:
            cw = torch.as_tensor(self.class_weights, dtype=torch.float32,
                                 device=input.device).contiguous()
        mod = self
        if dynamic != bool(self.dynamic_weights):
            raise NotImplementedError("empty batch")
        return _LossFunction.apply(input.contiguous().float(), target.contiguous(), mod, cw)


class _MSEFunction(torch.autograd.Function):
    """Forward: the loss and the per-image sums of squares (unet_mse_loss_fwd).  Backward: ONE
    launch of the gradient kernel with autograd's upstream scalar applied inside it."""

    @staticmethod
    def forward(ctx, output, target, mod, target_u8):
        loss, per_image = ops.mse_loss_fwd(output, target, target_u8)
        mod.last_per_image = per_image      # fp64 [N] on the device (no sync)
        if ctx.needs_input_grad[0]:
            ctx.held = (output, target, target_u8)
        return loss[0].clone()

    @staticmethod
    def backward(ctx, g):
        output, target, target_u8 = ctx.held
        ctx.held = None
        return ops.mse_loss_grad(output, target, g, target_u8), None, None, None


class MSELoss(nn.Module):
    """`nn.MSELoss()` (reduction "mean") on the HIP path: the autoencoder's loss
    (AE_pretrained/reconstruction/src/train.py:420-437).  `forward(output[N,C,H,W] fp32, target)`
    returns a 0-dim fp32 tensor supporting `.backward()`.  The target is the NCHW fp32 tensor, or -
    with `target_layout="nhwc_u8"` - the dataset's uint8 [N,H,W,3] image itself, read as
    v / 255 rounded once to fp32 (what the reference's CPU dataset computes for
    `image.float() / 255.0`: the two forms give the same loss bit for bit).  `last_per_image` keeps the per-image sums of squared differences (fp64,
    on the device) of the last call."""

    def __init__(self, size_average=None, reduce=None, reduction="mean", target_layout="nchw"):
        super().__init__()
        if size_average is not None or reduce is not None or reduction != "mean":
            raise NotImplementedError("MSELoss on the HIP path implements reduction='mean' "
                                      "(the reference setting)")
        if target_layout not in ("nchw", "nhwc_u8"):
            raise ValueError("target_layout must be 'nchw' or 'nhwc_u8'")
        self.reduction = reduction
        self.target_layout = target_layout
        self.last_per_image = None

    def forward(self, input, target):
        if not input.is_cuda:
            raise RuntimeError("unet-implementations_amd.MSELoss runs on MI355X only "
                               "(no CPU fallback exists)")
        if input.dim() != 4:
            raise ValueError("expected an NCHW output")
        u8 = self.target_layout == "nhwc_u8"
        if not u8 and target.dtype != torch.float32:
            target = target.float()
        return _MSEFunction.apply(input.contiguous().float(), target.contiguous(), self, u8)


class _SSIMFunction(torch.autograd.Function):
    """Forward: one fused pass for w_ssim * (1 - SSIM) + w_mse * MSE and the per-image SSIM and
    sums of squares (unet_ssim_fwd).  Backward: ONE launch of the gradient kernel with both weights
    and autograd's upstream (a scalar, or one value per image) applied inside it."""

    @staticmethod
    def forward(ctx, output, target, mod, target_u8, w_ssim, w_mse, per_image):
        loss, ssim, sq = ops.ssim_fwd(output, target, target_u8, w_ssim=w_ssim, w_mse=w_mse,
                                      want_loss=not per_image)
        mod.last_ssim_per_image = ssim      # fp64 [N] on the device (no sync)
        mod.last_per_image = sq
        if ctx.needs_input_grad[0]:
            ctx.held = (output, target, target_u8, w_ssim, w_mse, per_image)
        if per_image:
            return (1.0 - ssim).float()
        return loss[0].clone()

    @staticmethod
    def backward(ctx, g):
        output, target, target_u8, w_ssim, w_mse, per_image = ctx.held
        ctx.held = None
        d = ops.ssim_grad(output, target, g, per_image, target_u8, w_ssim=w_ssim, w_mse=w_mse)
        return d, None, None, None, None, None, None


def _check_input(name, input, target_layout):
    if not input.is_cuda:
        raise RuntimeError(f"unet-implementations_amd.{name} runs on MI355X only "
                           "(no CPU fallback exists)")
    if input.dim() != 4:
        raise ValueError("expected an NCHW output")
    return input.contiguous().float()


class SSIMLoss(nn.Module):
    """`SSIMLoss` (AE_pretrained/reconstruction/models/losses.py:178-245) on the HIP path:
    1 - SSIM with the 11-tap Gaussian window (sigma 1.5), C1 = 0.01^2, C2 = 0.03^2, zero padding.
    `size_average=True` returns a 0-dim fp32 tensor (1 - the mean SSIM over N*C*H*W);
    `size_average=False` one value per image [N].  The reference's constructor raises (its window
    builder calls torch.exp on a Python float); this implements the window it evidently intends,
    which equals utils/metrics.py's gaussian_kernel(11, 1.5).  `target_layout` as `MSELoss`.
    `last_ssim_per_image` / `last_per_image` keep the per-image SSIM and sums of squared
    differences (fp64, on the device) of the last call."""

    def __init__(self, window_size=11, size_average=True, target_layout="nchw"):
        super().__init__()
        if window_size != 11:
            raise NotImplementedError("the HIP SSIM kernels implement window_size=11")
        if target_layout not in ("nchw", "nhwc_u8"):
            raise ValueError("target_layout must be 'nchw' or 'nhwc_u8'")
        self.window_size = window_size
        self.size_average = size_average
        self.channel = 3
        self.target_layout = target_layout
        self.last_ssim_per_image = None
        self.last_per_image = None

    def forward(self, output, target):
        output = _check_input("SSIMLoss", output, self.target_layout)
        u8 = self.target_layout == "nhwc_u8"
        if not u8 and target.dtype != torch.float32:
            target = target.float()
        return _SSIMFunction.apply(output, target.contiguous(), self, u8, 1.0, 0.0,
                                   not self.size_average)


class ReconstructionLoss(nn.Module):
    """`ReconstructionLoss` (AE_pretrained/reconstruction/models/losses.py:12-79) on the HIP path:
    mse_weight * MSE + ssim_weight * (1 - SSIM), a 0-dim fp32 tensor.  With ssim_weight > 0 the
    loss is one fused forward (two launches) and one gradient launch; with ssim_weight == 0 it runs
    exactly `MSELoss`'s launches (the same bits).  The perceptual term needs VGG16 weights and is
    not implemented.  `target_layout` as `MSELoss`; `last_per_image` keeps the per-image sums of
    squared differences (fp64, on the device) of the last call."""

    def __init__(self, mse_weight=1.0, perceptual_weight=0.0, ssim_weight=0.0,
                 perceptual_layers=None, target_layout="nchw"):
        super().__init__()
        if perceptual_weight > 0:
            raise NotImplementedError("the perceptual (VGG16) term is not part of the HIP path")
        self.mse_weight = mse_weight
        self.perceptual_weight = perceptual_weight
        self.ssim_weight = ssim_weight
        self.target_layout = target_layout
        self.mse_loss = MSELoss(target_layout=target_layout)
        self.perceptual_loss = None
        self.ssim_loss = SSIMLoss(target_layout=target_layout) if ssim_weight > 0 else None
        self.last_per_image = None

    def forward(self, output, target):
        if self.ssim_loss is None:
            mse = self.mse_loss(output, target)
            self.last_per_image = self.mse_loss.last_per_image
            return mse if self.mse_weight == 1.0 else self.mse_weight * mse
        output = _check_input("ReconstructionLoss", output, self.target_layout)
        u8 = self.target_layout == "nhwc_u8"
        if not u8 and target.dtype != torch.float32:
            target = target.float()
        loss = _SSIMFunction.apply(output, target.contiguous(), self.ssim_loss, u8,
                                   float(self.ssim_weight), float(self.mse_weight), False)
        self.last_per_image = self.ssim_loss.last_per_image
        return loss
