"""unet-implementations_amd — the Our_UNet train step of Ulixes-8/UNet-Implementations
as hand-written gfx950 (MI355X) HIP kernels behind a C ABI, with the reference's
`UNet` / `SimpleLoss` / SGD module surface as the drop-in boundary.

The directory name contains a hyphen, so import it through the shim at the repo
root: `import unet_implementations_amd as ua`.
"""
from . import _lib, ops  # noqa: F401
from ._lib import LIB_PATH, UNetHipError, build, lib  # noqa: F401
from .losses import MSELoss, PerceptualLoss, ReconstructionLoss, SimpleLoss, SSIMLoss  # noqa: F401
from .metrics import (SegmentationMetrics, calculate_psnr, calculate_ssim,  # noqa: F401
                      compute_dice, compute_iou, compute_pixel_accuracy, evaluate_model_metrics,
                      evaluate_reconstructions)
from .optim import FusedAdam, FusedSGD  # noqa: F401
from .train import (create_lr_scheduler, create_model, create_optimizer,  # noqa: F401
                    get_loss_function, load_checkpoint, save_checkpoint, train_one_epoch,
                    train_step, validate, predict_masks, GraphedTrainStep)
from .clip_unet import CLIPUNet  # noqa: F401
from .clip_vit import ClipPatchExtractor, ClipVisionTransformer  # noqa: F401
from . import clip  # noqa: F401
from .unet import ConvBlock, SpatialDropout2d, UNet, UpBlock  # noqa: F401
from .autoencoder import Autoencoder  # noqa: F401
from . import ae  # noqa: F401
from . import evaluate  # noqa: F401
from . import render  # noqa: F401
from . import postprocess  # noqa: F401
from .postprocess import MaskCleanup  # noqa: F401
from . import latent  # noqa: F401
from . import augment  # noqa: F401
from . import dataprep  # noqa: F401
from .augment import AugmentConfig, BatchAugment  # noqa: F401
from .evaluate import generate_gradcam_heatmap, gradcam, gradcam_batch  # noqa: F401

__all__ = ["UNet", "Autoencoder", "CLIPUNet", "ClipPatchExtractor", "ClipVisionTransformer", "clip", "ConvBlock", "UpBlock", "SpatialDropout2d", "SimpleLoss", "MSELoss", "SSIMLoss", "PerceptualLoss", "ReconstructionLoss", "calculate_psnr", "calculate_ssim", "evaluate_reconstructions", "SegmentationMetrics", "compute_dice", "compute_iou", "compute_pixel_accuracy", "evaluate_model_metrics", "evaluate", "render", "postprocess", "MaskCleanup", "latent", "gradcam", "gradcam_batch", "generate_gradcam_heatmap", "FusedSGD", "FusedAdam", "ae", "augment", "dataprep", "AugmentConfig", "BatchAugment",
           "create_model", "create_optimizer", "create_lr_scheduler", "get_loss_function",
           "train_step", "GraphedTrainStep", "train_one_epoch", "save_checkpoint", "load_checkpoint", "validate", "predict_masks", "ops", "build", "lib", "UNetHipError", "LIB_PATH"]
