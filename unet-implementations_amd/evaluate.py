"""Test-set evaluation of Our_UNet/src/evaluate.py on the HIP path.

`evaluate_model` is the loop behind every number in the reference's
`evaluation_results.json` (src/evaluate.py:150-268): eval-mode forward, argmax, nearest resize of
the class map and of the mask to each image's `original_dims`, and the accumulators of
`SegmentationMetrics`.  The reference does the resizes with two `F.interpolate` calls per image,
copies both maps to the host and counts in numpy; here `unet_eval_confusion` does the whole tail of
a batch in one launch and the loop has no host sync until the results are read.

`confidence_maps` / `error_maps` return what `visualize_confidence_maps_batch` and
`create_error_visualization` (utils/visualize.py:96-238) compute before they plot, as device
tensors (`unet_eval_maps`).  `gradcam` / `gradcam_batch` / `generate_gradcam_heatmap` are the
tensors behind `visualize_gradcam` (utils/visualize.py:372-516): a gradient-only backward that
stops at the target stage and three small kernels (`unet_gradcam_*`), for a whole batch.
The pictures themselves - the tiles of those figures as uint8 RGB - are `ua.render`
(`unet_render_seg_panels`); matplotlib is not part of this package.
"""
import os

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .metrics import accumulate_test_metrics
from .train import class_names, create_model
from .unet import stage_feature_and_gradient


def load_model(model_path, device):
    """src/evaluate.py:103-147: the training configuration, weights from a checkpoint dictionary
    (`model_state_dict`) or a bare state dict, eval mode."""
    model = create_model(device)
    checkpoint = torch.load(model_path, map_location=device, weights_only=True)
    if "model_state_dict" in checkpoint:
        checkpoint = checkpoint["model_state_dict"]
    model.load_state_dict(checkpoint)
    model.eval()
    return model


def evaluate_model(model, test_loader, device, visualize_samples=0, output_dir=None, *,
                   postprocess=None):
    """The dictionary of src/evaluate.py:239-268 (pixel accuracy, mean IoU, per-class dice / iou /
    precision / recall, `mean_foreground_dice`), every image counted at its original size, plus
    `"confusion_matrix"`: int64 [K, K] numpy (K = model.num_classes, 2..32; the per-class entries
    are named class_0 .. class_{K-1} unless K == 3), target class x predicted class, what the reference's
    plot_confusion_matrix counts from the resized maps it keeps.

    With `visualize_samples > 0` and an `output_dir`, the first `visualize_samples` batches each
    leave `predictions_batch{i}.png`, `confidence_batch{i}.png` and `errors_batch{i}.png` there:
    the tiles of the three figures the reference shows per sample batch (src/evaluate.py:214-223),
    one row per image, rendered on the device from the logits of the metrics pass (`ua.render`,
    DESIGN.md section 9b) - the returned numbers are those of a `visualize_samples=0` run.
    Nothing is shown on a screen, so without an `output_dir` there is nowhere to put a picture and
    `visualize_samples > 0` raises.

    postprocess: a `ua.MaskCleanup` (for this dataset `MaskCleanup.pet()`); every batch's argmax
    map is cleaned on the device at network size before it is counted at the original sizes.  The
    pictures are drawn from the logits, so `postprocess` with `visualize_samples > 0` raises."""
    K = getattr(model, "num_classes", 3)
    if postprocess is not None and visualize_samples > 0:
        raise ValueError("the pictures are drawn from the logits, not from the cleaned maps: use "
                         "postprocess with visualize_samples=0 (rendering cleaned maps is not "
                         "covered)")
    if visualize_samples > 0 and K != 3:
        raise NotImplementedError("the rendered figures use the three-colour palette of the pet "
                                  f"trimap (got {K} classes): use visualize_samples=0")
    if visualize_samples > 0 and output_dir is None:
        raise NotImplementedError("plots are not part of the HIP path (use visualize_samples=0; "
                                  "confidence_maps / error_maps / gradcam return the plotted "
                                  "tensors)")
    on_batch = None
    if visualize_samples > 0:
        from . import render
        os.makedirs(str(output_dir), exist_ok=True)

        def on_batch(i, images, masks, logits):
            if i >= visualize_samples:
                return
            if masks.dtype not in (torch.int64, torch.uint8):
                masks = masks.long()
            logits = logits.detach().float()
            for stem, panels in (("predictions", render.PREDICTION_PANELS),
                                 ("confidence", render.CONFIDENCE_PANELS),
                                 ("errors", render.ERROR_PANELS)):
                render.write_png(os.path.join(str(output_dir), f"{stem}_batch{i}.png"),
                                 render.figure(images, logits, masks, panels))
    if postprocess is None:
        metrics = accumulate_test_metrics(model, test_loader, device, on_batch=on_batch)
    else:
        metrics = accumulate_test_metrics(model, test_loader, device, postprocess=postprocess)
    results = {"pixel_accuracy": metrics.compute_pixel_accuracy(),
               "mean_iou": metrics.compute_mean_iou()}
    names = class_names(K)
    for cls, name in enumerate(names):
        results[name] = {"dice": metrics.compute_dice(cls), "iou": metrics.compute_iou(cls),
                         "precision": metrics.compute_precision(cls),
                         "recall": metrics.compute_recall(cls)}
    fg = [d for d in (results[name]["dice"] for name in names[1:]) if not np.isnan(d)]
    results["mean_foreground_dice"] = float(np.mean(fg)) if fg else float("nan")
    results["confusion_matrix"] = metrics.confusion_matrix
    return results


@torch.no_grad()
def _eval_logits(model, images):
    was_training = model.training
    model.eval()
    try:
        return model(images).float()
    finally:
        model.train(was_training)


def _three_classes_only(model, what):
    """The visual helpers are the pet trimap's: refused for another class count before the
    device is touched."""
    K = getattr(model, "num_classes", 3)
    if K != 3:
        raise NotImplementedError(f"{what} covers the 3-class model (three-colour maps of the pet "
                                  f"trimap); got {K} classes")


def confidence_maps(model, images):
    """Softmax probabilities fp32 [B, 3, H, W] on the device (utils/visualize.py:117-119)."""
    _three_classes_only(model, "confidence_maps")
    return ops.eval_maps(_eval_logits(model, images), want_classes=False)[0]


def error_maps(model, images, masks):
    """uint8 [B, H, W] on the device: the category create_error_visualization colours
    (utils/visualize.py:205-222) - 0 none, 1 true positive (green), 2 false positive (red),
    3 false negative (blue), 4 wrong class (yellow); 255 in the mask counts as background."""
    _three_classes_only(model, "error_maps")
    if masks.dtype != torch.int64:
        masks = masks.long()
    return ops.eval_maps(_eval_logits(model, images), masks, want_probs=False,
                         want_classes=False)[2]


def _gradcam_target(model, target_layer):
    """The stage module whose output the walk holds for `target_layer`, or ValueError."""
    if target_layer is None:
        return model.decoder_stages[0]
    for stage in model.encoder_stages:
        if target_layer is stage:
            return stage
    for stage in model.decoder_stages:
        if target_layer is stage or target_layer is stage.conv_block:
            return stage
    name = next((n for n, m in model.named_modules() if m is target_layer), None)
    if name is None:
        raise ValueError("target_layer is not a module of this model")
    msg = (f"target_layer {name} ({type(target_layer).__name__}) is an inner module: the fused "
           "HIP walk never holds that tensor (a layer exists in memory only as its raw "
           "convolution output plus InstanceNorm coefficients).  Use encoder_stages[i], "
           "decoder_stages[i] or decoder_stages[i].conv_block; target_layer=None is "
           "decoder_stages[0].")
    if isinstance(target_layer, nn.Conv2d) and target_layer is not model.segmentation_output:
        msg += ("  For this convolution the request is also empty: its output feeds an "
                "InstanceNorm, the gradient with respect to an InstanceNorm input sums to zero "
                "over every (image, channel) plane, so the Grad-CAM channel weights - that "
                "spatial mean - are identically zero in exact arithmetic and the reference's "
                "picture for this target is rounding noise.")
    raise ValueError(msg)


def gradcam(model, images, target_class, target_layer=None, precision="fp32"):
    """Grad-CAM heatmaps of a whole batch: fp32 [B, H, W] on the device, no host sync - per image
    what the reference's generate_gradcam_heatmap (utils/visualize.py:372-439) returns for
    images[b:b+1].

    target_layer: encoder_stages[i], decoder_stages[i] or decoder_stages[i].conv_block (the same
    tensor as its stage); None = decoder_stages[0], the "first decoder stage" of the reference's
    docstring.  (The reference's code default, the inner Conv2d decoder_stages[0].conv_block.
    block[0], raises ValueError like every inner module: see the message.)
    precision: "fp32" (default) runs this pass in the fp32 operand mode whatever
    model.matmul_precision is (the master weights are fp32); None runs it in the model's own mode,
    bf16 layer tensors included.  Grad-CAM through many InstanceNorms is ill-conditioned for deep
    targets: no accuracy is claimed for the bf16 mode.

    Unlike the reference (model.zero_grad() + a full backward per image) this leaves every .grad,
    the gradient arena, model.training and dropout_mask_override as they were."""
    if precision not in (None, "fp32"):
        raise ValueError("precision must be 'fp32' or None (the model's own mode)")
    _three_classes_only(model, "Grad-CAM")
    target = _gradcam_target(model, target_layer)
    K = model.segmentation_output.out_channels
    if not 0 <= int(target_class) < K:
        raise ValueError(f"target_class {target_class} is outside [0, {K})")
    if not torch.is_tensor(images) or not images.is_cuda:
        raise RuntimeError("unet-implementations_amd.evaluate.gradcam runs on MI355X only "
                           "(no CPU fallback exists)")
    mode = model.matmul_precision
    if precision is not None:
        model.matmul_precision = precision
    try:
        feature, grad, slope = stage_feature_and_gradient(model, images, target_class, target)
    finally:
        model.matmul_precision = mode
    N, h, w, C = grad.shape
    ws = ops.gradcam_workspace(N, h * w, C, grad)
    weights = ops.gradcam_weights(grad, ws)
    cam, ws = ops.gradcam_map(feature, slope, weights, ws)
    return ops.gradcam_heatmap(cam, ws, images.shape[2:])


def generate_gradcam_heatmap(model, input_tensor, target_class, target_layer, device):
    """The reference's helper with its signature (utils/visualize.py:372-439): the squeezed numpy
    heatmap of `input_tensor` ([1, C, H, W] -> [H, W]), so its visualize_gradcam can import this
    one instead.  One device-to-host copy, at the end."""
    heat = gradcam(model, input_tensor.to(device), target_class, target_layer)
    return heat.squeeze().cpu().numpy()


def gradcam_batch(model, batch, device, target_class=1, target_layer=None):
    """(heatmaps fp32 [B, H, W], present bool [B]) on the device for a loader batch: what
    visualize_gradcam (utils/visualize.py:442-516) computes before it plots.  present[b] says
    whether batch["mask"][b] contains target_class - the images the reference's np.unique test
    (:474-476) does not skip."""
    images, masks = batch["image"].to(device), batch["mask"].to(device)
    present = (masks == target_class).flatten(1).any(dim=1)
    return gradcam(model, images, target_class, target_layer), present
