"""Test-set evaluation of Our_UNet/src/evaluate.py on the HIP path.

`evaluate_model` is the loop behind every number in the reference's
`evaluation_results.json` (src/evaluate.py:150-268): eval-mode forward, argmax, nearest resize of
the class map and of the mask to each image's `original_dims`, and the accumulators of
`SegmentationMetrics`.  The reference does the resizes with two `F.interpolate` calls per image,
copies both maps to the host and counts in numpy; here `unet_eval_confusion` does the whole tail of
a batch in one launch and the loop has no host sync until the results are read.

`confidence_maps` / `error_maps` return what `visualize_confidence_maps_batch` and
`create_error_visualization` (utils/visualize.py:96-238) compute before they plot, as device
tensors (`unet_eval_maps`).  Plotting itself (matplotlib) is not part of this package.
"""
import numpy as np
import torch

from . import ops
from .metrics import accumulate_test_metrics
from .train import create_model


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


def evaluate_model(model, test_loader, device, visualize_samples=0):
    """The dictionary of src/evaluate.py:239-268 (pixel accuracy, mean IoU, per-class dice / iou /
    precision / recall, `mean_foreground_dice`), every image counted at its original size, plus
    `"confusion_matrix"`: int64 [3, 3] numpy, target class x predicted class, what the reference's
    plot_confusion_matrix counts from the resized maps it keeps.  The reference's plots need
    matplotlib: `visualize_samples > 0` is not supported (see confidence_maps / error_maps)."""
    if visualize_samples > 0:
        raise NotImplementedError("plots are not part of the HIP path (use visualize_samples=0; "
                                  "confidence_maps / error_maps return the plotted tensors)")
    metrics = accumulate_test_metrics(model, test_loader, device)
    results = {"pixel_accuracy": metrics.compute_pixel_accuracy(),
               "mean_iou": metrics.compute_mean_iou()}
    for cls, name in enumerate(("background", "cat", "dog")):
        results[name] = {"dice": metrics.compute_dice(cls), "iou": metrics.compute_iou(cls),
                         "precision": metrics.compute_precision(cls),
                         "recall": metrics.compute_recall(cls)}
    fg = [d for d in (results["cat"]["dice"], results["dog"]["dice"]) if not np.isnan(d)]
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


def confidence_maps(model, images):
    """Softmax probabilities fp32 [B, 3, H, W] on the device (utils/visualize.py:117-119)."""
    return ops.eval_maps(_eval_logits(model, images), want_classes=False)[0]


def error_maps(model, images, masks):
    """uint8 [B, H, W] on the device: the category create_error_visualization colours
    (utils/visualize.py:205-222) - 0 none, 1 true positive (green), 2 false positive (red),
    3 false negative (blue), 4 wrong class (yellow); 255 in the mask counts as background."""
    if masks.dtype != torch.int64:
        masks = masks.long()
    return ops.eval_maps(_eval_logits(model, images), masks, want_probs=False,
                         want_classes=False)[2]
