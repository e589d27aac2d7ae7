"""Drop-in `SegmentationMetrics` (reference: Our_UNet/utils/metrics.py:7-235).

Same accumulators (`intersections`, `unions`, `true_positives`, `false_positives`,
`false_negatives`, `total_pixels`, `correct_pixels`) and `compute_*` methods as the reference
class, for the 3-class pet masks.  The reference moves every prediction / target to the host
and loops over classes in numpy (`_update_single`, :59-91); here one launch of
`unet_argmax_dice_counts` produces the nine integer counts per batch
{intersection, predicted, labelled} x class (ignore pixels masked out) and they are summed in
an int64 device tensor - no host sync until a `compute_*` method (or an accumulator) is read.

The reconstruction metrics of AE_pretrained/reconstruction/utils/metrics.py (`calculate_psnr`,
`calculate_ssim`, `evaluate_reconstructions`) keep the reference's signatures and return shapes;
each is one fused forward (`unet_ssim_fwd`, or `unet_mse_loss_fwd` for PSNR alone).

`update_from_logits(logits, target)` takes the network output itself (argmax inside the
kernel); with `original_dims` it counts at every image's original size, as the reference's
test-set evaluation does, through `unet_eval_confusion` (argmax, both nearest resizes and the
3 x 3 confusion matrix in one launch), and `confusion_matrix` holds the accumulated matrix; `update(pred, target)` takes class maps like the reference's method (device tensors;
routed through the same kernel as one-hot scores).  Targets hold {0, 1, 2, ignore_index}
(Our_UNet/src/train.py:300: everything else was mapped to 0 by the dataset).
"""
import numpy as np
import torch

from . import ops


class SegmentationMetrics:
    def __init__(self, num_classes: int = 3, ignore_index: int = 255):
        if not 2 <= num_classes <= ops.MAX_CLASSES:
            raise NotImplementedError(f"the HIP count kernels handle 2 to {ops.MAX_CLASSES} "
                                      f"classes (got {num_classes})")
        self.num_classes = num_classes
        self.ignore_index = ignore_index
        self._counts = None      # int64 [K, 3] on the device: {inter, predicted, labelled} per class
        self._cm = None          # int64 [K, K]: target class x predicted class (original-size path)
        self._cm_complete = True  # False once an update arrived without its confusion matrix
        self.reset()

    # reference: utils/metrics.py:25-34
    def reset(self):
        if self._counts is not None:
            self._counts.zero_()
        if self._cm is not None:
            self._cm.zero_()
        self._cm_complete = True

    def _add(self, counts):
        if self._counts is None:
            self._counts = counts.clone()
        else:
            if self._counts.device != counts.device:
                self._counts = self._counts.to(counts.device)
            self._counts += counts

    def update_from_confusion(self, cm):
        """Adds confusion matrices [K, K] or [B, K, K] (integers, target class x predicted class;
        tensor on any device, or array): what `update_from_logits(..., original_dims)` does with
        the output of `unet_eval_confusion`.  Intersections are the diagonal, predicted pixels the
        column sums, labelled pixels the row sums; no host sync."""
        cm = torch.as_tensor(cm)
        if cm.dtype != torch.int64:
            cm = cm.to(torch.int64)
        cm = cm.reshape(-1, self.num_classes, self.num_classes).sum(dim=0)
        if self._cm is None:
            self._cm = cm.clone()
        else:
            if self._cm.device != cm.device:
                self._cm = self._cm.to(cm.device)
            self._cm += cm
        self._add(torch.stack([torch.diagonal(cm), cm.sum(dim=0), cm.sum(dim=1)], dim=1))

    def update_from_logits(self, logits, target, original_dims=None):
        """logits fp32 [B, K, H, W], target int64 [B, H, W], both on the device.
        original_dims (int64 [B, 2] of (orig_h, orig_w), as the default collate builds it from the
        dataset's `original_dims`; a host tensor is copied over): count at each image's original
        size, both maps nearest-resized as evaluate_model does (src/evaluate.py:189-211)."""
        if not logits.is_cuda:
            raise RuntimeError("unet-implementations_amd.SegmentationMetrics runs on MI355X only "
                               "(no CPU fallback exists)")
        if logits.dim() != 4 or logits.shape[1] != self.num_classes:
            raise ValueError(f"logits [B, {self.num_classes}, H, W] expected (got "
                             f"{tuple(logits.shape)})")
        if target.dtype != torch.int64:
            target = target.long()
        if original_dims is not None:
            dims = torch.as_tensor(original_dims).to(device=logits.device, dtype=torch.int64,
                                                     non_blocking=True)
            self.update_from_confusion(ops.eval_confusion(logits.float(), target, dims,
                                                          self.ignore_index))
            return
        _, counts = ops.argmax_dice_counts(logits.float(), target, self.ignore_index,
                                           want_preds=False)
        self._cm_complete = False
        self._add(counts)

    def update_from_classes(self, preds_u8, target, original_dims=None):
        """preds_u8 uint8 [B, H, W] (a class map: `ops.argmax_classes`, or a `MaskCleanup` of it),
        target int64 [B, H, W], both on the device: counted through `unet_eval_confusion_classes`,
        at each image's original size with original_dims ([B, 2] of (orig_h, orig_w)), at network
        size without.  Always carries a confusion matrix."""
        if not torch.is_tensor(preds_u8) or preds_u8.dtype != torch.uint8:
            raise TypeError("update_from_classes takes a uint8 class map [B, H, W]")
        if not preds_u8.is_cuda:
            raise RuntimeError("unet-implementations_amd.SegmentationMetrics runs on MI355X only "
                               "(no CPU fallback exists)")
        if target.dtype != torch.int64:
            target = target.long()
        dims = None
        if original_dims is not None:
            dims = torch.as_tensor(original_dims).to(device=preds_u8.device, dtype=torch.int64,
                                                     non_blocking=True)
        self.update_from_confusion(ops.eval_confusion_classes(
            preds_u8, target, dims, self.num_classes, self.ignore_index))

    @property
    def confusion_matrix(self):
        """int64 [K, K] (numpy), target class x predicted class, accumulated by the updates that
        carried one (`update_from_logits` with `original_dims`, `update_from_confusion`)."""
        if not self._cm_complete:
            raise RuntimeError("confusion_matrix: some updates came without original_dims (the "
                               "network-size kernel counts per class only)")
        if self._cm is None:
            return np.zeros((self.num_classes, self.num_classes), dtype=np.int64)
        return self._cm.cpu().numpy()

    # reference: utils/metrics.py:36-57
    def update(self, pred, target):
        """pred / target: class maps [H, W] or [B, H, W] (torch tensors on the device)."""
        if not torch.is_tensor(pred) or not torch.is_tensor(target) or not pred.is_cuda:
            raise RuntimeError("unet-implementations_amd.SegmentationMetrics takes device tensors "
                               "(no CPU fallback exists)")
        if pred.dim() == 2:
            pred, target = pred[None], target[None]
        p = pred.long()
        scores = torch.stack([(p == c).float() for c in range(self.num_classes)], dim=1)
        self.update_from_logits(scores.contiguous(), target)

    # ---- accumulators with the reference's names (float64 numpy arrays / integers) -------------
    def _host(self):
        if self._counts is None:
            return np.zeros((self.num_classes, 3), dtype=np.int64)
        return self._counts.cpu().numpy()

    @property
    def intersections(self):
        return self._host()[:, 0].astype(np.float64)

    @property
    def unions(self):
        c = self._host()
        return (c[:, 1] + c[:, 2] - c[:, 0]).astype(np.float64)

    @property
    def true_positives(self):
        return self.intersections

    @property
    def false_positives(self):
        c = self._host()
        return (c[:, 1] - c[:, 0]).astype(np.float64)

    @property
    def false_negatives(self):
        c = self._host()
        return (c[:, 2] - c[:, 0]).astype(np.float64)

    @property
    def total_pixels(self):
        return int(self._host()[:, 2].sum())       # every valid pixel is labelled 0 .. K-1

    @property
    def correct_pixels(self):
        return int(self._host()[:, 0].sum())

    # ---- reference: utils/metrics.py:93-235 ----------------------------------------------------
    def compute_pixel_accuracy(self) -> float:
        total = self.total_pixels
        return float(self.correct_pixels / total) if total > 0 else float("nan")

    def compute_iou(self, cls: int) -> float:
        u = self.unions[cls]
        return float(self.intersections[cls] / u) if u > 0 else float("nan")

    def _mean_valid(self, fn):
        vals = [fn(c) for c in range(self.num_classes)]
        vals = [v for v in vals if not np.isnan(v)]
        return float(sum(vals) / len(vals)) if vals else float("nan")

    def compute_mean_iou(self) -> float:
        return self._mean_valid(self.compute_iou)

    def compute_dice(self, cls: int) -> float:
        tp, fp, fn = self.true_positives[cls], self.false_positives[cls], self.false_negatives[cls]
        den = 2 * tp + fp + fn
        return float(2 * tp / den) if den > 0 else float("nan")

    def compute_mean_dice(self) -> float:
        return self._mean_valid(self.compute_dice)

    def compute_precision(self, cls: int) -> float:
        tp, fp = self.true_positives[cls], self.false_positives[cls]
        return float(tp / (tp + fp)) if (tp + fp) > 0 else float("nan")

    def compute_recall(self, cls: int) -> float:
        tp, fn = self.true_positives[cls], self.false_negatives[cls]
        return float(tp / (tp + fn)) if (tp + fn) > 0 else float("nan")

    def compute_f1_score(self, cls: int) -> float:
        return self.compute_dice(cls)

    def get_all_metrics(self):
        results = {"pixel_accuracy": self.compute_pixel_accuracy(),
                   "mean_iou": self.compute_mean_iou(),
                   "mean_dice": self.compute_mean_dice(), "class_metrics": {}}
        for cls in range(self.num_classes):
            results["class_metrics"][f"class_{cls}"] = {
                "iou": self.compute_iou(cls), "dice": self.compute_dice(cls),
                "precision": self.compute_precision(cls), "recall": self.compute_recall(cls),
                "f1_score": self.compute_f1_score(cls)}
        return results


# ---- stand-alone forms (reference: utils/metrics.py:244-358) -------------------------------------
def _single(pred, target, ignore_index):
    metrics = SegmentationMetrics(num_classes=3, ignore_index=ignore_index)
    metrics.update(pred, target)
    return metrics


def compute_dice(pred, target, cls, ignore_index=255):
    """Dice of class `cls` for one prediction / target pair of class maps (device tensors)."""
    return _single(pred, target, ignore_index).compute_dice(cls)


def compute_iou(pred, target, cls, ignore_index=255):
    """IoU of class `cls` for one prediction / target pair of class maps (device tensors)."""
    return _single(pred, target, ignore_index).compute_iou(cls)


def compute_pixel_accuracy(pred, target, ignore_index=255):
    """Pixel accuracy of one prediction / target pair of class maps (device tensors)."""
    return _single(pred, target, ignore_index).compute_pixel_accuracy()


@torch.no_grad()
def accumulate_test_metrics(model, data_loader, device, ignore_index=255, on_batch=None,
                            num_classes=None, *, postprocess=None):
    """The loop of evaluate_model / evaluate_model_metrics: eval-mode forward, then one launch per
    batch for argmax, both nearest resizes to `original_dims` and all counting.  Nothing is read
    on the host until the returned SegmentationMetrics is asked for a value.
    on_batch(i, images, masks, logits), if given, sees every batch's device tensors after they
    were counted (evaluate_model renders its pictures from them: no second forward).
    postprocess: a `MaskCleanup`; each batch then runs forward, argmax, the cleanup at network
    size and the count of the cleaned map at the original sizes - still without a host read."""
    if num_classes is None:      # (the model's own count; the reference's loop is 3-class)
        num_classes = getattr(model, "num_classes", 3)
    if postprocess is not None:
        from .postprocess import _check_postprocess
        _check_postprocess(postprocess)
    model.eval()
    metrics = SegmentationMetrics(num_classes=num_classes, ignore_index=ignore_index)
    for i, batch in enumerate(data_loader):
        images = batch["image"].to(device, non_blocking=True)
        masks = batch["mask"].to(device, non_blocking=True)
        logits = model(images)
        if postprocess is None:
            metrics.update_from_logits(logits, masks, batch["original_dims"])
        else:
            preds = postprocess(ops.argmax_classes(logits.float()), num_classes)
            metrics.update_from_classes(preds, masks, batch["original_dims"])
        if on_batch is not None:
            on_batch(i, images, masks, logits)
    return metrics


def evaluate_model_metrics(model, data_loader, device, num_classes=3, ignore_index=255):
    """utils/metrics.py:305-358: `get_all_metrics()` over a dataset, every image counted at its
    original size."""
    if num_classes != 3:
        raise NotImplementedError("evaluate_model_metrics is the reference's 3-class helper; for "
                                  "K classes use SegmentationMetrics(num_classes=K) or "
                                  "evaluate.evaluate_model")
    return accumulate_test_metrics(model, data_loader, device, ignore_index).get_all_metrics()


# ---- reconstruction metrics (reference: AE_pretrained/reconstruction/utils/metrics.py) ----------
def _recon_operands(name, pred, target):
    if not torch.is_tensor(pred) or not pred.is_cuda:
        raise RuntimeError(f"unet-implementations_amd.{name} runs on MI355X only "
                           "(no CPU fallback exists)")
    if pred.dim() != 4:
        raise ValueError("expected NCHW predictions")
    pred = pred.contiguous().float()
    u8 = target.dtype == torch.uint8        # the dataset's [N,H,W,3] image itself
    if not u8 and target.dtype != torch.float32:
        target = target.float()
    return pred, target.contiguous(), u8


def _psnr(mse, max_val):
    return 10 * torch.log10(max_val ** 2 / torch.clamp(mse, min=1e-10))


def calculate_psnr(pred, target, max_val=1.0):
    """Per-image PSNR [B] (fp32) of (B, C, H, W) images (utils/metrics.py:15-41)."""
    pred, target, u8 = _recon_operands("calculate_psnr", pred, target)
    _, sq = ops.mse_loss_fwd(pred, target, u8)
    C, H, W = pred.shape[1:]
    return _psnr((sq / (C * H * W)).float(), max_val)


def _check_kernel(kernel_size):
    if kernel_size % 2 == 0:     # the reference's gaussian_kernel bumps an even size
        kernel_size += 1
    if kernel_size != 11:
        raise NotImplementedError("the HIP SSIM kernels implement an 11-tap window")


def _reduce(v, reduction):
    if reduction == "mean":
        return v.mean()
    if reduction == "sum":
        return v.sum()
    return v


def calculate_ssim(pred, target, kernel_size=11, sigma=1.5, max_val=1.0, reduction="none"):
    """SSIM per image [B] (fp32; or its mean / sum) with the Gaussian window of gaussian_kernel
    (kernel_size, sigma), zero padding, C1 = (0.01 max_val)^2, C2 = (0.03 max_val)^2
    (utils/metrics.py:76-147)."""
    _check_kernel(kernel_size)
    pred, target, u8 = _recon_operands("calculate_ssim", pred, target)
    _, ssim, _ = ops.ssim_fwd(pred, target, u8, window=ops.gaussian_window(11, float(sigma)),
                              c1=(0.01 * max_val) ** 2, c2=(0.03 * max_val) ** 2,
                              want_loss=False)
    return _reduce(ssim.float(), reduction)


def evaluate_reconstructions(pred, target):
    """{"psnr", "ssim", "mse"}, each per image [B] fp32, from one fused pass
    (utils/metrics.py:150-181)."""
    pred, target, u8 = _recon_operands("evaluate_reconstructions", pred, target)
    _, ssim, sq = ops.ssim_fwd(pred, target, u8, want_loss=False)
    C, H, W = pred.shape[1:]
    mse = (sq / (C * H * W)).float()
    return {"psnr": _psnr(mse, 1.0), "ssim": ssim.float(), "mse": mse}
