"""The pictures of the reference's evaluation on the HIP path (`ua.render`).

The reference draws four figures per batch with matplotlib (Our_UNet/utils/visualize.py:
visualize_prediction_batch, visualize_confidence_maps_batch, visualize_error_analysis_batch,
visualize_gradcam) and saves a comparison picture per test image with cv2
(AE_pretrained/reconstruction/utils/visualize.py: create_comparison_image).  Here the tiles of
those figures are rendered on the device by `unet_render_seg_panels` /
`unet_render_recon_panels` - one launch per figure from the image, the logits, the mask and the
heat map as they lie in device memory - and only the finished uint8 picture crosses to the host,
in `write_png`.  Titles, legends and colour bars are not drawn; DESIGN.md section 9b defines every
byte and lists what differs from the reference's files.

No matplotlib, cv2 or PIL at run time: the jet table is computed from its breakpoints and the PNG
encoder needs only zlib and struct.
"""
import struct
import zlib

import numpy as np
import torch

from . import ops
from .evaluate import _eval_logits, gradcam_batch

# the piecewise-linear "jet" of matplotlib (its segment data), per channel (x, value)
_JET = {
    "red": ((0.0, 0.0), (0.35, 0.0), (0.66, 1.0), (0.89, 1.0), (1.0, 0.5)),
    "green": ((0.0, 0.0), (0.125, 0.0), (0.375, 1.0), (0.64, 1.0), (0.91, 0.0), (1.0, 0.0)),
    "blue": ((0.0, 0.5), (0.11, 1.0), (0.34, 1.0), (0.65, 0.0), (1.0, 0.0)),
}
# the two ends of matplotlib's "Reds" (the ground-truth overlay of visualize_gradcam)
REDS_LOW, REDS_HIGH = (255, 245, 240), (103, 0, 12)


def jet_lut():
    """uint8 [256, 3] (numpy): matplotlib's 256-entry jet table as bytes, trunc(255 f) with f the
    piecewise-linear map interpolated at linspace(0, 1, 256).  A value v in [0, 1] shows entry
    min(int(v * 256), 255)."""
    x = np.linspace(0.0, 1.0, 256)
    lut = np.empty((256, 3), dtype=np.uint8)
    for c, name in enumerate(("red", "green", "blue")):
        pts = np.array(_JET[name], dtype=np.float64)
        lut[:, c] = (np.interp(x, pts[:, 0], pts[:, 1]) * 255).astype(np.uint8)
    return lut


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + \
        struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)


def png_bytes(hwc_uint8):
    """The PNG file (8-bit RGB, no interlace, filter 0 on every row) of a uint8 [H, W, 3] array."""
    a = np.ascontiguousarray(hwc_uint8)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise TypeError("write_png takes a uint8 [H, W, 3] picture")
    H, W, _ = a.shape
    rows = np.zeros((H, 1 + 3 * W), dtype=np.uint8)      # a filter-type byte in front of each row
    rows[:, 1:] = a.reshape(H, 3 * W)
    return b"".join((b"\x89PNG\r\n\x1a\n",
                     _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)),
                     _chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)),
                     _chunk(b"IEND", b"")))


def write_png(path, hwc_uint8):
    """Write a uint8 [H, W, 3] picture - a device or host tensor, or a numpy array - as a PNG.
    This is the one place the rendered bytes cross to the host."""
    if torch.is_tensor(hwc_uint8):
        hwc_uint8 = hwc_uint8.detach().cpu().numpy()
    data = png_bytes(hwc_uint8)
    with open(path, "wb") as f:
        f.write(data)


def _batch_operands(batch, device):
    images = batch["image"].to(device, non_blocking=True)
    masks = batch["mask"].to(device, non_blocking=True)
    if masks.dtype not in (torch.int64, torch.uint8):
        masks = masks.long()
    return images, masks


def _logits(model, images):
    """Eval-mode logits of a loader batch: normalised fp32 [B,3,H,W] or the uint8 [B,H,W,3]
    batch of the "nhwc_u8" input layout."""
    K = getattr(model, "num_classes", 3)
    if K != 3:      # (before the forward: nothing is launched for a figure that cannot be drawn)
        raise NotImplementedError("the rendered figures use the three-colour palette of the pet "
                                  f"trimap (got {K} classes)")
    if images.dtype != torch.uint8:
        return _eval_logits(model, images)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            return model(images, input_layout="nhwc_u8").float()
    finally:
        model.train(was_training)


def figure(images, logits, masks, panels, heat=None, target_class=1):
    """uint8 [B * H, P * W, 3] on the device: one row of `panels` per image of the batch."""
    if logits is not None and logits.dim() == 4 and logits.shape[1] != 3:
        raise NotImplementedError("the rendered figures use the three-colour palette of the pet "
                                  f"trimap (got {logits.shape[1]} classes)")
    out = ops.render_seg_panels(images, logits, masks, heat, panels, target_class)
    B, H, P, W, _ = out.shape
    return out.view(B * H, P * W, 3)


PREDICTION_PANELS = ("image", "gt", "pred")
CONFIDENCE_PANELS = ("image", "conf0", "conf1", "conf2")
ERROR_PANELS = ("image", "gt", "pred", "error")
GRADCAM_PANELS = ("image", "target", "heat")


def prediction_figure(model, batch, device):
    """image | ground truth | prediction (visualize_prediction_batch, utils/visualize.py:27-93)."""
    images, masks = _batch_operands(batch, device)
    return figure(images, _logits(model, images), masks, PREDICTION_PANELS)


def confidence_figure(model, batch, device):
    """image | confidence overlay of background, cat, dog (visualize_confidence_maps_batch,
    utils/visualize.py:96-175)."""
    images = batch["image"].to(device, non_blocking=True)
    return figure(images, _logits(model, images), None, CONFIDENCE_PANELS)


def error_figure(model, batch, device):
    """image | ground truth | prediction | error analysis (visualize_error_analysis_batch,
    utils/visualize.py:241-324)."""
    images, masks = _batch_operands(batch, device)
    return figure(images, _logits(model, images), masks, ERROR_PANELS)


def gradcam_figure(model, batch, device, target_class=1, target_layer=None):
    """image | ground truth of `target_class` | Grad-CAM overlay (visualize_gradcam,
    utils/visualize.py:442-516), for the images whose mask contains the class - the reference
    skips the others (:475), so their rows are absent.  Selecting the rows reads `present` on the
    host: the height of the result depends on it."""
    images, masks = _batch_operands(batch, device)
    heat, present = gradcam_batch(model, batch, device, target_class, target_layer)
    out = ops.render_seg_panels(images, None, masks, heat, GRADCAM_PANELS, target_class)
    out = out[present]
    B, H, P, W, _ = out.shape
    return out.reshape(B * H, P * W, 3)
