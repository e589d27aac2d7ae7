"""The train and validation loops of the CLIP_UNet sub-project (CLIP_UNet/src/train.py:592-768)
on the HIP path: the loops of `train.py` with the reference's `clip_extractor` argument.

Every step first runs the frozen CLIP tower on `batch["clip_image"]` (:714-719, :619-623) and
hands the [N, E, 16, 16] features to `CLIPUNet.forward(x, clip_features)`; without an extractor
`clip_features=None` goes through, as in the reference.  With uint8 batches
(`input_layout="nhwc_u8"`) and no `clip_image` entry the extractor reads the training image
itself: its patch gather resizes any size to the tower's resolution.  The loss stays a device
scalar (no per-step host sync).
"""
import torch

from . import ops
from .train import dice_scores


def extract_clip_features(clip_extractor, batch, images, device, input_layout=None):
    """`clip_extractor(batch["clip_image"])`, or None without an extractor."""
    if clip_extractor is None:
        return None
    clip_images = batch.get("clip_image") if hasattr(batch, "get") else None
    if clip_images is None:
        if input_layout != "nhwc_u8":
            raise KeyError('the batch has no "clip_image" entry (only uint8 "nhwc_u8" batches may '
                           "feed the training image itself to the extractor)")
        clip_images = images
    else:
        clip_images = clip_images.to(device, non_blocking=True)
    layout = "nhwc_u8" if clip_images.dtype == torch.uint8 else "nchw"
    return clip_extractor(clip_images, input_layout=layout)


def _forward(model, images, clip_features, input_layout):
    if input_layout is None:
        return model(images, clip_features)
    return model(images, clip_features, input_layout=input_layout)


def train_step(model, optimizer, loss_function, images, masks, clip_extractor=None,
               clip_images=None, grad_sync=None, input_layout=None):
    """One optimisation step of CLIP_UNet (:714-753); returns the loss as a 0-dim device tensor.
    `clip_images` is the batch's "clip_image" entry (None with "nhwc_u8": the image itself)."""
    batch = {} if clip_images is None else {"clip_image": clip_images}
    clip_features = extract_clip_features(clip_extractor, batch, images, images.device,
                                          input_layout)
    optimizer.zero_grad()
    outputs = _forward(model, images, clip_features, input_layout)
    loss = loss_function(outputs, masks)
    loss.backward()
    if grad_sync is not None:
        grad_sync()
    optimizer.step()
    return loss.detach()


def train_one_epoch(model, train_loader, optimizer, loss_function, device, clip_extractor=None,
                    input_layout=None):
    """Counterpart of train_one_epoch (:671-768): the average training loss of the epoch, read
    back once at its end."""
    model.train()
    total = torch.zeros((), device=device)
    n = 0
    for batch in train_loader:
        images = batch["image"].to(device, non_blocking=True)
        masks = batch["mask"].to(device, non_blocking=True)
        total += train_step(model, optimizer, loss_function, images, masks,
                            clip_extractor=clip_extractor, clip_images=batch.get("clip_image"),
                            input_layout=input_layout)
        n += 1
    return (total / max(n, 1)).item()


@torch.no_grad()
def validate(model, val_loader, loss_function, device, clip_extractor=None, ignore_label=255,
             input_layout=None):
    """Counterpart of validate (:592-668): eval-mode forward with the CLIP features, loss, and the
    per-batch Dice of the argmax predictions, averaged over batches; counts and Dice arithmetic
    stay on the device as in `train.validate`."""
    model.eval()
    val_loss = torch.zeros((), device=device)
    dice_sum = None      # float64 [K], sized by the first batch's logits
    n = 0
    for batch in val_loader:
        images = batch["image"].to(device, non_blocking=True)
        masks = batch["mask"].to(device, non_blocking=True)
        clip_features = extract_clip_features(clip_extractor, batch, images, device, input_layout)
        outputs = _forward(model, images, clip_features, input_layout)
        val_loss += loss_function(outputs, masks).detach()
        if getattr(loss_function, "target_layout", "int64") != "u8" and \
                masks.dtype != torch.int64:
            masks = masks.long()
        _, counts = ops.argmax_dice_counts(outputs, masks, ignore_label, want_preds=False)
        inter = counts[:, 0].double()
        union = (counts[:, 1] + counts[:, 2]).double()
        dice = torch.where(union > 0, 2.0 * inter / (union + 1e-5), torch.ones_like(inter))
        dice_sum = dice if dice_sum is None else dice_sum + dice
        n += 1
    n = max(n, 1)
    return (val_loss / n).item(), dice_scores(dice_sum, n)
