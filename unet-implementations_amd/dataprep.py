"""From decoded samples to the network-size uint8 batch, on the device.

The reference produces a network-size sample with OpenCV on the host, one sample at a time:

  data_augmentation/src/preprocess_dataset.py:307-355, CLIP_UNet/scripts/
  create_clip_resized_images.py:104-152   aspect-preserving resize into a centred S x S square
                                          (cv2.resize, INTER_LINEAR), S = 512 / 224
  data_augmentation/src/preprocess_training_labels.py:109-167   the same for the mask (INTER_NEAREST)
  PetSegmentationDataset.__getitem__ (src/train.py:293-296; CLIP_UNet/src/train.py:282)
                                          a plain stretch to 512 x 512 (and 224 x 224 for CLIP)
  data_augmentation/src/preprocess_test_val_labels.py:180-331   trimap bytes -> class labels
  src/train.py main (AE_pretrained/transfer_learning/src/train.py:820-846)   static class weights

Here a `DataLoader` collates its decoded samples, each at its own size, with `ragged_collate` into
one byte arena, and `DeviceLetterbox` turns every batch into the dictionaries `train_one_epoch`,
`validate`, `evaluate_model` and the `clip` / `ae` loops read - two copies to the device and one
kernel launch per output size (`ops.letterbox_u8`), no OpenCV and no per-sample work on the host.
File decoding (JPEG / PNG to bytes) stays with the dataset.
"""
import numpy as np
import torch
from torch.utils.data import default_collate, get_worker_info

from . import ops

ARENA_ALIGN = 16        # every image and mask starts on a 16-byte boundary of the arena
_RAGGED_KEYS = ("image", "mask")

# the breed substrings of is_cat_image (preprocess_test_val_labels.py:191-195)
CAT_BREEDS = ("abyssinian", "bengal", "birman", "bombay", "british", "egyptian", "maine", "persian",
              "ragdoll", "russian", "siamese", "sphynx")


def letterbox_geometry(h, w, size):
    """(out_h, out_w, pad_y, pad_x) of resize_image_with_padding (preprocess_dataset.py:321-347),
    in Python float arithmetic as the reference writes it."""
    h, w, size = int(h), int(w), int(size)
    if h > w:
        scale = size / h
        out_h, out_w = size, int(w * scale)
    else:
        scale = size / w
        out_w, out_h = size, int(h * scale)
    if out_h < 1 or out_w < 1:
        raise ValueError(f"a {h} x {w} sample has no {size} x {size} letterbox (a side becomes 0; "
                         "cv2.resize would throw)")
    return out_h, out_w, (size - out_h) // 2, (size - out_w) // 2


def stretch_geometry(h, w, size_hw):
    """(out_h, out_w, 0, 0): the dataset's cv2.resize(image, (W, H)) fills the whole tile."""
    S_h, S_w = (int(size_hw), int(size_hw)) if isinstance(size_hw, int) else \
        (int(size_hw[0]), int(size_hw[1]))
    return S_h, S_w, 0, 0


def is_cat_image(name):
    """The reference's rule: a cat if the file name contains one of the cat breed names."""
    lower = str(name).lower()
    return any(breed in lower for breed in CAT_BREEDS)


def trimap_lut(present, is_cat):
    """256 uint8 (numpy): what process_mask (preprocess_test_val_labels.py:254-303) makes of every
    byte of a mask whose set of byte values is `present` (an iterable of values).
    128, if present, is the animal; otherwise the smallest present value other than 0 and 255 is;
    255 stays 255; everything else is background.  The animal is 1 for a cat and 2 for a dog."""
    values = sorted(int(v) for v in present)
    cls = 1 if is_cat else 2
    lut = np.zeros(256, dtype=np.uint8)
    if 128 in values:
        lut[128] = cls
    else:
        foreground = [v for v in values if v not in (0, 255)]
        if foreground:
            lut[foreground[0]] = cls
    # process_mask's later fallbacks (:273-300 "non-zero pixels", "histogram analysis", and :306-315
    # "anything not 0 or 255") are unreachable once one of the two branches above is taken: they
    # need a mask with a value strictly between 0 and 255 and yet an empty `foreground_values`,
    # and a mask with no such value has nothing they could mark.  (A mask of one single value
    # skips the `elif len(unique_values) > 1` and reaches :306-315, which marks the bytes the rule
    # above marks.)
    lut[255] = 255
    return lut


def _device_trimap_luts(hist, is_cat):
    """`trimap_lut` for every row of hist int64 [B, 256] (device), is_cat bool [B] (device):
    uint8 [B, 256] built from the presence bits without reading anything on the host."""
    B = hist.shape[0]
    present = hist > 0
    cand = present.clone()
    cand[:, 0] = False
    cand[:, 255] = False
    first = torch.argmax(cand.to(torch.uint8), dim=1)              # first True (0 if none)
    has_fg = present[:, 128] | cand.any(dim=1)
    fg = torch.where(present[:, 128], torch.full_like(first, 128), first)
    cls = torch.where(is_cat, 1, 2).to(torch.uint8)
    cls = torch.where(has_fg, cls, torch.zeros_like(cls))           # no foreground: lut[0] = 0
    lut = torch.zeros((B, 256), dtype=torch.uint8, device=hist.device)
    lut.scatter_(1, fg[:, None], cls[:, None])
    lut[:, 255] = 255
    return lut


def _as_numpy_u8(x, what):
    a = x.numpy() if torch.is_tensor(x) else np.asarray(x)
    if a.dtype != np.uint8:
        raise TypeError(f"ragged_collate: {what} must be uint8, got {a.dtype}")
    return a


def _align(n):
    return (n + ARENA_ALIGN - 1) // ARENA_ALIGN * ARENA_ALIGN


def ragged_collate(samples):
    """collate_fn for decoded samples of different sizes: a list of {"image": uint8 [h, w, 3],
    "mask": uint8 [h, w] (optional), ...} (numpy or torch).  Returns
        "arena"          uint8 [bytes]: every image and mask, each at a 16-byte aligned offset
                         (pinned when collated in the main process of a machine with a GPU; in a
                         worker, leave pinning to DataLoader(pin_memory=True))
        "table"          int64 [B, 4]: image offset, mask offset (-1: none), h, w
        "original_dims"  int64 [B, 2]: (h, w)
    and every other key collated as `default_collate` does."""
    if not samples:
        raise ValueError("ragged_collate: empty batch")
    rows, total, items = [], 0, []
    for s in samples:
        img = _as_numpy_u8(s["image"], "image")
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError(f"ragged_collate: image must be [h, w, 3], got {img.shape}")
        h, w = img.shape[:2]
        msk = s.get("mask")
        if msk is not None:
            msk = _as_numpy_u8(msk, "mask")
            if msk.shape != (h, w):
                raise ValueError(f"ragged_collate: mask {msk.shape} does not match image {(h, w)}")
        img_off, total = total, _align(total + img.size)
        msk_off = -1
        if msk is not None:
            msk_off, total = total, _align(total + msk.size)
        rows.append((img_off, msk_off, h, w))
        items.append((img, msk))
    arena = torch.empty(total, dtype=torch.uint8)
    if torch.cuda.is_available() and get_worker_info() is None:
        arena = arena.pin_memory()
    flat = arena.numpy()
    for (img_off, msk_off, h, w), (img, msk) in zip(rows, items):
        flat[img_off:img_off + img.size] = img.reshape(-1)
        flat[img_off + img.size:_align(img_off + img.size)] = 0
        if msk is not None:
            flat[msk_off:msk_off + msk.size] = msk.reshape(-1)
            flat[msk_off + msk.size:_align(msk_off + msk.size)] = 0
    table = torch.tensor(rows, dtype=torch.int64)
    batch = {"arena": arena, "table": table, "original_dims": table[:, 2:4].clone()}
    rest = [{k: v for k, v in s.items() if k not in _RAGGED_KEYS and k != "original_dims"}
            for s in samples]
    if rest[0]:
        batch.update(default_collate(rest))
    return batch


def full_table(table, size, mode):
    """int64 [B, 8] (host): the records of `unet_letterbox_u8` for a `ragged_collate` table and one
    output size - `letterbox_geometry` (size: S) or `stretch_geometry` (size: S or (S_h, S_w))."""
    if mode not in ("letterbox", "stretch"):
        raise ValueError("mode must be 'letterbox' or 'stretch'")
    rows = []
    for img_off, msk_off, h, w in table.tolist():
        if mode == "letterbox":
            if not isinstance(size, int):
                raise ValueError("mode='letterbox' takes one square size")
            geom = letterbox_geometry(h, w, size)
        else:
            geom = stretch_geometry(h, w, size)
        rows.append((img_off, msk_off, h, w) + tuple(geom))
    return torch.tensor(rows, dtype=torch.int64)


def _size_hw(size):
    return (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))


class DeviceLetterbox:
    """Wraps a loader whose collate_fn is `ragged_collate` and yields network-size batches:

        "image"          uint8 [B, S, S, 3] on the device (what `input_layout="nhwc_u8"` takes)
        "mask"           uint8 [B, S, S] (what a loss of `target_layout="u8"` takes; the loops turn
                         it into int64 where a kernel wants that) - when the samples carry masks
        "original_dims"  int64 [B, 2], as the default collate builds it
        "clip_image"     uint8 [B, c, c, 3] with `clip_size=c`: the letterbox of
                         create_clip_resized_images.py or the stretch of CLIP_UNet/src/train.py:282,
                         according to `mode`
    and the loader's other keys ("which", "is_cat", ...) unchanged.  Per batch: one copy of the
    arena and one of the tables to the device, then one launch per output size.

    mode          "letterbox" (the preprocessing scripts) or "stretch" (the dataset's resize)
    label_lut     None, a uint8 [256] table applied to every mask, or "trimap": the byte histogram
                  of each original mask (`ops.byte_histogram_u8`) decides its table as `trimap_lut`
                  does, on the device; the batch must carry "is_cat" (bool per sample).  The
                  trimap rule is the pet dataset's: with `num_classes` other than 3 it raises
    image_format  "nhwc_u8" (default), or "nchw_f32": the image normalised with `mean` / `std` by
                  `ops.preprocess_u8`, as a [B, 3, S, S] view, for loops that call `model(images)`
                  without an input layout (`evaluate_model`, the `ae` loops)
    target        None, or "image": also yield "target" = the uint8 [B, S, S, 3] image (the
                  autoencoder's target for a loss of `target_layout="nhwc_u8"`)"""

    def __init__(self, loader, size=512, mode="letterbox", clip_size=None, label_lut=None,
                 device="cuda", image_format="nhwc_u8", mean=ops.IMAGENET_MEAN,
                 std=ops.IMAGENET_STD, target=None, num_classes=3):
        if isinstance(label_lut, str) and label_lut == "trimap" and num_classes != 3:
            raise NotImplementedError("label_lut='trimap' re-encodes the pet trimap's bytes into "
                                      f"its 3 classes (got num_classes={num_classes}): pass a "
                                      "uint8 [256] table, or None")
        if mode not in ("letterbox", "stretch"):
            raise ValueError("mode must be 'letterbox' or 'stretch'")
        if image_format not in ("nhwc_u8", "nchw_f32"):
            raise ValueError("image_format must be 'nhwc_u8' or 'nchw_f32'")
        if target not in (None, "image"):
            raise ValueError("target must be None or 'image'")
        if mode == "letterbox" and not isinstance(size, int):
            raise ValueError("mode='letterbox' takes one square size")
        if isinstance(label_lut, str):
            if label_lut != "trimap":
                raise ValueError("label_lut must be None, 'trimap' or a uint8 [256] table")
        elif label_lut is not None:
            label_lut = torch.as_tensor(np.asarray(label_lut)).reshape(-1)
            if label_lut.dtype != torch.uint8 or label_lut.numel() != 256:
                raise ValueError("label_lut must be None, 'trimap' or a uint8 [256] table")
        self.loader, self.size, self.mode = loader, size, mode
        self.clip_size, self.label_lut = clip_size, label_lut
        self.device = torch.device(device)
        self.image_format, self.mean, self.std, self.target = image_format, mean, std, target
        self._fixed_lut = None

    def __len__(self):
        return len(self.loader)

    @property
    def dataset(self):
        return self.loader.dataset

    def _luts(self, arena, table, batch, B):
        if self.label_lut is None:
            return None
        if not isinstance(self.label_lut, str):
            if self._fixed_lut is None:
                self._fixed_lut = self.label_lut.to(self.device)
            return self._fixed_lut[None].expand(B, 256).contiguous()
        if "is_cat" not in batch:
            raise KeyError('label_lut="trimap" needs an "is_cat" entry per sample')
        is_cat = torch.as_tensor(batch["is_cat"]).to(self.device, non_blocking=True).bool()
        return _device_trimap_luts(ops.byte_histogram_u8(arena, table), is_cat)

    def convert(self, batch):
        """One `ragged_collate` batch -> the dictionary described above."""
        host = batch["table"]
        B = host.shape[0]
        tables = [full_table(host, self.size, self.mode)]
        if self.clip_size is not None:
            tables.append(full_table(host, self.clip_size, self.mode))
        tables = torch.stack(tables)
        if self.device.type == "cuda":
            tables = tables.pin_memory()
        tables = tables.to(self.device, non_blocking=True)
        arena = batch["arena"].to(self.device, non_blocking=True)
        has_mask = bool((host[:, 1] >= 0).any())
        lut = self._luts(arena, tables[0], batch, B) if has_mask else None
        image, mask = ops.letterbox_u8(arena, tables[0], self.size, want_mask=has_mask, lut=lut)
        out = {k: v for k, v in batch.items() if k not in ("arena", "table")}
        if self.target == "image":
            out["target"] = image
        if self.image_format == "nchw_f32":
            out["image"] = ops.preprocess_u8(image, None, self.mean, self.std)[0].permute(0, 3, 1, 2)
        else:
            out["image"] = image
        if has_mask:
            out["mask"] = mask
        if self.clip_size is not None:
            out["clip_image"] = ops.letterbox_u8(arena, tables[1], self.clip_size,
                                                 want_mask=False)[0]
        return out

    def __iter__(self):
        for batch in self.loader:
            yield self.convert(batch)


def class_weights_from_counts(counts, num_classes=3, ignore_index=255):
    """The arithmetic of the reference's static class weights (src/train.py main) from byte counts
    [..., 256] (summed over the leading axes): class pixels clamped to >= 1, total valid pixels /
    class pixels, normalised to sum to num_classes - in fp32 as the reference computes it.
    Valid pixels are all that are not `ignore_index`."""
    counts = torch.as_tensor(counts).reshape(-1, 256).sum(dim=0)
    class_pixels = counts[:num_classes].to(torch.float32)
    total_valid = (counts.sum() - counts[ignore_index]).to(torch.float32)
    class_pixels = torch.clamp(class_pixels, min=1.0)
    weights = total_valid / class_pixels
    return weights * (num_classes / weights.sum())


def static_class_weights(loader, num_classes=3, ignore_index=255):
    """The scan of src/train.py main over a loader's masks (uint8 [B, H, W] under "mask", on any
    device - a `DeviceLetterbox` or a loader of pre-resized batches): one histogram launch per
    batch, summed on the device, one read at the end.  Returns the fp32 [num_classes] weights on
    the masks' device, for `SimpleLoss(class_weights=..., dynamic_weights=False)`."""
    total = None
    for batch in loader:
        masks = batch["mask"]
        if not masks.is_cuda:
            masks = masks.to("cuda", non_blocking=True)
        if masks.dtype != torch.uint8:
            masks = masks.to(torch.uint8)
        hist = ops.byte_histogram_u8(masks.contiguous()).sum(dim=0)
        total = hist if total is None else total + hist
    if total is None:
        raise ValueError("static_class_weights: the loader is empty")
    return class_weights_from_counts(total, num_classes, ignore_index)
