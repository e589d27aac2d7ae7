"""numpy restatement of the resize the letterbox kernel performs, written from the
description of OpenCV's generic fixed-point path and independently of csrc/letterbox.hip:

  linear_taps / resize_linear   INTER_LINEAR: per-axis taps with 11-bit weights, horizontal pass in
                                int, vertical pass with the two 16-bit shifts; the 2 x 2 area path
                                where both sides halve exactly
  nearest_index / resize_nearest  INTER_NEAREST
  letterbox_geometry / stretch_geometry, place, letterbox_batch   the tile of each sample
  histogram, trimap_lut         the byte counts and the label table built from them

Everything is integer arithmetic on numpy arrays except the tap positions, which are computed in
the precisions the description names (double for the position, float32 from the cast on)."""
import numpy as np

# (h, w, S): the ragged call of the GPU tests and the real sizes; the CPU tests walk the same list
SHAPES = [(37, 53, 32), (53, 37, 32), (64, 64, 32), (64, 48, 32), (20, 31, 48), (7, 5, 16),
          (1, 9, 16)]
REAL = [(500, 375, 512), (500, 375, 224)]
STRETCH = (32, 24)


def axis_scale(src, dst):
    return 1.0 / (float(dst) / float(src))            # Python floats are doubles


def linear_taps(src, dst):
    """(s0, s1, a0, a1), int32 arrays of length dst."""
    scale = axis_scale(src, dst)
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)   # two double roundings, then the cast
    fl = np.floor(f)
    s = fl.astype(np.int64)
    f = (f - fl).astype(np.float32)
    low, high = s < 0, s >= src - 1
    s = np.where(low, 0, s)
    f = np.where(low, np.float32(0), f)
    s = np.where(high, src - 1, s)
    f = np.where(high, np.float32(0), f).astype(np.float32)
    a0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int32)
    a1 = np.rint(f * np.float32(2048)).astype(np.int32)
    return s.astype(np.int32), np.minimum(s + 1, src - 1).astype(np.int32), a0, a1


def nearest_index(src, dst):
    scale = axis_scale(src, dst)
    s = np.floor(np.arange(dst, dtype=np.float64) * scale).astype(np.int64)
    return np.minimum(s, src - 1)


def is_area_case(h, w, out_h, out_w):
    return h == 2 * out_h and w == 2 * out_w


def resize_linear(img, out_h, out_w):
    """img uint8 [h, w] or [h, w, C] -> uint8 [out_h, out_w(, C)]."""
    img = np.asarray(img)
    h, w = img.shape[:2]
    v = img.astype(np.int32)
    if is_area_case(h, w, out_h, out_w):
        out = (v[0::2, 0::2] + v[0::2, 1::2] + v[1::2, 0::2] + v[1::2, 1::2] + 2) >> 2
        return out.astype(np.uint8)
    x0, x1, a0, a1 = linear_taps(w, out_w)
    y0, y1, b0, b1 = linear_taps(h, out_h)
    shape = (1, out_w) + (1,) * (v.ndim - 2)
    rows = v[:, x0] * a0.reshape(shape) + v[:, x1] * a1.reshape(shape)       # [h, out_w(, C)]
    shape = (out_h, 1) + (1,) * (v.ndim - 2)
    r0, r1 = rows[y0] >> 4, rows[y1] >> 4
    out = (((b0.reshape(shape) * r0) >> 16) + ((b1.reshape(shape) * r1) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def resize_nearest(mask, out_h, out_w):
    mask = np.asarray(mask)
    h, w = mask.shape[:2]
    return mask[nearest_index(h, out_h)][:, nearest_index(w, out_w)]


def letterbox_geometry(h, w, size):
    """(out_h, out_w, pad_y, pad_x) as resize_image_with_padding computes them."""
    if h > w:
        scale = size / h
        out_h, out_w = size, int(w * scale)
    else:
        scale = size / w
        out_w, out_h = size, int(h * scale)
    return out_h, out_w, (size - out_h) // 2, (size - out_w) // 2


def stretch_geometry(h, w, size_hw):
    return size_hw[0], size_hw[1], 0, 0


def place(resized, size_hw, pad_y, pad_x):
    tile = np.zeros(tuple(size_hw) + resized.shape[2:], dtype=np.uint8)
    tile[pad_y:pad_y + resized.shape[0], pad_x:pad_x + resized.shape[1]] = resized
    return tile


def trimap_lut(present, is_cat):
    """256 uint8: what process_mask makes of a mask whose set of byte values is `present`."""
    present = sorted(int(v) for v in present)
    cls = 1 if is_cat else 2
    lut = np.zeros(256, dtype=np.uint8)
    if 128 in present:
        lut[128] = cls
    else:
        fg = [v for v in present if v not in (0, 255)]
        if fg:
            lut[fg[0]] = cls
    lut[255] = 255
    return lut


def histogram(mask):
    return np.bincount(np.asarray(mask, dtype=np.uint8).ravel(), minlength=256).astype(np.uint64)


def letterbox_batch(samples, size_hw, mode="letterbox", luts=None):
    """samples: list of (image uint8 [h, w, 3], mask uint8 [h, w] or None).  Returns
    (images [B, S_h, S_w, 3], masks [B, S_h, S_w]); mode "letterbox" needs S_h == S_w."""
    S_h, S_w = size_hw
    images = np.zeros((len(samples), S_h, S_w, 3), dtype=np.uint8)
    masks = np.zeros((len(samples), S_h, S_w), dtype=np.uint8)
    for b, (img, msk) in enumerate(samples):
        h, w = img.shape[:2]
        if mode == "letterbox":
            assert S_h == S_w
            oh, ow, py, px = letterbox_geometry(h, w, S_h)
        else:
            oh, ow, py, px = stretch_geometry(h, w, size_hw)
        images[b] = place(resize_linear(img, oh, ow), size_hw, py, px)
        if msk is not None:
            m = resize_nearest(msk, oh, ow)
            if luts is not None:
                m = np.asarray(luts[b], dtype=np.uint8)[m]
            masks[b] = place(m, size_hw, py, px)
    return images, masks


def make_samples(shapes, seed, mask_values=(0, 1, 2, 255)):
    """Seeded ragged samples: smooth-plus-noise images (so neighbouring taps differ) and blocky
    masks over `mask_values`."""
    rng = np.random.default_rng(seed)
    out = []
    for h, w in shapes:
        img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        coarse = rng.integers(0, len(mask_values), size=((h + 3) // 4, (w + 4) // 5))
        msk = np.asarray(mask_values, dtype=np.uint8)[np.kron(coarse, np.ones((4, 5), dtype=np.int64))[:h, :w]]
        out.append((img, np.ascontiguousarray(msk)))
    return out
