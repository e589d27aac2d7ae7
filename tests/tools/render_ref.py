"""numpy restatement of the evaluation pictures: what
unet_render_seg_panels / unet_render_recon_panels must write, byte for byte, and the seeded inputs
the fixture tests/golden/render.npz and the GPU tests share.

The segmentation panels restate Our_UNet/utils/visualize.py (colorize_mask,
create_error_visualization, the denormalisation lines) and are pinned to the reference's own
output by render.npz (tests/tools/make_golden_render.py).  The autoencoder's comparison picture
restates AE_pretrained/reconstruction/utils/visualize.py; that module needs cv2, so its gray
conversion is OpenCV's documented fixed-point formula and rests on this restatement alone.
"""
import struct
import zlib

import numpy as np

MEAN = np.array([0.485, 0.456, 0.406])
STD = np.array([0.229, 0.224, 0.225])
REDS_LOW, REDS_HIGH = (255, 245, 240), (103, 0, 12)
PANELS = ("image", "gt", "pred", "error", "conf0", "conf1", "conf2", "target", "heat")
ERROR_COLOURS = np.array([[0, 0, 0], [0, 255, 0], [255, 0, 0], [0, 0, 255], [255, 255, 0]],
                         dtype=np.uint8)

_JET = (((0.0, 0.0), (0.35, 0.0), (0.66, 1.0), (0.89, 1.0), (1.0, 0.5)),
        ((0.0, 0.0), (0.125, 0.0), (0.375, 1.0), (0.64, 1.0), (0.91, 0.0), (1.0, 0.0)),
        ((0.0, 0.5), (0.11, 1.0), (0.34, 1.0), (0.65, 0.0), (1.0, 0.0)))


def jet_lut():
    x = np.linspace(0.0, 1.0, 256)
    cols = [(np.interp(x, *np.array(p).T) * 255).astype(np.uint8) for p in _JET]
    return np.stack(cols, axis=1)


# ---- segmentation panels -------------------------------------------------------------------------
def image_bytes(image):
    """uint8 [B,H,W,3] of an fp32 [B,3,H,W] normalised image (float32 array x float64 array, as the
    reference computes it), or of the uint8 [B,H,W,3] bytes themselves."""
    if image.dtype == np.uint8:
        return image
    img = image.transpose(0, 2, 3, 1) * STD + MEAN
    return (np.clip(img, 0, 1) * 255).astype(np.uint8)


def colorize(mask):
    out = np.zeros(mask.shape + (3,), dtype=np.uint8)
    out[mask == 1] = (255, 0, 0)
    out[mask == 2] = (0, 255, 0)
    return out


def error_code(pred, gt):
    gt = np.where(gt == 255, 0, gt)
    pf, gf = pred > 0, gt > 0
    code = np.zeros(pred.shape, dtype=np.int64)
    code[pf & gf & (pred == gt)] = 1
    code[pf & ~gf] = 2
    code[~pf & gf] = 3
    code[pf & gf & (pred != gt)] = 4
    return code


def half_sum(a, b):
    return ((a.astype(np.int32) + np.asarray(b).astype(np.int32)) >> 1).astype(np.uint8)


def softmax64(logits):
    z = logits.astype(np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def lut_index(v):
    v = np.where(np.isnan(v), 0.0, np.clip(v, 0.0, 1.0))
    return np.minimum((v * 256).astype(np.int64), 255)


def seg_panel(name, image, logits=None, mask=None, heat=None, target_class=1):
    """uint8 [B,H,W,3]: one panel."""
    img = image_bytes(image)
    if name == "image":
        return img
    if name == "gt":
        return colorize(mask)
    pred = logits.argmax(axis=1) if logits is not None else None      # first maximum wins
    if name == "pred":
        return colorize(pred)
    if name == "error":
        return half_sum(img, ERROR_COLOURS[error_code(pred, mask.astype(np.int64))])
    if name.startswith("conf"):
        return half_sum(img, jet_lut()[lut_index(softmax64(logits)[:, int(name[4])])])
    if name == "target":
        c = np.where((mask == target_class)[..., None], np.array(REDS_HIGH), np.array(REDS_LOW))
        return half_sum(img, c)
    if name == "heat":
        return half_sum(img, jet_lut()[lut_index(heat.astype(np.float64))])
    raise ValueError(name)


def seg_panels(image, logits, mask, heat, panels, target_class=1):
    """uint8 [B,H,P,W,3], the layout of unet_render_seg_panels."""
    return np.stack([seg_panel(p, image, logits, mask, heat, target_class) for p in panels], axis=2)


def conf_band(logits, c, margin=1e-3):
    """bool [B,H,W]: pixels whose p * 256 lies within `margin` of an integer - where an fp32
    softmax may land in the neighbouring table entry."""
    s = softmax64(logits)[:, c] * 256
    return np.abs(s - np.round(s)) < margin


# ---- the autoencoder's comparison picture --------------------------------------------------------
def unit_bytes(image):
    """uint8 [B,H,W,3] of an fp32 [B,3,H,W] image in [0, 1] (clamp, * 255 in float32, truncate),
    or the uint8 [B,H,W,3] bytes themselves."""
    if image.dtype == np.uint8:
        return image
    x = np.clip(image.astype(np.float32), np.float32(0), np.float32(1)).transpose(0, 2, 3, 1)
    return (x * np.float32(255)).astype(np.uint8)


def recon_panels(original, recon):
    """uint8 [B,H,3,W,3]: original | reconstruction | error map, the maximum per image."""
    o, r = unit_bytes(original), unit_bytes(recon)
    lut = jet_lut()
    maps = []
    for b in range(o.shape[0]):
        d = np.abs(o[b].astype(np.float32) - r[b].astype(np.float32))
        m = d.max()
        e = (d / m * np.float32(255)).astype(np.uint8).astype(np.int64) if m > 0 else \
            np.zeros(d.shape, dtype=np.int64)
        gray = (4899 * e[..., 0] + 9617 * e[..., 1] + 1868 * e[..., 2] + 8192) >> 14
        maps.append(lut[gray])
    return np.stack([o, r, np.stack(maps)], axis=2)


# ---- seeded inputs -------------------------------------------------------------------------------
def make_seg_case(seed, B, H, W):
    """(image_u8 [B,H,W,3], image_f32 [B,3,H,W], logits [B,3,H,W], mask int64 [B,H,W]).
    The normalised image is built from the bytes so that every value sits next to a truncation
    boundary: (v + 0.5) / 255 normalised in float64 and rounded to float32 comes back as v, and
    the pixels nudged to (v + 1e-4) / 255 and (v - 1e-4) / 255 decide between v and v - 1.
    The mask holds 0, 1, 2, 255 and an out-of-range 7; the logits hold exact two- and three-way
    ties."""
    rng = np.random.default_rng(seed)
    u8 = rng.integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)
    nudge = rng.choice(np.array([0.5, 1e-4, -1e-4, 0.999]), size=u8.shape)
    unit = (u8.astype(np.float64) + nudge) / 255
    f32 = ((unit - MEAN) / STD).transpose(0, 3, 1, 2).astype(np.float32)
    f32.reshape(-1)[:4] = (-9.0, 9.0, 0.0, -0.0)                   # below 0 and above 1 after denorm
    logits = (rng.standard_normal((B, 3, H, W)) * 2).astype(np.float32)
    flat = logits.reshape(B, 3, -1)
    n = flat.shape[2]
    flat[:, 1, 0:n:7] = flat[:, 0, 0:n:7]                          # 0 == 1
    flat[:, 2, 1:n:11] = flat[:, 1, 1:n:11]                        # 1 == 2
    flat[:, :, 2:n:13] = flat[:, 0:1, 2:n:13]                      # 0 == 1 == 2
    mask = rng.choice(np.array([0, 1, 2, 255, 7], dtype=np.int64), size=(B, H, W),
                      p=[0.4, 0.25, 0.25, 0.07, 0.03])
    return u8, np.ascontiguousarray(f32), logits, mask


def make_recon_case(seed, B, H, W):
    """(original fp32 [B,3,H,W] in [0,1] with some values outside, recon fp32): per-image
    differences of very different size, so the per-image maxima differ."""
    rng = np.random.default_rng(seed)
    o = rng.random((B, 3, H, W)).astype(np.float32)
    scale = np.array([0.02, 0.1, 1.0] * B, dtype=np.float32)[:B].reshape(B, 1, 1, 1)
    r = (o + scale * rng.standard_normal(o.shape).astype(np.float32)).astype(np.float32)
    o.reshape(-1)[:3] = (-0.25, 1.5, 1.0)
    return o, r


# ---- PNG decoding (8-bit RGB, filter 0..4, no interlace: more than write_png emits) --------------
def read_png(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, W = 8, b"", None
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body)
        if tag == b"IHDR":
            W, H, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", body)
            assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(H, 1 + 3 * W)
    assert not rows[:, 0].any(), "only filter type 0 is decoded"
    return rows[:, 1:].reshape(H, W, 3).copy()
