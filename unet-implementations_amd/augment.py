"""Online augmentation of uint8 training batches on the device (csrc/augment.hip).

The reference augments offline: data_augmentation/src/augment_dataset.py runs its pipeline on the
CPU once and stores a fixed set of augmented files, so a model sees the same pixels every epoch.
Here the batch that is already on the device as uint8 goes through ONE kernel launch that writes
an augmented uint8 batch of the same shape; everything downstream (`input_layout="nhwc_u8"`,
`SimpleLoss(target_layout="u8")`, `GraphedTrainStep`) takes it as it takes the dataset's bytes.

    cfg = AugmentConfig.from_yaml("augmentation_config.yaml", "cat")
    aug = BatchAugment(cfg, seed=0)
    images, masks = aug(images_u8, masks_u8)              # uint8 [N,H,W,3] / [N,H,W], new draws

Supported transforms, and how each is realised:

    HorizontalFlip, ShiftScaleRotate (about the centre), RandomResizedCrop (to the batch size),
    Perspective (four-corner displacement, keep_size)
        composed on the host in fp64 into ONE inverse homography per sample: the image is
        resampled once (bilinear, zeros outside), the mask once (nearest, a border value outside)
    CoarseDropout with one hole            the hole fields of the record
    RandomBrightnessContrast (v * alpha + beta * 255) and RGBShift
                                           folded into alpha / beta_c
    ToGray                                 the gray flag
    GaussNoise (var_limit -> sigma)        sigma
    SaltAndPepper                          two thresholds on a per-pixel random word
    OneOf(ElasticTransform, GridDistortion, OpticalDistortion)
        a second record of 64 floats per sample (`sample_warp`) that warps the OUTPUT frame in
        front of the homography, still one resampling pass: the elastic member's smoothed random
        displacement field is written by a kernel of its own (`unet_elastic_field`), the grid
        member is a monotone piecewise-linear map per axis, the optical member a radial
        polynomial.  Only a `BatchAugment` whose configuration has `distort_group_prob > 0`
        draws these records and launches the two kernels; `from_yaml(..., distortion=True)`
        reads the group from the reference's file.

    HueSaturationValue, OneOf(CLAHE, Equalize), OneOf(GaussianBlur, MotionBlur)
        a third record of 64 floats per sample (`sample_post`) and a SECOND STAGE of two kernels
        over the image the gather wrote (`unet_augment_post_u8`, csrc/augment_post.hip): a
        histogram kernel (per-sample counts for Equalize, per-tile LUTs for CLAHE on luma) and a
        tiled kernel that applies the HSV shift, the LUTs, the blur (separable Gaussian taps or
        the dense weights of a rasterised motion line, both from the record) and, last, salt /
        pepper, which moves there from the gather.  Only a `BatchAugment` whose configuration
        has one of these members on draws the record and launches the stage;
        `from_yaml(..., photometric=True)` reads them from the reference's file.

    ISONoise, OneOf(RandomShadow, RandomSunFlare, RandomFog)
        a fourth record of 272 floats per sample (`sample_light`) and a THIRD STAGE of two kernels
        (`unet_augment_light_u8`, csrc/augment_light.hip) over the image the gather or the second
        stage wrote: a statistics kernel (exact integer sums of the lightness, for the Poisson
        rate of ISO noise) and a tiled kernel that applies ISO noise (hue by a normal, lightness
        by a Poisson draw, in float HLS), then the shadow polygons, the flare's circles or the
        fog's points through byte-rounded blends, the fog's box mean from a staged tile.  Only a
        `BatchAugment` whose configuration has `iso_noise_prob > 0` or `lighting_group_prob > 0`
        draws the record and launches the stage; `from_yaml(..., lighting=True)` reads them from
        the reference's file.

`OneOf` groups keep the reference's structure over the supported members: the group probability
is drawn first, then one member by its normalised probability among the SUPPORTED members (with
the second stage on, the new members count: `sample_post`).

With `from_yaml(path, section, distortion=True, photometric=True, lighting=True)` every key of
the reference's file is read.
The semantics of what is supported are defined by this project (include/unet_hip.h, DESIGN 12,
12b, 12c, 12d), not recorded from the reference's augmentation library; the package ships no preset
numbers: every probability of `AugmentConfig` defaults to 0, which is the identity.
"""
import collections
import dataclasses
import itertools
import math
from typing import Tuple

import numpy as np
import torch

from . import ops

PARAMS_PER_SAMPLE = 24
WARP_PER_SAMPLE = 64
# warp record layout (include/unet_hip.h): value 0 is the mode, the rest belongs to the mode
WARP_NONE, WARP_ELASTIC, WARP_GRID, WARP_OPTICAL = 0, 1, 2, 3
W_AFFINE, W_ALPHA, W_RADIUS, W_TAPS = 1, 7, 8, 9                   # elastic
W_KX, W_INVCELL_X, W_KY, W_INVCELL_Y, W_AX, W_BX, W_AY, W_BY = 1, 2, 3, 4, 8, 16, 24, 32    # grid
W_CX, W_CY, W_K, W_INV_W, W_INV_H = 1, 2, 3, 4, 5                   # optical
MAX_RADIUS = 16
MAX_GRID_STEPS = 8
# record layout (include/unet_hip.h)
P_H, P_ALPHA, P_BETA, P_GRAY, P_SIGMA, P_HOLE, P_HOLE_FILL, P_MASK_BORDER, P_MASK_HOLE = \
    0, 9, 10, 13, 14, 15, 19, 20, 21
# post record layout (include/unet_hip.h): the second stage
POST_PER_SAMPLE = 64
Q_HSV, Q_DH, Q_DS, Q_DV, Q_HIST, Q_CLIP, Q_TY, Q_TX, Q_BLUR, Q_RADIUS, Q_TAPS, Q_DENSE = \
    0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 15
HIST_NONE, HIST_EQUALIZE, HIST_CLAHE = 0, 1, 2
BLUR_NONE, BLUR_SEPARABLE, BLUR_DENSE = 0, 1, 2
MAX_BLUR_RADIUS = {BLUR_SEPARABLE: 4, BLUR_DENSE: 3}
MAX_TILE_GRID = 8
# light record layout (include/unet_hip.h): the third stage
LIGHT_PER_SAMPLE = 272
L_ISO, L_SIGMA_H, L_INTENSITY, L_MODE, L_COUNT, L_BODY = 0, 1, 2, 3, 4, 16
L_SRC_X, L_SRC_Y, L_SRC_RADIUS, L_STEPS = 5, 6, 7, 8               # sun flare
L_FOG_RADIUS, L_FOG_ALPHA, L_FOG_BOX = 5, 6, 7                     # fog
LIGHT_NONE, LIGHT_SHADOW, LIGHT_FLARE, LIGHT_FOG = 0, 1, 2, 3
MAX_POLYGONS, MAX_FLARE_CIRCLES, MAX_FOG_POINTS, MAX_FLARE_STEPS, MAX_FOG_BOX = 2, 10, 128, 40, 9
PERSPECTIVE_CLIP = 3.0      # a corner moves inward by min(|z|, 3) * scale of the image size


def _pair(v):
    """A limit given as one number means (-v, v), as in the reference's library."""
    if isinstance(v, (int, float)):
        return (-float(v), float(v))
    a, b = v
    return (float(a), float(b))


def _blur_limit(v):
    """A kernel-size limit given as one number means (3, v), as in the reference's library."""
    if isinstance(v, (int, float)):
        return (3, int(v))
    a, b = v
    return (int(a), int(b))


@dataclasses.dataclass
class AugmentConfig:
    """Probabilities and limits of the supported transforms; the default is the identity."""
    horizontal_flip_prob: float = 0.0
    # ShiftScaleRotate about the image centre: shift in fractions of the size, scale 1 + U(limit),
    # rotation in degrees
    shift_scale_rotate_prob: float = 0.0
    shift_limit: Tuple[float, float] = (0.0, 0.0)
    scale_limit: Tuple[float, float] = (0.0, 0.0)
    rotate_limit: Tuple[float, float] = (0.0, 0.0)
    # RandomResizedCrop to the batch size: area fraction and (log-uniform) aspect ratio
    crop_prob: float = 0.0
    crop_scale: Tuple[float, float] = (1.0, 1.0)
    crop_ratio: Tuple[float, float] = (1.0, 1.0)
    # Perspective: each corner moves inward by min(|N(0, 1)|, 3) * s of the size, s ~ U(scale)
    perspective_prob: float = 0.0
    perspective_scale: Tuple[float, float] = (0.0, 0.0)
    # CoarseDropout, one hole (sizes in pixels, inclusive)
    dropout_prob: float = 0.0
    dropout_height: Tuple[int, int] = (0, 0)
    dropout_width: Tuple[int, int] = (0, 0)
    dropout_fill: float = 0.0
    dropout_mask_fill: float = 0.0
    # OneOf(RandomBrightnessContrast, RGBShift)
    color_prob: float = 0.0
    brightness_contrast_prob: float = 0.0
    brightness_limit: Tuple[float, float] = (0.0, 0.0)
    contrast_limit: Tuple[float, float] = (0.0, 0.0)
    rgb_shift_prob: float = 0.0
    rgb_shift_limit: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    # OneOf(ToGray)
    gray_group_prob: float = 0.0
    to_gray_prob: float = 0.0
    # OneOf(GaussNoise)
    noise_group_prob: float = 0.0
    gauss_noise_prob: float = 0.0
    gauss_var_limit: Tuple[float, float] = (0.0, 0.0)
    # SaltAndPepper: shares of the pixels
    salt_pepper_prob: float = 0.0
    salt_p: Tuple[float, float] = (0.0, 0.0)
    pepper_p: Tuple[float, float] = (0.0, 0.0)
    # value of mask pixels that come from outside the image
    mask_border_value: float = 0.0
    # OneOf(ElasticTransform, GridDistortion, OpticalDistortion): the warp record
    distort_group_prob: float = 0.0
    # displacement alpha * (uniform noise smoothed by a Gaussian of sigma), in pixels, on top of an
    # affine part that moves three anchor points by U(-alpha_affine, alpha_affine) pixels
    elastic_prob: float = 0.0
    elastic_alpha: float = 0.0
    elastic_sigma: float = 0.0
    elastic_alpha_affine: float = 0.0
    # num_steps cells per axis (1..8), each of weight 1 + U(-distort_limit, distort_limit) (< 1)
    grid_distortion_prob: float = 0.0
    grid_num_steps: int = 0
    grid_distort_limit: float = 0.0
    # f = 1 + k r^2 + k r^4, k ~ U(-distort_limit, distort_limit), about a centre shifted by
    # U(-shift_limit, shift_limit) of the size
    optical_distortion_prob: float = 0.0
    optical_distort_limit: float = 0.0
    optical_shift_limit: float = 0.0
    # the members of the three photometric groups that need the second stage (`sample_post`):
    # HueSaturationValue in the colour group: shifts U(-limit, limit), hue in half-degrees
    # (h in [0, 180)), saturation and value in levels
    hsv_prob: float = 0.0
    hue_shift_limit: float = 0.0
    sat_shift_limit: float = 0.0
    val_shift_limit: float = 0.0
    # CLAHE (clip limit U(1, clahe_clip_limit), tile grid (rows, columns), each 1..8 and dividing
    # the batch shape) and Equalize in the gray group
    clahe_prob: float = 0.0
    clahe_clip_limit: float = 1.0
    clahe_tile_grid: Tuple[int, int] = (8, 8)
    equalize_prob: float = 0.0
    # GaussianBlur (kernel size uniform over the odd values in [max(3, lo), hi], hi <= 9) and
    # MotionBlur (odd sizes in [max(3, lo), hi], hi <= 7) in the noise group
    gaussian_blur_prob: float = 0.0
    gaussian_blur_limit: Tuple[int, int] = (3, 3)
    motion_blur_prob: float = 0.0
    motion_blur_limit: Tuple[int, int] = (3, 3)
    # the third stage (`sample_light`).  ISONoise: colour shift and intensity drawn from their
    # ranges; the hue noise has sigma = color_shift * 360 * intensity degrees, the Poisson rate
    # of the lightness noise is intensity * 255 * std(L) of the sample
    iso_noise_prob: float = 0.0
    iso_color_shift: Tuple[float, float] = (0.0, 0.0)
    iso_intensity: Tuple[float, float] = (0.0, 0.0)
    # OneOf(RandomShadow, RandomSunFlare, RandomFog)
    lighting_group_prob: float = 0.0
    shadow_prob: float = 0.0
    sunflare_prob: float = 0.0
    sunflare_src_radius: int = 400      # 20..400; the source is drawn in src_radius // 10 steps
    fog_prob: float = 0.0
    fog_coef: Tuple[float, float] = (0.0, 0.0)
    fog_alpha_coef: float = 0.0

    @classmethod
    def from_yaml(cls, path, section, distortion=False, photometric=False, lighting=False):
        """The `section` ("cat" / "dog") of a file in the format of the reference's
        data_augmentation/config/augmentation_config.yaml.  Keys of unsupported transforms are
        ignored; a transform whose keys are absent stays off.  The elastic / grid / optical
        group (`elastic_transform_prob`, `elastic`, `grid_distortion`, `optical_distortion`) is
        read with `distortion=True` only: it costs a second record and a second kernel per
        batch, so a caller asks for it.  Likewise `photometric=True` reads the members that
        need the second stage (`hsv`; `clahe_prob`, `clahe_clip_limit`, `clahe_tile_grid_size`
        and `equalize_prob` of `clahe_equalize`; `gaussian_blur`; `motion_blur`), which then
        share their groups' probabilities with the old members (`sample_post`), and
        `lighting=True` the third stage (`iso_noise`; `lighting_transform_prob`, `shadow`,
        `sunflare`, `fog`).  With all three every key of the reference's file is read
        (`random_resized_crop.size` is read and not used: the crop is resized to the batch's
        own shape)."""
        import yaml      # lazily: only this constructor needs it
        with open(path) as f:
            doc = yaml.safe_load(f)
        if section not in doc:
            raise KeyError(f"{path} has no section '{section}' (found {sorted(doc)})")
        s = doc[section]
        c = cls()
        c.horizontal_flip_prob = float(s.get("horizontal_flip_prob", 0.0))
        c.shift_scale_rotate_prob = float(s.get("shift_scale_rotate_prob", 0.0))
        c.shift_limit = _pair(s.get("shift_limit", 0.0))
        c.scale_limit = _pair(s.get("scale_limit", 0.0))
        c.rotate_limit = _pair(s.get("rotate_limit", 0.0))
        g = s.get("random_resized_crop") or {}
        c.crop_prob = float(g.get("prob", 0.0))
        c.crop_scale = _pair(g.get("scale", (1.0, 1.0)))
        c.crop_ratio = _pair(g.get("ratio", (1.0, 1.0)))
        g.get("size")       # the crop is resized to the shape of the batch, whatever this says
        g = s.get("perspective") or {}
        c.perspective_prob = float(g.get("prob", 0.0))
        sc = g.get("scale", (0.0, 0.0))
        c.perspective_scale = (0.0, float(sc)) if isinstance(sc, (int, float)) else _pair(sc)
        g = s.get("coarse_dropout") or {}
        if int(g.get("max_holes", 1)) != 1:
            raise ValueError("CoarseDropout is supported with one hole (max_holes: 1)")
        c.dropout_prob = float(g.get("prob", 0.0))
        c.dropout_height = (int(g.get("min_height", 0)), int(g.get("max_height", 0)))
        c.dropout_width = (int(g.get("min_width", 0)), int(g.get("max_width", 0)))
        c.dropout_fill = float(g.get("fill_value", 0.0))
        c.color_prob = float(s.get("color_transform_prob", 0.0))
        g = s.get("brightness_contrast") or {}
        c.brightness_contrast_prob = float(g.get("prob", 0.0))
        c.brightness_limit = _pair(g.get("brightness_limit", 0.0))
        c.contrast_limit = _pair(g.get("contrast_limit", 0.0))
        g = s.get("rgb_shift") or {}
        c.rgb_shift_prob = float(g.get("prob", 0.0))
        c.rgb_shift_limit = tuple(float(g.get(k, 0.0))
                                  for k in ("r_shift_limit", "g_shift_limit", "b_shift_limit"))
        g = s.get("clahe_equalize") or {}
        c.gray_group_prob = float(g.get("prob", 0.0))
        c.to_gray_prob = float(g.get("to_gray_prob", 0.0))
        c.noise_group_prob = float(s.get("noise_transform_prob", 0.0))
        g = s.get("gauss_noise") or {}
        c.gauss_noise_prob = float(g.get("prob", 0.0))
        c.gauss_var_limit = _pair(g.get("var_limit", (0.0, 0.0)))
        g = s.get("salt_pepper") or {}
        c.salt_pepper_prob = float(g.get("prob", 0.0))
        c.salt_p = _pair(g.get("salt_p", (0.0, 0.0)))
        c.pepper_p = _pair(g.get("pepper_p", (0.0, 0.0)))
        if distortion:
            c.distort_group_prob = float(s.get("elastic_transform_prob", 0.0))
            g = s.get("elastic") or {}
            c.elastic_prob = float(g.get("prob", 0.0))
            c.elastic_alpha = float(g.get("alpha", 0.0))
            c.elastic_sigma = float(g.get("sigma", 0.0))
            c.elastic_alpha_affine = float(g.get("alpha_affine", 0.0))
            g = s.get("grid_distortion") or {}
            c.grid_distortion_prob = float(g.get("prob", 0.0))
            c.grid_num_steps = int(g.get("num_steps", 0))
            c.grid_distort_limit = float(g.get("distort_limit", 0.0))
            g = s.get("optical_distortion") or {}
            c.optical_distortion_prob = float(g.get("prob", 0.0))
            c.optical_distort_limit = float(g.get("distort_limit", 0.0))
            c.optical_shift_limit = float(g.get("shift_limit", 0.0))
        if photometric:
            g = s.get("hsv") or {}
            c.hsv_prob = float(g.get("prob", 0.0))
            c.hue_shift_limit = float(g.get("hue_shift_limit", 0.0))
            c.sat_shift_limit = float(g.get("sat_shift_limit", 0.0))
            c.val_shift_limit = float(g.get("val_shift_limit", 0.0))
            g = s.get("clahe_equalize") or {}
            c.clahe_prob = float(g.get("clahe_prob", 0.0))
            c.clahe_clip_limit = float(g.get("clahe_clip_limit", 1.0))
            c.clahe_tile_grid = tuple(int(v) for v in g.get("clahe_tile_grid_size", (8, 8)))
            c.equalize_prob = float(g.get("equalize_prob", 0.0))
            g = s.get("gaussian_blur") or {}
            c.gaussian_blur_prob = float(g.get("prob", 0.0))
            c.gaussian_blur_limit = _blur_limit(g.get("blur_limit", 3))
            g = s.get("motion_blur") or {}
            c.motion_blur_prob = float(g.get("prob", 0.0))
            c.motion_blur_limit = _blur_limit(g.get("blur_limit", 3))
        if lighting:
            g = s.get("iso_noise") or {}
            c.iso_noise_prob = float(g.get("prob", 0.0))
            c.iso_color_shift = tuple(float(v) for v in g.get("color_shift", (0.0, 0.0)))
            c.iso_intensity = tuple(float(v) for v in g.get("intensity", (0.0, 0.0)))
            c.lighting_group_prob = float(s.get("lighting_transform_prob", 0.0))
            c.shadow_prob = float((s.get("shadow") or {}).get("prob", 0.0))
            c.sunflare_prob = float((s.get("sunflare") or {}).get("prob", 0.0))
            g = s.get("fog") or {}
            c.fog_prob = float(g.get("prob", 0.0))
            c.fog_coef = (float(g.get("fog_coef_lower", 0.0)), float(g.get("fog_coef_upper", 0.0)))
            c.fog_alpha_coef = float(g.get("alpha_coef", 0.0))
        return c


def identity_params(n):
    """fp32 [n, 24]: the record that returns the batch unchanged."""
    p = torch.zeros(n, PARAMS_PER_SAMPLE, dtype=torch.float32)
    p[:, 0] = p[:, 4] = p[:, 8] = 1.0
    p[:, P_ALPHA] = 1.0
    return p


def validate_params(params, H, W):
    """Refuse a record the kernel would treat as "everything outside": every value must be
    finite and den = h6 x + h7 y + h8 positive at the four corners of the output (it is linear in
    (x, y), so it is then positive on every pixel)."""
    p = _record_array(params, "params", PARAMS_PER_SAMPLE, "augmentation record")
    for x, y in ((0.0, 0.0), (W, 0.0), (0.0, H), (W, H)):
        den = p[:, 6] * x + p[:, 7] * y + p[:, 8]
        if not (den > 0).all():
            raise ValueError("augmentation record has den <= 0 at an output corner "
                             f"(sample {int(np.argmin(den))})")


def pack_rng(rng):
    """int32 [n, 4] holding the bits of the uint32 words the kernel reads (`sample_params` keeps
    them as int64 in 0 .. 2^32 - 1, which every torch build can store)."""
    a = rng.detach().cpu().numpy() if torch.is_tensor(rng) else np.asarray(rng)
    if a.ndim != 2 or a.shape[1] != 4 or (a < 0).any() or (a > 0xFFFFFFFF).any():
        raise ValueError("rng must be [n, 4] with values in 0 .. 2^32 - 1")
    return torch.from_numpy(a.astype(np.uint32).view(np.int32).copy())


def _rect_to_quad(W, H, quad):
    """[m, 3, 3]: the homography that takes the corners (0,0), (W,0), (W,H), (0,H) of the
    rectangle to quad [m, 4, 2], with the last entry 1."""
    m = quad.shape[0]
    src = np.array([[0.0, 0.0], [W, 0.0], [W, H], [0.0, H]])
    A = np.zeros((m, 8, 8))
    b = np.zeros((m, 8))
    for k in range(4):
        x, y = src[k]
        u, v = quad[:, k, 0], quad[:, k, 1]
        A[:, 2 * k, 0:3] = (x, y, 1.0)
        A[:, 2 * k, 6] = -u * x
        A[:, 2 * k, 7] = -u * y
        A[:, 2 * k + 1, 3:6] = (x, y, 1.0)
        A[:, 2 * k + 1, 6] = -v * x
        A[:, 2 * k + 1, 7] = -v * y
        b[:, 2 * k] = u
        b[:, 2 * k + 1] = v
    h = np.linalg.solve(A, b[..., None])[..., 0]
    return np.concatenate([h, np.ones((m, 1))], axis=1).reshape(m, 3, 3)


def _fields(cfg, n, which):
    """`cfg` and `which` of a sampler, resolved once -> (f, cfgs, sel): f(name) is the field `name`
    per sample (fp64 [n] or [n, k]), cfgs the configurations, sel [n] the index of sample i's."""
    cfgs = [cfg] if isinstance(cfg, AugmentConfig) else list(cfg)
    if which is None:
        if len(cfgs) != 1:
            raise ValueError("several configurations need `which`")
        sel = np.zeros(n, dtype=np.int64)
    else:
        sel = np.asarray(torch.as_tensor(which).cpu().numpy(), dtype=np.int64).reshape(-1)
        if sel.shape[0] != n or (sel < 0).any() or (sel >= len(cfgs)).any():
            raise ValueError("`which` must hold n indices into the configurations")

    def f(name):
        return np.asarray([getattr(c, name) for c in cfgs], dtype=np.float64)[sel]
    return f, cfgs, sel


def _one_of(group, u, probs):
    """OneOf: where the group's draw `group` fired, one member by its probability (`probs`, an
    fp64 [n] array per member) normalised over the members, picked by the uniform `u`.  Yields a
    boolean [n] mask per member, each computed when it is asked for: u * total is held against
    the running sums, accumulated left to right; the last member takes what is left."""
    sums = list(itertools.accumulate(probs))
    left = np.asarray(group, dtype=bool) & (sums[-1] > 0)
    pick = u * sums[-1]
    for s in sums[:-1]:
        mask = left & (pick < s)
        yield mask
        left = left & ~mask
    yield left


def _record_array(record, kind, width, what):
    """The head of every `validate_*`: the record as fp64 [n, width], finite."""
    a = record.detach().cpu().numpy() if torch.is_tensor(record) else np.asarray(record)
    if a.ndim != 2 or a.shape[1] != width:
        raise ValueError(f"{kind} must be [n, {width}]")
    if not np.isfinite(a).all():
        raise ValueError(f"{what} holds a non-finite value")
    return a.astype(np.float64)


def sample_params(cfg, n, H, W, generator, which=None, return_applied=False,
                  return_groups=False):
    """Draw n records: (params fp32 [n, 24], rng int64 [n, 4] with values in 0 .. 2^32 - 1), both
    on the CPU.  `cfg` is an AugmentConfig, or a sequence of them with `which[i]` selecting the
    configuration of sample i (the reference's cat / dog split).  `generator` is a CPU
    torch.Generator; the same generator state gives the same records.  The records are validated
    (`validate_params`) before they are returned.  With `return_applied` a dict of boolean [n]
    arrays (which transform fired for which sample) comes third; with `return_groups` a dict of the
    raw draws of the three photometric groups ("color", "gray", "noise": the group probability
    fired, whatever its members' probabilities) comes last, for `sample_post`."""
    f, _, _ = _fields(cfg, n, which)
    U = torch.rand(n, 40, dtype=torch.float64, generator=generator).numpy()
    Z = torch.randn(n, 8, dtype=torch.float64, generator=generator).numpy()
    seeds = torch.randint(0, 1 << 32, (n, 2), dtype=torch.int64, generator=generator).numpy()
    col = iter(range(40))

    def uni(lim):       # U(lim[:, 0], lim[:, 1])
        return lim[:, 0] + (lim[:, 1] - lim[:, 0]) * U[:, next(col)]

    def fires(prob):
        return U[:, next(col)] < prob

    applied = {}
    eye = np.broadcast_to(np.eye(3), (n, 3, 3)).copy()
    Hinv = eye.copy()       # output -> source: the inverses, multiplied in the order applied
    cx, cy = W / 2.0, H / 2.0

    flip = fires(f("horizontal_flip_prob"))
    applied["flip"] = flip
    F = eye.copy()
    F[:, 0, 0], F[:, 0, 2] = -1.0, float(W)
    Hinv = np.where(flip[:, None, None], Hinv @ F, Hinv)

    ssr = fires(f("shift_scale_rotate_prob"))
    applied["shift_scale_rotate"] = ssr
    ang = np.radians(uni(f("rotate_limit")))
    sc = 1.0 + uni(f("scale_limit"))
    tx = cx + uni(f("shift_limit")) * W
    ty = cy + uni(f("shift_limit")) * H
    co, si = np.cos(ang) / sc, np.sin(ang) / sc
    S = eye.copy()      # inverse of T(c + d) R(ang) sc T(-c)
    S[:, 0, 0], S[:, 0, 1], S[:, 0, 2] = co, si, cx - (co * tx + si * ty)
    S[:, 1, 0], S[:, 1, 1], S[:, 1, 2] = -si, co, cy - (-si * tx + co * ty)
    Hinv = np.where(ssr[:, None, None], Hinv @ S, Hinv)

    crop = fires(f("crop_prob"))
    applied["crop"] = crop
    area = uni(f("crop_scale"))
    ratio = np.exp(uni(np.log(f("crop_ratio"))))
    cw = np.minimum(np.sqrt(area * ratio), 1.0) * W     # a crop larger than the image is clipped
    ch = np.minimum(np.sqrt(area / ratio), 1.0) * H
    x0 = U[:, next(col)] * (W - cw)
    y0 = U[:, next(col)] * (H - ch)
    C = eye.copy()      # inverse of "crop (x0, y0, cw, ch), resize to (W, H)"
    C[:, 0, 0], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2] = cw / W, x0, ch / H, y0
    Hinv = np.where(crop[:, None, None], Hinv @ C, Hinv)

    persp = fires(f("perspective_prob"))
    applied["perspective"] = persp
    d = np.minimum(np.abs(Z), PERSPECTIVE_CLIP) * uni(f("perspective_scale"))[:, None]
    if persp.any():
        quad = np.empty((n, 4, 2))
        quad[:, 0] = np.stack([d[:, 0] * W, d[:, 1] * H], 1)
        quad[:, 1] = np.stack([W - d[:, 2] * W, d[:, 3] * H], 1)
        quad[:, 2] = np.stack([W - d[:, 4] * W, H - d[:, 5] * H], 1)
        quad[:, 3] = np.stack([d[:, 6] * W, H - d[:, 7] * H], 1)
        Hinv[persp] = Hinv[persp] @ _rect_to_quad(float(W), float(H), quad[persp])
        # den = 1 at the centre of the output
        cen = Hinv[persp, 2, 0] * cx + Hinv[persp, 2, 1] * cy + Hinv[persp, 2, 2]
        Hinv[persp] = Hinv[persp] / cen[:, None, None]

    p = np.zeros((n, PARAMS_PER_SAMPLE), dtype=np.float64)
    p[:, 0:9] = Hinv.reshape(n, 9)
    p[:, P_ALPHA] = 1.0
    p[:, P_MASK_BORDER] = f("mask_border_value")

    drop = fires(f("dropout_prob"))
    applied["dropout"] = drop
    hh, hw = f("dropout_height"), f("dropout_width")
    dh = np.minimum(hh[:, 0] + np.floor(U[:, next(col)] * (hh[:, 1] - hh[:, 0] + 1)), H)
    dw = np.minimum(hw[:, 0] + np.floor(U[:, next(col)] * (hw[:, 1] - hw[:, 0] + 1)), W)
    dy = np.floor(U[:, next(col)] * (H - dh + 1))
    dx = np.floor(U[:, next(col)] * (W - dw + 1))
    hole = np.stack([dx, dy, dx + dw, dy + dh], 1)
    p[:, P_HOLE:P_HOLE + 4] = np.where(drop[:, None], hole, 0.0)
    p[:, P_HOLE_FILL] = f("dropout_fill")
    p[:, P_MASK_HOLE] = f("dropout_mask_fill")

    # OneOf(RandomBrightnessContrast, RGBShift)
    color_draw = fires(f("color_prob"))
    bc, rgb = _one_of(color_draw, U[:, next(col)],
                      (f("brightness_contrast_prob"), f("rgb_shift_prob")))
    applied["brightness_contrast"], applied["rgb_shift"] = bc, rgb
    alpha = 1.0 + uni(f("contrast_limit"))
    beta = uni(f("brightness_limit")) * 255.0
    p[:, P_ALPHA] = np.where(bc, alpha, 1.0)
    lim = f("rgb_shift_limit")
    for c in range(3):
        shift = (2.0 * U[:, next(col)] - 1.0) * lim[:, c]
        p[:, P_BETA + c] = np.where(bc, beta, 0.0) + np.where(rgb, shift, 0.0)

    gray_draw = fires(f("gray_group_prob"))
    gray = gray_draw & (f("to_gray_prob") > 0)
    applied["gray"] = gray
    p[:, P_GRAY] = gray

    noise_draw = fires(f("noise_group_prob"))
    gauss = noise_draw & (f("gauss_noise_prob") > 0)
    applied["gauss_noise"] = gauss
    p[:, P_SIGMA] = np.where(gauss, np.sqrt(np.maximum(uni(f("gauss_var_limit")), 0.0)), 0.0)

    sp = fires(f("salt_pepper_prob"))
    applied["salt_pepper"] = sp
    rng = np.zeros((n, 4), dtype=np.int64)
    rng[:, 0:2] = seeds
    for k, name in ((2, "pepper_p"), (3, "salt_p")):
        share = np.clip(uni(f(name)), 0.0, 1.0)
        thr = np.minimum(np.rint(share * 4294967296.0), 4294967295.0).astype(np.int64)
        rng[:, k] = np.where(sp, thr, 0)

    params = torch.from_numpy(p.astype(np.float32))
    validate_params(params, H, W)
    out = (params, torch.from_numpy(rng))
    if return_applied:
        out += (applied,)
    if return_groups:
        out += ({"color": color_draw, "gray": gray_draw, "noise": noise_draw},)
    return out


# ---- the warp record: elastic / grid / optical distortion --------------------------------------
def identity_warp(n):
    """fp32 [n, 64]: the warp record that leaves the pixel centres where they are (mode 0)."""
    return torch.zeros(n, WARP_PER_SAMPLE, dtype=torch.float32)


def gaussian_taps(sigma, radius=None):
    """(R, g fp64 [17]): radius R = min(ceil(3 sigma), 16) and the one-sided taps g[0..R] of the
    Gaussian, normalised so that the full kernel g[0] + 2 sum g[1..R] is 1; g[t] = 0 past R.
    `radius` names R instead (the blur's kernel size fixes it: R = (k - 1) / 2)."""
    sigma = float(sigma)
    if radius is not None:
        R = int(radius)
    else:
        R = min(int(math.ceil(3.0 * sigma)), MAX_RADIUS) if sigma > 0 else 0
    g = np.zeros(MAX_RADIUS + 1)
    t = np.arange(R + 1, dtype=np.float64)
    g[:R + 1] = np.exp(-t * t / (2.0 * sigma * sigma)) if R > 0 else 1.0
    g /= g[0] + 2.0 * g[1:].sum()
    return R, g


def _warp_reach(w, H, W):
    """fp64 [n]: the farthest a record can move a pixel centre of the output rectangle, in pixels
    (max norm): alpha plus the affine part's corner motion for an elastic record, 0 for a grid
    record (it maps [0, W] x [0, H] onto itself), the corner value of |f - 1| * extent for an
    optical one (both factors grow with the distance to the centre)."""
    mode = w[:, 0]
    corners = np.array([[0.0, 0.0], [W, 0.0], [0.0, H], [W, H]])
    reach = np.zeros(w.shape[0])
    for x, y in corners:
        ax = np.abs(w[:, 1] * x + w[:, 2] * y + w[:, 3] - x)
        ay = np.abs(w[:, 4] * x + w[:, 5] * y + w[:, 6] - y)
        elastic = np.maximum(ax, ay) + np.abs(w[:, W_ALPHA])
        ex, ey = x - w[:, W_CX], y - w[:, W_CY]
        r2 = (ex * w[:, W_INV_W]) ** 2 + (ey * w[:, W_INV_H]) ** 2
        f1 = np.abs(w[:, W_K] * r2 + w[:, W_K] * r2 * r2)
        optical = f1 * np.maximum(np.abs(ex), np.abs(ey))
        reach = np.maximum(reach, np.where(mode == WARP_ELASTIC, elastic,
                                           np.where(mode == WARP_OPTICAL, optical, 0.0)))
    return reach


def validate_warp(warp, params, H, W):
    """Refuse a warp record the kernels are not specified for, or one that can carry a pixel to
    where `params` has den <= 0: every value finite, the mode one of 0..3, an elastic record with
    alpha >= 0 and an integer radius in 0..16, a grid record with integer K in 1..8 per axis and
    increasing maps (a_k > 0), and den = h6 x + h7 y + h8 of `params` positive at the corners of
    the output rectangle GROWN by the record's largest possible displacement."""
    w = _record_array(warp, "warp", WARP_PER_SAMPLE, "warp record")
    p = params.detach().cpu().numpy() if torch.is_tensor(params) else np.asarray(params)
    if p.ndim != 2 or p.shape != (w.shape[0], PARAMS_PER_SAMPLE):
        raise ValueError(f"params must be [{w.shape[0]}, {PARAMS_PER_SAMPLE}]")
    p = p.astype(np.float64)
    mode = w[:, 0]
    if not np.isin(mode, (WARP_NONE, WARP_ELASTIC, WARP_GRID, WARP_OPTICAL)).all():
        raise ValueError("warp record has a mode outside 0..3")
    e = mode == WARP_ELASTIC
    rad = w[e, W_RADIUS]
    if (w[e, W_ALPHA] < 0).any() or (rad != np.rint(rad)).any() or (rad < 0).any() or \
            (rad > MAX_RADIUS).any():
        raise ValueError(f"elastic warp record needs alpha >= 0 and a radius in 0..{MAX_RADIUS}")
    for i in np.nonzero(mode == WARP_GRID)[0]:
        for k_at, a_at in ((W_KX, W_AX), (W_KY, W_AY)):
            K = w[i, k_at]
            if K != np.rint(K) or K < 1 or K > MAX_GRID_STEPS:
                raise ValueError(f"grid warp record needs 1 <= K <= {MAX_GRID_STEPS} "
                                 f"(sample {i}: {K})")
            if not (w[i, a_at:a_at + int(K)] > 0).all():
                raise ValueError(f"grid warp record is not increasing (sample {i})")
    reach = _warp_reach(w, H, W)
    for x, y in ((-reach, -reach), (W + reach, -reach), (-reach, H + reach),
                 (W + reach, H + reach)):
        den = p[:, 6] * x + p[:, 7] * y + p[:, 8]
        if not (den > 0).all():
            raise ValueError("warp record reaches den <= 0: the output rectangle grown by its "
                             f"largest displacement (sample {int(np.argmin(den))})")


def sample_warp(cfg, n, H, W, generator, which=None, return_applied=False):
    """Draw n warp records (fp32 [n, 64], on the CPU) of the group OneOf(ElasticTransform,
    GridDistortion, OpticalDistortion): the group probability is drawn first, then one member by
    its probability normalised over the three, as for the colour group.  `cfg`, `which` and
    `generator` as for `sample_params`; the draws come from a block of uniforms of their own, so
    `sample_params` is unaffected by whether this is called.  The records are NOT validated
    against a `params` here (`validate_warp`; `BatchAugment` does it).  With `return_applied` a
    dict of boolean [n] arrays comes second."""
    f, cfgs, sel = _fields(cfg, n, which)
    for c in cfgs:
        if c.distort_group_prob > 0 and c.grid_distortion_prob > 0:
            if not 1 <= int(c.grid_num_steps) <= MAX_GRID_STEPS or \
                    int(c.grid_num_steps) != c.grid_num_steps:
                raise ValueError(f"grid_num_steps must be 1..{MAX_GRID_STEPS}")
            if not 0 <= c.grid_distort_limit < 1:
                raise ValueError("grid_distort_limit must be in [0, 1): a cell of weight <= 0 "
                                 "would not be monotone")
        if min(c.elastic_alpha, c.elastic_sigma, c.elastic_alpha_affine,
               c.optical_distort_limit, c.optical_shift_limit) < 0:
            raise ValueError("the limits of the distortion group must not be negative")

    U = torch.rand(n, 32, dtype=torch.float64, generator=generator).numpy()
    S = 2.0 * U - 1.0                                   # U(-1, 1)
    elastic, grid, optical = _one_of(
        U[:, 0] < f("distort_group_prob"), U[:, 1],
        (f("elastic_prob"), f("grid_distortion_prob"), f("optical_distortion_prob")))
    applied = {"elastic": elastic, "grid_distortion": grid, "optical_distortion": optical}
    w = np.zeros((n, WARP_PER_SAMPLE), dtype=np.float64)
    w[:, 0] = np.where(elastic, WARP_ELASTIC, np.where(grid, WARP_GRID,
                                                       np.where(optical, WARP_OPTICAL, WARP_NONE)))

    # elastic: three anchors of the image, each moved by U(-alpha_affine, alpha_affine) pixels;
    # the record holds the INVERSE (moved anchors -> anchors: output -> source), solved in fp64
    if elastic.any():
        cx, cy, q = W / 2.0, H / 2.0, min(H, W) / 3.0
        src = np.array([[cx + q, cy + q], [cx + q, cy - q], [cx - q, cy - q]])
        dst = src[None] + S[:, 2:8].reshape(n, 3, 2) * f("elastic_alpha_affine")[:, None, None]
        dst = np.where(elastic[:, None, None], dst, src[None])
        M = np.concatenate([dst, np.ones((n, 3, 1))], axis=2)       # rows (x', y', 1)
        A = np.linalg.solve(M, np.broadcast_to(src, (n, 3, 2)))     # [n, 3, 2]: columns -> x, y
        w[:, W_AFFINE:W_AFFINE + 3] = np.where(elastic[:, None], A[:, :, 0], 0.0)
        w[:, W_AFFINE + 3:W_AFFINE + 6] = np.where(elastic[:, None], A[:, :, 1], 0.0)
        w[:, W_ALPHA] = np.where(elastic, f("elastic_alpha"), 0.0)
        for i in np.nonzero(elastic)[0]:
            R, g = gaussian_taps(cfgs[sel[i]].elastic_sigma)
            w[i, W_RADIUS] = R
            w[i, W_TAPS:W_TAPS + MAX_RADIUS + 1] = g

    # grid: per axis K cells of equal width in the output, cell k of weight s_k; knots
    # Y_k = size * cumsum(s) / sum(s) against X_k = size * k / K, so the map fixes 0 and the size
    if grid.any():
        K = np.where(grid, f("grid_num_steps"), 1.0)
        cell = np.arange(MAX_GRID_STEPS)[None, :]
        live = cell < K[:, None]
        for size, cols, k_at, inv_at, a_at, b_at in (
                (float(W), slice(8, 16), W_KX, W_INVCELL_X, W_AX, W_BX),
                (float(H), slice(16, 24), W_KY, W_INVCELL_Y, W_AY, W_BY)):
            s = np.where(live, 1.0 + S[:, cols] * f("grid_distort_limit")[:, None], 0.0)
            Y1 = size * (np.cumsum(s, axis=1) / s.sum(axis=1, keepdims=True))
            Y0 = np.concatenate([np.zeros((n, 1)), Y1[:, :-1]], axis=1)
            X1, X0 = size * ((cell + 1.0) / K[:, None]), size * (cell / K[:, None])
            a = np.where(live, (Y1 - Y0) / (X1 - X0), 0.0)
            b = np.where(live, Y0 - a * X0, 0.0)
            g2 = grid[:, None]
            w[:, a_at:a_at + MAX_GRID_STEPS] = np.where(g2, a, w[:, a_at:a_at + MAX_GRID_STEPS])
            w[:, b_at:b_at + MAX_GRID_STEPS] = np.where(g2, b, w[:, b_at:b_at + MAX_GRID_STEPS])
            w[:, k_at] = np.where(grid, K, w[:, k_at])
            w[:, inv_at] = np.where(grid, K / size, w[:, inv_at])

    # optical: f = 1 + k r^2 + k r^4 about a shifted centre, r in units of the image size
    w[:, W_CX] = np.where(optical, W / 2.0 + S[:, 25] * f("optical_shift_limit") * W, w[:, W_CX])
    w[:, W_CY] = np.where(optical, H / 2.0 + S[:, 26] * f("optical_shift_limit") * H, w[:, W_CY])
    w[:, W_K] = np.where(optical, S[:, 24] * f("optical_distort_limit"), w[:, W_K])
    w[:, W_INV_W] = np.where(optical, 1.0 / W, w[:, W_INV_W])
    w[:, W_INV_H] = np.where(optical, 1.0 / H, w[:, W_INV_H])

    warp = torch.from_numpy(w.astype(np.float32))
    return (warp, applied) if return_applied else warp


# ---- the post record: HSV shift, equalize / CLAHE, Gaussian / motion blur ----------------------
def identity_post(n):
    """fp32 [n, 64]: the post record that copies the image (everything off)."""
    return torch.zeros(n, POST_PER_SAMPLE, dtype=torch.float32)


def validate_post(post, H, W):
    """Refuse a post record the kernels are not specified for: every value finite, the HSV flag 0
    or 1, the histogram op and the blur mode in 0..2, a CLAHE record with clip_limit > 0 and an
    integer tile grid in 1..8 per axis that divides (H, W), a blur record with an integer radius
    in 1..4 (separable) or 1..3 (dense) below min(H, W) and taps / weights that are not negative
    and whose full sum is 1 within 1e-6."""
    q = _record_array(post, "post", POST_PER_SAMPLE, "post record")
    if not np.isin(q[:, Q_HSV], (0, 1)).all():
        raise ValueError("post record has an HSV flag other than 0 / 1")
    if not np.isin(q[:, Q_HIST], (HIST_NONE, HIST_EQUALIZE, HIST_CLAHE)).all():
        raise ValueError("post record has a histogram op outside 0..2")
    if not np.isin(q[:, Q_BLUR], (BLUR_NONE, BLUR_SEPARABLE, BLUR_DENSE)).all():
        raise ValueError("post record has a blur mode outside 0..2")
    for i in np.nonzero(q[:, Q_HIST] == HIST_CLAHE)[0]:
        for t, size in ((q[i, Q_TY], H), (q[i, Q_TX], W)):
            if t != np.rint(t) or t < 1 or t > MAX_TILE_GRID or size % int(t) != 0:
                raise ValueError(f"CLAHE tile grid must be integers in 1..{MAX_TILE_GRID} that "
                                 f"divide the shape (sample {i}: {t} on {size})")
        if not q[i, Q_CLIP] > 0:
            raise ValueError(f"CLAHE clip_limit must be positive (sample {i})")
    for i in np.nonzero(q[:, Q_BLUR] != BLUR_NONE)[0]:
        mode, R = int(q[i, Q_BLUR]), q[i, Q_RADIUS]
        if R != np.rint(R) or R < 1 or R > MAX_BLUR_RADIUS[mode]:
            raise ValueError(f"blur radius must be an integer in 1..{MAX_BLUR_RADIUS[mode]} "
                             f"(sample {i}: {R})")
        R = int(R)
        if R >= min(H, W):
            raise ValueError(f"blur radius {R} reaches across the image ({H} x {W})")
        if mode == BLUR_SEPARABLE:
            g = q[i, Q_TAPS:Q_TAPS + R + 1]
            total = g[0] + 2.0 * g[1:].sum()
        else:
            g = q[i, Q_DENSE:Q_DENSE + (2 * R + 1) ** 2]
            total = g.sum()
        if (g < 0).any():
            raise ValueError(f"blur weights must not be negative (sample {i})")
        if abs(total - 1.0) > 1e-6:
            raise ValueError(f"blur weights must sum to 1 (sample {i}: {total})")


def motion_line(k, a, b):
    """[k, k] fp64 weights of a motion-blur kernel: the line from cell a = (x, y) to cell b of the
    k x k grid, rasterised by the DDA rule: with n = max(|dx|, |dy|) (>= 1, the cells differ) the
    line has the n + 1 cells (x0 + floor(s dx / n + 0.5), y0 + floor(s dy / n + 0.5)), s = 0..n -
    one cell per step along the longer axis, so they are distinct - each of weight 1 / (n + 1).
    Row index is y (dy of the kernel), column index x."""
    (x0, y0), (x1, y1) = a, b
    dx, dy = x1 - x0, y1 - y0
    n = max(abs(dx), abs(dy))
    if n < 1:
        raise ValueError("a motion line needs two distinct cells")
    w = np.zeros((k, k))
    for s in range(n + 1):
        w[y0 + int(math.floor(s * dy / n + 0.5)), x0 + int(math.floor(s * dx / n + 0.5))] = 1.0
    return w / w.sum()


def _odd_sizes(limit, top, what):
    lo, hi = int(limit[0]), int(limit[1])
    ks = [k for k in range(max(3, lo), hi + 1) if k % 2 == 1]
    if hi > top or not ks:
        raise ValueError(f"{what} must hold an odd kernel size in 3..{top} and end at most there")
    return ks


def sample_post(cfg, n, H, W, generator, params, rng, groups, which=None, return_applied=False):
    """Draw n post records for a batch whose (params, rng) `sample_params` drew with
    `return_groups=True` -> (params, rng, post fp32 [n, 64]), on the CPU; params and rng are new
    tensors.  Each of the three photometric groups keeps the reference's OneOf structure over ALL
    members supported now: where the group's probability fired (`groups`), the sample goes to a
    new member with the new members' share of the group's probability mass -
        colour: HueSaturationValue against RandomBrightnessContrast + RGBShift,
        gray:   CLAHE + Equalize against ToGray,
        noise:  GaussianBlur + MotionBlur against GaussNoise -
    and the old member's fields in `params` are reset (alpha = 1 and beta = 0; gray 0; sigma 0), so
    the two never both act on a sample; otherwise the old member stands as `sample_params` drew
    it.  rng is returned as it came (salt / pepper stays where it is).  The draws come from a
    block of uniforms of their own.  With `return_applied` a dict of boolean [n] arrays comes
    last."""
    f, cfgs, sel = _fields(cfg, n, which)
    sizes = []
    for c in cfgs:
        sizes.append((
            _odd_sizes(c.gaussian_blur_limit, 9, "gaussian_blur_limit")
            if c.gaussian_blur_prob > 0 else [3],
            _odd_sizes(c.motion_blur_limit, 7, "motion_blur_limit")
            if c.motion_blur_prob > 0 else [3]))
        if min(c.hue_shift_limit, c.sat_shift_limit, c.val_shift_limit) < 0:
            raise ValueError("the HSV shift limits must not be negative")
        if c.clahe_prob > 0 and not c.clahe_clip_limit >= 1:
            raise ValueError("clahe_clip_limit must be at least 1 (the clip limit is drawn from "
                             "U(1, clahe_clip_limit))")

    U = torch.rand(n, 16, dtype=torch.float64, generator=generator).numpy()
    p = params.detach().cpu().numpy().astype(np.float64)      # a copy: params is not written
    q = np.zeros((n, POST_PER_SAMPLE), dtype=np.float64)

    # per group: the new members against the old ones, then one of the new members
    hsv = next(_one_of(groups["color"], U[:, 0],
                       (f("hsv_prob"), f("brightness_contrast_prob") + f("rgb_shift_prob"))))
    p[hsv, P_ALPHA] = 1.0
    p[hsv, P_BETA:P_BETA + 3] = 0.0
    q[:, Q_HSV] = hsv
    for k, name in ((Q_DH, "hue_shift_limit"), (Q_DS, "sat_shift_limit"),
                    (Q_DV, "val_shift_limit")):
        q[:, k] = np.where(hsv, (2.0 * U[:, k] - 1.0) * f(name), 0.0)

    pc, pe = f("clahe_prob"), f("equalize_prob")
    hist = next(_one_of(groups["gray"], U[:, 4], (pc + pe, f("to_gray_prob"))))
    clahe, equalize = _one_of(hist, U[:, 5], (pc, pe))
    p[hist, P_GRAY] = 0.0
    q[:, Q_HIST] = np.where(clahe, HIST_CLAHE, np.where(equalize, HIST_EQUALIZE, HIST_NONE))
    q[:, Q_CLIP] = np.where(clahe, 1.0 + (f("clahe_clip_limit") - 1.0) * U[:, 6], 0.0)
    grid = f("clahe_tile_grid")
    q[:, Q_TY] = np.where(clahe, grid[:, 0], 0.0)
    q[:, Q_TX] = np.where(clahe, grid[:, 1], 0.0)

    pg, pm = f("gaussian_blur_prob"), f("motion_blur_prob")
    blur = next(_one_of(groups["noise"], U[:, 7], (pg + pm, f("gauss_noise_prob"))))
    gaussian, motion = _one_of(blur, U[:, 8], (pg, pm))
    p[blur, P_SIGMA] = 0.0
    for i in np.nonzero(gaussian)[0]:
        ks = sizes[sel[i]][0]
        k = ks[min(int(U[i, 9] * len(ks)), len(ks) - 1)]
        R, g = gaussian_taps(0.3 * ((k - 1) * 0.5 - 1.0) + 0.8, radius=(k - 1) // 2)
        q[i, Q_BLUR], q[i, Q_RADIUS] = BLUR_SEPARABLE, R
        q[i, Q_TAPS:Q_TAPS + R + 1] = g[:R + 1]
    for i in np.nonzero(motion)[0]:
        ks = sizes[sel[i]][1]
        k = ks[min(int(U[i, 9] * len(ks)), len(ks) - 1)]
        a = min(int(U[i, 10] * k * k), k * k - 1)
        b = min(int(U[i, 11] * (k * k - 1)), k * k - 2)
        b += b >= a                                     # two distinct cells
        w = motion_line(k, (a % k, a // k), (b % k, b // k))
        q[i, Q_BLUR], q[i, Q_RADIUS] = BLUR_DENSE, (k - 1) // 2
        q[i, Q_DENSE:Q_DENSE + k * k] = w.reshape(-1)

    out = (torch.from_numpy(p.astype(np.float32)), rng, torch.from_numpy(q.astype(np.float32)))
    if return_applied:
        out += ({"hsv": hsv, "clahe": clahe, "equalize": equalize, "gaussian_blur": gaussian,
                 "motion_blur": motion},)
    return out


# ---- the light record: ISO noise, shadow / sun flare / fog --------------------------------------
def identity_light(n):
    """fp32 [n, 272]: the light record that copies the image (everything off)."""
    return torch.zeros(n, LIGHT_PER_SAMPLE, dtype=torch.float32)


def validate_light(light, H, W):
    """Refuse a light record the kernels are not specified for: every value finite, the ISO flag
    0 or 1 with sigma_h >= 0 and 0 <= intensity <= 1, the mode in 0..3, an integer count in 1..2
    (shadow), 0..10 (flare) or 0..128 (fog), integer flare steps T in 2..40 and an integer fog box
    k in 1..9 with k - 1 - k // 2 < min(H, W), radii that are not negative (the source's at least
    1), blend weights a in [0, 1] and flare colours in 0..255."""
    q = _record_array(light, "light", LIGHT_PER_SAMPLE, "light record")
    if not np.isin(q[:, L_ISO], (0, 1)).all():
        raise ValueError("light record has an ISO flag other than 0 / 1")
    iso = q[:, L_ISO] == 1
    if (q[iso, L_SIGMA_H] < 0).any() or (q[iso, L_INTENSITY] < 0).any() or \
            (q[iso, L_INTENSITY] > 1).any():
        raise ValueError("ISO noise needs sigma_h >= 0 and an intensity in [0, 1]")
    if not np.isin(q[:, L_MODE], (LIGHT_NONE, LIGHT_SHADOW, LIGHT_FLARE, LIGHT_FOG)).all():
        raise ValueError("light record has a mode outside 0..3")

    def whole(v, lo, hi, what, i):
        if v != np.rint(v) or v < lo or v > hi:
            raise ValueError(f"{what} must be an integer in {lo}..{hi} (sample {i}: {v})")
        return int(v)

    for i in np.nonzero(q[:, L_MODE] != LIGHT_NONE)[0]:
        mode = int(q[i, L_MODE])
        if mode == LIGHT_SHADOW:
            whole(q[i, L_COUNT], 1, MAX_POLYGONS, "the shadow's polygon count", i)
        elif mode == LIGHT_FLARE:
            n = whole(q[i, L_COUNT], 0, MAX_FLARE_CIRCLES, "the flare's circle count", i)
            whole(q[i, L_STEPS], 2, MAX_FLARE_STEPS, "the flare's step count T", i)
            if q[i, L_SRC_RADIUS] < 1:
                raise ValueError(f"the flare's source radius must be at least 1 (sample {i})")
            c = q[i, L_BODY:L_BODY + 7 * n].reshape(n, 7)
            if (c[:, 2] < 0).any():
                raise ValueError(f"a flare circle has a negative radius (sample {i})")
            if (c[:, 3] < 0).any() or (c[:, 3] > 1).any():
                raise ValueError(f"a flare circle's a must be in [0, 1] (sample {i})")
            if (c[:, 4:] < 0).any() or (c[:, 4:] > 255).any():
                raise ValueError(f"a flare circle's colour must be in 0..255 (sample {i})")
        else:
            whole(q[i, L_COUNT], 0, MAX_FOG_POINTS, "the fog's point count", i)
            k = whole(q[i, L_FOG_BOX], 1, MAX_FOG_BOX, "the fog's box size k", i)
            if k - 1 - k // 2 >= min(H, W):
                raise ValueError(f"the fog's box {k} reaches across the image ({H} x {W})")
            if q[i, L_FOG_RADIUS] < 0:
                raise ValueError(f"the fog's radius must not be negative (sample {i})")
            if not 0 <= q[i, L_FOG_ALPHA] <= 1:
                raise ValueError(f"the fog's a must be in [0, 1] (sample {i})")


def fog_points(hw, H, W, uniforms):
    """The reference library's haze-point loop: rings that grow outward from the centre, ring
    `index` holding (hw // 10) * index points, each at a uniform integer position of the ring's
    rectangle, moved by hw // 2.  `uniforms` yields the U[0, 1) numbers it consumes (two per
    point).  -> float64 [P, 2] as (x, y)"""
    pts = []
    midx, midy, index = W // 2 - 2 * hw, H // 2 - hw, 1
    while midx > -hw or midy > -hw:
        for _ in range(hw // 10 * index):
            x = midx + math.floor(next(uniforms) * (W - midx - hw - midx + 1))
            y = midy + math.floor(next(uniforms) * (H - midy - hw - midy + 1))
            pts.append((x + hw // 2, y + hw // 2))
        midy -= 3 * hw * H // (H + W)
        midx -= 3 * hw * W // (H + W)
        index += 1
    return np.asarray(pts, dtype=np.float64).reshape(-1, 2)


def fog_point_count(hw, H, W):
    """the number of points `fog_points` draws (it does not depend on the uniforms)"""
    n, midx, midy, index = 0, W // 2 - 2 * hw, H // 2 - hw, 1
    while midx > -hw or midy > -hw:
        n += hw // 10 * index
        midy -= 3 * hw * H // (H + W)
        midx -= 3 * hw * W // (H + W)
        index += 1
    return n


LIGHT_UNIFORMS = 5 + 2 * MAX_FOG_POINTS + 3     # the widest member (fog) behind the five heads


def sample_light(cfg, n, H, W, generator, which=None, return_applied=False):
    """Draw n light records (fp32 [n, 272], on the CPU): ISONoise on its own probability, then the
    group OneOf(RandomShadow, RandomSunFlare, RandomFog): the group probability first, then one
    member by its probability normalised over the three.  `cfg`, `which` and `generator` as for
    `sample_params`; the draws come from a block of uniforms of their own, drawn AFTER those of
    `sample_params`, `sample_warp` and `sample_post`, which are unaffected by whether this is
    called.  The draw rules are those of the reference's library:
        ISO     colour shift and intensity uniform over their ranges; sigma_h = shift 360 intensity
        shadow  1 or 2 polygons of five vertices at uniform integer positions of the image
        flare   centre uniform, angle 2 pi U, 6..10 circles at random points (every 10 pixels) of
                the line through the centre, radius an integer in 1..max(H // 100 - 2, 2),
                a ~ U(0.05, 0.2), channels integers in 205..255; T = src_radius // 10
        fog     coef uniform, hw = int((W // 3) coef), the haze-point loop (`fog_points`), radius
                hw // 2, a = alpha_coef coef, box k = hw // 10 (below 2: no box)
    A draw that exceeds a cap of the record (128 fog points, a box of 9) raises.  The records are
    validated (`validate_light`).  With `return_applied` a dict of boolean [n] arrays comes
    second."""
    f, cfgs, sel = _fields(cfg, n, which)
    for c in cfgs:
        if c.iso_noise_prob > 0:
            if not 0 <= min(c.iso_intensity) <= max(c.iso_intensity) <= 1:
                raise ValueError("iso_intensity must lie in [0, 1]")
            if min(c.iso_color_shift) < 0:
                raise ValueError("iso_color_shift must not be negative")
        if c.lighting_group_prob > 0 and c.sunflare_prob > 0:
            if int(c.sunflare_src_radius) != c.sunflare_src_radius or \
                    not 20 <= c.sunflare_src_radius <= 400:
                raise ValueError("sunflare_src_radius must be an integer in 20..400")
        if c.lighting_group_prob > 0 and c.fog_prob > 0:
            if not 0 <= min(c.fog_coef) <= max(c.fog_coef) <= 1 or not 0 <= c.fog_alpha_coef <= 1:
                raise ValueError("fog_coef and fog_alpha_coef must lie in [0, 1]")

    U = torch.rand(n, LIGHT_UNIFORMS, dtype=torch.float64, generator=generator).numpy()
    q = np.zeros((n, LIGHT_PER_SAMPLE), dtype=np.float64)

    iso = U[:, 0] < f("iso_noise_prob")
    cs, it = f("iso_color_shift"), f("iso_intensity")
    shift = cs[:, 0] + (cs[:, 1] - cs[:, 0]) * U[:, 1]
    intensity = it[:, 0] + (it[:, 1] - it[:, 0]) * U[:, 2]
    q[:, L_ISO] = iso
    q[:, L_SIGMA_H] = np.where(iso, shift * 360.0 * intensity, 0.0)
    q[:, L_INTENSITY] = np.where(iso, intensity, 0.0)

    shadow, flare, fog = _one_of(U[:, 3] < f("lighting_group_prob"), U[:, 4],
                                 (f("shadow_prob"), f("sunflare_prob"), f("fog_prob")))
    q[:, L_MODE] = np.where(shadow, LIGHT_SHADOW, np.where(flare, LIGHT_FLARE,
                                                           np.where(fog, LIGHT_FOG, LIGHT_NONE)))

    def whole(u, lo, hi):       # a uniform integer in lo..hi, both included
        return lo + min(int(u * (hi - lo + 1)), hi - lo)

    for i in np.nonzero(shadow)[0]:
        u = iter(U[i, 5:])
        count = whole(next(u), 1, MAX_POLYGONS)
        q[i, L_COUNT] = count
        for v in range(5 * count):
            q[i, L_BODY + 2 * v] = whole(next(u), 0, W)
            q[i, L_BODY + 2 * v + 1] = whole(next(u), 0, H)
    for i in np.nonzero(flare)[0]:
        u = iter(U[i, 5:])
        rs = int(cfgs[sel[i]].sunflare_src_radius)
        cx, cy = int(next(u) * W), int(next(u) * H)
        ang = 2.0 * math.pi * next(u)
        count = whole(next(u), 6, MAX_FLARE_CIRCLES)
        q[i, L_COUNT], q[i, L_SRC_X], q[i, L_SRC_Y] = count, cx, cy
        q[i, L_SRC_RADIUS], q[i, L_STEPS] = rs, rs // 10
        ts = range(-cx, W - cx, 10)                     # the points of the line, every 10 pixels
        for c in range(count):
            a = 0.05 + 0.15 * next(u)
            t = ts[whole(next(u), 0, len(ts) - 1)]
            rad = whole(next(u), 1, max(H // 100 - 2, 2))
            colour = [whole(next(u), 205, 255) for _ in range(3)]
            q[i, L_BODY + 7 * c:L_BODY + 7 * c + 7] = [
                int(cx + t * math.cos(ang)), int(cy + t * math.sin(ang)), rad, a] + colour
    for i in np.nonzero(fog)[0]:
        u = iter(U[i, 5:])
        lim = cfgs[sel[i]].fog_coef
        coef = lim[0] + (lim[1] - lim[0]) * next(u)
        hw = max(1, int((W // 3) * coef))
        count = fog_point_count(hw, H, W)
        if count > MAX_FOG_POINTS or hw // 10 > MAX_FOG_BOX:
            raise ValueError(f"a fog of coefficient {coef:.3f} on {H} x {W} draws {count} points "
                             f"and a box of {hw // 10}: the record holds {MAX_FOG_POINTS} points "
                             f"and a box of at most {MAX_FOG_BOX}")
        pts = fog_points(hw, H, W, u)
        q[i, L_COUNT], q[i, L_FOG_RADIUS] = count, hw // 2
        q[i, L_FOG_ALPHA] = cfgs[sel[i]].fog_alpha_coef * coef
        q[i, L_FOG_BOX] = max(hw // 10, 1)
        q[i, L_BODY:L_BODY + 2 * count] = pts.reshape(-1)

    light = torch.from_numpy(q.astype(np.float32))
    validate_light(light, H, W)
    if return_applied:
        return light, {"iso_noise": iso, "shadow": shadow, "sunflare": flare, "fog": fog}
    return light


# The record kinds a batch travels with, in the order they are copied to the device: the width and
# dtype of a row, and the record whose presence puts the kind into a ring slot (rng buffers exist
# with params whether a call names an rng or not; `gather_rng`, rng with zero salt / pepper
# thresholds, rides with post).
Record = collections.namedtuple("Record", "width dtype owner")
RECORDS = {
    "params": Record(PARAMS_PER_SAMPLE, torch.float32, "params"),
    "rng": Record(4, torch.int32, "params"),
    "warp": Record(WARP_PER_SAMPLE, torch.float32, "warp"),
    "post": Record(POST_PER_SAMPLE, torch.float32, "post"),
    "gather_rng": Record(4, torch.int32, "post"),
    "light": Record(LIGHT_PER_SAMPLE, torch.float32, "light"),
}
Staged = collections.namedtuple("Staged", "params rng warp post light gather_rng")
VALIDATE = {"warp": lambda rec, params, H, W: validate_warp(rec, params, H, W),
            "post": lambda rec, params, H, W: validate_post(rec, H, W),
            "light": lambda rec, params, H, W: validate_light(rec, H, W)}


class BatchAugment:
    """Draws the records of a batch and launches `unet_augment_u8` on the current stream.

        aug = BatchAugment(cfg, seed=0)                   # or BatchAugment([cat, dog], seed)
        image, mask = aug(images_u8, masks_u8)            # which=[0, 1, ...] with two configs
        aug(images_u8, masks_u8, out=(step.images, step.masks))   # into a GraphedTrainStep's
                                                          # static buffers: its __call__ then
                                                          # skips the copy (same data_ptr)

    `params=(params, rng)` (CPU tensors as `sample_params` returns them; `rng` may be None: then
    all noise is off) replaces the draw.  The records travel through a ring of two pinned host
    buffers with non_blocking copies; an event per buffer keeps it from being rewritten while
    its copy is in flight.

    When a configuration has `distort_group_prob > 0` (or `params=(params, rng, warp)` names warp
    records), a warp record per sample is drawn after `sample_params` (`sample_warp`), validated
    against the drawn params, staged through the same ring, and two launches follow:
    `unet_elastic_field` into a field buffer kept per batch shape, then `unet_augment_warp_u8`.
    Otherwise nothing of this happens: the same draws, the same single launch.

    When a configuration has one of `hsv_prob`, `clahe_prob`, `equalize_prob`,
    `gaussian_blur_prob`, `motion_blur_prob` on (or `params=(params, rng, warp or None, post)`
    names post records), `sample_post` is drawn after `sample_params` (and `sample_warp`), the
    records are validated (`validate_post`) and staged through the same ring, the gather runs
    with ZERO salt / pepper thresholds into an intermediate image kept per batch shape, and
    `unet_augment_post_u8` writes the output, applying salt / pepper last with the same word and
    rule.  Otherwise nothing of this happens either.

    When a configuration has `iso_noise_prob > 0` or `lighting_group_prob > 0` (or
    `params=(params, rng, warp or None, post or None, light)` names light records),
    `sample_light` is drawn last, the records are validated (`validate_light`) and staged through
    the same ring, whichever stage wrote the output before writes a second intermediate image
    kept per batch shape, and `unet_augment_light_u8` writes the output.  Salt / pepper stays
    where it is (in the post stage when there is one, else in the gather), in front of ISO
    noise as in the reference.  Otherwise nothing of this happens either."""

    def __init__(self, cfg, seed=0):
        self.cfg = cfg
        self.generator = torch.Generator()
        self.generator.manual_seed(int(seed))
        cfgs = [cfg] if isinstance(cfg, AugmentConfig) else list(cfg)
        self.distortion = any(c.distort_group_prob > 0 for c in cfgs)
        self.photometric = any(max(c.hsv_prob, c.clahe_prob, c.equalize_prob,
                                   c.gaussian_blur_prob, c.motion_blur_prob) > 0 for c in cfgs)
        self.lighting = any(max(c.iso_noise_prob, c.lighting_group_prob) > 0 for c in cfgs)
        self._ring = None       # {"n", "device", "kinds", "next", "slots": two of them}
        self._scratch = {}      # (kind, N, H, W, device): "field", "post", "light"

    def _stage(self, params, rng, device, warp=None, post=None, light=None):
        """-> Staged: the device copy of every record given (None for one that is not).
        `gather_rng` is rng with zero salt / pepper thresholds, for the gather in front of the
        post stage."""
        n = params.shape[0]
        host = {"params": params, "rng": pack_rng(rng) if rng is not None else None,
                "warp": warp, "post": post, "gather_rng": None, "light": light}     # as RECORDS
        if post is not None and rng is not None:
            host["gather_rng"] = host["rng"].clone()
            host["gather_rng"][:, 2:] = 0
        ring = self._ring
        if ring is None or ring["n"] != n or ring["device"] != device or \
                any(rec is not None and k not in ring["kinds"] for k, rec in host.items()):
            kinds = {k for k, rec in RECORDS.items() if host[rec.owner] is not None}
            ring = self._ring = {
                "n": n, "device": device, "kinds": kinds, "next": 0,
                "slots": [{"event": None,
                           "host": {k: torch.empty((n, RECORDS[k].width), dtype=RECORDS[k].dtype,
                                                   pin_memory=True) for k in kinds},
                           "device": {k: torch.empty((n, RECORDS[k].width),
                                                     dtype=RECORDS[k].dtype, device=device)
                                      for k in kinds}} for _ in range(2)]}
        slot = ring["slots"][ring["next"]]
        ring["next"] ^= 1
        if slot["event"] is not None:
            slot["event"].synchronize()         # the copy out of this host buffer has finished
        staged = dict.fromkeys(RECORDS)
        for k, rec in host.items():
            if rec is not None:
                slot["host"][k].copy_(rec)
                staged[k] = slot["device"][k].copy_(slot["host"][k], non_blocking=True)
        slot["event"] = torch.cuda.Event()
        slot["event"].record()
        return Staged(**staged)

    def _scratch_for(self, kind, N, H, W, device):
        """The scratch tensors of a stage, kept per batch shape: the displacement field ("field"),
        or (the intermediate image the stage reads, its workspace) ("post", "light")."""
        key = (kind, N, H, W, device)
        if key not in self._scratch:
            if kind == "field":     # zeros: the field kernel does not write non-elastic samples
                self._scratch[key] = torch.zeros((N, H, W, 2), dtype=torch.float32,
                                                 device=device)
            else:
                need = ops.lib().unet_augment_post_workspace_bytes(N) if kind == "post" else \
                    max(ops.lib().unet_augment_light_workspace_bytes(N), 16)
                self._scratch[key] = (torch.empty((N, H, W, 3), dtype=torch.uint8, device=device),
                                      torch.empty(need, dtype=torch.uint8, device=device))
        return self._scratch[key]

    def __call__(self, images_u8, masks_u8=None, which=None, out=None, params=None):
        if not torch.is_tensor(images_u8) or not images_u8.is_cuda:
            raise RuntimeError("unet-implementations_amd.BatchAugment runs on MI355X only "
                               "(no CPU fallback exists)")
        N, H, W, _ = images_u8.shape
        w = q = lt = None
        if params is None:
            if self.photometric:
                p, r, groups = sample_params(self.cfg, N, H, W, self.generator, which=which,
                                             return_groups=True)
            else:
                p, r = sample_params(self.cfg, N, H, W, self.generator, which=which)
            if self.distortion:
                w = sample_warp(self.cfg, N, H, W, self.generator, which=which)
            if self.photometric:
                p, r, q = sample_post(self.cfg, N, H, W, self.generator, p, r, groups,
                                      which=which)
            if self.lighting:
                lt = sample_light(self.cfg, N, H, W, self.generator, which=which)
        else:
            p, r, w, q, lt = (tuple(params) + (None, None, None, None))[:5] \
                if isinstance(params, (tuple, list)) else (params, None, None, None, None)
            if tuple(p.shape) != (N, PARAMS_PER_SAMPLE):
                raise ValueError(f"params must be [{N}, {PARAMS_PER_SAMPLE}]")
            validate_params(p, H, W)
        optional = {"warp": w, "post": q, "light": lt}
        for kind, rec in optional.items():
            if rec is not None:
                if tuple(rec.shape) != (N, RECORDS[kind].width):
                    raise ValueError(f"{kind} must be [{N}, {RECORDS[kind].width}]")
                VALIDATE[kind](rec, p, H, W)
                optional[kind] = rec.to(torch.float32)
        s = self._stage(p.to(torch.float32), r, images_u8.device, **optional)

        # The chain: the gather (behind the field kernel with a warp record), then the post and
        # the light stage where their records are there.  A stage writes the intermediate image
        # of the stage behind it, the last one the caller's; the mask is the gather's business
        # alone.  In front of a post stage the gather runs with salt / pepper off: the post
        # stage applies it last, with the same word and rule.
        dev = images_u8.device
        later = [kind for kind in ("post", "light") if getattr(s, kind) is not None]
        scratch = {kind: self._scratch_for(kind, N, H, W, dev) for kind in later}
        gather_out = out
        if later:
            image_out, mask_out = out if out is not None else (None, None)
            if masks_u8 is not None and mask_out is None:
                mask_out = torch.empty_like(masks_u8)
            gather_out = (scratch[later[0]][0], mask_out)
        gather_rng = s.rng if s.post is None else s.gather_rng
        if s.warp is None:
            image, mask = ops.augment_u8(images_u8, masks_u8, s.params, gather_rng,
                                         out=gather_out)
        else:
            field = self._scratch_for("field", N, H, W, dev)
            ops.elastic_field(s.warp, s.rng, (H, W), out=field)
            image, mask = ops.augment_warp_u8(images_u8, masks_u8, s.params, gather_rng, s.warp,
                                              field, out=gather_out)
        for kind, behind in zip(later, later[1:] + [None]):
            stage = ops.augment_post_u8 if kind == "post" else ops.augment_light_u8
            image = stage(image, getattr(s, kind), s.rng, workspace=scratch[kind][1],
                          out=image_out if behind is None else scratch[behind][0])
        return image, mask
