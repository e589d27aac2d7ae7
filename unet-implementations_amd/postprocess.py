"""Cleaning a predicted class map after the argmax, on the device.

Every pet image holds exactly one animal, and the network mixes the two species inside one image
and leaves stray islands and pinholes.  The usual repair - keep the largest blob, let the image
vote for one class, fill the holes - is what `scipy.ndimage` does per image on the host after a
`preds.cpu()`; here it is `unet_mask_cleanup_u8`, a handful of launches per batch with nothing read
back, so it sits inside `evaluate_model`'s loop without bringing the host tail back.

    pp = ua.MaskCleanup.pet()                      # vote="image", keep_largest, fill_holes
    results = ua.evaluate.evaluate_model(model, loader, device, postprocess=pp)

The definitions (all integers, exact) are in include/unet_hip.h, section "mask post-processing";
`tests/tools/postprocess_ref.py` restates them in numpy.
"""
from . import ops

_VOTES = (None, "image", "component")


def connected_components(classes, connectivity=8, mode="foreground", num_classes=None):
    """(labels, areas), uint32 [B, H, W], of a uint8 class map [B, H, W] on the device.

    mode "foreground": pixels != 0, neighbours join whatever their class; "class": pixels != 0,
    neighbours join only if their bytes are equal; "background": pixels == 0.  labels is 0 on
    unselected pixels, otherwise 1 + (y0 * W + x0) for the component's first pixel in raster
    order within its image (ranking the distinct labels gives scipy.ndimage.label's numbering);
    areas holds the pixel count at that first pixel and 0 elsewhere.  A byte >= num_classes reads
    as 0; with num_classes=None every byte below 32 is a class."""
    return ops.cc_label(classes, connectivity, mode, 32 if num_classes is None else num_classes)


class MaskCleanup:
    """The settings of one cleanup, applied in this order, each step skipped when it is off:

    1. removal: foreground components (`connectivity`) with area < `min_area` become 0; with
       `keep_largest` every component but the largest becomes 0 (ties to the first in raster
       order; the largest is chosen among all components, so if it is below `min_area` the image
       ends up empty);
    2. `vote`: "image" - every foreground pixel takes the class most foreground pixels of its
       image have; "component" - every foreground component takes its own majority class; ties go
       to the lower class;
    3. `fill_holes`: background components (dual connectivity) that touch no image edge and have
       area <= `max_hole_area` (0 = any area) take the class of the pixel left of their first
       pixel.

    With everything off the call copies the map (bytes >= num_classes become 0)."""

    def __init__(self, vote=None, keep_largest=False, min_area=0, fill_holes=False,
                 max_hole_area=0, connectivity=8):
        if vote not in _VOTES:
            raise ValueError(f"vote is None, 'image' or 'component' (got {vote!r})")
        if connectivity not in (4, 8):
            raise ValueError(f"connectivity is 4 or 8 (got {connectivity!r})")
        for name, v in (("min_area", min_area), ("max_hole_area", max_hole_area)):
            if isinstance(v, bool) or not isinstance(v, int):
                raise TypeError(f"{name} is an integer pixel count (got {v!r})")
            if not 0 <= v <= 1 << 30:
                raise ValueError(f"{name} is outside 0..2^30 (got {v})")
        self.vote = vote
        self.keep_largest = bool(keep_largest)
        self.min_area = min_area
        self.fill_holes = bool(fill_holes)
        self.max_hole_area = max_hole_area
        self.connectivity = connectivity

    @classmethod
    def pet(cls):
        """The dataset's one-animal rule: one blob, one class, no holes."""
        return cls(vote="image", keep_largest=True, fill_holes=True)

    def settings(self):
        return dict(vote=self.vote, keep_largest=self.keep_largest, min_area=self.min_area,
                    fill_holes=self.fill_holes, max_hole_area=self.max_hole_area,
                    connectivity=self.connectivity)

    def __repr__(self):
        return "MaskCleanup(" + ", ".join(f"{k}={v!r}" for k, v in self.settings().items()) + ")"

    def __call__(self, classes_u8, num_classes, check=False, workspace=None):
        """A new uint8 [B, H, W] tensor; nothing is read on the host unless check=True (which
        reads the kernels' status word and raises if a bounded loop ran into its limit)."""
        return ops.mask_cleanup(classes_u8, num_classes, check=check, workspace=workspace,
                                **self.settings())


def _check_postprocess(postprocess):
    if postprocess is not None and not isinstance(postprocess, MaskCleanup):
        raise TypeError(f"postprocess is a MaskCleanup or None (got {type(postprocess).__name__})")
    return postprocess


__all__ = ["MaskCleanup", "connected_components"]
