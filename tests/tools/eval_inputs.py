"""Seeded inputs of the test-set evaluation fixture (tests/golden/eval.npz), shared by its maker
(make_golden_eval.py) and by tests/test_eval_cpu.py / tests/test_eval_gpu.py.

Everything is built from PCG64 integers with exact arithmetic (small integers and multiples of
1/64, all representable in fp32), so a case regenerated anywhere is bit-identical to the one the
reference saw; the fixture stores a SHA-256 of every case to prove it.

A case is (name, seed, network H, W, dims, classes): one batch of len(dims) images whose original sizes
are dims[b] = (orig_h, orig_w).
  - logits: low-resolution noise up-sampled 8x so that classes form regions, plus fine noise in
    steps of 1/64 (natural ties), plus planted exact ties of two and of three classes;
  - targets: 16-pixel blocks of {0, 1, 2}, a band of 255 across the middle, and image 0 without
    class 2.  classes = 1 leaves only class 0 in logits and targets, so that the other classes'
    metrics are nan in the reference.
"""
import hashlib

import numpy as np

CASES = [
    # identity, exact 2x, a down-size in both axes, a non-integer up-size
    ("a64", 101, 64, 64, [(64, 64), (128, 128), (40, 50), (100, 150)], 3),
    # pet-like sizes, and two where the integer rule d * in / out reads another pixel
    ("b128", 102, 128, 128, [(500, 375), (333, 500), (82, 94)], 3),
    # the 512^2 batch: both sizes discriminate the fp32 rule from the integer rule
    ("c512", 103, 512, 512, [(82, 94), (110, 164)], 3),
    # W not a multiple of 4 (the scalar path) and H != W
    ("d37x50", 104, 37, 50, [(61, 83), (500, 375)], 3),
    # H != W with vector loads; one size beyond the network's in one axis only
    ("e48x80", 105, 48, 80, [(48, 80), (122, 60), (31, 166)], 3),
    # classes 1 and 2 neither predicted nor labelled: their metrics are nan
    ("f16", 106, 16, 16, [(23, 19)], 1),
]
# sizes of CASES that must discriminate the rules, as (in, out) pairs (asserted by the maker)
DISCRIMINATING = [(128, 82), (128, 94), (512, 82), (512, 94), (512, 110), (512, 164)]


def nearest_index(in_size, out_size):
    """ATen's nearest source index in fp32: min(floor(d * (in / out)), in - 1)."""
    scale = np.float32(in_size) / np.float32(out_size)
    src = np.floor(np.arange(out_size, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(src, in_size - 1)


def integer_rule_index(in_size, out_size):
    """The integer form d * in // out, which is NOT what F.interpolate computes."""
    return (np.arange(out_size, dtype=np.int64) * in_size) // out_size


def _upsample(a, f, H, W):
    return np.repeat(np.repeat(a, f, axis=-2), f, axis=-1)[..., :H, :W]


def make_case(seed, B, H, W, classes=3):
    """(logits float32 [B, 3, H, W], target int64 [B, H, W])."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ch, cw = -(-H // 8), -(-W // 8)
    coarse = rng.integers(-3, 4, size=(B, 3, ch, cw)).astype(np.int64)
    fine = rng.integers(-48, 49, size=(B, 3, H, W)).astype(np.int64)
    logits = (_upsample(coarse, 8, H, W) * 64 + fine).astype(np.float32) / np.float32(64)
    th, tw = -(-H // 16), -(-W // 16)
    target = _upsample(rng.integers(0, 3, size=(B, th, tw)).astype(np.int64), 16, H, W).copy()
    # planted ties: z0 == z1 > z2, z1 == z2 > z0, z0 == z2 > z1, and all three equal
    n = max(4, (H * W) // 16)
    pos = rng.integers(0, H * W, size=(B, n))
    kind = rng.integers(0, 4, size=(B, n))
    flat = logits.reshape(B, 3, H * W)
    patterns = np.array([[1.5, 1.5, -2.0], [-2.0, 0.25, 0.25], [0.75, -1.0, 0.75],
                         [-0.5, -0.5, -0.5]], dtype=np.float32)
    for b in range(B):
        u, first = np.unique(pos[b], return_index=True)      # a repeated position: first draw wins
        flat[b][:, u] = patterns[kind[b][first]].T
    target[0][target[0] == 2] = 0                       # image 0 has no class 2
    band = slice(max(H // 2 - 1, 0), H // 2 + 2)
    target[:, band, W // 8: W - W // 8] = 255            # a band of ignored pixels
    target[:, : max(H // 16, 1), : max(W // 16, 1)] = 255
    if classes == 1:
        logits[:, 1:] -= np.float32(100)
        target[target < 3] = 0
    return np.ascontiguousarray(logits), np.ascontiguousarray(target)


def case_digest(logits, target):
    h = hashlib.sha256()
    h.update(logits.tobytes())
    h.update(target.tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


def resized_confusion(pred, target, dims, ignore_index=255):
    """int64 [3, 3] = [target class][predicted class] of a class map and a mask (both [H, W]
    integer arrays), each nearest-resized to dims = (orig_h, orig_w): the gather form, written
    with the index rule above."""
    H, W = pred.shape
    ry, rx = nearest_index(H, dims[0]), nearest_index(W, dims[1])
    p = pred[ry][:, rx].astype(np.int64).ravel()
    t = target[ry][:, rx].astype(np.int64).ravel()
    keep = (t != ignore_index) & (t >= 0) & (t < 3)
    return np.bincount(t[keep] * 3 + p[keep], minlength=9).reshape(3, 3).astype(np.int64)
