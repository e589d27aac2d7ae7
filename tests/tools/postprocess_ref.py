"""Host reference of the mask post-processing (include/unet_hip.h, "mask post-processing"): a plain
numpy / Python union-find restatement of the definitions, the only judge of
tests/test_postprocess_gpu.py.  Nothing here is shared with the kernels.

    cc(classes, connectivity, mode, num_classes)   -> labels, areas   (uint32, like the device)
    cleanup(classes, num_classes, vote=..., ...)   -> uint8 map
    confusion_at_original_size(preds, target, dims, num_classes, ignore_index) -> int64 [B, K, K]

`cc` works on row runs: the runs of equal non-zero key in every row are found with numpy, runs of
adjacent rows that touch are united (the smaller raster index becomes the root), and a component's
label is 1 + the raster index of its root run's first pixel.

Hole filling reads "the pixel immediately left of the hole's first raster pixel".  That pixel
always exists and is foreground, for the 4-connected background (foreground connectivity 8) and
for the dual 8-connected background (foreground connectivity 4) alike: a background component
that touches no image edge has its first raster pixel at x > 0; were the left neighbour
background, it would be joined to that pixel (the left neighbour is a neighbour under both
connectivities), belong to the same hole and precede it in raster order - a contradiction.
`cleanup` asserts it.
"""
import numpy as np

MODES = ("foreground", "class", "background")
VOTES = (None, "image", "component")


def sanitize(classes, num_classes):
    """uint8 copy with every byte >= num_classes read as 0."""
    c = np.asarray(classes).astype(np.uint8).copy()
    c[c >= num_classes] = 0
    return c


def _keys(img, mode):
    if mode == "foreground":
        return (img != 0).astype(np.int64)
    if mode == "class":
        return img.astype(np.int64)
    if mode == "background":
        return (img == 0).astype(np.int64)
    raise ValueError(f"mode {mode!r}")


def _find(parent, x):
    root = x
    while parent[root] != root:
        root = parent[root]
    while parent[x] != root:
        parent[x], x = root, parent[x]
    return root


def _cc_image(img, connectivity, mode):
    H, W = img.shape
    k = _keys(img, mode)
    sel = k != 0
    change = np.ones((H, W + 1), dtype=bool)           # change[y, x]: key differs between x-1 and x
    change[:, 1:W] = k[:, 1:] != k[:, :-1]
    ys, xs = np.nonzero(sel & change[:, :W])           # run starts, raster order
    _, xe = np.nonzero(sel & change[:, 1:])            # run ends (inclusive), the same order
    xe = xe + 1
    keys = k[ys, xs]
    n = len(ys)
    parent = list(range(n))
    d = 1 if connectivity == 8 else 0
    row_first = np.searchsorted(ys, np.arange(H + 1))  # runs of row y: row_first[y]:row_first[y+1]
    ysl, xsl, xel, kl = ys.tolist(), xs.tolist(), xe.tolist(), keys.tolist()
    for y in range(1, H):
        a0, a1 = int(row_first[y - 1]), int(row_first[y])
        j0 = a0
        for b in range(a1, int(row_first[y + 1])):
            bs, be, bk = xsl[b], xel[b], kl[b]
            while j0 < a1 and xel[j0] + d <= bs:
                j0 += 1
            j = j0
            while j < a1 and xsl[j] < be + d:
                if kl[j] == bk:
                    ra, rb = _find(parent, j), _find(parent, b)
                    if ra < rb:
                        parent[rb] = ra
                    elif rb < ra:
                        parent[ra] = rb
                j += 1
    roots = np.array([_find(parent, i) for i in range(n)], dtype=np.int64)
    lengths = (xe - xs).astype(np.int64)
    first = ys.astype(np.int64) * W + xs               # raster index of each run's first pixel
    labels = np.zeros(H * W, dtype=np.uint32)
    areas = np.zeros(H * W, dtype=np.uint32)
    if n:
        run_label = (first[roots] + 1).astype(np.uint32)
        labels[np.repeat(first, lengths) + _ramp(lengths)] = np.repeat(run_label, lengths)
        np.add.at(areas, first[roots], lengths.astype(np.uint32))
    return labels.reshape(H, W), areas.reshape(H, W)


def _ramp(lengths):
    """0..l0-1, 0..l1-1, ... for the run lengths."""
    total = int(lengths.sum())
    starts = np.cumsum(lengths) - lengths
    return np.arange(total, dtype=np.int64) - np.repeat(starts, lengths)


def cc(classes, connectivity=8, mode="foreground", num_classes=32):
    """classes uint8 [B, H, W] (or [H, W]) -> (labels, areas), uint32 of the same shape."""
    if connectivity not in (4, 8):
        raise ValueError("connectivity is 4 or 8")
    c = sanitize(classes, num_classes)
    if c.ndim == 2:
        return _cc_image(c, connectivity, mode)
    out = [_cc_image(img, connectivity, mode) for img in c]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def _vote_winner(counts):
    """counts[c] for c = 0..K-1 (entry 0 unused): the class with most pixels, ties to the lower."""
    best, win = 0, 0
    for c in range(1, len(counts)):
        if counts[c] > best:
            best, win = counts[c], c
    return win


def _cleanup_image(img, K, vote, keep_largest, min_area, fill_holes, max_hole_area, connectivity):
    H, W = img.shape
    cur = img.copy()
    labels = None
    if keep_largest or min_area > 0:
        labels, areas = _cc_image(cur, connectivity, "foreground")
        flat_areas = areas.reshape(-1)
        roots = np.nonzero(flat_areas)[0]
        keep = np.zeros(H * W + 1, dtype=bool)          # indexed by label
        if len(roots):
            ok = flat_areas[roots] >= min_area
            if keep_largest:
                # the largest among ALL components, ties to the smaller label
                best = roots[np.argmax(flat_areas[roots])]      # argmax: first maximum
                ok &= roots == best
            keep[roots[ok] + 1] = True
        cur[~keep[labels]] = 0
    if vote == "image":
        win = _vote_winner(np.bincount(cur.reshape(-1), minlength=K)[:K])
        if win:
            cur[cur != 0] = win
    elif vote == "component":
        if labels is None:
            labels, _ = _cc_image(cur, connectivity, "foreground")
        flat = cur.reshape(-1)
        fg = np.nonzero(flat)[0]
        if len(fg):
            # per component, the pixels of each class; np.argmax takes the first maximum, which
            # is the lower class (the rule of _vote_winner)
            comps, which = np.unique(labels.reshape(-1)[fg], return_inverse=True)
            counts = np.bincount(which * K + flat[fg], minlength=len(comps) * K).reshape(-1, K)
            flat[fg] = (np.argmax(counts[:, 1:], axis=1) + 1).astype(np.uint8)[which]
    if fill_holes:
        dual = 4 if connectivity == 8 else 8
        blabels, bareas = _cc_image(cur, dual, "background")
        before = cur.copy()
        on_edge = set(np.concatenate([blabels[0], blabels[-1], blabels[:, 0],
                                      blabels[:, -1]]).tolist())
        fill = np.zeros(H * W + 1, dtype=np.uint8)      # indexed by label: 0 = not a hole
        for root in np.nonzero(bareas.reshape(-1))[0].tolist():
            if root + 1 in on_edge:
                continue
            if max_hole_area and int(bareas.reshape(-1)[root]) > max_hole_area:
                continue
            y0, x0 = divmod(root, W)
            assert x0 > 0 and before[y0, x0 - 1] != 0, "the left pixel of a hole is foreground"
            fill[root + 1] = before[y0, x0 - 1]
        filled = fill[blabels]
        cur[filled != 0] = filled[filled != 0]
    return cur


def cleanup(classes, num_classes, vote=None, keep_largest=False, min_area=0, fill_holes=False,
            max_hole_area=0, connectivity=8):
    """The cleanup of the header, steps 1-3 in order; uint8 [B, H, W] (or [H, W]) in and out."""
    if vote not in VOTES:
        raise ValueError(f"vote {vote!r}")
    if connectivity not in (4, 8):
        raise ValueError("connectivity is 4 or 8")
    c = sanitize(classes, num_classes)
    args = (num_classes, vote, keep_largest, min_area, fill_holes, max_hole_area, connectivity)
    if c.ndim == 2:
        return _cleanup_image(c, *args)
    return np.stack([_cleanup_image(img, *args) for img in c])


def confusion_at_original_size(preds, target, dims, num_classes, ignore_index=255,
                               nearest_source_index=None):
    """int64 [B, K, K] = [target class][predicted class] of preds (uint8 [B, H, W], a byte >= K
    read as 0) and target (int [B, H, W]), both nearest-resized to dims[b] = (orig_h, orig_w) with
    ua.train.nearest_source_index (dims None: at network size)."""
    if nearest_source_index is None:
        import unet_implementations_amd as ua
        nearest_source_index = ua.train.nearest_source_index
    preds = sanitize(preds, num_classes)
    target = np.asarray(target)
    B, H, W = preds.shape
    K = num_classes
    cm = np.zeros((B, K, K), dtype=np.int64)
    for b in range(B):
        p, t = preds[b], target[b]
        if dims is not None:
            oh, ow = int(dims[b][0]), int(dims[b][1])
            rows, cols = nearest_source_index(H, oh), nearest_source_index(W, ow)
            p, t = p[rows][:, cols], t[rows][:, cols]
        t = t.astype(np.int64).reshape(-1)
        p = p.astype(np.int64).reshape(-1)
        ok = (t != ignore_index) & (t >= 0) & (t < K)
        cm[b] = np.bincount(t[ok] * K + p[ok], minlength=K * K).reshape(K, K)
    return cm


# ---- inputs shared by the tests and tools/bench_postprocess.py -----------------------------------
def spiral(H, W):
    """uint8 [H, W]: a one-pixel-wide rectangular spiral of 1s with a one-pixel gap, starting at
    (0, 0) and winding inwards.  Under 4-connectivity it is one component whose first pixel is
    (0, 0), and its complement is one 4-connected background component."""
    m = np.zeros((H, W), dtype=np.uint8)
    y, x, d = 0, 0, 0
    m[0, 0] = 1
    while True:
        dy, dx = ((0, 1), (1, 0), (0, -1), (-1, 0))[d]
        steps = 0
        while True:
            ny, nx = y + dy, x + dx
            by, bx = ny + dy, nx + dx
            if not (0 <= ny < H and 0 <= nx < W) or m[ny, nx]:
                break
            if 0 <= by < H and 0 <= bx < W and m[by, bx]:      # keep the one-pixel gap
                break
            m[ny, nx] = 1
            y, x, steps = ny, nx, steps + 1
        if steps == 0:
            return m
        d = (d + 1) % 4


def speckled_blob(H, W, seed=0, speckle=0.1):
    """(noisy, clean) uint8 [H, W]: an elliptical blob of class 2 - `clean` - and the same blob
    speckled with class 1, pierced by three rectangular holes of areas 1, 9 and 10, beside two
    stray islands (classes 1 and 2) in the corners: what a pet prediction looks like."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    cy, cx, ry, rx = H / 2.0, W / 2.0, H * 0.36, W * 0.36
    blob = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    clean = np.where(blob, 2, 0).astype(np.uint8)
    noisy = clean.copy()
    noisy[blob & (rng.rand(H, W) < speckle)] = 1
    y0, x0 = int(cy), int(cx)
    for dy, dx, h, w in ((-6, -8, 1, 1), (-4, 3, 3, 3), (4, -5, 2, 5)):
        if 0 < y0 + dy and y0 + dy + h < H - 1 and 0 < x0 + dx and x0 + dx + w < W - 1:
            noisy[y0 + dy:y0 + dy + h, x0 + dx:x0 + dx + w] = 0
    noisy[1:3, 1:4] = 1
    noisy[H - 3:H - 1, W - 3:W - 1] = 2
    return noisy, clean
