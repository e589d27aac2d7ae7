"""References and inputs of the K-class tail (tests/test_kclass_cpu.py, tests/test_kclass_gpu.py).
Nothing here calls the library; everything runs on the CPU.

simple_loss_k is SimpleLoss written from the oracle's K-generic pieces - the arithmetic of
oracle.unet_ref.class_weights(num_classes=K), F.cross_entropy and oracle.unet_ref.dice_loss - in
the dtype it is asked for: float64 is the reference of every comparison, float32 is "the fp32
torch evaluation" whose own error against that reference sizes the bounds.  In float32 at K = 3 it
is oracle.unet_ref.simple_loss bit for bit (test_kclass_cpu.py), which is what makes the K
definitions the reference's definitions."""
import collections

import numpy as np
import torch
import torch.nn.functional as F

from oracle import unet_ref as O

LossK = collections.namedtuple("LossK", "loss ce dice class_weights dlogits")

# the floor of a bound: what tests/test_kernels_gpu.py::test_loss_vs_oracle holds
FLOOR = dict(loss=2e-6, ce=2e-6, dice=2e-6, weights=1e-6, dlogits=2e-5)


def class_weights_k(target, ignore_index, K, dtype):
    """oracle.unet_ref.class_weights(target, ignore_index, num_classes=K) with `dtype` where that
    function says float (the same operations in the same order)."""
    valid = target != ignore_index
    total = valid.sum().to(dtype)
    counts = torch.stack([((target == c) & valid).sum().to(dtype) for c in range(K)])
    counts = torch.where(counts == 0, torch.ones_like(counts), counts)
    w = total / counts
    return w * (K / w.sum())


def simple_loss_k(logits_f32, target, *, w_dice=1.0, w_ce=1.0, smooth=1e-5, ignore_index=255,
                  dynamic=True, fixed_weights=None, grad_scale=1.0, upstream=1.0,
                  dtype=torch.float64):
    """-> LossK evaluated in `dtype` on the fp32 logits; dlogits = grad_scale * upstream *
    dL/dlogits by autograd.  K = logits.shape[1]; fixed_weights=None with dynamic=False is the
    unweighted loss."""
    assert logits_f32.dtype == torch.float32
    K = logits_f32.shape[1]
    target = target.long()
    z = logits_f32.to(dtype).clone().requires_grad_(True)
    if dynamic:
        w = class_weights_k(target, ignore_index, K, dtype)
    elif fixed_weights is None:
        w = None
    else:
        w = torch.as_tensor(fixed_weights).to(dtype)
    ce = F.cross_entropy(z, target, weight=w, ignore_index=ignore_index)
    dice = O.dice_loss(z, target, ignore_index, smooth)
    loss = w_ce * ce + w_dice * dice
    (g,) = torch.autograd.grad(loss, z)
    if w is None:
        w = torch.ones(K, dtype=dtype)
    return LossK(loss.detach(), ce.detach(), dice.detach(), w,
                 g * (float(grad_scale) * float(upstream)))


def rel(got, ref):
    return abs(float(got) - float(ref)) / abs(float(ref))


def of_max(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    scale = ref.abs().max().item()
    err = (got - ref).abs().max().item()
    return err / scale if scale > 0 else err


def errors(loss, ce, dice, weights, dlogits, ref):
    """loss, ce, dice relative; class weights and dlogits relative to the reference's largest
    magnitude (the figures of tests/tools/loss_refs.py)."""
    return dict(loss=rel(loss, ref.loss), ce=rel(ce, ref.ce), dice=rel(dice, ref.dice),
                weights=of_max(weights, ref.class_weights), dlogits=of_max(dlogits, ref.dlogits))


def bounds(lg, labels, ref, **kw):
    """Per quantity max(floor, 3 x the fp32 torch evaluation's own error against `ref`) ->
    (bounds, that evaluation's errors)."""
    e32 = simple_loss_k(lg, labels, dtype=torch.float32, **kw)
    oe = errors(e32.loss, e32.ce, e32.dice, e32.class_weights, e32.dlogits, ref)
    return {k: max(FLOOR[k], 3.0 * oe[k]) for k in FLOOR}, oe


# --------------------------------------------------------------------------- loss inputs
STRAY = (200, 77)      # bytes of a raw uint8 mask that are no class for any K <= 32


def clean_mask_k(tg_u8, K, ignore_index):
    """The dataset's rule generalised: v >= K and v != ignore_index -> 0, as int64 labels."""
    t = tg_u8.long()
    return torch.where((t >= K) & (t != ignore_index), torch.zeros_like(t), t)


def make_loss_case(K, shape, kind, seed, ignore_index=255):
    """-> (logits fp32 [N, K, H, W], int64 labels [N, H, W], raw uint8 mask [N, H, W]) on the CPU.
    The first two rows and the last column are an ignored band.  kind: "missing" (no pixel of
    class K - 1 in the batch), "image_ignored" (the last image wholly ignored), "large" (logits
    of +-80).  The raw mask is the labels with ~6 % stray bytes (STRAY) the cleaning rule turns
    into class 0; the labels are that mask cleaned, so the two targets describe one problem."""
    N, H, W = shape
    g = torch.Generator().manual_seed(seed)
    lg = torch.randn(N, K, H, W, generator=g) * 2.0
    if kind == "large":
        sign = torch.where(torch.rand(N, K, H, W, generator=g) < 0.5, -1.0, 1.0)
        lg = sign * 80.0 + lg
    tg = torch.randint(0, K, (N, H, W), generator=g)
    if kind == "missing":
        tg[tg == K - 1] = 0
    stray = torch.rand(N, H, W, generator=g)
    tg[stray < 0.03] = STRAY[0]
    tg[(stray >= 0.03) & (stray < 0.06)] = STRAY[1]
    tg[:, :2, :] = ignore_index
    tg[:, :, -1:] = ignore_index
    if kind == "image_ignored":
        tg[-1] = ignore_index
    raw = tg.to(torch.uint8)
    return lg, clean_mask_k(raw, K, ignore_index), raw


def fixed_weights(K):
    return torch.linspace(0.2, 3.5, K)


# --------------------------------------------------------------------------- argmax inputs
def gapped_logits(N, K, H, W, seed, gap=1e-3):
    """fp32 logits whose top-2 gap is at least `gap` at every pixel (the maximum is raised where
    it was closer), so argmax is the same in any arithmetic."""
    g = torch.Generator().manual_seed(seed)
    lg = torch.randn(N, K, H, W, generator=g)
    top = lg.topk(2, dim=1)
    close = (top.values[:, 0] - top.values[:, 1]) < 2 * gap
    lg.scatter_add_(1, top.indices[:, :1], (close.float() * 1.0)[:, None])
    return lg


def top2_gap(lg):
    top = lg.topk(2, dim=1).values
    return (top[:, 0] - top[:, 1]).min().item()


def confusion(pred, target, K, ignore_index=255):
    """int64 [K, K] numpy, target class x predicted class, over the valid pixels."""
    pred, target = np.asarray(pred).reshape(-1), np.asarray(target).reshape(-1)
    ok = (target != ignore_index) & (target >= 0) & (target < K)
    cm = np.zeros((K, K), dtype=np.int64)
    np.add.at(cm, (target[ok], pred[ok]), 1)
    return cm


def nearest_index(in_size, out_size):
    """ATen's nearest source index in fp32: min(floor(d * (in / out)), in - 1)."""
    scale = np.float32(in_size) / np.float32(out_size)
    src = np.floor(np.arange(out_size, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(src, in_size - 1)


def resized_confusion(pred, target, dims, K, ignore_index=255):
    """Per image: both maps nearest-resized to dims[b] = (h, w), then `confusion`; a size outside
    1..16384 gives zeros."""
    out = []
    for p, t, (h, w) in zip(np.asarray(pred), np.asarray(target), dims):
        if not (1 <= h <= 16384 and 1 <= w <= 16384):
            out.append(np.zeros((K, K), dtype=np.int64))
            continue
        r, c = nearest_index(p.shape[0], h), nearest_index(p.shape[1], w)
        out.append(confusion(p[r][:, c], t[r][:, c], K, ignore_index))
    return np.stack(out)


# --------------------------------------------------------------------------- whole model
def state_dict_k(seed, K, clip_dim=None):
    """oracle.fill_state_dict with a seeded K x 32 head in place of its 3 x 32 one."""
    sd = O.fill_state_dict(seed, clip_dim=clip_dim)
    rng = np.random.Generator(np.random.PCG64(seed + 104729))
    std = np.sqrt(2.0 / K)
    sd["segmentation_output.weight"] = torch.from_numpy(
        (rng.standard_normal((K, 32, 1, 1)) * std).astype(np.float32))
    sd["segmentation_output.bias"] = torch.from_numpy(
        (rng.standard_normal(K) * 0.1).astype(np.float32))
    return sd


def batch_k(seed, n, h, w, K, ignore_index=255):
    """Images ~ N(0, 1) and labels 0..K-1 in 8 x 8 blocks with an ignored band."""
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(n, 3, h, w, generator=g)
    blocks = torch.randint(0, K, (n, h // 8, w // 8), generator=g)
    tgt = blocks.repeat_interleave(8, dim=1).repeat_interleave(8, dim=2).contiguous()
    tgt[:, :3, :] = ignore_index
    return img, tgt


def train_steps64(sd, img, tgt, masks_per_step, clip=None, lr=0.005, momentum=0.99,
                  weight_decay=1e-4):
    """The oracle's network in float64 with the K-class loss, len(masks_per_step) Nesterov steps
    -> dict(logits, grads: of step 0; losses: of every step; after: the parameters after every
    step)."""
    sd = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    names, bufs = list(sd), [None] * len(sd)
    out = dict(losses=[], after=[])
    for masks in masks_per_step:
        for v in sd.values():
            v.grad = None
        m64 = None if masks is None else [None if m is None else m.double() for m in masks]
        logits = O.unet_forward(sd, img.double(), m64,
                                clip_features=None if clip is None else clip.double())
        ce = F.cross_entropy(logits, tgt, weight=class_weights_k(tgt, 255, logits.shape[1],
                                                                 torch.float64), ignore_index=255)
        loss = ce + O.dice_loss(logits, tgt)
        loss.backward()
        if not out["losses"]:
            out["logits"] = logits.detach()
            out["grads"] = {k: sd[k].grad.detach().clone() for k in names}
        out["losses"].append(loss.item())
        O.sgd_nesterov_([sd[k] for k in names], [sd[k].grad for k in names], bufs, lr, momentum,
                        weight_decay)
        out["after"].append({k: v.detach().clone() for k, v in sd.items()})
    return out
