"""float64 references of SimpleLoss and of the Nesterov SGD step, and the case tables of
tests/test_loss_fp64_gpu.py.  tests/test_loss_refs_cpu.py checks, without a GPU, the references
against the fp32 oracle and torch.optim.SGD, and that every scalar argument of a case moves the
reference by at least 10x the bound the GPU test holds the kernels to.  Loaded by path like
fp64_layer_refs.py.  Nothing here calls the library; everything runs on the CPU.

simple_loss64 mirrors Our_UNet/models/losses.py as oracle.unet_ref.simple_loss does (class count
0 -> 1, class weights renormalised to sum 3, Dice over valid pixels only, fixed_weights=None with
dynamic=False = unweighted) in double on the fp32 logits widened to double.  One rule goes beyond
the oracle's domain: a pixel that is not ignored and whose label is none of the 3 classes (a 255
of a uint8 mask under another ignore_index - F.cross_entropy refuses such a target) is a valid
pixel of no class: it counts in the valid total and in Dice's probability sums and has no
cross-entropy term."""
import collections
import zlib

import torch
import torch.nn.functional as F

from oracle import unet_ref as O

Loss64 = collections.namedtuple("Loss64", "loss ce dice class_weights dlogits")


def class_weights64(target, ignore_index):
    valid = target != ignore_index
    total = valid.sum().double()
    counts = torch.stack([((target == c) & valid).sum().double() for c in range(3)])
    counts = torch.where(counts == 0, torch.ones_like(counts), counts)
    w = total / counts
    return w * (3.0 / w.sum())


def simple_loss64(logits_f32, target, *, w_dice, w_ce, smooth, ignore_index, dynamic,
                  fixed_weights, grad_scale=1, upstream=1, n_global=None, global_target=None):
    """-> Loss64 in double; dlogits = grad_scale * upstream * dL/dlogits by autograd in double.
    n_global / global_target: `logits_f32`, `target` are one shard of a concatenated batch of
    n_global images with the labels global_target; class weights, the cross-entropy denominator
    and Dice's mean are the batch's, dlogits is the shard's slice of the batch's gradient, and
    loss / ce / dice are the shard's ADDITIVE part of the batch's values (their sum over the shards
    is the batch's loss)."""
    assert logits_f32.dtype == torch.float32 and logits_f32.shape[1] == 3
    target = target.long()
    gt = target if global_target is None else global_target.long()
    ng = logits_f32.shape[0] if n_global is None else n_global
    z = logits_f32.double().clone().requires_grad_(True)
    if dynamic:
        w = class_weights64(gt, ignore_index)
    elif fixed_weights is None:
        w = torch.ones(3, dtype=torch.double)
    else:
        w = torch.as_tensor(fixed_weights).double()
    valid = target != ignore_index
    logp = F.log_softmax(z, dim=1)
    p = logp.exp()
    n = z.shape[0]
    num, den, dsum = 0.0, 0.0, 0.0
    for c in range(3):
        hot = ((target == c) & valid).double()
        num = num + w[c] * (-(logp[:, c] * hot).sum())
        den = den + w[c] * ((gt == c) & (gt != ignore_index)).sum().double()
        inter = (p[:, c] * hot).reshape(n, -1).sum(1)
        union = (p[:, c] * valid.double()).reshape(n, -1).sum(1) + hot.reshape(n, -1).sum(1)
        dsum = dsum + (1.0 - (2.0 * inter + smooth) / (union + smooth)).sum()
    ce = num / den
    dice = dsum / (3.0 * ng)
    loss = w_ce * ce + w_dice * dice
    (g,) = torch.autograd.grad(loss, z)
    return Loss64(loss.detach(), ce.detach(), dice.detach(), w, g * (float(grad_scale) * float(upstream)))


def sgd_nesterov64(p, g, buf, lr, mu, wd, first, grad_scale):
    """One step of optim.SGD(nesterov=True, dampening=0) in double on g * grad_scale -> (p, buf);
    first: the momentum buffer is created from the gradient (its contents are not read)."""
    p, g = p.double(), g.double() * grad_scale + p.double() * wd
    buf = g.clone() if first else buf.double() * mu + g
    return p - lr * (g + mu * buf), buf


# --------------------------------------------------------------------------- bounds
# The floor: what tests/test_kernels_gpu.py::test_loss_vs_oracle holds against the fp32 oracle.
FLOOR = dict(loss=2e-6, weights=1e-6, dlogits=2e-5)
TOL_SGD = 1e-6          # tests/test_kernels_gpu.py::test_sgd_golden, relative to max |.|


def rel(got, ref):
    return abs(float(got) - float(ref)) / abs(float(ref))


def of_max(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    scale = ref.abs().max().item()
    err = (got - ref).abs().max().item()
    return err / scale if scale > 0 else err


def errors(loss, ce, dice, weights, dlogits, ref):
    """The figures every comparison of the loss uses: loss, ce, dice relative; class weights and
    dlogits relative to the reference's largest magnitude."""
    return dict(loss=rel(loss, ref.loss), ce=rel(ce, ref.ce), dice=rel(dice, ref.dice),
                weights=of_max(weights, ref.class_weights), dlogits=of_max(dlogits, ref.dlogits))


BOUND_KEY = dict(loss="loss", ce="loss", dice="loss", weights="weights", dlogits="dlogits")


# --------------------------------------------------------------------------- loss cases
# shape (N, H, W); weights: "dynamic", "static" (STATIC) or "none" (dynamic off, no weights);
# logits: normal = N(0, 2), saturated = N(0, 2) * 30, offset = N(0, 2) + 1e3, equal = the three
# planes equal; targets: ring (random labels, the first two rows and the last column ignored
# where the image has them to spare), all_valid, absent_class (no pixel of class 2 in the batch),
# absent_in_one (image 0 has no pixel of class 1), image_ignored (the last image all ignored),
# one_pixel (every pixel but one ignored), u8_raw (a raw uint8 mask: labels, ignore 255, and
# stray values 7 and 100 the cleaning rule turns into class 0);
# form: the calls beyond the one-call form (see tests/test_loss_fp64_gpu.py); upstream: dL/dloss
# of the grad form; hides: arguments whose alteration this case cannot show, with the reason.
STATIC = (0.2, 1.0, 3.5)
LossCase = collections.namedtuple(
    "LossCase", "shape w_dice w_ce smooth ignore tdtype grad_scale weights logits targets form "
    "upstream hides",
    defaults=(1.0, 1.0, 1e-5, 255, "i64", 1.0, "dynamic", "normal", "ring", "one", 1.0, {}))
_C = LossCase
_BIG = {"smooth": "520 x 520: 1 / (pixels of a class) is 6e-6, below 10x the loss bound"}
_ONE = {"ignore_index": "a single valid pixel: nothing to ignore"}
LOSS_CASES = {
    # ---- shapes
    "shape-1x1x1": _C((1, 1, 1), targets="all_valid", hides=_ONE),
    "shape-2x17x9": _C((2, 17, 9)),
    "shape-2x24x40": _C((2, 24, 40)),
    "shape-1x520x520": _C((1, 520, 520), hides=_BIG),
    "shape-32x8x8": _C((32, 8, 8)),
    "shape-631x4x4": _C((631, 4, 4)),
    "shape-1024x4x4": _C((1024, 4, 4)),
    "shape-1024x4x4-none": _C((1024, 4, 4), weights="none", grad_scale=0.5),
    # ---- arguments, one at a time, at the two sweep shapes
    **{f"w-{wd}-{wc}-{h}x{w}": _C((2, h, w), w_dice=wd, w_ce=wc)
       for h, w in ((17, 9), (24, 40)) for wd, wc in ((0.3, 1.7), (0.0, 1.0), (1.0, 0.0))},
    **{f"smooth-1-{h}x{w}": _C((2, h, w), smooth=1.0) for h, w in ((17, 9), (24, 40))},
    **{f"ignore-{ig}-{h}x{w}": _C((2, h, w), ignore=ig)
       for h, w in ((17, 9), (24, 40)) for ig in (7, -100)},
    **{f"u8-ignore-{ig}-{h}x{w}": _C((2, h, w), ignore=ig, tdtype="u8", targets="u8_raw", form="u8")
       for h, w in ((17, 9), (24, 40)) for ig in (255, 7)},
    **{f"gscale-{name}-{h}x{w}": _C((2, h, w), grad_scale=gs)
       for h, w in ((17, 9), (24, 40)) for name, gs in (("half", 0.5), ("third", 1.0 / 3.0))},
    **{f"weights-{wt}-{h}x{w}": _C((2, h, w), weights=wt)
       for h, w in ((17, 9), (24, 40)) for wt in ("static", "none")},
    # ---- logits
    "logits-saturated": _C((2, 24, 40), logits="saturated"),
    "logits-offset": _C((2, 24, 40), logits="offset"),
    "logits-offset-17x9": _C((2, 17, 9), logits="offset"),
    "logits-equal": _C((2, 24, 40), logits="equal"),
    # ---- targets
    "targets-absent-class": _C((2, 24, 40), targets="absent_class"),
    "targets-absent-in-one": _C((2, 24, 40), targets="absent_in_one"),
    "targets-image-ignored": _C((2, 24, 40), targets="image_ignored"),
    "targets-one-pixel": _C((2, 24, 40), targets="one_pixel"),
    # ---- forms
    "form-grad": _C((2, 24, 40), form="grad", upstream=-2.75),
    "form-grad-17x9-static": _C((2, 17, 9), form="grad", upstream=-2.75, weights="static",
                                grad_scale=0.5, smooth=1.0),
    "form-shard1": _C((2, 24, 40), form="shard1"),
    "form-shard3": _C((6, 24, 40), form="shard3"),
    # ---- crossed
    "cross-shard3-static-third": _C((6, 17, 9), form="shard3", weights="static",
                                    grad_scale=1.0 / 3.0, w_dice=0.3, w_ce=1.7),
    "cross-shard3-u8-ignore7": _C((6, 17, 9), form="shard3", ignore=7, tdtype="u8",
                                  targets="u8_raw", smooth=1.0),
    "cross-shard1-631x4x4": _C((631, 4, 4), form="shard1"),
    "cross-grad-1024x4x4": _C((1024, 4, 4), form="grad", upstream=-2.75, grad_scale=0.5),
    "cross-520-static-saturated": _C((1, 520, 520), weights="static", logits="saturated",
                                     ignore=7, hides=_BIG),
    "cross-u8-520": _C((1, 520, 520), tdtype="u8", targets="u8_raw", form="u8", hides=_BIG),
    "cross-image-ignored-ignore-100": _C((2, 17, 9), targets="image_ignored", ignore=-100,
                                         w_dice=0.3, w_ce=1.7),
}
SHARDS = (1, 2, 3)      # images per shard of a shard3 case


def case_seed(name):
    return zlib.crc32(name.encode()) % 100000


def make_loss_case(case, seed):
    """-> (logits fp32 [N, 3, H, W], target int64 or uint8 [N, H, W]) on the CPU."""
    N, H, W = case.shape
    g = torch.Generator().manual_seed(seed)
    lg = torch.randn(N, 3, H, W, generator=g) * 2.0
    if case.logits == "saturated":
        lg = lg * 30.0
    elif case.logits == "offset":
        lg = lg + 1e3
    elif case.logits == "equal":
        lg = lg[:, :1].expand(N, 3, H, W).contiguous()
    tg = torch.randint(0, 3, (N, H, W), generator=g)
    ig = case.ignore
    if case.targets in ("ring", "absent_class", "absent_in_one", "image_ignored", "u8_raw"):
        if H > 2:
            tg[:, :2, :] = ig
        if W > 1:
            tg[:, :, -1:] = ig
    if case.targets == "absent_class":
        tg[tg == 2] = 0
    elif case.targets == "absent_in_one":
        tg[0][tg[0] == 1] = 2
    elif case.targets == "image_ignored":
        tg[-1] = ig
    elif case.targets == "one_pixel":
        keep = tg[0, H // 2, W // 3].item()
        tg[:] = ig
        tg[0, H // 2, W // 3] = keep
    elif case.targets == "u8_raw":
        stray = torch.rand(N, H, W, generator=g)
        tg[tg == ig] = 255                      # the mask's own ignore label
        tg[stray < 0.05] = 7
        tg[(stray >= 0.05) & (stray < 0.08)] = 100
        tg[(stray >= 0.08) & (stray < 0.12)] = 255
    if case.tdtype == "u8":
        tg = tg.to(torch.uint8)
    return lg, tg


def clean_mask(tg_u8):
    """The dataset's rule (v > 2 and v != 255 -> 0) on a uint8 mask -> int64 labels."""
    t = tg_u8.long()
    return torch.where((t > 2) & (t != 255), torch.zeros_like(t), t)


def labels_of(case, tg):
    return clean_mask(tg) if case.tdtype == "u8" else tg


def fixed_weights_of(case):
    return torch.tensor(STATIC) if case.weights == "static" else None


def ref_kwargs(case):
    return dict(w_dice=case.w_dice, w_ce=case.w_ce, smooth=case.smooth, ignore_index=case.ignore,
                dynamic=case.weights == "dynamic", fixed_weights=fixed_weights_of(case),
                grad_scale=case.grad_scale)


def reference(case, lg, tg, **over):
    """The fp64 value and gradient of the case's whole batch (upstream = 1)."""
    return simple_loss64(lg, labels_of(case, tg), **{**ref_kwargs(case), **over})


def oracle_errors(case, lg, tg, ref):
    """The fp32 oracle's own errors against `ref` (None where the labels leave its domain: a
    non-ignored label outside 0..2)."""
    t = labels_of(case, tg)
    if bool(((t != case.ignore) & ((t < 0) | (t > 2))).any()):
        return None
    x = lg.clone().requires_grad_(True)
    kw = dict(ignore_index=case.ignore, smooth=case.smooth, dynamic_weights=case.weights == "dynamic",
              fixed_weights=fixed_weights_of(case))
    loss = O.simple_loss(x, t, case.w_dice, case.w_ce, **kw)
    (loss * case.grad_scale).backward()
    with torch.no_grad():
        ce = O.simple_loss(lg, t, 0.0, 1.0, **kw)
        dice = O.simple_loss(lg, t, 1.0, 0.0, **kw)
    w = O.class_weights(t, case.ignore) if case.weights == "dynamic" else ref.class_weights
    return errors(loss.detach(), ce, dice, w, x.grad, ref)


def bounds(case, lg, tg, ref):
    """Per quantity: max(floor, 3 x the fp32 oracle's own error against the same reference) ->
    (bounds, the oracle's errors or None)."""
    oe = oracle_errors(case, lg, tg, ref)
    out = {}
    for k, key in BOUND_KEY.items():
        out[k] = FLOOR[key] if oe is None else max(FLOOR[key], 3.0 * oe[k])
    return out, oe


# the alteration of each argument: what a kernel that ignored or mixed up the argument computes
def alterations(case):
    """-> {argument: overrides of ref_kwargs / reference()} for the arguments the case has."""
    alt = {
        "w_dice": dict(w_dice=case.w_dice + 0.5),
        "w_ce": dict(w_ce=case.w_ce + 0.5),
        "smooth": dict(smooth=1.0 if case.smooth != 1.0 else 1e-5),
        "ignore_index": dict(ignore_index=255 if case.ignore != 255 else 254),
        "grad_scale": dict(grad_scale=1.0 if case.grad_scale != 1.0 else 0.5),
    }
    if case.weights == "static":
        alt["static weights"] = dict(fixed_weights=None)
    if case.form == "grad":
        alt["upstream"] = dict(upstream=1.0)
    if case.form == "shard3":
        alt["n_global"] = dict(n_global=case.shape[0] + 1)
    return alt


def moved(alt, ref):
    """How far the altered reference lies from the reference, in the comparison's own figures."""
    return errors(alt.loss, alt.ce, alt.dice, alt.class_weights, alt.dlogits, ref)


# --------------------------------------------------------------------------- SGD cases
SGD_SIZES = (1, 2, 3, 4, 5, 1003, 4 * 256 * 4096 + 4 * 256 + 3)
SGD_ARGS = {              # (lr, mu, wd)
    "default": (0.005, 0.99, 1e-4),
    "mu0": (0.005, 0.0, 1e-4),
    "wd0": (0.005, 0.99, 0.0),
    "lr0": (0.0, 0.99, 1e-4),
}
SGD_GRAD_SCALES = (1.0, 0.5)
SGD_STEPS = 3
SGD_HIDES = {("mu0", "first"): "mu = 0: buf * 0 + g is g, the first step's value"}


def make_sgd_case(n, seed):
    """-> p0, the momentum buffer's contents before the first step (garbage the first step must
    not read), and the gradients of the SGD_STEPS steps."""
    g = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=g)
    junk = torch.randn(n, generator=g) * 3.0
    grads = [torch.randn(n, generator=g) for _ in range(SGD_STEPS)]
    return p0, junk, grads


def sgd_trajectory64(p0, junk, grads, lr, mu, wd, grad_scale, first=True):
    """[(p, buf)] after each step in double; first: step 0 is a first step."""
    p, buf, out = p0.double(), junk.double(), []
    for s, g in enumerate(grads):
        p, buf = sgd_nesterov64(p, g, buf, lr, mu, wd, first and s == 0, grad_scale)
        out.append((p, buf))
    return out


def sgd_alterations(lr, mu, wd, grad_scale):
    return {
        "lr": dict(lr=lr + 0.005),
        "mu": dict(mu=0.5 if mu != 0.5 else 0.99),
        "wd": dict(wd=wd + 1e-4),
        "grad_scale": dict(grad_scale=1.0 if grad_scale != 1.0 else 0.5),
        "first": dict(first=False),
    }
