"""GPU: no kernel writes outside the workspace its entry point was given, and none depends on
what the workspace held.

Every multi-region workspace of csrc/ is carved by the layout function that also measures it
(csrc/ws_layout.h).  Here the allocator the wrappers use (`ops._ws`) is replaced by one that hands
out the requested bytes as a view 4096 bytes into a larger buffer, both 4096-byte guards and the
workspace itself filled with 0xA5.  After the call the guards are intact and every output is
bit-equal to the same call made with the stock allocator.  The stock run is the reference, so the
file holds before and after the layouts were written once.

Shapes are the smallest that still select the multi-region forms.  The stem fold takes W % 128 ==
0 and is not selected at 64 x 64, so the fp32 step also runs at 64 x 128, the smallest size at
which the stem fold, the 32-channel fold and the head fold are all selected."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import unet_ref as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096
FILL = 0xA5


def _load(name):
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(ROOT, "tests", "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class guarded:
    """`with guarded(ops) as g:` - ops._ws hands out guarded views for the block; g.alloc(n) does
    the same for a caller-kept workspace; g.check() holds every guard handed out so far."""

    def __init__(self, ops):
        self.ops, self.bufs = ops, []

    def alloc(self, nbytes, like=None):
        n = max(int(nbytes), 16)
        buf = torch.full((n + 2 * GUARD,), FILL, dtype=torch.uint8,
                         device=like.device if like is not None else DEV)
        self.bufs.append((buf, n))
        return buf[GUARD:GUARD + n]

    def __enter__(self):
        self.stock = self.ops._ws
        self.ops._ws = self.alloc
        return self

    def __exit__(self, *exc):
        self.ops._ws = self.stock
        return False

    def check(self, at_least=1):
        torch.cuda.synchronize()
        assert len(self.bufs) >= at_least, f"{len(self.bufs)} workspaces were asked for"
        for i, (buf, n) in enumerate(self.bufs):
            assert bool((buf[:GUARD] == FILL).all()), f"workspace {i} ({n} bytes): front guard"
            assert bool((buf[GUARD + n:] == FILL).all()), f"workspace {i} ({n} bytes): back guard"


def both_ways(ua, call, at_least=1):
    """call() with the stock allocator and with the guarded one -> asserts guards and equality"""
    ref = call(None)
    torch.cuda.synchronize()
    with guarded(ua.ops) as g:
        got = call(g)
        g.check(at_least)
    assert len(ref) == len(got)
    for i, (a, b) in enumerate(zip(ref, got)):
        assert a.dtype == b.dtype and a.shape == b.shape, i
        assert torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8)), \
            f"output {i} differs"
    return ref


# --------------------------------------------------------------------------- the 64 x 64 net
def count(names, what):
    return sum(what in n for n in names)


def _step(ua, g, H, W, precision, folds=True):
    """One eager step (forward, loss, backward) of the net with the net64 fixture's weights at
    batch 2 -> ([loss, logits, every gradient], launch names)."""
    model = ua.UNet()
    model.load_state_dict(O.fill_state_dict(int(g["seed_w"])))
    model = model.to(DEV).train()
    model.matmul_precision = precision
    model.fullres_folds = model.wgrad32_folds = folds
    model.dropout_mask_override = O.draw_dropout_masks(int(g["seed_drop"]), 2)
    img, tgt = O.synthetic_batch(int(g["seed_x"]), 2, H, W)
    with ua.ops.record_launches() as rec:
        logits = model(img.to(DEV))
        loss = ua.get_loss_function()(logits, tgt.to(DEV))
        loss.backward()
    torch.cuda.synchronize()
    outs = [loss.detach().clone(), logits.detach().clone()]
    outs += [p.grad.detach().clone() for _, p in model.named_parameters()]
    return outs, rec.names


@pytest.mark.parametrize("H,W", [(64, 64), (64, 128)])
def test_fp32_train_step_with_the_folds_selected(ua, golden, H, W):
    g = golden("net64")
    names = {}

    def call(guard):
        outs, names["guarded" if guard else "stock"] = _step(ua, g, H, W, "fp32")
        return outs

    ua.ops.set_c32_winograd("always")
    try:
        both_ways(ua, call, at_least=40)
        _, plain = _step(ua, g, H, W, "fp32", folds=False)
    finally:
        ua.ops.set_c32_winograd(True)
    assert names["guarded"] == names["stock"]
    run = names["guarded"]
    # the head fold: a second head_bwd launch forms dz; the 32-channel fold runs in the Winograd
    # weight gradient; the stem fold in the raw-row stem weight gradient (W % 128 == 0).  Each
    # replaces one in_bwd_apply launch of the step without folds.
    stem = W % 128 == 0
    assert count(run, "head_bwd_kernel") == 2 and count(plain, "head_bwd_kernel") == 1
    assert count(run, "conv_wgrad_wino32_kernel") >= 2
    assert count(run, "conv_stem_wgrad_rows_kernel") == (1 if stem else 0)
    fewer = count(plain, "in_bwd_apply") - count(run, "in_bwd_apply")
    print(f"{H} x {W}: {len(run)} launches, {fewer} in_bwd_apply launches folded away")
    assert fewer >= (3 if stem else 2)


def test_bf16_train_step(ua, golden):
    g = golden("net64")
    both_ways(ua, lambda guard: _step(ua, g, 64, 64, "bf16")[0], at_least=40)


# --------------------------------------------------------------------------- Grad-CAM
def test_gradcam_calls_share_one_workspace(ua):
    N, h, C = 2, 8, 32           # HW = 64
    gen = torch.Generator().manual_seed(3)
    grad = torch.randn(N, h, h, C, generator=gen).to(DEV)
    act = torch.randn(N, h, h, C, generator=gen).to(DEV)

    def call(guard):
        ws = ua.ops.gradcam_workspace(N, h * h, C, grad)
        w = ua.ops.gradcam_weights(grad, ws)
        cam, ws2 = ua.ops.gradcam_map(act, 0.01, w, ws)
        assert ws2 is ws
        return [w, cam, ua.ops.gradcam_heatmap(cam, ws, (16, 16))]

    w, cam, heat = both_ways(ua, call)
    assert float(cam.max()) > 0 and float(heat.max()) > 0


# --------------------------------------------------------------------------- mask cleaning
def _class_maps():
    gen = np.random.default_rng(5)
    m = gen.integers(0, 3, (2, 16, 16), dtype=np.uint8)
    m[:, 4:12, 4:12] = 1
    m[:, 6:9, 6:9] = 0          # a hole
    m[0, 0:3, 0:3] = 2
    return torch.from_numpy(m).to(DEV)


def test_mask_cleanup_with_vote_and_hole_fill(ua):
    maps = _class_maps()
    for vote in ("component", "image"):
        out, = both_ways(ua, lambda guard: [ua.ops.mask_cleanup(
            maps, 3, vote=vote, keep_largest=True, min_area=2, fill_holes=True, check=True)])
        assert not torch.equal(out, maps)


def test_cc_label(ua):
    maps = _class_maps()
    for mode in ("foreground", "background"):
        labels, areas = both_ways(ua, lambda guard: list(ua.ops.cc_label(
            maps, connectivity=8, mode=mode, num_classes=3, check=True)))
        assert int(areas.view(torch.int32).max()) > 1


# --------------------------------------------------------------------------- augmentation
def test_augment_post_and_light(ua):
    P, L = _load("post_ref"), _load("light_ref")
    shape = (2, 16, 16)
    image = torch.from_numpy(P.batch(shape, "all")).to(DEV)
    # (the record tables are keyed by the shapes of their own suites: batch 0 of 16 x 24 holds
    # HSV, equalize on sample 0, CLAHE on one tile on sample 1, both blurs - all fit 16 x 16)
    post = torch.as_tensor(P.records(ua.augment, (2, 16, 24), "all")[0],
                           dtype=torch.float32).to(DEV)
    light = torch.as_tensor(L.records((3, 16, 16), "fog")[0][:2], dtype=torch.float32).to(DEV)
    rng = ua.augment.pack_rng(np.array([[11, 22, 1 << 28, 1 << 27], [33, 44, 1 << 27, 0]],
                                       dtype=np.int64)).to(DEV)
    lib = ua.lib()

    # (these two wrappers allocate for themselves: the guarded workspace is passed in)
    def post_call(guard):
        ws = guard.alloc(lib.unet_augment_post_workspace_bytes(2)) if guard else None
        return [ua.ops.augment_post_u8(image, post, rng, workspace=ws)]

    def light_call(guard):
        ws = guard.alloc(lib.unet_augment_light_workspace_bytes(2)) if guard else None
        return [ua.ops.augment_light_u8(image, light, rng, workspace=ws)]

    for call in (post_call, light_call):
        out, = both_ways(ua, call)
        assert bool((out != image).any())


# --------------------------------------------------------------------------- the loss
@pytest.mark.parametrize("K", [3, 5])
def test_dice_wce_loss(ua, K):
    gen = torch.Generator().manual_seed(K)
    logits = torch.randn(2, K, 16, 16, generator=gen).to(DEV)
    target = torch.randint(0, K, (2, 16, 16), generator=gen)
    target[0, :2] = 255
    target = target.to(DEV)

    def call(guard):
        out, dl = ua.ops.dice_wce_loss_fwd_bwd(logits, target, 1.0, 1.0, 1.0, 255, True)
        return [out[:3 + K], dl]       # {loss, ce, dice, w[0..K-1]}; at K = 3 two unused floats follow

    out, dl = both_ways(ua, call)
    assert float(out[0]) > 0 and float(dl.abs().max()) > 0
