"""The K-class tail (2..32 classes: head, loss, counts, confusion) without a GPU: the exports and
the ABI version, what the Python surface accepts and what it refuses before touching a device,
the C entry points' refusals before a launch, the references of tests/test_kclass_gpu.py against
the oracle, and the build of csrc/head.hip and csrc/loss.hip."""
import ctypes
import importlib.util
import os
import subprocess

import pytest
import torch

from oracle import unet_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location(
    "kclass_refs", os.path.join(ROOT, "tests", "tools", "kclass_refs.py"))
KR = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(KR)

EXPORTS = ("unet_dice_wce_lossk_workspace_bytes", "unet_dice_wce_lossk_fwd_bwd",
           "unet_dice_wce_lossk_fwd_bwd_u8", "unet_dice_wce_lossk_grad",
           "unet_dice_wce_lossk_grad_u8", "unet_argmax_countsk", "unet_argmax_countsk_u8",
           "unet_eval_confusionk")
UNET_E_INVALID = -1


def test_new_exports_are_present_and_the_abi_version_is_11(ua):
    handle = ctypes.CDLL(ua.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    for name in EXPORTS:
        assert hasattr(handle, name), name
        assert name + "(" in header, name
        assert hasattr(ua.lib(), name), name
    assert ua.lib().unet_abi_version() == 11
    assert "#define UNET_ABI_VERSION 11" in header


def test_unet_accepts_2_to_32_classes(ua):
    for K in (2, 5, 21, 32):
        m = ua.UNet(num_classes=K)
        m.check_supported()
        assert m.segmentation_output.out_channels == K and m.num_classes == K
    ua.CLIPUNet(num_classes=5).check_supported()


@pytest.mark.parametrize("K", [1, 33])
def test_unet_refuses_a_class_count_outside_2_to_32(ua, K):
    with pytest.raises((NotImplementedError, ValueError), match="32"):
        ua.UNet(num_classes=K).check_supported()


def test_segmentation_metrics_constructs_for_k_classes(ua):
    m = ua.SegmentationMetrics(num_classes=5)
    assert m.confusion_matrix.shape == (5, 5) and m.intersections.shape == (5,)
    cm = torch.arange(50).reshape(2, 5, 5)
    m.update_from_confusion(cm)
    s = cm.sum(0)
    assert m.confusion_matrix.tolist() == s.tolist()
    assert m.intersections.tolist() == torch.diagonal(s).double().tolist()
    assert m.total_pixels == int(s.sum())
    for K in (1, 33):
        with pytest.raises(NotImplementedError, match="32"):
            ua.SegmentationMetrics(num_classes=K)


def test_what_k_classes_do_not_cover_is_refused_without_a_device(ua):
    logits, target = torch.zeros(1, 5, 8, 8), torch.zeros(1, 8, 8, dtype=torch.int64)
    with pytest.raises(NotImplementedError, match="3 classes"):
        ua.SimpleLoss(batch_sync="global")(logits, target)
    with pytest.raises(NotImplementedError, match="3 classes"):
        ua.ops.dice_wce_loss_shard_stats(logits, target, 1e-5, 255)
    with pytest.raises(ValueError, match="32"):
        ua.SimpleLoss()(torch.zeros(1, 33, 8, 8), target)
    with pytest.raises(ValueError, match="32"):
        ua.ops.dice_wce_loss_fwd_bwd(torch.zeros(1, 33, 8, 8), target, 1e-5, 1.0, 1.0, 255, True)
    with pytest.raises(ValueError, match="32"):
        ua.ops.argmax_dice_counts(torch.zeros(1, 33, 8, 8), target)
    with pytest.raises(ValueError, match="class_weights"):
        ua.SimpleLoss(dynamic_weights=False, class_weights=[1.0, 2.0, 3.0])(logits, target)
    model = ua.UNet(num_classes=5)
    images = torch.zeros(1, 3, 64, 64)
    batch = {"image": images, "mask": torch.zeros(1, 64, 64, dtype=torch.int64)}
    with pytest.raises(NotImplementedError, match="3-class"):
        ua.evaluate.confidence_maps(model, images)
    with pytest.raises(NotImplementedError, match="3-class"):
        ua.evaluate.error_maps(model, images, batch["mask"])
    with pytest.raises(NotImplementedError, match="3-class"):
        ua.evaluate.gradcam(model, images, 1)
    with pytest.raises(NotImplementedError, match="3-class"):
        ua.unet.stage_feature_and_gradient(model, images, 1, model.decoder_stages[0])
    with pytest.raises(NotImplementedError, match="3 classes"):
        ua.ops.eval_maps(logits, target)
    for fig in (ua.render.prediction_figure, ua.render.confidence_figure, ua.render.error_figure,
                ua.render.gradcam_figure):
        with pytest.raises(NotImplementedError, match="5 classes"):
            fig(model, batch, "cpu")
    with pytest.raises(NotImplementedError, match="5 classes"):
        ua.render.figure(images, logits, None, ua.render.PREDICTION_PANELS)
    with pytest.raises(NotImplementedError, match="three-colour"):
        ua.evaluate.evaluate_model(model, [], "cpu", visualize_samples=1, output_dir="unused")
    with pytest.raises(NotImplementedError, match="trimap"):
        ua.dataprep.DeviceLetterbox([], label_lut="trimap", num_classes=5)
    # (a table of one's own is how K classes are re-encoded)
    import numpy as np
    ua.dataprep.DeviceLetterbox([], label_lut=np.arange(256, dtype=np.uint8), num_classes=5,
                                device="cpu")
    with pytest.raises(NotImplementedError):
        ua.evaluate_model_metrics(None, [], "cpu", num_classes=5)


def test_c_entry_points_refuse_before_any_launch(ua):
    """K = 33, a uint8 ignore_index below K and a batch past the documented 1024 images are
    UNET_E_INVALID; the pointers are never dereferenced (they point nowhere)."""
    L = ua.lib()
    p = 4096      # not a device address: a launch would fault, a refusal never reads it

    def loss(fn, N, K, ignore):
        return fn(p, p, p, None, p, 1 << 40, N, K, 8, 8, 1e-5, 1.0, 1.0, ignore, 1, None, 1.0, None)

    def grad(fn, N, K, ignore):
        return fn(p, p, p, 1 << 40, None, p, N, K, 8, 8, ignore, None)

    for N, K in ((2, 33), (2, 1), (1025, 5)):
        assert loss(L.unet_dice_wce_lossk_fwd_bwd, N, K, 255) == UNET_E_INVALID
        assert grad(L.unet_dice_wce_lossk_grad, N, K, 255) == UNET_E_INVALID
        assert L.unet_dice_wce_lossk_workspace_bytes(N, K, 8, 8) == 0
    for ignore in (4, 0, 256, -100):
        assert loss(L.unet_dice_wce_lossk_fwd_bwd_u8, 2, 5, ignore) == UNET_E_INVALID
        assert grad(L.unet_dice_wce_lossk_grad_u8, 2, 5, ignore) == UNET_E_INVALID
        assert L.unet_argmax_countsk_u8(p, p, p, p, 2, 5, 8, 8, ignore, None) == UNET_E_INVALID
    assert L.unet_argmax_countsk(p, p, p, p, 2, 33, 8, 8, 255, None) == UNET_E_INVALID
    assert L.unet_eval_confusionk(p, p, None, p, 2, 33, 8, 8, 255, None) == UNET_E_INVALID
    assert L.unet_eval_confusionk(p, p, None, p, 2, 5, 8, 8, 4, None) == UNET_E_INVALID
    assert L.unet_head1x1_fwd(p, p, p, p, 1, 64, 32, 33, None) == UNET_E_INVALID
    assert L.unet_head1x1_bwd(p, p, p, p, p, p, p, 1 << 40, 1, 64, 32, 33, None) == UNET_E_INVALID
    assert L.unet_dice_wce_lossk_workspace_bytes(64, 32, 512, 512) > 0     # 64 images at K = 32
    assert L.unet_dice_wce_lossk_workspace_bytes(1024, 32, 8, 8) > 0


def test_the_k_form_takes_3_classes_with_the_3_class_workspace_and_refusals(ua):
    """K = 3 through the K-form: the workspace is byte for byte the 3-class one, and what the
    3-class exports refuse - 1025 images, a uint8 ignore_index that is a class - is refused."""
    L = ua.lib()
    p = 4096
    for N in (1, 8, 1024):
        for H, W in ((8, 8), (512, 512)):
            assert L.unet_dice_wce_lossk_workspace_bytes(N, 3, H, W) == \
                L.unet_dice_wce_loss_workspace_bytes(N, H, W) > 0, (N, H, W)

    def loss(fn, N, ignore, ws=1 << 40):
        return fn(p, p, p, None, p, ws, N, 3, 8, 8, 1e-5, 1.0, 1.0, ignore, 1, None, 1.0, None)

    def grad(fn, N, ignore, ws=1 << 40):
        return fn(p, p, p, ws, None, p, N, 3, 8, 8, ignore, None)

    for sfx in ("", "_u8"):
        fwd, bwd = (getattr(L, f"unet_dice_wce_lossk_{n}{sfx}") for n in ("fwd_bwd", "grad"))
        assert loss(fwd, 1025, 255) == UNET_E_INVALID and b"bad shape" in L.unet_last_error()
        assert grad(bwd, 1025, 255) == UNET_E_INVALID and b"bad shape" in L.unet_last_error()
        # (1024 images pass the checks and stop at the workspace size, still before a launch)
        assert loss(fwd, 1024, 255, ws=16) == -3 and grad(bwd, 1024, 255, ws=16) == -3
    assert L.unet_dice_wce_lossk_workspace_bytes(1025, 3, 8, 8) == 0
    assert loss(L.unet_dice_wce_lossk_fwd_bwd_u8, 2, 2) == UNET_E_INVALID
    assert b"ignore_index in 3..255" in L.unet_last_error()
    assert grad(L.unet_dice_wce_lossk_grad_u8, 2, 2) == UNET_E_INVALID
    assert b"ignore_index in 3..255" in L.unet_last_error()
    assert L.unet_argmax_countsk_u8(p, p, p, p, 2, 3, 8, 8, 2, None) == UNET_E_INVALID
    assert b"ignore_index in 3..255" in L.unet_last_error()
    assert L.unet_eval_confusionk(p, p, None, p, 2, 3, 8, 8, 2, None) == UNET_E_INVALID


# --------------------------------------------------------------------------- the references
@pytest.mark.parametrize("dynamic", [True, False])
def test_reference_at_3_classes_is_the_oracles_simple_loss_bit_for_bit(dynamic):
    lg, labels, _ = KR.make_loss_case(3, (2, 24, 40), "missing", 11)
    fixed = None if dynamic else KR.fixed_weights(3)
    got = KR.simple_loss_k(lg, labels, w_dice=0.7, w_ce=1.3, dynamic=dynamic, fixed_weights=fixed,
                           dtype=torch.float32)
    x = lg.clone().requires_grad_(True)
    want = O.simple_loss(x, labels, 0.7, 1.3, dynamic_weights=dynamic, fixed_weights=fixed)
    want.backward()
    assert torch.equal(got.loss, want.detach()) and torch.equal(got.dlogits, x.grad)
    for K in (2, 3, 5, 32):
        _, labels, _ = KR.make_loss_case(K, (2, 24, 40), "missing", 12)
        assert torch.equal(KR.class_weights_k(labels, 255, K, torch.float32),
                           O.class_weights(labels, 255, num_classes=K))


@pytest.mark.parametrize("K", [2, 5, 21])
def test_every_argument_moves_the_reference_by_ten_bounds(K):
    """A comparison that could not see K, a class weight, smooth or ignore_index proves nothing:
    altering each moves the float64 reference by at least 10 x the bound the GPU test holds."""
    shape = (2, 17, 9)
    lg, labels, _ = KR.make_loss_case(K, shape, "image_ignored", 5)
    kw = dict(dynamic=False, fixed_weights=KR.fixed_weights(K), smooth=1.0)
    ref = KR.simple_loss_k(lg, labels, **kw)
    bound, _ = KR.bounds(lg, labels, ref, **kw)
    other = KR.fixed_weights(K).clone()
    other[K // 2] *= 1.5
    wider = torch.cat([lg, torch.zeros_like(lg[:, :1])], dim=1)       # one more class plane
    alts = {
        "K": (KR.simple_loss_k(wider, labels, **{**kw, "fixed_weights": torch.cat(
            [KR.fixed_weights(K), torch.ones(1)])}), True),
        "one class weight": (KR.simple_loss_k(lg, labels, **{**kw, "fixed_weights": other}), False),
        "smooth": (KR.simple_loss_k(lg, labels, **{**kw, "smooth": 1e-5}), False),
        # (a kernel that missed ignore_index counts the ignored band; as class 0 here, since
        # F.cross_entropy takes no label outside 0..K-1)
        "ignore_index": (KR.simple_loss_k(lg, torch.where(labels == 255, 0, labels), **kw), False),
    }
    for what, (alt, cut) in alts.items():
        dl = alt.dlogits[:, :K] if cut else alt.dlogits
        w = alt.class_weights[:K] if cut else alt.class_weights
        moved = KR.errors(alt.loss, alt.ce, alt.dice, w, dl, ref)
        seen = [k for k in moved if moved[k] >= 10 * bound[k]]
        assert seen, f"{what}: moved {moved}, bounds {bound}"
        assert "loss" in seen or "dlogits" in seen, f"{what}: {moved}"


def test_gapped_logits_and_the_confusion_reference():
    lg = KR.gapped_logits(2, 5, 9, 7, 3)
    assert KR.top2_gap(lg) >= 1e-3
    pred = lg.argmax(1).numpy()
    tgt = torch.randint(0, 5, (2, 9, 7), generator=torch.Generator().manual_seed(1))
    tgt[:, 0] = 255
    m = O.segmentation_metrics([pred], [tgt.numpy()], num_classes=5)
    cm = sum(KR.confusion(p, t, 5) for p, t in zip(pred, tgt.numpy()))
    assert cm.diagonal().tolist() == m["intersections"].tolist()
    assert cm.sum() == m["total_pixels"]
    same = KR.resized_confusion(pred, tgt.numpy(), [(9, 7), (0, 7)], 5)
    assert (same[0] == KR.confusion(pred[0], tgt[0].numpy(), 5)).all() and same[1].sum() == 0


# --------------------------------------------------------------------------- the build
TAIL_KERNELS = {
    "head": ("head_fwd_kernel", "head_bwd_kernel", "head_bwd_finalize_kernel", "headk_fwd_kernel",
             "headk_bwd_kernel", "headk_bwd_finalize_kernel"),
    "loss": ("loss_reduce_kernel", "loss_reduce_u8_kernel", "loss_finalize_kernel",
             "loss_shard_stats_kernel", "loss_shard_apply_kernel", "loss_grad_kernel",
             "loss_grad_u8_kernel", "argmax_counts_kernel", "lossk_reduce_kernel",
             "lossk_finalize_kernel", "lossk_grad_kernel", "argmax_countsk_kernel"),
}


def test_head_and_loss_kernels_use_no_scratch_and_the_hazard_check_is_clean():
    for unit, kernels in TAIL_KERNELS.items():
        obj = os.path.join(ROOT, "unet-implementations_amd", "csrc", "build", unit + ".o")
        if not os.path.exists(obj):
            pytest.skip("no built objects (run __graft_entry__.build() first)")
        regs = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_regs.sh"), obj],
                              capture_output=True, text=True, check=True).stdout
        lines = [ln for ln in regs.splitlines() if " scratch " in ln]
        names = " ".join(lines)
        for kernel in kernels:
            assert "N_1%d%s" % (len(kernel), kernel) in names, kernel      # (the mangled name)
        assert lines and all(ln.split()[-1] == "0" for ln in lines), regs
        # (--max-states: the 32-class instantiations are long straight-line kernels whose exact
        # path-by-path walk takes minutes; past 300 states the tool walks merged paths instead,
        # which is sound - it can only over-report)
        r = subprocess.run(["python3", os.path.join(ROOT, "tools", "asm_hazard_check.py"),
                            "--max-states=300", obj], capture_output=True, text=True)
        assert r.returncode == 0 and " 0 hazards, 0 incomplete" in r.stdout, r.stdout[-2000:]
