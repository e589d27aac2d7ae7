"""CPU (-m "not gpu"): the uint8-batch surface without a device - the `_b16` stems and the
uint8-target twins of the loss / metric entry points are declared, exported and bound, the ABI
version is unchanged, their host-side argument checks answer before any launch, and the Python
surface validates its arguments."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "unet_hip.h")

LOSS_TWINS = ("unet_dice_wce_loss_fwd_bwd", "unet_dice_wce_loss_grad",
              "unet_dice_wce_loss_shard_stats", "unet_dice_wce_loss_shard_apply",
              "unet_argmax_dice_counts")
NEW = ("unet_stem_u8_fwd_b16", "unet_stem_u8_bwd_weight_b16") + \
    tuple(n + "_u8" for n in LOSS_TWINS)


def test_entry_points_declared_exported_and_bound(ua):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    handle = ctypes.CDLL(ua.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), f"{name} not declared in unet_hip.h"
        assert hasattr(handle, name), f"{name} not exported"
        assert name in ua._lib.SIGNATURES
    S = ua._lib.SIGNATURES
    for name in LOSS_TWINS:     # a twin takes the arguments of its int64 form
        assert S[name + "_u8"] == S[name]
    assert S["unet_stem_u8_fwd_b16"] == S["unet_stem_u8_fwd"]
    assert S["unet_stem_u8_bwd_weight_b16"] == S["unet_stem_u8_bwd_weight"]


def test_abi_version_is_unchanged(ua):
    assert ua._lib.ABI_VERSION == 11 and ua.lib().unet_abi_version() == 11
    assert re.search(r"#define\s+UNET_ABI_VERSION\s+11\b", open(HEADER).read())


def test_stem_arguments_are_rejected_before_any_launch(ua):
    lib = ua.lib()
    m3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    px = ctypes.c_int(0)
    # (image, mean, std, w, bias, y, workspace, bytes, &px, N, H, W, Cout, stream)
    rc = lib.unet_stem_u8_fwd_b16(None, m3, m3, 1, 1, 1, 1, 1 << 30, ctypes.byref(px), 1, 8, 128,
                                  32, None)
    assert rc == -1 and b"null" in lib.unet_last_error()
    rc = lib.unet_stem_u8_fwd_b16(1, m3, m3, 1, 1, None, 1, 1 << 30, ctypes.byref(px), 1, 8, 128,
                                  32, None)
    assert rc == -1 and b"null" in lib.unet_last_error()
    for w in (96, 64, 130):
        rc = lib.unet_stem_u8_fwd_b16(1, m3, m3, 1, 1, 1, 1, 1 << 30, ctypes.byref(px), 1, 8, w,
                                      32, None)
        assert rc == -1 and b"W % 128" in lib.unet_last_error()
    rc = lib.unet_stem_u8_fwd_b16(1, m3, m3, 1, 1, 1, 1, 16, ctypes.byref(px), 1, 8, 128, 32, None)
    assert rc == -3
    # (image, mean, std, dy, dw, workspace, bytes, N, H, W, Cout, stream)
    rc = lib.unet_stem_u8_bwd_weight_b16(None, m3, m3, 1, 1, 1, 1 << 30, 1, 8, 128, 32, None)
    assert rc == -1 and b"null" in lib.unet_last_error()
    rc = lib.unet_stem_u8_bwd_weight_b16(1, m3, m3, None, 1, 1, 1 << 30, 1, 8, 128, 32, None)
    assert rc == -1 and b"null" in lib.unet_last_error()
    for w in (96, 130):
        rc = lib.unet_stem_u8_bwd_weight_b16(1, m3, m3, 1, 1, 1, 1 << 30, 1, 8, w, 32, None)
        assert rc == -1 and b"W % 128" in lib.unet_last_error()
    rc = lib.unet_stem_u8_bwd_weight_b16(1, m3, m3, 1, 1, 1, 16, 1, 8, 128, 32, None)
    assert rc == -3


BAD_IGNORE = (-100, -1, 0, 1, 2, 256, 1000)


def test_uint8_target_arguments_are_rejected_before_any_launch(ua):
    lib = ua.lib()
    big = 1 << 30

    def fwd_bwd(logits, target, ignore):
        return lib.unet_dice_wce_loss_fwd_bwd_u8(logits, target, 1, None, 1, big, 1, 8, 8, 1e-5,
                                                 1.0, 1.0, ignore, 1, None, 1.0, None)

    def grad(logits, target, ignore):
        return lib.unet_dice_wce_loss_grad_u8(logits, target, 1, big, None, 1, 1, 8, 8, ignore,
                                              None)

    def stats(logits, target, ignore):
        return lib.unet_dice_wce_loss_shard_stats_u8(logits, target, 1, 1, big, 1, 8, 8, 1e-5,
                                                     ignore, None)

    def apply(logits, target, ignore):
        return lib.unet_dice_wce_loss_shard_apply_u8(logits, target, 1, 1, 1, None, 1, big, 1, 8,
                                                     8, 1e-5, 1.0, 1.0, ignore, 1, None, 1.0, None)

    def counts(logits, target, ignore):
        return lib.unet_argmax_dice_counts_u8(logits, target, None, 1, 1, 8, 8, ignore, None)

    for fn in (fwd_bwd, grad, stats, apply, counts):
        assert fn(None, 1, 255) == -1
        assert fn(1, None, 255) == -1
        for bad in BAD_IGNORE:
            assert fn(1, 1, bad) == -1 and b"ignore_index in 3..255" in lib.unet_last_error(), \
                (fn.__name__, bad)
    # the int64 forms keep taking any ignore_index: -100 (torch's default) passes the checks and
    # stops at the workspace size, still before a launch
    rc = lib.unet_dice_wce_loss_fwd_bwd(1, 1, 1, None, 1, 16, 1, 8, 8, 1e-5, 1.0, 1.0, -100, 1,
                                        None, 1.0, None)
    assert rc == -3
    rc = lib.unet_dice_wce_loss_fwd_bwd_u8(1, 1, 1, None, 1, 16, 1, 8, 8, 1e-5, 1.0, 1.0, 255, 1,
                                           None, 1.0, None)
    assert rc == -3


def test_python_surface_checks_its_arguments(ua):
    with pytest.raises(ValueError, match="target_layout"):
        ua.SimpleLoss(target_layout="x")
    assert ua.SimpleLoss().target_layout == "int64"
    assert ua.get_loss_function().target_layout == "int64"
    assert ua.SimpleLoss(target_layout="u8").target_layout == "u8"
    for fn in (ua.train_step, ua.GraphedTrainStep.__init__, ua.validate):
        assert inspect.signature(fn).parameters["input_layout"].default is None
    assert inspect.signature(ua.CLIPUNet.forward).parameters["input_layout"].default == "nchw"
    # no CPU fallback: the u8 loss refuses host tensors like the default one
    z, t = torch.zeros(1, 3, 8, 8), torch.zeros(1, 8, 8, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ua.SimpleLoss(target_layout="u8")(z, t)
    with pytest.raises(TypeError):
        ua.ops._target_twin("unet_argmax_dice_counts", torch.zeros(1, dtype=torch.int32))
