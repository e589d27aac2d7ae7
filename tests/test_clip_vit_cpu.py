"""CPU (-m "not gpu"): the CLIP image tower without a device - the ABI surface and every host-side
refusal, the module tree against OpenAI CLIP's key set, the stock-torch restatement against
tests/golden/clip_extractor.npz (recorded through the reference's ClipPatchExtractor), and the
measured error of the bf16 emulation, which is the yardstick of the GPU tolerances."""
import ctypes
import importlib.util
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load("clip_vit_ref", ["tools", "clip_vit_ref.py"])

SYMBOLS = ("unet_vit_patchify", "unet_vit_gemm_bf16", "unet_vit_tokens_ln", "unet_vit_layernorm",
           "unet_vit_attention", "unet_vit_head")


def test_symbols_header_bindings_and_abi_version(ua):
    handle = ctypes.CDLL(ua.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(handle, name), name
        assert name in ua._lib.SIGNATURES, name
        assert "int " + name + "(" in header, name
    assert "#define UNET_ABI_VERSION 11" in header
    assert ua.lib().unet_abi_version() == ua._lib.ABI_VERSION == 11
    assert "vit.hip" in open(os.path.join(ROOT, "unet-implementations_amd", "csrc", "Makefile")).read()


def test_entry_points_refuse_bad_arguments_before_any_device_work(ua):
    lib = ua.lib()
    m = (ctypes.c_float * 3)(*R.CLIP_MEAN)
    s = (ctypes.c_float * 3)(*R.CLIP_STD)
    err = lib.unet_last_error
    # patch gather
    assert lib.unet_vit_patchify(None, 0, m, s, 1, 1, 224, 224, 224, 16, 768, None) == -1
    assert b"null" in err()
    assert lib.unet_vit_patchify(1, 1, None, None, 1, 1, 224, 224, 224, 16, 768, None) == -1
    assert lib.unet_vit_patchify(1, 0, m, s, 1, 1, 224, 224, 224, 15, 688, None) == -1
    assert b"R % P" in err()
    assert lib.unet_vit_patchify(1, 0, m, s, 1, 1, 224, 224, 224, 14, 588, None) == -1
    assert b"Kp" in err()
    # GEMM
    assert lib.unet_vit_gemm_bf16(None, 1, 1, 1, 0, 17, 64, 64, None) == -1
    assert b"null" in err()
    assert lib.unet_vit_gemm_bf16(1, 1, None, 1, 1, 17, 64, 64, None) == -1
    assert b"bias" in err()
    assert lib.unet_vit_gemm_bf16(1, 1, 1, 1, 4, 17, 64, 64, None) == -1
    assert lib.unet_vit_gemm_bf16(1, 1, 1, 1, 0, 17, 96, 64, None) == -1
    assert b"Nout % 64" in err()
    assert lib.unet_vit_gemm_bf16(1, 1, 1, 1, 0, 17, 64, 72, None) == -1
    # tokens + ln_pre, LayerNorm, head: T > 257, D % 64 != 0
    assert lib.unet_vit_tokens_ln(None, 1, 1, 1, 1, 1e-5, 1, 1, 50, 128, None) == -1
    assert lib.unet_vit_tokens_ln(1, 1, 1, 1, 1, 1e-5, 1, 1, 577, 1024, None) == -1
    assert b"257" in err()
    assert lib.unet_vit_tokens_ln(1, 1, 1, 1, 1, 1e-5, 1, 1, 50, 96, None) == -1
    assert b"multiple of 64" in err()
    assert lib.unet_vit_layernorm(1, None, 1, 1e-5, 1, 4, 128, None) == -1
    assert lib.unet_vit_layernorm(1, 1, 1, 1e-5, 1, 4, 100, None) == -1
    assert lib.unet_vit_layernorm(1, 1, 1, 1e-5, 1, 4, 2048, None) == -1
    assert lib.unet_vit_head(1, 1, 1, 1e-5, None, 1, 1, 50, 128, 512, 16, None) == -1
    assert lib.unet_vit_head(1, 1, 1, 1e-5, 1, 1, 1, 577, 128, 512, 16, None) == -1
    assert lib.unet_vit_head(1, 1, 1, 1e-5, 1, 1, 1, 50, 96, 512, 16, None) == -1
    # attention: T > 257, D % 64 != 0, head dimension != 64
    assert lib.unet_vit_attention(None, 1, 1, 50, 128, 2, None) == -1
    assert b"null" in err()
    assert lib.unet_vit_attention(1, 1, 1, 258, 128, 2, None) == -1
    assert b"257" in err()
    assert lib.unet_vit_attention(1, 1, 1, 50, 96, 2, None) == -1
    assert b"multiple of 64" in err()
    assert lib.unet_vit_attention(1, 1, 1, 50, 128, 4, None) == -1
    assert b"head dimension" in err()


def test_no_vit_kernel_uses_scratch_and_the_hazard_check_is_clean():
    obj = os.path.join(ROOT, "unet-implementations_amd", "csrc", "build", "vit.o")
    if not os.path.exists(obj):
        pytest.skip("no built objects (run __graft_entry__.build() first)")
    regs = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_regs.sh"), obj],
                          capture_output=True, text=True, check=True).stdout
    lines = [l for l in regs.splitlines() if "scratch" in l]
    assert len(lines) >= 20, regs
    assert all(l.split()[-1] == "0" for l in lines), regs
    r = subprocess.run(["python3", os.path.join(ROOT, "tools", "asm_hazard_check.py"), obj],
                       capture_output=True, text=True)
    assert r.returncode == 0 and " 0 hazards, 0 incomplete" in r.stdout, r.stdout[-2000:]


def openai_vit_keys(width, layers, patch, tokens, out_dim):
    """The key set and shapes of clip.model.VisionTransformer.state_dict()."""
    D = width
    keys = {"conv1.weight": (D, 3, patch, patch), "class_embedding": (D,),
            "positional_embedding": (tokens, D), "ln_pre.weight": (D,), "ln_pre.bias": (D,),
            "ln_post.weight": (D,), "ln_post.bias": (D,), "proj": (D, out_dim)}
    for i in range(layers):
        p = f"transformer.resblocks.{i}."
        keys.update({p + "ln_1.weight": (D,), p + "ln_1.bias": (D,),
                     p + "attn.in_proj_weight": (3 * D, D), p + "attn.in_proj_bias": (3 * D,),
                     p + "attn.out_proj.weight": (D, D), p + "attn.out_proj.bias": (D,),
                     p + "ln_2.weight": (D,), p + "ln_2.bias": (D,),
                     p + "mlp.c_fc.weight": (4 * D, D), p + "mlp.c_fc.bias": (4 * D,),
                     p + "mlp.c_proj.weight": (D, 4 * D), p + "mlp.c_proj.bias": (D,)})
    return keys


def test_state_dict_is_openai_clips_for_vit_b16(ua):
    m = ua.ClipVisionTransformer()
    sd = m.state_dict()
    want = openai_vit_keys(768, 12, 16, 197, 512)
    assert len(want) == 152 == 5 + 12 * 12 + 3
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert all(not p.requires_grad for p in m.parameters())
    # the restatement has the same tree: its state dict loads, with and without the prefix
    ref = R.VisionTransformer(**R.GEOMETRIES["vit_b16"])
    assert {k: tuple(v.shape) for k, v in ref.state_dict().items()} == want
    m.load_state_dict(ref.state_dict())


def test_from_state_dict_infers_the_geometry_with_and_without_the_prefix(ua):
    sd = R.seeded_state_dict(R.GEOMETRIES["fixture"])
    for given in (sd, {"visual." + k: v for k, v in sd.items()} | {"logit_scale": torch.ones(())}):
        m = ua.ClipVisionTransformer.from_state_dict(given)
        assert (m.input_resolution, m.patch_size, m.width, m.layers, m.heads, m.output_dim,
                m.tokens) == (224, 32, 128, 2, 2, 512, 50)
        assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    ext = ua.ClipPatchExtractor(R.StandInClip(R.build(R.GEOMETRIES["fixture"])), device="cpu")
    assert ext.feature_dim == 512 and ext.grid_size == (7, 7)
    assert torch.equal(ext.visual.proj, sd["proj"])


def test_supported_geometries_construct_and_others_name_the_limit(ua):
    with torch.device("meta"):
        l14 = ua.ClipVisionTransformer(224, 14, 1024, 24, 16, 768)
        b32 = ua.ClipVisionTransformer(224, 32, 768, 12, 12, 512)
        assert l14.tokens == 257 and b32.tokens == 50
        with pytest.raises(NotImplementedError, match="577 tokens"):
            ua.ClipVisionTransformer(336, 14, 1024, 24, 16, 768)
        with pytest.raises(NotImplementedError, match="head dimension"):
            ua.ClipVisionTransformer(224, 16, 768, 12, 8, 512)
        with pytest.raises(NotImplementedError, match="multiple of 64"):
            ua.ClipVisionTransformer(224, 16, 800, 12, 12, 512)


def test_loop_functions_pass_none_through_without_an_extractor(ua):
    assert ua.clip.extract_clip_features(None, {}, None, "cpu") is None
    with pytest.raises(KeyError, match="clip_image"):
        ua.clip.extract_clip_features(lambda x, input_layout: x, {}, torch.zeros(1), "cpu")
    seen = {}

    def fake(x, input_layout):
        seen["layout"], seen["x"] = input_layout, x
        return "features"

    u8 = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    assert ua.clip.extract_clip_features(fake, {}, u8, "cpu", "nhwc_u8") == "features"
    assert seen["layout"] == "nhwc_u8" and seen["x"] is u8
    ci = torch.zeros(1, 3, 8, 8)
    ua.clip.extract_clip_features(fake, {"clip_image": ci}, u8, "cpu", "nhwc_u8")
    assert seen["layout"] == "nchw" and torch.equal(seen["x"], ci)


def test_restatement_reproduces_the_golden_of_the_reference_extractor(golden):
    """The resize (F.interpolate, bilinear, align_corners=False, only when the size differs) and
    the broadcast semantics of ClipPatchExtractor.forward, with the weights rebuilt from the seed."""
    g = golden("clip_extractor")
    geometry = R.GEOMETRIES["fixture"]
    sd = R.seeded_state_dict(geometry, int(g["seed_w"]))
    for key, val in R.pin_weights(sd).items():
        assert np.array_equal(np.asarray(val), g[key]), key
    assert int(g["feature_dim"]) == 512 and tuple(g["grid_size"]) == (7, 7)
    visual = R.build(geometry, int(g["seed_w"]))
    for tag in ("224", "96x128"):
        y = R.extractor_ref(visual, R.normalise_u8(g[f"u8_{tag}"]))
        assert tuple(y.shape) == (2, 512, 16, 16)
        ref = torch.from_numpy(g[f"embed_{tag}"])
        err = ((y[:, :, 0, 0] - ref).abs().max() / ref.abs().max()).item()
        print(f"restatement vs golden {tag}: {err:.3e}")
        assert err <= 1e-6
        # interpolation from 1 x 1 is a copy up to the rounding of w0 v + w1 v: the 256 positions
        # agree to an fp32 ulp (the recorded flag says whether they were bitwise equal)
        dev = ((y - y[:, :, :1, :1]).abs().max() / y.abs().max()).item()
        assert dev == float(g[f"grid_max_dev_{tag}"]) <= 2.0 ** -23
        assert bool(g[f"grid_equal_{tag}"]) == (dev == 0.0)


def test_bf16_emulation_error_is_measured_and_recorded():
    """The error of the bf16 rounding model against the fp64 restatement: the yardstick the GPU
    tolerances (2 x this error on the same inputs) refer to.  Written to
    profiles/clip_vit_bf16_error.txt."""
    rows = []
    for name, n in (("fixture", 2), ("full_width", 2)):
        geometry = R.GEOMETRIES[name]
        sd = R.seeded_state_dict(geometry)
        x = R.normalise_u8(R.images_u8(77, n, 224, 224))
        with torch.no_grad():
            ref = R.build(geometry, dtype=torch.float64)(x.double())
        same = R.emulate(sd, x, geometry["heads"], emulate_bf16=False)
        assert R.errors(same, ref)[1] <= 1e-12        # the emulation's GEMM form IS the network
        l2, mx = R.errors(R.emulate(sd, x, geometry["heads"]), ref)
        tokens = (geometry["input_resolution"] // geometry["patch_size"]) ** 2 + 1
        rows.append(f"{name:<12} D={geometry['width']:<5} T={tokens:<4} layers={geometry['layers']} "
                    f"N={n}  rel_l2={l2:.3e}  max_rel={mx:.3e}")
        print(rows[-1])
        # bf16 operands carry 2^-9 relative rounding error each: the embedding cannot be better than
        # ~1e-4 nor, two blocks deep, worse than a few per cent
        assert 1e-5 < l2 < 5e-2 and mx < 1e-1
    text = ("# bf16 emulation of the CLIP tower (tests/tools/clip_vit_ref.py: operands rounded where\n"
            "# csrc/vit.hip rounds them, fp64 accumulation) against the fp64 restatement; embedding\n"
            "# [N, 512], seeded weights, uint8 224 x 224 inputs.  Written by\n"
            "# tests/test_clip_vit_cpu.py::test_bf16_emulation_error_is_measured_and_recorded\n"
            + "\n".join(rows) + "\n")
    path = os.path.join(ROOT, "profiles", "clip_vit_bf16_error.txt")
    try:
        with open(path, "w") as f:
            f.write(text)
    except OSError:
        pass    # a read-only checkout still runs the measurement
