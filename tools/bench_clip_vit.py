#!/usr/bin/env python3
"""Time the CLIP image tower of CLIP_UNet (ClipPatchExtractor.forward, ViT-B/16) on the HIP path
against the same network through stock torch-ROCm in bf16, in one process.

    python tools/bench_clip_vit.py [--out profiles/clip_vit_bench.json]

Per batch size (8: the benchmark batch, 16: the reference's CLIP batch) and input (uint8 224 x 224,
uint8 512 x 512 - the resize path): HIP events around `--iters` warm iterations, the two sides
alternating, median of `--runs` runs.  The baseline is the restatement module of
tests/tools/clip_vit_ref.py moved to the device in bf16, fed the normalised fp32 NCHW batch the
reference's loader delivers (its resize and broadcast included).  Also: both sides' embedding error against the fp64 restatement on two images, the extractor as a share of
the CLIP_UNet train step (the step of `bench.py --clip`, bs 8 at 512 x 512, alone and with the
extractor in front), and per-kernel-group times from event brackets around every entry point, with
the GEMM group's fraction of the dense bf16 matrix peak.  Prints one JSON line."""
import argparse
import importlib.util
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import unet_implementations_amd as ua  # noqa: E402

PEAK_BF16_MFMA_TFLOPS = 2500.0   # MI355X dense bf16 matrix peak (spec)


def _ref():
    spec = importlib.util.spec_from_file_location(
        "clip_vit_ref", os.path.join(ROOT, "tests", "tools", "clip_vit_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(fns, iters, runs):
    """{name: median ms per call}: every run times each side once, in turn."""
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(runs):
        for k, fn in fns.items():
            ms[k].append(timed(fn, iters))
    return {k: statistics.median(v) for k, v in ms.items()}, {k: (min(v), max(v)) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_clip_vit needs the GPU (no timing is taken without one)")
    dev = torch.device("cuda", 0)
    R = _ref()
    geometry = R.GEOMETRIES["vit_b16"]
    visual = R.build(geometry)
    ext = ua.ClipPatchExtractor(R.StandInClip(visual), device=dev)
    base = R.build(geometry).to(dev).to(torch.bfloat16)
    T, D, L = 197, geometry["width"], geometry["layers"]
    result = {"model": "ViT-B/16 @ 224 (seeded weights)", "iters": args.iters, "runs": args.runs,
              "cases": []}
    with torch.no_grad():
        for bs in (8, 16):
            for hw in (224, 512):
                u8 = torch.from_numpy(R.images_u8(bs + hw, bs, hw, hw)).to(dev)
                x32 = R.normalise_u8(u8.cpu()).to(dev)
                fns = {"hip": lambda: ext(u8, input_layout="nhwc_u8"),
                       "torch_bf16": lambda: R.extractor_ref(base, x32)}
                med, spread = alternate(fns, args.iters, args.runs)
                got = fns["hip"]()[:, :, 0, 0].double()
                ref = fns["torch_bf16"]()[:, :, 0, 0].double()
                result["cases"].append({
                    "batch": bs, "input": f"uint8 {hw}x{hw}", "hip_ms": med["hip"],
                    "torch_bf16_ms": med["torch_bf16"], "hip_min_max_ms": spread["hip"],
                    "torch_min_max_ms": spread["torch_bf16"],
                    "speedup_vs_torch": med["torch_bf16"] / med["hip"],
                    "hip_img_per_s": bs / med["hip"] * 1e3,
                    "rel_l2_hip_vs_torch_bf16": ((got - ref).norm() / ref.norm()).item()})
        # both sides against the fp64 restatement (CPU) on two images: 12 blocks deep
        u8 = R.images_u8(5, 2, 224, 224)
        x32 = R.normalise_u8(u8)
        ref = R.build(geometry, dtype=torch.float64)(x32.double())
        result["embedding_error_vs_fp64_n2"] = {
            "hip": R.errors(ext(torch.from_numpy(u8), input_layout="nhwc_u8")[:, :, 0, 0], ref),
            "torch_bf16": R.errors(R.extractor_ref(base, x32.to(dev))[:, :, 0, 0], ref),
            "what": "(relative L2, max error / max |y|)"}
        # per-kernel-group times at bs 16, 224 x 224 (event brackets around every entry point: a
        # pass of its own, the brackets cost stream time)
        bs = 16
        u8 = torch.from_numpy(R.images_u8(1, bs, 224, 224)).to(dev)
        timer = ua.ops.KernelTimer()
        ua.ops.set_timer(timer)
        passes = 10
        for _ in range(passes):
            ext(u8, input_layout="nhwc_u8")
        ua.ops.set_timer(None)
        groups = {}
        for tag, d in timer.summary().items():
            name = {"vit_gemm": "gemm", "vit_attention": "attention", "vit_ln": "layernorm"}.get(
                tag, "rest")
            grp = groups.setdefault(name, {"ms": 0.0, "launches": 0, "flops": 0.0})
            grp["ms"] += d["ms"] / passes
            grp["launches"] += d["launches"] // passes
            grp["flops"] += d["flops"] / passes
        for grp in groups.values():
            if grp["flops"]:
                grp["tflops"] = grp["flops"] / (grp["ms"] * 1e-3) * 1e-12
        M = bs * T
        gemm_flops = 2.0 * M * (L * 12 * D * D) + 2.0 * bs * 196 * 768 * D
        g = groups["gemm"]
        assert abs(g["flops"] - gemm_flops) <= 1e-6 * gemm_flops
        g["frac_of_bf16_dense_peak"] = g["tflops"] / PEAK_BF16_MFMA_TFLOPS
        result["kernel_groups_bs16_224"] = groups

    # the extractor as a share of the CLIP_UNet train step (bench.py --clip: bs 8, 512 x 512, fp32)
    from oracle.unet_ref import synthetic_batch
    torch.manual_seed(1234)
    model = ua.CLIPUNet(with_clip_features=True, clip_dim=512).to(dev).train()
    opt = ua.create_optimizer(model)
    lossf = ua.get_loss_function()
    img, tgt = synthetic_batch(1234, 8, 512, 512)
    img, tgt = img.to(dev), tgt.to(dev)
    feats = torch.randn(8, 512, 16, 16, device=dev)
    clip224 = torch.from_numpy(R.images_u8(2, 8, 224, 224)).to(dev)

    def step_alone():
        return ua.clip.train_step(model, opt, lossf, img, tgt,
                                  clip_extractor=lambda x, input_layout: feats, clip_images=clip224)

    def step_with():
        return ua.clip.train_step(model, opt, lossf, img, tgt, clip_extractor=ext,
                                  clip_images=clip224)

    med, spread = alternate({"step": step_alone, "step_plus_extractor": step_with},
                            max(10, args.iters // 5), args.runs)
    result["clip_unet_step_bs8_512"] = {
        "step_ms": med["step"], "step_plus_extractor_ms": med["step_plus_extractor"],
        "step_min_max_ms": spread["step"], "with_min_max_ms": spread["step_plus_extractor"],
        "extractor_ms": med["step_plus_extractor"] - med["step"],
        "extractor_share_of_step": (med["step_plus_extractor"] - med["step"]) / med["step_plus_extractor"],
        "img_per_s_alone": 8 / med["step"] * 1e3,
        "img_per_s_with_extractor": 8 / med["step_plus_extractor"] * 1e3}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
