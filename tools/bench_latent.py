#!/usr/bin/env python3
"""The latent-space analysis (`ua.latent`, csrc/latent.hip) on one MI355X, stage by stage, on
synthetic codes (three Gaussian clusters plus an offset) at the reference's size - N = 3669 test
images, D = 131072 = 512 x 16 x 16 bottleneck values, a 1.9 GB fp32 matrix - and at N = 512.

Per size, in one process: the column mean, the centred Gram (executed TFLOP/s against the 157.3
TFLOP/s fp32 matrix peak: only the tiles on or above the diagonal are formed), PCA from G, the
perplexity search + joint P, one t-SNE iteration, the whole t-SNE (1000 iterations) and the
raster; and a torch composition of the same stages, timed in alternation with them:
(X - mean) @ (X - mean).T, torch.linalg.eigh of G, a dense torch t-SNE iteration.  Device events
around repeated calls for the kernels, a host clock around synchronised work for the multi-launch
stages.  Writes one JSON document (default profiles/latent_bench.json) and prints it.

    python tools/bench_latent.py [--sizes 3669 512] [--dim 131072] [--reps 5] [--out PATH]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import unet_implementations_amd as ua  # noqa: E402

DEV = torch.device("cuda", 0)
FP32_MATRIX_PEAK_TFLOPS = 157.3


def synthetic_codes(n, d, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    centres = torch.randn(3, d, device=DEV, generator=g)
    labels = torch.randint(0, 3, (n,), device=DEV, generator=g)
    x = torch.randn(n, d, device=DEV, generator=g)
    x += centres[labels] * 0.6 + 0.4
    return x, labels


def event_ms(fn, steps, reps):
    """Median over `reps` of the device time of `steps` back-to-back calls, per call."""
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / steps)
    return statistics.median(times), [min(times), max(times)]


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def alternate(fa, fb, reps):
    """Wall times of two forms in alternation (other work shares the host) -> medians, spreads."""
    fa(), fb()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(wall_ms(fa)[0])
        tb.append(wall_ms(fb)[0])
    return (statistics.median(ta), [min(ta), max(ta)]), (statistics.median(tb), [min(tb), max(tb)])


def torch_tsne_iteration(P, y, update, gains, exaggeration, momentum, lr):
    diff = y[:, None, :] - y[None, :, :]
    q = 1.0 / (1.0 + (diff * diff).sum(dim=2))
    q.fill_diagonal_(0.0)
    Z = q.sum()
    first = ((P * exaggeration * q)[:, :, None] * diff).sum(dim=1)
    second = ((q * q)[:, :, None] * diff).sum(dim=1)
    grad = 4.0 * (first - second / Z)
    inc = update * grad < 0
    gains = torch.where(inc, gains + 0.2, gains * 0.8).clamp_min(0.01)
    update = momentum * update - lr * gains * grad
    return y + update, update, gains


def bench_size(n, d, reps):
    x, labels = synthetic_codes(n, d)
    out = {"N": n, "D": d, "codes_GB": 4e-9 * n * d}
    ms, spread = event_ms(lambda: ua.ops.latent_col_mean(x), 3, reps)
    out["col_mean"] = {"ms": ms, "spread_ms": spread, "GBps": 4e-6 * n * d / ms}
    mean = ua.ops.latent_col_mean(x)

    # the Gram, against torch's centred product, alternating
    (g_ms, g_spread), (t_ms, t_spread) = alternate(
        lambda: ua.ops.latent_gram(x, mean), lambda: (x - mean) @ (x - mean).T, reps)
    nb = -(-n // 128)
    executed = 2.0 * (nb * (nb + 1) // 2) * 128 * 128 * d
    g = ua.ops.latent_gram(x, mean)
    ref = (x - mean) @ (x - mean).T
    out["gram"] = {
        "ms": g_ms, "spread_ms": g_spread, "split_k": ua.ops.latent_gram_splitk(n, d),
        "executed_TFLOPs": executed / g_ms / 1e9,
        "share_of_fp32_matrix_peak": executed / g_ms / 1e9 / FP32_MATRIX_PEAK_TFLOPS,
        "full_product_TFLOPs_equivalent": 2.0 * n * n * d / g_ms / 1e9,
        "torch_centre_and_matmul_ms": t_ms, "torch_spread_ms": t_spread,
        "torch_over_hip": t_ms / g_ms,
        "max_difference_over_max": float((g - ref).abs().max() / ref.abs().max())}
    xc64 = x.double()
    xc64 -= xc64.mean(dim=0)
    g64 = xc64 @ xc64.T
    del xc64
    out["gram"]["error_vs_fp64_over_max"] = float((g.double() - g64).abs().max() / g64.abs().max())
    out["gram"]["torch_error_vs_fp64_over_max"] = float((ref.double() - g64).abs().max() /
                                                        g64.abs().max())
    del ref, g64

    # PCA from G (subspace iteration + the projection pass) against a full eigh of G
    G = ua.latent.LatentGram(g, x, mean)
    (p_ms, p_spread), (e_ms, e_spread) = alternate(
        lambda: ua.latent.pca_2d(G), lambda: torch.linalg.eigh(g), max(2, reps // 2))
    pca = ua.latent.pca_2d(G)
    out["pca"] = {"ms": p_ms, "spread_ms": p_spread, "iterations": pca.n_iter,
                  "residuals": pca.residuals, "torch_eigh_ms": e_ms, "torch_spread_ms": e_spread,
                  "torch_over_hip": e_ms / p_ms}
    ms, spread = event_ms(lambda: ua.ops.latent_gram_apply(g, pca.scores.new_ones(n, 8)), 20, reps)
    out["pca"]["gram_apply_ms"] = ms

    if n <= ua.latent.TSNE_MAX_N:
        ms, spread = event_ms(lambda: ua.ops.tsne_joint_p(g, 30.0), 2, reps)
        out["perplexity_search_and_joint_p"] = {"ms": ms, "spread_ms": spread}
        P, _ = ua.ops.tsne_joint_p(g, 30.0)
        s = pca.scores.double()
        y0 = (s / s[:, 0].std(unbiased=False) * 1e-4).float()
        state = torch.zeros((2, n, 6), device=DEV)
        state[0, :, :2] = y0
        state[0, :, 4:] = 1.0
        rows = torch.empty((n, 8), device=DEV)
        lr = max(n / 48.0, 50.0)

        def hip_iteration():
            ua.ops.tsne_step(P, state[0], state[1], rows, 12.0, 0.5, lr)

        yt, ut, gt = y0.clone(), torch.zeros_like(y0), torch.ones_like(y0)
        h_ms, h_spread = event_ms(hip_iteration, 50, reps)
        t_ms, t_spread = event_ms(lambda: torch_tsne_iteration(P, yt, ut, gt, 12.0, 0.5, lr), 5,
                                  reps)
        y1 = torch_tsne_iteration(P, y0, ut, gt, 12.0, 0.5, lr)[0]
        out["tsne_iteration"] = {
            "ms": h_ms, "spread_ms": h_spread, "P_read_GBps": 4e-6 * n * n / h_ms,
            "torch_dense_ms": t_ms, "torch_spread_ms": t_spread, "torch_over_hip": t_ms / h_ms,
            "max_difference_over_max": float((state[1, :, :2] - y1).abs().max() / y1.abs().max())}
        times, res = [], None
        for _ in range(max(2, reps // 2)):
            t, res = wall_ms(lambda: ua.latent.tsne_2d(G, perplexity=30.0, init=y0))
            times.append(t)
        out["tsne_whole"] = {"ms": statistics.median(times), "spread_ms": [min(times), max(times)],
                             "iterations": res.n_iter + 1, "kl_divergence": res.kl_divergence}
        coords = res.y
    else:
        coords = pca.scores
    pal = torch.tensor(ua.latent.VIRIDIS3, dtype=torch.uint8, device=DEV)
    centres = ua.latent.pixel_centres(coords, (600, 800)).contiguous()
    lab = labels.to(torch.uint8)
    ms, spread = event_ms(lambda: ua.ops.latent_scatter(centres, lab, pal, (600, 800), 4), 20, reps)
    out["raster_600x800"] = {"ms": ms, "spread_ms": spread}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[3669, 512])
    ap.add_argument("--dim", type=int, default=131072)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "latent_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_latent.py needs an MI355X (no CPU fallback exists)")
    result = {"device": torch.cuda.get_device_name(0),
              "fp32_matrix_peak_TFLOPs": FP32_MATRIX_PEAK_TFLOPS,
              "sizes": [bench_size(n, args.dim, args.reps) for n in args.sizes]}
    text = json.dumps(result, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
