"""Operands and float64 references shared by the per-layer kernel tests: the harness tests/tools/
step_kernel_harness.py (tests/test_fp32_step_kernels_gpu.py, tests/test_bf16x3_step_kernels_gpu.py),
tests/test_bf16_bench_layers_gpu.py, tests/test_fused_gpu.py, tests/test_fullres_folds_gpu.py and
tests/test_wgrad32_folds_gpu.py.  The operand recipe (device-seeded tensors, activation
coefficients with ~15 % dropped channels, He-scaled weights, the layer a BSTATS epilogue reduces
for) for fp32 tensors, plain fp64 evaluations of every operation of the train step, one image at a time, on the GPU, and the
float64 emulation of the split-bf16 operand mode's six products (with one left out on request).
Nothing here calls the library."""
import torch
import torch.nn.functional as F

DEV = "cuda"
SLOPE = 0.01             # nn.LeakyReLU's default: the network's slope
EPS = 1e-5               # nn.InstanceNorm2d's default


# --------------------------------------------------------------------------- operands
def grand(shape, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(shape, generator=g, device=DEV) * scale


def coeffs(n, c, seed):
    """Activation coefficients alpha / beta [n, c] with ~15 % dropped channels (alpha = beta = 0)."""
    al, be = grand((n, c), seed) * 0.5 + 1.0, grand((n, c), seed + 1) * 0.7
    g = torch.Generator(device=DEV).manual_seed(seed + 2)
    drop = torch.rand((n, c), generator=g, device=DEV) < 0.15
    return (torch.where(drop, torch.zeros_like(al), al).contiguous(),
            torch.where(drop, torch.zeros_like(be), be).contiguous())


def keep_mask(n, c, seed, keep=0.8):
    """A dropout mask [n, c], already divided by the keep probability."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    return ((torch.rand((n, c), generator=g, device=DEV) < keep).float() / keep).contiguous()


def he_weight(cout, cin, seed, fan):
    return grand((cout, cin, 3, 3), seed, scale=(2.0 / fan) ** 0.5)


def norm_layer(n, H, W, C, seed):
    """The layer whose InstanceNorm-backward reductions a BSTATS epilogue emits -> (raw fp32 output
    y [n, H, W, C] with a non-zero mean, statistics [4, n, C], gamma, beta, dropout mask); the
    statistics are fp64 values rounded once."""
    y = (grand((n, H, W, C), seed, 1.5) + 0.3).contiguous()
    gamma, beta = grand((C,), seed + 1) * 0.2 + 1.0, grand((C,), seed + 2) * 0.2
    yd = y.double()
    mean = yd.mean(dim=(1, 2))
    rstd = 1.0 / torch.sqrt(yd.var(dim=(1, 2), unbiased=False) + EPS)
    al = gamma.double()[None] * rstd
    st = torch.stack([mean, rstd, al, beta.double()[None] - mean * al]).float().contiguous()
    return y, st, gamma, beta, keep_mask(n, C, seed + 3)


# --------------------------------------------------------------------------- fp64 references
def nchw64(t):
    return t.double().permute(0, 3, 1, 2)


def act64(x, al, be, rounded=False):
    """NHWC raw tensor -> NCHW float64 activated operand lrelu(x alpha[n, c] + beta[n, c]);
    rounded: evaluated in fp32 and rounded to the tensor's storage type as a loader would."""
    if rounded:
        a = F.leaky_relu(x.float() * al[:, None, None, :] + be[:, None, None, :], SLOPE).to(x.dtype)
        return a.double().permute(0, 3, 1, 2)
    z = x.double() * al.double()[:, None, None, :] + be.double()[:, None, None, :]
    return F.leaky_relu(z, SLOPE).permute(0, 3, 1, 2)


def ref_conv(a, w, b, stride):
    return torch.cat([F.conv2d(a[i:i + 1].contiguous(), w, b, stride=stride, padding=1)
                      for i in range(a.shape[0])])


def ref_dgrad(dy, w, stride, H, W):
    return torch.cat([torch.nn.grad.conv2d_input((1, w.shape[1], H, W), w, dy[i:i + 1].contiguous(),
                                                 stride=stride, padding=1)
                      for i in range(dy.shape[0])])


def ref_wgrad(a, dy, stride):
    shape = (dy.shape[1], a.shape[1], 3, 3)
    dw = torch.zeros(shape, dtype=a.dtype, device=a.device)
    for i in range(a.shape[0]):
        dw += torch.nn.grad.conv2d_weight(a[i:i + 1].contiguous(), shape, dy[i:i + 1].contiguous(),
                                          stride=stride, padding=1)
    return dw


def upsample64(a):
    """bilinear 2x of an NCHW tensor, one image at a time"""
    return torch.cat([F.interpolate(a[i:i + 1], scale_factor=2, mode="bilinear",
                                    align_corners=False) for i in range(a.shape[0])])


def ref_taps(dy):
    """D[n, i, j, t C + c] = (U^T shift_t(dy))[n, c, i, j] with U the bilinear 2x up-sampling,
    shift_t(dy)[P] = dy[P - (ky - 1, kx - 1)] (zero outside), t = 3 ky + kx.  dy: NCHW."""
    n, C, H2, W2 = dy.shape
    out = []
    for i in range(n):
        p = F.pad(dy[i:i + 1], (1, 1, 1, 1))
        sh = torch.cat([p[:, :, 2 - ky:2 - ky + H2, 2 - kx:2 - kx + W2]
                        for ky in range(3) for kx in range(3)], 1)
        low = torch.zeros(1, 9 * C, H2 // 2, W2 // 2, dtype=dy.dtype, device=dy.device,
                          requires_grad=True)
        up = F.interpolate(low, scale_factor=2, mode="bilinear", align_corners=False)
        out.append(torch.autograd.grad(up, low, sh)[0].permute(0, 2, 3, 1))
    return torch.cat(out)


def ref_up_wgrad(a, D):
    """dw[co, ci, ky, kx] = sum_q a[q, ci] D[q, t Cout + co].  a: NCHW, D: [n, h, w, 9 Cout]."""
    n, Cx, h, w = a.shape
    C9 = D.shape[3]
    ref = torch.zeros(Cx, C9, dtype=a.dtype, device=a.device)
    for i in range(n):
        ref += a[i].reshape(Cx, h * w) @ D[i].reshape(h * w, C9)
    return ref.reshape(Cx, 3, 3, C9 // 9).permute(3, 0, 1, 2)


def ref_up_dgrad(D, w):
    """g[q, ci] = sum_{t, co} D[q, t Cout + co] w[co, ci, t] -> [n, h, w, Cin].  w: OIHW slice."""
    n, h, wd_, C9 = D.shape
    B = w.permute(2, 3, 0, 1).reshape(C9, w.shape[1])
    return torch.cat([(D[i].reshape(-1, C9) @ B).reshape(1, h, wd_, -1) for i in range(n)])


def ref_in_bwd(g, y, gamma, beta, mask, eps=EPS):
    """InstanceNorm2d(affine) + LeakyReLU + channel dropout backward in fp64 through autograd:
    g = dL/da, y = raw input (both NHWC) -> (dy NHWC, dgamma, dbeta)."""
    n, H, W, C = y.shape
    dy, dgm, dbt = [], torch.zeros(C, dtype=torch.double, device=y.device), \
        torch.zeros(C, dtype=torch.double, device=y.device)
    for i in range(n):
        yi = y[i:i + 1].double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        gm = gamma.double().clone().requires_grad_(True)
        bt = beta.double().clone().requires_grad_(True)
        a = F.leaky_relu(F.instance_norm(yi, weight=gm, bias=bt, eps=eps), SLOPE)
        if mask is not None:
            a = a * mask[i].double().view(1, C, 1, 1)
        gy, gg, gb = torch.autograd.grad(a, (yi, gm, bt), g[i:i + 1].double().permute(0, 3, 1, 2))
        dy.append(gy.permute(0, 2, 3, 1))
        dgm += gg
        dbt += gb
    return torch.cat(dy), dgm, dbt


# --------------------------------------------------------------------------- split-bf16 terms
# The split-bf16 ("bf16x3") operand mode (csrc/common.h split3, csrc/conv_lowp.hip): an fp32
# operand x is staged as x = h + m + l and a product a b is formed as the six terms of weight
# >= 2^-16.  The pairs are (term of the first operand, term of the second), 0 = h, 1 = m, 2 = l.
SIX_PRODUCTS = ((0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0))
THIRD_ORDER = ((0, 2), (1, 1), (2, 0))        # the three products of weight 2^-16


def split3(t):
    """h = bf16(t), m = bf16(t - h), l = bf16(t - h - m) -> three float64 tensors.  For an fp32
    tensor these are the loaders' terms bit for bit (both differences are exact in fp32); a
    float64 operand (an activated source, which a loader holds rounded to fp32) keeps its own
    value as the target, so that the emulation's residual stays at the 2^-24 of the three
    dropped products and not at the rounding of the activation."""
    t = t.double()
    h = t.to(torch.bfloat16).double()
    m = (t - h).to(torch.bfloat16).double()
    l = (t - h - m).to(torch.bfloat16).double()
    return h, m, l


def split_products(fn, a, b):
    """fn is bilinear in (a, b) (ref_conv without a bias, ref_dgrad, ref_wgrad as a callable of the
    two operands): its float64 value on each of the six term pairs -> {(i, j): fn(a_i, b_j)}"""
    sa, sb = split3(a), split3(b)
    return {(i, j): fn(sa[i], sb[j]) for i, j in SIX_PRODUCTS}


def six_products(fn, a, b, leave_out=None, terms=None):
    """The float64 evaluation of fn on the six-product expansion of its two operands, optionally
    with one product (a pair of SIX_PRODUCTS) left out; terms: split_products(fn, a, b) when the
    caller already has them."""
    terms = split_products(fn, a, b) if terms is None else terms
    assert leave_out is None or leave_out in terms
    return sum(v for k, v in terms.items() if k != leave_out)


def rel_l2(out, ref):
    ref = ref.double()
    return ((out.double() - ref).norm() / (ref.norm() + 1e-300)).item()


def term_check(fn, a, b, exact, extra=None):
    """-> (e_drop, e_six): relative L2 error, against the exact float64 reference `exact`, of the
    six-product emulation with the least harmful third-order product left out, and of the full
    six-product emulation.  extra: what the reference adds to the bilinear part (a bias)."""
    terms = split_products(fn, a, b)
    add = 0 if extra is None else extra
    e_six = rel_l2(six_products(fn, a, b, terms=terms) + add, exact)
    e_drop = min(rel_l2(six_products(fn, a, b, leave_out=k, terms=terms) + add, exact)
                 for k in THIRD_ORDER)
    return e_drop, e_six


# --------------------------------------------------------------------------- comparisons
def metric(what, out, ref, tol, scale=None):
    """max |out - ref| / scale (default: max |ref|) against tol"""
    ref = ref.double()
    s = ref.abs().max().item() if scale is None else float(scale)
    e = (out.double() - ref).abs().max().item() / (s + 1e-300)
    return dict(what=what, err=e, tol=tol)


def failures(metrics):
    return [f"{m['what']}: max error {m['err']:.3e} > {m['tol']:.1e}"
            for m in metrics if not m["err"] <= m["tol"]]


def report(metrics):
    return "  ".join(f"{m['what']} {m['err']:.2e}/{m['tol']:.0e}" for m in metrics)
