"""Operands and float64 references of tests/test_wgrad_fp64_gpu.py: one weight-gradient call per
row of its table, the reference rounding what the row's kernel rounds before it multiplies - and
nothing else, so that what is left for the bound is the fp32 accumulation.  Nothing here calls
the library; tests/test_wgrad_refs_cpu.py holds the references to an independent nine-tap einsum
and checks, on the references alone, that every row's drawn inputs leave the reference
unambiguous and that the row would notice one missing dy pixel.

WHAT EACH FAMILY ROUNDS (read from the loaders of csrc/conv_wgrad.hip; act4 = csrc/conv_params.h
act4f: z = v * alpha + beta in fp32 - one fused multiply-add where the compiler contracts it -,
then max(z, slope * z)):

  conv_wgrad_kernel<.., float, float, NW>, conv_wgrad_taps_kernel<.., float, float, NW>,
  conv_wgrad_wino_kernel, conv_wgrad_wino32_kernel, the stem kernels
      nothing: fp32 operands, act4 in fp32, staged as fp32 (conv_wgrad_kernel::put_slot,
      l. 248-258).  The reference is float64 of the fp32 operands.
  conv_wgrad_bf16_kernel<.., NPL = 3, ..> (split bf16, fp32 tensors)
      nothing to one fp32 rounding: the activated fp32 value is split into three bf16 planes
      (store_stage -> put -> split3, l. 770-790) and six products are formed.  Reference as above.
  conv_wgrad_bf16_kernel<.., NPL = 1, .., float, float, false, 1> (unet_conv3x3_bwd_weight_bf16)
      both operands are rounded to bf16 while staged (put -> to_bf16); the entry has no
      activation.  The row draws its operands as bf16 numbers, so the rounding is exact and the
      reference is float64 of the same numbers.
  conv_wgrad_bf16_kernel<.., __bf16, __bf16, ACT, STRIDE> (bf16 tensors, segment kernels)
      x and dy are read as stored (buf_ld4<__bf16> widens); the activated operand is ROUNDED TO
      BF16 after the fp32 activation (store_stage l. 787-789: act4, then put -> to_bf16 l. 764-772).
  conv_wgrad_b16_ring_kernel
      the same (l. 1022-1026): `act4(widen16(..))`, then `h[e] = (__bf16)lo[e]` on the way to LDS.
  conv_wgrad_taps_b16_kernel
      the same (l. 581-585): store_stage `v = act4(..)`, then `h[0] = (__bf16)v[0] ..`.  D is copied
      as stored.
      (tests/test_wgrad_defer_gpu.py::Layer.ref keeps an unrounded fp32 activation for its bf16
      "up" rows, which run this kernel, under an 8e-3 bound that covers the difference; what it
      does for "in" - rounded after an fp32 activation - is what the ring and segment loaders do.)
  conv_wgrad_kernel<.., __bf16, __bf16, 4>, conv_wgrad_taps_kernel<.., __bf16, __bf16, 4>
  (bf16 tensors on the fp32 matrix cores)
      x and dy are read as stored and widened; NOTHING is rounded after the activation: act4's
      fp32 result goes to LDS as fp32 (put_slot l. 251-253 / act_slot, store_stage l. 408-416 write
      f32x4).
  uint8 stem
      the image is normalised on load, (u8 / 255 - mean) / std; the reference evaluates that in
      float64 from the fp32 mean and std the call is given.

Where the activated operand is rounded to bf16, the reference rounds the float64 activation
(`act="fp64"`): a fused multiply-add rounds the exact x alpha + beta once to fp32, which a
rounding of the float64 value to bf16 reproduces except on double-rounding ties.  The other
legitimate reading, an unfused fp32 multiply and add and then the rounding (`act="fp32"`), gives
the AMBIGUITY of the reference: a few operand elements land on the other side of a bf16 tie.
test_wgrad_refs_cpu.py requires it to stay below a tenth of the row's bound."""
import importlib.util
import os

import torch
import torch.nn.functional as F

_HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load("fp64_layer_refs")
SLOPE = R.SLOPE
BF = torch.bfloat16
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)

# kernels whose loader rounds the ACTIVATED operand to bf16 (see above)
ROUNDING_KERNELS = ("conv_wgrad_b16_ring_kernel", "conv_wgrad_taps_b16_kernel",
                    "conv_wgrad_bf16_kernel")


def rounds_activation(row):
    """Does the row's kernel round the activated operand to bf16?  Only the bf16-tensor kernels
    of the bf16 matrix cores do; every launch of a row must agree."""
    if row.mode != "b16" or not row.act:
        return False
    answers = {any(k in name for k in ROUNDING_KERNELS) for name in row.kernel}
    assert len(answers) == 1, f"the launches of one row round differently: {row.kernel}"
    return answers.pop()


def r16(t):
    return t.to(BF).float()


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _coeffs(n, c, seed):
    """alpha / beta [n, c] with ~15 % dropped channels (the recipe of fp64_layer_refs.coeffs on
    the CPU generator, so that the CPU tests see the operands the GPU test runs)"""
    al, be = _randn((n, c), seed) * 0.5 + 1.0, _randn((n, c), seed + 1) * 0.7
    drop = torch.rand((n, c), generator=torch.Generator().manual_seed(seed + 2)) < 0.15
    return (torch.where(drop, torch.zeros_like(al), al).contiguous(),
            torch.where(drop, torch.zeros_like(be), be).contiguous())


class Operands:
    """The seeded operands of one row, on the CPU, NHWC, fp32 values (bf16 numbers where the row's
    tensors are bf16 or its entry rounds to bf16):
      x [N, H, W, Cx] (u8: uint8 [N, H, W, 3]), coef = (alpha, beta) or None,
      dy [N, Ho, Wo, Cout] - for "up" the tap gradients D [N, H, W, 9 Cout]."""

    def __init__(self, row):
        self.row = row
        s, seed = row, row.seed
        self.Ho, self.Wo = (s.H - 1) // s.stride + 1, (s.W - 1) // s.stride + 1
        as_b16 = s.mode in ("b16", "bf16")
        self.coef = _coeffs(s.N, s.Cx, seed + 10) if s.act else None
        if s.entry == "u8":
            self.x = torch.randint(0, 256, (s.N, s.H, s.W, 3), dtype=torch.uint8,
                                   generator=torch.Generator().manual_seed(seed))
        else:
            self.x = _randn((s.N, s.H, s.W, s.Cx), seed)
            if as_b16 and s.Cx != 3:          # (the RGB image stays fp32)
                self.x = r16(self.x)
        dshape = (s.N, s.H, s.W, 9 * s.Cout) if s.entry == "up" else (s.N, self.Ho, self.Wo, s.Cout)
        self.dy = _randn(dshape, seed + 1)
        if as_b16:
            self.dy = r16(self.dy)

    # ---- the activated operand, NCHW float64
    def a64(self, act="fp64", dev="cpu"):
        s = self.row
        x = self.x.to(dev)
        if s.entry == "u8":
            m = torch.tensor(IMAGENET_MEAN, dtype=torch.float32, device=dev).double()
            sd = torch.tensor(IMAGENET_STD, dtype=torch.float32, device=dev).double()
            return ((x.double() / 255.0 - m) / sd).permute(0, 3, 1, 2)
        if self.coef is None:
            return R.nchw64(x)
        al, be = (c.to(dev) for c in self.coef)
        if not rounds_activation(s):
            return R.act64(x, al, be)
        if act == "fp32":     # unfused fp32 multiply and add, then the rounding
            return R.act64(x.to(BF), al, be, rounded=True)
        return R.act64(x, al, be).to(BF).double()

    def dy64(self, dev="cpu", drop_pixel=False):
        """dy (or D) in float64: NCHW for the 3x3 forms, [N, h, w, 9 Cout] for "up".
        drop_pixel: the last pixel (N - 1, Ho - 1, Wo - 1) zeroed in all channels."""
        d = self.dy.to(dev).double()
        if drop_pixel:
            d = d.clone()
            d[-1, -1, -1, :] = 0
        return d if self.row.entry == "up" else d.permute(0, 3, 1, 2)


def reference(row, a, dy):
    """dw of the row's slice in float64: [Cout, Cx, ks, ks], or [Cout, Cx] for conv1x1"""
    if row.entry == "up":
        return R.ref_up_wgrad(a, dy)
    g = R.ref_wgrad(a, dy, row.stride)
    if row.ks == 1:
        g = g[:, :, 1:2, 1:2]
    return g.reshape(row.Cout, row.Cx) if row.entry == "1x1" else g


def einsum_reference(row, a, dy):
    """The same written tap by tap, without torch.nn.grad.conv2d_weight:
    dw[co, ci, ky, kx] = sum_{n, oy, ox} a[n, ci, s oy + ky - 1, s ox + kx - 1] dy[n, co, oy, ox]"""
    if row.entry == "up":
        n, h, w, c9 = dy.shape
        return torch.einsum("nchw,nhwtk->kct", a, dy.reshape(n, h, w, 9, c9 // 9)) \
            .reshape(c9 // 9, a.shape[1], 3, 3)
    s = row.stride
    Ho, Wo = dy.shape[2], dy.shape[3]
    p = F.pad(a, (1, 1, 1, 1))
    taps = [torch.einsum("nchw,nkhw->kc",
                         p[:, :, ky:ky + s * (Ho - 1) + 1:s, kx:kx + s * (Wo - 1) + 1:s], dy)
            for ky in range(3) for kx in range(3)]
    g = torch.stack(taps, 2).reshape(dy.shape[1], a.shape[1], 3, 3)
    if row.ks == 1:
        g = g[:, :, 1:2, 1:2]
    return g.reshape(row.Cout, row.Cx) if row.entry == "1x1" else g


def rel(a, b):
    """max |a - b| / max |b|"""
    return ((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300)).item()


def bias_reference(ops, dev="cpu"):
    return ops.dy64(dev).sum(dim=(0, 2, 3))
