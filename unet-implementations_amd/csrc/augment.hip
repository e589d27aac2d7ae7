// augment.hip — online augmentation of a uint8 training batch, one launch per batch:
//
//   unet_augment_u8   image [N,H,W,3] + mask [N,H,W] (uint8)  ->  an augmented pair of the same
//                     shape, from one fp32 record of 24 values and one 4-word random record per
//                     sample, both read ON THE DEVICE (a launch captured in a HIP graph follows
//                     new records on replay).
//
// It stands where the reference runs data_augmentation/src/augment_dataset.py offline on the CPU
// and stores a fixed augmented set.  The semantics are defined by this project (the reference's
// augmentation library is not a dependency): DESIGN §12 and the comment of unet_augment_u8 in
// include/unet_hip.h.  One inverse homography resamples the image once (bilinear, taps outside
// the image contribute 0) and the mask once (nearest, a border value outside); a rectangular
// hole, a gain / offset per channel, a gray switch, Gaussian noise and salt / pepper follow.
//
// The arithmetic is normative: every fp32 operation is rounded on its own (contraction is off for the
// whole file; hipcc would fuse multiply-adds otherwise), so a restatement with the same
// operation order reproduces the bytes.  Range tests are made in float BEFORE any conversion to
// an integer: a NaN, infinite or huge coordinate fails them and never becomes an index.
//
// The kernel gathers (four 3-byte taps per output pixel): inputs and outputs must not overlap.
// 8 x 512 x 512 moves 17 MB; the call is bound by launch and gather latency, not by bandwidth,
// and is written plainly.
#include "common.h"

// no fused multiply-adds anywhere below: hipcc contracts device code by default
#pragma clang fp contract(off)

namespace {

constexpr int AUG_PARAMS = 24;
constexpr int AUG_MAX_DIM = 32768;             // (float)H, (float)W exact; indices fit int
constexpr long long AUG_MAX_PIXELS = 1ll << 30;

// Philox4x32-10 (Salmon et al., SC'11): counter c[4], key k[2] -> four random words.
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3,
                                              unsigned k0, unsigned k1, unsigned (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// Box-Muller on one pair of words: u1 = ((a >> 8) + 1) 2^-24 in (0, 1], u2 = (b >> 8) 2^-24 in
// [0, 1) (both exact in fp32), r = sqrt(-2 ln u1), z = r cos(2 pi u2) and r sin(2 pi u2).
__device__ __forceinline__ void box_muller(unsigned a, unsigned b, float& zc, float& zs) {
#pragma clang fp contract(off)
  const float u1 = (float)((a >> 8) + 1u) * 5.9604644775390625e-8f;
  const float t2 = (float)(b >> 8) * 1.1920928955078125e-7f;      // 2 u2, exact
  const float r = sqrtf(-2.f * logf(u1));
  zc = r * cospif(t2);
  zs = r * sinpif(t2);
}

// one tap of the bilinear gather: 0 unless the tap lies inside the image
__device__ __forceinline__ void tap3(const unsigned char* __restrict__ img, bool ok, int y, int x,
                                     int W, float (&p)[3]) {
  p[0] = p[1] = p[2] = 0.f;
  if (ok) {
    const unsigned char* s = img + ((size_t)y * W + x) * 3;
    p[0] = (float)s[0]; p[1] = (float)s[1]; p[2] = (float)s[2];
  }
}

struct AugPixel { unsigned char c[3]; unsigned char m; };

// output pixel (i, j) of one sample; `pix` is its index i W + j in the sample (the counter of the
// random words: the result depends on (seed, pixel) only)
template <bool MASK>
__device__ __forceinline__ AugPixel augment_pixel(const unsigned char* __restrict__ img,
                                                  const unsigned char* __restrict__ msk,
                                                  const float (&r)[AUG_PARAMS], unsigned seed_lo,
                                                  unsigned seed_hi, unsigned pepper_thr,
                                                  unsigned salt_thr, bool noise, int i, int j,
                                                  long long pix, int H, int W) {
#pragma clang fp contract(off)
  const float xc = ((float)j + 0.5f), yc = ((float)i + 0.5f);
  const float den = (((r[6] * xc) + (r[7] * yc)) + r[8]);
  const float u = __fdiv_rn((((r[0] * xc) + (r[1] * yc)) + r[2]), den);
  const float v = __fdiv_rn((((r[3] * xc) + (r[4] * yc)) + r[5]), den);
  const bool front = den > 0.f;                 // false for NaN as well
  const float Wf = (float)W, Hf = (float)H;
  const bool hole = (float)j >= r[15] && (float)j < r[17] && (float)i >= r[16] && (float)i < r[18];

  float s[3];
  AugPixel o;
  if (hole) {
    s[0] = s[1] = s[2] = r[19];
  } else {
    const float fx = (u - 0.5f), fy = (v - 0.5f);
    const float x0 = floorf(fx), y0 = floorf(fy);
    // every test in float: NaN compares false, +-inf and huge values fail the bounds
    const bool xa = x0 >= 0.f && x0 < Wf, xb = x0 >= -1.f && x0 < Wf - 1.f;
    const bool ya = y0 >= 0.f && y0 < Hf, yb = y0 >= -1.f && y0 < Hf - 1.f;
    s[0] = s[1] = s[2] = 0.f;
    if (front && (xa || xb) && (ya || yb)) {    // otherwise no tap is inside: the sum is 0
      const float ax = (fx - x0), ay = (fy - y0);
      const int xi = (int)x0, yi = (int)y0;     // in [-1, W - 1] x [-1, H - 1] here
      float p00[3], p01[3], p10[3], p11[3];
      tap3(img, ya && xa, yi, xi, W, p00);
      tap3(img, ya && xb, yi, xi + 1, W, p01);
      tap3(img, yb && xa, yi + 1, xi, W, p10);
      tap3(img, yb && xb, yi + 1, xi + 1, W, p11);
      const float bx = (1.f - ax), by = (1.f - ay);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float top = ((bx * p00[c]) + (ax * p01[c]));
        const float bot = ((bx * p10[c]) + (ax * p11[c]));
        s[c] = ((by * top) + (ay * bot));
      }
    }
  }
  if (MASK) {
    if (hole) {
      o.m = (unsigned char)fminf(fmaxf(r[21], 0.f), 255.f);
    } else {
      const float mx = floorf(u), my = floorf(v);
      const bool in = front && mx >= 0.f && mx < Wf && my >= 0.f && my < Hf;
      o.m = in ? msk[(size_t)(int)my * W + (int)mx]
               : (unsigned char)fminf(fmaxf(r[20], 0.f), 255.f);
    }
  } else {
    o.m = 0;
  }

  float a[3];
#pragma unroll
  for (int c = 0; c < 3; ++c)
    a[c] = fminf(fmaxf(((r[9] * s[c]) + r[10 + c]), 0.f), 255.f);
  if (r[13] != 0.f) {
    const float g = (((0.299f * a[0]) + (0.587f * a[1])) + (0.114f * a[2]));
    a[0] = a[1] = a[2] = g;
  }
  const unsigned plo = (unsigned)pix, phi = (unsigned)(pix >> 32);
  if (noise && r[14] > 0.f) {                   // workgroup-uniform
    unsigned w[4];
    philox4x32_10(plo, phi, 0u, 0u, seed_lo, seed_hi, w);
    float z[4];
    box_muller(w[0], w[1], z[0], z[1]);
    box_muller(w[2], w[3], z[2], z[3]);
#pragma unroll
    for (int c = 0; c < 3; ++c) a[c] = (a[c] + (r[14] * z[c]));
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) o.c[c] = (unsigned char)fminf(fmaxf(rintf(a[c]), 0.f), 255.f);
  if (noise && (pepper_thr | salt_thr)) {       // workgroup-uniform
    unsigned w[4];
    philox4x32_10(plo, phi, 1u, 0u, seed_lo, seed_hi, w);
    if (w[0] < pepper_thr) o.c[0] = o.c[1] = o.c[2] = 0;
    else if (salt_thr != 0u && w[0] >= 0u - salt_thr) o.c[0] = o.c[1] = o.c[2] = 255;
  }
  return o;
}

// grid (pixel tiles, N), 256 threads.  VEC: W % 4 == 0 and 4-byte aligned outputs, so a thread
// owns four pixels of one row: one 12-byte image store and one 4-byte mask store.
template <bool VEC, bool MASK>
__global__ __launch_bounds__(256) void augment_u8_kernel(
    const unsigned char* __restrict__ image, const unsigned char* __restrict__ mask,
    unsigned char* __restrict__ image_out, unsigned char* __restrict__ mask_out,
    const float* __restrict__ params, const unsigned* __restrict__ rng, int H, int W) {
  const int n = blockIdx.y;
  const int HW = H * W;
  constexpr int NV = VEC ? 4 : 1;
  // the record: a workgroup-uniform address
  float r[AUG_PARAMS];
#pragma unroll
  for (int k = 0; k < AUG_PARAMS; ++k) r[k] = params[(size_t)n * AUG_PARAMS + k];
  unsigned seed_lo = 0, seed_hi = 0, pepper_thr = 0, salt_thr = 0;
  const bool noise = rng != nullptr;
  if (noise) {
    seed_lo = rng[4 * n]; seed_hi = rng[4 * n + 1];
    pepper_thr = rng[4 * n + 2]; salt_thr = rng[4 * n + 3];
  }
  const int p = (blockIdx.x * 256 + threadIdx.x) * NV;
  if (p >= HW) return;
  const unsigned char* img = image + (size_t)n * HW * 3;
  const unsigned char* msk = MASK ? mask + (size_t)n * HW : nullptr;
  const int i = p / W, j = p - i * W;           // VEC: the four pixels share row i
  AugPixel o[NV];
#pragma unroll
  for (int q = 0; q < NV; ++q)
    o[q] = augment_pixel<MASK>(img, msk, r, seed_lo, seed_hi, pepper_thr, salt_thr, noise, i,
                               j + q, (long long)p + q, H, W);
  unsigned char* io = image_out + ((size_t)n * HW + p) * 3;
  if constexpr (VEC) {
    struct alignas(4) U3 { unsigned a, b, c; };
    U3 w;
    w.a = o[0].c[0] | (o[0].c[1] << 8) | (o[0].c[2] << 16) | ((unsigned)o[1].c[0] << 24);
    w.b = o[1].c[1] | (o[1].c[2] << 8) | (o[2].c[0] << 16) | ((unsigned)o[2].c[1] << 24);
    w.c = o[2].c[2] | (o[3].c[0] << 8) | (o[3].c[1] << 16) | ((unsigned)o[3].c[2] << 24);
    *reinterpret_cast<U3*>(io) = w;
    if (MASK)
      *reinterpret_cast<uchar4*>(mask_out + (size_t)n * HW + p) =
          make_uchar4(o[0].m, o[1].m, o[2].m, o[3].m);
  } else {
    io[0] = o[0].c[0]; io[1] = o[0].c[1]; io[2] = o[0].c[2];
    if (MASK) mask_out[(size_t)n * HW + p] = o[0].m;
  }
}

bool aug_aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// [a, a + an) and [b, b + bn) share a byte
bool aug_overlap(const void* a, size_t an, const void* b, size_t bn) {
  if (!a || !b) return false;
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + bn && y < x + an;
}

}  // namespace

extern "C" int unet_augment_params_per_sample(void) { return AUG_PARAMS; }

extern "C" int unet_augment_u8(const uint8_t* image, const uint8_t* mask, uint8_t* image_out,
                               uint8_t* mask_out, const float* params, const uint32_t* rng, int N,
                               int H, int W, unet_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  UNET_REQUIRE(image && image_out && params, "augment_u8: null pointer (image, image_out, params)");
  UNET_REQUIRE(!mask || mask_out, "augment_u8: a mask was given without mask_out");
  UNET_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0 && H <= AUG_MAX_DIM && W <= AUG_MAX_DIM &&
                   (long long)H * W <= AUG_MAX_PIXELS,
               "augment_u8: bad shape (N in 1..65535, H, W in 1..32768, H * W <= 2^30)");
  const size_t px = (size_t)N * H * W;
  const void* outs[2] = {image_out, mask ? mask_out : nullptr};
  const size_t out_bytes[2] = {px * 3, px};
  const void* ins[4] = {image, mask, params, rng};
  const size_t in_bytes[4] = {px * 3, px, (size_t)N * AUG_PARAMS * sizeof(float),
                              (size_t)N * 4 * sizeof(uint32_t)};
  for (int o = 0; o < 2; ++o)
    for (int i = 0; i < 4; ++i)
      UNET_REQUIRE(!aug_overlap(outs[o], out_bytes[o], ins[i], in_bytes[i]),
                   "augment_u8: an output overlaps an input (the kernel gathers; it cannot run "
                   "in place)");
  UNET_REQUIRE(!aug_overlap(outs[0], out_bytes[0], outs[1], out_bytes[1]),
               "augment_u8: image_out overlaps mask_out");
  const bool vec = (W % 4 == 0) && aug_aligned4(image_out) && (!mask || aug_aligned4(mask_out));
  const long long HW = (long long)H * W;
  const dim3 grid((unsigned)ceil_div64(HW, 256ll * (vec ? 4 : 1)), N), block(256);
  if (vec && mask)
    hipLaunchKernelGGL((augment_u8_kernel<true, true>), grid, block, 0, stream, image, mask,
                       image_out, mask_out, params, rng, H, W);
  else if (vec)
    hipLaunchKernelGGL((augment_u8_kernel<true, false>), grid, block, 0, stream, image, mask,
                       image_out, mask_out, params, rng, H, W);
  else if (mask)
    hipLaunchKernelGGL((augment_u8_kernel<false, true>), grid, block, 0, stream, image, mask,
                       image_out, mask_out, params, rng, H, W);
  else
    hipLaunchKernelGGL((augment_u8_kernel<false, false>), grid, block, 0, stream, image, mask,
                       image_out, mask_out, params, rng, H, W);
  UNET_CHECK_LAUNCH("augment_u8");
  return UNET_OK;
}
