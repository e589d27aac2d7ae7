// augment.hip — online augmentation of a uint8 training batch, one launch per batch:
//
//   unet_augment_u8   image [N,H,W,3] + mask [N,H,W] (uint8)  ->  an augmented pair of the same
//                     shape, from one fp32 record of 24 values and one 4-word random record per
//                     sample, both read ON THE DEVICE (a launch captured in a HIP graph follows
//                     new records on replay).
//
//   unet_elastic_field      the displacement field of the elastic samples of a batch: uniform
//                           noise from Philox stream 2, smoothed by a separable Gaussian whose
//                           taps come from the record, through two LDS tiles (no exp on the device)
//   unet_augment_warp_u8    unet_augment_u8 behind a per-pixel warp of the output frame (elastic /
//                           grid / optical distortion, a second record of 64 floats per sample);
//                           the same pixel function, instantiated with the warp stage
//
// It stands where the reference runs data_augmentation/src/augment_dataset.py offline on the CPU
// and stores a fixed augmented set.  The semantics are defined by this project (the reference's
// augmentation library is not a dependency): DESIGN §12 and the comment of unet_augment_u8 in
// include/unet_hip.h.  One inverse homography resamples the image once (bilinear, taps outside
// the image contribute 0) and the mask once (nearest, a border value outside); a rectangular
// hole, a gain / offset per channel, a gray switch, Gaussian noise and salt / pepper follow.
//
// The arithmetic is normative: every fp32 operation is rounded on its own (contraction is off for
// the whole file; hipcc would fuse multiply-adds otherwise), so a restatement with the same
// operation order reproduces the bytes.  Range tests are made in float BEFORE any conversion to
// an integer: a NaN, infinite or huge coordinate fails them and never becomes an index.
//
// The kernel gathers (four 3-byte taps per output pixel): inputs and outputs must not overlap.
// 8 x 512 x 512 moves 17 MB; the call is bound by launch and gather latency, not by bandwidth,
// and is written plainly.
#include "augment_common.h"

// no fused multiply-adds anywhere below: hipcc contracts device code by default
#pragma clang fp contract(off)

namespace {

constexpr int AUG_PARAMS = 24;
constexpr int AUG_WARP = 64;                   // floats per warp record (layout: unet_hip.h)
constexpr int AUG_MAX_R = 16;                  // largest radius of the Gaussian of the field
constexpr int AUG_MAX_K = 8;                   // most cells per axis of the grid distortion

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

// one axis of the grid distortion: cell k = min((int)floor(c invcell), K - 1), then a_k c + b_k.
// The clamp is made in float, before the conversion, and to the record's eight slots whatever K
// says, so no record indexes past its own 64 floats.
__device__ __forceinline__ float grid_axis(const float* __restrict__ w, float c, float Kf,
                                           float invcell, int a_at) {
#pragma clang fp contract(off)
  const float t = floorf((c * invcell));
  const float top = fminf(fmaxf(Kf, 1.f), (float)AUG_MAX_K) - 1.f;
  const int k = (int)fminf(fmaxf(t, 0.f), top);             // fmaxf(NaN, 0) = 0
  return ((w[a_at + k] * c) + w[a_at + AUG_MAX_K + k]);
}

// the warp stage: output pixel centre (xc, yc) -> (xw, yw).  `w` is the sample's record and
// `mode` its first value (both workgroup-uniform), `fld` the sample's slice of the displacement
// field or null, `pix` the pixel index.
__device__ __forceinline__ void warp_point(const float* __restrict__ w, int mode,
                                           const float* __restrict__ fld, long long pix, float xc,
                                           float yc, float& xw, float& yw) {
#pragma clang fp contract(off)
  xw = xc; yw = yc;
  if (mode == 1) {
    float dx = 0.f, dy = 0.f;
    if (fld) {
      const float2 d = *reinterpret_cast<const float2*>(fld + 2 * pix);
      dx = d.x; dy = d.y;
    }
    xw = ((((w[1] * xc) + (w[2] * yc)) + w[3]) + dx);
    yw = ((((w[4] * xc) + (w[5] * yc)) + w[6]) + dy);
  } else if (mode == 2) {
    xw = grid_axis(w, xc, w[1], w[2], 8);
    yw = grid_axis(w, yc, w[3], w[4], 24);
  } else if (mode == 3) {
    const float cx = w[1], cy = w[2], k = w[3];
    const float ex = (xc - cx), ey = (yc - cy);
    const float xn = (ex * w[4]), yn = (ey * w[5]);
    const float r2 = ((xn * xn) + (yn * yn));
    const float kr = (k * r2);
    const float f = ((1.f + kr) + (kr * r2));
    xw = (cx + (ex * f));
    yw = (cy + (ey * f));
  }
}

// output pixel (i, j) of one sample; `pix` is its index i W + j in the sample (the counter of the
// random words: the result depends on (seed, pixel) only)
// WARP: the pixel centre goes through `warp_point` first (unet_augment_warp_u8); without it
// this is the pixel of unet_augment_u8.
template <bool MASK, bool WARP>
__device__ __forceinline__ AugPixel augment_pixel(const unsigned char* __restrict__ img,
                                                  const unsigned char* __restrict__ msk,
                                                  const float (&r)[AUG_PARAMS], unsigned seed_lo,
                                                  unsigned seed_hi, unsigned pepper_thr,
                                                  unsigned salt_thr, bool noise, int i, int j,
                                                  long long pix, int H, int W,
                                                  const float* __restrict__ wrec, int wmode,
                                                  const float* __restrict__ fld) {
#pragma clang fp contract(off)
  float xc = ((float)j + 0.5f), yc = ((float)i + 0.5f);
  if constexpr (WARP) {
    float xw, yw;
    warp_point(wrec, wmode, fld, pix, xc, yc, xw, yw);
    xc = xw; yc = yw;
  }
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
template <bool VEC, bool MASK, bool WARP>
__global__ __launch_bounds__(256) void augment_u8_kernel(
    const unsigned char* __restrict__ image, const unsigned char* __restrict__ mask,
    unsigned char* __restrict__ image_out, unsigned char* __restrict__ mask_out,
    const float* __restrict__ params, const unsigned* __restrict__ rng, int H, int W,
    const float* __restrict__ warp, const float* __restrict__ field) {
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
  const float* wrec = nullptr;
  const float* fld = nullptr;
  int wmode = 0;
  if constexpr (WARP) {                         // the mode: workgroup-uniform
    wrec = warp + (size_t)n * AUG_WARP;
    const float m = wrec[0];
    wmode = m == 1.f ? 1 : m == 2.f ? 2 : m == 3.f ? 3 : 0;
    if (field) fld = field + (size_t)n * HW * 2;
  }
  AugPixel o[NV];
#pragma unroll
  for (int q = 0; q < NV; ++q)
    o[q] = augment_pixel<MASK, WARP>(img, msk, r, seed_lo, seed_hi, pepper_thr, salt_thr, noise,
                                     i, j + q, (long long)p + q, H, W, wrec, wmode, fld);
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

// ---- the displacement field of the elastic samples --------------------------------------------
constexpr int FT = 32;                         // edge of the output tile
constexpr int FN = FT + 2 * AUG_MAX_R;         // 64: the tile plus its halo at the largest radius

// grid (tiles in x, tiles in y, N), 256 threads.  The uniform noise of the tile and its halo goes
// from Philox straight into LDS (it is indexed by the pixel, so neighbouring tiles regenerate the
// same halo values), the row pass into a second LDS array, the column pass to global memory.
// 48 KB of LDS; a sample whose record is not elastic costs its workgroups one scalar load.
__global__ __launch_bounds__(256) void elastic_field_kernel(
    float* __restrict__ field, const float* __restrict__ warp, const unsigned* __restrict__ rng,
    int H, int W) {
#pragma clang fp contract(off)
  const int n = blockIdx.z;
  const float* w = warp + (size_t)n * AUG_WARP;
  if (w[0] != 1.f) return;                      // workgroup-uniform
  __shared__ float noise[2][FN][FN];
  __shared__ float rowp[2][FN][FT];
  __shared__ float taps[AUG_MAX_R + 1];
  const int tid = threadIdx.x;
  const int R = (int)fminf(fmaxf(w[8], 0.f), (float)AUG_MAX_R);     // in float first; NaN -> 0
  const float alpha = w[7];
  if (tid <= AUG_MAX_R) taps[tid] = w[9 + tid];
  const int i0 = blockIdx.y * FT, j0 = blockIdx.x * FT;
  const int E = FT + 2 * R;                     // edge of the noise region, <= FN
  const bool have = rng != nullptr;
  unsigned seed_lo = 0, seed_hi = 0;
  if (have) { seed_lo = rng[4 * n]; seed_hi = rng[4 * n + 1]; }
  for (int e = tid; e < E * E; e += 256) {
    const int a = e / E, b = e - a * E;
    const int i = i0 - R + a, j = j0 - R + b;
    float n0 = 0.f, n1 = 0.f;                   // outside the image, or without rng: exactly 0
    if (have && i >= 0 && i < H && j >= 0 && j < W) {
      const long long pix = (long long)i * W + j;
      unsigned wd[4];
      philox4x32_10((unsigned)pix, (unsigned)(pix >> 32), 2u, 0u, seed_lo, seed_hi, wd);
      n0 = ((2.f * ((float)(wd[0] >> 8) * 5.9604644775390625e-8f)) - 1.f);
      n1 = ((2.f * ((float)(wd[1] >> 8) * 5.9604644775390625e-8f)) - 1.f);
    }
    noise[0][a][b] = n0;
    noise[1][a][b] = n1;
  }
  __syncthreads();
  for (int e = tid; e < E * FT; e += 256) {     // row pass: every row of the region, 32 columns
    const int a = e / FT, c = e - a * FT;
    float s0 = 0.f, s1 = 0.f;
    for (int t = -R; t <= R; ++t) {
      const float g = taps[t < 0 ? -t : t];
      s0 = (s0 + (g * noise[0][a][c + R + t]));
      s1 = (s1 + (g * noise[1][a][c + R + t]));
    }
    rowp[0][a][c] = s0;
    rowp[1][a][c] = s1;
  }
  __syncthreads();
  for (int e = tid; e < FT * FT; e += 256) {    // column pass, times alpha
    const int a = e / FT, c = e - a * FT;
    const int i = i0 + a, j = j0 + c;
    if (i >= H || j >= W) continue;
    float s0 = 0.f, s1 = 0.f;
    for (int t = -R; t <= R; ++t) {
      const float g = taps[t < 0 ? -t : t];
      s0 = (s0 + (g * rowp[0][a + R + t][c]));
      s1 = (s1 + (g * rowp[1][a + R + t][c]));
    }
    float* o = field + (((size_t)n * H + i) * W + j) * 2;
    *reinterpret_cast<float2*>(o) = make_float2((alpha * s0), (alpha * s1));
  }
}

// the checks and the launch of both gather entry points; `warped` is unet_augment_warp_u8
int augment_launch(const char* name, bool warped, const uint8_t* image, const uint8_t* mask,
                   uint8_t* image_out, uint8_t* mask_out, const float* params,
                   const uint32_t* rng, const float* warp, const float* field, int N, int H, int W,
                   hipStream_t stream) {
  UNET_REQUIRE(image && image_out && params, "%s: null pointer (image, image_out, params)", name);
  UNET_REQUIRE(!warped || warp, "%s: null pointer (warp)", name);
  UNET_REQUIRE(!mask || mask_out, "%s: a mask was given without mask_out", name);
  UNET_REQUIRE(aug_shape_ok(N, H, W),
               "%s: bad shape (N in 1..65535, H, W in 1..32768, H * W <= 2^30)", name);
  UNET_REQUIRE(!field || aug_aligned8(field), "%s: field is not 8-byte aligned", name);
  const size_t px = (size_t)N * H * W;
  const void* outs[2] = {image_out, mask ? mask_out : nullptr};
  const size_t out_bytes[2] = {px * 3, px};
  const void* ins[6] = {image, mask, params, rng, warp, field};
  const size_t in_bytes[6] = {px * 3, px, (size_t)N * AUG_PARAMS * sizeof(float),
                              (size_t)N * 4 * sizeof(uint32_t),
                              (size_t)N * AUG_WARP * sizeof(float), px * 2 * sizeof(float)};
  for (int o = 0; o < 2; ++o)
    for (int i = 0; i < 6; ++i)
      UNET_REQUIRE(!aug_overlap(outs[o], out_bytes[o], ins[i], in_bytes[i]),
                   "%s: an output overlaps an input (the kernel gathers; it cannot run in place)",
                   name);
  UNET_REQUIRE(!aug_overlap(outs[0], out_bytes[0], outs[1], out_bytes[1]),
               "%s: image_out overlaps mask_out", name);
  const bool vec = (W % 4 == 0) && aug_aligned4(image_out) && (!mask || aug_aligned4(mask_out));
  const long long HW = (long long)H * W;
  const dim3 grid((unsigned)ceil_div64(HW, 256ll * (vec ? 4 : 1)), N), block(256);
#define AUG_LAUNCH(VEC, MASK, WARP)                                                             \
  hipLaunchKernelGGL((augment_u8_kernel<VEC, MASK, WARP>), grid, block, 0, stream, image, mask, \
                     image_out, mask_out, params, rng, H, W, warp, field)
  if (warped) {
    if (vec && mask) AUG_LAUNCH(true, true, true);
    else if (vec) AUG_LAUNCH(true, false, true);
    else if (mask) AUG_LAUNCH(false, true, true);
    else AUG_LAUNCH(false, false, true);
  } else {
    if (vec && mask) AUG_LAUNCH(true, true, false);
    else if (vec) AUG_LAUNCH(true, false, false);
    else if (mask) AUG_LAUNCH(false, true, false);
    else AUG_LAUNCH(false, false, false);
  }
#undef AUG_LAUNCH
  UNET_CHECK_LAUNCH(name);
  return UNET_OK;
}

}  // namespace

extern "C" int unet_augment_params_per_sample(void) { return AUG_PARAMS; }

extern "C" int unet_augment_warp_params_per_sample(void) { return AUG_WARP; }

extern "C" int unet_augment_u8(const uint8_t* image, const uint8_t* mask, uint8_t* image_out,
                               uint8_t* mask_out, const float* params, const uint32_t* rng, int N,
                               int H, int W, unet_stream_t stream_) {
  return augment_launch("augment_u8", false, image, mask, image_out, mask_out, params, rng,
                        nullptr, nullptr, N, H, W, (hipStream_t)stream_);
}

extern "C" int unet_augment_warp_u8(const uint8_t* image, const uint8_t* mask, uint8_t* image_out,
                                    uint8_t* mask_out, const float* params, const uint32_t* rng,
                                    const float* warp, const float* field, int N, int H, int W,
                                    unet_stream_t stream_) {
  return augment_launch("augment_warp_u8", true, image, mask, image_out, mask_out, params, rng,
                        warp, field, N, H, W, (hipStream_t)stream_);
}

extern "C" int unet_elastic_field(float* field, const float* warp, const uint32_t* rng, int N,
                                  int H, int W, unet_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  UNET_REQUIRE(field && warp, "elastic_field: null pointer (field, warp)");
  UNET_REQUIRE(aug_shape_ok(N, H, W),
               "elastic_field: bad shape (N in 1..65535, H, W in 1..32768, H * W <= 2^30)");
  UNET_REQUIRE(aug_aligned8(field), "elastic_field: field is not 8-byte aligned");
  const size_t bytes = (size_t)N * H * W * 2 * sizeof(float);
  UNET_REQUIRE(!aug_overlap(field, bytes, warp, (size_t)N * AUG_WARP * sizeof(float)) &&
                   !aug_overlap(field, bytes, rng, (size_t)N * 4 * sizeof(uint32_t)),
               "elastic_field: field overlaps warp or rng");
  const dim3 grid((unsigned)ceil_div64(W, FT), (unsigned)ceil_div64(H, FT), N), block(256);
  hipLaunchKernelGGL(elastic_field_kernel, grid, block, 0, stream, field, warp, rng, H, W);
  UNET_CHECK_LAUNCH("elastic_field");
  return UNET_OK;
}
