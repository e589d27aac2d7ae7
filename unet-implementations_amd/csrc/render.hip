// render.hip — the pictures of the reference's evaluation as uint8 RGB panels, on the device:
//
//   unet_render_seg_panels    image | ground truth | prediction | error analysis | confidence
//                             overlays | Grad-CAM overlays of Our_UNet/utils/visualize.py, any
//                             ordered subset, one launch per batch.
//   unet_render_recon_panels  original | reconstruction | error map of create_comparison_image
//                             (AE_pretrained/reconstruction/utils/visualize.py:53-95), two launches.
//
// Both are streaming kernels: a thread takes 4 neighbouring pixels of one row, reads every operand
// once (16-byte loads where the row allows) and writes 12 bytes per requested panel.  Argmax,
// softmax and the error category are computed once per pixel and reused by every panel.  The
// output [B][H][P][W][3] is the row-concatenated picture [B * H][P * W][3] as it stands.
//
// Everything that decides a byte is integer arithmetic, except three places whose operation
// order the byte definitions fix (include/unet_hip.h); those use the explicitly rounded
// intrinsics, because the compiler would otherwise contract a multiply and an add into one FMA:
//   - the denormalised image: double(x) * std + mean, clip, * 255 in double (numpy's float32
//     array times float64 array);
//   - the [0, 1] image of the autoencoder: clamp, * 255 in fp32;
//   - the error map: d / max, then * 255, each rounded to fp32.
// The softmax is the one of unet_eval_maps (library exp, correctly rounded division).
#include "common.h"

namespace {

constexpr int RENDER_MAX_PANELS = 9;
constexpr long long RENDER_MAX_PIXELS = 1ll << 30;   // per image, as the evaluation kernels

enum RenderPanel {
  P_IMAGE = UNET_RENDER_IMAGE, P_GT = UNET_RENDER_GT, P_PRED = UNET_RENDER_PRED,
  P_ERROR = UNET_RENDER_ERROR, P_CONF0 = UNET_RENDER_CONF0, P_CONF1 = UNET_RENDER_CONF1,
  P_CONF2 = UNET_RENDER_CONF2, P_TARGET = UNET_RENDER_TARGET, P_HEAT = UNET_RENDER_HEAT,
  P_COUNT
};

// a colour is one word: r | g << 8 | b << 16
constexpr unsigned rgb(unsigned r, unsigned g, unsigned b) { return r | (g << 8) | (b << 16); }
constexpr unsigned REDS_LOW = rgb(255, 245, 240), REDS_HIGH = rgb(103, 0, 12);

// (a + b) >> 1 per byte, no carry between the bytes: the truncating half-sum of the alpha-0.5
// blends ((img * 0.5 + colour * 0.5).astype(uint8))
__device__ __forceinline__ unsigned half_sum(unsigned a, unsigned b) {
  return (a & b) + (((a ^ b) & 0xfefefefeu) >> 1);
}

// trunc(clip(double(x) * std + mean, 0, 1) * 255); NaN gives 0
__device__ __forceinline__ unsigned denorm_byte(float x, double std, double mean) {
  double v = __dadd_rn(__dmul_rn((double)x, std), mean);
  v = v > 0.0 ? (v > 1.0 ? 1.0 : v) : 0.0;
  return (unsigned)(int)__dmul_rn(v, 255.0);
}

// trunc(clamp(x, 0, 1) * 255) with an fp32 multiply; NaN gives 0
__device__ __forceinline__ unsigned unit_byte(float x) {
  x = x > 0.f ? (x > 1.f ? 1.f : x) : 0.f;
  return (unsigned)(int)__fmul_rn(x, 255.f);
}

// matplotlib's table index of a value in [0, 1]: min(int(v * 256), 255); v * 256 is exact
__device__ __forceinline__ int lut_index(float v) {
  v = v > 0.f ? (v > 1.f ? 1.f : v) : 0.f;        // NaN -> 0
  const int i = (int)(v * 256.f);
  return i > 255 ? 255 : i;
}

__device__ __forceinline__ unsigned class_colour(long long c) {
  return c == 1 ? rgb(255, 0, 0) : c == 2 ? rgb(0, 255, 0) : 0u;
}

// first maximum wins, like torch.argmax and unet_eval_maps
__device__ __forceinline__ int argmax3(float z0, float z1, float z2) {
  int am = 0;
  float best = z0;
  if (z1 > best) { best = z1; am = 1; }
  if (z2 > best) { best = z2; am = 2; }
  return am;
}

// colour of create_error_visualization's category (the rule of unet_eval_maps: 255 in the mask
// reads as background): true positive green, false positive red, false negative blue, wrong
// class yellow, none black
__device__ __forceinline__ unsigned error_colour(int am, long long t) {
  const bool pf = am > 0, gf = (t != 255) && (t > 0);
  if (pf && gf) return (long long)am == t ? rgb(0, 255, 0) : rgb(255, 255, 0);
  if (pf) return rgb(255, 0, 0);
  return gf ? rgb(0, 0, 255) : 0u;
}

// the jet table as 256 words in LDS; every thread of the 256 loads one entry
__device__ __forceinline__ void load_lut(unsigned* lut, const unsigned char* __restrict__ jet) {
  const int t = threadIdx.x;
  lut[t] = rgb(jet[3 * t], jet[3 * t + 1], jet[3 * t + 2]);
  __syncthreads();
}

// four RGB pixels <-> the 12 bytes they occupy, as three dwords
__device__ __forceinline__ void unpack12(unsigned w0, unsigned w1, unsigned w2, unsigned (&c)[4]) {
  c[0] = w0 & 0xffffffu;
  c[1] = (w0 >> 24) | ((w1 & 0xffffu) << 8);
  c[2] = (w1 >> 16) | ((w2 & 0xffu) << 16);
  c[3] = w2 >> 8;
}

// n <= 4 pixels of a uint8 [..][3] row at p (VEC: 4 pixels, p 4-byte aligned)
template <bool VEC>
__device__ __forceinline__ void load_rgb(const unsigned char* __restrict__ p, int n,
                                         unsigned (&c)[4]) {
  if constexpr (VEC) {
    const unsigned* w = reinterpret_cast<const unsigned*>(p);
    unpack12(w[0], w[1], w[2], c);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = j < n ? rgb(p[3 * j], p[3 * j + 1], p[3 * j + 2]) : 0u;
  }
}

template <bool VEC>
__device__ __forceinline__ void store_rgb(unsigned char* __restrict__ p, int n,
                                          const unsigned (&c)[4]) {
  if constexpr (VEC) {
    unsigned* w = reinterpret_cast<unsigned*>(p);
    w[0] = c[0] | (c[1] << 24);
    w[1] = (c[1] >> 8) | (c[2] << 16);
    w[2] = (c[2] >> 16) | (c[3] << 8);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < n) {
        p[3 * j] = (unsigned char)(c[j] & 255u);
        p[3 * j + 1] = (unsigned char)((c[j] >> 8) & 255u);
        p[3 * j + 2] = (unsigned char)(c[j] >> 16);
      }
  }
}

// n <= 4 floats of a row at p (VEC: 4 floats, p 16-byte aligned); absent ones read as 0
template <bool VEC>
__device__ __forceinline__ void load_f32(const float* __restrict__ p, int n, float (&v)[4]) {
  if constexpr (VEC) {
    const f32x4 a = ld4(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = a[j];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = j < n ? p[j] : 0.f;
  }
}

// the thread's pixel group: row y, first column x, n = min(4, W - x) pixels; false past the end
__device__ __forceinline__ bool pixel_group(int H, int W, int& y, int& x, int& n) {
  const int W4 = (W + 3) >> 2;
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= (long long)H * W4) return false;
  y = (int)(q / W4);
  x = (int)(q - (long long)y * W4) * 4;
  n = W - x < 4 ? W - x : 4;
  return true;
}

// n <= 4 pixels of an image as bytes: uint8 [H][W][3] of image b, or fp32 [3][H][W] converted
// by `to_byte(value, channel)`
template <bool VEC, typename F>
__device__ __forceinline__ void load_image(const void* __restrict__ image, bool is_u8, int b,
                                           size_t HW, size_t pix, int n, unsigned (&c)[4],
                                           F to_byte) {
  if (is_u8) {
    load_rgb<VEC>(static_cast<const unsigned char*>(image) + ((size_t)b * HW + pix) * 3, n, c);
  } else {
    const float* p = static_cast<const float*>(image) + (size_t)b * 3 * HW + pix;
    float r[4], g[4], bl[4];
    load_f32<VEC>(p, n, r);
    load_f32<VEC>(p + HW, n, g);
    load_f32<VEC>(p + 2 * HW, n, bl);
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = rgb(to_byte(r[j], 0), to_byte(g[j], 1), to_byte(bl[j], 2));
  }
}

struct SegArgs {
  const void* image;
  const float* logits;
  const void* mask;
  const float* heat;
  const unsigned char* jet;
  unsigned char* out;
  unsigned long long panels;   // 4 bits per panel: id + 1, in order
  int H, W, P;
  int image_u8, mask_u8, target_class;
  int need_soft;
};

// grid (ceil(H * ceil(W / 4) / 256), B), 256 threads.  VEC: W % 4 == 0 and every pointer aligned
// for the wide form of its loads / stores.
template <bool VEC>
__global__ __launch_bounds__(256) void render_seg_kernel(const SegArgs a) {
  __shared__ unsigned lut[256];
  load_lut(lut, a.jet);
  int y, x, n;
  if (!pixel_group(a.H, a.W, y, x, n)) return;
  const int b = blockIdx.y;
  const size_t HW = (size_t)a.H * a.W, pix = (size_t)y * a.W + x;

  unsigned img[4];
  load_image<VEC>(a.image, a.image_u8 != 0, b, HW, pix, n, img, [](float v, int ch) {
    const double std = ch == 0 ? 0.229 : ch == 1 ? 0.224 : 0.225;
    const double mean = ch == 0 ? 0.485 : ch == 1 ? 0.456 : 0.406;
    return denorm_byte(v, std, mean);
  });

  long long t[4] = {0, 0, 0, 0};
  if (a.mask) {
    if (a.mask_u8) {
      const unsigned char* m = static_cast<const unsigned char*>(a.mask) + (size_t)b * HW + pix;
      if constexpr (VEC) {
        const unsigned w = *reinterpret_cast<const unsigned*>(m);
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = (w >> (8 * j)) & 255u;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = j < n ? m[j] : 0;
      }
    } else {
      const long long* m = static_cast<const long long*>(a.mask) + (size_t)b * HW + pix;
      if constexpr (VEC) {
        typedef long long i64x2 __attribute__((ext_vector_type(2)));
        const i64x2 t01 = *reinterpret_cast<const i64x2*>(m);
        const i64x2 t23 = *reinterpret_cast<const i64x2*>(m + 2);
        t[0] = t01[0]; t[1] = t01[1]; t[2] = t23[0]; t[3] = t23[1];
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = j < n ? m[j] : 0;
      }
    }
  }

  int am[4] = {0, 0, 0, 0};
  float prob[3][4];
  if (a.logits) {
    const float* z = a.logits + (size_t)b * 3 * HW + pix;
    float z0[4], z1[4], z2[4];
    load_f32<VEC>(z, n, z0);
    load_f32<VEC>(z + HW, n, z1);
    load_f32<VEC>(z + 2 * HW, n, z2);
#pragma unroll
    for (int j = 0; j < 4; ++j) am[j] = argmax3(z0[j], z1[j], z2[j]);
    if (a.need_soft) {
      // softmax as unet_eval_maps (and F.softmax in fp32) computes it
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float m = fmaxf(z0[j], fmaxf(z1[j], z2[j]));
        const float e0 = expf(z0[j] - m), e1 = expf(z1[j] - m), e2 = expf(z2[j] - m);
        const float s = e0 + e1 + e2;
        prob[0][j] = __fdiv_rn(e0, s);
        prob[1][j] = __fdiv_rn(e1, s);
        prob[2][j] = __fdiv_rn(e2, s);
      }
    }
  }

  float heat[4] = {0.f, 0.f, 0.f, 0.f};
  if (a.heat) load_f32<VEC>(a.heat + (size_t)b * HW + pix, n, heat);

  unsigned char* row = a.out + ((size_t)b * a.H + y) * a.P * a.W * 3 + (size_t)x * 3;
  for (int k = 0; k < a.P; ++k) {
    const int id = (int)((a.panels >> (4 * k)) & 15u) - 1;
    unsigned c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      unsigned v;
      switch (id) {
        case P_IMAGE: v = img[j]; break;
        case P_GT: v = class_colour(t[j]); break;
        case P_PRED: v = class_colour(am[j]); break;
        case P_ERROR: v = half_sum(img[j], error_colour(am[j], t[j])); break;
        case P_CONF0: v = half_sum(img[j], lut[lut_index(prob[0][j])]); break;
        case P_CONF1: v = half_sum(img[j], lut[lut_index(prob[1][j])]); break;
        case P_CONF2: v = half_sum(img[j], lut[lut_index(prob[2][j])]); break;
        case P_TARGET:
          v = half_sum(img[j], t[j] == (long long)a.target_class ? REDS_HIGH : REDS_LOW);
          break;
        default: v = half_sum(img[j], lut[lut_index(heat[j])]); break;   // P_HEAT
      }
      c[j] = v;
    }
    store_rgb<VEC>(row + (size_t)k * a.W * 3, n, c);
  }
}

struct ReconArgs {
  const void* original;
  const float* recon;
  const unsigned char* jet;
  unsigned* maxima;            // [B]
  unsigned char* out;
  int H, W;
  int original_u8;
};

template <bool VEC>
__device__ __forceinline__ void recon_bytes(const ReconArgs& a, int b, size_t HW, size_t pix,
                                            int n, unsigned (&o)[4], unsigned (&r)[4]) {
  const auto to_byte = [](float v, int) { return unit_byte(v); };
  load_image<VEC>(a.original, a.original_u8 != 0, b, HW, pix, n, o, to_byte);
  load_image<VEC>(a.recon, false, b, HW, pix, n, r, to_byte);
}

__device__ __forceinline__ unsigned abs_diff(unsigned p, unsigned q) { return p > q ? p - q : q - p; }

// maxima[b] = max over the pixels and channels of image b of |original byte - reconstruction
// byte|: an integer maximum, the same whatever the order of the workgroups.  maxima is zeroed by
// the entry point.
template <bool VEC>
__global__ __launch_bounds__(256) void render_recon_max_kernel(const ReconArgs a) {
  __shared__ unsigned red[4];
  int y, x, n;
  unsigned m = 0;
  const int b = blockIdx.y;
  if (pixel_group(a.H, a.W, y, x, n)) {
    const size_t HW = (size_t)a.H * a.W, pix = (size_t)y * a.W + x;
    unsigned o[4], r[4];
    recon_bytes<VEC>(a, b, HW, pix, n, o, r);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < n) {
#pragma unroll
        for (int s = 0; s < 24; s += 8) m = max(m, abs_diff((o[j] >> s) & 255u, (r[j] >> s) & 255u));
      }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = max(max(red[0], red[1]), max(red[2], red[3]));
    if (m) atomicMax(&a.maxima[b], m);
  }
}

// out[b][y][0..2][x] = original | reconstruction | jet[gray(e)], e = trunc(d / max * 255) per
// channel, gray = OpenCV's fixed-point RGB2GRAY
template <bool VEC>
__global__ __launch_bounds__(256) void render_recon_kernel(const ReconArgs a) {
  __shared__ unsigned lut[256];
  load_lut(lut, a.jet);
  int y, x, n;
  if (!pixel_group(a.H, a.W, y, x, n)) return;
  const int b = blockIdx.y;
  const size_t HW = (size_t)a.H * a.W, pix = (size_t)y * a.W + x;
  unsigned o[4], r[4], c[4];
  recon_bytes<VEC>(a, b, HW, pix, n, o, r);
  const unsigned mx = a.maxima[b];
  const float fm = (float)mx;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    unsigned e[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const unsigned d = abs_diff((o[j] >> (8 * ch)) & 255u, (r[j] >> (8 * ch)) & 255u);
      e[ch] = mx ? (unsigned)(int)__fmul_rn(__fdiv_rn((float)d, fm), 255.f) : 0u;
    }
    const unsigned gray = (4899u * e[0] + 9617u * e[1] + 1868u * e[2] + 8192u) >> 14;
    c[j] = lut[gray > 255u ? 255u : gray];
  }
  unsigned char* row = a.out + ((size_t)b * a.H + y) * 3 * a.W * 3 + (size_t)x * 3;
  store_rgb<VEC>(row, n, o);
  store_rgb<VEC>(row + (size_t)a.W * 3, n, r);
  store_rgb<VEC>(row + (size_t)2 * a.W * 3, n, c);
}

bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

dim3 render_grid(int B, int H, int W) {
  return dim3((unsigned)ceil_div64((long long)H * ((W + 3) / 4), 256), (unsigned)B);
}

}  // namespace

extern "C" int unet_render_seg_panels(const void* image, int image_is_u8, const float* logits_nchw,
                                      const void* mask, int mask_is_u8, const float* heat,
                                      const uint8_t* jet, int target_class, uint64_t panels,
                                      uint8_t* out, int B, int H, int W, unet_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  UNET_REQUIRE(image && jet && out, "render_seg_panels: null pointer (image, jet or out)");
  UNET_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && (long long)H * W <= RENDER_MAX_PIXELS,
               "render_seg_panels: bad shape (B in 1..65535, H, W >= 1, H * W <= 2^30)");
  int P = 0, need_soft = 0;
  while (P < 16 && ((panels >> (4 * P)) & 15u)) ++P;
  UNET_REQUIRE(P >= 1 && P <= RENDER_MAX_PANELS && (P == 16 || (panels >> (4 * P)) == 0),
               "render_seg_panels: bad panel list (1..%d panels, 4 bits each: id + 1, no gaps)",
               RENDER_MAX_PANELS);
  for (int k = 0; k < P; ++k) {
    const int id = (int)((panels >> (4 * k)) & 15u) - 1;
    UNET_REQUIRE(id < P_COUNT, "render_seg_panels: unknown panel id %d", id);
    const bool needs_mask = id == P_GT || id == P_ERROR || id == P_TARGET;
    const bool needs_logits = id == P_PRED || id == P_ERROR || (id >= P_CONF0 && id <= P_CONF2);
    UNET_REQUIRE(!needs_mask || mask, "render_seg_panels: panel %d needs the mask", id);
    UNET_REQUIRE(!needs_logits || logits_nchw, "render_seg_panels: panel %d needs the logits", id);
    UNET_REQUIRE(id != P_HEAT || heat, "render_seg_panels: the heat panel needs the heat map");
    need_soft |= (id >= P_CONF0 && id <= P_CONF2);
  }
  const bool vec = (W % 4 == 0) && aligned_to(image, image_is_u8 ? 4 : 16) &&
                   aligned_to(logits_nchw, 16) && aligned_to(mask, mask_is_u8 ? 4 : 16) &&
                   aligned_to(heat, 16) && aligned_to(out, 4);
  SegArgs a;
  a.image = image; a.logits = logits_nchw; a.mask = mask; a.heat = heat; a.jet = jet; a.out = out;
  a.panels = panels; a.H = H; a.W = W; a.P = P;
  a.image_u8 = image_is_u8; a.mask_u8 = mask_is_u8; a.target_class = target_class;
  a.need_soft = need_soft;
  const dim3 grid = render_grid(B, H, W), block(256);
  if (vec)
    hipLaunchKernelGGL(render_seg_kernel<true>, grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL(render_seg_kernel<false>, grid, block, 0, stream, a);
  UNET_CHECK_LAUNCH("render_seg_panels");
  return UNET_OK;
}

extern "C" int unet_render_recon_panels(const void* original, int original_is_u8,
                                        const float* recon_nchw, const uint8_t* jet,
                                        uint32_t* maxima, uint8_t* out, int B, int H, int W,
                                        unet_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  UNET_REQUIRE(original && recon_nchw && jet && maxima && out, "render_recon_panels: null pointer");
  UNET_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && (long long)H * W <= RENDER_MAX_PIXELS,
               "render_recon_panels: bad shape (B in 1..65535, H, W >= 1, H * W <= 2^30)");
  UNET_REQUIRE(aligned_to(maxima, 4), "render_recon_panels: maxima must be 4-byte aligned");
  const bool vec = (W % 4 == 0) && aligned_to(original, original_is_u8 ? 4 : 16) &&
                   aligned_to(recon_nchw, 16) && aligned_to(out, 4);
  ReconArgs a;
  a.original = original; a.recon = recon_nchw; a.jet = jet; a.maxima = maxima; a.out = out;
  a.H = H; a.W = W; a.original_u8 = original_is_u8;
  UNET_HIP_CALL(hipMemsetAsync(maxima, 0, (size_t)B * sizeof(uint32_t), stream));
  const dim3 grid = render_grid(B, H, W), block(256);
  if (vec) {
    hipLaunchKernelGGL(render_recon_max_kernel<true>, grid, block, 0, stream, a);
    hipLaunchKernelGGL(render_recon_kernel<true>, grid, block, 0, stream, a);
  } else {
    hipLaunchKernelGGL(render_recon_max_kernel<false>, grid, block, 0, stream, a);
    hipLaunchKernelGGL(render_recon_kernel<false>, grid, block, 0, stream, a);
  }
  UNET_CHECK_LAUNCH("render_recon_panels");
  return UNET_OK;
}
