// augment_light.hip — the third stage of the online augmentation: ISO noise and the lighting group
// (shadow | sun flare | fog), applied to the uint8 image the gather (augment.hip) or the post
// stage (augment_post.hip) wrote:
//
//   ISO noise  ->  one of { shadow | sun flare | fog }
//
// from one fp32 record of 272 values per sample (`light`) read ON THE DEVICE, so a captured launch
// sequence follows new records on replay.  Two kernels behind one memset, the same launches for
// every batch:
//
//   light_stats_kernel   grid (64, N).  ISO samples: every workgroup sums s = max + min and s^2
//                        over its share of the sample in 64-bit integers and adds both to the
//                        sample's two sums in the workspace with integer atomics (exact, hence
//                        independent of the order).  Workgroups of every other sample return at
//                        once.
//   light_apply_kernel   grid (32 x 32 pixel tiles, N).  The record into LDS; for ISO, lambda
//                        from the sums and the 256-entry Poisson table into LDS; then per pixel
//                        ISO -> byte -> shadow | flare | fog blends -> byte.  Fog with a box of
//                        k >= 2 stages the tile plus halo in LDS (the whole chain applied once
//                        per staged pixel) and takes the box mean from there; no other mode
//                        stages anything.  The fog's points are binned per tile first: only
//                        those whose circle can reach the workgroup's pixels stay in LDS.
//
// The arithmetic is normative (the comment of unet_augment_light_u8 in include/unet_hip.h): every
// fp32 (and, in HLS, fp64) operation is rounded on its own, contraction is off for the whole file,
// and every count, step number and box size is range-tested in float before it becomes an index
// or a loop bound.
#include "augment_common.h"

#include <cfloat>

// no fused multiply-adds anywhere below: hipcc contracts device code by default
#pragma clang fp contract(off)

namespace {

constexpr int LIGHT = 272;                     // floats per record (layout: unet_hip.h)
constexpr int LT = 32;                         // edge of the output tile
constexpr int LIGHT_MAX_BOX = 9;               // largest box of the fog
constexpr int LE = LT + LIGHT_MAX_BOX - 1;     // 40: the tile plus its halo at the largest box
constexpr int STATS_WG = 64;                   // workgroups per sample of the statistics kernel
constexpr size_t LIGHT_SUM_BYTES = 2 * sizeof(unsigned long long);   // per sample
constexpr int L_BODY = 16;                     // first value of a mode's list
constexpr double HUE_BELOW_360 = 0x1.67fffffffffffp+8;               // the largest double below 360

// a record value as a count: clamped in float (a NaN becomes lo), then truncated
__device__ __forceinline__ int clamp_count(float v, float lo, float hi) {
  return (int)fminf(fmaxf(v, lo), hi);
}

// HLS is carried in fp64 (each operation rounded on its own): S and the hue's fraction are
// quotients, and only in fp64 does the way back return a channel that rounds to the fp32 value it
// came from - which is what makes the identity round trip, and the shadow's halving, exact.
__device__ __forceinline__ void hls_forward(const unsigned char (&p)[3], double& H, double& L,
                                            double& S) {
#pragma clang fp contract(off)
  const double r = (double)p[0], g = (double)p[1], b = (double)p[2];
  const double V = fmax(r, fmax(g, b)), m = fmin(r, fmin(g, b));
  const double s = (V + m), d = (V - m);
  L = __ddiv_rn(s, 510.0);
  S = d == 0.0 ? 0.0 : s <= 255.0 ? __ddiv_rn(d, s) : __ddiv_rn(d, (510.0 - s));
  double h = 0.0;
  if (d != 0.0) {
    if (V == r) h = (60.0 * __ddiv_rn((g - b), d));
    else if (V == g) h = (120.0 + (60.0 * __ddiv_rn((b - r), d)));
    else h = (240.0 + (60.0 * __ddiv_rn((r - g), d)));
  }
  if (h < 0.0) h = (h + 360.0);
  H = h;
}

// the channels are rounded to fp32, then to bytes
__device__ __forceinline__ void hls_back(double H, double L, double S, unsigned char (&p)[3]) {
#pragma clang fp contract(off)
  const double l2 = (510.0 * L);
  const double c = l2 <= 255.0 ? (l2 * S) : ((510.0 - l2) * S);
  const double hp = __ddiv_rn(H, 60.0);
  const double k = fmin(fmax(floor(hp), 0.0), 5.0);
  const double f = (hp - k);
  const int sector = (int)k;
  const double x = (sector & 1) ? (c * (1.0 - f)) : (c * f);
  const double lo = (0.5 * (l2 - c));
  const double hi = (lo + c), mid = (lo + x);
  const double o0 = sector == 0 || sector == 5 ? hi : sector == 1 || sector == 4 ? mid : lo;
  const double o1 = sector == 1 || sector == 2 ? hi : sector == 0 || sector == 3 ? mid : lo;
  const double o2 = sector == 3 || sector == 4 ? hi : sector == 2 || sector == 5 ? mid : lo;
  p[0] = to_byte((float)o0); p[1] = to_byte((float)o1); p[2] = to_byte((float)o2);
}

// grid (STATS_WG, N), 256 threads
__global__ __launch_bounds__(256) void light_stats_kernel(
    const unsigned char* __restrict__ image, const float* __restrict__ light,
    unsigned long long* __restrict__ sums, int H, int W) {
  const int n = blockIdx.y, k = blockIdx.x, tid = threadIdx.x;
  if (light[(size_t)n * LIGHT] != 1.f) return;                // workgroup-uniform
  __shared__ unsigned long long red[2][256];
  const unsigned char* img = image + (size_t)n * H * W * 3;
  const long long HW = (long long)H * W;
  unsigned long long s1 = 0, s2 = 0;
  for (long long e = (long long)k * 256 + tid; e < HW; e += STATS_WG * 256) {
    const unsigned char* q = img + (size_t)e * 3;
    const unsigned r = q[0], g = q[1], b = q[2];
    const unsigned s = max(r, max(g, b)) + min(r, min(g, b));
    s1 += s;
    s2 += s * s;
  }
  red[0][tid] = s1; red[1][tid] = s2;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) {
      red[0][tid] += red[0][tid + off];
      red[1][tid] += red[1][tid + off];
    }
    __syncthreads();
  }
  if (tid < 2 && red[tid][0] != 0ull) atomicAdd(&sums[2 * (size_t)n + tid], red[tid][0]);
}

// what the modes read of a record once per workgroup; every count is already range-tested
struct LightMode {
  bool iso;
  int mode;                                    // 0 none, 1 shadow, 2 flare, 3 fog
  int count;                                   // polygons, circles or points
  int steps;                                   // T of the flare's source
  int box;                                     // k of the fog
  unsigned seed_lo, seed_hi;
};

// ISO noise on one pixel, in place: hue by a normal, lightness by a Poisson draw from the table
__device__ __forceinline__ void iso_pixel(const float* rec, const float* cdf, long long pix,
                                          unsigned seed_lo, unsigned seed_hi,
                                          unsigned char (&p)[3]) {
#pragma clang fp contract(off)
  unsigned w[4];
  philox4x32_10((unsigned)pix, (unsigned)(pix >> 32), 3u, 0u, seed_lo, seed_hi, w);
  const float u1 = (float)((w[0] >> 8) + 1u) * 5.9604644775390625e-8f;
  const float t2 = (float)(w[1] >> 8) * 1.1920928955078125e-7f;     // 2 u2, exact
  const float z = sqrtf(-2.f * logf(u1)) * cospif(t2);
  const float uT = ((float)(w[2] >> 8) * 5.9604644775390625e-8f) * cdf[255];
  int lo = 0, hi = 256;                        // the number of c_j <= uT: c does not decrease
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cdf[mid] <= uT) lo = mid + 1; else hi = mid;
  }
  const float kf = (float)min(lo, 255);
  double H, L, S;
  hls_forward(p, H, L, S);
  double h2 = (H + ((double)rec[1] * (double)z));
  h2 = (h2 - (360.0 * floor(__ddiv_rn(h2, 360.0))));
  h2 = fmin(fmax(h2, 0.0), HUE_BELOW_360);
  const double L2 = fmin((L + (__ddiv_rn((double)kf, 255.0) * (1.0 - L))), 1.0);
  hls_back(h2, L2, S, p);
}

__device__ __forceinline__ bool in_circle(float xf, float yf, float cx, float cy, float r) {
#pragma clang fp contract(off)
  const float dx = (xf - cx), dy = (yf - cy);
  const float rr = fmaxf(r, 0.f);
  return ((dx * dx) + (dy * dy)) <= (rr * rr);               // a NaN anywhere: outside
}

__device__ __forceinline__ float blend(float a, float ov, float o) {
#pragma clang fp contract(off)
  return (float)to_byte(((a * ov) + ((1.f - a) * o)));
}

// The chain of input pixel (i, j) up to, and without, the fog's box mean.
__device__ __forceinline__ void light_pixel(const unsigned char* __restrict__ img, int i, int j,
                                            int W, const LightMode& md, const float* rec,
                                            const float* cdf, const float* pts,
                                            unsigned char (&p)[3]) {
#pragma clang fp contract(off)
  const long long pix = (long long)i * W + j;
  const unsigned char* src = img + (size_t)pix * 3;
  p[0] = src[0]; p[1] = src[1]; p[2] = src[2];
  if (md.iso) iso_pixel(rec, cdf, pix, md.seed_lo, md.seed_hi, p);
  if (md.mode == 1) {
    const float xc = ((float)j + 0.5f), yc = ((float)i + 0.5f);
    int inside = 0;
    for (int q = 0; q < md.count; ++q) {
      const float* v = rec + L_BODY + 10 * q;
      int cross = 0;
      for (int e = 0; e < 5; ++e) {
        const int e2 = e == 4 ? 0 : e + 1;
        const float x1 = v[2 * e], y1 = v[2 * e + 1], x2 = v[2 * e2], y2 = v[2 * e2 + 1];
        if ((y1 <= yc) != (y2 <= yc)) {
          const float t = __fdiv_rn((yc - y1), (y2 - y1));
          cross += xc < (x1 + (t * (x2 - x1)));
        }
      }
      inside += cross & 1;
    }
    if (inside) {
      double H, L, S;
      hls_forward(p, H, L, S);
      hls_back(H, (L * (inside == 2 ? 0.25 : 0.5)), S, p);
    }
  } else if (md.mode == 2) {
    const float xf = (float)j, yf = (float)i;
    float o[3] = {(float)p[0], (float)p[1], (float)p[2]};
    float ov[3] = {o[0], o[1], o[2]};
    for (int q = 0; q < md.count; ++q) {
      const float* v = rec + L_BODY + 7 * q;
      const bool in = in_circle(xf, yf, v[0], v[1], v[2]);
      const float a = v[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (in) ov[c] = v[4 + c];
        o[c] = blend(a, ov[c], o[c]);
      }
    }
    const float tm1 = (float)(md.steps - 1);
    const float rs1 = (rec[7] - 1.f);
    for (int t = 0; t < md.steps; ++t) {
      const float rt = (1.f + __fdiv_rn((rs1 * (float)t), tm1));
      const bool in = in_circle(xf, yf, rec[5], rec[6], rt);
      const float q = __fdiv_rn((float)(md.steps - 1 - t), tm1);
      const float a = ((q * q) * q);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (in) ov[c] = 255.f;
        o[c] = blend(a, ov[c], o[c]);
      }
    }
    p[0] = (unsigned char)o[0]; p[1] = (unsigned char)o[1]; p[2] = (unsigned char)o[2];
  } else if (md.mode == 3) {
    const float xf = (float)j, yf = (float)i;
    const float a = rec[6], a255 = (a * 255.f), na = (1.f - a), rad = rec[5];
    float o[3] = {(float)p[0], (float)p[1], (float)p[2]};
    for (int q = 0; q < md.count; ++q) {
      if (in_circle(xf, yf, pts[2 * q], pts[2 * q + 1], rad)) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = (float)to_byte((a255 + (na * o[c])));
      }
    }
    p[0] = (unsigned char)o[0]; p[1] = (unsigned char)o[1]; p[2] = (unsigned char)o[2];
  }
}

// grid (tiles in x, tiles in y, N), 256 threads
__global__ __launch_bounds__(256) void light_apply_kernel(
    const unsigned char* __restrict__ image, unsigned char* __restrict__ image_out,
    const float* __restrict__ light, const unsigned* __restrict__ rng,
    const unsigned long long* __restrict__ sums, int H, int W) {
#pragma clang fp contract(off)
  __shared__ float rec[LIGHT];
  __shared__ float cdf[256];
  __shared__ uchar4 tile[LE][LE];
  __shared__ float near_pts[2 * 128];
  __shared__ unsigned char near[128];
  const int n = blockIdx.z, tid = threadIdx.x;
  const int i0 = blockIdx.y * LT, j0 = blockIdx.x * LT;
  for (int e = tid; e < LIGHT; e += 256) rec[e] = light[(size_t)n * LIGHT + e];
  __syncthreads();
  LightMode md;                                // workgroup-uniform, as every branch on it
  md.iso = rec[0] == 1.f && rng != nullptr;
  md.mode = rec[3] == 1.f ? 1 : rec[3] == 2.f ? 2 : rec[3] == 3.f ? 3 : 0;
  md.count = md.mode == 1 ? clamp_count(rec[4], 0.f, 2.f)
           : md.mode == 2 ? clamp_count(rec[4], 0.f, 10.f)
           : md.mode == 3 ? clamp_count(rec[4], 0.f, 128.f) : 0;
  md.steps = clamp_count(rec[8], 2.f, 40.f);
  md.box = md.mode == 3 ? clamp_count(rec[7], 1.f, (float)LIGHT_MAX_BOX) : 1;
  md.seed_lo = md.seed_hi = 0u;
  if (md.iso) {
    md.seed_lo = rng[4 * n]; md.seed_hi = rng[4 * n + 1];
    if (tid == 0) {     // lambda in fp64 from the exact sums, then the table, one rounding each
      const double cnt = (double)((long long)H * W);
      const double mean = __ddiv_rn((double)sums[2 * (size_t)n], cnt);
      const double var = fmax((__ddiv_rn((double)sums[2 * (size_t)n + 1], cnt) - (mean * mean)), 0.0);
      const double sd = __ddiv_rn(__dsqrt_rn(var), 510.0);
      const float lam = (float)fmin(fmax((((double)rec[2] * 255.0) * sd), 0.0), 64.0);
      float t = 1.f, acc = 0.f;
      for (int k = 0; k < 256; ++k) {
        if (k > 0 && t != 0.f) {               // once 0 it stays 0
          t = __fdiv_rn((t * lam), (float)k);
          if (t < FLT_MIN) t = 0.f;
        }
        acc = (acc + t);
        cdf[k] = acc;
      }
    }
    __syncthreads();
  }
  const unsigned char* img = image + (size_t)n * H * W * 3;
  unsigned char* dst_n = image_out + (size_t)n * H * W * 3;

  // Fog: only the points whose circle can reach a pixel this workgroup evaluates stay, in their
  // order.  Those pixels lie within 35 of the tile's first pixel on either side (the tile, its
  // halo of at most 4, and what a reflection at the border brings back).  A point goes only if it
  // is farther than radius + 1 from that range on one axis, tested in fp64, and only for a radius
  // up to 2^20, where a pixel that far away fails the fp32 test of in_circle whatever the
  // rounding; a NaN anywhere keeps the point (in_circle then calls it outside).
  const float* pts = rec + L_BODY;
  if (md.mode == 3) {
    if (tid < 128) {
      bool keep = tid < md.count;
      if (keep && rec[5] <= 1048576.f) {
        const double reach = (double)fmaxf(rec[5], 0.f) + 1.0;
        const double cx = (double)rec[L_BODY + 2 * tid], cy = (double)rec[L_BODY + 2 * tid + 1];
        if (cx + reach < (double)(j0 - 36) || cx - reach > (double)(j0 + 36) ||
            cy + reach < (double)(i0 - 36) || cy - reach > (double)(i0 + 36)) keep = false;
      }
      near[tid] = keep;
    }
    __syncthreads();
    int kept = 0;
    for (int q = 0; q < md.count; ++q) {       // every thread counts: md.count stays uniform
      if (q == tid && near[q]) {
        near_pts[2 * kept] = rec[L_BODY + 2 * q];
        near_pts[2 * kept + 1] = rec[L_BODY + 2 * q + 1];
      }
      kept += near[q];
    }
    __syncthreads();
    md.count = kept;
    pts = near_pts;
  }

  if (md.box < 2) {     // no neighbourhood: pixel in, pixel out
    for (int e = tid; e < LT * LT; e += 256) {
      const int a = e / LT, c = e - a * LT;
      const int i = i0 + a, j = j0 + c;
      if (i >= H || j >= W) continue;
      unsigned char p[3];
      light_pixel(img, i, j, W, md, rec, cdf, pts, p);
      unsigned char* dst = dst_n + ((size_t)i * W + j) * 3;
      dst[0] = p[0]; dst[1] = p[1]; dst[2] = p[2];
    }
    return;
  }

  // fog with a box: the tile plus halo through the whole chain up to the last fog blend; a halo
  // pixel regenerates what its own tile computes (the random words are indexed by the pixel)
  const int before = md.box / 2;               // the window is -before .. box - 1 - before
  const int E = LT + md.box - 1;
  for (int e = tid; e < E * E; e += 256) {
    const int a = e / E, b = e - a * E;
    const int i = reflect(i0 - before + a, H), j = reflect(j0 - before + b, W);
    unsigned char p[3];
    light_pixel(img, i, j, W, md, rec, cdf, pts, p);
    tile[a][b] = make_uchar4(p[0], p[1], p[2], 0);
  }
  __syncthreads();
  const float area = (float)(md.box * md.box);
  for (int e = tid; e < LT * LT; e += 256) {
    const int a = e / LT, c = e - a * LT;
    const int i = i0 + a, j = j0 + c;
    if (i >= H || j >= W) continue;
    int s0 = 0, s1 = 0, s2 = 0;                // a sum of at most 81 bytes: exact in fp32 as well
    for (int dy = 0; dy < md.box; ++dy)
      for (int dx = 0; dx < md.box; ++dx) {
        const uchar4 q = tile[a + dy][c + dx];
        s0 += q.x; s1 += q.y; s2 += q.z;
      }
    unsigned char* dst = dst_n + ((size_t)i * W + j) * 3;
    dst[0] = to_byte(__fdiv_rn((float)s0, area));
    dst[1] = to_byte(__fdiv_rn((float)s1, area));
    dst[2] = to_byte(__fdiv_rn((float)s2, area));
  }
}

}  // namespace

extern "C" int unet_augment_light_params_per_sample(void) { return LIGHT; }

extern "C" size_t unet_augment_light_workspace_bytes(int N) {
  return N > 0 ? (size_t)N * LIGHT_SUM_BYTES : 0;
}

namespace {

// the checks and the launches of the three entry points: `stats` / `apply` name the kernels to run
int light_launch(const char* name, bool stats, bool apply, const uint8_t* image,
                 uint8_t* image_out, const float* light, const uint32_t* rng, void* workspace,
                 size_t workspace_bytes, int N, int H, int W, hipStream_t stream) {
  const size_t need = unet_augment_light_workspace_bytes(N);
  if (const int rc = aug_stage_check(name, "light", "fog", apply, image, image_out, light, LIGHT, rng, workspace,
                                     workspace_bytes, need, N, H, W))
    return rc;
  // workspace: sums [N][2] uint64 (zeroed here, every call)
  unsigned long long* sums = static_cast<unsigned long long*>(workspace);
  if (stats) {
    UNET_HIP_CALL(hipMemsetAsync(sums, 0, need, stream));
    hipLaunchKernelGGL(light_stats_kernel, dim3(STATS_WG, N), dim3(256), 0, stream, image, light,
                       sums, H, W);
    UNET_CHECK_LAUNCH(name);
  }
  if (apply) {
    const dim3 grid((unsigned)ceil_div64(W, LT), (unsigned)ceil_div64(H, LT), N);
    hipLaunchKernelGGL(light_apply_kernel, grid, dim3(256), 0, stream, image, image_out, light,
                       rng, sums, H, W);
    UNET_CHECK_LAUNCH(name);
  }
  return UNET_OK;
}

}  // namespace

extern "C" int unet_augment_light_u8(const uint8_t* image, uint8_t* image_out, const float* light,
                                     const uint32_t* rng, void* workspace, size_t workspace_bytes,
                                     int N, int H, int W, unet_stream_t stream) {
  return light_launch("augment_light_u8", true, true, image, image_out, light, rng, workspace,
                      workspace_bytes, N, H, W, (hipStream_t)stream);
}

extern "C" int unet_augment_light_stats(const uint8_t* image, const float* light, void* workspace,
                                        size_t workspace_bytes, int N, int H, int W,
                                        unet_stream_t stream) {
  return light_launch("augment_light_stats", true, false, image, nullptr, light, nullptr,
                      workspace, workspace_bytes, N, H, W, (hipStream_t)stream);
}

extern "C" int unet_augment_light_apply(const uint8_t* image, uint8_t* image_out,
                                        const float* light, const uint32_t* rng, void* workspace,
                                        size_t workspace_bytes, int N, int H, int W,
                                        unet_stream_t stream) {
  return light_launch("augment_light_apply", false, true, image, image_out, light, rng, workspace,
                      workspace_bytes, N, H, W, (hipStream_t)stream);
}
