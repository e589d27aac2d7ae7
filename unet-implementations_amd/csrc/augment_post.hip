// augment_post.hip — the second stage of the online augmentation: the photometric transforms that
// need more than the pixel itself, applied to the uint8 image the gather kernel (augment.hip)
// wrote:
//
//   HSV shift  ->  equalize | CLAHE  ->  Gaussian | motion blur  ->  salt / pepper
//
// from one fp32 record of 64 values per sample (`post`) read ON THE DEVICE, so a captured launch
// sequence follows new records on replay.  Two kernels, the same launches for every batch:
//
//   post_hist_kernel    grid (64, N).  Equalize samples: every workgroup histograms its share of
//                       the sample (three channels) in LDS and adds it to the sample's counts in
//                       the workspace with integer atomics.  CLAHE samples: workgroup k owns
//                       tile k, histograms its luma in LDS, clips, scans and writes the tile's
//                       256-byte LUT.  Workgroups of every other sample return at once.
//   post_apply_kernel   grid (32 x 32 pixel tiles, N).  LUTs into LDS, the tile plus the blur's
//                       halo into LDS as bytes (HSV and the histogram op applied once per staged
//                       pixel), the blur from LDS, salt / pepper, store.
//
// The arithmetic is normative (the comment of unet_augment_post_u8 in include/unet_hip.h): every
// fp32 operation is rounded on its own, contraction is off for the whole file, and every range
// test is made in float before a value becomes an index.
#include "augment_common.h"

// no fused multiply-adds anywhere below: hipcc contracts device code by default
#pragma clang fp contract(off)

namespace {

constexpr int POST = 64;                       // floats per record (layout: unet_hip.h)
constexpr int PT = 32;                         // edge of the output tile
constexpr int POST_MAX_R = 4;                  // largest blur radius
constexpr int PE = PT + 2 * POST_MAX_R;        // 40: the tile plus its halo at the largest radius
constexpr int HIST_WG = 64;                    // workgroups per sample of the histogram kernel,
                                               // and the most CLAHE tiles (8 x 8)
constexpr size_t POST_COUNT_BYTES = 3 * 256 * sizeof(unsigned);   // per sample
constexpr size_t POST_LUT_BYTES = HIST_WG * 256;                  // per sample
constexpr float HUE_BELOW_180 = 0x1.67fffep+7f;                   // the largest float below 180

// HueSaturationValue on one pixel, in place (hue in half-degrees, S and V in levels)
__device__ __forceinline__ void hsv_shift(float dh, float ds, float dv, unsigned char (&p)[3]) {
#pragma clang fp contract(off)
  const float r = (float)p[0], g = (float)p[1], b = (float)p[2];
  const float V = fmaxf(r, fmaxf(g, b)), m = fminf(r, fminf(g, b));
  const float d = (V - m);
  const float S = V == 0.f ? 0.f : __fdiv_rn((255.f * d), V);
  float h = 0.f;
  if (d != 0.f) {
    if (V == r) h = (30.f * __fdiv_rn((g - b), d));
    else if (V == g) h = (60.f + (30.f * __fdiv_rn((b - r), d)));
    else h = (120.f + (30.f * __fdiv_rn((r - g), d)));
  }
  if (h < 0.f) h = (h + 180.f);
  float h2 = (h + dh);
  h2 = (h2 - (180.f * floorf(__fdiv_rn(h2, 180.f))));
  h2 = fminf(fmaxf(h2, 0.f), HUE_BELOW_180);
  const float S2 = fminf(fmaxf((S + ds), 0.f), 255.f);
  const float V2 = fminf(fmaxf((V + dv), 0.f), 255.f);
  const float c = __fdiv_rn((V2 * S2), 255.f);
  const float hp = __fdiv_rn(h2, 30.f);
  const float k = fminf(fmaxf(floorf(hp), 0.f), 5.f);
  const float f = (hp - k);
  const float P = (V2 - c), Q = (V2 - (c * f)), T = (V2 - (c * (1.f - f)));
  const int sector = (int)k;
  const float o0 = sector == 0 || sector == 5 ? V2 : sector == 1 ? Q : sector == 4 ? T : P;
  const float o1 = sector == 1 || sector == 2 ? V2 : sector == 0 ? T : sector == 3 ? Q : P;
  const float o2 = sector == 3 || sector == 4 ? V2 : sector == 2 ? T : sector == 5 ? Q : P;
  p[0] = to_byte(o0); p[1] = to_byte(o1); p[2] = to_byte(o2);
}

__device__ __forceinline__ int luma(const unsigned char (&p)[3]) {
#pragma clang fp contract(off)
  return (int)to_byte((((0.299f * (float)p[0]) + (0.587f * (float)p[1])) + (0.114f * (float)p[2])));
}

// the input pixel behind the HSV stage
__device__ __forceinline__ void load_hsv(const unsigned char* __restrict__ img, size_t pix,
                                         bool hsv, float dh, float ds, float dv,
                                         unsigned char (&p)[3]) {
  const unsigned char* s = img + pix * 3;
  p[0] = s[0]; p[1] = s[1]; p[2] = s[2];
  if (hsv) hsv_shift(dh, ds, dv, p);
}

// The histogram op of a record: 0 none, 1 equalize, 2 CLAHE with (ty, tx) set.  A CLAHE record
// whose grid is not two integers in 1..8 that divide the shape is "none".  Workgroup-uniform.
__device__ __forceinline__ int hist_op(const float* rec, int H, int W, int& ty, int& tx) {
  ty = tx = 1;
  if (rec[4] == 1.f) return 1;
  if (rec[4] != 2.f) return 0;
  const float fy = rec[6], fx = rec[7];
  if (!(fy >= 1.f && fy <= 8.f && fx >= 1.f && fx <= 8.f)) return 0;      // NaN fails
  if (fy != floorf(fy) || fx != floorf(fx)) return 0;
  if (H % (int)fy != 0 || W % (int)fx != 0) return 0;
  ty = (int)fy; tx = (int)fx;
  return 2;
}

// inclusive scan of one value per thread over the 256 threads, through s[256]; s holds the scan
// on return (s[255] is the total)
__device__ __forceinline__ unsigned scan256(unsigned* s, int tid, unsigned v) {
  __syncthreads();                              // s may still be read from an earlier scan
  s[tid] = v;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const unsigned a = tid >= off ? s[tid - off] : 0u;
    __syncthreads();
    s[tid] += a;
    __syncthreads();
  }
  return s[tid];
}

// grid (HIST_WG, N), 256 threads: four waves, one sub-histogram per wave and channel in LDS (LDS
// atomics of one wave never meet another wave's), merged at the end.
__global__ __launch_bounds__(256) void post_hist_kernel(
    const unsigned char* __restrict__ image, const float* __restrict__ post,
    unsigned* __restrict__ counts, unsigned char* __restrict__ luts, int H, int W) {
#pragma clang fp contract(off)
  const int n = blockIdx.y, k = blockIdx.x, tid = threadIdx.x;
  const float* rec = post + (size_t)n * POST;
  int ty, tx;
  const int op = hist_op(rec, H, W, ty, tx);
  if (op == 0 || (op == 2 && k >= ty * tx)) return;         // workgroup-uniform
  __shared__ unsigned sub[4][3][256];
  __shared__ unsigned scan[256];
  for (int e = tid; e < 4 * 3 * 256; e += 256) (&sub[0][0][0])[e] = 0u;
  __syncthreads();
  const bool hsv = rec[0] == 1.f;
  const float dh = rec[1], ds = rec[2], dv = rec[3];
  const unsigned char* img = image + (size_t)n * H * W * 3;
  const int wave = tid >> 6;
  unsigned char p[3];
  if (op == 1) {
    const long long HW = (long long)H * W;
    for (long long e = (long long)k * 256 + tid; e < HW; e += HIST_WG * 256) {
      load_hsv(img, (size_t)e, hsv, dh, ds, dv, p);
#pragma unroll
      for (int c = 0; c < 3; ++c) atomicAdd(&sub[wave][c][p[c]], 1u);
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const unsigned s = sub[0][c][tid] + sub[1][c][tid] + sub[2][c][tid] + sub[3][c][tid];
      if (s) atomicAdd(&counts[((size_t)n * 3 + c) * 256 + tid], s);
    }
    return;
  }
  // CLAHE: tile k
  const int th = H / ty, tw = W / tx, area = th * tw;
  const int r0 = (k / tx) * th, c0 = (k % tx) * tw;
  for (int e = tid; e < area; e += 256) {
    const int a = e / tw, b = e - a * tw;
    load_hsv(img, (size_t)(r0 + a) * W + (c0 + b), hsv, dh, ds, dv, p);
    atomicAdd(&sub[wave][0][luma(p)], 1u);
  }
  __syncthreads();
  int h = (int)(sub[0][0][tid] + sub[1][0][tid] + sub[2][0][tid] + sub[3][0][tid]);
  const float t = fmaxf(floorf(__fdiv_rn((rec[5] * (float)area), 256.f)), 1.f);   // NaN -> 1
  const int climit = t >= (float)area ? area : (int)t;       // no bin holds more than area
  scan256(scan, tid, (unsigned)max(h - climit, 0));
  const int excess = (int)scan[255];
  h = min(h, climit);
  const int batch = excess / 256, resid = excess - 256 * batch;
  h += batch;
  if (resid > 0) {
    const int step = max(256 / resid, 1);
    if (tid % step == 0 && tid / step < resid) h += 1;
  }
  const unsigned cdf = scan256(scan, tid, (unsigned)h);
  const float scale = __fdiv_rn(255.f, (float)area);
  luts[((size_t)n * HIST_WG + k) * 256 + tid] =
      (unsigned char)fminf(rintf(((float)cdf * scale)), 255.f);
}

// grid (tiles in x, tiles in y, N), 256 threads
__global__ __launch_bounds__(256) void post_apply_kernel(
    const unsigned char* __restrict__ image, unsigned char* __restrict__ image_out,
    const float* __restrict__ post, const unsigned* __restrict__ rng,
    const unsigned* __restrict__ counts, const unsigned char* __restrict__ luts, int H, int W) {
#pragma clang fp contract(off)
  __shared__ float rec[POST];
  __shared__ __align__(16) unsigned char lut[POST_LUT_BYTES];
  __shared__ unsigned scan[256];
  __shared__ unsigned first;
  __shared__ uchar4 tile[PE][PE];
  __shared__ float rowp[PE][PT][3];
  const int n = blockIdx.z, tid = threadIdx.x;
  const int i0 = blockIdx.y * PT, j0 = blockIdx.x * PT;
  if (tid < POST) rec[tid] = post[(size_t)n * POST + tid];
  __syncthreads();
  int ty, tx;
  const int op = hist_op(rec, H, W, ty, tx);                 // workgroup-uniform, as all modes
  const bool hsv = rec[0] == 1.f;
  const float dh = rec[1], ds = rec[2], dv = rec[3];
  const int bm = rec[8] == 1.f ? 1 : rec[8] == 2.f ? 2 : 0;
  // the radius is clamped in float: NaN -> 1, and no value reaches past the record or the halo
  const int R = bm == 0 ? 0 : (int)fminf(fmaxf(rec[9], 1.f), bm == 1 ? 4.f : 3.f);

  if (op == 1) {        // the three LUTs of equalize from the sample's counts
    const unsigned total = (unsigned)(H * W);
    for (int c = 0; c < 3; ++c) {
      const unsigned v = counts[((size_t)n * 3 + c) * 256 + tid];
      const unsigned cdf = scan256(scan, tid, v);
      if (v > 0u && cdf == v) first = v;                     // the first non-empty bin
      __syncthreads();
      const unsigned h0 = first;
      unsigned char o = (unsigned char)tid;                  // one value only: unchanged
      if (h0 != total) {
        const float scale = __fdiv_rn(255.f, (float)(total - h0));
        o = cdf == 0u ? 0 : (unsigned char)fminf(rintf(((float)(cdf - h0) * scale)), 255.f);
      }
      lut[c * 256 + tid] = o;
    }
  } else if (op == 2) { // the tiles' LUTs as the histogram kernel wrote them
    const uint4* src = reinterpret_cast<const uint4*>(luts + (size_t)n * POST_LUT_BYTES);
    for (int e = tid; e < ty * tx * 16; e += 256) reinterpret_cast<uint4*>(lut)[e] = src[e];
  }
  __syncthreads();

  const unsigned char* img = image + (size_t)n * H * W * 3;
  const float inv_th = __fdiv_rn(1.f, (float)(H / ty)), inv_tw = __fdiv_rn(1.f, (float)(W / tx));
  const int E = PT + 2 * R;
  for (int e = tid; e < E * E; e += 256) {
    const int a = e / E, b = e - a * E;
    const int i = reflect(i0 - R + a, H), j = reflect(j0 - R + b, W);
    unsigned char p[3];
    load_hsv(img, (size_t)i * W + j, hsv, dh, ds, dv, p);
    if (op == 1) {
#pragma unroll
      for (int c = 0; c < 3; ++c) p[c] = lut[c * 256 + p[c]];
    } else if (op == 2) {
      const int Y = luma(p);
      const float fx = (((float)j * inv_tw) - 0.5f), fy = (((float)i * inv_th) - 0.5f);
      const float x1f = floorf(fx), y1f = floorf(fy);
      const float ax = (fx - x1f), ay = (fy - y1f);
      const float xm = (float)(tx - 1), ym = (float)(ty - 1);
      const int x1 = (int)fminf(fmaxf(x1f, 0.f), xm), x2 = (int)fminf(fmaxf((x1f + 1.f), 0.f), xm);
      const int y1 = (int)fminf(fmaxf(y1f, 0.f), ym), y2 = (int)fminf(fmaxf((y1f + 1.f), 0.f), ym);
      const unsigned char* row1 = lut + y1 * tx * 256 + Y;   // L[y1][.][Y]
      const unsigned char* row2 = lut + y2 * tx * 256 + Y;
      const float l11 = (float)row1[x1 * 256], l12 = (float)row1[x2 * 256];
      const float l21 = (float)row2[x1 * 256], l22 = (float)row2[x2 * 256];
      const float top = (((1.f - ax) * l11) + (ax * l12));
      const float bot = (((1.f - ax) * l21) + (ax * l22));
      const int dY = (int)to_byte((((1.f - ay) * top) + (ay * bot))) - Y;
#pragma unroll
      for (int c = 0; c < 3; ++c) p[c] = (unsigned char)min(max((int)p[c] + dY, 0), 255);
    }
    tile[a][b] = make_uchar4(p[0], p[1], p[2], 0);
  }
  __syncthreads();

  if (bm == 1) {        // row pass: every row of the staged region, 32 columns, kept in fp32
    for (int e = tid; e < E * PT; e += 256) {
      const int a = e / PT, c = e - a * PT;
      float s0 = 0.f, s1 = 0.f, s2 = 0.f;
      for (int t = -R; t <= R; ++t) {
        const float g = rec[10 + (t < 0 ? -t : t)];
        const uchar4 q = tile[a][c + R + t];
        s0 = (s0 + (g * (float)q.x));
        s1 = (s1 + (g * (float)q.y));
        s2 = (s2 + (g * (float)q.z));
      }
      rowp[a][c][0] = s0; rowp[a][c][1] = s1; rowp[a][c][2] = s2;
    }
    __syncthreads();
  }

  unsigned seed_lo = 0, seed_hi = 0, pepper_thr = 0, salt_thr = 0;
  if (rng != nullptr) {
    seed_lo = rng[4 * n]; seed_hi = rng[4 * n + 1];
    pepper_thr = rng[4 * n + 2]; salt_thr = rng[4 * n + 3];
  }
  const int L = 2 * R + 1;
  for (int e = tid; e < PT * PT; e += 256) {
    const int a = e / PT, c = e - a * PT;
    const int i = i0 + a, j = j0 + c;
    if (i >= H || j >= W) continue;
    unsigned char o[3];
    if (bm == 0) {
      const uchar4 q = tile[a][c];
      o[0] = q.x; o[1] = q.y; o[2] = q.z;
    } else {
      float s0 = 0.f, s1 = 0.f, s2 = 0.f;
      if (bm == 1) {
        for (int t = -R; t <= R; ++t) {
          const float g = rec[10 + (t < 0 ? -t : t)];
          const float* q = rowp[a + R + t][c];
          s0 = (s0 + (g * q[0]));
          s1 = (s1 + (g * q[1]));
          s2 = (s2 + (g * q[2]));
        }
      } else {
        for (int dy = 0; dy < L; ++dy)
          for (int dx = 0; dx < L; ++dx) {
            const float w = rec[15 + dy * L + dx];
            const uchar4 q = tile[a + dy][c + dx];
            s0 = (s0 + (w * (float)q.x));
            s1 = (s1 + (w * (float)q.y));
            s2 = (s2 + (w * (float)q.z));
          }
      }
      o[0] = to_byte(s0); o[1] = to_byte(s1); o[2] = to_byte(s2);
    }
    if (pepper_thr | salt_thr) {                // workgroup-uniform
      const long long pix = (long long)i * W + j;
      unsigned w[4];
      philox4x32_10((unsigned)pix, (unsigned)(pix >> 32), 1u, 0u, seed_lo, seed_hi, w);
      if (w[0] < pepper_thr) o[0] = o[1] = o[2] = 0;
      else if (salt_thr != 0u && w[0] >= 0u - salt_thr) o[0] = o[1] = o[2] = 255;
    }
    unsigned char* dst = image_out + (((size_t)n * H + i) * W + j) * 3;
    dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
  }
}

}  // namespace

extern "C" int unet_augment_post_params_per_sample(void) { return POST; }

namespace {

// workspace: counts [N][3][256] uint32 (zeroed by every hist call), then LUTs [N][64][256] bytes
struct PostWs { unsigned* counts; unsigned char* luts; size_t bytes; };
PostWs post_ws(void* base, int N) {
  WsLayout l(base);
  return {l.take<unsigned>((size_t)N * (POST_COUNT_BYTES / sizeof(unsigned)), 1),
          l.take<unsigned char>((size_t)N * POST_LUT_BYTES, 1), l.bytes()};
}

// the checks and the launches of the three entry points: `hist` / `apply` name the kernels to run
int post_launch(const char* name, bool hist, bool apply, const uint8_t* image, uint8_t* image_out,
                const float* post, const uint32_t* rng, void* workspace, size_t workspace_bytes,
                int N, int H, int W, hipStream_t stream) {
  const PostWs ws = post_ws(workspace, N > 0 ? N : 0);
  if (const int rc = aug_stage_check(name, "post", "blur", apply, image, image_out, post, POST, rng, workspace,
                                     workspace_bytes, ws.bytes, N, H, W))
    return rc;
  if (hist) {
    UNET_HIP_CALL(hipMemsetAsync(ws.counts, 0, (size_t)N * POST_COUNT_BYTES, stream));
    hipLaunchKernelGGL(post_hist_kernel, dim3(HIST_WG, N), dim3(256), 0, stream, image, post,
                       ws.counts, ws.luts, H, W);
    UNET_CHECK_LAUNCH(name);
  }
  if (apply) {
    const dim3 grid((unsigned)ceil_div64(W, PT), (unsigned)ceil_div64(H, PT), N);
    hipLaunchKernelGGL(post_apply_kernel, grid, dim3(256), 0, stream, image, image_out, post, rng,
                       ws.counts, ws.luts, H, W);
    UNET_CHECK_LAUNCH(name);
  }
  return UNET_OK;
}

}  // namespace

extern "C" size_t unet_augment_post_workspace_bytes(int N) {
  return N > 0 ? post_ws(nullptr, N).bytes : 0;
}

extern "C" int unet_augment_post_u8(const uint8_t* image, uint8_t* image_out, const float* post,
                                    const uint32_t* rng, void* workspace, size_t workspace_bytes,
                                    int N, int H, int W, unet_stream_t stream) {
  return post_launch("augment_post_u8", true, true, image, image_out, post, rng, workspace,
                     workspace_bytes, N, H, W, (hipStream_t)stream);
}

extern "C" int unet_augment_post_hist(const uint8_t* image, const float* post, void* workspace,
                                      size_t workspace_bytes, int N, int H, int W,
                                      unet_stream_t stream) {
  return post_launch("augment_post_hist", true, false, image, nullptr, post, nullptr, workspace,
                     workspace_bytes, N, H, W, (hipStream_t)stream);
}

extern "C" int unet_augment_post_apply(const uint8_t* image, uint8_t* image_out,
                                       const float* post, const uint32_t* rng, void* workspace,
                                       size_t workspace_bytes, int N, int H, int W,
                                       unet_stream_t stream) {
  return post_launch("augment_post_apply", false, true, image, image_out, post, rng, workspace,
                     workspace_bytes, N, H, W, (hipStream_t)stream);
}
