// gradcam.hip — the tail of Grad-CAM (Our_UNet/utils/visualize.py:423-437) on the walk's own
// tensors, for a whole batch, without a host sync:
//
//   unet_gradcam_weights   w[n][c]   = mean over the pixels of G[n][p][c]        (visualize.py:424)
//   unet_gradcam_map       cam[n][p] = max(0, sum_c w[n][c] * act(A)[n][p][c])   (:427-428)
//                          + per-workgroup (min, max) of cam
//   unet_gradcam_heatmap   per image: cam - min, / max(cam - min) unless that is 0, then the
//                          bilinear resize (align_corners = False) to the input size     (:431-437)
//
// A is the stage output as the fused walk keeps it - the RAW convolution output plus the folded
// InstanceNorm coefficients, activated while it is loaded - and G its gradient, both NHWC in the
// walk's storage type (fp32 or bf16).  All sums are fp32 in a fixed order (per-workgroup partials,
// a second level): no floating-point atomics, two runs are bit-identical.  The two passes over G
// and A are single HBM-bound reads with the lanes across the channels (C is innermost).
#include <math.h>

#include "common.h"

namespace {

constexpr int GC_THREADS = 256;
constexpr int GC_FL = 32;            // lanes per channel of the second level of the weights
constexpr int GC_MAX_BLOCKS = 2048;  // workgroups of one launch (about 8 per CU)

bool gc_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// slabs of pixels per image for the channel means: ~GC_MAX_BLOCKS workgroups in all, at least 8
// pixels per thread
int gc_weight_slabs(int N, int HW, int C) {
  const int groups = GC_THREADS / (C / 4);
  const int most = HW / (groups * 8);
  const int want = ceil_div(GC_MAX_BLOCKS, N);
  const int s = want < most ? want : most;
  return s < 1 ? 1 : s;
}

// pixels per workgroup of the map launch (>= 64), a function of (N, HW) only: the heatmap launch
// recomputes it to know how many (min, max) pairs the map launch left per image
int gc_map_per(int N, int HW) {
  const int per = ceil_div(HW, ceil_div(GC_MAX_BLOCKS, N));
  return per < 64 ? 64 : per;
}
int gc_map_tiles(int N, int HW) { return ceil_div(HW, gc_map_per(N, HW)); }

// The (min, max) pairs the map launch leaves per tile and image, then the slabs of the channel
// means.  C == 0: the prefix the map and heatmap launches use (the heatmap is not told C).
struct GcWs { float2* minmax; float* partial; size_t bytes; };
GcWs gc_ws(void* base, int N, int HW, int C) {
  WsLayout l(base);
  return {l.take<float2>((size_t)N * gc_map_tiles(N, HW), 256),
          C ? l.take<float>((size_t)N * gc_weight_slabs(N, HW, C) * C, 256) : nullptr, l.bytes()};
}

// level 1 of w = mean_p G: grid (slabs, N); lanes across the channels (4 each), the workgroup's
// pixel groups down its slab; the groups are summed in order through LDS.  One slab: w directly.
template <typename T>
__global__ __launch_bounds__(GC_THREADS) void gradcam_weights_kernel(
    const T* __restrict__ g, float* __restrict__ partial, float* __restrict__ w, int HW, int C,
    int slabs) {
  __shared__ __attribute__((aligned(16))) float smem[GC_THREADS * 4];   // [groups][C]
  const int lpp = C >> 2, groups = GC_THREADS / lpp;
  const int tid = threadIdx.x, grp = tid / lpp, c4 = tid - grp * lpp;
  const int n = blockIdx.y, s = blockIdx.x;
  const int per = (HW + slabs - 1) / slabs;
  const int p0 = s * per, p1 = min(p0 + per, HW);
  const T* base = g + (size_t)n * HW * C + c4 * 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int p = p0 + grp; p < p1; p += groups) acc += ld4(base + (size_t)p * C);
  *reinterpret_cast<f32x4*>(smem + grp * C + c4 * 4) = acc;
  __syncthreads();
  for (int c = tid; c < C; c += GC_THREADS) {
    float a = 0.f;
    for (int q = 0; q < groups; ++q) a += smem[q * C + c];
    if (slabs == 1)
      w[(size_t)n * C + c] = __fdiv_rn(a, (float)HW);
    else
      partial[((size_t)n * slabs + s) * C + c] = a;
  }
}

// level 2: block = 32 channels x GC_FL lanes, grid (C / 32, N), as the InstanceNorm finalisers
__global__ __launch_bounds__(32 * GC_FL) void gradcam_weights_finalize_kernel(
    const float* __restrict__ partial, float* __restrict__ w, int HW, int C, int slabs) {
  __shared__ float sa[GC_FL][33];
  const int cl = threadIdx.x & 31, l = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl, n = blockIdx.y;
  float a = 0.f;
  if (c < C)
    for (int s = l; s < slabs; s += GC_FL) a += partial[((size_t)n * slabs + s) * C + c];
  sa[l][cl] = a;
  __syncthreads();
  if (l == 0 && c < C) {
    a = 0.f;
    for (int k = 0; k < GC_FL; ++k) a += sa[k][cl];
    w[(size_t)n * C + c] = __fdiv_rn(a, (float)HW);
  }
}

// (min, max) over the workgroup -> every thread
__device__ __forceinline__ void block_minmax(float& mn, float& mx, float* smn, float* smx) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, off, 64));
    mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { smn[wave] = mn; smx[wave] = mx; }
  __syncthreads();
  mn = fminf(fminf(smn[0], smn[1]), fminf(smn[2], smn[3]));
  mx = fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3]));
}

// cam = relu(sum_c w_c * act(x)_c): grid (tiles, N).  min(C / 4, 64) lanes share a pixel, 4
// channels each per pass (P passes of 256 channels where C > 256), so a wave reads whole
// contiguous pixels; the lanes of a pixel are summed with a butterfly (a fixed order).  w, alpha,
// beta of the image stay in registers.  alpha == NULL: x is a plain tensor.
template <typename T, int P>
__global__ __launch_bounds__(GC_THREADS) void gradcam_map_kernel(
    const T* __restrict__ x, const float* __restrict__ alpha, const float* __restrict__ beta,
    float slope, const float* __restrict__ w, float* __restrict__ cam,
    float2* __restrict__ minmax, int HW, int C, int per) {
  __shared__ float smn[4], smx[4];
  const int lpp = P > 1 ? 64 : (C >> 2), groups = GC_THREADS / lpp;
  const int tid = threadIdx.x, grp = tid / lpp, c0 = (tid - grp * lpp) * 4;
  const int n = blockIdx.y;
  const int p0 = blockIdx.x * per, p1 = min(p0 + per, HW);     // never empty (gc_map_tiles)
  const f32x4 one = {1.f, 1.f, 1.f, 1.f}, zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 wv[P], al[P], be[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const size_t o = (size_t)n * C + c0 + j * 256;
    wv[j] = ld4(w + o);
    al[j] = alpha ? ld4(alpha + o) : one;
    be[j] = alpha ? ld4(beta + o) : zero;
  }
  const float sl = alpha ? slope : 1.f;
  const T* xb = x + (size_t)n * HW * C + c0;
  float* cb = cam + (size_t)n * HW;
  float mn = INFINITY, mx = -INFINITY;
  for (int pb = p0; pb < p1; pb += groups) {
    const int p = pb + grp;
    const bool valid = p < p1;
    const int pc = valid ? p : p1 - 1;       // every lane of the wave takes part in the butterfly
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const f32x4 v = ld4(xb + (size_t)pc * C + j * 256);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float z = fmaf(v[k], al[j][k], be[j][k]);     // as in_apply_fwd_kernel
        acc = fmaf(wv[j][k], z > 0.f ? z : z * sl, acc);
      }
    }
    for (int off = lpp >> 1; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    const float r = fmaxf(acc, 0.f);
    if (valid) {
      if (c0 == 0) cb[p] = r;
      mn = fminf(mn, r);
      mx = fmaxf(mx, r);
    }
  }
  block_minmax(mn, mx, smn, smx);
  if (tid == 0) minmax[(size_t)n * gridDim.x + blockIdx.x] = float2{mn, mx};
}

// PyTorch's bilinear source index (align_corners = False): bil_src of common.h.
// grid (blocks, N): every workgroup first reduces its image's (min, max) pairs, then writes
// out[n][Y][X] = blend of the four NORMALISED taps ((c - min) / (max - min), correctly rounded
// as torch's division); max == min leaves the image at zero without dividing.
__global__ __launch_bounds__(GC_THREADS) void gradcam_heatmap_kernel(
    const float* __restrict__ cam, const float2* __restrict__ minmax, float* __restrict__ out,
    int tiles, int h, int w, int H, int W) {
  __shared__ float smn[4], smx[4];
  const int n = blockIdx.y;
  float mn = INFINITY, mx = -INFINITY;
  for (int t = threadIdx.x; t < tiles; t += GC_THREADS) {
    const float2 v = minmax[(size_t)n * tiles + t];
    mn = fminf(mn, v.x);
    mx = fmaxf(mx, v.y);
  }
  block_minmax(mn, mx, smn, smx);
  const float range = mx - mn;
  const bool live = range != 0.f;
  const float* c = cam + (size_t)n * h * w;
  float* o = out + (size_t)n * H * W;
  const float sy = (float)h / (float)H, sx = (float)w / (float)W;
  const int total = H * W;
  for (int i = blockIdx.x * GC_THREADS + threadIdx.x; i < total; i += gridDim.x * GC_THREADS) {
    float v = 0.f;
    if (live) {
      const int Y = i / W, X = i - Y * W;
      int y0, y1, x0, x1;
      float ly, lx;
      bil_src(Y, sy, h, y0, y1, ly);
      bil_src(X, sx, w, x0, x1, lx);
      const float t00 = __fdiv_rn(c[(size_t)y0 * w + x0] - mn, range);
      const float t01 = __fdiv_rn(c[(size_t)y0 * w + x1] - mn, range);
      const float t10 = __fdiv_rn(c[(size_t)y1 * w + x0] - mn, range);
      const float t11 = __fdiv_rn(c[(size_t)y1 * w + x1] - mn, range);
      const float top = (1.f - lx) * t00 + lx * t01;
      const float bot = (1.f - lx) * t10 + lx * t11;
      v = (1.f - ly) * top + ly * bot;
    }
    o[i] = v;
  }
}

bool gc_shape_ok(int N, long long HW, int C) {
  // lanes across the channels: C / 4 lanes divide the workgroup, or whole passes of 256 channels
  return N > 0 && N <= 65535 && HW > 0 && HW <= (1ll << 30) && C >= 4 && C % 4 == 0 &&
         ((C <= 256 && GC_THREADS % (C / 4) == 0) || C == 512 || C == 1024);
}

template <typename T>
int launch_map(const unet_act_src* a, float slope, const float* w, float* cam, float2* mm, int N,
               int HW, hipStream_t stream) {
  const int C = a->C, per = gc_map_per(N, HW);
  const dim3 grid(gc_map_tiles(N, HW), N), block(GC_THREADS);
  const T* x = reinterpret_cast<const T*>(a->x);
  if (C <= 256)
    hipLaunchKernelGGL((gradcam_map_kernel<T, 1>), grid, block, 0, stream, x, a->alpha, a->beta,
                       slope, w, cam, mm, HW, C, per);
  else if (C == 512)
    hipLaunchKernelGGL((gradcam_map_kernel<T, 2>), grid, block, 0, stream, x, a->alpha, a->beta,
                       slope, w, cam, mm, HW, C, per);
  else
    hipLaunchKernelGGL((gradcam_map_kernel<T, 4>), grid, block, 0, stream, x, a->alpha, a->beta,
                       slope, w, cam, mm, HW, C, per);
  UNET_CHECK_LAUNCH("gradcam_map");
  return UNET_OK;
}

}  // namespace

extern "C" size_t unet_gradcam_workspace_bytes(int N, int HW, int C) {
  if (!gc_shape_ok(N, HW, C)) return 0;
  return gc_ws(nullptr, N, HW, C).bytes;
}

extern "C" int unet_gradcam_weights(const void* g, int g_bf16, float* w, void* workspace,
                                    size_t workspace_bytes, int N, int HW, int C,
                                    unet_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  UNET_REQUIRE(g && w && workspace, "gradcam_weights: null pointer");
  UNET_REQUIRE(gc_shape_ok(N, HW, C),
               "gradcam_weights: bad shape N=%d HW=%d C=%d (C = 4..256 a power of two, 512 or "
               "1024; HW <= 2^30)", N, HW, C);
  UNET_REQUIRE(gc_aligned(g) && gc_aligned(w) && gc_aligned(workspace),
               "gradcam_weights: pointers must be 16-byte aligned");
  const GcWs ws = gc_ws(workspace, N, HW, C);
  UNET_REQUIRE_WS(workspace_bytes, ws.bytes, "gradcam_weights: workspace too small");
  const int slabs = gc_weight_slabs(N, HW, C);
  const dim3 grid(slabs, N), block(GC_THREADS);
  if (g_bf16)
    hipLaunchKernelGGL(gradcam_weights_kernel<__bf16>, grid, block, 0, stream,
                       reinterpret_cast<const __bf16*>(g), ws.partial, w, HW, C, slabs);
  else
    hipLaunchKernelGGL(gradcam_weights_kernel<float>, grid, block, 0, stream,
                       reinterpret_cast<const float*>(g), ws.partial, w, HW, C, slabs);
  UNET_CHECK_LAUNCH("gradcam_weights");
  if (slabs > 1) {
    hipLaunchKernelGGL(gradcam_weights_finalize_kernel, dim3(ceil_div(C, 32), N),
                       dim3(32 * GC_FL), 0, stream, ws.partial, w, HW, C, slabs);
    UNET_CHECK_LAUNCH("gradcam_weights_finalize");
  }
  return UNET_OK;
}

extern "C" int unet_gradcam_map(const unet_act_src* a, int a_bf16, float slope, const float* w,
                                float* cam, void* workspace, size_t workspace_bytes, int N,
                                int HW, unet_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  UNET_REQUIRE(a && a->x && (!a->alpha || a->beta) && w && cam && workspace,
               "gradcam_map: null pointer");
  UNET_REQUIRE(gc_shape_ok(N, HW, a->C),
               "gradcam_map: bad shape N=%d HW=%d C=%d (C = 4..256 a power of two, 512 or 1024; "
               "HW <= 2^30)", N, HW, a->C);
  UNET_REQUIRE(slope >= 0.f && slope <= 1.f, "gradcam_map: slope must lie in [0, 1]");
  UNET_REQUIRE(gc_aligned(a->x) && gc_aligned(a->alpha) && gc_aligned(a->beta) && gc_aligned(w) &&
               gc_aligned(workspace), "gradcam_map: pointers must be 16-byte aligned");
  const GcWs ws = gc_ws(workspace, N, HW, 0);
  UNET_REQUIRE_WS(workspace_bytes, ws.bytes, "gradcam_map: workspace too small");
  return a_bf16 ? launch_map<__bf16>(a, slope, w, cam, ws.minmax, N, HW, stream)
                : launch_map<float>(a, slope, w, cam, ws.minmax, N, HW, stream);
}

extern "C" int unet_gradcam_heatmap(const float* cam, const void* workspace,
                                    size_t workspace_bytes, float* heatmap, int N, int h, int w,
                                    int H, int W, unet_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  UNET_REQUIRE(cam && workspace && heatmap, "gradcam_heatmap: null pointer");
  UNET_REQUIRE(N > 0 && N <= 65535 && h > 0 && w > 0 && H > 0 && W > 0 &&
               (long long)h * w <= (1ll << 30) && (long long)H * W <= (1ll << 30),
               "gradcam_heatmap: bad shape (N in 1..65535, h * w and H * W in 1..2^30)");
  const GcWs ws = gc_ws(const_cast<void*>(workspace), N, h * w, 0);
  UNET_REQUIRE_WS(workspace_bytes, ws.bytes, "gradcam_heatmap: workspace too small");
  int blocks = ceil_div(H * W, GC_THREADS * 4);
  const int most = ceil_div(GC_MAX_BLOCKS, N);
  blocks = blocks > most ? most : blocks;
  hipLaunchKernelGGL(gradcam_heatmap_kernel, dim3(blocks, N), dim3(GC_THREADS), 0, stream, cam,
                     ws.minmax, heatmap, gc_map_tiles(N, h * w), h, w, H, W);
  UNET_CHECK_LAUNCH("gradcam_heatmap");
  return UNET_OK;
}
