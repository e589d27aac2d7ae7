// ssim.hip — SSIM with the 11-tap Gaussian window over fp32 NCHW images: forward (per-image SSIM
// and sum of squared differences from one read of the two images) and the gradient of
// w_ssim * (1 - mean SSIM) + w_mse * mean((x - y)^2) with respect to the prediction in one launch.
// Zero padding outside the image, as conv2d(padding=5).  Every reduction goes through
// per-workgroup partials in double and a fixed-order finalize (no atomics: bit-reproducible, and
// an image's values do not depend on the batch it arrives in).
//
// Replaces calculate_ssim / calculate_psnr (AE_pretrained/reconstruction/utils/metrics.py:15-147)
// and SSIMLoss (AE_pretrained/reconstruction/models/losses.py:178-245).
#include "common.h"

namespace {

constexpr int SR = 5;             // window radius (11 taps)
constexpr int ST = 2 * SR + 1;

struct Gauss11 {
  float g[ST];
};

// target: fp32 NCHW (u8 == 0) or the dataset's uint8 NHWC image, t = v / 255 rounded once to fp32
// (the same value unet_mse_loss_fwd reads)
__device__ __forceinline__ float ssim_target(const void* target, int u8, int n, int k, int C,
                                             size_t HW, size_t p) {
  if (u8) {
    const unsigned char v = reinterpret_cast<const unsigned char*>(target)[((size_t)n * HW + p) * C + k];
    return (float)((double)v / 255.0);
  }
  return reinterpret_cast<const float*>(target)[((size_t)n * C + k) * HW + p];
}

// x (pred) and y (target) of the region rows y0.., cols x0.. (RH x RW) into LDS, 0 outside the image
template <int RH, int RW>
__device__ __forceinline__ void stage_xy(float* __restrict__ xs, float* __restrict__ ys,
                                         const float* __restrict__ pred,
                                         const void* __restrict__ target, int u8, int n, int k,
                                         int C, int H, int W, int y0, int x0) {
  const size_t HW = (size_t)H * W;
  const float* xp = pred + ((size_t)n * C + k) * HW;
  for (int i = threadIdx.x; i < RH * RW; i += 256) {
    const int hy = i / RW, hx = i - hy * RW;
    const int gy = y0 + hy, gx = x0 + hx;
    float xv = 0.f, yv = 0.f;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      const size_t p = (size_t)gy * W + gx;
      xv = xp[p];
      yv = ssim_target(target, u8, n, k, C, HW, p);
    }
    xs[i] = xv;
    ys[i] = yv;
  }
}

// horizontal 11-tap pass of the five maps x, y, x^2, y^2, xy: rows RH of the x/y region (width
// XW) -> hb[m][r][c] for OW output columns; a thread owns a strip of SEG columns of one row
template <int RH, int XW, int OW, int SEG>
__device__ __forceinline__ void hpass5(const float* __restrict__ xs, const float* __restrict__ ys,
                                       float* __restrict__ hb, const Gauss11& g) {
  static_assert(OW % SEG == 0, "strip");
  constexpr int NS = OW / SEG;
  for (int s = threadIdx.x; s < RH * NS; s += 256) {
    const int r = s / NS, c0 = (s - r * NS) * SEG;
    float xr[SEG + 2 * SR], yr[SEG + 2 * SR];
#pragma unroll
    for (int j = 0; j < SEG + 2 * SR; ++j) {
      xr[j] = xs[r * XW + c0 + j];
      yr[j] = ys[r * XW + c0 + j];
    }
#pragma unroll
    for (int j = 0; j < SEG; ++j) {
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
#pragma unroll
      for (int t = 0; t < ST; ++t) {
        const float xv = xr[j + t], yv = yr[j + t], w = g.g[t];
        a0 = fmaf(w, xv, a0);
        a1 = fmaf(w, yv, a1);
        a2 = fmaf(w, xv * xv, a2);
        a3 = fmaf(w, yv * yv, a3);
        a4 = fmaf(w, xv * yv, a4);
      }
      const int o = r * OW + c0 + j;
      hb[0 * RH * OW + o] = a0;
      hb[1 * RH * OW + o] = a1;
      hb[2 * RH * OW + o] = a2;
      hb[3 * RH * OW + o] = a3;
      hb[4 * RH * OW + o] = a4;
    }
  }
}

// vertical 11-tap pass of M maps for a strip of SEG output rows starting at r0 in column c:
// hb[m][r][c] (RH rows, width OW; rows >= RH read as 0) -> acc[j][m]
template <int M, int RH, int OW, int SEG>
__device__ __forceinline__ void vstrip(const float* __restrict__ hb, int r0, int c,
                                       float (&acc)[SEG][M], const Gauss11& g) {
#pragma unroll
  for (int j = 0; j < SEG; ++j)
#pragma unroll
    for (int m = 0; m < M; ++m) acc[j][m] = 0.f;
#pragma unroll
  for (int rr = 0; rr < SEG + 2 * SR; ++rr) {
    const int r = r0 + rr;
    float v[M];
#pragma unroll
    for (int m = 0; m < M; ++m) v[m] = r < RH ? hb[m * RH * OW + r * OW + c] : 0.f;
#pragma unroll
    for (int j = 0; j < SEG; ++j) {
      const int t = rr - j;
      if (t >= 0 && t < ST) {
#pragma unroll
        for (int m = 0; m < M; ++m) acc[j][m] = fmaf(g.g[t], v[m], acc[j][m]);
      }
    }
  }
}

// the SSIM map from the five window moments, in the reference's order of operations
__device__ __forceinline__ float ssim_of(const float (&e)[5], float c1, float c2) {
  const float mx2 = e[0] * e[0], my2 = e[1] * e[1], mxy = e[0] * e[1];
  const float sxx = e[2] - mx2, syy = e[3] - my2, sxy = e[4] - mxy;
  return ((2.f * mxy + c1) * (2.f * sxy + c2)) / ((mx2 + my2 + c1) * (sxx + syy + c2));
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// ------------------------------------------------------------------ forward
// A workgroup owns a 32 x 32 output tile of one (image, channel) plane: the 42 x 42 x / y halo in
// LDS, the horizontal pass into hb (42 rows x 32 columns x 5 maps), then four output rows of one
// column per thread.
constexpr int FTW = 32, FTH = 32;
constexpr int FXW = FTW + 2 * SR, FXH = FTH + 2 * SR;   // 42 x 42

__global__ __launch_bounds__(256) void ssim_reduce_kernel(const float* __restrict__ pred,
                                                          const void* __restrict__ target, int u8,
                                                          Gauss11 g, float c1, float c2,
                                                          double* __restrict__ partial, int C,
                                                          int H, int W, int tiles_x) {
  __shared__ float xs[FXH * FXW], ys[FXH * FXW];
  __shared__ float hb[5 * FXH * FTW];
  __shared__ double red[4][2];
  const int tile = blockIdx.x, k = blockIdx.y, n = blockIdx.z;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int y0 = ty * FTH, x0 = tx * FTW;
  stage_xy<FXH, FXW>(xs, ys, pred, target, u8, n, k, C, H, W, y0 - SR, x0 - SR);
  __syncthreads();
  hpass5<FXH, FXW, FTW, 8>(xs, ys, hb, g);
  __syncthreads();
  const int c = threadIdx.x & 31, r0 = (threadIdx.x >> 5) * 4;
  float acc[4][5];
  vstrip<5, FXH, FTW, 4>(hb, r0, c, acc, g);
  double s_ssim = 0.0, s_sq = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int gy = y0 + r0 + j, gx = x0 + c;
    if (gy < H && gx < W) {
      s_ssim += (double)ssim_of(acc[j], c1, c2);
      const int li = (r0 + j + SR) * FXW + c + SR;
      const float d = xs[li] - ys[li];
      s_sq += (double)(d * d);
    }
  }
  s_ssim = wave_sum_d(s_ssim);
  s_sq = wave_sum_d(s_sq);
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6][0] = s_ssim;
    red[threadIdx.x >> 6][1] = s_sq;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const int q = threadIdx.x;
    const size_t tiles = gridDim.x;
    partial[(((size_t)n * C + k) * tiles + tile) * 2 + q] =
        (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
  }
}

// per image: the partials of its C x tiles workgroups, strided over the 256 threads and
// tree-summed (an order fixed by C x tiles alone, independent of N); then
// loss_out[0] = w_ssim * (1 - mean SSIM) + w_mse * mean sq over all N * C * H * W elements
__global__ __launch_bounds__(256) void ssim_finalize_kernel(const double* __restrict__ partial,
                                                            int N, int per_image_blocks,
                                                            double chw, double w_ssim,
                                                            double w_mse,
                                                            double* __restrict__ ssim_per_image,
                                                            double* __restrict__ sq_per_image,
                                                            float* __restrict__ loss_out) {
  __shared__ double red[2][256];
  const int tid = threadIdx.x;
  for (int n = 0; n < N; ++n) {
    double s = 0.0, q = 0.0;
    const double* p = partial + (size_t)n * per_image_blocks * 2;
    for (int b = tid; b < per_image_blocks; b += 256) {
      s += p[2 * b];
      q += p[2 * b + 1];
    }
    red[0][tid] = s;
    red[1][tid] = q;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
      if (tid < off) {
        red[0][tid] += red[0][tid + off];
        red[1][tid] += red[1][tid + off];
      }
      __syncthreads();
    }
    if (tid == 0) {
      ssim_per_image[n] = red[0][0] / chw;
      sq_per_image[n] = red[1][0];
    }
    __syncthreads();
  }
  if (tid == 0 && loss_out) {
    double s = 0.0, q = 0.0;
    for (int n = 0; n < N; ++n) {
      s += ssim_per_image[n];
      q += sq_per_image[n];
    }
    loss_out[0] = (float)(w_ssim * (1.0 - s / N) + w_mse * (q / (chw * N)));
  }
}

// ------------------------------------------------------------------ gradient
// A workgroup owns a 32 x 16 output tile of one plane.  The x / y region carries a 10-pixel halo
// (52 x 36); the window moments and from them A = dS/dmu_x, B = dS/dE[x^2], C = dS/dE[xy] are
// formed on the 5-pixel halo (42 x 26, zero outside the image); the blur of A, B, C back to the
// tile gives dS_mean/dx.
constexpr int GTW = 32, GTH = 16;
constexpr int GXW = GTW + 4 * SR, GXH = GTH + 4 * SR;   // 52 x 36
constexpr int GMW = GTW + 2 * SR, GMH = GTH + 2 * SR;   // 42 x 26
constexpr int GHSEG = 6, GVSEG = 5;                     // moment strips (42 = 7 x 6; 26 <= 6 x 5)

__global__ __launch_bounds__(256) void ssim_grad_kernel(const float* __restrict__ pred,
                                                        const void* __restrict__ target, int u8,
                                                        Gauss11 g, float c1, float c2,
                                                        const float* __restrict__ upstream,
                                                        int upstream_per_image, float cs,
                                                        float cm, float* __restrict__ dpred,
                                                        int C, int H, int W, int tiles_x) {
  __shared__ float xs[GXH * GXW], ys[GXH * GXW];
  __shared__ float hb[5 * GXH * GMW];      // moments' horizontal pass, later A/B/C's
  __shared__ float abc[3 * GMH * GMW];
  const int tile = blockIdx.x, k = blockIdx.y, n = blockIdx.z;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int y0 = ty * GTH, x0 = tx * GTW;
  stage_xy<GXH, GXW>(xs, ys, pred, target, u8, n, k, C, H, W, y0 - 2 * SR, x0 - 2 * SR);
  __syncthreads();
  hpass5<GXH, GXW, GMW, GHSEG>(xs, ys, hb, g);
  __syncthreads();
  // moments -> A, B, C on the 42 x 26 region (a strip of 5 rows of one column per thread)
  {
    constexpr int NG = (GMH + GVSEG - 1) / GVSEG;   // 6 row groups
    const int t = threadIdx.x;
    if (t < GMW * NG) {
      const int c = t % GMW, r0 = (t / GMW) * GVSEG;
      float e[GVSEG][5];
      vstrip<5, GXH, GMW, GVSEG>(hb, r0, c, e, g);
#pragma unroll
      for (int j = 0; j < GVSEG; ++j) {
        const int r = r0 + j;
        if (r < GMH) {
          const int gy = y0 - SR + r, gx = x0 - SR + c;
          float A = 0.f, B = 0.f, Cc = 0.f;
          if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const float mx = e[j][0], my = e[j][1];
            const float mx2 = mx * mx, my2 = my * my, mxy = mx * my;
            const float sxx = e[j][2] - mx2, syy = e[j][3] - my2, sxy = e[j][4] - mxy;
            const float N1 = 2.f * mxy + c1, N2 = 2.f * sxy + c2;
            const float D1 = mx2 + my2 + c1, D2 = sxx + syy + c2;
            const float inv = 1.f / (D1 * D2);
            const float S = N1 * N2 * inv;
            A = 2.f * (my * (N2 - N1) * inv + mx * S * (1.f / D2 - 1.f / D1));
            B = -S / D2;
            Cc = 2.f * N1 * inv;
          }
          abc[0 * GMH * GMW + r * GMW + c] = A;
          abc[1 * GMH * GMW + r * GMW + c] = B;
          abc[2 * GMH * GMW + r * GMW + c] = Cc;
        }
      }
    }
  }
  __syncthreads();
  // horizontal pass of A, B, C: 26 rows x 32 columns into hb (strips of 8 columns)
  for (int s = threadIdx.x; s < GMH * (GTW / 8); s += 256) {
    const int r = s / (GTW / 8), c0 = (s - r * (GTW / 8)) * 8;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      float v[8 + 2 * SR];
#pragma unroll
      for (int j = 0; j < 8 + 2 * SR; ++j) v[j] = abc[m * GMH * GMW + r * GMW + c0 + j];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float a = 0.f;
#pragma unroll
        for (int t = 0; t < ST; ++t) a = fmaf(g.g[t], v[j + t], a);
        hb[m * GMH * GTW + r * GTW + c0 + j] = a;
      }
    }
  }
  __syncthreads();
  // vertical pass to the tile (two rows of one column per thread) and the gradient
  const int c = threadIdx.x & 31, r0 = (threadIdx.x >> 5) * 2;
  float bl[2][3];
  vstrip<3, GMH, GTW, 2>(hb, r0, c, bl, g);
  const float up = upstream ? upstream[upstream_per_image ? n : 0] : 1.f;
  const size_t HW = (size_t)H * W;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int gy = y0 + r0 + j, gx = x0 + c;
    if (gy < H && gx < W) {
      const int li = (r0 + j + 2 * SR) * GXW + c + 2 * SR;
      const float xv = xs[li], yv = ys[li];
      const float ds = bl[j][0] + 2.f * xv * bl[j][1] + yv * bl[j][2];
      dpred[((size_t)n * C + k) * HW + (size_t)gy * W + gx] = up * (cm * (xv - yv) - cs * ds);
    }
  }
}

bool ssim_shape_ok(int N, int C, int H, int W) {
  return N > 0 && C > 0 && H > 0 && W > 0 && N < 65536 && C < 65536;
}

int ssim_fwd_tiles(int H, int W, int* tiles_x) {
  *tiles_x = ceil_div(W, FTW);
  return *tiles_x * ceil_div(H, FTH);
}

}  // namespace

extern "C" size_t unet_ssim_workspace_bytes(int N, int C, int H, int W) {
  if (!ssim_shape_ok(N, C, H, W)) return 0;
  int tx;
  return (size_t)N * C * ssim_fwd_tiles(H, W, &tx) * 2 * sizeof(double);
}

extern "C" int unet_ssim_fwd(const float* pred, const void* target, int target_u8,
                             const float* gauss11, float c1, float c2, double* ssim_per_image,
                             double* sq_per_image, float* loss_out, double w_ssim, double w_mse,
                             void* workspace, size_t workspace_bytes, int N, int C, int H, int W,
                             unet_stream_t stream) {
  UNET_REQUIRE(pred && target && gauss11 && ssim_per_image && sq_per_image && workspace,
               "ssim_fwd: null pointer");
  UNET_REQUIRE(ssim_shape_ok(N, C, H, W) && (!target_u8 || C == 3),
               "ssim_fwd: bad shape (N, C < 65536; a uint8 target needs C == 3)");
  UNET_REQUIRE_WS(workspace_bytes, unet_ssim_workspace_bytes(N, C, H, W),
                  "ssim_fwd: workspace too small");
  Gauss11 g;
  for (int t = 0; t < ST; ++t) g.g[t] = gauss11[t];
  int tiles_x;
  const int tiles = ssim_fwd_tiles(H, W, &tiles_x);
  double* partial = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(ssim_reduce_kernel, dim3((unsigned)tiles, (unsigned)C, (unsigned)N),
                     dim3(256), 0, (hipStream_t)stream, pred, target, target_u8, g, c1, c2,
                     partial, C, H, W, tiles_x);
  UNET_CHECK_LAUNCH("ssim_reduce");
  hipLaunchKernelGGL(ssim_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, N,
                     C * tiles, (double)C * H * W, w_ssim, w_mse, ssim_per_image, sq_per_image,
                     loss_out);
  UNET_CHECK_LAUNCH("ssim_finalize");
  return UNET_OK;
}

extern "C" int unet_ssim_grad(const float* pred, const void* target, int target_u8,
                              const float* gauss11, float c1, float c2, const float* upstream,
                              int upstream_per_image, double w_ssim, double w_mse,
                              float* dpred, int N, int C, int H, int W, unet_stream_t stream) {
  UNET_REQUIRE(pred && target && gauss11 && dpred, "ssim_grad: null pointer");
  UNET_REQUIRE(ssim_shape_ok(N, C, H, W) && (!target_u8 || C == 3),
               "ssim_grad: bad shape (N, C < 65536; a uint8 target needs C == 3)");
  UNET_REQUIRE(!upstream_per_image || upstream, "ssim_grad: a per-image upstream needs upstream");
  Gauss11 g;
  for (int t = 0; t < ST; ++t) g.g[t] = gauss11[t];
  // the element count behind each mean: the whole batch, or one image (per-image upstream)
  const double K = (double)C * H * W * (upstream_per_image ? 1 : N);
  const int tiles_x = ceil_div(W, GTW), tiles = tiles_x * ceil_div(H, GTH);
  hipLaunchKernelGGL(ssim_grad_kernel, dim3((unsigned)tiles, (unsigned)C, (unsigned)N), dim3(256),
                     0, (hipStream_t)stream, pred, target, target_u8, g, c1, c2, upstream,
                     upstream_per_image, (float)(w_ssim / K), (float)(2.0 * w_mse / K), dpred, C,
                     H, W, tiles_x);
  UNET_CHECK_LAUNCH("ssim_grad");
  return UNET_OK;
}
