// perceptual.hip — the glue of the perceptual (VGG16 feature) loss around the convolution kernels:
// image normalisation into the stacked output / target tensor, ReLU + 2x2 max-pooling, the
// feature-MSE reductions, the ReLU / pool / feature-loss backward of one trunk layer and the
// 64 -> 3 data gradient of conv1_1.  All HBM-bound, fp32 arithmetic on NHWC layer tensors; every
// reduction goes through per-workgroup partials in double and a fixed-order finalize (no float
// atomics: bit-reproducible).
//
// Replaces PerceptualLoss._normalize / .forward (AE_pretrained/reconstruction/models/losses.py:
// 134-168) and their autograd around the VGG16 trunk's Conv2d modules.
#include "common.h"

namespace {

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ f32x4 relu4(const f32x4 v) {
  return f32x4{fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)};
}

// blocks of a grid-stride launch over `items` work items of 256 threads
unsigned stream_grid(long long items) {
  long long b = ceil_div64(items, 256);
  if (b > 256 * 16) b = 256 * 16;
  return b < 1 ? 1u : (unsigned)b;
}

// ------------------------------------------------------------------ normalisation
struct Norm3 { float mean[3], std[3]; };

// (x - mean[c]) / std[c], both operations correctly rounded (the device's default fp32 division
// is not): the two-operation form of PerceptualLoss._normalize
__device__ __forceinline__ float norm1(float x, float mean, float std) {
  return __fdiv_rn(__fsub_rn(x, mean), std);
}

// blockIdx.y = image of the stacked tensor: [0, N) the output, [N, 2N) the target.  PX pixels per
// thread: 4 when H * W % 4 == 0 (every plane row of four and every group of 12 output floats is
// then 16-byte aligned), else 1.
template <int PX>
__global__ __launch_bounds__(256) void perceptual_prep_kernel(const float* __restrict__ out,
                                                              const void* __restrict__ target,
                                                              int u8, float* __restrict__ xn,
                                                              int N, long long HW, const Norm3 nm) {
  const int img = blockIdx.y;
  const bool is_t = img >= N;
  const int n = is_t ? img - N : img;
  const long long groups = HW / PX;
  float* dst = xn + (size_t)img * HW * 3;
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < groups;
       q += (long long)gridDim.x * 256) {
    const long long p = q * PX;
    float v[3][PX];
    if (is_t && u8) {
      const unsigned char* t = reinterpret_cast<const unsigned char*>(target) + ((size_t)n * HW + p) * 3;
      unsigned char b[3 * PX];
      if (PX == 4) {
        const unsigned* t4 = reinterpret_cast<const unsigned*>(t);   // 12 bytes, 4-byte aligned
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const unsigned u = t4[i];
#pragma unroll
          for (int j = 0; j < 4; ++j) b[i * 4 + j] = (unsigned char)(u >> (8 * j));
        }
      } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) b[i] = t[i];
      }
      // double quotient rounded once to fp32 = the correctly rounded fp32 v / 255 (mse_target of
      // recon.hip)
#pragma unroll
      for (int j = 0; j < PX; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c][j] = (float)((double)b[j * 3 + c] / 255.0);
    } else {
      const float* src = (is_t ? reinterpret_cast<const float*>(target) : out) + (size_t)n * 3 * HW + p;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (PX == 4) {
          const f32x4 t = *reinterpret_cast<const f32x4*>(src + (size_t)c * HW);
#pragma unroll
          for (int j = 0; j < 4; ++j) v[c][j] = t[j];
        } else {
          v[c][0] = src[(size_t)c * HW];
        }
      }
    }
    float o[3 * PX];
#pragma unroll
    for (int j = 0; j < PX; ++j)
#pragma unroll
      for (int c = 0; c < 3; ++c) o[j * 3 + c] = norm1(v[c][j], nm.mean[c], nm.std[c]);
    if (PX == 4) {
#pragma unroll
      for (int i = 0; i < 3; ++i)
        st4(dst + p * 3 + i * 4, f32x4{o[i * 4], o[i * 4 + 1], o[i * 4 + 2], o[i * 4 + 3]});
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) dst[p * 3 + c] = o[c];
    }
  }
}

// ------------------------------------------------------------------ ReLU + 2x2 max-pooling
// one item = four channels of one pooled pixel
__global__ __launch_bounds__(256) void relu_maxpool2x2_fwd_kernel(const float* __restrict__ y,
                                                                  float* __restrict__ p,
                                                                  long long items, int H, int W,
                                                                  int Ho, int Wo, int C4) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items;
       i += (long long)gridDim.x * 256) {
    const int ch = (int)(i % C4);
    long long r = i / C4;
    const int xo = (int)(r % Wo);
    r /= Wo;
    const int yo = (int)(r % Ho);
    const long long m = r / Ho;
    const float* s = y + ((((size_t)m * H + 2 * yo) * W + 2 * xo) * C4 + ch) * 4;
    const size_t row = (size_t)W * C4 * 4;
    const f32x4 a = ld4(s), b = ld4(s + (size_t)C4 * 4), c = ld4(s + row),
                d = ld4(s + row + (size_t)C4 * 4);
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = fmaxf(fmaxf(fmaxf(a[k], b[k]), fmaxf(c[k], d[k])), 0.f);
    st4(p + (size_t)i * 4, o);
  }
}

// ------------------------------------------------------------------ feature MSE
constexpr int FM_MAX_BLOCKS = 256;   // per image pair

// blocks per image pair: a function of the elements of one image only
int fm_blocks(long long vec4_per_image) {
  long long b = ceil_div64(vec4_per_image, 256 * 8);
  if (b > FM_MAX_BLOCKS) b = FM_MAX_BLOCKS;
  return b < 1 ? 1 : (int)b;
}

// blockIdx.y = image pair n: sum over the image of (relu(y[n]) - relu(y[n + N]))^2, each term
// formed in fp32 (one rounding of the difference, one of the square) and summed in double
__global__ __launch_bounds__(256) void feature_mse_reduce_kernel(const float* __restrict__ y,
                                                                 double* __restrict__ partial,
                                                                 int N, long long vec4) {
#pragma clang fp contract(off)
  __shared__ double red[4];
  const int n = blockIdx.y;
  const float* a = y + (size_t)n * vec4 * 4;
  const float* b = y + ((size_t)n + N) * vec4 * 4;
  double s = 0.0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < vec4;
       i += (long long)gridDim.x * 256) {
    const f32x4 u = relu4(ld4(a + (size_t)i * 4)), v = relu4(ld4(b + (size_t)i * 4));
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float d = u[k] - v[k];
      s += (double)(d * d);
    }
  }
  s = wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0)
    partial[(size_t)n * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// per-image sums: the partials of one image in slab order
__global__ __launch_bounds__(256) void feature_mse_finalize_kernel(const double* __restrict__ partial,
                                                                   int N, int nblocks,
                                                                   double* __restrict__ sums) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  double s = 0.0;
  for (int b = 0; b < nblocks; ++b) s += partial[(size_t)n * nblocks + b];
  sums[n] = s;
}

// ------------------------------------------------------------------ ReLU / pool / tap backward
// dz = y_o > 0 ? g_in + coef * (relu(y_o) - relu(y_t)) : 0 for four channels
__device__ __forceinline__ f32x4 relu_bwd4(const f32x4 yo, const f32x4 g, bool tap, const f32x4 yt,
                                           float coef) {
  f32x4 o;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float v = g[k];
    if (tap) v = fmaf(coef, fmaxf(yo[k], 0.f) - fmaxf(yt[k], 0.f), v);
    o[k] = yo[k] > 0.f ? v : 0.f;
  }
  return o;
}

// g_in = the same-resolution gradient g, or nothing (g == nullptr)
__global__ __launch_bounds__(256) void perceptual_relu_bwd_kernel(const float* __restrict__ yo,
                                                                  const float* __restrict__ yt,
                                                                  float coef,
                                                                  const float* __restrict__ g,
                                                                  float* __restrict__ dz,
                                                                  long long vec4) {
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < vec4;
       i += (long long)gridDim.x * 256) {
    const size_t o = (size_t)i * 4;
    st4(dz + o, relu_bwd4(ld4(yo + o), g ? ld4(g + o) : zero, yt != nullptr,
                          yt ? ld4(yt + o) : zero, coef));
  }
}

// g_in = the gradient gp [N][Ho][Wo][C] of the following 2x2 max-pool, routed to the window's
// first maximum in row-major order (positions of an ignored odd row / column receive none).
// One item = four channels of one 2x2 window of the ceil(H/2) x ceil(W/2) window grid.
__global__ __launch_bounds__(256) void perceptual_relu_pool_bwd_kernel(
    const float* __restrict__ yo, const float* __restrict__ yt, float coef,
    const float* __restrict__ gp, float* __restrict__ dz, long long items, int H, int W, int Ho,
    int Wo, int Hc, int Wc, int C4) {
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items;
       i += (long long)gridDim.x * 256) {
    const int ch = (int)(i % C4);
    long long r = i / C4;
    const int xw = (int)(r % Wc);
    r /= Wc;
    const int yw = (int)(r % Hc);
    const long long n = r / Hc;
    const bool pooled = yw < Ho && xw < Wo;   // else: the odd last row / column
    f32x4 v[4], gsel[4];
    bool ok[4];
    size_t off[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int yy = 2 * yw + (q >> 1), xx = 2 * xw + (q & 1);
      ok[q] = yy < H && xx < W;
      off[q] = ((((size_t)n * H + yy) * W + xx) * C4 + ch) * 4;
      v[q] = ok[q] ? ld4(yo + off[q]) : zero;
      gsel[q] = zero;
    }
    if (pooled) {   // all four positions are inside the image
      const f32x4 gv = ld4(gp + ((((size_t)n * Ho + yw) * Wo + xw) * C4 + ch) * 4);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        // first maximum of the ReLU outputs: strictly above everything before it
        int best = 0;
        float m = fmaxf(v[0][k], 0.f);
#pragma unroll
        for (int q = 1; q < 4; ++q) {
          const float a = fmaxf(v[q][k], 0.f);
          if (a > m) { m = a; best = q; }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) gsel[q][k] = best == q ? gv[k] : 0.f;
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (ok[q])
        st4(dz + off[q], relu_bwd4(v[q], gsel[q], yt != nullptr, yt ? ld4(yt + off[q]) : zero, coef));
  }
}

// ------------------------------------------------------------------ data gradient of conv1_1
// dx[n][c][y][x] = (sum_{ky,kx,k} dz[n][y+1-ky][x+1-kx][k] w[k][c][ky][kx]) / std[c]: a Cout -> 3
// 3x3 convolution per pixel with the taps flipped, the structure of recon_fwd_kernel (recon.hip).
// A workgroup owns 8 rows x 32 columns of one image (one pixel per thread) and walks Cout in chunks
// of 32 channels: the 10 x 34 halo of the chunk in LDS as 340 pixels x 8 groups of four channels,
// the group index xor-swizzled by the pixel's low bits.
constexpr int STW = 32, STH = 8;
constexpr int SHW = STW + 2, SHH = STH + 2, SHP = SHW * SHH;   // 340 halo pixels
constexpr int SSTAGE = (SHP * 8 + 255) / 256;                  // 11 group loads per thread

__device__ __forceinline__ int ssw(int hp, int ch) { return hp * 8 + (ch ^ (hp & 7)); }

__global__ __launch_bounds__(256) void perceptual_stem_bwd_data_kernel(
    const float* __restrict__ dz, const float* __restrict__ w, float* __restrict__ dx, int H, int W,
    int Cout, const Norm3 nm) {
  __shared__ f32x4 at[SHP * 8];
  __shared__ f32x4 wl[9 * 3 * 8];
  const int tid = threadIdx.x;
  const int n = blockIdx.z, y0 = blockIdx.y * STH, x0 = blockIdx.x * STW;
  const int py = tid >> 5, px = tid & 31;
  const int ch = tid & 7;   // the same group on every staging pass (256 % 8 == 0)
  float acc[3] = {0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < Cout; k0 += 32) {
    __syncthreads();   // the previous chunk's LDS reads are done
    // weights of the chunk: wl[tap][c][group] = w[k0 + 4 group + jj][c][tap]
    for (int i = tid; i < 9 * 3 * 8; i += 256) {
      const int tap = i / 24, r = i - tap * 24, c = r >> 3, g = r & 7;
      f32x4 v;
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) v[jj] = w[((size_t)(k0 + g * 4 + jj) * 3 + c) * 9 + tap];
      wl[i] = v;
    }
    f32x4 v[SSTAGE];
#pragma unroll
    for (int it = 0; it < SSTAGE; ++it) {   // every load of the tile in flight together
      const int hp = (it * 256 + tid) >> 3;
      const int hy = hp / SHW, hx = hp - hy * SHW;
      const int y = y0 + hy - 1, x = x0 + hx - 1;
      const bool ok = hp < SHP && y >= 0 && y < H && x >= 0 && x < W;
      v[it] = ok ? ld4(dz + (((size_t)n * H + y) * W + x) * Cout + k0 + ch * 4)
                 : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int it = 0; it < SSTAGE; ++it) {
      const int hp = (it * 256 + tid) >> 3;
      if (hp < SHP) at[ssw(hp, ch)] = v[it];
    }
    __syncthreads();
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int hp = (py + 2 - tap / 3) * SHW + px + 2 - tap % 3;
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        const f32x4 d = at[ssw(hp, g)];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const f32x4 wv = wl[(tap * 3 + c) * 8 + g];
          acc[c] = fmaf(d[0], wv[0], acc[c]);
          acc[c] = fmaf(d[1], wv[1], acc[c]);
          acc[c] = fmaf(d[2], wv[2], acc[c]);
          acc[c] = fmaf(d[3], wv[3], acc[c]);
        }
      }
    }
  }
  const int y = y0 + py, x = x0 + px;
  if (y < H && x < W) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
      dx[(((size_t)n * 3 + c) * H + y) * W + x] = __fdiv_rn(acc[c], nm.std[c]);
  }
}

bool shape_ok(long long M, int H, int W, int C) {
  return M > 0 && M < 65536 && H > 0 && W > 0 && C > 0 && C % 32 == 0;
}

}  // namespace

extern "C" int unet_perceptual_prep(const float* out_nchw, const void* target, int target_u8,
                                    const float* mean3, const float* std3, float* xn, int N, int H,
                                    int W, unet_stream_t stream) {
  UNET_REQUIRE(out_nchw && target && mean3 && std3 && xn, "perceptual_prep: null pointer");
  UNET_REQUIRE(N > 0 && 2 * (long long)N < 65536 && H > 0 && W > 0, "perceptual_prep: bad shape");
  Norm3 nm;
  for (int c = 0; c < 3; ++c) {
    nm.mean[c] = mean3[c];
    nm.std[c] = std3[c];
  }
  const long long HW = (long long)H * W;
  const bool vec = HW % 4 == 0 && ((uintptr_t)out_nchw | (uintptr_t)target | (uintptr_t)xn) % 16 == 0;
  if (vec) {
    long long bx = ceil_div64(HW / 4, 256);
    if (bx > 1024) bx = 1024;
    hipLaunchKernelGGL(perceptual_prep_kernel<4>, dim3((unsigned)bx, (unsigned)(2 * N)), dim3(256),
                       0, (hipStream_t)stream, out_nchw, target, target_u8, xn, N, HW, nm);
  } else {
    long long bx = ceil_div64(HW, 256);
    if (bx > 1024) bx = 1024;
    hipLaunchKernelGGL(perceptual_prep_kernel<1>, dim3((unsigned)bx, (unsigned)(2 * N)), dim3(256),
                       0, (hipStream_t)stream, out_nchw, target, target_u8, xn, N, HW, nm);
  }
  UNET_CHECK_LAUNCH("perceptual_prep");
  return UNET_OK;
}

extern "C" int unet_relu_maxpool2x2_fwd(const float* y, float* p, int M, int H, int W, int C,
                                        unet_stream_t stream) {
  UNET_REQUIRE(y && p, "relu_maxpool2x2_fwd: null pointer");
  UNET_REQUIRE(shape_ok(M, H, W, C) && H >= 2 && W >= 2,
               "relu_maxpool2x2_fwd: needs H, W >= 2 and C %% 32 == 0 (got %dx%d C=%d)", H, W, C);
  const int Ho = H / 2, Wo = W / 2, C4 = C / 4;
  const long long items = (long long)M * Ho * Wo * C4;
  hipLaunchKernelGGL(relu_maxpool2x2_fwd_kernel, dim3(stream_grid(items)), dim3(256), 0,
                     (hipStream_t)stream, y, p, items, H, W, Ho, Wo, C4);
  UNET_CHECK_LAUNCH("relu_maxpool2x2_fwd");
  return UNET_OK;
}

extern "C" size_t unet_feature_mse_workspace_bytes(int N, int H, int W, int C) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 4) return 0;
  return (size_t)N * fm_blocks((long long)H * W * (C / 4)) * sizeof(double);
}

extern "C" int unet_feature_mse_fwd(const float* y, double* sums, void* workspace,
                                    size_t workspace_bytes, int N, int H, int W, int C,
                                    unet_stream_t stream) {
  UNET_REQUIRE(y && sums && workspace, "feature_mse_fwd: null pointer");
  UNET_REQUIRE(shape_ok(2 * (long long)N, H, W, C), "feature_mse_fwd: bad shape (C %% 32 == 0)");
  UNET_REQUIRE_WS(workspace_bytes, unet_feature_mse_workspace_bytes(N, H, W, C),
                  "feature_mse_fwd: workspace too small");
  const long long vec4 = (long long)H * W * (C / 4);
  const int blocks = fm_blocks(vec4);
  double* partial = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(feature_mse_reduce_kernel, dim3(blocks, N), dim3(256), 0, (hipStream_t)stream,
                     y, partial, N, vec4);
  UNET_CHECK_LAUNCH("feature_mse_reduce");
  hipLaunchKernelGGL(feature_mse_finalize_kernel, dim3(ceil_div(N, 256)), dim3(256), 0,
                     (hipStream_t)stream, partial, N, blocks, sums);
  UNET_CHECK_LAUNCH("feature_mse_finalize");
  return UNET_OK;
}

extern "C" int unet_perceptual_relu_bwd(const float* y_o, const float* y_t, float coef,
                                        const float* g, const float* gp, float* dz, int N, int H,
                                        int W, int C, unet_stream_t stream) {
  UNET_REQUIRE(y_o && dz, "perceptual_relu_bwd: null pointer");
  UNET_REQUIRE(!(g && gp), "perceptual_relu_bwd: g and gp are exclusive");
  UNET_REQUIRE(y_t || g || gp, "perceptual_relu_bwd: neither a tap nor an incoming gradient");
  UNET_REQUIRE(shape_ok(N, H, W, C), "perceptual_relu_bwd: bad shape (C %% 32 == 0)");
  const int C4 = C / 4;
  if (gp) {
    UNET_REQUIRE(H >= 2 && W >= 2, "perceptual_relu_bwd: a pooled layer needs H, W >= 2");
    const int Hc = (H + 1) / 2, Wc = (W + 1) / 2;
    const long long items = (long long)N * Hc * Wc * C4;
    hipLaunchKernelGGL(perceptual_relu_pool_bwd_kernel, dim3(stream_grid(items)), dim3(256), 0,
                       (hipStream_t)stream, y_o, y_t, coef, gp, dz, items, H, W, H / 2, W / 2, Hc,
                       Wc, C4);
  } else {
    const long long vec4 = (long long)N * H * W * C4;
    hipLaunchKernelGGL(perceptual_relu_bwd_kernel, dim3(stream_grid(vec4)), dim3(256), 0,
                       (hipStream_t)stream, y_o, y_t, coef, g, dz, vec4);
  }
  UNET_CHECK_LAUNCH("perceptual_relu_bwd");
  return UNET_OK;
}

extern "C" int unet_perceptual_stem_bwd_data(const float* dz, const float* w_oihw,
                                             const float* std3, float* dout_nchw, int N, int H,
                                             int W, int Cout, unet_stream_t stream) {
  UNET_REQUIRE(dz && w_oihw && std3 && dout_nchw, "perceptual_stem_bwd_data: null pointer");
  UNET_REQUIRE(shape_ok(N, H, W, Cout) && ceil_div(H, STH) < 65536,
               "perceptual_stem_bwd_data: bad shape (Cout %% 32 == 0, N < 65536)");
  Norm3 nm{};
  for (int c = 0; c < 3; ++c) nm.std[c] = std3[c];
  const dim3 grid((unsigned)ceil_div(W, STW), (unsigned)ceil_div(H, STH), (unsigned)N);
  hipLaunchKernelGGL(perceptual_stem_bwd_data_kernel, grid, dim3(256), 0, (hipStream_t)stream, dz,
                     w_oihw, dout_nchw, H, W, Cout, nm);
  UNET_CHECK_LAUNCH("perceptual_stem_bwd_data");
  return UNET_OK;
}
