// recon.hip — the autoencoder's pretraining step: 3x3 reconstruction head (conv 32 -> 3, pad 1,
// bias, sigmoid) forward and backward, the MSE loss against the input image, and Adam over the
// flat parameter arena.  All HBM-bound; every reduction goes through per-workgroup partials and
// a fixed-order finalize in double (no float atomics: bit-reproducible).
//
// Replaces reconstruction_output (AE_pretrained/reconstruction/models/autoencoder.py:377-387),
// nn.MSELoss (AE_pretrained/reconstruction/src/train.py:420-437) and optim.Adam (:377-397).
#include "common.h"
#include "conv_params.h"

namespace {
using unet_conv::act4;

// A workgroup owns a tile of 8 rows x 32 columns of one image (one output pixel per thread) and
// stages the ACTIVATED 10 x 34 halo of the 32-channel input in LDS: 340 pixels x 8 chunks of four
// channels, the chunk index xor-swizzled by the pixel's low bits so the eight b128 reads of
// neighbouring pixels fall on different banks.
constexpr int RTW = 32, RTH = 8;
constexpr int RHW = RTW + 2, RHH = RTH + 2, RHP = RHW * RHH;   // 340 halo pixels
constexpr int RK = 3;                                          // output channels
constexpr int RSTAGE = (RHP * 8 + 255) / 256;                  // 11 chunk loads per thread
constexpr int RCOLS = RK * 32 * 9 + RK;                        // dW (864) then db (3)
constexpr int RMAX_BLOCKS = 1024;

__device__ __forceinline__ int sw(int hp, int ch) { return hp * 8 + (ch ^ (hp & 7)); }

// the activated halo tile: lrelu(x * alpha + beta) inside the image, 0 in the padding (the
// padding is applied after the activation, as the reference's Conv2d sees it)
template <typename TS>
__device__ __forceinline__ void stage_act_tile(f32x4* __restrict__ at, const TS* __restrict__ a,
                                               const float* __restrict__ alpha,
                                               const float* __restrict__ beta, float slope, int n,
                                               int y0, int x0, int H, int W) {
  const int tid = threadIdx.x;
  const int ch = tid & 7;        // the same chunk on every pass (256 % 8 == 0)
  f32x4 al = {1.f, 1.f, 1.f, 1.f}, be = {0.f, 0.f, 0.f, 0.f};
  if (alpha) {
    al = *reinterpret_cast<const f32x4*>(alpha + (size_t)n * 32 + ch * 4);
    be = *reinterpret_cast<const f32x4*>(beta + (size_t)n * 32 + ch * 4);
  }
  f32x4 v[RSTAGE];
  bool ok[RSTAGE];
#pragma unroll
  for (int it = 0; it < RSTAGE; ++it) {   // every load of the tile in flight together
    const int hp = (it * 256 + tid) >> 3;
    const int hy = hp / RHW, hx = hp - hy * RHW;
    const int y = y0 + hy - 1, x = x0 + hx - 1;
    ok[it] = hp < RHP && y >= 0 && y < H && x >= 0 && x < W;
    v[it] = ok[it] ? ld4(a + (((size_t)n * H + y) * W + x) * 32 + ch * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int it = 0; it < RSTAGE; ++it) {
    const int hp = (it * 256 + tid) >> 3;
    if (hp < RHP) {
      f32x4 u = v[it];
      if (alpha) u = act4(u, al, be, slope, ok[it]);
      at[sw(hp, ch)] = u;
    }
  }
}

// weights w[k][c][ky][kx] (OIHW) -> LDS wl[tap][k][c] (four channels per f32x4)
__device__ __forceinline__ void stage_weights(f32x4* __restrict__ wl, const float* __restrict__ w) {
  for (int i = threadIdx.x; i < 9 * RK * 8; i += 256) {
    const int tap = i / (RK * 8), r = i - tap * RK * 8, k = r >> 3, ch = r & 7;
    f32x4 v;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) v[jj] = w[(k * 32 + ch * 4 + jj) * 9 + tap];
    wl[i] = v;
  }
}

// ------------------------------------------------------------------ forward
template <typename TS>
__global__ __launch_bounds__(256) void recon_fwd_kernel(const TS* __restrict__ a,
                                                        const float* __restrict__ alpha,
                                                        const float* __restrict__ beta, float slope,
                                                        const float* __restrict__ w,
                                                        const float* __restrict__ b,
                                                        float* __restrict__ out, int H, int W) {
  __shared__ f32x4 at[RHP * 8];
  __shared__ f32x4 wl[9 * RK * 8];
  const int n = blockIdx.z, y0 = blockIdx.y * RTH, x0 = blockIdx.x * RTW;
  stage_weights(wl, w);
  stage_act_tile(at, a, alpha, beta, slope, n, y0, x0, H, W);
  __syncthreads();
  const int py = threadIdx.x >> 5, px = threadIdx.x & 31;
  float acc[RK];
#pragma unroll
  for (int k = 0; k < RK; ++k) acc[k] = b ? b[k] : 0.f;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int hp = (py + tap / 3) * RHW + px + tap % 3;
#pragma unroll
    for (int ch = 0; ch < 8; ++ch) {
      const f32x4 v = at[sw(hp, ch)];
#pragma unroll
      for (int k = 0; k < RK; ++k) {
        const f32x4 wv = wl[(tap * RK + k) * 8 + ch];
        acc[k] = fmaf(v[0], wv[0], acc[k]);
        acc[k] = fmaf(v[1], wv[1], acc[k]);
        acc[k] = fmaf(v[2], wv[2], acc[k]);
        acc[k] = fmaf(v[3], wv[3], acc[k]);
      }
    }
  }
  const int y = y0 + py, x = x0 + px;
  if (y < H && x < W) {
#pragma unroll
    for (int k = 0; k < RK; ++k)
      out[(((size_t)n * RK + k) * H + y) * W + x] = 1.f / (1.f + expf(-acc[k]));
  }
}

// ------------------------------------------------------------------ backward
struct ReconBs {   // InstanceNorm-backward reductions of the layer in front of the head
  const float* mean; const float* rstd; const float* gamma; const float* beta; const float* mask;
  float2* partial;          // nullptr: no reductions
};

// Workgroup b takes the contiguous tiles [b * tpb, (b + 1) * tpb) of ONE image (tpb divides the
// tiles of an image).  Per tile: dz = dout * out * (1 - out) of the 10 x 34 halo and the activated
// input halo go to LDS; each thread writes da of its pixel (the 3 -> 32 transposed 3x3 conv of
// dz); 216 threads own one (tap, four channels, third of the pixels) slot of dW each and keep
// its 3 x 4 sums in registers over all the workgroup's tiles.
template <typename TS, bool BS>
__global__ __launch_bounds__(256) void recon_bwd_kernel(
    const TS* __restrict__ a, const float* __restrict__ alpha, const float* __restrict__ beta,
    float slope, const float* __restrict__ dout, const float* __restrict__ out,
    const float* __restrict__ w, TS* __restrict__ da, float* __restrict__ partial, int H, int W,
    int tiles_x, int tiles_per_image, int tpb, const ReconBs bs) {
  __shared__ f32x4 at[RHP * 8];
  __shared__ f32x4 dzt[RHP];
  __shared__ f32x4 wl[9 * RK * 8];
  const int tid = threadIdx.x;
  const int py = tid >> 5, px = tid & 31;
  stage_weights(wl, w);
  // dW slot of this thread
  const int job = tid < 216 ? tid : 0;
  const int pq = job / 72, jr = job - pq * 72, jtap = jr >> 3, jch = jr & 7;
  f32x4 dwacc[RK];
  float dbacc[RK];
#pragma unroll
  for (int k = 0; k < RK; ++k) {
    dwacc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    dbacc[k] = 0.f;
  }
  constexpr bool with_bs = BS;   // bs.partial != nullptr
  float s1[32], s2[32];
#pragma unroll
  for (int c = 0; c < 32; ++c) s1[c] = s2[c] = 0.f;
  const int t_first = blockIdx.x * tpb;
  const int n = t_first / tiles_per_image;
  const size_t HW = (size_t)H * W;
  for (int t = t_first; t < t_first + tpb; ++t) {
    const int r = t - n * tiles_per_image;
    const int ty = r / tiles_x, tx = r - ty * tiles_x;
    const int y0 = ty * RTH, x0 = tx * RTW;
    __syncthreads();   // the previous tile's LDS reads are done
    for (int hp = tid; hp < RHP; hp += 256) {
      const int hy = hp / RHW, hx = hp - hy * RHW;
      const int y = y0 + hy - 1, x = x0 + hx - 1;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (y >= 0 && y < H && x >= 0 && x < W) {
#pragma unroll
        for (int k = 0; k < RK; ++k) {
          const size_t o = ((size_t)n * RK + k) * HW + (size_t)y * W + x;
          const float s = out[o];
          v[k] = dout[o] * s * (1.f - s);
        }
      }
      dzt[hp] = v;
    }
    stage_act_tile(at, a, alpha, beta, slope, n, y0, x0, H, W);
    __syncthreads();
    // da of this thread's pixel: da[y][x][c] = sum_{ky,kx,k} dz[k][y+1-ky][x+1-kx] w[k][c][ky][kx]
    {
      f32x4 acc[8];
#pragma unroll
      for (int ch = 0; ch < 8; ++ch) acc[ch] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const f32x4 dz = dzt[(py + 2 - tap / 3) * RHW + px + 2 - tap % 3];
#pragma unroll
        for (int k = 0; k < RK; ++k)
#pragma unroll
          for (int ch = 0; ch < 8; ++ch) {
            const f32x4 wv = wl[(tap * RK + k) * 8 + ch];
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) acc[ch][jj] = fmaf(dz[k], wv[jj], acc[ch][jj]);
          }
      }
      const int y = y0 + py, x = x0 + px;
      const f32x4 dzc = dzt[(py + 1) * RHW + px + 1];   // 0 outside the image
#pragma unroll
      for (int k = 0; k < RK; ++k) dbacc[k] += dzc[k];
      if (y < H && x < W) {
        const size_t pix = ((size_t)n * H + y) * W + x;
#pragma unroll
        for (int ch = 0; ch < 8; ++ch) st4(da + pix * 32 + ch * 4, acc[ch]);
        if (with_bs) {   // uniform
          // S1 = sum gz, S2 = sum gz * xhat, gz = da * mask * (z > 0 ? 1 : slope) (fp32 da, as the
          // 1x1 head's and the convolutions' epilogues)
#pragma unroll
          for (int ch = 0; ch < 8; ++ch) {
            const size_t o = (size_t)n * 32 + ch * 4;
            const f32x4 yv = ld4(a + pix * 32 + ch * 4);
            const f32x4 g = *reinterpret_cast<const f32x4*>(bs.gamma + ch * 4);
            const f32x4 bb = *reinterpret_cast<const f32x4*>(bs.beta + ch * 4);
            const f32x4 mu = *reinterpret_cast<const f32x4*>(bs.mean + o);
            const f32x4 rs = *reinterpret_cast<const f32x4*>(bs.rstd + o);
            const f32x4 mk = bs.mask ? *reinterpret_cast<const f32x4*>(bs.mask + o)
                                     : f32x4{1.f, 1.f, 1.f, 1.f};
            const f32x4 cA = g * rs, cB = bb - mu * cA;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
              const float z = fmaf(yv[jj], cA[jj], cB[jj]);
              const float gz = acc[ch][jj] * mk[jj] * (z > 0.f ? 1.f : slope);
              s1[ch * 4 + jj] += gz;
              s2[ch * 4 + jj] = fmaf(gz, (yv[jj] - mu[jj]) * rs[jj], s2[ch * 4 + jj]);
            }
          }
        }
      }
    }
    // dW slot: sum over this third of the tile's pixels of dz[k](p) * act(a)[p + tap][c]
    if (tid < 216) {
      const int ky = jtap / 3, kx = jtap - ky * 3;
      for (int p = pq; p < RTW * RTH; p += 3) {
        const int qy = p >> 5, qx = p & 31;
        const f32x4 dz = dzt[(qy + 1) * RHW + qx + 1];
        const int hp = (qy + ky) * RHW + qx + kx;
        const f32x4 v = at[sw(hp, jch)];
#pragma unroll
        for (int k = 0; k < RK; ++k)
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) dwacc[k][jj] = fmaf(dz[k], v[jj], dwacc[k][jj]);
      }
    }
  }
  __syncthreads();
  // per-workgroup partial: the three pixel thirds merged in fixed order
  float* red = reinterpret_cast<float*>(at);
  if (tid < 216) {
#pragma unroll
    for (int k = 0; k < RK; ++k)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) red[tid * 12 + k * 4 + jj] = dwacc[k][jj];
  }
  const int lane = tid & 63, wave = tid >> 6;
  float* redb = red + 216 * 12;   // [4 waves][RK]
#pragma unroll
  for (int k = 0; k < RK; ++k) {
    const float s = wave_sum(dbacc[k]);
    if (lane == 0) redb[wave * RK + k] = s;
  }
  __syncthreads();
  float* pw = partial + (size_t)blockIdx.x * RCOLS;
  if (tid < 72) {
    const int tap = tid >> 3, ch = tid & 7;
#pragma unroll
    for (int k = 0; k < RK; ++k)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int i = k * 4 + jj;
        const float s = (red[tid * 12 + i] + red[(tid + 72) * 12 + i]) + red[(tid + 144) * 12 + i];
        pw[(k * 32 + ch * 4 + jj) * 9 + tap] = s;
      }
  } else if (tid < 72 + RK) {
    const int k = tid - 72;
    pw[RK * 32 * 9 + k] = (redb[k] + redb[RK + k]) + (redb[2 * RK + k] + redb[3 * RK + k]);
  }
  if (with_bs) {   // uniform: per channel, wave sums then the four waves in order
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 32; ++c) {
      const float a1 = wave_sum(s1[c]), a2 = wave_sum(s2[c]);
      if (lane == 0) {
        red[(wave * 32 + c) * 2] = a1;
        red[(wave * 32 + c) * 2 + 1] = a2;
      }
    }
    __syncthreads();
    if (tid < 64) {
      const int c = tid >> 1, q = tid & 1;
      const float s = (red[(c) * 2 + q] + red[(32 + c) * 2 + q]) +
                      (red[(64 + c) * 2 + q] + red[(96 + c) * 2 + q]);
      // partial[(image * summaries_per_image + j) * 32 + c] = (S1, S2): workgroup b IS summary b
      reinterpret_cast<float*>(bs.partial)[((size_t)blockIdx.x * 32 + c) * 2 + q] = s;
    }
  }
}

// one block per column (864 weights then 3 biases): 256 threads stride the slabs in double,
// fixed-order tree
__global__ __launch_bounds__(256) void recon_bwd_finalize_kernel(const float* __restrict__ partial,
                                                                 float* __restrict__ dw,
                                                                 float* __restrict__ db,
                                                                 int nblocks) {
  __shared__ double red[256];
  const int i = blockIdx.x;
  double s = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += 256) s += (double)partial[(size_t)b * RCOLS + i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (i < RK * 32 * 9) dw[i] = (float)red[0];
    else db[i - RK * 32 * 9] = (float)red[0];
  }
}

// ------------------------------------------------------------------ MSE loss
constexpr int MSE_BLOCKS = 64;   // per image

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// target: fp32 NCHW (u8 == 0) or the dataset's uint8 NHWC image, t = v / 255 in fp32
__device__ __forceinline__ float mse_target(const void* target, int u8, int n, int k, int C,
                                            size_t HW, size_t p) {
  if (u8) {
    const unsigned char v = reinterpret_cast<const unsigned char*>(target)[((size_t)n * HW + p) * C + k];
    // double quotient rounded once to fp32: equal to the correctly rounded fp32 v / 255 for
    // every v (the fp32 division of the reference's CPU dataset; the device's fp32 division is
    // not correctly rounded by default)
    return (float)((double)v / 255.0);
  }
  return reinterpret_cast<const float*>(target)[((size_t)n * C + k) * HW + p];
}

__global__ __launch_bounds__(256) void mse_reduce_kernel(const float* __restrict__ out,
                                                         const void* __restrict__ target, int u8,
                                                         double* __restrict__ partial, int C,
                                                         long long HW) {
  __shared__ double red[4];
  const int n = blockIdx.y;
  double s = 0.0;
  for (int k = 0; k < C; ++k) {
    const float* o = out + ((size_t)n * C + k) * HW;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < HW; p += (long long)gridDim.x * 256) {
      const float d = o[p] - mse_target(target, u8, n, k, C, HW, p);
      s += (double)(d * d);
    }
  }
  s = wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0)
    partial[(size_t)n * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// single block: per-image sums (slab order), then the mean over N * C * H * W
__global__ __launch_bounds__(256) void mse_finalize_kernel(const double* __restrict__ partial,
                                                           int N, int nblocks, double numel,
                                                           double* __restrict__ per_image,
                                                           float* __restrict__ loss_out) {
  for (int n = threadIdx.x; n < N; n += 256) {
    double s = 0.0;
    for (int b = 0; b < nblocks; ++b) s += partial[(size_t)n * nblocks + b];
    per_image[n] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int n = 0; n < N; ++n) s += per_image[n];
    loss_out[0] = (float)(s / numel);
  }
}

// dout = upstream * (2 / numel) * (out - t); one (image, channel) plane per grid row
__global__ __launch_bounds__(256) void mse_grad_kernel(const float* __restrict__ out,
                                                       const void* __restrict__ target, int u8,
                                                       const float* __restrict__ upstream,
                                                       float* __restrict__ dout, int C,
                                                       long long HW, float norm) {
  const int n = blockIdx.y / C, k = blockIdx.y - n * C;
  const float up = upstream ? upstream[0] : 1.f;
  const size_t base = ((size_t)n * C + k) * HW;
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < HW; p += (long long)gridDim.x * 256) {
    const float d = out[base + p] - mse_target(target, u8, n, k, C, HW, p);
    dout[base + p] = norm * d * up;
  }
}

// ------------------------------------------------------------------ Adam
// hyper (fp64, device): {lr, beta1, beta2, eps, weight_decay, grad_scale, step, -}.  The bias
// corrections are formed in double from the step count, as torch.optim.Adam does on the host.
__global__ void adam_advance_kernel(double* __restrict__ hyper) { hyper[6] += 1.0; }

__device__ __forceinline__ float adam_one(float& p, float g, float& m, float& v, float gs, float wd,
                                          float b1c, float b2, float b2c, float ss, float bc2s,
                                          float eps) {
  g = g * gs + wd * p;
  m = m + b1c * (g - m);                        // torch: exp_avg.lerp_(grad, 1 - beta1)
  v = v * b2 + b2c * g * g;                     // exp_avg_sq.mul_(beta2).addcmul_(g, g, 1 - beta2)
  const float denom = sqrtf(v) / bc2s + eps;
  p = p + (-ss * m) / denom;                    // param.addcdiv_(exp_avg, denom, -step_size)
  return p;
}

template <bool VEC>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v,
                                                   long long n, const double* __restrict__ hyper) {
  const double lr = hyper[0], b1 = hyper[1], b2 = hyper[2], t = hyper[6];
  const float eps = (float)hyper[3], wd = (float)hyper[4], gs = (float)hyper[5];
  const float ss = (float)(lr / (1.0 - pow(b1, t)));
  const float bc2s = (float)sqrt(1.0 - pow(b2, t));
  const float b1c = (float)(1.0 - b1), b2f = (float)b2, b2c = (float)(1.0 - b2);
  const long long stride = (long long)gridDim.x * 256;
  if (VEC) {
    const long long n4 = n >> 2;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
      f32x4 pv = *reinterpret_cast<f32x4*>(p + i * 4);
      const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i * 4);
      f32x4 mv = *reinterpret_cast<f32x4*>(m + i * 4);
      f32x4 vv = *reinterpret_cast<f32x4*>(v + i * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float pj = pv[j], mj = mv[j], vj = vv[j];
        adam_one(pj, gv[j], mj, vj, gs, wd, b1c, b2f, b2c, ss, bc2s, eps);
        pv[j] = pj; mv[j] = mj; vv[j] = vj;
      }
      *reinterpret_cast<f32x4*>(p + i * 4) = pv;
      *reinterpret_cast<f32x4*>(m + i * 4) = mv;
      *reinterpret_cast<f32x4*>(v + i * 4) = vv;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
      const long long i = (n4 << 2) + threadIdx.x;
      adam_one(p[i], g[i], m[i], v[i], gs, wd, b1c, b2f, b2c, ss, bc2s, eps);
    }
  } else {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride)
      adam_one(p[i], g[i], m[i], v[i], gs, wd, b1c, b2f, b2c, ss, bc2s, eps);
  }
}

unsigned adam_grid(long long items) {
  long long b = ceil_div64(items, 256);
  if (b > 256 * 16) b = 256 * 16;
  if (b < 1) b = 1;
  return (unsigned)b;
}

// tiles per workgroup of the head backward: the smallest divisor of the tiles of one image that
// keeps the grid within RMAX_BLOCKS (a workgroup's tiles then always lie in one image)
int recon_tpb(int N, int tiles_per_image) {
  const long long tiles = (long long)N * tiles_per_image;
  for (int d = (int)ceil_div64(tiles, RMAX_BLOCKS); d <= tiles_per_image; ++d)
    if (tiles_per_image % d == 0) return d;
  return tiles_per_image;
}

int recon_shape_ok(int N, int H, int W) { return N > 0 && N <= RMAX_BLOCKS && H > 0 && W > 0; }

}  // namespace

extern "C" int unet_recon3x3_fwd(const unet_act_src* x, int x_bf16, float slope, const float* w,
                                 const float* b, float* out, int N, int H, int W, int K,
                                 unet_stream_t stream) {
  UNET_REQUIRE(x && x->x && w && b && out && (!x->alpha || x->beta), "recon3x3_fwd: null pointer");
  UNET_REQUIRE(x->C == 32 && K == RK && recon_shape_ok(N, H, W),
               "recon3x3_fwd: needs C == 32, K == 3, 0 < N <= 1024 (got C=%d K=%d N=%d)", x->C, K, N);
  const dim3 grid((unsigned)ceil_div(W, RTW), (unsigned)ceil_div(H, RTH), (unsigned)N);
  if (x_bf16)
    hipLaunchKernelGGL(recon_fwd_kernel<__bf16>, grid, dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const __bf16*>(x->x), x->alpha, x->beta, slope, w, b, out,
                       H, W);
  else
    hipLaunchKernelGGL(recon_fwd_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const float*>(x->x), x->alpha, x->beta, slope, w, b, out,
                       H, W);
  UNET_CHECK_LAUNCH("recon_fwd");
  return UNET_OK;
}

extern "C" size_t unet_recon3x3_bwd_workspace_bytes(int N, int H, int W) {
  if (!recon_shape_ok(N, H, W)) return 0;
  const int tpi = ceil_div(W, RTW) * ceil_div(H, RTH);
  const int blocks = N * tpi / recon_tpb(N, tpi);
  return (size_t)blocks * RCOLS * sizeof(float);
}

extern "C" int unet_recon3x3_bwd(const unet_act_src* x, int x_bf16, float slope,
                                 const float* dout, const float* out, const float* w, void* da,
                                 float* dw, float* db, void* workspace, size_t workspace_bytes,
                                 int N, int H, int W, int K, unet_bwd_stats* bs,
                                 unet_stream_t stream) {
  UNET_REQUIRE(x && x->x && (!x->alpha || x->beta) && dout && out && w && da && dw && db &&
                   workspace, "recon3x3_bwd: null pointer");
  UNET_REQUIRE(x->C == 32 && K == RK && recon_shape_ok(N, H, W),
               "recon3x3_bwd: needs C == 32, K == 3, 0 < N <= 1024 (got C=%d K=%d N=%d)", x->C, K, N);
  UNET_REQUIRE_WS(workspace_bytes, unet_recon3x3_bwd_workspace_bytes(N, H, W),
                  "recon3x3_bwd: workspace too small");
  const int tiles_x = ceil_div(W, RTW), tpi = tiles_x * ceil_div(H, RTH);
  const int tpb = recon_tpb(N, tpi);
  const int blocks = N * tpi / tpb;
  ReconBs rb{};
  if (bs) {
    bs->tiles_out = 0;
    if (x->alpha && bs->y == x->x && bs->mean && bs->rstd && bs->gamma && bs->beta &&
        bs->partial && bs->partial_bytes >= (size_t)blocks * 32 * sizeof(float2)) {
      UNET_REQUIRE(bs->slope == slope, "recon3x3_bwd: bs->slope differs from slope");
      rb.mean = bs->mean; rb.rstd = bs->rstd; rb.gamma = bs->gamma; rb.beta = bs->beta;
      rb.mask = bs->mask; rb.partial = reinterpret_cast<float2*>(bs->partial);
      bs->tiles_out = tpi / tpb;   // summaries per image
    }
  }
  float* partial = reinterpret_cast<float*>(workspace);
  const bool with_bs = rb.partial != nullptr;
  if (x_bf16) {
    auto kern = with_bs ? recon_bwd_kernel<__bf16, true> : recon_bwd_kernel<__bf16, false>;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const __bf16*>(x->x), x->alpha, x->beta, slope, dout, out,
                       w, reinterpret_cast<__bf16*>(da), partial, H, W, tiles_x, tpi, tpb, rb);
  } else {
    auto kern = with_bs ? recon_bwd_kernel<float, true> : recon_bwd_kernel<float, false>;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const float*>(x->x), x->alpha, x->beta, slope, dout, out,
                       w, reinterpret_cast<float*>(da), partial, H, W, tiles_x, tpi, tpb, rb);
  }
  UNET_CHECK_LAUNCH("recon_bwd");
  hipLaunchKernelGGL(recon_bwd_finalize_kernel, dim3(RCOLS), dim3(256), 0, (hipStream_t)stream,
                     partial, dw, db, blocks);
  UNET_CHECK_LAUNCH("recon_bwd_finalize");
  return UNET_OK;
}

namespace {
int mse_blocks(long long HW) {
  long long b = ceil_div64(HW, 256 * 8);
  if (b > MSE_BLOCKS) b = MSE_BLOCKS;
  return b < 1 ? 1 : (int)b;
}
}  // namespace

extern "C" size_t unet_mse_loss_workspace_bytes(int N, int C, int H, int W) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)N * mse_blocks((long long)H * W) * sizeof(double);
}

extern "C" int unet_mse_loss_fwd(const float* out, const void* target, int target_u8,
                                 float* loss_out, double* per_image, void* workspace,
                                 size_t workspace_bytes, int N, int C, int H, int W,
                                 unet_stream_t stream) {
  UNET_REQUIRE(out && target && loss_out && per_image && workspace, "mse_loss_fwd: null pointer");
  UNET_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && (!target_u8 || C == 3),
               "mse_loss_fwd: bad shape (a uint8 target needs C == 3)");
  UNET_REQUIRE_WS(workspace_bytes, unet_mse_loss_workspace_bytes(N, C, H, W),
                  "mse_loss_fwd: workspace too small");
  const long long HW = (long long)H * W;
  const int blocks = mse_blocks(HW);
  double* partial = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(mse_reduce_kernel, dim3(blocks, N), dim3(256), 0, (hipStream_t)stream, out,
                     target, target_u8, partial, C, HW);
  UNET_CHECK_LAUNCH("mse_reduce");
  hipLaunchKernelGGL(mse_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, N,
                     blocks, (double)N * C * HW, per_image, loss_out);
  UNET_CHECK_LAUNCH("mse_finalize");
  return UNET_OK;
}

extern "C" int unet_mse_loss_grad(const float* out, const void* target, int target_u8,
                                  const float* upstream, float* dout, int N, int C, int H, int W,
                                  unet_stream_t stream) {
  UNET_REQUIRE(out && target && dout, "mse_loss_grad: null pointer");
  UNET_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && (!target_u8 || C == 3) && (long long)N * C < 65536,
               "mse_loss_grad: bad shape (a uint8 target needs C == 3)");
  const long long HW = (long long)H * W;
  long long bx = ceil_div64(HW, 256 * 4);
  if (bx > 1024) bx = 1024;
  hipLaunchKernelGGL(mse_grad_kernel, dim3((unsigned)bx, (unsigned)(N * C)), dim3(256), 0,
                     (hipStream_t)stream, out, target, target_u8, upstream, dout, C, HW,
                     (float)(2.0 / ((double)N * C * HW)));
  UNET_CHECK_LAUNCH("mse_grad");
  return UNET_OK;
}

extern "C" int unet_adam_step(float* params, const float* grads, float* exp_avg,
                              float* exp_avg_sq, int64_t n, double* hyper, int advance_step,
                              unet_stream_t stream) {
  UNET_REQUIRE(params && grads && exp_avg && exp_avg_sq && hyper && n > 0,
               "adam_step: bad argument");
  if (advance_step) {
    hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, hyper);
    UNET_CHECK_LAUNCH("adam_advance");
  }
  const bool vec = ((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg |
                    (uintptr_t)exp_avg_sq) % 16 == 0;
  if (vec)
    hipLaunchKernelGGL(adam_kernel<true>, dim3(adam_grid((n + 3) / 4)), dim3(256), 0,
                       (hipStream_t)stream, params, grads, exp_avg, exp_avg_sq, (long long)n, hyper);
  else
    hipLaunchKernelGGL(adam_kernel<false>, dim3(adam_grid(n)), dim3(256), 0, (hipStream_t)stream,
                       params, grads, exp_avg, exp_avg_sq, (long long)n, hyper);
  UNET_CHECK_LAUNCH("adam");
  return UNET_OK;
}
