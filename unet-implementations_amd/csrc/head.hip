// head.hip — the 1x1 segmentation head (NHWC activations -> NCHW logits), forward and backward,
// for 1 <= K <= 32 classes.  Two kernel sets behind the unet_head1x1_* entry points, which check
// the operands and choose on K:
//
//   K <= 4   head_fwd_kernel / head_bwd_kernel / head_bwd_finalize_kernel on the vector units: the
//            head of the 3-class network, with the InstanceNorm-backward reductions and the fold
//            of the layer in front
//   K > 4    headk_fwd_kernel / headk_bwd_kernel / headk_bwd_finalize_kernel on the fp32 matrix
//            cores: plain da, no reductions
//
// Both are HBM-bound; dw / db go through per-block slabs and a finalize in fixed order.
//
// Replaces segmentation_output (Our_UNet/models/unet.py:374-381,:430).
#include "common.h"
#include "conv_params.h"

namespace {
using unet_conv::act4;

constexpr int HT = 256;  // pixels per head tile
// ... of the backward kernel, whose tile lives in registers: 64 pixels = 92 VGPRs, five waves per
// SIMD.  At 256 pixels (234 VGPRs, two waves) it ran at 2.1 TB/s: 192 -> 136 us on fp32 tensors,
// 161 -> 108 us on bf16 (tools/bench_head.py; 128 pixels: 178 VGPRs, no gain; 32: 164 / 119 us).
#ifndef UNET_HEAD_BWD_TILE
#define UNET_HEAD_BWD_TILE 64
#endif
constexpr int HB = UNET_HEAD_BWD_TILE;

// ------------------------------------------------------------------ head forward
// 8 lanes per pixel, 4 channels per lane: a wave's load instruction reads 8 whole pixels
// (1 KB contiguous), the 32-channel dot products are finished with three xor-shuffles inside
// each 8-lane group; no LDS.  Lane 0 of a group writes the pixel's K logits (NCHW planes).
template <typename TS>
__global__ __launch_bounds__(256) void head_fwd_kernel(const TS* __restrict__ a,
                                                       const float* __restrict__ w,
                                                       const float* __restrict__ b,
                                                       float* __restrict__ logits, long long M,
                                                       int HW, int K,
                                                       const float* __restrict__ alpha,
                                                       const float* __restrict__ beta,
                                                       float slope) {
  // alpha != nullptr (fused layer pipeline): `a` is the raw output of the last convolution
  // and its InstanceNorm + LeakyReLU + dropout is applied on load
  const int tid = threadIdx.x;
  const int seg = tid & 7;                       // channels 4*seg .. 4*seg+3
  f32x4 wk[4];
  float bk[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    wk[k] = k < K ? *reinterpret_cast<const f32x4*>(w + k * 32 + seg * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    bk[k] = (k < K && b) ? b[k] : 0.f;
  }
  const long long m0 = (long long)blockIdx.x * HT;
  // all loads of the tile first (rows past M are clamped and masked: no branch, the eight pixel
  // loads are in flight together); one coefficient row and one image index for the whole tile
  // where a tile never straddles images (no 64-bit division per pixel) - as head_bwd_kernel
  const bool one_image = HW % HT == 0;
  const long long n_tile = m0 / HW;
  f32x4 al = {1.f, 1.f, 1.f, 1.f}, be = {0.f, 0.f, 0.f, 0.f};
  if (alpha && one_image) {
    const size_t o = (size_t)n_tile * 32 + seg * 4;
    al = *reinterpret_cast<const f32x4*>(alpha + o);
    be = *reinterpret_cast<const f32x4*>(beta + o);
  }
  f32x4 av[HT / 32];
#pragma unroll
  for (int it = 0; it < HT / 32; ++it) {          // 32 pixels per pass of the 256 threads
    const long long m = m0 + it * 32 + (tid >> 3);
    const long long mc = m < M ? m : M - 1;
    av[it] = ld4(a + (size_t)mc * 32 + seg * 4);
  }
#pragma unroll
  for (int it = 0; it < HT / 32; ++it) {
    const long long m = m0 + it * 32 + (tid >> 3);
    const long long mc = m < M ? m : M - 1;
    const long long n = one_image ? n_tile : mc / HW;
    f32x4 v = av[it];
    if (alpha) {   // uniform
      if (!one_image) {
        al = *reinterpret_cast<const f32x4*>(alpha + (size_t)n * 32 + seg * 4);
        be = *reinterpret_cast<const f32x4*>(beta + (size_t)n * 32 + seg * 4);
      }
      v = act4(v, al, be, slope, true);
    }
    float acc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      // same accumulation order inside a lane as the scalar loop: c = 4*seg .. 4*seg+3
      float s = v[0] * wk[k][0];
      s = fmaf(v[1], wk[k][1], s);
      s = fmaf(v[2], wk[k][2], s);
      s = fmaf(v[3], wk[k][3], s);
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      s += __shfl_xor(s, 4, 64);
      acc[k] = s + bk[k];
    }
    if (seg == 0 && m < M) {
      const long long pp = m - n * HW;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < K) logits[((size_t)n * K + k) * HW + pp] = acc[k];
    }
  }
}

// ------------------------------------------------------------------ head backward
// InstanceNorm-backward reductions of the layer in front of the head (unet_bwd_stats)
struct HeadBs {
  const float* mean; const float* rstd; const float* gamma; const float* beta; const float* mask;
  float2* partial;          // nullptr: no reductions
  int tiles_per_block;
  // apply != 0 (second launch of unet_head1x1_in_bwd_fold, fp32 tensors): da is not a result.
  // The launch forms it again per lane, applies that layer's InstanceNorm + LeakyReLU + dropout
  // backward with coef = (c1, c2) per image and channel and writes dz where da would go;
  // workgroup 0 also writes the layer's parameter gradients from `sums` (N images).
  int apply;
  const float2* coef; const float2* sums;
  float* dgamma; float* dbeta; float* dbias;
  int N;
};

// The apply launch: same tiles per workgroup, same loads and the same multiply-add order for da
// as the launch below; nothing is reduced.  Every tile is whole (the launcher checks M % HB == 0)
// and a workgroup's tiles lie in one image.
__device__ __forceinline__ void head_bwd_apply_body(const float* __restrict__ a,
                                                    const float* __restrict__ dl,
                                                    const float* __restrict__ w,
                                                    float* __restrict__ dz, int HW, int K,
                                                    long long tiles, float slope,
                                                    const HeadBs& bs) {
  const int tid = threadIdx.x;
  const int seg = tid & 7, grp = tid >> 3;
  if (blockIdx.x == 0)
    in_bwd_param_grads(bs.sums, bs.coef, bs.gamma, bs.rstd, bs.N, HW, 32, tid, 256, bs.dgamma,
                       bs.dbeta, bs.dbias);
  f32x4 wk[4];
#pragma unroll
  for (int k = 0; k < 4; ++k)
    wk[k] = k < K ? *reinterpret_cast<const f32x4*>(w + k * 32 + seg * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
  const long long t_first = (long long)blockIdx.x * bs.tiles_per_block;
  const long long t_last = min(t_first + bs.tiles_per_block, tiles);
  const long long n = t_first * HB / HW;
  const size_t o = (size_t)n * 32 + seg * 4;
  const f32x4 mu = *reinterpret_cast<const f32x4*>(bs.mean + o);
  const f32x4 rs = *reinterpret_cast<const f32x4*>(bs.rstd + o);
  const f32x4 al = *reinterpret_cast<const f32x4*>(bs.gamma + seg * 4) * rs;
  const f32x4 be = in_bwd_shift(*reinterpret_cast<const f32x4*>(bs.beta + seg * 4), mu, al);
  const f32x4 mk = bs.mask ? *reinterpret_cast<const f32x4*>(bs.mask + o) : f32x4{1.f, 1.f, 1.f, 1.f};
  f32x4 c1, c2;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float2 cf = bs.coef[o + k];
    c1[k] = cf.x;
    c2[k] = cf.y;
  }
  for (long long t = t_first; t < t_last; ++t) {
    const long long m0 = t * HB;
    f32x4 yv[HB / 32];
    float dv[HB / 32][4];
#pragma unroll
    for (int it = 0; it < HB / 32; ++it) {
      const long long m = m0 + it * 32 + grp, pp = m - n * HW;
      yv[it] = ld4(a + (size_t)m * 32 + seg * 4);
#pragma unroll
      for (int k = 0; k < 4; ++k) dv[it][k] = k < K ? dl[((size_t)n * K + k) * HW + pp] : 0.f;
    }
#pragma unroll
    for (int it = 0; it < HB / 32; ++it) {
      const long long m = m0 + it * 32 + grp;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < K) {
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) v[jj] = fmaf(dv[it][k], wk[k][jj], v[jj]);
        }
      st4(dz + (size_t)m * 32 + seg * 4, in_bwd_dz4(v, yv[it], mu, rs, al, be, mk, slope, c1, c2));
    }
  }
}
// partial[block][K*32 + K]: dw then db
#ifndef UNET_HEAD_BWD_OCC
#define UNET_HEAD_BWD_OCC 1
#endif
template <typename TS>
__global__ __launch_bounds__(256, UNET_HEAD_BWD_OCC) void head_bwd_kernel(const TS* __restrict__ a,
                                                       const float* __restrict__ dl,
                                                       const float* __restrict__ w,
                                                       TS* __restrict__ da,
                                                       float* __restrict__ partial, long long M,
                                                       int HW, int K, long long tiles,
                                                       const float* __restrict__ alpha,
                                                       const float* __restrict__ beta,
                                                       float slope, const HeadBs bs) {
  // 8 lanes per pixel, 4 channels per lane (as head_fwd_kernel): a and da move as whole pixels
  // (1 KB per wave instruction), the K logit gradients of a pixel are broadcast loads; every
  // lane keeps its own dw[k][4 channels] partial sums over the pixels it sees, merged per block
  // through LDS in fixed order.
  __shared__ float red[32][4 * 32 + 4];
  if constexpr (sizeof(TS) == 4)
    if (bs.apply) {   // uniform
      head_bwd_apply_body(a, dl, w, da, HW, K, tiles, slope, bs);
      return;
    }
  const int tid = threadIdx.x;
  const int seg = tid & 7, grp = tid >> 3;
  f32x4 wk[4], dwacc[4];
  float dbacc[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    wk[k] = k < K ? *reinterpret_cast<const f32x4*>(w + k * 32 + seg * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    dwacc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    dbacc[k] = 0.f;
  }
  const bool one_image = HW % HB == 0;   // a tile never straddles images
  // bs.partial != nullptr (round 4; the launcher checks that a workgroup's tiles - a contiguous
  // range then - lie in ONE image): da is the final gradient of the layer that produced `a`, so
  // the two reductions of its InstanceNorm + LeakyReLU + dropout backward,
  //   S1 = sum gz,  S2 = sum gz * xhat,   gz = da * mask * (z > 0 ? 1 : slope),
  // are formed here from values the kernel already holds (same expressions as the convolution
  // epilogues, conv_params.h) - no pass over (da, y) by in_bwd_reduce_kernel.
  const bool with_bs = bs.partial != nullptr;
  f32x4 cA = {0.f, 0.f, 0.f, 0.f}, cB = cA, cM = cA, cMu = cA, cRs = cA, s1 = cA, s2 = cA;
  const long long t_first = with_bs ? (long long)blockIdx.x * bs.tiles_per_block : blockIdx.x;
  const long long t_step = with_bs ? 1 : gridDim.x;
  const long long t_last = with_bs ? min(t_first + bs.tiles_per_block, tiles) : tiles;
  if (with_bs) {
    const size_t o = (size_t)(t_first * HB / HW) * 32 + seg * 4;
    const f32x4 g = *reinterpret_cast<const f32x4*>(bs.gamma + seg * 4);
    const f32x4 b = *reinterpret_cast<const f32x4*>(bs.beta + seg * 4);
    cMu = *reinterpret_cast<const f32x4*>(bs.mean + o);
    cRs = *reinterpret_cast<const f32x4*>(bs.rstd + o);
    cA = g * cRs;
    cB = b - cMu * cA;
    cM = bs.mask ? *reinterpret_cast<const f32x4*>(bs.mask + o) : f32x4{1.f, 1.f, 1.f, 1.f};
  }
  for (long long t = t_first; t < t_last; t += t_step) {
    const long long m0 = t * HB;
    // all loads of the tile first (rows past M are clamped and masked: no branch, so the eight
    // pixel loads and 8 x K gradient loads are in flight together)
    f32x4 av[HB / 32], yv[HB / 32];
    float dv[HB / 32][4];
    f32x4 al = {1.f, 1.f, 1.f, 1.f}, be = {0.f, 0.f, 0.f, 0.f};
    if (alpha && one_image) {   // uniform: one coefficient row for the whole tile
      const size_t o = (size_t)(m0 / HW) * 32 + seg * 4;
      al = *reinterpret_cast<const f32x4*>(alpha + o);
      be = *reinterpret_cast<const f32x4*>(beta + o);
    }
#pragma unroll
    for (int it = 0; it < HB / 32; ++it) {
      const long long m = m0 + it * 32 + grp;
      const long long mc = m < M ? m : M - 1;
      av[it] = ld4(a + (size_t)mc * 32 + seg * 4);
      yv[it] = av[it];
      const long long n = one_image ? m0 / HW : mc / HW, pp = mc - n * HW;
      if (alpha) {   // uniform: the operand is a raw convolution output, activated on load
        if (!one_image) {
          al = *reinterpret_cast<const f32x4*>(alpha + (size_t)n * 32 + seg * 4);
          be = *reinterpret_cast<const f32x4*>(beta + (size_t)n * 32 + seg * 4);
        }
        av[it] = act4(av[it], al, be, slope, true);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k)
        dv[it][k] = (k < K && m < M) ? dl[((size_t)n * K + k) * HW + pp] : 0.f;
    }
#pragma unroll
    for (int it = 0; it < HB / 32; ++it) {
      const long long m = m0 + it * 32 + grp;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < K) {
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) {
            v[jj] = fmaf(dv[it][k], wk[k][jj], v[jj]);
            dwacc[k][jj] = fmaf(dv[it][k], av[it][jj], dwacc[k][jj]);
          }
          dbacc[k] += dv[it][k];
        }
      if (da && m < M) st4(da + (size_t)m * 32 + seg * 4, v);   // (no da: the fold's first launch)
      if (with_bs) {   // uniform (rows past M carry dv = 0, so v = 0 and gz = 0)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const float z = fmaf(yv[it][jj], cA[jj], cB[jj]);
          const float gz = v[jj] * cM[jj] * (z > 0.f ? 1.f : slope);   // (fp32 v, as the conv epilogues)
          s1[jj] += gz;
          s2[jj] = fmaf(gz, (yv[it][jj] - cMu[jj]) * cRs[jj], s2[jj]);
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) red[grp][k * 32 + seg * 4 + jj] = dwacc[k][jj];
    if (seg == 0) red[grp][128 + k] = dbacc[k];
  }
  __syncthreads();
  if (tid < K * 32 + K) {
    const int col = tid < K * 32 ? tid : 128 + (tid - K * 32);
    float sm = 0.f;
#pragma unroll
    for (int g = 0; g < 32; ++g) sm += red[g][col];
    partial[(size_t)blockIdx.x * (K * 32 + K) + tid] = sm;
  }
  if (with_bs) {   // uniform: the 32 pixel groups of the workgroup merged in fixed order
    __syncthreads();
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      red[grp][seg * 4 + jj] = s1[jj];
      red[grp][32 + seg * 4 + jj] = s2[jj];
    }
    __syncthreads();
    if (tid < 64) {
      float sm = 0.f;
#pragma unroll
      for (int g = 0; g < 32; ++g) sm += red[g][tid];
      // partial[(image * tiles_per_image + tile) * 32 + c] = (S1, S2): workgroup b IS tile b
      reinterpret_cast<float*>(bs.partial)[((size_t)blockIdx.x * 32 + (tid & 31)) * 2 + (tid >> 5)] = sm;
    }
  }
}

// one block per output column (K*32 weights then K biases): 256 threads stride the slabs,
// fixed-order LDS tree
__global__ __launch_bounds__(256) void head_bwd_finalize_kernel(const float* __restrict__ partial,
                                                                float* __restrict__ dw,
                                                                float* __restrict__ db,
                                                                int nblocks, int K) {
  __shared__ float red[256];
  const int i = blockIdx.x;
  const int cols = K * 32 + K;
  float s = 0.f;
  for (int b = threadIdx.x; b < nblocks; b += 256) s += partial[(size_t)b * cols + i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (i < K * 32) {
      if (dw) dw[i] = red[0];
    } else if (db) {
      db[i - K * 32] = red[0];
    }
  }
}

// ------------------------------------------------------------------ the head for 5 <= K <= 32
// One v_mfma_f32_32x32x2_f32 tile per wave and 32 pixels.  The 32 output columns of the
// instruction are the (zero-padded) classes, its reduction dimension the 32 channels - or, for
// the weight gradient, the 32 pixels.  Lane l supplies A[i = l & 31][k = l >> 5] and
// B[k = l >> 5][j = l & 31] of each of the 16 steps and holds D[(r & 3) + 8 (r >> 2) + 4 (l >> 5)]
// [l & 31] in accumulator register r.  A dot product does not care in which order its terms come,
// so the forward hands lane half h the channels 16 h .. 16 h + 15 of its pixel (step s multiplies
// channels s and 16 + s): every lane reads 64 contiguous bytes and nothing goes through LDS.
constexpr int HK_FWD_BLOCKS = 4096;

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
// class (forward, dw) or pixel (da) row that accumulator register r of lane half h holds
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// image index of pixel m: one division per tile (n0 = image of the tile's first pixel, bnd = the
// first pixel of image n0 + 1) where a tile touches at most two images
__device__ __forceinline__ long long image_of(long long m, long long n0, long long bnd, int HW) {
  if (HW >= 32) return n0 + (m >= bnd ? 1 : 0);
  return m / HW;
}
__device__ __forceinline__ float act1(float v, float al, float be, float slope) {
  const float z = v * al + be;
  return fmaxf(z, z * slope);
}

// ------------------------------------------------------------------ head forward, 5 <= K <= 32
// D[class][pixel] = W[class][:] . act(x)[pixel][:]: a lane ends up with 16 classes of ONE pixel,
// so for each accumulator register the 32 lanes of a half store 32 consecutive pixels of one
// class plane (128 contiguous bytes).
template <typename TS>
__global__ __launch_bounds__(256) void headk_fwd_kernel(const TS* __restrict__ a,
                                                        const float* __restrict__ w,
                                                        const float* __restrict__ b,
                                                        float* __restrict__ logits, long long M,
                                                        int HW, int K, long long tiles,
                                                        const float* __restrict__ alpha,
                                                        const float* __restrict__ beta,
                                                        float slope) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 31, h = lane >> 5;
  float wr[16], bias[16];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f32x4 v = col < K ? ld4(w + col * 32 + 16 * h + 4 * q) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) wr[4 * q + j] = v[j];
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int c = acc_row(r, h);
    bias[r] = (b && c < K) ? b[c] : 0.f;
  }
  for (long long t = (long long)blockIdx.x * 4 + wave; t < tiles; t += (long long)gridDim.x * 4) {
    const long long m0 = t * 32, m = m0 + col;
    const long long mc = m < M ? m : M - 1;   // rows past M: clamped load, no store
    const long long n0 = m0 / HW;
    const long long n = image_of(mc, n0, (n0 + 1) * HW, HW), pp = mc - n * HW;
    const TS* src = a + (size_t)mc * 32 + 16 * h;
    f32x4 x[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) x[q] = ld4(src + 4 * q);
    if (alpha) {   // uniform: a raw convolution output, InstanceNorm + LeakyReLU + dropout on load
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const size_t o = (size_t)n * 32 + 16 * h + 4 * q;
        x[q] = act4(x[q], ld4(alpha + o), ld4(beta + o), slope, true);
      }
    }
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int s = 0; s < 16; ++s) acc = mfma32(wr[s], x[s >> 2][s & 3], acc);
    if (m < M) {
      float* o = logits + (size_t)n * K * HW + pp;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = acc_row(r, h);
        if (c < K) o[(size_t)c * HW] = acc[r] + bias[r];
      }
    }
  }
}

// ------------------------------------------------------------------ head backward, 5 <= K <= 32
// Per wave and 32-pixel tile, the tile of dlogits goes to LDS once ([class][pixel], coalesced
// plane loads, zeros for classes >= K and pixels >= M) and is the A operand of both products:
//   da[pixel][channel] = sum_class T[class][pixel] W[class][channel]   (k = class, ceil(K/2) steps)
//   dw[class][channel] += sum_pixel T[class][pixel] act(x)[pixel][channel]   (k = pixel)
// da leaves as whole pixels (a register of a lane half = 32 channels = 128 bytes), x arrives as
// whole pixels.  dw stays in the wave's accumulator over all its tiles; db[class] is the row sum
// of T.  The four waves merge in fixed order into partial[block][K*32 + K] (dw then db), and
// headk_bwd_finalize_kernel sums the blocks in double, in block order.
template <typename TS>
__global__ __launch_bounds__(256) void headk_bwd_kernel(const TS* __restrict__ a,
                                                        const float* __restrict__ dl,
                                                        const float* __restrict__ w,
                                                        TS* __restrict__ da,
                                                        float* __restrict__ partial, long long M,
                                                        int HW, int K, long long groups,
                                                        const float* __restrict__ alpha,
                                                        const float* __restrict__ beta,
                                                        float slope) {
  __shared__ float T[4][32][33];     // (33: the transposed read of the dw product is conflict-free)
  __shared__ float red[4][33][32];   // dw[class][channel], row 32 = db[class]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 31, h = lane >> 5;
  const int ksteps = (K + 1) >> 1;
  float wb[16];
#pragma unroll
  for (int s = 0; s < 16; ++s) wb[s] = (2 * s + h < K) ? w[(2 * s + h) * 32 + col] : 0.f;
  f32x16 dwacc;
#pragma unroll
  for (int r = 0; r < 16; ++r) dwacc[r] = 0.f;
  float dbacc = 0.f;
  // every wave of a workgroup makes the same number of trips (a tile past the end is all masked)
  for (long long g = blockIdx.x; g < groups; g += gridDim.x) {
    const long long m0 = (g * 4 + wave) * 32, m = m0 + col;
    const long long mlast = M - 1;
    const long long n0 = (m0 < M ? m0 : mlast) / HW, bnd = (n0 + 1) * HW;
    // the x loads of the dw product go out first: they and the dlogits loads are in flight
    // together (one memory round trip per tile, not two)
    float xv[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const long long pm = m0 + 2 * s + h;
      xv[s] = ld1(a + (size_t)(pm < M ? pm : mlast) * 32 + col);
    }
    {
      const long long mc = m < M ? m : mlast;
      const long long n = image_of(mc, n0, bnd, HW), pp = mc - n * HW;
      const float* src = dl + (size_t)n * K * HW + pp;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int c = 2 * i + h;
        T[wave][c][col] = (c < K && m < M) ? src[(size_t)c * HW] : 0.f;
      }
    }
    __syncthreads();
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int s = 0; s < 16; ++s)
      if (s < ksteps) acc = mfma32(T[wave][2 * s + h][col], wb[s], acc);   // uniform
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long long pm = m0 + acc_row(r, h);
      if (pm < M) st1(da + (size_t)pm * 32 + col, acc[r]);
    }
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const long long pm = m0 + 2 * s + h;
      const long long pc = pm < M ? pm : mlast;
      float x = xv[s];
      if (alpha) {   // uniform
        const size_t o = (size_t)image_of(pc, n0, bnd, HW) * 32 + col;
        x = act1(x, alpha[o], beta[o], slope);
      }
      dwacc = mfma32(T[wave][col][2 * s + h], x, dwacc);
    }
    float sdb = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) sdb += T[wave][col][16 * h + j];
    dbacc += sdb;
    __syncthreads();   // (the next trip overwrites T)
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) red[wave][acc_row(r, h)][col] = dwacc[r];
  const float other = __shfl_xor(dbacc, 32, 64);
  if (h == 0) red[wave][32][col] = dbacc + other;   // pixels 0..15 + pixels 16..31 of every tile
  __syncthreads();
  const int cols = K * 32 + K;
  for (int i = threadIdx.x; i < cols; i += 256) {
    const int row = i < K * 32 ? i >> 5 : 32, c = i < K * 32 ? i & 31 : i - K * 32;
    partial[(size_t)blockIdx.x * cols + i] =
        (red[0][row][c] + red[1][row][c]) + (red[2][row][c] + red[3][row][c]);
  }
}

// one workgroup per output value (K*32 weights then K biases): 256 threads stride the blocks'
// slabs in double, fixed-order LDS tree
__global__ __launch_bounds__(256) void headk_bwd_finalize_kernel(const float* __restrict__ partial,
                                                                 float* __restrict__ dw,
                                                                 float* __restrict__ db,
                                                                 int nblocks, int K) {
  __shared__ double red[256];
  const int i = blockIdx.x;
  const int cols = K * 32 + K;
  double s = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += 256) s += (double)partial[(size_t)b * cols + i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (i < K * 32) {
      if (dw) dw[i] = (float)red[0];
    } else if (db) {
      db[i - K * 32] = (float)red[0];
    }
  }
}

#ifndef UNET_HEAD_BWD_BLOCKS
#define UNET_HEAD_BWD_BLOCKS 1024
#endif
int head_bwd_blocks(long long tiles) { return (int)(tiles < UNET_HEAD_BWD_BLOCKS ? tiles : UNET_HEAD_BWD_BLOCKS); }

}  // namespace

// ---- the matrix-core head: the unet_head1x1_* entry points below check the operands and come
// here for K > 4.  M = N * HW pixels; alpha / beta (nullable) activate `a` on load.
static int unet_headk_fwd(const void* a, int a_is_bf16, const float* w, const float* b, float* logits,
                   long long M, int HW, int K, const float* alpha, const float* beta, float slope,
                   hipStream_t stream) {
  const long long tiles = ceil_div64(M, 32);
  const long long want = ceil_div64(tiles, 4);
  const dim3 grid((unsigned)(want < HK_FWD_BLOCKS ? want : HK_FWD_BLOCKS));
  if (a_is_bf16)
    hipLaunchKernelGGL(headk_fwd_kernel<__bf16>, grid, dim3(256), 0, stream,
                       reinterpret_cast<const __bf16*>(a), w, b, logits, M, HW, K, tiles, alpha,
                       beta, slope);
  else
    hipLaunchKernelGGL(headk_fwd_kernel<float>, grid, dim3(256), 0, stream,
                       reinterpret_cast<const float*>(a), w, b, logits, M, HW, K, tiles, alpha,
                       beta, slope);
  UNET_CHECK_LAUNCH("headk_fwd");
  return UNET_OK;
}

// partial: max_blocks slabs of K*32 + K floats (unet_head1x1_bwd_workspace_bytes)
static int unet_headk_bwd(const void* a, int b16, const float* dl, const float* w, void* da, float* dw,
                   float* db, float* partial, int max_blocks, long long M, int HW, int K,
                   const float* alpha, const float* beta, float slope, hipStream_t stream) {
  const long long groups = ceil_div64(ceil_div64(M, 32), 4);
  const int blocks = (int)(groups < max_blocks ? groups : max_blocks);
  if (b16)
    hipLaunchKernelGGL(headk_bwd_kernel<__bf16>, dim3(blocks), dim3(256), 0, stream,
                       reinterpret_cast<const __bf16*>(a), dl, w, reinterpret_cast<__bf16*>(da),
                       partial, M, HW, K, groups, alpha, beta, slope);
  else
    hipLaunchKernelGGL(headk_bwd_kernel<float>, dim3(blocks), dim3(256), 0, stream,
                       reinterpret_cast<const float*>(a), dl, w, reinterpret_cast<float*>(da),
                       partial, M, HW, K, groups, alpha, beta, slope);
  UNET_CHECK_LAUNCH("headk_bwd");
  if (dw || db) {
    hipLaunchKernelGGL(headk_bwd_finalize_kernel, dim3(K * 32 + K), dim3(256), 0, stream,
                       (const float*)partial, dw, db, blocks, K);
    UNET_CHECK_LAUNCH("headk_bwd_finalize");
  }
  return UNET_OK;
}

extern "C" int unet_head1x1_fwd(const float* a, const float* w, const float* b, float* logits,
                                int N, int HW, int C, int K, unet_stream_t stream) {
  UNET_REQUIRE(a && w && logits, "head1x1_fwd: null pointer");
  UNET_REQUIRE(C == 32 && K >= 1 && K <= UNET_MAX_CLASSES && N > 0 && HW > 0,
               "head1x1_fwd: needs C == 32, K <= 32 (got C=%d K=%d)", C, K);
  const long long M = (long long)N * HW;
  if (K > 4)   // the matrix-core head
    return unet_headk_fwd(a, 0, w, b, logits, M, HW, K, nullptr, nullptr, 0.f, (hipStream_t)stream);
  hipLaunchKernelGGL(head_fwd_kernel<float>, dim3((unsigned)ceil_div64(M, HT)), dim3(256), 0,
                     (hipStream_t)stream, a, w, b, logits, M, HW, K, (const float*)nullptr,
                     (const float*)nullptr, 0.f);
  UNET_CHECK_LAUNCH("head_fwd");
  return UNET_OK;
}

extern "C" int unet_head1x1_in_fwd(const unet_act_src* x, float slope, const float* w,
                                   const float* b, float* logits, int N, int HW, int K,
                                   unet_stream_t stream) {
  UNET_REQUIRE(x && x->x && w && logits, "head1x1_in_fwd: null pointer");
  UNET_REQUIRE(x->C == 32 && K >= 1 && K <= UNET_MAX_CLASSES && N > 0 && HW > 0 &&
                   (!x->alpha || x->beta),
               "head1x1_in_fwd: needs C == 32, K <= 32 (got C=%d K=%d)", x->C, K);
  const long long M = (long long)N * HW;
  if (K > 4)
    return unet_headk_fwd(x->x, 0, w, b, logits, M, HW, K, x->alpha, x->beta, slope,
                          (hipStream_t)stream);
  hipLaunchKernelGGL(head_fwd_kernel<float>, dim3((unsigned)ceil_div64(M, HT)), dim3(256), 0,
                     (hipStream_t)stream, x->x, w, b, logits, M, HW, K, x->alpha, x->beta, slope);
  UNET_CHECK_LAUNCH("head_fwd");
  return UNET_OK;
}

extern "C" int unet_head1x1_in_fwd_b16(const unet_act_src* x, float slope, const float* w,
                                       const float* b, float* logits, int N, int HW, int K,
                                       unet_stream_t stream) {
  UNET_REQUIRE(x && x->x && w && logits, "head1x1_in_fwd_b16: null pointer");
  UNET_REQUIRE(x->C == 32 && K >= 1 && K <= UNET_MAX_CLASSES && N > 0 && HW > 0 &&
                   (!x->alpha || x->beta),
               "head1x1_in_fwd_b16: needs C == 32, K <= 32 (got C=%d K=%d)", x->C, K);
  const long long M = (long long)N * HW;
  if (K > 4)
    return unet_headk_fwd(x->x, 1, w, b, logits, M, HW, K, x->alpha, x->beta, slope,
                          (hipStream_t)stream);
  hipLaunchKernelGGL(head_fwd_kernel<__bf16>, dim3((unsigned)ceil_div64(M, HT)), dim3(256), 0,
                     (hipStream_t)stream, reinterpret_cast<const __bf16*>(x->x), w, b, logits, M,
                     HW, K, x->alpha, x->beta, slope);
  UNET_CHECK_LAUNCH("head_fwd(b16)");
  return UNET_OK;
}

// Reductions of the InstanceNorm backward of the layer in front (bs): a workgroup then takes a
// contiguous range of tiles, which must lie in one image and divide it evenly - one summary
// "tile" of tiles_per_block * HB pixels per workgroup.  -> summaries per image, with *hb filled
// in; 0 (*hb untouched): this shape or these operands have no such form.
static int head_bs_plan(const float* a, const float* alpha, long long M, int HW,
                        const unet_bwd_stats* bs, HeadBs* hb) {
  if (!(alpha && bs->y == a && bs->mean && bs->rstd && bs->gamma && bs->beta && bs->partial &&
        M % HB == 0))
    return 0;
  const long long tiles = M / HB;
  const int blocks = head_bwd_blocks(tiles);
  const long long tpb = ceil_div64(tiles, blocks);
  const long long px = tpb * HB;
  if (!(tiles % tpb == 0 && tiles / tpb == blocks && HW % px == 0 &&
        bs->partial_bytes >= (size_t)blocks * 32 * sizeof(float2)))
    return 0;
  hb->mean = bs->mean; hb->rstd = bs->rstd; hb->gamma = bs->gamma; hb->beta = bs->beta;
  hb->mask = bs->mask; hb->partial = reinterpret_cast<float2*>(bs->partial);
  hb->tiles_per_block = (int)tpb;
  return (int)(HW / px);
}

extern "C" size_t unet_head1x1_bwd_workspace_bytes(int N, int HW, int C, int K) {
  if (N <= 0 || HW <= 0) return 0;
  const long long tiles = ceil_div64((long long)N * HW, HB);
  return (size_t)head_bwd_blocks(tiles) * (K * 32 + K) * sizeof(float);
}

// operands of unet_head1x1_in_bwd_fold beyond those of unet_head1x1_in_bwd_bs
struct HeadFold { float2* coef; float2* sums; float* dgamma; float* dbeta; float* dbias; };
static int head1x1_bwd_impl(const float* a, const float* dlogits, const float* w, float* da,
                            float* dw, float* db, void* workspace, size_t workspace_bytes, int N,
                            int HW, int C, int K, const float* alpha, const float* beta,
                            float slope, unet_stream_t stream, int b16 = 0,
                            unet_bwd_stats* bs = nullptr, const HeadFold* fold = nullptr) {
  UNET_REQUIRE(a && dlogits && w && da && workspace, "head1x1_bwd: null pointer");
  UNET_REQUIRE(C == 32 && K >= 1 && K <= UNET_MAX_CLASSES && N > 0 && HW > 0,
               "head1x1_bwd: needs C == 32, K <= 32 (got C=%d K=%d)", C, K);
  UNET_REQUIRE_WS(workspace_bytes, unet_head1x1_bwd_workspace_bytes(N, HW, C, K),
                  "head1x1_bwd: workspace too small");
  const long long M = (long long)N * HW;
  const long long tiles = ceil_div64(M, HB);
  const int blocks = head_bwd_blocks(tiles);
  float* partial = reinterpret_cast<float*>(workspace);
  if (K > 4) {
    // the matrix-core head: plain da, no InstanceNorm-backward reductions
    // (tiles_out == 0: the caller runs unet_instnorm_lrelu_drop_bwd, as for a shape that does
    // not split evenly)
    if (bs) bs->tiles_out = 0;
    return unet_headk_bwd(a, b16, dlogits, w, da, dw, db, partial, blocks, M, HW, K, alpha, beta,
                          slope, (hipStream_t)stream);
  }
  HeadBs hb{};
  if (bs) {
    bs->tiles_out = head_bs_plan(a, alpha, M, HW, bs, &hb);
    UNET_REQUIRE(bs->tiles_out == 0 || bs->slope == slope,
                 "head1x1_in_bwd_bs: bs->slope differs from slope");
  }
  // the fold: da is never stored - this launch leaves the reductions and the dw / db slabs only
  const bool folded = fold && bs && bs->tiles_out > 0 && !b16;
  float* da0 = folded ? nullptr : da;
  if (b16)
    hipLaunchKernelGGL(head_bwd_kernel<__bf16>, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const __bf16*>(a), dlogits, w,
                       reinterpret_cast<__bf16*>(da), partial, M, HW, K, tiles, alpha, beta, slope,
                       hb);
  else
    hipLaunchKernelGGL(head_bwd_kernel<float>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a,
                       dlogits, w, da0, partial, M, HW, K, tiles, alpha, beta, slope, hb);
  UNET_CHECK_LAUNCH("head_bwd");
  if (dw || db) {     // (neither: data gradient only - Grad-CAM)
    hipLaunchKernelGGL(head_bwd_finalize_kernel, dim3(K * 32 + K), dim3(256), 0,
                       (hipStream_t)stream, partial, dw, db, blocks, K);
    UNET_CHECK_LAUNCH("head_bwd_finalize");
  }
  if (!folded) return UNET_OK;
  // ... then the summaries are merged and a second launch forms da again, per lane, on the way
  // to dz (written where da would have gone)
  const int rc = unet_instnorm_bwd_merge_partials(bs->partial, bs->tiles_out, fold->coef,
                                                  fold->sums, N, HW, 32, stream);
  if (rc != UNET_OK) return rc;
  hb.apply = 1;
  hb.coef = fold->coef; hb.sums = fold->sums;
  hb.dgamma = fold->dgamma; hb.dbeta = fold->dbeta; hb.dbias = fold->dbias;
  hb.N = N;
  hipLaunchKernelGGL(head_bwd_kernel<float>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a,
                     dlogits, w, da, partial, M, HW, K, tiles, alpha, beta, slope, hb);
  UNET_CHECK_LAUNCH("head_bwd(apply)");
  return UNET_OK;
}

extern "C" int unet_head1x1_bwd(const float* a, const float* dlogits, const float* w, float* da,
                                float* dw, float* db, void* workspace, size_t workspace_bytes,
                                int N, int HW, int C, int K, unet_stream_t stream) {
  return head1x1_bwd_impl(a, dlogits, w, da, dw, db, workspace, workspace_bytes, N, HW, C, K,
                          nullptr, nullptr, 0.f, stream);
}

extern "C" int unet_head1x1_in_bwd(const unet_act_src* x, float slope, const float* dlogits,
                                   const float* w, float* da, float* dw, float* db,
                                   void* workspace, size_t workspace_bytes, int N, int HW, int K,
                                   unet_stream_t stream) {
  UNET_REQUIRE(x && x->x && (!x->alpha || x->beta), "head1x1_in_bwd: null source");
  return head1x1_bwd_impl(x->x, dlogits, w, da, dw, db, workspace, workspace_bytes, N, HW, x->C, K,
                          x->alpha, x->beta, slope, stream);
}

// ... with the reductions of the InstanceNorm + LeakyReLU + dropout backward of the layer whose
// raw output x->x is (bs->y == x->x): da is that layer's final dL/da, so the kernel that writes
// it also sums gz and gz * xhat per workgroup (bs->tiles_out summaries per image; 0 = the shape
// does not split evenly: run unet_instnorm_lrelu_drop_bwd as usual)
extern "C" int unet_head1x1_in_bwd_bs(const unet_act_src* x, float slope, const float* dlogits,
                                      const float* w, float* da, float* dw, float* db,
                                      void* workspace, size_t workspace_bytes, int N, int HW,
                                      int K, unet_bwd_stats* bs, unet_stream_t stream) {
  UNET_REQUIRE(x && x->x && (!x->alpha || x->beta), "head1x1_in_bwd_bs: null source");
  return head1x1_bwd_impl(x->x, dlogits, w, da, dw, db, workspace, workspace_bytes, N, HW, x->C, K,
                          x->alpha, x->beta, slope, stream, 0, bs);
}

extern "C" int unet_head1x1_in_bwd_bs_b16(const unet_act_src* x, float slope, const float* dlogits,
                                          const float* w, uint16_t* da, float* dw, float* db,
                                          void* workspace, size_t workspace_bytes, int N, int HW,
                                          int K, unet_bwd_stats* bs, unet_stream_t stream) {
  UNET_REQUIRE(x && x->x && (!x->alpha || x->beta), "head1x1_in_bwd_bs_b16: null source");
  return head1x1_bwd_impl(x->x, dlogits, w, reinterpret_cast<float*>(da), dw, db, workspace,
                          workspace_bytes, N, HW, x->C, K, x->alpha, x->beta, slope, stream, 1, bs);
}

// x and da are bf16 tensors (mixed-precision pipeline); logits gradient and dw / db stay fp32
extern "C" int unet_head1x1_in_bwd_b16(const unet_act_src* x, float slope, const float* dlogits,
                                       const float* w, uint16_t* da, float* dw, float* db,
                                       void* workspace, size_t workspace_bytes, int N, int HW,
                                       int K, unet_stream_t stream) {
  UNET_REQUIRE(x && x->x && (!x->alpha || x->beta), "head1x1_in_bwd_b16: null source");
  return head1x1_bwd_impl(x->x, dlogits, w, reinterpret_cast<float*>(da), dw, db, workspace,
                          workspace_bytes, N, HW, x->C, K, x->alpha, x->beta, slope, stream, 1);
}

// The head's backward and the InstanceNorm + LeakyReLU + dropout backward of the layer in front
// as one call (fp32 tensors): where unet_head1x1_in_bwd_bs would leave that layer's reductions
// (bs->tiles_out > 0 on return), da never reaches memory - `dz` receives the layer's dL/dz and
// dgamma / dbeta / dbias (each nullable) its parameter gradients.  bs->tiles_out == 0: the call
// did what unet_head1x1_in_bwd_bs does, `dz` holds da and unet_instnorm_lrelu_drop_bwd is the
// caller's next step.  Workspace: the slabs of unet_head1x1_bwd, then the (coef, sums) pair.
struct HeadFoldWs { InBwdPair pair; size_t bytes; };
static HeadFoldWs head_fold_ws(void* base, int N, int HW, int K) {
  WsLayout l(base);
  l.take<char>(unet_head1x1_bwd_workspace_bytes(N, HW, 32, K), 256);   // at the base: the callee's
  return {in_bwd_pair(l, N, 32), l.bytes()};
}

extern "C" size_t unet_head1x1_in_bwd_fold_workspace_bytes(int N, int HW, int K) {
  if (N <= 0 || HW <= 0) return 0;
  return head_fold_ws(nullptr, N, HW, K).bytes;
}

extern "C" int unet_head1x1_in_bwd_fold(const unet_act_src* x, float slope, const float* dlogits,
                                        const float* w, float* dz, float* dw, float* db,
                                        float* dgamma, float* dbeta, float* dbias,
                                        void* workspace, size_t workspace_bytes, int N, int HW,
                                        int K, unet_bwd_stats* bs, unet_stream_t stream) {
  UNET_REQUIRE(x && x->x && (!x->alpha || x->beta) && bs && workspace,
               "head1x1_in_bwd_fold: null pointer");
  UNET_REQUIRE(N > 0 && HW > 0 && K >= 1 && K <= UNET_MAX_CLASSES,
               "head1x1_in_bwd_fold: bad shape");
  const HeadFoldWs ws = head_fold_ws(workspace, N, HW, K);
  UNET_REQUIRE_WS(workspace_bytes, ws.bytes, "head1x1_in_bwd_fold: workspace too small");
  const HeadFold fold{ws.pair.coef, ws.pair.sums, dgamma, dbeta, dbias};
  return head1x1_bwd_impl(x->x, dlogits, w, dz, dw, db, workspace, workspace_bytes, N, HW, x->C, K,
                          x->alpha, x->beta, slope, stream, 0, bs, &fold);
}
