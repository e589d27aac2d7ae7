// head_loss_k.hip — the tail of the network for a class count K other than the pet trimap's 3:
//
//   unet_headk_fwd / unet_headk_bwd   the 1x1 head for 5 <= K <= 32 on the fp32 matrix cores
//                                     (reached through the unet_head1x1_* entry points, K > 4)
//   unet_dice_wce_lossk_*             SimpleLoss for 2 <= K <= 32: reduce, finalize, gradient
//   unet_argmax_countsk[_u8]          argmax and the integers behind validate()'s Dice scores
//
// The definitions are the reference's with 3 replaced by K (Our_UNet/models/losses.py:24-121,
// Our_UNet/src/train.py:556-577).  Nothing here is launched by a 3-class step: K == 3 (loss,
// counts) and K <= 4 (head) keep the kernels of head_loss.hip.
//
// Head: one v_mfma_f32_32x32x2_f32 tile per wave and 32 pixels.  The 32 output columns of the
// instruction are the (zero-padded) classes, its reduction dimension the 32 channels - or, for
// the weight gradient, the 32 pixels.  Lane l supplies A[i = l & 31][k = l >> 5] and
// B[k = l >> 5][j = l & 31] of each of the 16 steps and holds D[(r & 3) + 8 (r >> 2) + 4 (l >> 5)]
// [l & 31] in accumulator register r.  A dot product does not care in which order its terms come,
// so the forward hands lane half h the channels 16 h .. 16 h + 15 of its pixel (step s multiplies
// channels s and 16 + s): every lane reads 64 contiguous bytes and nothing goes through LDS.
#include "common.h"
#include "conv_params.h"

namespace {
using unet_conv::act4;

constexpr int KMAX = 32;          // UNET_MAX_CLASSES
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

// ------------------------------------------------------------------ K-class SimpleLoss
// Per image 4K + 1 sums: cnt[K], nll[K], I[K], P[K], valid.  KP = K padded to 4, 8, 16 or 32 is
// the template parameter: the class loops unroll, every per-class value lives in a register of
// its own and the class of a pixel's own label selects with compares (never an index).
constexpr int LOSSK_BLOCKS = 128;   // per image
constexpr int LOSSK_MAX_N = 1024;   // images per call (unet_hip.h)

struct LossCoefK {   // written by finalize, read by the gradient kernel
  float w[KMAX];
  float inv_wsum;    // w_ce * grad_scale / sum_i w[t_i]
  float wdice;
};

// Label of a pixel as a small int: its class 0..K-1, -1 = ignore_index, -2 = no class (an int64
// label outside 0..K-1; the uint8 rule v >= K && v != ignore_index -> 0 leaves none).  Behind the
// empty asm the two target types are the same code for the optimiser - equal bits are the
// contract of the `_u8` twins.
__device__ __forceinline__ int labelk(const long long* tg, int K, int ignore_index) {
  const long long t = tg[0];
  int ti = t == (long long)ignore_index ? -1 : (t >= 0 && t < K) ? (int)t : -2;
  asm("" : "+v"(ti));
  return ti;
}
__device__ __forceinline__ int labelk(const unsigned char* tg, int K, int ignore_index) {
  const int v = tg[0];
  int ti = v == ignore_index ? -1 : v >= K ? 0 : v;
  asm("" : "+v"(ti));
  return ti;
}

// softmax over the K planes of pixel p (classes >= K: -inf, probability 0), the order of
// softmax3: max, exp, sum in class order, one reciprocal
template <int KP>
__device__ __forceinline__ void softmaxk(const float* __restrict__ z, int HW, int p, int K,
                                         float (&zz)[KP], float (&pr)[KP], float& lse) {
#pragma clang fp contract(off)
#pragma unroll
  for (int c = 0; c < KP; ++c) zz[c] = c < K ? z[(size_t)c * HW + p] : -INFINITY;
  float m = zz[0];
#pragma unroll
  for (int c = 1; c < KP; ++c) m = fmaxf(m, zz[c]);
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < KP; ++c) {
    pr[c] = expf(zz[c] - m);
    s += pr[c];
  }
  const float inv = 1.f / s;
#pragma unroll
  for (int c = 0; c < KP; ++c) pr[c] *= inv;
  lse = m + logf(s);
}

template <int KP, typename TT>
__global__ __launch_bounds__(256) void lossk_reduce_kernel(const float* __restrict__ logits,
                                                           const TT* __restrict__ target,
                                                           float* __restrict__ partial, int HW,
                                                           int K, int ignore_index) {
#pragma clang fp contract(off)
  __shared__ float red[4][4 * KP + 1];
  const int n = blockIdx.y;
  const float* z = logits + (size_t)n * K * HW;
  const TT* tg = target + (size_t)n * HW;
  float cnt[KP], nll[KP], qi[KP], qp[KP], nvalid = 0.f;
#pragma unroll
  for (int c = 0; c < KP; ++c) cnt[c] = nll[c] = qi[c] = qp[c] = 0.f;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
    const int t = labelk(tg + p, K, ignore_index);
    if (t == -1) continue;
    float zz[KP], pr[KP], lse;
    softmaxk<KP>(z, HW, p, K, zz, pr, lse);
    nvalid += 1.f;
#pragma unroll
    for (int c = 0; c < KP; ++c) {
      const bool own = t == c;
      qp[c] += pr[c];
      cnt[c] += own ? 1.f : 0.f;
      nll[c] += own ? lse - zz[c] : 0.f;
      qi[c] += own ? pr[c] : 0.f;
    }
  }
  // lanes -> wave (xor tree) -> the workgroup's slab (waves in order); finalize sums the slabs
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < KP; ++c) {
    const float s0 = wave_sum(cnt[c]), s1 = wave_sum(nll[c]), s2 = wave_sum(qi[c]),
                s3 = wave_sum(qp[c]);
    if (lane == 0) {
      red[wave][c] = s0; red[wave][KP + c] = s1; red[wave][2 * KP + c] = s2;
      red[wave][3 * KP + c] = s3;
    }
  }
  const float sv = wave_sum(nvalid);
  if (lane == 0) red[wave][4 * KP] = sv;
  __syncthreads();
  const int LQ = 4 * K + 1;
  if ((int)threadIdx.x < LQ) {
    const int i = threadIdx.x;
    const int q = i == 4 * K ? 4 * KP : (i / K) * KP + i % K;
    partial[((size_t)n * gridDim.x + blockIdx.x) * LQ + i] =
        (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
  }
}

// One workgroup of 1024 threads.  Column sums over the slabs, in slab order, in double, into `sums` (global: the
// batch's N (4K + 1) doubles need not fit LDS); then thread c < K reduces class c over the images
// in image order and writes its Dice gradient coefficients; then thread 0 combines the K classes.
__global__ __launch_bounds__(1024) void lossk_finalize_kernel(
    const float* __restrict__ partial, double* __restrict__ sums, int N, int K, int nblocks,
    float smooth, float w_dice, float w_ce, int dynamic_weights,
    const float* __restrict__ class_weights, float grad_scale, float* __restrict__ loss_out,
    LossCoefK* __restrict__ coef, float* __restrict__ dice_ab) {
  __shared__ double s_cnt[KMAX], s_nll[KMAX], s_dice[KMAX], s_total;
  const int LQ = 4 * K + 1;
  for (int i = threadIdx.x; i < N * LQ; i += blockDim.x) {
    const int n = i / LQ, k = i - n * LQ;
    const float* col = partial + (size_t)n * nblocks * LQ + k;
    // 16 loads in flight, then their adds: the order - and so the value - of the plain loop
    double s = 0.0;
    int b = 0;
    for (; b + 16 <= nblocks; b += 16) {
      float v[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = col[(size_t)(b + j) * LQ];
#pragma unroll
      for (int j = 0; j < 16; ++j) s += (double)v[j];
    }
    for (; b < nblocks; ++b) s += (double)col[(size_t)b * LQ];
    sums[i] = s;
  }
  __syncthreads();   // global writes of this workgroup are visible to it after the barrier
  const int c = threadIdx.x;
  if (c < K) {
    double cnt = 0, nll = 0, dmean = 0;
    const double k = 1.0 / ((double)K * N);
    for (int n = 0; n < N; ++n) {
      const double* q = sums + (size_t)n * LQ;
      const double T = q[c], I = q[2 * K + c], P = q[3 * K + c], U = P + T;
      cnt += T;
      nll += q[K + c];
      dmean += (2.0 * I + smooth) / (U + smooth);
      // d(dice loss)/dp_c at pixel i of image n = A [t_i == c] + B (valid pixels)
      dice_ab[((size_t)n * K + c) * 2 + 0] = (float)(-2.0 * k / (U + smooth));
      dice_ab[((size_t)n * K + c) * 2 + 1] =
          (float)((2.0 * I + smooth) * k / ((U + smooth) * (U + smooth)));
    }
    s_cnt[c] = cnt; s_nll[c] = nll; s_dice[c] = 1.0 - dmean / N;
  } else if (c == 64) {
    double total = 0;
    for (int n = 0; n < N; ++n) total += sums[(size_t)n * LQ + 4 * K];
    s_total = total;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  float w[KMAX];
  if (dynamic_weights) {
    // Our_UNet/models/losses.py:44-60 with K for 3: count 0 -> 1, total/count, sum made K
    float ws = 0.f;
    for (int i = 0; i < K; ++i) {
      const float cp = s_cnt[i] == 0 ? 1.f : (float)s_cnt[i];
      w[i] = (float)s_total / cp;
      ws += w[i];
    }
    for (int i = 0; i < K; ++i) w[i] = w[i] * ((float)K / ws);
  } else {
    for (int i = 0; i < K; ++i) w[i] = class_weights ? class_weights[i] : 1.f;
  }
  double num = 0, den = 0, dice_sum = 0;
  for (int i = 0; i < K; ++i) {
    num += (double)w[i] * s_nll[i];
    den += (double)w[i] * s_cnt[i];
    dice_sum += s_dice[i];
  }
  const float ce = (float)(num / den);
  const float dice = (float)(dice_sum / K);
  loss_out[0] = w_ce * ce + w_dice * dice;
  loss_out[1] = ce;
  loss_out[2] = dice;
  for (int i = 0; i < KMAX; ++i) {
    if (i < K) loss_out[3 + i] = w[i];
    coef->w[i] = i < K ? w[i] : 0.f;
  }
  coef->inv_wsum = (float)((double)w_ce * grad_scale / den);
  coef->wdice = w_dice * grad_scale;
}

template <int KP, typename TT>
__global__ __launch_bounds__(256) void lossk_grad_kernel(const float* __restrict__ logits,
                                                         const TT* __restrict__ target,
                                                         const LossCoefK* __restrict__ coef,
                                                         const float* __restrict__ dice_ab,
                                                         float* __restrict__ dlogits, int HW,
                                                         int K, int ignore_index,
                                                         const float* __restrict__ upstream) {
#pragma clang fp contract(off)
  const int n = blockIdx.y;
  const float* z = logits + (size_t)n * K * HW;
  float* dz = dlogits + (size_t)n * K * HW;
  const TT* tg = target + (size_t)n * HW;
  // dL/d(loss) from autograd (a device scalar; NULL = 1), applied to the finished gradient
  const float up = upstream ? upstream[0] : 1.f;
  const float iw = coef->inv_wsum, wd = coef->wdice;
  float wc[KP], A[KP], B[KP];
#pragma unroll
  for (int c = 0; c < KP; ++c) {
    wc[c] = coef->w[c];    // (zeros past K)
    A[c] = c < K ? dice_ab[((size_t)n * K + c) * 2 + 0] : 0.f;
    B[c] = c < K ? dice_ab[((size_t)n * K + c) * 2 + 1] : 0.f;
  }
  for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
    const int t = labelk(tg + p, K, ignore_index);
    float g[KP];
    if (t == -1) {
#pragma unroll
      for (int c = 0; c < KP; ++c) g[c] = 0.f;
    } else {
      float zz[KP], pr[KP], lse;
      softmaxk<KP>(z, HW, p, K, zz, pr, lse);
      float wt = 0.f, dot = 0.f;
#pragma unroll
      for (int c = 0; c < KP; ++c) {
        const bool own = t == c;
        wt = own ? wc[c] : wt;
        zz[c] = B[c] + (own ? A[c] : 0.f);     // a_c (the logits are not needed again)
        dot += zz[c] * pr[c];
      }
      const float k = wt * iw;
#pragma unroll
      for (int c = 0; c < KP; ++c) {
        // weighted CE, w_t (p - onehot) / sum w, and Dice through the softmax Jacobian,
        // p_c (a_c - sum_j a_j p_j)
        const float ce = k * (pr[c] - (t == c ? 1.f : 0.f));
        g[c] = ce + wd * pr[c] * (zz[c] - dot);
      }
    }
#pragma unroll
    for (int c = 0; c < KP; ++c)
      if (c < K) dz[(size_t)c * HW + p] = g[c] * up;
  }
}

// ------------------------------------------------------------------ argmax / counts
// preds = argmax over the K planes (first maximum wins, like torch.argmax); counts[c] =
// {intersection, predicted, labelled} as exact integers, ignore_index pixels excluded.
template <int KP, typename TT>
__global__ __launch_bounds__(256) void argmax_countsk_kernel(const float* __restrict__ logits,
                                                             const TT* __restrict__ target,
                                                             unsigned char* __restrict__ preds,
                                                             unsigned long long* __restrict__ counts,
                                                             int HW, int K, int ignore_index) {
  __shared__ unsigned int red[4][3 * KP];
  const int n = blockIdx.y;
  const float* z = logits + (size_t)n * K * HW;
  const TT* tg = target + (size_t)n * HW;
  unsigned int qi[KP], qp[KP], ql[KP];
#pragma unroll
  for (int c = 0; c < KP; ++c) qi[c] = qp[c] = ql[c] = 0;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
    int am = 0;
    float best = z[p];
#pragma unroll
    for (int c = 1; c < KP; ++c)
      if (c < K) {
        const float v = z[(size_t)c * HW + p];
        if (v > best) { best = v; am = c; }
      }
    if (preds) preds[(size_t)n * HW + p] = (unsigned char)am;
    if (!target) continue;           // prediction only (inference)
    const int t = labelk(tg + p, K, ignore_index);
    if (t == -1) continue;
#pragma unroll
    for (int c = 0; c < KP; ++c) {
      const unsigned int pc = am == c, mc = t == c;
      qi[c] += pc & mc;
      qp[c] += pc;
      ql[c] += mc;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < KP; ++c) {
    unsigned int v0 = qi[c], v1 = qp[c], v2 = ql[c];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      v0 += __shfl_xor(v0, off, 64);
      v1 += __shfl_xor(v1, off, 64);
      v2 += __shfl_xor(v2, off, 64);
    }
    if (lane == 0) { red[wave][c * 3] = v0; red[wave][c * 3 + 1] = v1; red[wave][c * 3 + 2] = v2; }
  }
  __syncthreads();
  if (target && (int)threadIdx.x < 3 * K) {
    const int i = threadIdx.x;
    const unsigned int s = red[0][i] + red[1][i] + red[2][i] + red[3][i];
    if (s) atomicAdd(&counts[i], (unsigned long long)s);   // integer: order-independent
  }
}

struct LossWsK {
  float* partial; LossCoefK* coef; float* dice_ab; double* sums;
};
size_t lossk_ws_layout(int N, int K, LossWsK* out, char* base) {
  const size_t LQ = 4 * (size_t)K + 1;
  const size_t partial_b = align_up((size_t)N * LOSSK_BLOCKS * LQ * sizeof(float), 256);
  const size_t coef_b = align_up(sizeof(LossCoefK), 256);
  const size_t ab_b = align_up((size_t)N * K * 2 * sizeof(float), 256);
  if (out) {
    out->partial = reinterpret_cast<float*>(base);
    out->coef = reinterpret_cast<LossCoefK*>(base + partial_b);
    out->dice_ab = reinterpret_cast<float*>(base + partial_b + coef_b);
    out->sums = reinterpret_cast<double*>(base + partial_b + coef_b + ab_b);
  }
  return partial_b + coef_b + ab_b + align_up((size_t)N * LQ * sizeof(double), 256);
}

int lossk_blocks_for(int HW) {
  int blocks = ceil_div(HW, 256 * 8);
  if (blocks > LOSSK_BLOCKS) blocks = LOSSK_BLOCKS;
  return blocks < 1 ? 1 : blocks;
}

// the checks every K-class entry point makes before a launch
template <typename TT>
int checkk(const char* name, int N, int K, int H, int W, int ignore_index,
           int max_n = LOSSK_MAX_N) {
  UNET_REQUIRE(K >= 2 && K <= KMAX, "%s: needs 2 <= K <= %d classes (got %d)", name, KMAX, K);
  UNET_REQUIRE(N > 0 && N <= max_n && H > 0 && W > 0 && (long long)H * W * K <= 0x7fffffffll,
               "%s: bad shape (1 <= N <= %d images, K * H * W < 2^31)", name, max_n);
  if constexpr (sizeof(TT) == 1)
    UNET_REQUIRE(ignore_index >= K && ignore_index <= 255,
                 "%s: a uint8 target needs ignore_index in K..255 (got %d, K = %d)", name,
                 ignore_index, K);
  return UNET_OK;
}

// KERNEL<KP, TT> for the padded class count of K
#define UNET_KP_DISPATCH(KERNEL, TT, grid, stream, ...)                                          \
  do {                                                                                           \
    if (K <= 4) hipLaunchKernelGGL((KERNEL<4, TT>), grid, dim3(256), 0, stream, __VA_ARGS__);      \
    else if (K <= 8) hipLaunchKernelGGL((KERNEL<8, TT>), grid, dim3(256), 0, stream, __VA_ARGS__); \
    else if (K <= 16)                                                                            \
      hipLaunchKernelGGL((KERNEL<16, TT>), grid, dim3(256), 0, stream, __VA_ARGS__);             \
    else hipLaunchKernelGGL((KERNEL<32, TT>), grid, dim3(256), 0, stream, __VA_ARGS__);          \
  } while (0)

template <typename TT>
int launch_lossk_grad(const float* logits, const TT* target, const LossWsK& ws, float* dlogits,
                      int N, int K, int HW, int ignore_index, const float* upstream,
                      hipStream_t stream) {
  int gblocks = ceil_div(HW, 256 * 4);
  if (gblocks < 1) gblocks = 1;
  UNET_KP_DISPATCH(lossk_grad_kernel, TT, dim3(gblocks, N), stream, logits, target,
                   (const LossCoefK*)ws.coef, (const float*)ws.dice_ab, dlogits, HW, K,
                   ignore_index, upstream);
  UNET_CHECK_LAUNCH("lossk_grad");
  return UNET_OK;
}

template <typename TT>
int lossk_fwd_bwd_impl(const float* logits, const TT* target, float* loss_out, float* dlogits,
                       void* workspace, size_t workspace_bytes, int N, int K, int H, int W,
                       float smooth, float w_dice, float w_ce, int ignore_index,
                       int dynamic_weights, const float* class_weights, float grad_scale,
                       hipStream_t stream) {
  UNET_REQUIRE(logits && target && loss_out && workspace, "dice_wce_lossk: null pointer");
  const int rc = checkk<TT>("dice_wce_lossk", N, K, H, W, ignore_index);
  if (rc != UNET_OK) return rc;
  if (workspace_bytes < lossk_ws_layout(N, K, nullptr, nullptr)) {
    unet_set_error("dice_wce_lossk: workspace too small");
    return UNET_E_WORKSPACE;
  }
  LossWsK ws;
  lossk_ws_layout(N, K, &ws, reinterpret_cast<char*>(workspace));
  const int HW = H * W, blocks = lossk_blocks_for(HW);
  UNET_KP_DISPATCH(lossk_reduce_kernel, TT, dim3(blocks, N), stream, logits, target, ws.partial,
                   HW, K, ignore_index);
  UNET_CHECK_LAUNCH("lossk_reduce");
  hipLaunchKernelGGL(lossk_finalize_kernel, dim3(1), dim3(1024), 0, stream,
                     (const float*)ws.partial, ws.sums, N, K, blocks, smooth, w_dice, w_ce,
                     dynamic_weights, class_weights, grad_scale, loss_out, ws.coef, ws.dice_ab);
  UNET_CHECK_LAUNCH("lossk_finalize");
  if (dlogits)
    return launch_lossk_grad(logits, target, ws, dlogits, N, K, HW, ignore_index, nullptr, stream);
  return UNET_OK;
}

template <typename TT>
int lossk_grad_impl(const float* logits, const TT* target, const void* workspace,
                    size_t workspace_bytes, const float* upstream, float* dlogits, int N, int K,
                    int H, int W, int ignore_index, hipStream_t stream) {
  UNET_REQUIRE(logits && target && workspace && dlogits, "dice_wce_lossk_grad: null pointer");
  const int rc = checkk<TT>("dice_wce_lossk_grad", N, K, H, W, ignore_index);
  if (rc != UNET_OK) return rc;
  if (workspace_bytes < lossk_ws_layout(N, K, nullptr, nullptr)) {
    unet_set_error("dice_wce_lossk_grad: workspace too small");
    return UNET_E_WORKSPACE;
  }
  LossWsK ws;
  lossk_ws_layout(N, K, &ws, reinterpret_cast<char*>(const_cast<void*>(workspace)));
  return launch_lossk_grad(logits, target, ws, dlogits, N, K, H * W, ignore_index, upstream,
                           stream);
}

template <typename TT>
int argmax_countsk_impl(const float* logits, const TT* target, uint8_t* preds, uint64_t* counts,
                        int N, int K, int H, int W, int ignore_index, hipStream_t stream) {
  UNET_REQUIRE(logits && ((target && counts) || (!target && preds)),
               "argmax_countsk: needs target + counts, or preds alone");
  const int rc = checkk<TT>("argmax_countsk", N, K, H, W, ignore_index, 65535);
  if (rc != UNET_OK) return rc;
  const int HW = H * W;
  if (counts) UNET_HIP_CALL(hipMemsetAsync(counts, 0, (size_t)K * 3 * sizeof(uint64_t), stream));
  int blocks = ceil_div(HW, 256 * 4);
  if (blocks > 256) blocks = 256;
  UNET_KP_DISPATCH(argmax_countsk_kernel, TT, dim3(blocks, N), stream, logits, target, preds,
                   reinterpret_cast<unsigned long long*>(counts), HW, K, ignore_index);
  UNET_CHECK_LAUNCH("argmax_countsk");
  return UNET_OK;
}

inline const long long* i64(const int64_t* t) { return reinterpret_cast<const long long*>(t); }
}  // namespace

// ---- the head, reached from the unet_head1x1_* entry points of head_loss.hip for K > 4 ---------
int unet_headk_fwd(const void* a, int a_is_bf16, const float* w, const float* b, float* logits,
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
int unet_headk_bwd(const void* a, int b16, const float* dl, const float* w, void* da, float* dw,
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

// ---- K-class loss and counts ---------------------------------------------------------------------
extern "C" size_t unet_dice_wce_lossk_workspace_bytes(int N, int K, int H, int W) {
  if (N <= 0 || N > LOSSK_MAX_N || K < 2 || K > KMAX || H <= 0 || W <= 0) return 0;
  return lossk_ws_layout(N, K, nullptr, nullptr);
}

#define UNET_LOSSK_FWD_BWD_ARGS                                                                   \
  float *loss_out, float *dlogits, void *workspace, size_t workspace_bytes, int N, int K, int H,  \
      int W, float smooth, float w_dice, float w_ce, int ignore_index, int dynamic_weights,       \
      const float *class_weights, float grad_scale, unet_stream_t stream
#define UNET_LOSSK_FWD_BWD_PASS                                                                   \
  loss_out, dlogits, workspace, workspace_bytes, N, K, H, W, smooth, w_dice, w_ce, ignore_index,  \
      dynamic_weights, class_weights, grad_scale, (hipStream_t)stream

extern "C" int unet_dice_wce_lossk_fwd_bwd(const float* logits, const int64_t* target,
                                           UNET_LOSSK_FWD_BWD_ARGS) {
  return lossk_fwd_bwd_impl(logits, i64(target), UNET_LOSSK_FWD_BWD_PASS);
}
extern "C" int unet_dice_wce_lossk_fwd_bwd_u8(const float* logits, const uint8_t* target,
                                              UNET_LOSSK_FWD_BWD_ARGS) {
  return lossk_fwd_bwd_impl(logits, target, UNET_LOSSK_FWD_BWD_PASS);
}
#undef UNET_LOSSK_FWD_BWD_ARGS
#undef UNET_LOSSK_FWD_BWD_PASS

extern "C" int unet_dice_wce_lossk_grad(const float* logits, const int64_t* target,
                                        const void* workspace, size_t workspace_bytes,
                                        const float* upstream, float* dlogits, int N, int K,
                                        int H, int W, int ignore_index, unet_stream_t stream) {
  return lossk_grad_impl(logits, i64(target), workspace, workspace_bytes, upstream, dlogits, N, K,
                         H, W, ignore_index, (hipStream_t)stream);
}
extern "C" int unet_dice_wce_lossk_grad_u8(const float* logits, const uint8_t* target,
                                           const void* workspace, size_t workspace_bytes,
                                           const float* upstream, float* dlogits, int N, int K,
                                           int H, int W, int ignore_index, unet_stream_t stream) {
  return lossk_grad_impl(logits, target, workspace, workspace_bytes, upstream, dlogits, N, K, H, W,
                         ignore_index, (hipStream_t)stream);
}

extern "C" int unet_argmax_countsk(const float* logits_nchw, const int64_t* target, uint8_t* preds,
                                   uint64_t* counts, int N, int K, int H, int W, int ignore_index,
                                   unet_stream_t stream) {
  return argmax_countsk_impl(logits_nchw, i64(target), preds, counts, N, K, H, W, ignore_index,
                             (hipStream_t)stream);
}
extern "C" int unet_argmax_countsk_u8(const float* logits_nchw, const uint8_t* target,
                                      uint8_t* preds, uint64_t* counts, int N, int K, int H, int W,
                                      int ignore_index, unet_stream_t stream) {
  return argmax_countsk_impl(logits_nchw, target, preds, counts, N, K, H, W, ignore_index,
                             (hipStream_t)stream);
}
