// loss.hip — SimpleLoss (dynamic inverse-frequency weighted CE + soft Dice, ignore_index) forward
// + closed-form gradient, and the argmax / integer counts behind validate()'s Dice scores, for
// 2 <= K <= 32 classes.  All HBM-bound; per-(n,class) reductions go through per-block slabs and a
// single-block finalize in double (fixed order).
//
// Two kernel sets behind one host implementation per operation, which chooses on K:
//
//   K == 3   loss_reduce[_u8]_kernel, loss_finalize_kernel, loss_grad[_u8]_kernel,
//            argmax_counts_kernel: the pet trimap's, what a 3-class step launches; the sharded
//            (data-parallel) pair loss_shard_stats_kernel / loss_shard_apply_kernel exists for
//            this set only
//   else     lossk_reduce_kernel, lossk_finalize_kernel, lossk_grad_kernel, argmax_countsk_kernel,
//            instantiated for K padded to 4, 8, 16 or 32: the reference's definitions with 3
//            replaced by K
//
// Replaces SimpleLoss.forward + autograd (Our_UNet/models/losses.py:24-121) and the counting of
// validate() (Our_UNet/src/train.py:556-577).
#include "common.h"

namespace {

constexpr int KMAX = 32;          // UNET_MAX_CLASSES

// ------------------------------------------------------------------ loss, 3 classes
constexpr int LQ = 13;  // cnt[3], nll[3], I[3], P[3], valid
constexpr int LOSS_BLOCKS = 128;  // per image (either kernel set)
constexpr int LOSS_MAX_N = 1024;  // images per call (unet_hip.h); sizes loss_finalize_kernel's LDS opt-in

struct LossCoef {  // written by finalize, read by the gradient kernel
  float w[3];
  float inv_wsum;   // w_ce / sum_i w[t_i]
  float wdice;
};

__device__ __forceinline__ void softmax3(float z0, float z1, float z2, float& p0, float& p1,
                                         float& p2, float& lse) {
  const float m = fmaxf(z0, fmaxf(z1, z2));
  const float e0 = expf(z0 - m), e1 = expf(z1 - m), e2 = expf(z2 - m);
  const float s = e0 + e1 + e2;
  const float inv = 1.f / s;
  p0 = e0 * inv; p1 = e1 * inv; p2 = e2 * inv;
  lse = m + logf(s);
}

// Labels of V consecutive pixels.  TT = long long: the int64 target as stored.  TT = unsigned
// char: the dataset's raw uint8 mask, cleaned on load with its rule v > 2 && v != 255 -> 0
// (Our_UNet/src/train.py:300; the identity on a cleaned mask) - V = 4 pixels are ONE 4-byte load.
template <int V>
__device__ __forceinline__ void load_targets(const long long* tg, long long (&t)[V]) {
#pragma unroll
  for (int j = 0; j < V; ++j) t[j] = tg[j];
}
template <int V>
__device__ __forceinline__ void load_targets(const unsigned char* tg, long long (&t)[V]) {
  static_assert(V == 1 || V == 4, "one byte or one 32-bit word");
  unsigned w;
  if constexpr (V == 4) w = *reinterpret_cast<const unsigned*>(tg);
  else w = tg[0];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const unsigned v = (w >> (8 * j)) & 0xffu;
    t[j] = (v > 2u && v != 255u) ? 0 : (long long)v;
    // the label's small range is hidden from the optimiser: knowing it, hipcc compares in 16 bits
    // and then fuses other multiply-adds in the gradient kernel than in the int64 instantiation
    // (one-ulp differences in dlogits); behind this the two instantiations are the same code
    asm("" : "+v"(t[j]));
  }
}
template <typename TT>
__device__ __forceinline__ long long load_target(const TT* tg) {
  long long t[1];
  load_targets<1>(tg, t);
  return t[0];
}
// V consecutive floats as one load (V = 4: 16 bytes, the address 16-byte aligned)
template <int V>
__device__ __forceinline__ void ldv(const float* p, float (&v)[V]) {
  if constexpr (V == 4) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(p);
    v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
  } else {
    v[0] = p[0];
  }
}
// One pixel per lane for either target type: the per-lane fp32 sums and their merge order are
// what the loss value is made of, so the uint8 form keeps the int64 form's pixel-to-lane map (and
// with it the same bits); the label is 1 of the 13 bytes a pixel costs here.
template <typename TT>
__device__ __forceinline__ void loss_reduce_body(const float* __restrict__ logits,
                                                 const TT* __restrict__ target,
                                                 float* __restrict__ partial, int HW,
                                                 int ignore_index) {
  __shared__ float red[4][LQ];
  const int n = blockIdx.y;
  const float* z = logits + (size_t)n * 3 * HW;
  const TT* tg = target + (size_t)n * HW;
  float q[LQ];
#pragma unroll
  for (int i = 0; i < LQ; ++i) q[i] = 0.f;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
    const long long t = load_target(tg + p);
    const bool valid = (t != (long long)ignore_index);
    float p0, p1, p2, lse;
    const float z0 = z[p], z1 = z[HW + p], z2 = z[2 * HW + p];
    softmax3(z0, z1, z2, p0, p1, p2, lse);
    if (valid) {
      q[12] += 1.f;
      q[9] += p0; q[10] += p1; q[11] += p2;
      if (t == 0) { q[0] += 1.f; q[3] += lse - z0; q[6] += p0; }
      else if (t == 1) { q[1] += 1.f; q[4] += lse - z1; q[7] += p1; }
      else if (t == 2) { q[2] += 1.f; q[5] += lse - z2; q[8] += p2; }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < LQ; ++i) {
    const float s = wave_sum(q[i]);
    if (lane == 0) red[wave][i] = s;
  }
  __syncthreads();
  if (threadIdx.x < LQ) {
    const int i = threadIdx.x;
    partial[((size_t)n * gridDim.x + blockIdx.x) * LQ + i] =
        (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
  }
}

// (the two instantiations as kernels of their own: the int64 one keeps its name)
__global__ __launch_bounds__(256) void loss_reduce_kernel(const float* __restrict__ logits,
                                                          const long long* __restrict__ target,
                                                          float* __restrict__ partial, int HW,
                                                          int ignore_index) {
  loss_reduce_body(logits, target, partial, HW, ignore_index);
}
__global__ __launch_bounds__(256) void loss_reduce_u8_kernel(const float* __restrict__ logits,
                                                             const unsigned char* __restrict__ target,
                                                             float* __restrict__ partial, int HW,
                                                             int ignore_index) {
  loss_reduce_body(logits, target, partial, HW, ignore_index);
}

// Sum of one column over the slabs, in slab order, in double: 32 loads in flight, then their adds
// (the order - and so the value - of the plain loop, which waited for one L2 round trip per slab:
// 27 us per step for the 128 slabs of a 512 x 512 image).
__device__ __forceinline__ double loss_column_sum(const float* __restrict__ col, int nblocks) {
  double s = 0.0;
  int b = 0;
  for (; b + 32 <= nblocks; b += 32) {
    float v[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) v[j] = col[(size_t)(b + j) * LQ];
#pragma unroll
    for (int j = 0; j < 32; ++j) s += (double)v[j];
  }
  for (; b < nblocks; ++b) s += (double)col[(size_t)b * LQ];
  return s;
}

// single block: thread i < N*LQ sums its column over the slabs (double), then thread 0
// evaluates the loss and the gradient coefficients.
__global__ __launch_bounds__(256) void loss_finalize_kernel(
    const float* __restrict__ partial, int N, int nblocks, float smooth, float w_dice, float w_ce,
    int dynamic_weights, const float* __restrict__ class_weights, float grad_scale,
    float* __restrict__ loss_out, LossCoef* __restrict__ coef, float* __restrict__ dice_ab) {
  extern __shared__ double sums[];  // [N][LQ]
  for (int i = threadIdx.x; i < N * LQ; i += blockDim.x) {
    const int n = i / LQ, k = i - n * LQ;
    sums[i] = loss_column_sum(partial + (size_t)n * nblocks * LQ + k, nblocks);
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double cnt[3] = {0, 0, 0}, nll[3] = {0, 0, 0}, total = 0;
  for (int n = 0; n < N; ++n) {
    for (int c = 0; c < 3; ++c) {
      cnt[c] += sums[n * LQ + c];
      nll[c] += sums[n * LQ + 3 + c];
    }
    total += sums[n * LQ + 12];
  }
  float w[3];
  if (dynamic_weights) {
    // Our_UNet/models/losses.py:44-60: count 0 -> 1, w = total/count, renormalised to sum 3
    float cw[3], ws = 0.f;
    for (int c = 0; c < 3; ++c) {
      const float cp = cnt[c] == 0 ? 1.f : (float)cnt[c];
      cw[c] = (float)total / cp;
      ws += cw[c];
    }
    for (int c = 0; c < 3; ++c) w[c] = cw[c] * (3.f / ws);
  } else {
    for (int c = 0; c < 3; ++c) w[c] = class_weights ? class_weights[c] : 1.f;
  }
  double num = 0, den = 0;
  for (int c = 0; c < 3; ++c) {
    num += (double)w[c] * nll[c];
    den += (double)w[c] * cnt[c];
  }
  const float ce = (float)(num / den);
  double dice_sum = 0;
  for (int c = 0; c < 3; ++c) {
    double dmean = 0;
    for (int n = 0; n < N; ++n) {
      const double I = sums[n * LQ + 6 + c], P = sums[n * LQ + 9 + c], T = sums[n * LQ + c];
      const double U = P + T;
      dmean += (2.0 * I + smooth) / (U + smooth);
      // d(dice loss)/dp_c at pixel i of image n = A*[t_i == c] + B (times valid mask)
      const double k = 1.0 / (3.0 * N);
      dice_ab[(n * 3 + c) * 2 + 0] = (float)(-2.0 * k / (U + smooth));
      dice_ab[(n * 3 + c) * 2 + 1] = (float)((2.0 * I + smooth) * k / ((U + smooth) * (U + smooth)));
    }
    dice_sum += 1.0 - dmean / N;
  }
  const float dice = (float)(dice_sum / 3.0);
  loss_out[0] = w_ce * ce + w_dice * dice;
  loss_out[1] = ce;
  loss_out[2] = dice;
  for (int c = 0; c < 3; ++c) {
    loss_out[3 + c] = w[c];
    coef->w[c] = w[c];
  }
  coef->inv_wsum = (float)((double)w_ce * grad_scale / den);
  coef->wdice = w_dice * grad_scale;
}

// ---- sharded batch (data parallel, "global-exact"): the loss of the concatenated batch ------
// Phase 1 leaves this shard's per-image sums in the workspace and its contribution to the
// batch-wide statistics in stats[10] = {cnt[3], nll[3], valid, sum_n dice_n[3]}; the host sums
// stats over the shards (an all-reduce of 80 bytes); phase 2 turns the global statistics into
// the loss value (identical on every shard) and this shard's gradient coefficients.
constexpr int LSTATS = 10;

__global__ __launch_bounds__(256) void loss_shard_stats_kernel(const float* __restrict__ partial,
                                                               int N, int nblocks, float smooth,
                                                               double* __restrict__ sums,
                                                               double* __restrict__ stats) {
  for (int i = threadIdx.x; i < N * LQ; i += blockDim.x) {
    const int n = i / LQ, k = i - n * LQ;
    sums[i] = loss_column_sum(partial + (size_t)n * nblocks * LQ + k, nblocks);
  }
  __syncthreads();   // global writes of this block are visible to it after the barrier
  if (threadIdx.x >= LSTATS) return;
  const int k = threadIdx.x;
  double s = 0.0;
  if (k < 7) {
    const int col = k < 6 ? k : 12;
    for (int n = 0; n < N; ++n) s += sums[n * LQ + col];
  } else {
    const int c = k - 7;
    for (int n = 0; n < N; ++n) {
      const double I = sums[n * LQ + 6 + c], U = sums[n * LQ + 9 + c] + sums[n * LQ + c];
      s += (2.0 * I + smooth) / (U + smooth);
    }
  }
  stats[k] = s;
}

__global__ void loss_shard_apply_kernel(const double* __restrict__ sums, int N,
                                        const double* __restrict__ g, int n_global, float smooth,
                                        float w_dice, float w_ce, int dynamic_weights,
                                        const float* __restrict__ class_weights, float grad_scale,
                                        float* __restrict__ loss_out, LossCoef* __restrict__ coef,
                                        float* __restrict__ dice_ab) {
  const double k = 1.0 / (3.0 * n_global);
  for (int i = threadIdx.x; i < N * 3; i += blockDim.x) {
    const int n = i / 3, c = i - n * 3;
    const double I = sums[n * LQ + 6 + c], U = sums[n * LQ + 9 + c] + sums[n * LQ + c];
    dice_ab[i * 2 + 0] = (float)(-2.0 * k / (U + smooth));
    dice_ab[i * 2 + 1] = (float)((2.0 * I + smooth) * k / ((U + smooth) * (U + smooth)));
  }
  if (threadIdx.x != 0) return;
  const double total = g[6];
  float w[3];
  if (dynamic_weights) {
    float cw[3], ws = 0.f;
    for (int c = 0; c < 3; ++c) {
      const float cp = g[c] == 0 ? 1.f : (float)g[c];
      cw[c] = (float)total / cp;
      ws += cw[c];
    }
    for (int c = 0; c < 3; ++c) w[c] = cw[c] * (3.f / ws);
  } else {
    for (int c = 0; c < 3; ++c) w[c] = class_weights ? class_weights[c] : 1.f;
  }
  double num = 0, den = 0, dice_sum = 0;
  for (int c = 0; c < 3; ++c) {
    num += (double)w[c] * g[3 + c];
    den += (double)w[c] * g[c];
    dice_sum += 1.0 - g[7 + c] / n_global;
  }
  const float ce = (float)(num / den);
  const float dice = (float)(dice_sum / 3.0);
  loss_out[0] = w_ce * ce + w_dice * dice;
  loss_out[1] = ce;
  loss_out[2] = dice;
  for (int c = 0; c < 3; ++c) {
    loss_out[3 + c] = w[c];
    coef->w[c] = w[c];
  }
  coef->inv_wsum = (float)((double)w_ce * grad_scale / den);
  coef->wdice = w_dice * grad_scale;
}

// One pixel per lane for either target type as well: equal bits with the int64 form are the
// contract of the uint8 twins, and a four-pixel form of this arithmetic is other code (the
// compiler fuses other multiply-adds: one-ulp differences in dlogits).
template <typename TT>
__device__ __forceinline__ void loss_grad_body(const float* __restrict__ logits,
                                               const TT* __restrict__ target,
                                               const LossCoef* __restrict__ coef,
                                               const float* __restrict__ dice_ab,
                                               float* __restrict__ dlogits, int HW,
                                               int ignore_index,
                                               const float* __restrict__ upstream) {
  const int n = blockIdx.y;
  const float* z = logits + (size_t)n * 3 * HW;
  float* dz = dlogits + (size_t)n * 3 * HW;
  // dL/d(loss) handed down by autograd (a device scalar; 1 for loss.backward()): applied to the
  // finished gradient, i.e. the same rounding as a separate `dlogits *= g` pass
  const float up = upstream ? upstream[0] : 1.f;
  const TT* tg = target + (size_t)n * HW;
  const float w0 = coef->w[0], w1 = coef->w[1], w2 = coef->w[2];
  const float iw = coef->inv_wsum, wd = coef->wdice;
  float A[3], B[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    A[c] = dice_ab[(n * 3 + c) * 2 + 0];
    B[c] = dice_ab[(n * 3 + c) * 2 + 1];
  }
  for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
    const long long t = load_target(tg + p);
    float g0 = 0.f, g1 = 0.f, g2 = 0.f;
    if (t != (long long)ignore_index) {
      float p0, p1, p2, lse;
      softmax3(z[p], z[HW + p], z[2 * HW + p], p0, p1, p2, lse);
      const float wt = (t == 0) ? w0 : (t == 1) ? w1 : (t == 2) ? w2 : 0.f;
      const float k = wt * iw;
      // weighted CE: w_t (p - onehot) / sum w
      g0 = k * (p0 - (t == 0 ? 1.f : 0.f));
      g1 = k * (p1 - (t == 1 ? 1.f : 0.f));
      g2 = k * (p2 - (t == 2 ? 1.f : 0.f));
      // dice through the softmax Jacobian: p_k (a_k - sum_c a_c p_c)
      const float a0 = B[0] + (t == 0 ? A[0] : 0.f);
      const float a1 = B[1] + (t == 1 ? A[1] : 0.f);
      const float a2 = B[2] + (t == 2 ? A[2] : 0.f);
      const float dot = a0 * p0 + a1 * p1 + a2 * p2;
      g0 += wd * p0 * (a0 - dot);
      g1 += wd * p1 * (a1 - dot);
      g2 += wd * p2 * (a2 - dot);
    }
    dz[p] = g0 * up; dz[HW + p] = g1 * up; dz[2 * HW + p] = g2 * up;
  }
}

__global__ __launch_bounds__(256) void loss_grad_kernel(const float* __restrict__ logits,
                                                        const long long* __restrict__ target,
                                                        const LossCoef* __restrict__ coef,
                                                        const float* __restrict__ dice_ab,
                                                        float* __restrict__ dlogits, int HW,
                                                        int ignore_index,
                                                        const float* __restrict__ upstream) {
  loss_grad_body(logits, target, coef, dice_ab, dlogits, HW, ignore_index, upstream);
}
__global__ __launch_bounds__(256) void loss_grad_u8_kernel(const float* __restrict__ logits,
                                                           const unsigned char* __restrict__ target,
                                                           const LossCoef* __restrict__ coef,
                                                           const float* __restrict__ dice_ab,
                                                           float* __restrict__ dlogits, int HW,
                                                           int ignore_index,
                                                           const float* __restrict__ upstream) {
  loss_grad_body(logits, target, coef, dice_ab, dlogits, HW, ignore_index, upstream);
}

// ------------------------------------------------------------------ validation metrics
// argmax over the 3 class planes (lowest index wins ties, like torch.argmax) and, per class,
// the exact integer counts the reference's validate() turns into Dice scores
// (Our_UNet/src/train.py:556-577): counts[c] = {intersection, predicted, labelled}, pixels
// labelled ignore_index excluded.
// V pixels per lane (comparisons and integer counts: any pixel-to-lane map gives the same result).
// V = 4 (uint8 targets, HW % 4 == 0, aligned tensors): one 4-byte label load, 16-byte logit loads
// and the four predictions as one 32-bit word; V = 1: any shape.
template <typename TT, int V>
__global__ __launch_bounds__(256) void argmax_counts_kernel(const float* __restrict__ logits,
                                                            const TT* __restrict__ target,
                                                            unsigned char* __restrict__ preds,
                                                            unsigned long long* __restrict__ counts,
                                                            int HW, int ignore_index) {
  __shared__ unsigned int red[4][9];
  const int n = blockIdx.y;
  const float* z = logits + (size_t)n * 3 * HW;
  const TT* tg = target + (size_t)n * HW;
  unsigned int q[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) q[i] = 0;
  for (int p = (blockIdx.x * 256 + threadIdx.x) * V; p < HW; p += gridDim.x * 256 * V) {
    float zv[3][V];
#pragma unroll
    for (int c = 0; c < 3; ++c) ldv<V>(z + (size_t)c * HW + p, zv[c]);
    int am[V];
    unsigned packed = 0;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      am[j] = 0;
      float best = zv[0][j];
      if (zv[1][j] > best) { best = zv[1][j]; am[j] = 1; }
      if (zv[2][j] > best) { best = zv[2][j]; am[j] = 2; }
      packed |= (unsigned)am[j] << (8 * j);
    }
    if (preds) {
      if constexpr (V == 4) *reinterpret_cast<unsigned*>(preds + (size_t)n * HW + p) = packed;
      else preds[(size_t)n * HW + p] = (unsigned char)am[0];
    }
    if (!target) continue;           // prediction only (inference)
    long long tv[V];
    load_targets<V>(tg + p, tv);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const long long t = tv[j];
      if (t != (long long)ignore_index) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const unsigned int pc = (am[j] == c), mc = (t == c);
          q[c * 3 + 0] += pc & mc;
          q[c * 3 + 1] += pc;
          q[c * 3 + 2] += mc;
        }
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    unsigned int v = q[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) red[wave][i] = v;
  }
  __syncthreads();
  if (target && threadIdx.x < 9) {
    const unsigned int s = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] +
                           red[3][threadIdx.x];
    if (s) atomicAdd(&counts[threadIdx.x], (unsigned long long)s);   // integer: order-independent
  }
}

// ------------------------------------------------------------------ K-class SimpleLoss
// Per image 4K + 1 sums: cnt[K], nll[K], I[K], P[K], valid.  KP = K padded to 4, 8, 16 or 32 is
// the template parameter: the class loops unroll, every per-class value lives in a register of
// its own and the class of a pixel's own label selects with compares (never an index).

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

// ------------------------------------------------------------------ host side
// One workspace layout for both kernel sets: per image LOSS_BLOCKS slabs of 4K + 1 sums, the
// coefficient record, the Dice gradient's (A, B) per image and class, the per-image sums in
// double.  Either set's record fits the 256 bytes the layout gives it, so at K == 3 the size is
// what the 3-class layout always was, and a workspace sized by either export serves both.
static_assert(LQ == 4 * 3 + 1, "the 3-class slab is the K-class slab at K == 3");
static_assert(sizeof(LossCoef) <= 256 && sizeof(LossCoefK) <= 256, "one 256-byte record");
struct LossWs {
  float* partial; void* coef; float* dice_ab; double* sums; size_t bytes;
  LossCoef* coef3() const { return static_cast<LossCoef*>(coef); }
  LossCoefK* coefk() const { return static_cast<LossCoefK*>(coef); }
};
LossWs loss_ws(void* base, int N, int K) {
  const size_t slab = 4 * (size_t)K + 1;
  WsLayout l(base);
  return {l.take<float>((size_t)N * LOSS_BLOCKS * slab, 256), l.take<char>(256, 256),
          l.take<float>((size_t)N * K * 2, 256), l.take<double>((size_t)N * slab, 256), l.bytes()};
}

int loss_blocks_for(int HW) {
  int blocks = ceil_div(HW, 256 * 8);
  if (blocks > LOSS_BLOCKS) blocks = LOSS_BLOCKS;
  return blocks < 1 ? 1 : blocks;
}

// The checks every entry point makes before a launch.  Both kernel sets index a batch's planes
// with int.  Target types: int64 labels, or (the `_u8` twins) the dataset's uint8 mask - a uint8
// label cannot equal an ignore_index outside 0..255, and one below K would ignore a class.
template <typename TT>
int loss_check(const char* name, int N, int K, int H, int W, int ignore_index,
               int max_n = LOSS_MAX_N) {
  UNET_REQUIRE(K >= 2 && K <= KMAX, "%s: needs 2 <= K <= %d classes (got %d)", name, KMAX, K);
  UNET_REQUIRE(N > 0 && N <= max_n && H > 0 && W > 0 && (long long)H * W * K <= 0x7fffffffll,
               "%s: bad shape (1 <= N <= %d images, K * H * W < 2^31)", name, max_n);
  if constexpr (sizeof(TT) == 1)
    UNET_REQUIRE(ignore_index >= K && ignore_index <= 255,
                 "%s: a uint8 target needs ignore_index in %d..255 (got %d)", name, K,
                 ignore_index);
  return UNET_OK;
}

// ... and, for the entry points that take a workspace, its size and its parts
template <typename TT>
int loss_open(const char* name, const void* workspace, size_t workspace_bytes, int N, int K,
              int H, int W, int ignore_index, LossWs* ws) {
  const int rc = loss_check<TT>(name, N, K, H, W, ignore_index);
  if (rc != UNET_OK) return rc;
  *ws = loss_ws(const_cast<void*>(workspace), N, K);
  UNET_REQUIRE_WS(workspace_bytes, ws->bytes, "%s: workspace too small", name);
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

// four pixels per lane: uint8 targets on images of whole 4-pixel groups, every tensor aligned for
// its 4- / 16-byte accesses (fresh allocations are; a view at an odd offset is not)
template <typename TT>
bool four_pixel_lanes(int HW, const void* f32_a, const void* f32_b, const void* u8_a,
                      const void* u8_b) {
  if (sizeof(TT) != 1 || HW % 4) return false;
  return (reinterpret_cast<uintptr_t>(f32_a) | reinterpret_cast<uintptr_t>(f32_b)) % 16 == 0 &&
         (reinterpret_cast<uintptr_t>(u8_a) | reinterpret_cast<uintptr_t>(u8_b)) % 4 == 0;
}

// the 3-class reduce (the loss and phase 1 of the sharded loss)
template <typename TT>
int launch_loss_reduce(const float* logits, const TT* target, float* partial, int N, int HW,
                       int blocks, int ignore_index, hipStream_t stream) {
  if constexpr (sizeof(TT) == 1)
    hipLaunchKernelGGL(loss_reduce_u8_kernel, dim3(blocks, N), dim3(256), 0, stream, logits,
                       target, partial, HW, ignore_index);
  else
    hipLaunchKernelGGL(loss_reduce_kernel, dim3(blocks, N), dim3(256), 0, stream, logits, target,
                       partial, HW, ignore_index);
  UNET_CHECK_LAUNCH("loss_reduce");
  return UNET_OK;
}

template <typename TT>
int launch_loss_grad(const float* logits, const TT* target, const LossWs& ws, float* dlogits,
                     int N, int K, int HW, int ignore_index, const float* upstream,
                     hipStream_t stream) {
  int gblocks = ceil_div(HW, 256 * 4);
  if (gblocks < 1) gblocks = 1;
  const dim3 grid(gblocks, N);
  if (K != 3)
    UNET_KP_DISPATCH(lossk_grad_kernel, TT, grid, stream, logits, target,
                     (const LossCoefK*)ws.coefk(), (const float*)ws.dice_ab, dlogits, HW, K,
                     ignore_index, upstream);
  else if constexpr (sizeof(TT) == 1)
    hipLaunchKernelGGL(loss_grad_u8_kernel, grid, dim3(256), 0, stream, logits, target, ws.coef3(),
                       ws.dice_ab, dlogits, HW, ignore_index, upstream);
  else
    hipLaunchKernelGGL(loss_grad_kernel, grid, dim3(256), 0, stream, logits, target, ws.coef3(),
                       ws.dice_ab, dlogits, HW, ignore_index, upstream);
  UNET_CHECK_LAUNCH("loss_grad");
  return UNET_OK;
}

template <typename TT>
int loss_fwd_bwd_impl(const float* logits, const TT* target, float* loss_out, float* dlogits,
                      void* workspace, size_t workspace_bytes, int N, int K, int H, int W,
                      float smooth, float w_dice, float w_ce, int ignore_index,
                      int dynamic_weights, const float* class_weights, float grad_scale,
                      hipStream_t stream) {
  UNET_REQUIRE(logits && target && loss_out && workspace, "dice_wce_loss: null pointer");
  LossWs ws;
  int rc = loss_open<TT>("dice_wce_loss", workspace, workspace_bytes, N, K, H, W, ignore_index,
                         &ws);
  if (rc != UNET_OK) return rc;
  const int HW = H * W, blocks = loss_blocks_for(HW);
  if (K != 3) {
    UNET_KP_DISPATCH(lossk_reduce_kernel, TT, dim3(blocks, N), stream, logits, target, ws.partial,
                     HW, K, ignore_index);
    UNET_CHECK_LAUNCH("lossk_reduce");
    hipLaunchKernelGGL(lossk_finalize_kernel, dim3(1), dim3(1024), 0, stream,
                       (const float*)ws.partial, ws.sums, N, K, blocks, smooth, w_dice, w_ce,
                       dynamic_weights, class_weights, grad_scale, loss_out, ws.coefk(),
                       ws.dice_ab);
    UNET_CHECK_LAUNCH("lossk_finalize");
  } else {
    rc = launch_loss_reduce(logits, target, ws.partial, N, HW, blocks, ignore_index, stream);
    if (rc != UNET_OK) return rc;
    // N * 104 bytes of dynamic LDS pass the 64 KiB a launch may ask for unasked at N = 631: opt
    // in, once per device, to what the largest admitted batch needs (104 KiB of the CU's 160)
    UNET_SET_DYN_LDS(loss_finalize_kernel, (size_t)LOSS_MAX_N * LQ * sizeof(double));
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(256), (size_t)N * LQ * sizeof(double),
                       stream, ws.partial, N, blocks, smooth, w_dice, w_ce, dynamic_weights,
                       class_weights, grad_scale, loss_out, ws.coef3(), ws.dice_ab);
    UNET_CHECK_LAUNCH("loss_finalize");
  }
  if (dlogits)
    return launch_loss_grad(logits, target, ws, dlogits, N, K, HW, ignore_index, nullptr, stream);
  return UNET_OK;
}

template <typename TT>
int loss_grad_impl(const float* logits, const TT* target, const void* workspace,
                   size_t workspace_bytes, const float* upstream, float* dlogits, int N, int K,
                   int H, int W, int ignore_index, hipStream_t stream) {
  UNET_REQUIRE(logits && target && workspace && dlogits, "dice_wce_loss_grad: null pointer");
  LossWs ws;
  const int rc = loss_open<TT>("dice_wce_loss_grad", workspace, workspace_bytes, N, K, H, W,
                               ignore_index, &ws);
  if (rc != UNET_OK) return rc;
  return launch_loss_grad(logits, target, ws, dlogits, N, K, H * W, ignore_index, upstream,
                          stream);
}

template <typename TT>
int argmax_counts_impl(const float* logits_nchw, const TT* target, uint8_t* preds,
                       uint64_t* counts, int N, int K, int H, int W, int ignore_index,
                       hipStream_t stream) {
  UNET_REQUIRE(logits_nchw && ((target && counts) || (!target && preds)),
               "argmax_dice_counts: needs target + counts, or preds alone");
  const int rc = loss_check<TT>("argmax_dice_counts", N, K, H, W, ignore_index, 65535);
  if (rc != UNET_OK) return rc;
  const int HW = H * W;
  if (counts) UNET_HIP_CALL(hipMemsetAsync(counts, 0, (size_t)K * 3 * sizeof(uint64_t), stream));
  int blocks = ceil_div(HW, 256 * 4);
  if (blocks > 256) blocks = 256;
  const dim3 grid(blocks, N);
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
  if (K != 3)
    UNET_KP_DISPATCH(argmax_countsk_kernel, TT, grid, stream, logits_nchw, target, preds, cnt, HW,
                     K, ignore_index);
  else if (four_pixel_lanes<TT>(HW, logits_nchw, nullptr, target, preds))   // (uint8 targets only)
    hipLaunchKernelGGL((argmax_counts_kernel<TT, sizeof(TT) == 1 ? 4 : 1>), grid, dim3(256), 0,
                       stream, logits_nchw, target, preds, cnt, HW, ignore_index);
  else
    hipLaunchKernelGGL((argmax_counts_kernel<TT, 1>), grid, dim3(256), 0, stream, logits_nchw,
                       target, preds, cnt, HW, ignore_index);
  UNET_CHECK_LAUNCH("argmax_counts");
  return UNET_OK;
}

// ---- the sharded loss: 3 classes only
template <typename TT>
int loss_shard_stats_impl(const float* logits, const TT* target, double* stats, void* workspace,
                          size_t workspace_bytes, int N, int H, int W, float smooth,
                          int ignore_index, hipStream_t stream) {
  UNET_REQUIRE(logits && target && stats && workspace, "loss_shard_stats: null pointer");
  LossWs ws;
  int rc = loss_open<TT>("loss_shard_stats", workspace, workspace_bytes, N, 3, H, W, ignore_index,
                         &ws);
  if (rc != UNET_OK) return rc;
  const int HW = H * W, blocks = loss_blocks_for(HW);
  rc = launch_loss_reduce(logits, target, ws.partial, N, HW, blocks, ignore_index, stream);
  if (rc != UNET_OK) return rc;
  hipLaunchKernelGGL(loss_shard_stats_kernel, dim3(1), dim3(256), 0, stream, ws.partial, N, blocks,
                     smooth, ws.sums, stats);
  UNET_CHECK_LAUNCH("loss_shard_stats");
  return UNET_OK;
}

template <typename TT>
int loss_shard_apply_impl(const float* logits, const TT* target, const double* global_stats,
                          int N_global, float* loss_out, float* dlogits, void* workspace,
                          size_t workspace_bytes, int N, int H, int W, float smooth, float w_dice,
                          float w_ce, int ignore_index, int dynamic_weights,
                          const float* class_weights, float grad_scale, hipStream_t stream) {
  UNET_REQUIRE(logits && target && global_stats && loss_out && workspace,
               "loss_shard_apply: null pointer");
  UNET_REQUIRE(N_global >= N, "loss_shard_apply: bad shape (N_global < N)");
  LossWs ws;
  const int rc = loss_open<TT>("loss_shard_apply", workspace, workspace_bytes, N, 3, H, W,
                               ignore_index, &ws);
  if (rc != UNET_OK) return rc;
  hipLaunchKernelGGL(loss_shard_apply_kernel, dim3(1), dim3(256), 0, stream, ws.sums, N,
                     global_stats, N_global, smooth, w_dice, w_ce, dynamic_weights, class_weights,
                     grad_scale, loss_out, ws.coef3(), ws.dice_ab);
  UNET_CHECK_LAUNCH("loss_shard_apply");
  if (dlogits)
    return launch_loss_grad(logits, target, ws, dlogits, N, 3, H * W, ignore_index, nullptr,
                            stream);
  return UNET_OK;
}

inline const long long* i64(const int64_t* t) { return reinterpret_cast<const long long*>(t); }
}  // namespace

// ---- exports: the int64-target entry points and their uint8-target twins (`_u8`: the dataset's
// raw mask, cleaned on load), one implementation each, instantiated on the target type.  The
// K-class forms take any 2 <= K <= 32; the forms without a K are the same call at K == 3.
extern "C" size_t unet_dice_wce_loss_workspace_bytes(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  return loss_ws(nullptr, N, 3).bytes;
}
extern "C" size_t unet_dice_wce_lossk_workspace_bytes(int N, int K, int H, int W) {
  if (N <= 0 || N > LOSS_MAX_N || K < 2 || K > KMAX || H <= 0 || W <= 0) return 0;
  return loss_ws(nullptr, N, K).bytes;
}

// (the argument list after the classes, and how the implementation receives it)
#define UNET_LOSS_FWD_BWD_ARGS                                                                   \
  int H, int W, float smooth, float w_dice, float w_ce, int ignore_index, int dynamic_weights,   \
      const float *class_weights, float grad_scale, unet_stream_t stream
#define UNET_LOSS_FWD_BWD_PASS                                                                   \
  H, W, smooth, w_dice, w_ce, ignore_index, dynamic_weights, class_weights, grad_scale,          \
      (hipStream_t)stream

extern "C" int unet_dice_wce_lossk_fwd_bwd(const float* logits, const int64_t* target,
                                           float* loss_out, float* dlogits, void* workspace,
                                           size_t workspace_bytes, int N, int K,
                                           UNET_LOSS_FWD_BWD_ARGS) {
  return loss_fwd_bwd_impl(logits, i64(target), loss_out, dlogits, workspace, workspace_bytes, N,
                           K, UNET_LOSS_FWD_BWD_PASS);
}
extern "C" int unet_dice_wce_lossk_fwd_bwd_u8(const float* logits, const uint8_t* target,
                                              float* loss_out, float* dlogits, void* workspace,
                                              size_t workspace_bytes, int N, int K,
                                              UNET_LOSS_FWD_BWD_ARGS) {
  return loss_fwd_bwd_impl(logits, target, loss_out, dlogits, workspace, workspace_bytes, N, K,
                           UNET_LOSS_FWD_BWD_PASS);
}
extern "C" int unet_dice_wce_loss_fwd_bwd(const float* logits, const int64_t* target,
                                          float* loss_out, float* dlogits, void* workspace,
                                          size_t workspace_bytes, int N, UNET_LOSS_FWD_BWD_ARGS) {
  return loss_fwd_bwd_impl(logits, i64(target), loss_out, dlogits, workspace, workspace_bytes, N,
                           3, UNET_LOSS_FWD_BWD_PASS);
}
extern "C" int unet_dice_wce_loss_fwd_bwd_u8(const float* logits, const uint8_t* target,
                                             float* loss_out, float* dlogits, void* workspace,
                                             size_t workspace_bytes, int N,
                                             UNET_LOSS_FWD_BWD_ARGS) {
  return loss_fwd_bwd_impl(logits, target, loss_out, dlogits, workspace, workspace_bytes, N, 3,
                           UNET_LOSS_FWD_BWD_PASS);
}
#undef UNET_LOSS_FWD_BWD_ARGS
#undef UNET_LOSS_FWD_BWD_PASS

extern "C" int unet_dice_wce_lossk_grad(const float* logits, const int64_t* target,
                                        const void* workspace, size_t workspace_bytes,
                                        const float* upstream, float* dlogits, int N, int K,
                                        int H, int W, int ignore_index, unet_stream_t stream) {
  return loss_grad_impl(logits, i64(target), workspace, workspace_bytes, upstream, dlogits, N, K,
                        H, W, ignore_index, (hipStream_t)stream);
}
extern "C" int unet_dice_wce_lossk_grad_u8(const float* logits, const uint8_t* target,
                                           const void* workspace, size_t workspace_bytes,
                                           const float* upstream, float* dlogits, int N, int K,
                                           int H, int W, int ignore_index, unet_stream_t stream) {
  return loss_grad_impl(logits, target, workspace, workspace_bytes, upstream, dlogits, N, K, H, W,
                        ignore_index, (hipStream_t)stream);
}
extern "C" int unet_dice_wce_loss_grad(const float* logits, const int64_t* target,
                                       const void* workspace, size_t workspace_bytes,
                                       const float* upstream, float* dlogits, int N, int H, int W,
                                       int ignore_index, unet_stream_t stream) {
  return loss_grad_impl(logits, i64(target), workspace, workspace_bytes, upstream, dlogits, N, 3,
                        H, W, ignore_index, (hipStream_t)stream);
}
extern "C" int unet_dice_wce_loss_grad_u8(const float* logits, const uint8_t* target,
                                          const void* workspace, size_t workspace_bytes,
                                          const float* upstream, float* dlogits, int N, int H,
                                          int W, int ignore_index, unet_stream_t stream) {
  return loss_grad_impl(logits, target, workspace, workspace_bytes, upstream, dlogits, N, 3, H, W,
                        ignore_index, (hipStream_t)stream);
}

extern "C" int unet_argmax_countsk(const float* logits_nchw, const int64_t* target, uint8_t* preds,
                                   uint64_t* counts, int N, int K, int H, int W, int ignore_index,
                                   unet_stream_t stream) {
  return argmax_counts_impl(logits_nchw, i64(target), preds, counts, N, K, H, W, ignore_index,
                            (hipStream_t)stream);
}
extern "C" int unet_argmax_countsk_u8(const float* logits_nchw, const uint8_t* target,
                                      uint8_t* preds, uint64_t* counts, int N, int K, int H, int W,
                                      int ignore_index, unet_stream_t stream) {
  return argmax_counts_impl(logits_nchw, target, preds, counts, N, K, H, W, ignore_index,
                            (hipStream_t)stream);
}
extern "C" int unet_argmax_dice_counts(const float* logits_nchw, const int64_t* target,
                                       uint8_t* preds, uint64_t* counts, int N, int H, int W,
                                       int ignore_index, unet_stream_t stream) {
  return argmax_counts_impl(logits_nchw, i64(target), preds, counts, N, 3, H, W, ignore_index,
                            (hipStream_t)stream);
}
extern "C" int unet_argmax_dice_counts_u8(const float* logits_nchw, const uint8_t* target,
                                          uint8_t* preds, uint64_t* counts, int N, int H, int W,
                                          int ignore_index, unet_stream_t stream) {
  return argmax_counts_impl(logits_nchw, target, preds, counts, N, 3, H, W, ignore_index,
                            (hipStream_t)stream);
}

// ---- the sharded loss (3 classes)
extern "C" int unet_dice_wce_loss_shard_stats(const float* logits, const int64_t* target,
                                              double* stats, void* workspace,
                                              size_t workspace_bytes, int N, int H, int W,
                                              float smooth, int ignore_index,
                                              unet_stream_t stream) {
  return loss_shard_stats_impl(logits, i64(target), stats, workspace, workspace_bytes, N, H, W,
                               smooth, ignore_index, (hipStream_t)stream);
}
extern "C" int unet_dice_wce_loss_shard_stats_u8(const float* logits, const uint8_t* target,
                                                 double* stats, void* workspace,
                                                 size_t workspace_bytes, int N, int H, int W,
                                                 float smooth, int ignore_index,
                                                 unet_stream_t stream) {
  return loss_shard_stats_impl(logits, target, stats, workspace, workspace_bytes, N, H, W, smooth,
                               ignore_index, (hipStream_t)stream);
}

#define UNET_LOSS_SHARD_APPLY_ARGS                                                               \
  const double *global_stats, int N_global, float *loss_out, float *dlogits, void *workspace,    \
      size_t workspace_bytes, int N, int H, int W, float smooth, float w_dice, float w_ce,       \
      int ignore_index, int dynamic_weights, const float *class_weights, float grad_scale,       \
      unet_stream_t stream

extern "C" int unet_dice_wce_loss_shard_apply(const float* logits, const int64_t* target,
                                              UNET_LOSS_SHARD_APPLY_ARGS) {
  return loss_shard_apply_impl(logits, i64(target), global_stats, N_global, loss_out, dlogits,
                               workspace, workspace_bytes, N, H, W, smooth, w_dice, w_ce,
                               ignore_index, dynamic_weights, class_weights, grad_scale,
                               (hipStream_t)stream);
}
extern "C" int unet_dice_wce_loss_shard_apply_u8(const float* logits, const uint8_t* target,
                                                 UNET_LOSS_SHARD_APPLY_ARGS) {
  return loss_shard_apply_impl(logits, target, global_stats, N_global, loss_out, dlogits,
                               workspace, workspace_bytes, N, H, W, smooth, w_dice, w_ce,
                               ignore_index, dynamic_weights, class_weights, grad_scale,
                               (hipStream_t)stream);
}
#undef UNET_LOSS_SHARD_APPLY_ARGS
