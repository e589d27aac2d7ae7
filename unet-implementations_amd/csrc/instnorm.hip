// instnorm.hip — InstanceNorm2d(eps, affine) + LeakyReLU + SpatialDropout2d,
// forward and backward, on NHWC fp32 planes.  Pure HBM-bound streaming kernels:
// float4 per lane along the contiguous channel axis, per-(n,c) reductions done
// as per-thread register partials -> LDS -> per-block slabs -> a finalize
// kernel that merges slabs in fixed order (deterministic run to run).
//
// Statistics use chunked Welford/Chan merging of (count, mean, M2) so the
// variance does not suffer E[x^2]-E[x]^2 cancellation (the reference's CPU path
// accumulates in double: aten::native_batch_norm as lowered from
// nn.InstanceNorm2d, Our_UNet/models/unet.py:118-119).
#include "common.h"

namespace {

constexpr int kThreads = 256;

__host__ __device__ inline int split_for(int N, int HW, int C) {
  // enough blocks to fill the chip (~2048) but at least 64 pixels-iterations per block
  int ppi = kThreads / (C / 4);
  if (ppi < 1) ppi = 1;
  int max_split = HW / (ppi * 8);
  if (max_split < 1) max_split = 1;
  int want = (2048 + N - 1) / N;
  int s = want < max_split ? want : max_split;
  return s < 1 ? 1 : s;
}

// ---------------------------------------------------------------- statistics
// grid (split, N); partial[n][s][c] = (mean, M2), count implied by the pixel range.
// The merges of chunk and lane means are first order in the rounding of those means, an ulp of
// |mean|: on a block far from 0 (|mean| / std = R) M2 comes out wrong by ~7e-8 R relative, which
// many pixels per lane average away and few do not (2 x 2 pixels at R = 5000: rstd to 1.7e-4).
// So on a block of at most 64 pixels the thread that merges a channel tests R: above 64 (~2e-6
// in rstd) it forms the block's M2 again in one pass around the merged mean, M2 = sum(d^2) -
// (sum d)^2 / n with d = y - mean (the second term is a correction of rounding size, nothing
// cancels): at most 64 loads.  Larger blocks average the error by ~sqrt(8 / n): measured 6e-6 in
// rstd at R = 1000 on 77 pixels.
template <typename TS>
__global__ __launch_bounds__(kThreads) void in_stats_kernel(const TS* __restrict__ y,
                                                            float2* __restrict__ partial, int HW,
                                                            int C, int split) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // [groups][C][3]
  const int lpp = C >> 2;
  const int groups = kThreads / lpp;  // pixel groups per iteration
  const int tid = threadIdx.x;
  const int grp = tid / lpp, c4 = tid - grp * lpp;
  const int n = blockIdx.y, s = blockIdx.x;
  const int per = (HW + split - 1) / split;
  const int p_begin = s * per;
  const int p_end = min(p_begin + per, HW);
  const TS* base = y + (size_t)n * HW * C + c4 * 4;

  float cnt = 0.f;
  f32x4 mean = {0.f, 0.f, 0.f, 0.f}, m2 = {0.f, 0.f, 0.f, 0.f};
  if (grp < groups) {
    int pp = p_begin + grp;
    while (pp < p_end) {
      f32x4 v[8];
      int k = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int q = pp + j * groups;
        if (q < p_end) {
          v[j] = ld4(base + (size_t)q * C);
          ++k;
        } else {
          v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
      }
      const float kf = (float)k, inv = 1.f / kf;
      f32x4 sm = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 8; ++j) sm += v[j];
      const f32x4 mu = sm * inv;
      f32x4 q2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < k) {
          const f32x4 d = v[j] - mu;
          q2 += d * d;
        }
      // merge chunk (kf, mu, q2) into (cnt, mean, m2)
      const float nt = cnt + kf;
      const float f = kf / nt;
      const f32x4 d = mu - mean;
      mean += d * f;
      m2 += q2 + d * d * (cnt * f);
      cnt = nt;
      pp += 8 * groups;
    }
  }
  // block merge across pixel groups
  float* sm_cnt = smem;                    // [groups][lpp]
  float* sm_mean = smem + groups * lpp;    // [groups][C]
  float* sm_m2 = sm_mean + groups * C;     // [groups][C]
  if (grp < groups) {
    sm_cnt[grp * lpp + c4] = cnt;
    *reinterpret_cast<f32x4*>(sm_mean + grp * C + c4 * 4) = mean;
    *reinterpret_cast<f32x4*>(sm_m2 + grp * C + c4 * 4) = m2;
  }
  __syncthreads();
  for (int c = tid; c < C; c += kThreads) {
    float n0 = 0.f, mu = 0.f, q = 0.f;
    for (int g = 0; g < groups; ++g)
      wf_merge(n0, mu, q, sm_cnt[g * lpp + (c >> 2)], sm_mean[g * C + c], sm_m2[g * C + c]);
    if (n0 <= 64.f && q > 0.f && mu * mu * n0 > 4096.f * q) {
      const TS* col = y + (size_t)n * HW * C + c;
      float s1 = 0.f, s2 = 0.f;
      for (int p = p_begin; p < p_end; ++p) {
        const float d = (float)col[(size_t)p * C] - mu;
        s1 += d;
        s2 = fmaf(d, d, s2);
      }
      const float dm = s1 / n0;
      q = fmaxf(s2 - s1 * dm, 0.f);
      mu += dm;
    }
    partial[((size_t)n * split + s) * C + c] = float2{mu, q};
  }
}

// block = 32 channels x FL lanes, grid (C/32, N): lane l merges slabs l, l+FL, ... in order,
// then the FL lane results are merged by a fixed pairwise tree (deterministic).
constexpr int FL = 32;
__global__ __launch_bounds__(32 * FL) void in_stats_finalize_kernel(
    const float2* __restrict__ partial, const float* __restrict__ gamma,
    const float* __restrict__ beta, float eps, const float* __restrict__ mask,
    float* __restrict__ mean, float* __restrict__ rstd, float* __restrict__ alpha,
    float* __restrict__ beta2, int N, int HW, int C, int split) {
  __shared__ float sn[FL][33], sm[FL][33], sq[FL][33];
  const int cl = threadIdx.x & 31, l = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl, n = blockIdx.y;
  const int per = (HW + split - 1) / split;
  float cnt = 0.f, mu = 0.f, q = 0.f;
  if (c < C) {
    for (int s = l; s < split; s += FL) {
      const int pb = s * per;
      int pe = pb + per;
      if (pe > HW) pe = HW;
      const int k = pe - pb;
      if (k <= 0) break;
      const float2 v = partial[((size_t)n * split + s) * C + c];
      wf_merge(cnt, mu, q, (float)k, v.x, v.y);
    }
  }
  sn[l][cl] = cnt; sm[l][cl] = mu; sq[l][cl] = q;
  __syncthreads();
  // fixed pairwise tree over the FL lane results: (l, l + stride)
#pragma unroll
  for (int stride = FL / 2; stride >= 1; stride >>= 1) {
    if (l < stride) {
      wf_merge(cnt, mu, q, sn[l + stride][cl], sm[l + stride][cl], sq[l + stride][cl]);
      sn[l][cl] = cnt; sm[l][cl] = mu; sq[l][cl] = q;
    }
    __syncthreads();
  }
  if (l == 0 && c < C) {
    const int i = n * C + c;
    const float var = q / (float)HW;  // biased, like F.instance_norm
    const float rs = 1.0f / sqrtf(var + eps);
    mean[i] = mu;
    rstd[i] = rs;
    const float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
    const float a = g * rs;
    // with `mask` (the fused layer pipeline) the dropout factor m >= 0 is folded into the
    // coefficients: lrelu(z) * m == lrelu(z * m)
    const float mk = mask ? mask[i] : 1.f;
    if (alpha) alpha[i] = a * mk;
    if (beta2) beta2[i] = (b - mu * a) * mk;
  }
}

// Finalize for the statistics epilogue of the convolutions: every one of the `tiles` summaries
// of an image holds the same number of pixels `per`, so the merge needs no running counts or
// divisions:  mean = avg(mean_t),  M2 = sum(M2_t) + per * sum((mean_t - mean)^2).
// block = 32 channels x FL lanes, grid (C/32, N); two passes over the (L2-resident) summaries,
// fixed-order LDS trees (deterministic).
__global__ __launch_bounds__(32 * FL) void in_stats_finalize_eq_kernel(
    const float2* __restrict__ partial, const float* __restrict__ gamma,
    const float* __restrict__ beta, float eps, const float* __restrict__ mask,
    float* __restrict__ mean, float* __restrict__ rstd, float* __restrict__ alpha,
    float* __restrict__ beta2, int HW, int C, int tiles, float per) {
  __shared__ float sa[FL][33];
  const int cl = threadIdx.x & 31, l = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl, n = blockIdx.y;
  const float2* src = partial + (size_t)n * tiles * C + c;
  auto block_sum = [&](float v) {
    sa[l][cl] = v;
    __syncthreads();
#pragma unroll
    for (int stride = FL / 2; stride >= 1; stride >>= 1) {
      if (l < stride) sa[l][cl] += sa[l + stride][cl];
      __syncthreads();
    }
    const float r = sa[0][cl];
    __syncthreads();
    return r;
  };
  float s = 0.f;
  if (c < C)
    for (int t = l; t < tiles; t += FL) s += src[(size_t)t * C].x;
  const float mu = block_sum(s) / (float)tiles;
  float q = 0.f;
  if (c < C)
    for (int t = l; t < tiles; t += FL) {
      const float2 v = src[(size_t)t * C];
      const float d = v.x - mu;
      q += fmaf(per * d, d, v.y);
    }
  q = block_sum(q);
  if (l == 0 && c < C) {
    const int i = n * C + c;
    const float var = q / (float)HW;  // biased, like F.instance_norm
    const float rs = 1.0f / sqrtf(var + eps);
    mean[i] = mu;
    rstd[i] = rs;
    const float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
    const float a = g * rs;
    const float mk = mask ? mask[i] : 1.f;
    if (alpha) alpha[i] = a * mk;
    if (beta2) beta2[i] = (b - mu * a) * mk;
  }
}

// Many tiles (the 512x512 / 256x256 layers: 2048 / 512 summaries per image and channel): the
// merge above would run on C/32 x N blocks only.  Two launches instead: G groups of tiles per
// (image, 32 channels) reduce shifted sums
//   S1 = sum(mean_t - K),  S2 = sum(M2_t + per (mean_t - K)^2),   K = mean of tile 0
// then one small kernel combines: M2 = S2 - tiles per (S1/tiles)^2.  Where the tile means cluster
// around the channel mean that subtraction cancels nothing of size, and every rounding error of
// the sums is a few ulp of S2.  That is an assumption about the plane (a bright image corner over
// a flat background breaks it: tile 0 lies far from the mean, S2 >> M2, and rstd lost four
// digits), so the combine kernel tests it.  S1 and S2 each carry a few eps of relative rounding
// error (lane sums of <= 8 terms, a 5-level tree, 16 groups) and M2 inherits that of S2
// magnified by S2 / M2 = 1 + (K - mean)^2 / var: while S2 <= 16 M2 (tile 0 within 3.9 standard
// deviations of the plane mean) the shifted result stands, good to ~1e-6 in rstd; otherwise the
// plane's wave merges its summaries again the way in_stats_finalize_eq_kernel does, mean =
// avg(mean_t), M2 = sum(M2_t) + per sum((mean_t - mean)^2), 64 lanes striding over the tiles and
// a fixed butterfly (2 x tiles / 64 loads per lane).  Deterministic either way.
constexpr int kFinGroups = 16;
__global__ __launch_bounds__(32 * FL) void in_stats_finalize_grp_kernel(
    const float2* __restrict__ partial, float2* __restrict__ grp, int C, int tiles, float per) {
  __shared__ float sa[FL][33], sb[FL][33];
  const int cl = threadIdx.x & 31, l = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl, n = blockIdx.y, g = blockIdx.z;
  const float2* src = partial + (size_t)n * tiles * C + c;
  const int t0 = (int)((long long)tiles * g / kFinGroups), t1 = (int)((long long)tiles * (g + 1) / kFinGroups);
  float s1 = 0.f, s2 = 0.f;
  if (c < C) {
    const float K = src[0].x;
    for (int t = t0 + l; t < t1; t += FL) {
      const float2 v = src[(size_t)t * C];
      const float d = v.x - K;
      s1 += d;
      s2 += fmaf(per * d, d, v.y);
    }
  }
  sa[l][cl] = s1; sb[l][cl] = s2;
  __syncthreads();
#pragma unroll
  for (int stride = FL / 2; stride >= 1; stride >>= 1) {
    if (l < stride) { sa[l][cl] += sa[l + stride][cl]; sb[l][cl] += sb[l + stride][cl]; }
    __syncthreads();
  }
  if (l == 0 && c < C) grp[((size_t)n * kFinGroups + g) * C + c] = float2{sa[0][cl], sb[0][cl]};
}

// block = 4 waves, one (image, channel) plane per wave.  Every lane forms the sums of the 16 groups
// in group order (the order a single thread would use), so the test below is uniform over the
// wave; where it fails the wave's 64 lanes stride over the plane's summaries together.
__device__ __forceinline__ float wave_sum(float v) {   // xor butterfly: the same bits on every lane
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

__global__ __launch_bounds__(256) void in_stats_finalize_comb_kernel(
    const float2* __restrict__ partial, const float2* __restrict__ grp,
    const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
    const float* __restrict__ mask, float* __restrict__ mean, float* __restrict__ rstd,
    float* __restrict__ alpha, float* __restrict__ beta2, int N, int HW, int C, int tiles,
    float per) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N * C) return;
  const int n = i / C, c = i - n * C;
  float2 mine = {0.f, 0.f};
  if (lane < kFinGroups) mine = grp[((size_t)n * kFinGroups + lane) * C + c];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int g = 0; g < kFinGroups; ++g) {
    s1 += __shfl(mine.x, g);
    s2 += __shfl(mine.y, g);
  }
  const float2* src = partial + (size_t)n * tiles * C + c;
  const float K = src[0].x;
  const float d = s1 / (float)tiles;
  float mu = K + d;
  float q = s2 - (float)tiles * per * d * d;
  if (!(s2 <= 16.f * q)) {   // the shift was a bad origin for this plane (also: q < 0, NaN)
    float a = 0.f;
    for (int t = lane; t < tiles; t += 64) a += src[(size_t)t * C].x;
    mu = wave_sum(a) / (float)tiles;
    a = 0.f;
    for (int t = lane; t < tiles; t += 64) {
      const float2 v = src[(size_t)t * C];
      const float dd = v.x - mu;
      a += fmaf(per * dd, dd, v.y);
    }
    q = wave_sum(a);
  }
  if (lane != 0) return;
  const float var = fmaxf(q, 0.f) / (float)HW;
  const float rs = 1.0f / sqrtf(var + eps);
  mean[i] = mu;
  rstd[i] = rs;
  const float gm = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
  const float a = gm * rs;
  const float mk = mask ? mask[i] : 1.f;
  if (alpha) alpha[i] = a * mk;
  if (beta2) beta2[i] = (b - mu * a) * mk;
}

// ---------------------------------------------------------------- forward apply
__global__ __launch_bounds__(kThreads) void in_apply_fwd_kernel(
    const float* __restrict__ y, const float* __restrict__ alpha, const float* __restrict__ beta2,
    const float* __restrict__ mask, float slope, float* __restrict__ a, long long total4, int HW,
    int C) {
  const int lpp = C >> 2;
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < total4; i += stride) {
    const long long pix = i / lpp;
    const int c = (int)(i - pix * lpp) * 4;
    const int n = (int)(pix / HW);
    const f32x4 v = *reinterpret_cast<const f32x4*>(y + i * 4);
    const f32x4 al = *reinterpret_cast<const f32x4*>(alpha + (size_t)n * C + c);
    const f32x4 be = *reinterpret_cast<const f32x4*>(beta2 + (size_t)n * C + c);
    f32x4 mk = {1.f, 1.f, 1.f, 1.f};
    if (mask) mk = *reinterpret_cast<const f32x4*>(mask + (size_t)n * C + c);
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float z = fmaf(v[k], al[k], be[k]);
      o[k] = (z > 0.f ? z : z * slope) * mk[k];
    }
    *reinterpret_cast<f32x4*>(a + i * 4) = o;
  }
}

// ---------------------------------------------------------------- backward
// pass 1: per (n,c) S1 = sum gz, S2 = sum gz*xhat, gz = ga*mask*lrelu'(z)
template <typename TS>
__global__ __launch_bounds__(kThreads) void in_bwd_reduce_kernel(
    const TS* __restrict__ ga, const TS* __restrict__ y, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ mask, float slope,
    float2* __restrict__ partial, int HW, int C, int split) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // [groups][C][2]
  const int lpp = C >> 2;
  const int groups = kThreads / lpp;
  const int tid = threadIdx.x;
  const int grp = tid / lpp, c4 = tid - grp * lpp;
  const int n = blockIdx.y, s = blockIdx.x;
  const int per = (HW + split - 1) / split;
  const int p_begin = s * per;
  const int p_end = min(p_begin + per, HW);
  f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
  if (grp < groups) {
    const int c = c4 * 4;
    const f32x4 mu = *reinterpret_cast<const f32x4*>(mean + (size_t)n * C + c);
    const f32x4 rs = *reinterpret_cast<const f32x4*>(rstd + (size_t)n * C + c);
    const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + c);
    const f32x4 b = *reinterpret_cast<const f32x4*>(beta + c);
    f32x4 mk = {1.f, 1.f, 1.f, 1.f};
    if (mask) mk = *reinterpret_cast<const f32x4*>(mask + (size_t)n * C + c);
    const size_t base = (size_t)n * HW * C + c;
    for (int pp = p_begin + grp; pp < p_end; pp += groups) {
      const f32x4 yv = ld4(y + base + (size_t)pp * C);
      const f32x4 gv = ld4(ga + base + (size_t)pp * C);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float xh = (yv[k] - mu[k]) * rs[k];
        const float al = g[k] * rs[k];
        const float z = fmaf(yv[k], al, b[k] - mu[k] * al);  // same expression as the forward
        const float gz = gv[k] * mk[k] * (z > 0.f ? 1.f : slope);
        s1[k] += gz;
        s2[k] = fmaf(gz, xh, s2[k]);
      }
    }
  }
  float* sm1 = smem;               // [groups][C]
  float* sm2 = smem + groups * C;  // [groups][C]
  if (grp < groups) {
    *reinterpret_cast<f32x4*>(sm1 + grp * C + c4 * 4) = s1;
    *reinterpret_cast<f32x4*>(sm2 + grp * C + c4 * 4) = s2;
  }
  __syncthreads();
  for (int c = tid; c < C; c += kThreads) {
    float a = 0.f, b = 0.f;
    for (int g = 0; g < groups; ++g) {
      a += sm1[g * C + c];
      b += sm2[g * C + c];
    }
    partial[((size_t)n * split + s) * C + c] = float2{a, b};
  }
}

// finalize 1: block = 32 channels x FL lanes, grid (C/32, N): sums[n][c] = (S1, S2),
// coef[n][c] = (S1/HW, S2/HW).  Lane l merges summaries l, l+FL, ... in order.  At 32 channels
// and 8 images the grid is 8 workgroups and a lane of the 512 x 512 layers walks 128 summaries:
// one L2 round trip each when every add waits for its own load (19.5 us).  kFin1Batch loads are
// issued before their adds instead - the order of the adds, and with it every bit of the
// result, is that of the plain loop.
constexpr int kFin1Batch = 16;
__global__ __launch_bounds__(32 * FL) void in_bwd_finalize1_kernel(const float2* __restrict__ partial,
                                                               float2* __restrict__ coef,
                                                               float2* __restrict__ sums, int HW,
                                                               int C, int split) {
  // The tile summaries are merged in double: S1 and S2 are sums of signed terms (for the first
  // layers, of 2^18 pixels whose sum is far smaller than their magnitudes), and an fp32 running
  // sum over up to 4096 tiles was the largest rounding term of dgamma / dbeta (round 4: the
  // bs-8 = 4 x bs-2 test held encoder_stages.0's dbeta at 0.6-1.2e-4 of its maximum).
  __shared__ double sa[FL][33], sb[FL][33];
  const int cl = threadIdx.x & 31, l = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl, n = blockIdx.y;
  double da_ = 0.0, db_ = 0.0;
  if (c < C) {
    const float2* src = partial + (size_t)n * split * C + c;
    int s = l;
    for (; s + (kFin1Batch - 1) * FL < split; s += kFin1Batch * FL) {
      float2 v[kFin1Batch];
#pragma unroll
      for (int j = 0; j < kFin1Batch; ++j) v[j] = src[(size_t)(s + j * FL) * C];
#pragma unroll
      for (int j = 0; j < kFin1Batch; ++j) {
        da_ += (double)v[j].x;
        db_ += (double)v[j].y;
      }
    }
    for (; s < split; s += FL) {
      const float2 v = src[(size_t)s * C];
      da_ += (double)v.x;
      db_ += (double)v.y;
    }
  }
  sa[l][cl] = da_; sb[l][cl] = db_;
  __syncthreads();
  if (l == 0 && c < C) {
    da_ = 0.0; db_ = 0.0;
#pragma unroll 4
    for (int k = 0; k < FL; ++k) { da_ += sa[k][cl]; db_ += sb[k][cl]; }
    float a = (float)da_, b = (float)db_;
    const float inv = 1.f / (float)HW;
    coef[(size_t)n * C + c] = float2{a * inv, b * inv};
    sums[(size_t)n * C + c] = float2{a, b};
  }
}

// pass 2: dy = gamma*rstd*(gz - c1 - xhat*c2); per-block column sums of dy -> dbias slabs
template <typename TS>
__global__ __launch_bounds__(kThreads) void in_bwd_apply_kernel(
    const TS* ga /* may alias dy */, const TS* __restrict__ y, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ mask, float slope,
    const float2* __restrict__ coef, TS* dy, float* __restrict__ dbias_partial,
    int HW, int C, int split, const float2* __restrict__ sums, float* __restrict__ dgamma,
    float* __restrict__ dbeta, float* __restrict__ dbias) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // [groups][C]
  const int lpp = C >> 2;
  const int groups = kThreads / lpp;
  const int tid = threadIdx.x;
  const int grp = tid / lpp, c4 = tid - grp * lpp;
  const int n = blockIdx.y, s = blockIdx.x;
  // block (0, 0) also emits the layer's parameter gradients from `sums`
  if (sums && n == 0 && s == 0)
    in_bwd_param_grads(sums, coef, gamma, rstd, gridDim.y, HW, C, tid, kThreads, dgamma, dbeta,
                       dbias);
  const int per = (HW + split - 1) / split;
  const int p_begin = s * per;
  const int p_end = min(p_begin + per, HW);
  f32x4 sd = {0.f, 0.f, 0.f, 0.f};
  if (grp < groups) {
    const int c = c4 * 4;
    const f32x4 mu = *reinterpret_cast<const f32x4*>(mean + (size_t)n * C + c);
    const f32x4 rs = *reinterpret_cast<const f32x4*>(rstd + (size_t)n * C + c);
    const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + c);
    const f32x4 b = *reinterpret_cast<const f32x4*>(beta + c);
    f32x4 mk = {1.f, 1.f, 1.f, 1.f};
    if (mask) mk = *reinterpret_cast<const f32x4*>(mask + (size_t)n * C + c);
    f32x4 c1, c2;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float2 cf = coef[(size_t)n * C + c + k];
      c1[k] = cf.x;
      c2[k] = cf.y;
    }
    const f32x4 al = g * rs, be = in_bwd_shift(b, mu, al);   // z: same expression as the forward
    const size_t base = (size_t)n * HW * C + c;
    for (int pp = p_begin + grp; pp < p_end; pp += groups) {
      const f32x4 yv = ld4(y + base + (size_t)pp * C);
      const f32x4 gv = ld4(ga + base + (size_t)pp * C);
      const f32x4 o = in_bwd_dz4(gv, yv, mu, rs, al, be, mk, slope, c1, c2);
      sd += o;
      st4(dy + base + (size_t)pp * C, o);
    }
  }
  if (dbias_partial) {
    if (grp < groups) *reinterpret_cast<f32x4*>(smem + grp * C + c4 * 4) = sd;
    __syncthreads();
    for (int c = tid; c < C; c += kThreads) {
      float a = 0.f;
      for (int g = 0; g < groups; ++g) a += smem[g * C + c];
      dbias_partial[((size_t)n * split + s) * C + c] = a;
    }
  }
}

bool shape_ok(int N, int HW, int C) {
  return N > 0 && HW > 0 && C >= 4 && C % 4 == 0 && C <= 1024 && (kThreads % (C / 4) == 0 || C / 4 > kThreads);
}

// Per-block slabs, then the backward's pair.  RESERVED behind them (once dbias slabs and their
// stage; no kernel reads them): sizes are pinned, unet_conv_in_fwd_workspace_bytes maxes with it.
struct InWs { float2* partial; InBwdPair pair; size_t bytes; };
InWs in_ws(void* base, int N, int HW, int C) {
  constexpr size_t kColsumChunks = 32;
  const size_t slabs = (size_t)N * split_for(N, HW, C) * C;
  WsLayout l(base);
  InWs w{l.take<float2>(slabs, 256), in_bwd_pair(l, N, C), 0};
  l.take<float>(slabs, 256), l.take<float>(kColsumChunks * C, 256);   // reserved
  w.bytes = l.bytes();
  return w;
}

}  // namespace

extern "C" size_t unet_instnorm_workspace_bytes(int N, int HW, int C) {
  if (N <= 0 || HW <= 0 || C <= 0) return 0;
  return in_ws(nullptr, N, HW, C).bytes;
}

extern "C" int unet_instnorm_stats(const float* y, const float* gamma, const float* beta, float eps,
                                   float* mean, float* rstd, float* alpha, float* beta2,
                                   void* workspace, size_t workspace_bytes, int N, int HW, int C,
                                   unet_stream_t stream_) {
  return unet_in_stats_masked(y, gamma, beta, eps, nullptr, mean, rstd, alpha, beta2, workspace,
                              workspace_bytes, N, HW, C, (hipStream_t)stream_, 0);
}

// stand-alone statistics pass; `mask` folds the dropout factor into alpha / beta2
int unet_in_stats_masked(const float* y, const float* gamma, const float* beta, float eps,
                         const float* mask, float* mean, float* rstd, float* alpha, float* beta2,
                         void* workspace, size_t workspace_bytes, int N, int HW, int C,
                         hipStream_t stream, int y_is_bf16) {
  UNET_REQUIRE(y && mean && rstd && workspace, "instnorm_stats: null pointer");
  UNET_REQUIRE(shape_ok(N, HW, C) && C <= 1024 && kThreads % (C / 4) == 0,
               "instnorm_stats: unsupported shape N=%d HW=%d C=%d", N, HW, C);
  const InWs ws = in_ws(workspace, N, HW, C);
  UNET_REQUIRE_WS(workspace_bytes, ws.bytes, "instnorm_stats: workspace too small");
  const int split = split_for(N, HW, C);
  const int groups = kThreads / (C / 4);
  float2* const partial = ws.partial;
  const size_t lds = (size_t)groups * (C / 4 + 2 * C) * sizeof(float);
  if (y_is_bf16)
    hipLaunchKernelGGL(in_stats_kernel<__bf16>, dim3(split, N), dim3(kThreads), lds, stream,
                       reinterpret_cast<const __bf16*>(y), partial, HW, C, split);
  else
    hipLaunchKernelGGL(in_stats_kernel<float>, dim3(split, N), dim3(kThreads), lds, stream, y,
                       partial, HW, C, split);
  UNET_CHECK_LAUNCH("in_stats");
  hipLaunchKernelGGL(in_stats_finalize_kernel, dim3(ceil_div(C, 32), N), dim3(32 * FL), 0, stream,
                     partial, gamma, beta, eps, mask, mean, rstd, alpha, beta2, N, HW, C, split);
  UNET_CHECK_LAUNCH("in_stats_finalize");
  return UNET_OK;
}

// Finalize per-tile (mean, M2) summaries written by a convolution's statistics epilogue:
// partial[(n * tiles + t) * C + c], every tile holding px_per_tile pixels of image n.
int unet_in_finalize_tiles(const void* partial, int tiles, int px_per_tile, const float* gamma,
                           const float* beta, float eps, const float* mask, float* mean,
                           float* rstd, float* alpha, float* beta2, int N, int HW, int C,
                           hipStream_t stream, void* grp_scratch) {
  UNET_REQUIRE(partial && mean && rstd && tiles > 0 && tiles * px_per_tile == HW,
               "in_finalize_tiles: %d tiles of %d pixels do not cover %d", tiles, px_per_tile, HW);
  if (tiles >= 512 && grp_scratch) {   // few blocks otherwise: two-level merge
    float2* grp = reinterpret_cast<float2*>(grp_scratch);
    hipLaunchKernelGGL(in_stats_finalize_grp_kernel, dim3(ceil_div(C, 32), N, kFinGroups),
                       dim3(32 * FL), 0, stream, reinterpret_cast<const float2*>(partial), grp, C,
                       tiles, (float)px_per_tile);
    UNET_CHECK_LAUNCH("in_stats_finalize(groups)");
    hipLaunchKernelGGL(in_stats_finalize_comb_kernel, dim3(ceil_div(N * C, 4)), dim3(256), 0,
                       stream, reinterpret_cast<const float2*>(partial), grp, gamma, beta, eps, mask,
                       mean, rstd, alpha, beta2, N, HW, C, tiles, (float)px_per_tile);
    UNET_CHECK_LAUNCH("in_stats_finalize(combine)");
    return UNET_OK;
  }
  hipLaunchKernelGGL(in_stats_finalize_eq_kernel, dim3(ceil_div(C, 32), N), dim3(32 * FL), 0,
                     stream, reinterpret_cast<const float2*>(partial), gamma, beta, eps, mask, mean,
                     rstd, alpha, beta2, HW, C, tiles, (float)px_per_tile);
  UNET_CHECK_LAUNCH("in_stats_finalize(tiles)");
  return UNET_OK;
}

// Merge of the per-tile (S1, S2) summaries a producer of dL/da left (`tiles` per image), for
// the callers that form dz themselves as well (head.hip, conv_wgrad.hip)
extern "C" int unet_instnorm_bwd_merge_partials(const void* partial, int tiles, void* coef,
                                                void* sums, int N, int HW, int C,
                                                unet_stream_t stream) {
  UNET_REQUIRE(partial && coef && sums && tiles > 0 && N > 0 && HW > 0 && C > 0,
               "instnorm_bwd_merge_partials: bad arguments");
  hipLaunchKernelGGL(in_bwd_finalize1_kernel, dim3(ceil_div(C, 32), N), dim3(32 * FL), 0,
                     (hipStream_t)stream, reinterpret_cast<const float2*>(partial),
                     reinterpret_cast<float2*>(coef), reinterpret_cast<float2*>(sums), HW, C, tiles);
  UNET_CHECK_LAUNCH("in_bwd_finalize1");
  return UNET_OK;
}

extern "C" int unet_instnorm_lrelu_drop_fwd(const float* y, const float* alpha, const float* beta2,
                                            const float* mask, float slope, float* a, int N, int HW,
                                            int C, unet_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  UNET_REQUIRE(y && alpha && beta2 && a, "instnorm_lrelu_drop_fwd: null pointer");
  UNET_REQUIRE(N > 0 && HW > 0 && C > 0 && C % 4 == 0, "instnorm_lrelu_drop_fwd: bad shape");
  const long long total4 = (long long)N * HW * (C / 4);
  long long blocks = ceil_div64(total4, kThreads);
  if (blocks > 256 * 16) blocks = 256 * 16;
  hipLaunchKernelGGL(in_apply_fwd_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, stream, y,
                     alpha, beta2, mask, slope, a, total4, HW, C);
  UNET_CHECK_LAUNCH("in_apply_fwd");
  return UNET_OK;
}

template <typename TS>
static int instnorm_bwd_impl(const TS* ga, const TS* y, const float* mean, const float* rstd,
                             const float* gamma, const float* beta, const float* mask, float slope,
                             TS* dy, float* dgamma, float* dbeta, float* dbias, void* workspace,
                             size_t workspace_bytes, int N, int HW, int C, hipStream_t stream,
                             const float2* ext_partial = nullptr, int ext_tiles = 0) {
  UNET_REQUIRE(ga && y && mean && rstd && gamma && beta && dy && workspace,
               "instnorm_lrelu_drop_bwd: null pointer");
  UNET_REQUIRE(shape_ok(N, HW, C) && kThreads % (C / 4) == 0,
               "instnorm_lrelu_drop_bwd: unsupported shape N=%d HW=%d C=%d", N, HW, C);
  const InWs ws = in_ws(workspace, N, HW, C);
  UNET_REQUIRE_WS(workspace_bytes, ws.bytes, "instnorm_lrelu_drop_bwd: workspace too small");
  const int split = split_for(N, HW, C);
  const int groups = kThreads / (C / 4);
  float2 *const partial = ws.partial, *const coef = ws.pair.coef, *const sums = ws.pair.sums;
  const size_t lds2 = (size_t)groups * 2 * C * sizeof(float);
  if (ext_partial) {   // the producer of ga already summarised the reductions per tile
    hipLaunchKernelGGL(in_bwd_finalize1_kernel, dim3(ceil_div(C, 32), N), dim3(32 * FL), 0, stream,
                       ext_partial, coef, sums, HW, C, ext_tiles);
  } else {
    hipLaunchKernelGGL(in_bwd_reduce_kernel<TS>, dim3(split, N), dim3(kThreads), lds2, stream, ga,
                       y, mean, rstd, gamma, beta, mask, slope, partial, HW, C, split);
    UNET_CHECK_LAUNCH("in_bwd_reduce");
    hipLaunchKernelGGL(in_bwd_finalize1_kernel, dim3(ceil_div(C, 32), N), dim3(32 * FL), 0, stream,
                       partial, coef, sums, HW, C, split);
  }
  UNET_CHECK_LAUNCH("in_bwd_finalize1");
  const size_t lds1 = (size_t)groups * C * sizeof(float);
  // block (0, 0) of the apply launch also emits dgamma / dbeta / dbias from `sums`
  hipLaunchKernelGGL(in_bwd_apply_kernel<TS>, dim3(split, N), dim3(kThreads), lds1, stream, ga, y, mean,
                     rstd, gamma, beta, mask, slope, coef, dy, (float*)nullptr, HW, C, split, sums,
                     dgamma, dbeta, dbias);
  UNET_CHECK_LAUNCH("in_bwd_apply");
  return UNET_OK;
}

extern "C" int unet_instnorm_lrelu_drop_bwd_partials(const float* ga, const float* y,
                                                     const float* mean, const float* rstd,
                                                     const float* gamma, const float* beta,
                                                     const float* mask, float slope, float* dy,
                                                     float* dgamma, float* dbeta, float* dbias,
                                                     const void* partial, int tiles,
                                                     void* workspace, size_t workspace_bytes,
                                                     int N, int HW, int C, unet_stream_t stream) {
  UNET_REQUIRE(partial && tiles > 0, "instnorm_lrelu_drop_bwd_partials: no summaries");
  return instnorm_bwd_impl<float>(ga, y, mean, rstd, gamma, beta, mask, slope, dy, dgamma, dbeta,
                                  dbias, workspace, workspace_bytes, N, HW, C, (hipStream_t)stream,
                                  reinterpret_cast<const float2*>(partial), tiles);
}

extern "C" int unet_instnorm_lrelu_drop_bwd(const float* ga, const float* y, const float* mean,
                                            const float* rstd, const float* gamma,
                                            const float* beta, const float* mask, float slope,
                                            float* dy, float* dgamma, float* dbeta, float* dbias,
                                            void* workspace, size_t workspace_bytes, int N, int HW,
                                            int C, unet_stream_t stream_) {
  return instnorm_bwd_impl<float>(ga, y, mean, rstd, gamma, beta, mask, slope, dy, dgamma, dbeta,
                                  dbias, workspace, workspace_bytes, N, HW, C, (hipStream_t)stream_);
}

// bf16 storage (mixed-precision pipeline): ga, y, dy are bf16 tensors, the arithmetic is fp32
extern "C" int unet_instnorm_lrelu_drop_bwd_b16(const uint16_t* ga, const uint16_t* y,
                                                const float* mean, const float* rstd,
                                                const float* gamma, const float* beta,
                                                const float* mask, float slope, uint16_t* dy,
                                                float* dgamma, float* dbeta, float* dbias,
                                                void* workspace, size_t workspace_bytes, int N,
                                                int HW, int C, unet_stream_t stream_) {
  return instnorm_bwd_impl<__bf16>(reinterpret_cast<const __bf16*>(ga),
                                   reinterpret_cast<const __bf16*>(y), mean, rstd, gamma, beta,
                                   mask, slope, reinterpret_cast<__bf16*>(dy), dgamma, dbeta, dbias,
                                   workspace, workspace_bytes, N, HW, C, (hipStream_t)stream_);
}

extern "C" int unet_instnorm_lrelu_drop_bwd_partials_b16(
    const uint16_t* ga, const uint16_t* y, const float* mean, const float* rstd,
    const float* gamma, const float* beta, const float* mask, float slope, uint16_t* dy,
    float* dgamma, float* dbeta, float* dbias, const void* partial, int tiles, void* workspace,
    size_t workspace_bytes, int N, int HW, int C, unet_stream_t stream) {
  UNET_REQUIRE(partial && tiles > 0, "instnorm_lrelu_drop_bwd_partials_b16: no summaries");
  return instnorm_bwd_impl<__bf16>(reinterpret_cast<const __bf16*>(ga),
                                   reinterpret_cast<const __bf16*>(y), mean, rstd, gamma, beta,
                                   mask, slope, reinterpret_cast<__bf16*>(dy), dgamma, dbeta, dbias,
                                   workspace, workspace_bytes, N, HW, C, (hipStream_t)stream,
                                   reinterpret_cast<const float2*>(partial), tiles);
}
