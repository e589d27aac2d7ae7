// vit.hip — the frozen CLIP ViT image tower of CLIP_UNet (ClipPatchExtractor.forward,
// CLIP_UNet/models/unet.py:581-613, which calls clip_model.encode_image on every train step,
// CLIP_UNet/src/train.py:714-719).  Forward only.  The residual stream, LayerNorm statistics,
// softmax and every epilogue are fp32; GEMM and attention operands are bf16 on the matrix cores
// (v_mfma_f32_32x32x16_bf16) with fp32 accumulators.  No atomics: two runs are bit-identical.
//
//   patch gather   image (fp32 NCHW / uint8 NHWC, any size, resized on the fly) -> bf16 [N G^2, Kp]
//   GEMM           Y = A W^T with A [M,K], W [Nout,K] bf16, four epilogues
//   tokens + ln_pre, LayerNorm, attention (one launch for all (image, head) pairs), head
#include "common.h"

namespace {

constexpr int VIT_MAX_T = 257;    // tokens: a whole score row lives in registers
constexpr int VIT_MAX_D = 1024;   // width: a LayerNorm row lives in one wave's registers

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

unsigned stream_grid(long long items) {
  long long b = ceil_div64(items, 256);
  if (b > 256 * 16) b = 256 * 16;
  return b < 1 ? 1u : (unsigned)b;
}

// ------------------------------------------------------------------ patch gather
struct Norm3 { float mean[3], std[3]; };

// one pixel of channel c: the fp32 NCHW value as it is, or the uint8 NHWC value normalised as
// ToTensor + Normalize do ((v / 255 - mean) / std, every operation correctly rounded)
template <bool U8>
__device__ __forceinline__ float vit_px(const void* __restrict__ img, int n, int c, int y, int x,
                                        int H, int W, const Norm3& nm) {
  if (U8) {
    const unsigned char b =
        reinterpret_cast<const unsigned char*>(img)[(((size_t)n * H + y) * W + x) * 3 + c];
    return __fdiv_rn(__fsub_rn(__fdiv_rn((float)b, 255.f), nm.mean[c]), nm.std[c]);
  }
  return reinterpret_cast<const float*>(img)[(((size_t)n * 3 + c) * H + y) * W + x];
}

// out[(n G^2 + gy G + gx)][k], k = (c P + py) P + px (the order of conv1.weight.reshape(D, -1)),
// columns K .. Kp-1 zero.  H x W != R x R: F.interpolate(mode="bilinear", align_corners=False) of
// the (normalised) image, sampled here.
template <bool U8>
__global__ __launch_bounds__(256) void vit_patchify_kernel(const void* __restrict__ img,
                                                           __bf16* __restrict__ out,
                                                           long long total, int H, int W, int R,
                                                           int P, int G, int K, int Kp, float sh,
                                                           float sw, const Norm3 nm) {
  const bool same = H == R && W == R;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * 256) {
    const int k = (int)(idx % Kp);
    const long long row = idx / Kp;
    if (k >= K) {
      out[idx] = (__bf16)0.f;
      continue;
    }
    const int g = (int)(row % (G * G)), n = (int)(row / (G * G));
    const int gy = g / G, gx = g - gy * G;
    const int c = k / (P * P), rem = k - c * P * P;
    const int py = rem / P, px = rem - py * P;
    const int Y = gy * P + py, X = gx * P + px;
    float v;
    if (same) {
      v = vit_px<U8>(img, n, c, Y, X, H, W, nm);
    } else {
      int y0, y1, x0, x1;
      float ly, lx;
      bil_src(Y, sh, H, y0, y1, ly);
      bil_src(X, sw, W, x0, x1, lx);
      const float p00 = vit_px<U8>(img, n, c, y0, x0, H, W, nm);
      const float p01 = vit_px<U8>(img, n, c, y0, x1, H, W, nm);
      const float p10 = vit_px<U8>(img, n, c, y1, x0, H, W, nm);
      const float p11 = vit_px<U8>(img, n, c, y1, x1, H, W, nm);
      const float wx0 = 1.f - lx, wy0 = 1.f - ly;
      const float t0 = __builtin_fmaf(p01, lx, p00 * wx0);
      const float t1 = __builtin_fmaf(p11, lx, p10 * wx0);
      v = __builtin_fmaf(t1, ly, t0 * wy0);
    }
    out[idx] = (__bf16)v;
  }
}

// ------------------------------------------------------------------ LayerNorm
// One wave per row, the row in registers (D / 64 <= 16 values a lane): mean, then the variance of
// the centred values, both fp32.  MODE 0: fp32 row -> bf16 row.  MODE 1: token assembly + ln_pre:
// row (n, t) = (t == 0 ? cls : patches[n (T-1) + t-1]) + pos[t], normalised -> the fp32 stream.
template <int MODE>
__global__ __launch_bounds__(256) void vit_ln_kernel(const float* __restrict__ x,
                                                     const float* __restrict__ cls,
                                                     const float* __restrict__ pos,
                                                     const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, float eps,
                                                     void* __restrict__ out, long long rows, int D,
                                                     int T) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int cnt = D >> 6;
  const float* src;
  const float* add = nullptr;
  if (MODE == 1) {
    const long long n = row / T;
    const int t = (int)(row - n * T);
    src = t == 0 ? cls : x + ((size_t)n * (T - 1) + (t - 1)) * D;
    add = pos + (size_t)t * D;
  } else {
    src = x + (size_t)row * D;
  }
  float v[16];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    v[i] = 0.f;
    if (i < cnt) {
      float a = src[lane + 64 * i];
      if (MODE == 1) a += add[lane + 64 * i];
      v[i] = a;
      s += a;
    }
  }
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i)
    if (i < cnt) {
      const float d = v[i] - mean;
      q += d * d;
    }
  const float rstd = 1.f / sqrtf(wave_sum(q) / (float)D + eps);
#pragma unroll
  for (int i = 0; i < 16; ++i)
    if (i < cnt) {
      const int d = lane + 64 * i;
      const float y = (v[i] - mean) * rstd * gamma[d] + beta[d];
      if (MODE == 1) reinterpret_cast<float*>(out)[(size_t)row * D + d] = y;
      else reinterpret_cast<__bf16*>(out)[(size_t)row * D + d] = (__bf16)y;
    }
}

// ------------------------------------------------------------------ GEMM  Y = A W^T
// A [M,K], W [Nout,K] bf16, K contiguous in both: the 32x32x16 fragments of both operands (lane
// (r, h) holds row r, k = 8h .. 8h+7) are 16 contiguous bytes of a row.  BM x BN x 64 tiles, four
// waves as 2 x 2, one LDS buffer with the next tile's global loads in flight over the products.
// LDS rows are 72 elements (144 B): 16 consecutive rows at one k offset cover all 64 banks once.
// Rows >= M / >= Nout and 16-byte chunks at k >= K are zero-filled, never read (K % 16 == 0).
enum { EPI_F32 = 0, EPI_BIAS_B16 = 1, EPI_BIAS_GELU_B16 = 2, EPI_BIAS_RESID_F32 = 3 };

template <int BM, int BN, int EPI>
__global__ __launch_bounds__(256) void vit_gemm_kernel(const __bf16* __restrict__ A,
                                                       const __bf16* __restrict__ Wt,
                                                       const float* __restrict__ bias,
                                                       void* __restrict__ out, int M, int Nout,
                                                       int K) {
  constexpr int BK = 64, LD = 72;
  constexpr int TM = BM / 64, TN = BN / 64;          // 32 x 32 tiles of a wave
  constexpr int ACH = BM * 8 / 256, WCH = BN * 8 / 256;
  __shared__ __attribute__((aligned(16))) __bf16 As[BM * LD];
  __shared__ __attribute__((aligned(16))) __bf16 Ws[BN * LD];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;

  uint4 ra[ACH], rw[WCH];
  auto gload = [&](int k0) {
#pragma unroll
    for (int i = 0; i < ACH; ++i) {
      const int q = tid + 256 * i, row = q >> 3, kk = k0 + 8 * (q & 7);
      ra[i] = make_uint4(0, 0, 0, 0);
      if (m0 + row < M && kk < K)
        ra[i] = *reinterpret_cast<const uint4*>(A + (size_t)(m0 + row) * K + kk);
    }
#pragma unroll
    for (int i = 0; i < WCH; ++i) {
      const int q = tid + 256 * i, row = q >> 3, kk = k0 + 8 * (q & 7);
      rw[i] = make_uint4(0, 0, 0, 0);
      if (n0 + row < Nout && kk < K)
        rw[i] = *reinterpret_cast<const uint4*>(Wt + (size_t)(n0 + row) * K + kk);
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  gload(0);
  for (int k0 = 0; k0 < K; k0 += BK) {
#pragma unroll
    for (int i = 0; i < ACH; ++i) {
      const int q = tid + 256 * i;
      *reinterpret_cast<uint4*>(&As[(q >> 3) * LD + 8 * (q & 7)]) = ra[i];
    }
#pragma unroll
    for (int i = 0; i < WCH; ++i) {
      const int q = tid + 256 * i;
      *reinterpret_cast<uint4*>(&Ws[(q >> 3) * LD + 8 * (q & 7)]) = rw[i];
    }
    __syncthreads();
    if (k0 + BK < K) gload(k0 + BK);
#pragma unroll
    for (int ks = 0; ks < BK / 16; ++ks) {
      bf16x8 a[TM], b[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i)
        a[i] = *reinterpret_cast<const bf16x8*>(&As[(wm * (BM / 2) + i * 32 + r) * LD + ks * 16 + 8 * h]);
#pragma unroll
      for (int j = 0; j < TN; ++j)
        b[j] = *reinterpret_cast<const bf16x8*>(&Ws[(wn * (BN / 2) + j * 32 + r) * LD + ks * 16 + 8 * h]);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }

  // C layout: column = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = n0 + wn * (BN / 2) + j * 32 + r;
    if (col >= Nout) continue;
    const float bv = EPI == EPI_F32 ? 0.f : bias[col];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = m0 + wm * (BM / 2) + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (row >= M) continue;
        const size_t o = (size_t)row * Nout + col;
        const float y = acc[i][j][e] + bv;
        if (EPI == EPI_F32) {
          reinterpret_cast<float*>(out)[o] = acc[i][j][e];
        } else if (EPI == EPI_BIAS_B16) {
          reinterpret_cast<__bf16*>(out)[o] = (__bf16)y;
        } else if (EPI == EPI_BIAS_GELU_B16) {
          // QuickGELU: x sigmoid(1.702 x)
          reinterpret_cast<__bf16*>(out)[o] = (__bf16)(y / (1.f + __expf(-1.702f * y)));
        } else {
          float* s = reinterpret_cast<float*>(out) + o;
          *s = *s + y;
        }
      }
    }
  }
}

template <int BM, int BN>
void vit_gemm_launch(int epi, dim3 grid, hipStream_t st, const __bf16* A, const __bf16* W,
                     const float* bias, void* out, int M, int Nout, int K) {
  switch (epi) {
    case EPI_F32:
      hipLaunchKernelGGL((vit_gemm_kernel<BM, BN, EPI_F32>), grid, dim3(256), 0, st, A, W, bias,
                         out, M, Nout, K);
      break;
    case EPI_BIAS_B16:
      hipLaunchKernelGGL((vit_gemm_kernel<BM, BN, EPI_BIAS_B16>), grid, dim3(256), 0, st, A, W,
                         bias, out, M, Nout, K);
      break;
    case EPI_BIAS_GELU_B16:
      hipLaunchKernelGGL((vit_gemm_kernel<BM, BN, EPI_BIAS_GELU_B16>), grid, dim3(256), 0, st, A,
                         W, bias, out, M, Nout, K);
      break;
    default:
      hipLaunchKernelGGL((vit_gemm_kernel<BM, BN, EPI_BIAS_RESID_F32>), grid, dim3(256), 0, st, A,
                         W, bias, out, M, Nout, K);
      break;
  }
}

// ------------------------------------------------------------------ attention
// One workgroup = one (image, head) pair and 128 queries (32 a wave).  The head's K [Tp][64] and
// V^T [64][Tp] (Tp = 32 NKT >= T) sit in LDS, zero beyond T.
//   S^T = K Q^T (A = K rows, B = Q rows straight from global memory): a lane holds ITS query's
//   scores against 16 keys of every 32-key tile - the whole row is in the registers of lanes
//   r and r + 32, so the softmax is plain: mask, max, exp, sum (fp32), one exchange each.
//   O^T = V^T P^T: the score tile is the B operand as it lies (registers 8s .. 8s+7 -> bf16 are
//   k-step s; element j of lane half h is key 16s + 8 (j >> 2) + 4h + (j & 3)), so the A operand
//   takes V^T's keys in that order: two 8-byte reads of a V^T row.
// V^T rows are Tp + 4 elements: the row stride in dwords is 2 x odd, so the 32 rows a half-wave
// reads at one key offset fall on 32 distinct bank pairs.
template <int NKT>
__global__ __launch_bounds__(256) void vit_attn_kernel(const __bf16* __restrict__ qkv,
                                                       __bf16* __restrict__ out, int T, int D,
                                                       int heads) {
  constexpr int TP = 32 * NKT, KLD = 72, VLD = TP + 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char vit_smem[];
  __bf16* Ks = reinterpret_cast<__bf16*>(vit_smem);   // [TP][KLD]
  __bf16* Vt = Ks + TP * KLD;                         // [64][VLD]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int n = blockIdx.y / heads, hd = blockIdx.y - n * heads;
  const size_t ld = 3 * (size_t)D;
  const __bf16* base = qkv + (size_t)n * T * ld + 64 * hd;

  for (int q = tid; q < TP * 8; q += 256) {
    const int t = q >> 3, c = q & 7;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (t < T) v = *reinterpret_cast<const uint4*>(base + (size_t)t * ld + D + 8 * c);
    *reinterpret_cast<uint4*>(&Ks[t * KLD + 8 * c]) = v;
  }
  for (int q = tid; q < TP * 4; q += 256) {
    const int t0 = 2 * (q >> 3), c = q & 7;
    uint4 v0 = make_uint4(0, 0, 0, 0), v1 = make_uint4(0, 0, 0, 0);
    if (t0 < T) v0 = *reinterpret_cast<const uint4*>(base + (size_t)t0 * ld + 2 * D + 8 * c);
    if (t0 + 1 < T) v1 = *reinterpret_cast<const uint4*>(base + (size_t)(t0 + 1) * ld + 2 * D + 8 * c);
    const unsigned w0[4] = {v0.x, v0.y, v0.z, v0.w}, w1[4] = {v1.x, v1.y, v1.z, v1.w};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const unsigned lo = (w0[i >> 1] >> (16 * (i & 1))) & 0xffffu;
      const unsigned hi = (w1[i >> 1] >> (16 * (i & 1))) & 0xffffu;
      *reinterpret_cast<unsigned*>(&Vt[(8 * c + i) * VLD + t0]) = lo | (hi << 16);
    }
  }
  __syncthreads();

  const int q0 = blockIdx.x * 128 + wave * 32;
  if (q0 >= T) return;                       // (no barrier follows)
  const int qi = q0 + r, qc = qi < T ? qi : T - 1;
  bf16x8 bq[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)
    bq[ks] = *reinterpret_cast<const bf16x8*>(base + (size_t)qc * ld + ks * 16 + 8 * h);

  f32x16 s[NKT];
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const bf16x8 a = *reinterpret_cast<const bf16x8*>(&Ks[(kt * 32 + r) * KLD + ks * 16 + 8 * h]);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bq[ks], acc, 0, 0, 0);
    }
    s[kt] = acc;
  }
  // S / 8, keys >= T masked before the maximum
  float mx = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int key = kt * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
      const float v = key < T ? s[kt][e] * 0.125f : -INFINITY;
      s[kt][e] = v;
      mx = fmaxf(mx, v);
    }
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  float sum = 0.f;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float p = __expf(s[kt][e] - mx);
      s[kt][e] = p;
      sum += p;
    }
  sum += __shfl_xor(sum, 32, 64);

  f32x16 o[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[dt][e] = 0.f;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int sI = 0; sI < 2; ++sI) {
      bf16x8 pb;
#pragma unroll
      for (int j = 0; j < 8; ++j) pb[j] = (__bf16)s[kt][8 * sI + j];
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        const __bf16* vp = &Vt[(dt * 32 + r) * VLD + kt * 32 + 16 * sI + 4 * h];
        const bf16x4 lo = *reinterpret_cast<const bf16x4*>(vp);
        const bf16x4 hi = *reinterpret_cast<const bf16x4*>(vp + 8);
        const bf16x8 a = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, pb, o[dt], 0, 0, 0);
      }
    }
  if (qi >= T) return;
  const float inv = 1.f / sum;
  __bf16* dst = out + ((size_t)n * T + qi) * D + 64 * hd;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      st4(dst + dt * 32 + 8 * g + 4 * h, f32x4{o[dt][4 * g] * inv, o[dt][4 * g + 1] * inv,
                                              o[dt][4 * g + 2] * inv, o[dt][4 * g + 3] * inv});
}

template <int NKT>
int vit_attn_launch(const __bf16* qkv, __bf16* out, int N, int T, int D, int heads,
                    hipStream_t st) {
  constexpr size_t lds = (size_t)32 * NKT * 72 * 2 + (size_t)64 * (32 * NKT + 4) * 2;
  UNET_SET_DYN_LDS((vit_attn_kernel<NKT>), lds);
  hipLaunchKernelGGL((vit_attn_kernel<NKT>), dim3(ceil_div(T, 128), N * heads), dim3(256), lds, st,
                     qkv, out, T, D, heads);
  return UNET_OK;
}

// ------------------------------------------------------------------ head
// ln_post of image n's class row, @ proj [D][E] (fp32), written as the [E][GG] planes of the
// extractor's output (bilinear interpolation from 1 x 1 is a copy).  One workgroup per image and
// 64 outputs; four partial sums a column, added in a fixed order.
__global__ __launch_bounds__(256) void vit_head_kernel(const float* __restrict__ x,
                                                       const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float eps,
                                                       const float* __restrict__ proj,
                                                       float* __restrict__ out, int T, int D,
                                                       int E, int GG) {
  __shared__ float xn[VIT_MAX_D];
  __shared__ float red[4];
  __shared__ float part[4][64];
  __shared__ float val[64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int n = blockIdx.y, e0 = blockIdx.x * 64;
  const float* row = x + (size_t)n * T * D;
  float s = 0.f;
  for (int d = tid; d < D; d += 256) s += row[d];
  s = wave_sum(s);
  if (lane == 0) red[wave] = s;
  __syncthreads();
  const float mean = (red[0] + red[1] + red[2] + red[3]) / (float)D;
  __syncthreads();
  float q = 0.f;
  for (int d = tid; d < D; d += 256) {
    const float c = row[d] - mean;
    q += c * c;
  }
  q = wave_sum(q);
  if (lane == 0) red[wave] = q;
  __syncthreads();
  const float rstd = 1.f / sqrtf((red[0] + red[1] + red[2] + red[3]) / (float)D + eps);
  for (int d = tid; d < D; d += 256) xn[d] = (row[d] - mean) * rstd * gamma[d] + beta[d];
  __syncthreads();
  const int e = e0 + lane;
  float acc = 0.f;
  if (e < E)
    for (int d = wave; d < D; d += 4) acc = __builtin_fmaf(xn[d], proj[(size_t)d * E + e], acc);
  part[wave][lane] = acc;
  __syncthreads();
  if (tid < 64) val[tid] = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
  __syncthreads();
  const int ne = E - e0 < 64 ? E - e0 : 64;
  float* dst = out + ((size_t)n * E + e0) * GG;
  for (int i = tid; i < ne * GG; i += 256) dst[i] = val[i / GG];
}

bool vit_width_ok(int D) { return D >= 64 && D % 64 == 0 && D <= VIT_MAX_D; }

}  // namespace

extern "C" int unet_vit_patchify(const void* image, int image_u8, const float* mean3,
                                 const float* std3, void* patches, int N, int H, int W, int R,
                                 int P, int Kp, unet_stream_t stream) {
  UNET_REQUIRE(image && patches, "vit_patchify: null pointer");
  UNET_REQUIRE(!image_u8 || (mean3 && std3), "vit_patchify: uint8 input needs mean3 / std3");
  UNET_REQUIRE(N > 0 && H > 0 && W > 0 && R > 0 && P > 0 && R % P == 0,
               "vit_patchify: bad shape (R %% P == 0)");
  UNET_REQUIRE(Kp >= 3 * P * P && Kp % 16 == 0 && Kp < 3 * P * P + 64,
               "vit_patchify: Kp must be 3 P^2 rounded up to a multiple of 16 or 64");
  UNET_REQUIRE((long long)N * H * W * 3 < (1ll << 40) && (long long)N * R * R < (1ll << 31),
               "vit_patchify: shape too large");
  const int G = R / P;
  Norm3 nm{};
  for (int c = 0; c < 3; ++c) {
    nm.mean[c] = image_u8 ? mean3[c] : 0.f;
    nm.std[c] = image_u8 ? std3[c] : 1.f;
  }
  const long long total = (long long)N * G * G * Kp;
  const float sh = (float)H / (float)R, sw = (float)W / (float)R;
  if (image_u8)
    hipLaunchKernelGGL(vit_patchify_kernel<true>, dim3(stream_grid(total)), dim3(256), 0,
                       (hipStream_t)stream, image, reinterpret_cast<__bf16*>(patches), total, H, W,
                       R, P, G, 3 * P * P, Kp, sh, sw, nm);
  else
    hipLaunchKernelGGL(vit_patchify_kernel<false>, dim3(stream_grid(total)), dim3(256), 0,
                       (hipStream_t)stream, image, reinterpret_cast<__bf16*>(patches), total, H, W,
                       R, P, G, 3 * P * P, Kp, sh, sw, nm);
  UNET_CHECK_LAUNCH("vit_patchify");
  return UNET_OK;
}

extern "C" int unet_vit_gemm_bf16(const void* a, const void* w, const float* bias, void* out,
                                  int epilogue, int M, int Nout, int K, unet_stream_t stream) {
  UNET_REQUIRE(a && w && out, "vit_gemm_bf16: null pointer");
  UNET_REQUIRE(epilogue >= EPI_F32 && epilogue <= EPI_BIAS_RESID_F32,
               "vit_gemm_bf16: epilogue must be 0..3");
  UNET_REQUIRE(epilogue == EPI_F32 || bias, "vit_gemm_bf16: this epilogue needs a bias");
  UNET_REQUIRE(M > 0 && Nout > 0 && K > 0 && Nout % 64 == 0 && K % 16 == 0,
               "vit_gemm_bf16: bad shape (Nout %% 64 == 0, K %% 16 == 0)");
  UNET_REQUIRE((long long)M * Nout < (1ll << 31) && (long long)M * K < (1ll << 31) &&
                   (long long)Nout * K < (1ll << 31) && ceil_div(M, 64) < 65536,
               "vit_gemm_bf16: shape too large");
  const __bf16* A = reinterpret_cast<const __bf16*>(a);
  const __bf16* Wt = reinterpret_cast<const __bf16*>(w);
  hipStream_t st = (hipStream_t)stream;
  const long long rows128 = ceil_div(M, 128);
  if (rows128 * ceil_div(Nout, 128) >= 192)
    vit_gemm_launch<128, 128>(epilogue, dim3(ceil_div(Nout, 128), (unsigned)rows128), st, A, Wt,
                              bias, out, M, Nout, K);
  else if (rows128 * (Nout / 64) >= 128)
    vit_gemm_launch<128, 64>(epilogue, dim3(Nout / 64, (unsigned)rows128), st, A, Wt, bias, out, M,
                             Nout, K);
  else
    vit_gemm_launch<64, 64>(epilogue, dim3(Nout / 64, ceil_div(M, 64)), st, A, Wt, bias, out, M,
                            Nout, K);
  UNET_CHECK_LAUNCH("vit_gemm_bf16");
  return UNET_OK;
}

extern "C" int unet_vit_tokens_ln(const float* patches, const float* cls, const float* pos,
                                  const float* gamma, const float* beta, float eps, float* out,
                                  int N, int T, int D, unet_stream_t stream) {
  UNET_REQUIRE(patches && cls && pos && gamma && beta && out, "vit_tokens_ln: null pointer");
  UNET_REQUIRE(N > 0 && T >= 2 && T <= VIT_MAX_T, "vit_tokens_ln: bad shape (2 <= T <= 257)");
  UNET_REQUIRE(vit_width_ok(D), "vit_tokens_ln: D must be a multiple of 64, at most 1024");
  const long long rows = (long long)N * T;
  UNET_REQUIRE(rows * D < (1ll << 31), "vit_tokens_ln: shape too large");
  hipLaunchKernelGGL(vit_ln_kernel<1>, dim3((unsigned)ceil_div64(rows, 4)), dim3(256), 0,
                     (hipStream_t)stream, patches, cls, pos, gamma, beta, eps, (void*)out, rows, D,
                     T);
  UNET_CHECK_LAUNCH("vit_tokens_ln");
  return UNET_OK;
}

extern "C" int unet_vit_layernorm(const float* x, const float* gamma, const float* beta, float eps,
                                  void* out, int rows, int D, unet_stream_t stream) {
  UNET_REQUIRE(x && gamma && beta && out, "vit_layernorm: null pointer");
  UNET_REQUIRE(rows > 0, "vit_layernorm: bad shape");
  UNET_REQUIRE(vit_width_ok(D), "vit_layernorm: D must be a multiple of 64, at most 1024");
  UNET_REQUIRE((long long)rows * D < (1ll << 31), "vit_layernorm: shape too large");
  hipLaunchKernelGGL(vit_ln_kernel<0>, dim3((unsigned)ceil_div(rows, 4)), dim3(256), 0,
                     (hipStream_t)stream, x, (const float*)nullptr, (const float*)nullptr, gamma,
                     beta, eps, out, (long long)rows, D, 1);
  UNET_CHECK_LAUNCH("vit_layernorm");
  return UNET_OK;
}

extern "C" int unet_vit_attention(const void* qkv, void* out, int N, int T, int D, int heads,
                                  unet_stream_t stream) {
  UNET_REQUIRE(qkv && out, "vit_attention: null pointer");
  UNET_REQUIRE(N > 0 && T >= 1 && T <= VIT_MAX_T, "vit_attention: bad shape (1 <= T <= 257)");
  UNET_REQUIRE(D > 0 && D % 64 == 0, "vit_attention: D must be a multiple of 64");
  UNET_REQUIRE(heads > 0 && D == 64 * heads, "vit_attention: the head dimension must be 64");
  UNET_REQUIRE((long long)N * heads < 65536 && (long long)N * T * 3 * D < (1ll << 31),
               "vit_attention: shape too large");
  const __bf16* q = reinterpret_cast<const __bf16*>(qkv);
  __bf16* o = reinterpret_cast<__bf16*>(out);
  hipStream_t st = (hipStream_t)stream;
  const int nkt = ceil_div(T, 32);
  int rc;
  if (nkt <= 1) rc = vit_attn_launch<1>(q, o, N, T, D, heads, st);
  else if (nkt <= 2) rc = vit_attn_launch<2>(q, o, N, T, D, heads, st);
  else if (nkt <= 4) rc = vit_attn_launch<4>(q, o, N, T, D, heads, st);
  else if (nkt <= 7) rc = vit_attn_launch<7>(q, o, N, T, D, heads, st);
  else rc = vit_attn_launch<9>(q, o, N, T, D, heads, st);
  if (rc != UNET_OK) return rc;
  UNET_CHECK_LAUNCH("vit_attention");
  return UNET_OK;
}

extern "C" int unet_vit_head(const float* x, const float* gamma, const float* beta, float eps,
                             const float* proj, float* out, int N, int T, int D, int E, int grid,
                             unet_stream_t stream) {
  UNET_REQUIRE(x && gamma && beta && proj && out, "vit_head: null pointer");
  UNET_REQUIRE(N > 0 && N < 65536 && T >= 1 && T <= VIT_MAX_T && E > 0 && grid > 0 && grid <= 64,
               "vit_head: bad shape (T <= 257, grid <= 64)");
  UNET_REQUIRE(vit_width_ok(D), "vit_head: D must be a multiple of 64, at most 1024");
  UNET_REQUIRE((long long)N * E * grid * grid < (1ll << 31), "vit_head: shape too large");
  hipLaunchKernelGGL(vit_head_kernel, dim3(ceil_div(E, 64), N), dim3(256), 0, (hipStream_t)stream,
                     x, gamma, beta, eps, proj, out, T, D, E, grid * grid);
  UNET_CHECK_LAUNCH("vit_head");
  return UNET_OK;
}
