// latent.hip — the autoencoder's latent-space analysis (AE_pretrained/reconstruction/src/
// evaluate.py:380-440, utils/visualize.py:179-231) on the device, from the code matrix X [N][D]:
//
//   unet_latent_col_mean     mean[d] = sum_i X[i][d] / N
//   unet_latent_gram         G = (X - mean)(X - mean)^T on the fp32 matrix cores: only the tiles on
//                            or above the diagonal, split over D into slabs, the slabs summed in
//                            order and mirrored.  PCA (dual form) and t-SNE (every pairwise
//                            distance) both start from it.
//   unet_latent_gram_apply   Z = G Q for the 8-column block of the subspace iteration
//   unet_latent_project      V[c][d] = sum_i (X[i][d] - mean[d]) w[i][c]: the two components
//   unet_tsne_cond_p         scikit-learn's per-row binary search for the perplexity, one
//                            workgroup per row, the row's distances in LDS
//   unet_tsne_joint_p        P = (Pc + Pc^T) / max(sum, eps), floored at eps
//   unet_tsne_step           one gradient-descent iteration of the exact t-SNE, two launches
//   unet_latent_scatter      the scatter picture: one thread per pixel, integer blends
//
// Every sum has a fixed order (per-thread runs, wave butterflies, slabs in ascending order): no
// floating-point atomics, two runs are bit-identical.
#include <float.h>
#include <math.h>

#include "common.h"

namespace {

constexpr int LT_THREADS = 256;

bool lt_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- column sums: the mean and the projection ------------------------------------------------
// The rows are cut into slabs (about 2048 workgroups in all, at least 32 rows each); a thread
// owns four columns and walks its slab's rows in order; the slabs are summed in order.
int cs_rows_per_slab(int N, int D) {
  const int colblocks = ceil_div(D / 4, LT_THREADS);
  int s = ceil_div(2048, colblocks);
  const int most = ceil_div(N, 32);
  s = s < most ? s : most;
  s = s > 64 ? 64 : s;
  return ceil_div(N, s < 1 ? 1 : s);
}
int cs_slabs(int N, int D) { return ceil_div(N, cs_rows_per_slab(N, D)); }

// NW == 0: partial[s][0][d] = sum_i x[i][d];  NW == 2: partial[s][c][d] = sum_i (x - m) w[i][c]
template <int NW>
__global__ __launch_bounds__(LT_THREADS) void colsum_kernel(
    const float* __restrict__ x, const float* __restrict__ m, const float* __restrict__ w,
    float* __restrict__ partial, int N, int D, int per) {
  const int d4 = (blockIdx.x * LT_THREADS + threadIdx.x) * 4;
  if (d4 >= D) return;
  const int s = blockIdx.y;
  const int i0 = s * per, i1 = min(i0 + per, N);
  constexpr int NOUT = NW ? NW : 1;
  f32x4 acc[NOUT];
#pragma unroll
  for (int c = 0; c < NOUT; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 mv = {0.f, 0.f, 0.f, 0.f};
  if (NW) mv = ld4(m + d4);
  const float* xp = x + d4;
#pragma unroll 4
  for (int i = i0; i < i1; ++i) {
    const f32x4 v = ld4(xp + (size_t)i * D);
    if (NW) {
      const f32x4 c = v - mv;
#pragma unroll
      for (int k = 0; k < NOUT; ++k) {
        const float wk = w[(size_t)i * NW + k];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[k][e] = __builtin_fmaf(c[e], wk, acc[k][e]);
      }
    } else {
      acc[0] += v;
    }
  }
#pragma unroll
  for (int c = 0; c < NOUT; ++c) st4(partial + ((size_t)s * NOUT + c) * D + d4, acc[c]);
}

// out[c][d] = (sum over the slabs, ascending) / div
__global__ __launch_bounds__(LT_THREADS) void colsum_finalize_kernel(
    const float* __restrict__ partial, float* __restrict__ out, int D, int slabs, int nout,
    float div) {
  const int d4 = (blockIdx.x * LT_THREADS + threadIdx.x) * 4;
  if (d4 >= D) return;
  const int c = blockIdx.y;
  f32x4 a = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < slabs; ++s) a += ld4(partial + ((size_t)s * nout + c) * D + d4);
#pragma unroll
  for (int e = 0; e < 4; ++e) a[e] = __fdiv_rn(a[e], div);
  st4(out + (size_t)c * D + d4, a);
}

bool lt_shape_ok(int N, int D) {
  return N >= 2 && N <= 65536 && D >= 4 && D % 4 == 0 && D <= (1 << 28);
}

// ---- centred Gram on the fp32 matrix cores ---------------------------------------------------
// A workgroup (4 waves as 2 x 2, 64 x 64 outputs each = 2 x 2 v_mfma_f32_32x32x2_f32 tiles) owns
// one 128 x 128 tile (bi <= bj) of G and one slab of D.  Per 32-deep chunk the 128 x 32 pieces of
// the two row blocks go global -> registers (mean subtracted, rows past N and columns past the
// slab zeroed) -> LDS [row][36]; the loads of chunk k + 1 are issued before the products of chunk
// k.  A lane reads four consecutive k of its row per ds_read_b128 and feeds them to four MFMAs:
// within a group of eight k the halves of the wave take k = g8 + t and g8 + 4 + t at step t, the
// same permutation on both operands.  X is addressed with 64-bit row offsets from plain pointers:
// no buffer descriptor spans it.
constexpr int GR_T = 128, GR_BK = 32, GR_LD = 36;

struct GramPlan { int nb, tiles, chunks, per, slabs; };
GramPlan gram_plan(int N, int D) {
  GramPlan p;
  p.nb = ceil_div(N, GR_T);
  p.tiles = p.nb * (p.nb + 1) / 2;
  p.chunks = ceil_div(D, GR_BK);
  const int want = ceil_div(1024, p.tiles);      // about four workgroups per CU
  int most = p.chunks / 8;                       // a slab is at least 256 deep
  most = most < 1 ? 1 : most;
  const int s0 = want < most ? want : most;
  p.per = ceil_div(p.chunks, s0);
  p.slabs = ceil_div(p.chunks, p.per);
  return p;
}

__device__ __forceinline__ void gram_tile(int t, int nb, int& bi, int& bj) {
  bi = 0;
  while (t >= nb - bi) { t -= nb - bi; ++bi; }
  bj = bi + t;
}

__global__ __launch_bounds__(LT_THREADS) void gram_kernel(
    const float* __restrict__ x, const float* __restrict__ mean, float* __restrict__ partial,
    int N, int D, int nb, int per) {
  __shared__ __attribute__((aligned(16))) float sm[2 * GR_T * GR_LD];
  int bi, bj;
  gram_tile(blockIdx.x, nb, bi, bj);
  const bool diag = bi == bj;
  float* sa = sm;
  float* sb = sm + GR_T * GR_LD;
  const float* sbr = diag ? sa : sb;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int lr = tid >> 3, lq = (tid & 7) * 4;
  const int k_begin = blockIdx.y * per * GR_BK;
  const int k_end = min(D, k_begin + per * GR_BK);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

  f32x16 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

  f32x4 va[4], vb[4];
  auto fetch = [&](int k0) {
    const int k = k0 + lq;
    const bool kin = k < k_end;       // D and the slab bounds are multiples of 4: whole quads
    const f32x4 mv = kin ? ld4(mean + k) : zero;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ra = bi * GR_T + lr + 32 * i;
      va[i] = (kin && ra < N) ? ld4(x + (size_t)ra * D + k) - mv : zero;
      if (!diag) {
        const int rb = bj * GR_T + lr + 32 * i;
        vb[i] = (kin && rb < N) ? ld4(x + (size_t)rb * D + k) - mv : zero;
      }
    }
  };

  fetch(k_begin);
  for (int k0 = k_begin; k0 < k_end; k0 += GR_BK) {
    __syncthreads();                 // the previous chunk's fragment reads are done
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<f32x4*>(sa + (lr + 32 * i) * GR_LD + lq) = va[i];
      if (!diag) *reinterpret_cast<f32x4*>(sb + (lr + 32 * i) * GR_LD + lq) = vb[i];
    }
    __syncthreads();
    if (k0 + GR_BK < k_end) fetch(k0 + GR_BK);
    const float* pa = sa + (wr * 64 + (lane & 31)) * GR_LD + 4 * (lane >> 5);
    const float* pb = sbr + (wc * 64 + (lane & 31)) * GR_LD + 4 * (lane >> 5);
#pragma unroll
    for (int g = 0; g < GR_BK / 8; ++g) {
      f32x4 a[2], b[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        a[m] = *reinterpret_cast<const f32x4*>(pa + m * 32 * GR_LD + g * 8);
        b[m] = *reinterpret_cast<const f32x4*>(pb + m * 32 * GR_LD + g * 8);
      }
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int n = 0; n < 2; ++n)
            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m][t], b[n][t], acc[m][n], 0, 0, 0);
    }
  }

  // C/D map of the 32 x 32 forms: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  float* pt = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (GR_T * GR_T);
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wr * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const int col = wc * 64 + n * 32 + (lane & 31);
        pt[row * GR_T + col] = acc[m][n][r];
      }
}

// G[r][c] = sum over the slabs (ascending) of the tile's partials, for r <= c, and its mirror
__global__ __launch_bounds__(LT_THREADS) void gram_reduce_kernel(
    const float* __restrict__ partial, float* __restrict__ g, int N, int nb, int slabs) {
  int bi, bj;
  gram_tile(blockIdx.x, nb, bi, bj);
  const int idx = (blockIdx.y * LT_THREADS + threadIdx.x) * 4;
  const int row = idx / GR_T, col = idx % GR_T;
  const size_t tile = (size_t)GR_T * GR_T;
  const float* pt = partial + (size_t)blockIdx.x * tile + idx;
  f32x4 a = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < slabs; ++s) a += ld4(pt + (size_t)s * gridDim.x * tile);
  const int gr = bi * GR_T + row;
  if (gr >= N) return;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int gc = bj * GR_T + col + e;
    if (gc >= N || gc < gr) continue;
    g[(size_t)gr * N + gc] = a[e];
    if (gc != gr) g[(size_t)gc * N + gr] = a[e];
  }
}

// Z[i][0..7] = sum_j G[i][j] Q[j][0..7]: a wave per row, lanes across j, butterfly sums
__global__ __launch_bounds__(LT_THREADS) void gram_apply_kernel(
    const float* __restrict__ g, const float* __restrict__ q, float* __restrict__ z, int N) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  float a[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) a[c] = 0.f;
  const float* gr = g + (size_t)row * N;
  for (int j = lane; j < N; j += 64) {
    const float v = gr[j];
    const f32x4 q0 = ld4(q + (size_t)j * 8), q1 = ld4(q + (size_t)j * 8 + 4);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      a[c] = __builtin_fmaf(v, q0[c], a[c]);
      a[4 + c] = __builtin_fmaf(v, q1[c], a[4 + c]);
    }
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) a[c] = wave_sum(a[c]);
  if (lane == 0) {
    st4(z + (size_t)row * 8, f32x4{a[0], a[1], a[2], a[3]});
    st4(z + (size_t)row * 8 + 4, f32x4{a[4], a[5], a[6], a[7]});
  }
}

// ---- t-SNE ------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// the workgroup's sum of a double, in a fixed order, to every thread; red: 4 doubles of LDS
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
  v = wave_sum_f64(v);
  __syncthreads();                   // red may still be read from the previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// sklearn.manifold._utils._binary_search_perplexity for row i = blockIdx.x, on the row's squared
// distances max(G_ii + G_jj - 2 G_ij, 0) minus their off-diagonal minimum (the conditional
// distribution does not see the shift; exp does: distances of order 1e5 would underflow every
// term).  100 steps, tolerance 1e-5 on the entropy, beta from 1, doubled / halved while unbounded
// and bisected after; sums in fp64, exp in fp32.
__global__ __launch_bounds__(LT_THREADS) void tsne_cond_p_kernel(
    const float* __restrict__ g, const float* __restrict__ diag, float perplexity,
    float* __restrict__ pc, double* __restrict__ rowsum, int N) {
  extern __shared__ float sd[];
  __shared__ double red[4];
  __shared__ float smin[4];
  const int i = blockIdx.x, tid = threadIdx.x;
  const float gii = diag[i];
  const float* gr = g + (size_t)i * N;
  float mn = INFINITY;
  for (int j = tid; j < N; j += LT_THREADS) {
    float d = fmaxf((gii + diag[j]) - 2.f * gr[j], 0.f);
    if (j == i) d = 0.f; else mn = fminf(mn, d);
    sd[j] = d;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mn = fminf(mn, __shfl_xor(mn, off, 64));
  if ((tid & 63) == 0) smin[tid >> 6] = mn;
  __syncthreads();
  mn = fminf(fminf(smin[0], smin[1]), fminf(smin[2], smin[3]));
  for (int j = tid; j < N; j += LT_THREADS) sd[j] -= mn;      // a thread's own elements

  const double target = log((double)perplexity);
  double beta = 1.0, bmin = -INFINITY, bmax = INFINITY, S = 1.0;
  for (int step = 0; step < 100; ++step) {
    const float fb = (float)beta;
    double s = 0.0, sdp = 0.0;
    for (int j = tid; j < N; j += LT_THREADS)
      if (j != i) {
        const float p = expf(-sd[j] * fb);
        s += (double)p;
        sdp += (double)(sd[j] * p);
      }
    S = block_sum_f64(s, red);
    const double SD = block_sum_f64(sdp, red);
    if (S == 0.0) S = 1e-8;
    const double diff = log(S) + beta * (SD / S) - target;
    if (fabs(diff) <= 1e-5) break;
    if (diff > 0.0) {
      bmin = beta;
      beta = bmax == INFINITY ? beta * 2.0 : (beta + bmax) * 0.5;
    } else {
      bmax = beta;
      beta = bmin == -INFINITY ? beta * 0.5 : (beta + bmin) * 0.5;
    }
  }
  const float fb = (float)beta;
  double s = 0.0;
  for (int j = tid; j < N; j += LT_THREADS) {
    const float p = j == i ? 0.f : (float)((double)expf(-sd[j] * fb) / S);
    pc[(size_t)i * N + j] = p;
    s += (double)p;
  }
  s = block_sum_f64(s, red);
  if (tid == 0) rowsum[i] = s;
}

// rowsum[N] = 2 sum_i rowsum[i] = sum of Pc + Pc^T, one workgroup, a fixed order
__global__ __launch_bounds__(LT_THREADS) void tsne_total_kernel(double* __restrict__ rowsum, int N) {
  __shared__ double red[4];
  double s = 0.0;
  for (int j = threadIdx.x; j < N; j += LT_THREADS) s += rowsum[j];
  s = block_sum_f64(s, red);
  if (threadIdx.x == 0) rowsum[N] = 2.0 * s;
}

__global__ __launch_bounds__(LT_THREADS) void tsne_joint_p_kernel(
    const float* __restrict__ pc, const double* __restrict__ rowsum, float* __restrict__ p, int N) {
  const size_t idx = (size_t)blockIdx.x * LT_THREADS + threadIdx.x;
  if (idx >= (size_t)N * N) return;
  const int i = (int)(idx / N), j = (int)(idx - (size_t)i * N);
  const double total = fmax(rowsum[N], DBL_EPSILON);
  float v = 0.f;
  if (i != j)
    v = fmaxf((float)(((double)pc[idx] + (double)pc[(size_t)j * N + i]) / total),
              (float)DBL_EPSILON);
  p[idx] = v;
}

// state [N][6] = (y0, y1, update0, update1, gains0, gains1); rows [N][8] = the row sums below
constexpr int TS_ROWS = 8;       // rows per workgroup of the gradient pass (2 per wave)

// rows[i] = { sum_j eP q dy0, sum_j eP q dy1, sum_j q^2 dy0, sum_j q^2 dy1, sum_j q,
//             sum_j eP (log eP - log q), sum_j eP, 0 },  q = 1 / (1 + |y_i - y_j|^2), j != i
__global__ __launch_bounds__(LT_THREADS) void tsne_grad_kernel(
    const float* __restrict__ p, const float* __restrict__ state, float* __restrict__ rows,
    float exaggeration, int want_stats, int N) {
  extern __shared__ float2 sy[];
  for (int j = threadIdx.x; j < N; j += LT_THREADS)
    sy[j] = float2{state[(size_t)j * 6], state[(size_t)j * 6 + 1]};
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int rr = 0; rr < TS_ROWS / 4; ++rr) {
    const int i = blockIdx.x * TS_ROWS + wave * (TS_ROWS / 4) + rr;
    if (i >= N) break;               // wave-uniform
    const float2 yi = sy[i];
    const float* pr = p + (size_t)i * N;
    float ax = 0.f, ay = 0.f, rx = 0.f, ry = 0.f, z = 0.f;
    double ka = 0.0, sp = 0.0;      // the error terms in fp64: the sums nearly cancel in the KL
    for (int j = lane; j < N; j += 64) {
      if (j == i) continue;
      const float pij = pr[j] * exaggeration;
      const float2 yj = sy[j];
      const float dx = yi.x - yj.x, dy = yi.y - yj.y;
      const float d1 = 1.f + (dx * dx + dy * dy);
      const float q = __fdiv_rn(1.f, d1);
      const float pq = pij * q, q2 = q * q;
      ax += pq * dx;
      ay += pq * dy;
      rx += q2 * dx;
      ry += q2 * dy;
      z += q;
      if (want_stats) {
        ka += (double)pij * (log((double)pij) + log((double)d1));
        sp += (double)pij;
      }
    }
    ax = wave_sum(ax); ay = wave_sum(ay); rx = wave_sum(rx); ry = wave_sum(ry);
    z = wave_sum(z);
    if (want_stats) { ka = wave_sum_f64(ka); sp = wave_sum_f64(sp); }
    if (lane == 0) {
      st4(rows + (size_t)i * 8, f32x4{ax, ay, rx, ry});
      st4(rows + (size_t)i * 8 + 4, f32x4{z, (float)ka, (float)sp, 0.f});
    }
  }
}

// one element of sklearn's _gradient_descent: the gradient, the new gain and the new update
__device__ __forceinline__ void tsne_element(float first, float second, float zinv, float u,
                                             float gain, float momentum, float lr, float& grad,
                                             float& gain_out, float& u_out) {
#pragma clang fp contract(off)
  grad = 4.f * (first - second * zinv);
  const bool inc = (u < 0.f && grad > 0.f) || (u > 0.f && grad < 0.f);   // update * grad < 0
  gain_out = fmaxf(inc ? gain + 0.2f : gain * 0.8f, 0.01f);
  u_out = momentum * u - lr * (gain_out * grad);
}

// Z = sum_i rows[i][4] (every workgroup, the same order), then the descent step of the
// workgroup's rows from state_in to state_out; with want_stats workgroup 0 also leaves
// stats = { KL = sum eP log(eP / Q), |gains * grad| } (the norm _gradient_descent tests).
__global__ __launch_bounds__(LT_THREADS) void tsne_update_kernel(
    const float* __restrict__ rows, const float* __restrict__ state_in,
    float* __restrict__ state_out, double* __restrict__ stats, float momentum, float lr,
    int want_stats, int N) {
  __shared__ double red[4];
  double zs = 0.0;
  for (int j = threadIdx.x; j < N; j += LT_THREADS) zs += (double)rows[(size_t)j * 8 + 4];
  const double Z = block_sum_f64(zs, red);
  const float zinv = (float)(1.0 / Z);
  const int i = blockIdx.x * LT_THREADS + threadIdx.x;
  if (i < N) {
    const float* r = rows + (size_t)i * 8;
    const float* si = state_in + (size_t)i * 6;
    float* so = state_out + (size_t)i * 6;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      float grad, gain, u;
      tsne_element(r[c], r[2 + c], zinv, si[2 + c], si[4 + c], momentum, lr, grad, gain, u);
      so[c] = si[c] + u;
      so[2 + c] = u;
      so[4 + c] = gain;
    }
  }
  if (want_stats && blockIdx.x == 0) {
    double ss = 0.0, ka = 0.0, sp = 0.0;
    for (int j = threadIdx.x; j < N; j += LT_THREADS) {
      const float* r = rows + (size_t)j * 8;
      const float* si = state_in + (size_t)j * 6;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        float grad, gain, u;
        tsne_element(r[c], r[2 + c], zinv, si[2 + c], si[4 + c], momentum, lr, grad, gain, u);
        const double gg = (double)gain * (double)grad;
        ss += gg * gg;
      }
      ka += (double)r[5];
      sp += (double)r[6];
    }
    ss = block_sum_f64(ss, red);
    ka = block_sum_f64(ka, red);
    sp = block_sum_f64(sp, red);
    if (threadIdx.x == 0) {
      stats[0] = ka + log(Z) * sp;
      stats[1] = sqrt(ss);
    }
  }
}

// ---- scatter picture ---------------------------------------------------------------------------
// One thread per pixel of a 16 x 16 block; the points go through LDS 256 at a time, in index
// order; a point covers the pixel where dx^2 + dy^2 <= r^2; each covering point blends
// dst = (dst * 77 + src * 179 + 128) >> 8 per channel over the white ground.
__global__ __launch_bounds__(LT_THREADS) void scatter_kernel(
    const int* __restrict__ centres, const uint8_t* __restrict__ labels,
    const uint8_t* __restrict__ palette, int K, uint8_t* __restrict__ out, int N, int H, int W,
    int radius) {
  __shared__ int sx[LT_THREADS], sy[LT_THREADS];
  __shared__ unsigned sc[LT_THREADS];
  const int tid = threadIdx.y * 16 + threadIdx.x;
  const int px = blockIdx.x * 16 + threadIdx.x, py = blockIdx.y * 16 + threadIdx.y;
  const int r2 = radius * radius;
  unsigned cr = 255, cg = 255, cb = 255;
  for (int base = 0; base < N; base += LT_THREADS) {
    const int n = base + tid;
    __syncthreads();
    if (n < N) {
      const int l = labels[n];
      sx[tid] = centres[2 * n];
      sy[tid] = centres[2 * n + 1];
      // a label outside the palette is refused by the caller; here it draws nothing
      sc[tid] = l < K ? (0x1000000u | palette[3 * l] | (palette[3 * l + 1] << 8) |
                         (palette[3 * l + 2] << 16)) : 0u;
    }
    __syncthreads();
    const int cnt = min(LT_THREADS, N - base);
    for (int k = 0; k < cnt; ++k) {
      const int dx = px - sx[k], dy = py - sy[k];
      const unsigned c = sc[k];
      if (!c || dx > radius || dx < -radius || dy > radius || dy < -radius) continue;
      if (dx * dx + dy * dy > r2) continue;
      cr = (cr * 77u + (c & 255u) * 179u + 128u) >> 8;
      cg = (cg * 77u + ((c >> 8) & 255u) * 179u + 128u) >> 8;
      cb = (cb * 77u + ((c >> 16) & 255u) * 179u + 128u) >> 8;
    }
  }
  if (px < W && py < H) {
    uint8_t* o = out + ((size_t)py * W + px) * 3;
    o[0] = (uint8_t)cr; o[1] = (uint8_t)cg; o[2] = (uint8_t)cb;
  }
}

constexpr int TSNE_MAX_N = 8192;

}  // namespace

extern "C" size_t unet_latent_colsum_workspace_bytes(int N, int D) {
  if (!lt_shape_ok(N, D)) return 0;
  return align_up((size_t)cs_slabs(N, D) * 2 * D * sizeof(float), 256);
}

static int latent_colsum(const char* name, const float* x, const float* mean, const float* w,
                         float* out, void* workspace, size_t workspace_bytes, int N, int D,
                         hipStream_t stream) {
  UNET_REQUIRE(x && out && workspace && (!w || mean), "%s: null pointer", name);
  UNET_REQUIRE(lt_shape_ok(N, D), "%s: bad shape N=%d D=%d (N in 2..65536, D a multiple of 4)",
               name, N, D);
  UNET_REQUIRE(lt_aligned(x) && lt_aligned(mean) && lt_aligned(out) && lt_aligned(workspace),
               "%s: pointers must be 16-byte aligned", name);
  UNET_REQUIRE_WS(workspace_bytes, unet_latent_colsum_workspace_bytes(N, D),
                  "%s: workspace too small", name);
  const int per = cs_rows_per_slab(N, D), slabs = cs_slabs(N, D);
  const int colblocks = ceil_div(D / 4, LT_THREADS);
  float* partial = reinterpret_cast<float*>(workspace);
  if (w)
    hipLaunchKernelGGL(colsum_kernel<2>, dim3(colblocks, slabs), dim3(LT_THREADS), 0, stream, x,
                       mean, w, partial, N, D, per);
  else
    hipLaunchKernelGGL(colsum_kernel<0>, dim3(colblocks, slabs), dim3(LT_THREADS), 0, stream, x,
                       mean, w, partial, N, D, per);
  UNET_CHECK_LAUNCH(name);
  hipLaunchKernelGGL(colsum_finalize_kernel, dim3(colblocks, w ? 2 : 1), dim3(LT_THREADS), 0,
                     stream, partial, out, D, slabs, w ? 2 : 1, w ? 1.f : (float)N);
  UNET_CHECK_LAUNCH(name);
  return UNET_OK;
}

extern "C" int unet_latent_col_mean(const float* x, float* mean, void* workspace,
                                    size_t workspace_bytes, int N, int D, unet_stream_t stream) {
  return latent_colsum("latent_col_mean", x, nullptr, nullptr, mean, workspace, workspace_bytes,
                       N, D, (hipStream_t)stream);
}

extern "C" int unet_latent_project(const float* x, const float* mean, const float* w, float* out,
                                   void* workspace, size_t workspace_bytes, int N, int D,
                                   unet_stream_t stream) {
  UNET_REQUIRE(w && mean, "latent_project: null pointer");
  return latent_colsum("latent_project", x, mean, w, out, workspace, workspace_bytes, N, D,
                       (hipStream_t)stream);
}

extern "C" size_t unet_latent_gram_workspace_bytes(int N, int D) {
  if (!lt_shape_ok(N, D)) return 0;
  const GramPlan p = gram_plan(N, D);
  return (size_t)p.slabs * p.tiles * GR_T * GR_T * sizeof(float);
}

extern "C" int unet_latent_gram_splitk(int N, int D) {
  return lt_shape_ok(N, D) ? gram_plan(N, D).slabs : 0;
}

extern "C" int unet_latent_gram(const float* x, const float* mean, float* g, void* workspace,
                                size_t workspace_bytes, int N, int D, unet_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  UNET_REQUIRE(x && mean && g && workspace, "latent_gram: null pointer");
  UNET_REQUIRE(lt_shape_ok(N, D),
               "latent_gram: bad shape N=%d D=%d (N in 2..65536, D a multiple of 4)", N, D);
  UNET_REQUIRE(lt_aligned(x) && lt_aligned(mean) && lt_aligned(workspace),
               "latent_gram: pointers must be 16-byte aligned");
  UNET_REQUIRE_WS(workspace_bytes, unet_latent_gram_workspace_bytes(N, D),
                  "latent_gram: workspace too small");
  const GramPlan p = gram_plan(N, D);
  float* partial = reinterpret_cast<float*>(workspace);
  hipLaunchKernelGGL(gram_kernel, dim3(p.tiles, p.slabs), dim3(LT_THREADS), 0, stream, x, mean,
                     partial, N, D, p.nb, p.per);
  UNET_CHECK_LAUNCH("latent_gram");
  hipLaunchKernelGGL(gram_reduce_kernel, dim3(p.tiles, GR_T * GR_T / (4 * LT_THREADS)),
                     dim3(LT_THREADS), 0, stream, partial, g, N, p.nb, p.slabs);
  UNET_CHECK_LAUNCH("latent_gram_reduce");
  return UNET_OK;
}

extern "C" int unet_latent_gram_apply(const float* g, const float* q, float* z, int N,
                                      unet_stream_t stream) {
  UNET_REQUIRE(g && q && z, "latent_gram_apply: null pointer");
  UNET_REQUIRE(N >= 2 && N <= 65536, "latent_gram_apply: N must lie in 2..65536");
  UNET_REQUIRE(lt_aligned(q) && lt_aligned(z), "latent_gram_apply: q and z must be 16-byte aligned");
  hipLaunchKernelGGL(gram_apply_kernel, dim3(ceil_div(N, 4)), dim3(LT_THREADS), 0,
                     (hipStream_t)stream, g, q, z, N);
  UNET_CHECK_LAUNCH("latent_gram_apply");
  return UNET_OK;
}

extern "C" int unet_tsne_cond_p(const float* g, const float* diag, float perplexity, float* pc,
                                double* rowsum, int N, unet_stream_t stream) {
  UNET_REQUIRE(g && diag && pc && rowsum, "tsne_cond_p: null pointer");
  UNET_REQUIRE(N >= 2 && N <= TSNE_MAX_N, "tsne_cond_p: N must lie in 2..%d", TSNE_MAX_N);
  UNET_REQUIRE(perplexity > 0.f && perplexity < (float)N,
               "tsne_cond_p: perplexity must be positive and less than N");
  hipLaunchKernelGGL(tsne_cond_p_kernel, dim3(N), dim3(LT_THREADS), (size_t)N * sizeof(float),
                     (hipStream_t)stream, g, diag, perplexity, pc, rowsum, N);
  UNET_CHECK_LAUNCH("tsne_cond_p");
  return UNET_OK;
}

extern "C" int unet_tsne_joint_p(const float* pc, double* rowsum, float* p, int N,
                                 unet_stream_t stream) {
  UNET_REQUIRE(pc && rowsum && p, "tsne_joint_p: null pointer");
  UNET_REQUIRE(N >= 2 && N <= TSNE_MAX_N, "tsne_joint_p: N must lie in 2..%d", TSNE_MAX_N);
  hipLaunchKernelGGL(tsne_total_kernel, dim3(1), dim3(LT_THREADS), 0, (hipStream_t)stream, rowsum,
                     N);
  UNET_CHECK_LAUNCH("tsne_total");
  const long long blocks = ceil_div64((long long)N * N, LT_THREADS);
  hipLaunchKernelGGL(tsne_joint_p_kernel, dim3((unsigned)blocks), dim3(LT_THREADS), 0,
                     (hipStream_t)stream, pc, rowsum, p, N);
  UNET_CHECK_LAUNCH("tsne_joint_p");
  return UNET_OK;
}

extern "C" int unet_tsne_step(const float* p, const float* state_in, float* state_out,
                              float* rows, double* stats, float exaggeration, float momentum,
                              float lr, int want_stats, int N, unet_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  UNET_REQUIRE(p && state_in && state_out && rows && (stats || !want_stats),
               "tsne_step: null pointer");
  UNET_REQUIRE(state_in != state_out, "tsne_step: state_in and state_out must differ");
  UNET_REQUIRE(N >= 2 && N <= TSNE_MAX_N, "tsne_step: N must lie in 2..%d", TSNE_MAX_N);
  UNET_REQUIRE(lt_aligned(rows), "tsne_step: rows must be 16-byte aligned");
  hipLaunchKernelGGL(tsne_grad_kernel, dim3(ceil_div(N, TS_ROWS)), dim3(LT_THREADS),
                     (size_t)N * sizeof(float2), stream, p, state_in, rows, exaggeration,
                     want_stats, N);
  UNET_CHECK_LAUNCH("tsne_grad");
  hipLaunchKernelGGL(tsne_update_kernel, dim3(ceil_div(N, LT_THREADS)), dim3(LT_THREADS), 0,
                     stream, rows, state_in, state_out, stats, momentum, lr, want_stats, N);
  UNET_CHECK_LAUNCH("tsne_update");
  return UNET_OK;
}

extern "C" int unet_latent_scatter(const int* centres, const uint8_t* labels,
                                   const uint8_t* palette, int K, uint8_t* out, int N, int H,
                                   int W, int radius, unet_stream_t stream) {
  UNET_REQUIRE(centres && labels && palette && out, "latent_scatter: null pointer");
  UNET_REQUIRE(N >= 0 && N <= (1 << 24) && K >= 1 && K <= 256 && H > 0 && W > 0 && H <= 16384 &&
               W <= 16384 && radius >= 0 && radius <= 1024,
               "latent_scatter: bad shape (K in 1..256, H, W in 1..16384, radius in 0..1024)");
  hipLaunchKernelGGL(scatter_kernel, dim3(ceil_div(W, 16), ceil_div(H, 16)), dim3(16, 16), 0,
                     (hipStream_t)stream, centres, labels, palette, K, out, N, H, W, radius);
  UNET_CHECK_LAUNCH("latent_scatter");
  return UNET_OK;
}
