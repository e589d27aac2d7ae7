// evaluate.hip — the tail of test-set evaluation after the eval-mode forward, on the device:
//
//   unet_eval_confusion  argmax over the 3 class planes, the nearest-neighbour resize of the
//                        class map and of the mask to each image's original size, and the 3 x 3
//                        confusion matrix of the resized pair - one launch per batch, no host sync.
//   unet_eval_maps       softmax probabilities, class map and error-category map from one read
//                        of the logits (what the reference's visual helpers plot).
//
// Replaces the per-image loop of evaluate_model (Our_UNet/src/evaluate.py:189-211: two
// F.interpolate calls, two device-to-host copies and about a dozen numpy passes per image) and
// the tensor work of visualize_confidence_maps_batch / create_error_visualization
// (Our_UNet/utils/visualize.py:96-238).
//
// Nearest resize is separable and copies: output pixel (dy, dx) shows source pixel
// (src(dy), src(dx)) of BOTH maps.  So the confusion matrix at the original size is a weighted
// count over the SOURCE pixels with the integer weight
//     (number of output rows that map to y) x (number of output columns that map to x),
// which reads every logit once, coalesced, and costs the same for a 300 x 200 original as for a
// 3000 x 2000 one.  src() is ATen's rule in fp32 as ATen computes it (nearest_src below); it is
// non-decreasing in d, so "how many d map to s" is the difference of two lower bounds, each found
// from an estimate corrected by evaluating the rule itself.  All counts are integers and are
// summed with integer adds: the result does not depend on the order of the workgroups.
#include "common.h"

namespace {

constexpr int EVAL_MAX_DIM = 16384;      // largest original height / width
constexpr long long EVAL_MAX_PIXELS = 1ll << 30;   // per image: pixel indices stay in int
constexpr int EVAL_BLOCKS = 128;         // workgroups per image (grid-stride over the pixels)
constexpr int EVAL_RED_BYTES = 4 * 9 * (int)sizeof(unsigned long long);
// the multiplicity tables live in LDS while H + W entries fit a 64 KiB allocation; larger
// network sizes compute each pixel's multiplicities directly
constexpr int EVAL_TABLE_MAX = (60 * 1024) / 4;

// ATen's nearest source index, min((int)floorf((float)d * ((float)in / (float)out)), in - 1),
// with the multiply and the floor kept as two fp32 operations.  scale = (float)in / (float)out.
__device__ __forceinline__ int nearest_src(int d, float scale, int in) {
  const float f = fminf(floorf(__fmul_rn((float)d, scale)), 2147483520.f);
  return min((int)f, in - 1);
}

// smallest d in [0, out] with nearest_src(d) >= s (out when there is none).  nearest_src is
// non-decreasing in d ((float)d is exact up to 2^24, rounding and floor are monotone), so the two
// loops end at the bound whatever the estimate was; the estimate only keeps them short.
__device__ __forceinline__ int first_d_reaching(int s, float scale, float inv_scale, int in,
                                                int out) {
  if (s <= 0) return 0;
  if (s >= in) return out;
  int d = (int)fminf(ceilf((float)s * inv_scale), (float)out);
  while (d > 0 && nearest_src(d - 1, scale, in) >= s) --d;
  while (d < out && nearest_src(d, scale, in) < s) ++d;
  return d;
}

// number of output indices that show source index s
__device__ __forceinline__ unsigned int multiplicity(int s, float scale, float inv_scale, int in,
                                                     int out) {
  return (unsigned int)(first_d_reaching(s + 1, scale, inv_scale, in, out) -
                        first_d_reaching(s, scale, inv_scale, in, out));
}

// first maximum wins, like torch.argmax and argmax_counts_kernel
__device__ __forceinline__ int argmax3(float z0, float z1, float z2) {
  int am = 0;
  float best = z0;
  if (z1 > best) { best = z1; am = 1; }
  if (z2 > best) { best = z2; am = 2; }
  return am;
}

// q[t * 3 + am] += w without indexing the register array by a run-time value.  A target outside
// {0, 1, 2} (ignore_index, or a label the dataset would have mapped away) matches no counter.
__device__ __forceinline__ void count_pixel(unsigned long long (&q)[9], long long t, int am,
                                            unsigned int w) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) q[r * 3 + c] += (t == r && am == c) ? w : 0u;
}

// cm[b][target class][predicted class] over the pixels of image b at its original size.
// grid (<= EVAL_BLOCKS, B), 256 threads, dynamic LDS = EVAL_RED_BYTES (+ 4 (H + W) with TABLE).
// VEC: H * W and W are multiples of 4 and the pointers are 16-byte aligned, so four pixels of one
// row travel in one 16-byte load per plane.
template <bool VEC, bool TABLE>
__global__ __launch_bounds__(256) void eval_confusion_kernel(
    const float* __restrict__ logits, const long long* __restrict__ target,
    const long long* __restrict__ dims, unsigned long long* __restrict__ cm, int H, int W,
    int ignore_index) {
  extern __shared__ __attribute__((aligned(16))) unsigned char eval_smem[];
  unsigned long long* red = reinterpret_cast<unsigned long long*>(eval_smem);      // [4][9]
  unsigned int* rowm = reinterpret_cast<unsigned int*>(eval_smem + EVAL_RED_BYTES);  // [H]
  unsigned int* colm = rowm + H;                                                     // [W]
  const int b = blockIdx.y;
  const int HW = H * W;
  const bool resize = dims != nullptr;
  int oh = H, ow = W;
  if (resize) {
    // an out-of-range size leaves this image's counts at the zeros of the memset (the whole
    // workgroup leaves together: every thread reads the same two words)
    const long long dh = dims[2 * b], dw = dims[2 * b + 1];
    if (dh < 1 || dh > EVAL_MAX_DIM || dw < 1 || dw > EVAL_MAX_DIM) return;
    oh = (int)dh;
    ow = (int)dw;
  }
  const float sh = __fdiv_rn((float)H, (float)oh), sw = __fdiv_rn((float)W, (float)ow);
  const float ish = (float)oh / (float)H, isw = (float)ow / (float)W;
  if (TABLE && resize) {
    for (int i = threadIdx.x; i < H; i += 256) rowm[i] = multiplicity(i, sh, ish, H, oh);
    for (int i = threadIdx.x; i < W; i += 256) colm[i] = multiplicity(i, sw, isw, W, ow);
    __syncthreads();
  }
  const size_t plane = (size_t)HW;
  const float* z = logits + (size_t)b * 3 * plane;
  const long long* tg = target + (size_t)b * plane;
  const long long ign = ignore_index;
  unsigned long long q[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) q[i] = 0;

  constexpr int NV = VEC ? 4 : 1;
  for (int p = (blockIdx.x * 256 + threadIdx.x) * NV; p < HW; p += gridDim.x * 256 * NV) {
    float z0[NV], z1[NV], z2[NV];
    long long t[NV];
    if constexpr (VEC) {
      const f32x4 a = ld4(z + p), c = ld4(z + plane + p), e = ld4(z + 2 * plane + p);
      typedef long long i64x2 __attribute__((ext_vector_type(2)));
      const i64x2 t01 = *reinterpret_cast<const i64x2*>(tg + p);
      const i64x2 t23 = *reinterpret_cast<const i64x2*>(tg + p + 2);
#pragma unroll
      for (int j = 0; j < 4; ++j) { z0[j] = a[j]; z1[j] = c[j]; z2[j] = e[j]; }
      t[0] = t01[0]; t[1] = t01[1]; t[2] = t23[0]; t[3] = t23[1];
    } else {
      z0[0] = z[p]; z1[0] = z[plane + p]; z2[0] = z[2 * plane + p];
      t[0] = tg[p];
    }
    const int y = p / W, x = p - y * W;     // VEC: W % 4 == 0, the four pixels share row y
    unsigned int wy = 1;
    if (resize) wy = TABLE ? rowm[y] : multiplicity(y, sh, ish, H, oh);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      unsigned int wx = 1;
      if (resize) wx = TABLE ? colm[x + j] : multiplicity(x + j, sw, isw, W, ow);
      // wy, wx <= 16384: the product fits 32 bits
      const unsigned int w = (t[j] != ign) ? wy * wx : 0u;
      count_pixel(q, t[j], argmax3(z0[j], z1[j], z2[j]), w);
    }
  }

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    unsigned long long v = q[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) red[wave * 9 + i] = v;
  }
  __syncthreads();
  if (threadIdx.x < 9) {
    const unsigned long long s = red[threadIdx.x] + red[9 + threadIdx.x] + red[18 + threadIdx.x] +
                                 red[27 + threadIdx.x];
    if (s) atomicAdd(&cm[(size_t)b * 9 + threadIdx.x], s);   // integer: order-independent
  }
}

// The same counting for K classes (2..32).  K * K counters do not fit a lane's registers, so a
// workgroup counts into an LDS table with integer atomics (exact and order-independent, like the
// global adds) and then adds its non-zero entries to cm[b][target class][predicted class].
// grid (<= EVAL_BLOCKS, B), 256 threads, dynamic LDS = 8 K K (+ 4 (H + W) with TABLE).
template <bool TABLE>
__global__ __launch_bounds__(256) void eval_confusionk_kernel(
    const float* __restrict__ logits, const long long* __restrict__ target,
    const long long* __restrict__ dims, unsigned long long* __restrict__ cm, int K, int H, int W,
    int ignore_index) {
  extern __shared__ __attribute__((aligned(16))) unsigned char eval_smem[];
  unsigned long long* tab = reinterpret_cast<unsigned long long*>(eval_smem);       // [K][K]
  unsigned int* rowm = reinterpret_cast<unsigned int*>(eval_smem + 8 * K * K);      // [H]
  unsigned int* colm = rowm + H;                                                    // [W]
  const int b = blockIdx.y;
  const int HW = H * W;
  const bool resize = dims != nullptr;
  int oh = H, ow = W;
  if (resize) {   // (an out-of-range size: zero counts, as eval_confusion_kernel)
    const long long dh = dims[2 * b], dw = dims[2 * b + 1];
    if (dh < 1 || dh > EVAL_MAX_DIM || dw < 1 || dw > EVAL_MAX_DIM) return;
    oh = (int)dh;
    ow = (int)dw;
  }
  const float sh = __fdiv_rn((float)H, (float)oh), sw = __fdiv_rn((float)W, (float)ow);
  const float ish = (float)oh / (float)H, isw = (float)ow / (float)W;
  for (int i = threadIdx.x; i < K * K; i += 256) tab[i] = 0;
  if (TABLE && resize) {
    for (int i = threadIdx.x; i < H; i += 256) rowm[i] = multiplicity(i, sh, ish, H, oh);
    for (int i = threadIdx.x; i < W; i += 256) colm[i] = multiplicity(i, sw, isw, W, ow);
  }
  __syncthreads();
  const size_t plane = (size_t)HW;
  const float* z = logits + (size_t)b * K * plane;
  const long long* tg = target + (size_t)b * plane;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
    const long long t = tg[p];
    if (t == (long long)ignore_index || t < 0 || t >= K) continue;
    int am = 0;                      // first maximum wins, like torch.argmax
    float best = z[p];
    for (int c = 1; c < K; ++c) {
      const float v = z[(size_t)c * plane + p];
      if (v > best) { best = v; am = c; }
    }
    unsigned int w = 1;
    if (resize) {
      const int y = p / W, x = p - y * W;
      const unsigned int wy = TABLE ? rowm[y] : multiplicity(y, sh, ish, H, oh);
      const unsigned int wx = TABLE ? colm[x] : multiplicity(x, sw, isw, W, ow);
      w = wy * wx;                   // wy, wx <= 16384: the product fits 32 bits
    }
    if (w) atomicAdd(&tab[(int)t * K + am], (unsigned long long)w);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < K * K; i += 256)
    if (tab[i]) atomicAdd(&cm[(size_t)b * K * K + i], tab[i]);
}

// eval_confusionk_kernel with the class map given: preds[b][p] (a byte >= K reads as 0) stands
// where the argmax loop stood.  The same multiplicity rule, the same LDS table, the same grid.
template <bool TABLE>
__global__ __launch_bounds__(256) void eval_confusion_classes_kernel(
    const unsigned char* __restrict__ preds, const long long* __restrict__ target,
    const long long* __restrict__ dims, unsigned long long* __restrict__ cm, int K, int H, int W,
    int ignore_index) {
  extern __shared__ __attribute__((aligned(16))) unsigned char eval_smem[];
  unsigned long long* tab = reinterpret_cast<unsigned long long*>(eval_smem);       // [K][K]
  unsigned int* rowm = reinterpret_cast<unsigned int*>(eval_smem + 8 * K * K);      // [H]
  unsigned int* colm = rowm + H;                                                    // [W]
  const int b = blockIdx.y;
  const int HW = H * W;
  const bool resize = dims != nullptr;
  int oh = H, ow = W;
  if (resize) {   // (an out-of-range size: zero counts, as eval_confusion_kernel)
    const long long dh = dims[2 * b], dw = dims[2 * b + 1];
    if (dh < 1 || dh > EVAL_MAX_DIM || dw < 1 || dw > EVAL_MAX_DIM) return;
    oh = (int)dh;
    ow = (int)dw;
  }
  const float sh = __fdiv_rn((float)H, (float)oh), sw = __fdiv_rn((float)W, (float)ow);
  const float ish = (float)oh / (float)H, isw = (float)ow / (float)W;
  for (int i = threadIdx.x; i < K * K; i += 256) tab[i] = 0;
  if (TABLE && resize) {
    for (int i = threadIdx.x; i < H; i += 256) rowm[i] = multiplicity(i, sh, ish, H, oh);
    for (int i = threadIdx.x; i < W; i += 256) colm[i] = multiplicity(i, sw, isw, W, ow);
  }
  __syncthreads();
  const size_t plane = (size_t)HW;
  const unsigned char* pr = preds + (size_t)b * plane;
  const long long* tg = target + (size_t)b * plane;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
    const long long t = tg[p];
    if (t == (long long)ignore_index || t < 0 || t >= K) continue;
    int am = pr[p];
    if (am >= K) am = 0;
    unsigned int w = 1;
    if (resize) {
      const int y = p / W, x = p - y * W;
      const unsigned int wy = TABLE ? rowm[y] : multiplicity(y, sh, ish, H, oh);
      const unsigned int wx = TABLE ? colm[x] : multiplicity(x, sw, isw, W, ow);
      w = wy * wx;                   // wy, wx <= 16384: the product fits 32 bits
    }
    if (w) atomicAdd(&tab[(int)t * K + am], (unsigned long long)w);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < K * K; i += 256)
    if (tab[i]) atomicAdd(&cm[(size_t)b * K * K + i], tab[i]);
}

// error category of create_error_visualization (utils/visualize.py:205-222), both masks with
// 255 mapped to background first: 0 none, 1 true positive, 2 false positive, 3 false negative,
// 4 wrong class.  The prediction is an argmax (0..2), so only the mask can hold 255.
__device__ __forceinline__ unsigned char error_code(int am, long long t) {
  const bool pf = am > 0, gf = (t != 255) && (t > 0);
  if (pf && gf) return (long long)am == t ? 1 : 4;
  if (pf) return 2;
  return gf ? 3 : 0;
}

// grid (blocks, B), 256 threads; any of probs / classes / errors may be NULL
template <bool VEC>
__global__ __launch_bounds__(256) void eval_maps_kernel(const float* __restrict__ logits,
                                                        const long long* __restrict__ target,
                                                        float* __restrict__ probs,
                                                        unsigned char* __restrict__ classes,
                                                        unsigned char* __restrict__ errors,
                                                        int HW) {
  const int b = blockIdx.y;
  const size_t plane = (size_t)HW;
  const float* z = logits + (size_t)b * 3 * plane;
  constexpr int NV = VEC ? 4 : 1;
  for (int p = (blockIdx.x * 256 + threadIdx.x) * NV; p < HW; p += gridDim.x * 256 * NV) {
    float z0[NV], z1[NV], z2[NV];
    if constexpr (VEC) {
      const f32x4 a = ld4(z + p), c = ld4(z + plane + p), e = ld4(z + 2 * plane + p);
#pragma unroll
      for (int j = 0; j < 4; ++j) { z0[j] = a[j]; z1[j] = c[j]; z2[j] = e[j]; }
    } else {
      z0[0] = z[p]; z1[0] = z[plane + p]; z2[0] = z[2 * plane + p];
    }
    int am[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) am[j] = argmax3(z0[j], z1[j], z2[j]);
    if (probs) {
      // softmax as F.softmax computes it in fp32: exp(z - max) / sum, with the library's exp
      // and a correctly rounded division
      float p0[NV], p1[NV], p2[NV];
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        const float m = fmaxf(z0[j], fmaxf(z1[j], z2[j]));
        const float e0 = expf(z0[j] - m), e1 = expf(z1[j] - m), e2 = expf(z2[j] - m);
        const float s = e0 + e1 + e2;
        p0[j] = __fdiv_rn(e0, s); p1[j] = __fdiv_rn(e1, s); p2[j] = __fdiv_rn(e2, s);
      }
      float* o = probs + (size_t)b * 3 * plane + p;
      if constexpr (VEC) {
        st4(o, f32x4{p0[0], p0[1], p0[2], p0[3]});
        st4(o + plane, f32x4{p1[0], p1[1], p1[2], p1[3]});
        st4(o + 2 * plane, f32x4{p2[0], p2[1], p2[2], p2[3]});
      } else {
        o[0] = p0[0]; o[plane] = p1[0]; o[2 * plane] = p2[0];
      }
    }
    if (classes) {
      unsigned char* o = classes + (size_t)b * plane + p;
      if constexpr (VEC)
        *reinterpret_cast<uchar4*>(o) = make_uchar4(am[0], am[1], am[2], am[3]);
      else
        o[0] = (unsigned char)am[0];
    }
    if (errors) {
      const long long* tg = target + (size_t)b * plane + p;
      unsigned char* o = errors + (size_t)b * plane + p;
      if constexpr (VEC) {
        typedef long long i64x2 __attribute__((ext_vector_type(2)));
        const i64x2 t01 = *reinterpret_cast<const i64x2*>(tg);
        const i64x2 t23 = *reinterpret_cast<const i64x2*>(tg + 2);
        *reinterpret_cast<uchar4*>(o) =
            make_uchar4(error_code(am[0], t01[0]), error_code(am[1], t01[1]),
                        error_code(am[2], t23[0]), error_code(am[3], t23[1]));
      } else {
        o[0] = error_code(am[0], tg[0]);
      }
    }
  }
}

bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

int eval_blocks(long long HW, int px_per_thread) {
  const long long blocks = ceil_div64(HW, 256ll * px_per_thread * 2);
  return (int)(blocks < 1 ? 1 : blocks > EVAL_BLOCKS ? EVAL_BLOCKS : blocks);
}

}  // namespace

// K == 3 runs eval_confusion_kernel (four pixels per lane where W % 4 == 0 and the tensors are
// 16-byte aligned), any other K eval_confusionk_kernel; both index a batch's planes with int.
extern "C" int unet_eval_confusionk(const float* logits_nchw, const int64_t* target,
                                    const int64_t* dims, uint64_t* cm, int B, int K, int H, int W,
                                    int ignore_index, unet_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  UNET_REQUIRE(logits_nchw && target && cm, "eval_confusion: null pointer");
  UNET_REQUIRE(K >= 2 && K <= UNET_MAX_CLASSES, "eval_confusion: needs 2 <= K <= %d (got %d)",
               UNET_MAX_CLASSES, K);
  UNET_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && (long long)H * W <= EVAL_MAX_PIXELS &&
                   (long long)H * W * K <= 0x7fffffffll,
               "eval_confusion: bad shape (B in 1..65535, H * W <= 2^30, K * H * W < 2^31)");
  UNET_REQUIRE(ignore_index < 0 || ignore_index >= K,
               "eval_confusion: ignore_index %d is a class index", ignore_index);
  const long long HW = (long long)H * W;
  UNET_HIP_CALL(hipMemsetAsync(cm, 0, (size_t)B * K * K * sizeof(uint64_t), stream));
  const dim3 block(256);
  const long long* tg = reinterpret_cast<const long long*>(target);
  const long long* dm = reinterpret_cast<const long long*>(dims);
  unsigned long long* out = reinterpret_cast<unsigned long long*>(cm);
  if (K != 3) {
    const size_t tab = (size_t)8 * K * K;
    const bool table = !dims || tab + 4 * ((size_t)H + W) <= 64 * 1024;
    const size_t lds = tab + ((dims && table) ? 4 * ((size_t)H + W) : 0);
    const dim3 grid(eval_blocks(HW, 1), B);
    if (table)
      hipLaunchKernelGGL(eval_confusionk_kernel<true>, grid, block, lds, stream, logits_nchw, tg,
                         dm, out, K, H, W, ignore_index);
    else
      hipLaunchKernelGGL(eval_confusionk_kernel<false>, grid, block, lds, stream, logits_nchw, tg,
                         dm, out, K, H, W, ignore_index);
    UNET_CHECK_LAUNCH("eval_confusionk");
    return UNET_OK;
  }
  const bool vec = (W % 4 == 0) && aligned_to(logits_nchw, 16) && aligned_to(target, 16);
  const bool table = !dims || H + (long long)W <= EVAL_TABLE_MAX;
  const size_t lds = EVAL_RED_BYTES + ((dims && table) ? 4 * ((size_t)H + W) : 0);
  const dim3 grid(eval_blocks(HW, vec ? 4 : 1), B);
  if (vec && table)
    hipLaunchKernelGGL((eval_confusion_kernel<true, true>), grid, block, lds, stream, logits_nchw,
                       tg, dm, out, H, W, ignore_index);
  else if (vec)
    hipLaunchKernelGGL((eval_confusion_kernel<true, false>), grid, block, lds, stream,
                       logits_nchw, tg, dm, out, H, W, ignore_index);
  else if (table)
    hipLaunchKernelGGL((eval_confusion_kernel<false, true>), grid, block, lds, stream,
                       logits_nchw, tg, dm, out, H, W, ignore_index);
  else
    hipLaunchKernelGGL((eval_confusion_kernel<false, false>), grid, block, lds, stream,
                       logits_nchw, tg, dm, out, H, W, ignore_index);
  UNET_CHECK_LAUNCH("eval_confusion");
  return UNET_OK;
}

extern "C" int unet_eval_confusion(const float* logits_nchw, const int64_t* target,
                                   const int64_t* dims, uint64_t* cm, int B, int H, int W,
                                   int ignore_index, unet_stream_t stream) {
  return unet_eval_confusionk(logits_nchw, target, dims, cm, B, 3, H, W, ignore_index, stream);
}

extern "C" int unet_eval_confusion_classes(const uint8_t* preds, const int64_t* target,
                                           const int64_t* dims, uint64_t* cm, int B, int K, int H,
                                           int W, int ignore_index, unet_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  UNET_REQUIRE(preds && target && cm, "eval_confusion_classes: null pointer");
  UNET_REQUIRE(B > 0 && B <= 65535, "eval_confusion_classes: B = %d is outside 1..65535", B);
  UNET_REQUIRE(K >= 2 && K <= UNET_MAX_CLASSES,
               "eval_confusion_classes: K = %d is outside 2..%d", K, UNET_MAX_CLASSES);
  UNET_REQUIRE(H > 0 && H <= EVAL_MAX_DIM && W > 0 && W <= EVAL_MAX_DIM &&
                   (long long)H * W <= EVAL_MAX_PIXELS,
               "eval_confusion_classes: H = %d, W = %d (each 1..16384, H * W <= 2^30)", H, W);
  UNET_REQUIRE(ignore_index < 0 || ignore_index >= K,
               "eval_confusion_classes: ignore_index %d is a class index", ignore_index);
  const long long HW = (long long)H * W;
  const size_t tab = (size_t)8 * K * K;
  const bool table = !dims || tab + 4 * ((size_t)H + W) <= 64 * 1024;
  const size_t lds = tab + ((dims && table) ? 4 * ((size_t)H + W) : 0);
  UNET_HIP_CALL(hipMemsetAsync(cm, 0, (size_t)B * K * K * sizeof(uint64_t), stream));
  const dim3 grid(eval_blocks(HW, 1), B), block(256);
  const long long* tg = reinterpret_cast<const long long*>(target);
  const long long* dm = reinterpret_cast<const long long*>(dims);
  unsigned long long* out = reinterpret_cast<unsigned long long*>(cm);
  if (table)
    hipLaunchKernelGGL(eval_confusion_classes_kernel<true>, grid, block, lds, stream, preds, tg,
                       dm, out, K, H, W, ignore_index);
  else
    hipLaunchKernelGGL(eval_confusion_classes_kernel<false>, grid, block, lds, stream, preds, tg,
                       dm, out, K, H, W, ignore_index);
  UNET_CHECK_LAUNCH("eval_confusion_classes");
  return UNET_OK;
}

extern "C" int unet_eval_maps(const float* logits_nchw, const int64_t* target, float* probs,
                              uint8_t* classes, uint8_t* errors, int B, int H, int W,
                              unet_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  UNET_REQUIRE(logits_nchw, "eval_maps: null pointer (logits)");
  UNET_REQUIRE(probs || classes || errors, "eval_maps: no output requested");
  UNET_REQUIRE(!errors || target, "eval_maps: the error map needs the target");
  UNET_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && (long long)H * W <= EVAL_MAX_PIXELS,
               "eval_maps: bad shape (B in 1..65535, H, W >= 1, H * W <= 2^30)");
  const long long HW = (long long)H * W;
  const bool vec = (HW % 4 == 0) && aligned_to(logits_nchw, 16) && aligned_to(probs, 16) &&
                   aligned_to(classes, 4) && aligned_to(errors, 4) &&
                   (!errors || aligned_to(target, 16));
  const dim3 grid(eval_blocks(HW, vec ? 4 : 1), B), block(256);
  const long long* tg = reinterpret_cast<const long long*>(target);
  if (vec)
    hipLaunchKernelGGL(eval_maps_kernel<true>, grid, block, 0, stream, logits_nchw, tg, probs,
                       classes, errors, (int)HW);
  else
    hipLaunchKernelGGL(eval_maps_kernel<false>, grid, block, 0, stream, logits_nchw, tg, probs,
                       classes, errors, (int)HW);
  UNET_CHECK_LAUNCH("eval_maps");
  return UNET_OK;
}
