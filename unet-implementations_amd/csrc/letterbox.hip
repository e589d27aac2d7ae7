// letterbox.hip — from decoded samples of different sizes to the network-size uint8 batch, on the
// device:
//
//   unet_letterbox_u8       every sample of a ragged batch resized (image: OpenCV's INTER_LINEAR in
//                           its fixed-point form, mask: INTER_NEAREST) and placed in its S_h x S_w
//                           tile, padding included - one launch per output size, no host sync.
//   unet_byte_histogram_u8  the byte histogram of every sample's mask at its original size (the
//                           values present, for the label table; the class pixel counts, for the
//                           static class weights).
//
// Replaces the per-sample cv2.resize + pad of the reference's preprocessing scripts and dataset
// (header comment of this section in unet_hip.h lists the places).
//
// The arithmetic is a restatement of OpenCV's generic path, integer from the tap weights on, so the
// bytes do not depend on the launch shape.  The only floating-point part is the tap table of each
// axis; its expressions are compiled with contraction off (a fused (d + 0.5) * scale - 0.5 can land
// on the other side of an integer) and evaluated once per workgroup into LDS.
//
// Launch shape: grid (ceil(S_h / LB_ROWS), B), 256 threads.  A workgroup owns LB_ROWS full rows of
// one tile and walks them in chunks of NB consecutive BYTES of the row (NB = 16, 4 or 1 by the
// alignment of S_w and of the outputs), so the stores of a wave are one contiguous run whatever
// the padding is; a byte of the padding is a 0 in the same store.  Source bytes are read one at a
// time: sample offsets are byte-granular (a 37 x 53 x 3 image is 5883 bytes), and the four taps of
// neighbouring output bytes share their cache lines.
#include "common.h"

namespace {

constexpr int LB_MAX_DIM = 16384;   // largest source height / width
constexpr int LB_MAX_S = 4096;      // largest tile height / width
constexpr int LB_ROWS = 8;          // tile rows per workgroup
constexpr int LB_F = UNET_LETTERBOX_FIELDS;
constexpr int HIST_BLOCKS = 32;     // workgroups per sample (the sizes are not known on the host)

struct LbRec {
  long long img, msk;               // byte offsets
  int h, w, oh, ow, py, px;
  bool dims_ok, img_ok, msk_ok, geom_ok;
};

// Every thread of the workgroup reads the same eight words: the flags are uniform.
__device__ __forceinline__ LbRec lb_record(const long long* __restrict__ table, int b,
                                           unsigned long long arena_bytes, int S_h, int S_w) {
  const long long* r = table + (size_t)b * LB_F;
  LbRec q;
  q.img = r[0]; q.msk = r[1];
  const long long h = r[2], w = r[3], oh = r[4], ow = r[5], py = r[6], px = r[7];
  q.dims_ok = h >= 1 && h <= LB_MAX_DIM && w >= 1 && w <= LB_MAX_DIM;
  q.geom_ok = oh >= 1 && oh <= S_h && ow >= 1 && ow <= S_w && py >= 0 && px >= 0 &&
              py + oh <= S_h && px + ow <= S_w;
  q.h = (int)h; q.w = (int)w; q.oh = (int)oh; q.ow = (int)ow; q.py = (int)py; q.px = (int)px;
  const unsigned long long px_count = q.dims_ok ? (unsigned long long)(h * w) : 0ull;
  q.img_ok = q.dims_ok && q.img >= 0 && (unsigned long long)q.img <= arena_bytes &&
             3ull * px_count <= arena_bytes - (unsigned long long)q.img;
  q.msk_ok = q.dims_ok && q.msk >= 0 && (unsigned long long)q.msk <= arena_bytes &&
             px_count <= arena_bytes - (unsigned long long)q.msk;
  return q;
}

// scale = 1.0 / ((double)dst / (double)src), two correctly rounded divisions
__device__ __forceinline__ double lb_scale(int src, int dst) {
  return __ddiv_rn(1.0, __ddiv_rn((double)dst, (double)src));
}

// Linear taps of output index d: packed (s0 | s1 << 16, a0 | a1 << 16); s < 16384, a <= 2048.
__device__ __forceinline__ uint2 lb_linear_tap(int d, double scale, int src) {
  // Plain operators under the pragma: the header's __dmul_rn / __dsub_rn are inline functions
  // compiled WITH contraction, and the pair comes out as one v_fma_f64 once they are inlined.
#pragma clang fp contract(off)
  const double t = ((double)d + 0.5) * scale;
  float f = (float)(t - 0.5);
  const float fl = floorf(f);
  int s = (int)fl;
  f = f - fl;
  if (s < 0) { s = 0; f = 0.f; }
  if (s >= src - 1) { s = src - 1; f = 0.f; }
  const int s1 = min(s + 1, src - 1);
  const int a0 = (int)rintf((1.f - f) * 2048.f);
  const int a1 = (int)rintf(f * 2048.f);
  return make_uint2((unsigned)s | ((unsigned)s1 << 16), (unsigned)a0 | ((unsigned)a1 << 16));
}

// the 2 x 2 block of the area path in the same form (the weights are not read)
__device__ __forceinline__ uint2 lb_area_tap(int d) {
  return make_uint2((unsigned)(2 * d) | ((unsigned)(2 * d + 1) << 16), 0u);
}

__device__ __forceinline__ int lb_nearest(int d, double scale, int src) {
  return min((int)floor((double)d * scale), src - 1);
}

template <int NB>
__device__ __forceinline__ void lb_store(unsigned char* p, const unsigned char (&v)[NB]) {
  if constexpr (NB == 1) {
    p[0] = v[0];
  } else {
    unsigned int wd[NB / 4];
#pragma unroll
    for (int i = 0; i < NB / 4; ++i)
      wd[i] = (unsigned)v[4 * i] | ((unsigned)v[4 * i + 1] << 8) | ((unsigned)v[4 * i + 2] << 16) |
              ((unsigned)v[4 * i + 3] << 24);
    if constexpr (NB == 4) *reinterpret_cast<unsigned int*>(p) = wd[0];
    else *reinterpret_cast<uint4*>(p) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
  }
}

// NB: bytes per store; S_w % NB == 0 and both outputs NB-aligned (the launcher's choice).
// dynamic LDS: uint2 xt[S_w], uint2 yt[LB_ROWS], unsigned short xn[S_w], unsigned short yn[LB_ROWS]
template <int NB>
__global__ __launch_bounds__(256) void letterbox_kernel(
    const unsigned char* __restrict__ arena, unsigned long long arena_bytes,
    const long long* __restrict__ table, unsigned char* __restrict__ image_out,
    unsigned char* __restrict__ mask_out, const unsigned char* __restrict__ lut, int S_h, int S_w) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lb_smem[];
  uint2* xt = reinterpret_cast<uint2*>(lb_smem);
  uint2* yt = xt + S_w;
  unsigned short* xn = reinterpret_cast<unsigned short*>(yt + LB_ROWS);
  unsigned short* yn = xn + S_w;

  const int b = blockIdx.y;
  const int y0 = blockIdx.x * LB_ROWS;
  const int rows = min(LB_ROWS, S_h - y0);
  const LbRec q = lb_record(table, b, arena_bytes, S_h, S_w);
  const bool img_ok = q.img_ok && q.geom_ok;
  // a bad record has no mask either
  const bool msk_ok = mask_out != nullptr && q.msk_ok && img_ok;
  const bool area = q.h == 2 * q.oh && q.w == 2 * q.ow;

  if (img_ok || msk_ok) {
    const double sx = lb_scale(q.w, q.ow), sy = lb_scale(q.h, q.oh);
    for (int d = threadIdx.x; d < q.ow; d += 256) {
      if (img_ok) xt[q.px + d] = area ? lb_area_tap(d) : lb_linear_tap(d, sx, q.w);
      if (msk_ok) xn[q.px + d] = (unsigned short)lb_nearest(d, sx, q.w);
    }
    if (threadIdx.x < rows) {
      const int d = y0 + (int)threadIdx.x - q.py;
      if (d >= 0 && d < q.oh) {
        if (img_ok) yt[threadIdx.x] = area ? lb_area_tap(d) : lb_linear_tap(d, sy, q.h);
        if (msk_ok) yn[threadIdx.x] = (unsigned short)lb_nearest(d, sy, q.h);
      }
    }
  }
  __syncthreads();

  // ---- image rows: S_w * 3 bytes each ----
  {
    const int row_bytes = S_w * 3;
    const int chunks = row_bytes / NB;
    const unsigned char* src = arena + (img_ok ? q.img : 0);
    unsigned char* dst = image_out + ((size_t)b * S_h + y0) * row_bytes;
    for (int i = threadIdx.x; i < rows * chunks; i += 256) {
      const int r = i / chunks, c = i - r * chunks;
      const int yd = y0 + r - q.py;
      const bool row_in = img_ok && yd >= 0 && yd < q.oh;
      unsigned char v[NB];
#pragma unroll
      for (int k = 0; k < NB; ++k) v[k] = 0;
      if (row_in) {
        const uint2 ty = yt[r];
        // (y * w + x) * 3 + 2 < 3 * 2^28: int
        const int r0 = (int)(ty.x & 0xffffu) * q.w, r1 = (int)(ty.x >> 16) * q.w;
        const int b0 = (int)(ty.y & 0xffffu), b1 = (int)(ty.y >> 16);
#pragma unroll
        for (int k = 0; k < NB; ++k) {
          const int j = c * NB + k;
          const int x = j / 3, ch = j - 3 * x;
          if (x >= q.px && x < q.px + q.ow) {
            const uint2 tx = xt[x];
            const int x0 = (int)(tx.x & 0xffffu), x1 = (int)(tx.x >> 16);
            const int p00 = src[(r0 + x0) * 3 + ch], p01 = src[(r0 + x1) * 3 + ch];
            const int p10 = src[(r1 + x0) * 3 + ch], p11 = src[(r1 + x1) * 3 + ch];
            int o;
            if (area) {
              o = (p00 + p01 + p10 + p11 + 2) >> 2;
            } else {
              const int a0 = (int)(tx.y & 0xffffu), a1 = (int)(tx.y >> 16);
              const int R0 = p00 * a0 + p01 * a1, R1 = p10 * a0 + p11 * a1;
              o = (((b0 * (R0 >> 4)) >> 16) + ((b1 * (R1 >> 4)) >> 16) + 2) >> 2;
            }
            v[k] = (unsigned char)o;
          }
        }
      }
      lb_store<NB>(dst + (size_t)r * row_bytes + (size_t)c * NB, v);
    }
  }

  // ---- mask rows: S_w bytes each ----
  if (mask_out != nullptr) {
    const int chunks = S_w / NB;
    const unsigned char* src = arena + (msk_ok ? q.msk : 0);
    const unsigned char* tb = lut ? lut + (size_t)b * 256 : nullptr;
    unsigned char* dst = mask_out + ((size_t)b * S_h + y0) * S_w;
    for (int i = threadIdx.x; i < rows * chunks; i += 256) {
      const int r = i / chunks, c = i - r * chunks;
      const int yd = y0 + r - q.py;
      const bool row_in = msk_ok && yd >= 0 && yd < q.oh;
      unsigned char v[NB];
#pragma unroll
      for (int k = 0; k < NB; ++k) v[k] = 0;
      if (row_in) {
        const int r0 = (int)yn[r] * q.w;
#pragma unroll
        for (int k = 0; k < NB; ++k) {
          const int x = c * NB + k;
          if (x >= q.px && x < q.px + q.ow) {
            const unsigned char m = src[r0 + (int)xn[x]];
            v[k] = tb ? tb[m] : m;
          }
        }
      }
      lb_store<NB>(dst + (size_t)r * S_w + (size_t)c * NB, v);
    }
  }
}

// hist[b][v] += occurrences of v in the mask of sample b.  grid (HIST_BLOCKS, B), 256 threads.
// A mask is piecewise constant, so a thread counts runs in registers and touches LDS once per
// change of value; each wave has its own LDS table.  The body is read in aligned 16-byte words
// (the mask may start at any byte): workgroup 0 also takes the bytes before and after them.
__global__ __launch_bounds__(256) void byte_histogram_kernel(
    const unsigned char* __restrict__ arena, unsigned long long arena_bytes,
    const long long* __restrict__ table, unsigned long long* __restrict__ hist) {
  __shared__ unsigned int bins[4][256];
  const int b = blockIdx.y;
  const LbRec q = lb_record(table, b, arena_bytes, 0, 0);
  if (!q.msk_ok) return;                       // uniform; the counts stay at the zeros of the memset
  for (int i = threadIdx.x; i < 4 * 256; i += 256) (&bins[0][0])[i] = 0;
  __syncthreads();

  const unsigned char* p = arena + q.msk;
  const long long n = (long long)q.h * q.w;    // <= 2^28
  long long head = (long long)((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15);
  head = head < n ? head : n;
  const long long nvec = (n - head) >> 4;
  const long long tail = head + (nvec << 4);

  unsigned int* mine = bins[threadIdx.x >> 6];
  int cur = 0;
  unsigned int cnt = 0;
  // a workgroup sees at most 2^28 bytes: the 32-bit counters cannot wrap
  auto add = [&](int v) {
    if (v == cur) {
      ++cnt;
    } else {
      if (cnt) atomicAdd(&mine[cur], cnt);
      cur = v;
      cnt = 1;
    }
  };
  if (blockIdx.x == 0) {
    for (long long i = threadIdx.x; i < head; i += 256) add(p[i]);
    for (long long i = tail + threadIdx.x; i < n; i += 256) add(p[i]);
  }
  const uint4* pv = reinterpret_cast<const uint4*>(p + head);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nvec;
       i += (long long)gridDim.x * 256) {
    const uint4 u = pv[i];
    const unsigned int wd[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) add((int)((wd[k] >> (8 * j)) & 255u));
  }
  if (cnt) atomicAdd(&mine[cur], cnt);
  __syncthreads();
  const unsigned long long s = (unsigned long long)bins[0][threadIdx.x] + bins[1][threadIdx.x] +
                               bins[2][threadIdx.x] + bins[3][threadIdx.x];
  if (s) atomicAdd(&hist[(size_t)b * 256 + threadIdx.x], s);   // integer: order-independent
}

bool lb_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" int unet_letterbox_u8(const uint8_t* arena, size_t arena_bytes, const int64_t* table,
                                 int B, int S_h, int S_w, uint8_t* image_out, uint8_t* mask_out,
                                 const uint8_t* lut, unet_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  UNET_REQUIRE(arena && table && image_out, "letterbox_u8: null pointer (arena, table, image_out)");
  UNET_REQUIRE(!lut || mask_out, "letterbox_u8: a lut needs mask_out");
  UNET_REQUIRE(B > 0 && B <= 65535, "letterbox_u8: bad batch size %d (1..65535)", B);
  UNET_REQUIRE(S_h >= 1 && S_h <= LB_MAX_S && S_w >= 1 && S_w <= LB_MAX_S,
               "letterbox_u8: bad size %d x %d (1..%d)", S_h, S_w, LB_MAX_S);
  const size_t lds = (size_t)S_w * (sizeof(uint2) + sizeof(unsigned short)) +
                     LB_ROWS * (sizeof(uint2) + sizeof(unsigned short));      // <= 40 KiB + 80
  const dim3 grid(ceil_div(S_h, LB_ROWS), B), block(256);
  const long long* tb = reinterpret_cast<const long long*>(table);
  const unsigned long long nbytes = arena_bytes;
  const int nb = (S_w % 16 == 0 && lb_aligned(image_out, 16) && lb_aligned(mask_out, 16)) ? 16
                 : (S_w % 4 == 0 && lb_aligned(image_out, 4) && lb_aligned(mask_out, 4)) ? 4 : 1;
  if (nb == 16)
    hipLaunchKernelGGL(letterbox_kernel<16>, grid, block, lds, stream, arena, nbytes, tb, image_out,
                       mask_out, lut, S_h, S_w);
  else if (nb == 4)
    hipLaunchKernelGGL(letterbox_kernel<4>, grid, block, lds, stream, arena, nbytes, tb, image_out,
                       mask_out, lut, S_h, S_w);
  else
    hipLaunchKernelGGL(letterbox_kernel<1>, grid, block, lds, stream, arena, nbytes, tb, image_out,
                       mask_out, lut, S_h, S_w);
  UNET_CHECK_LAUNCH("letterbox_u8");
  return UNET_OK;
}

extern "C" int unet_byte_histogram_u8(const uint8_t* arena, size_t arena_bytes,
                                      const int64_t* table, int B, uint64_t* hist,
                                      unet_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  UNET_REQUIRE(arena && table && hist, "byte_histogram_u8: null pointer");
  UNET_REQUIRE(B > 0 && B <= 65535, "byte_histogram_u8: bad batch size %d (1..65535)", B);
  UNET_HIP_CALL(hipMemsetAsync(hist, 0, (size_t)B * 256 * sizeof(uint64_t), stream));
  hipLaunchKernelGGL(byte_histogram_kernel, dim3(HIST_BLOCKS, B), dim3(256), 0, stream, arena,
                     (unsigned long long)arena_bytes,
                     reinterpret_cast<const long long*>(table),
                     reinterpret_cast<unsigned long long*>(hist));
  UNET_CHECK_LAUNCH("byte_histogram_u8");
  return UNET_OK;
}
