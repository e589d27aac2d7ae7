// postprocess.hip — what happens to a predicted class map after the argmax, on the device:
//
//   unet_cc_label_u8      connected-component labelling of a uint8 class map (4- or 8-connectivity;
//                         foreground, per-class or background components) with per-component areas
//   unet_mask_cleanup_u8  component removal (min_area, keep_largest), per-image or per-component
//                         class vote and hole filling, in that order
//
// Definitions: include/unet_hip.h (section "mask post-processing") and DESIGN.md section 15.
//
// Labelling is union-find in three launches, none of which waits for the host:
//   cc_tile_kernel    one workgroup per 64 x 32 tile resolves the tile's components in LDS (row
//                     runs from one ballot per row, then row-to-row unions) and writes parent[p] =
//                     the tile-local root as an index into the IMAGE.  Raster order inside a tile
//                     is raster order of the image restricted to the tile, so a root is already
//                     the smallest index of its tile-local component.
//   cc_merge_kernel   one thread per pixel on a tile seam unions it with its neighbours across
//                     the seam: atomicMin towards the smaller root, retried until stable.
//   cc_finish_kernel  every pixel walks to its root and writes labels = root + 1; areas are
//                     integer atomicAdds at the root, one per distinct root inside a wave.
// A root is always the smallest index of its set (a union links the larger root under the
// smaller), so labels do not depend on the order in which workgroups ran.  Every data-dependent
// loop has an iteration bound; on overrun the kernel sets the workspace's status word and goes on
// to its end, so a bug is a failed check and never a hung device.
//
// All arithmetic is integer; there is no floating point and no float atomic in this file.
#include "common.h"

namespace {

constexpr int CC_TW = 64, CC_TH = 32, CC_TILE = CC_TW * CC_TH;   // tile: one wave per row
constexpr unsigned CC_NONE = 0xffffffffu;       // parent of an unselected pixel
constexpr unsigned CC_EDGE_BIT = 0x80000000u;   // in an area word: the component touches an edge
constexpr int PP_MAX_DIM = 16384;
constexpr long long PP_MAX_PIXELS = 1ll << 30;
constexpr int PP_BLOCKS = 256;                  // workgroups per image of the per-pixel kernels
constexpr size_t PP_HEADER = 256;               // status word (+ padding)
enum { MODE_FOREGROUND = 0, MODE_CLASS = 1, MODE_BACKGROUND = 2 };
enum { ST_TILE_FIND = 1, ST_TILE_UNION = 2, ST_MERGE_FIND = 4, ST_MERGE_UNION = 8,
       ST_FINISH_FIND = 16 };

// The byte two neighbours compare: they join when their keys are equal and not 0.
template <int MODE>
__device__ __forceinline__ unsigned key_of(unsigned v, int K) {
  if (v >= (unsigned)K) v = 0;
  if (MODE == MODE_CLASS) return v;
  if (MODE == MODE_BACKGROUND) return v == 0 ? 1u : 0u;
  return v != 0 ? 1u : 0u;
}

__device__ __forceinline__ unsigned lds_load(const unsigned* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// root of x in the LDS forest (L[r] == r), at most CC_TILE steps
__device__ __forceinline__ unsigned tile_find(const unsigned* L, unsigned x, unsigned* status) {
  for (int it = 0; it < CC_TILE; ++it) {
    const unsigned p = lds_load(&L[x]);
    if (p == x) return x;
    x = p;
  }
  atomicOr(status, (unsigned)ST_TILE_FIND);
  return x;
}

// Links the larger root under the smaller.  atomicMin returns what the word held: when that is
// not the root we believed in, somebody else linked it first and the union is retried from there.
__device__ __forceinline__ void tile_union(unsigned* L, unsigned a, unsigned b, unsigned* status) {
  for (int it = 0; it < CC_TILE; ++it) {
    a = tile_find(L, a, status);
    b = tile_find(L, b, status);
    if (a == b) return;
    if (a < b) { const unsigned t = a; a = b; b = t; }    // a > b
    const unsigned old = atomicMin(&L[a], b);
    if (old == a) return;
    a = old;
  }
  atomicOr(status, (unsigned)ST_TILE_UNION);
}

// grid (tiles_x * tiles_y, B), 256 threads.  Wave w owns rows w, w + 4, ... of the tile, the lane
// is the column.  parent[b][p] = image index of p's tile-local root, CC_NONE when p is unselected.
template <int CONN, int MODE>
__global__ __launch_bounds__(256) void cc_tile_kernel(const unsigned char* __restrict__ classes,
                                                      unsigned* __restrict__ parent,
                                                      unsigned* __restrict__ status, int K, int H,
                                                      int W, int tiles_x) {
  __shared__ unsigned L[CC_TILE];
  __shared__ unsigned char Kb[CC_TILE];
  const int b = blockIdx.y;
  const int ty0 = (blockIdx.x / tiles_x) * CC_TH, tx0 = (blockIdx.x % tiles_x) * CC_TW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t img = (size_t)b * H * W;
  const int gx = tx0 + lane;

  // row runs: a run starts where the key differs from the left neighbour's; every lane of a run
  // takes the start of its run as its parent
#pragma unroll
  for (int i = 0; i < CC_TH / 4; ++i) {
    const int row = wave + 4 * i, gy = ty0 + row;
    unsigned k = 0;
    if (gy < H && gx < W) k = key_of<MODE>(classes[img + (size_t)gy * W + gx], K);
    const unsigned kl = __shfl_up(k, 1, 64);
    const bool start = k != 0 && (lane == 0 || kl != k);
    const unsigned long long starts = __ballot(start);
    const unsigned long long upto = starts & (~0ull >> (63 - lane));
    const int rs = upto ? 63 - __builtin_clzll(upto) : lane;     // (k != 0 => upto != 0)
    Kb[row * CC_TW + lane] = (unsigned char)k;
    L[row * CC_TW + lane] = (unsigned)(row * CC_TW + (k ? rs : lane));
  }
  __syncthreads();

  // row-to-row unions.  A pair is skipped when the pair one column to the side joins the same
  // two runs: that leaves one union per pair of touching runs in the common case.
#pragma unroll
  for (int i = 0; i < CC_TH / 4; ++i) {
    const int row = wave + 4 * i;
    if (row == 0) continue;
    const int p = row * CC_TW + lane, q = p - CC_TW;
    const unsigned k = Kb[p];
    if (k == 0) continue;
    const bool up = Kb[q] == k;
    const bool left = lane > 0 && Kb[p - 1] == k;
    const bool ul = lane > 0 && Kb[q - 1] == k;
    if (up && !(left && ul)) tile_union(L, (unsigned)p, (unsigned)q, status);
    if (CONN == 8 && !up) {
      // (with `up` joined, both diagonals lie in the run of the pixel above)
      const bool right = lane < CC_TW - 1 && Kb[p + 1] == k;
      const bool ur = lane < CC_TW - 1 && Kb[q + 1] == k;
      if (ul && !left) tile_union(L, (unsigned)p, (unsigned)(q - 1), status);
      if (ur && !right) tile_union(L, (unsigned)p, (unsigned)(q + 1), status);
    }
  }
  __syncthreads();

#pragma unroll
  for (int i = 0; i < CC_TH / 4; ++i) {
    const int row = wave + 4 * i, gy = ty0 + row;
    if (gy >= H || gx >= W) continue;
    const int p = row * CC_TW + lane;
    unsigned out = CC_NONE;
    if (Kb[p]) {
      const unsigned r = tile_find(L, (unsigned)p, status);
      out = (unsigned)((ty0 + (int)(r / CC_TW)) * W + tx0 + (int)(r % CC_TW));
    }
    parent[img + (size_t)gy * W + gx] = out;
  }
}

// Parent words are rewritten by other workgroups during the merge: relaxed agent-scope atomic
// loads are served by L2, a plain load may be served by a stale L1 line.
__device__ __forceinline__ unsigned agent_load(const unsigned* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ unsigned merge_find(const unsigned* par, unsigned x, int limit,
                                               unsigned* status) {
  for (int it = 0; it <= limit; ++it) {
    const unsigned p = agent_load(&par[x]);
    if (p == x) return x;
    x = p;
  }
  atomicOr(status, (unsigned)ST_MERGE_FIND);
  return CC_NONE;
}

// par: one image's parent plane.  a, b: selected pixels that join.
__device__ __forceinline__ void merge_union(unsigned* par, unsigned a, unsigned b, int limit,
                                            unsigned* status) {
  const unsigned a0 = a, b0 = b;
  for (int it = 0; it <= limit; ++it) {
    a = merge_find(par, a, limit, status);
    b = merge_find(par, b, limit, status);
    if (a == CC_NONE || b == CC_NONE) return;             // overrun: the status word says so
    if (a == b) break;
    if (a < b) { const unsigned t = a; a = b; b = t; }    // a > b
    const unsigned old = atomicMin(&par[a], b);
    if (old == a) { a = b; break; }
    a = old;              // (a + b falls with every retry: at most 2 H W of them)
    if (it == limit) { atomicOr(status, (unsigned)ST_MERGE_UNION); return; }
  }
  // shorten the two paths that were just walked: a is an ancestor of both (or equal)
  if (a < a0) atomicMin(&par[a0], a);
  if (a < b0) atomicMin(&par[b0], a);
}

// grid (blocks, B), 256 threads, one thread per seam pixel: the first row of every tile row but
// the first (n_h * W pixels, joined upwards), then the first column of every tile column but the
// first (n_v * H pixels, joined to the left).  A pair never leaves the image: x - 1 and x + 1 are
// tested against 0 and W, so column W - 1 never meets column 0 of the next row.
template <int CONN, int MODE>
__global__ __launch_bounds__(256) void cc_merge_kernel(const unsigned char* __restrict__ classes,
                                                       unsigned* __restrict__ parent,
                                                       unsigned* __restrict__ status, int K, int H,
                                                       int W, int n_h, int n_v) {
  const int b = blockIdx.y;
  const int HW = H * W;
  const unsigned char* cls = classes + (size_t)b * HW;
  unsigned* par = parent + (size_t)b * HW;
  const long long total = (long long)n_h * W + (long long)n_v * H;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total;
       i += (long long)gridDim.x * 256) {
    int y, x;
    bool horiz;        // a pixel of a horizontal seam (joined upwards)
    if (i < (long long)n_h * W) {
      horiz = true;
      y = ((int)(i / W) + 1) * CC_TH;
      x = (int)(i % W);
    } else {
      const long long j = i - (long long)n_h * W;
      horiz = false;
      x = ((int)(j / H) + 1) * CC_TW;
      y = (int)(j % H);
    }
    const unsigned p = (unsigned)(y * W + x);
    const unsigned k = key_of<MODE>(cls[p], K);
    if (k == 0) continue;
    if (horiz) {
      const bool up = key_of<MODE>(cls[p - W], K) == k;
      if (up) merge_union(par, p, p - W, HW, status);
      if (CONN == 8 && !up) {
        if (x > 0 && key_of<MODE>(cls[p - W - 1], K) == k)
          merge_union(par, p, p - W - 1, HW, status);
        if (x < W - 1 && key_of<MODE>(cls[p - W + 1], K) == k)
          merge_union(par, p, p - W + 1, HW, status);
      }
    } else {
      const bool left = key_of<MODE>(cls[p - 1], K) == k;
      if (left) merge_union(par, p, p - 1, HW, status);
      if (CONN == 8 && !left) {
        if (y > 0 && key_of<MODE>(cls[p - W - 1], K) == k)
          merge_union(par, p, p - W - 1, HW, status);
        if (y < H - 1 && key_of<MODE>(cls[p + W - 1], K) == k)
          merge_union(par, p, p + W - 1, HW, status);
      }
    }
  }
}

// One integer atomicAdd per DISTINCT key inside the wave, whatever the lanes' order: the wave
// elects its first pending lane, every lane with that lane's key is counted by one ballot, the
// elected lane adds the count, and the election repeats for the lanes that are left (at most 64
// rounds, one per distinct key).  A percolating component or a one-pixel-wide spiral arm, whose
// pixels are not neighbours along the row, still sends one add per wave to its root instead of one
// per pixel: same-address atomics retire one after the other (about 8 ns each measured), so their
// count is what bounds the kernel.  key == CC_NONE adds nothing.  Every lane of the wave calls
// this; the loop condition is wave-uniform.
__device__ __forceinline__ void add_by_key(unsigned* dst, unsigned key, int lane) {
  unsigned long long todo = __ballot(key != CC_NONE);
  while (todo) {
    const int leader = __builtin_ctzll(todo);
    const unsigned k = __shfl(key, leader, 64);
    const unsigned long long same = __ballot(key == k) & todo;
    if (lane == leader) atomicAdd(&dst[k], (unsigned)__popcll(same));
    todo &= ~same;
  }
}

// the same election for the edge bit: one atomicOr per distinct key
__device__ __forceinline__ void or_by_key(unsigned* dst, unsigned key, unsigned bit, int lane) {
  unsigned long long todo = __ballot(key != CC_NONE);
  while (todo) {
    const int leader = __builtin_ctzll(todo);
    const unsigned k = __shfl(key, leader, 64);
    if (lane == leader) atomicOr(&dst[k], bit);
    todo &= ~__ballot(key == k);
  }
}

// grid (blocks, B), 256 threads.  labels = root + 1 (0 unselected); areas (zeroed by the caller)
// += pixels at the root.  EDGE: a selected pixel on the image's border sets CC_EDGE_BIT in its
// root's area word (an area is at most 2^30).  The parent word is left pointing at the root.
template <bool EDGE>
__global__ __launch_bounds__(256) void cc_finish_kernel(unsigned* __restrict__ parent,
                                                        unsigned* __restrict__ labels,
                                                        unsigned* __restrict__ areas,
                                                        unsigned* __restrict__ status, int H,
                                                        int W) {
  const int b = blockIdx.y;
  const int HW = H * W;
  unsigned* par = parent + (size_t)b * HW;
  unsigned* lab = labels + (size_t)b * HW;
  unsigned* are = areas + (size_t)b * HW;
  const int lane = threadIdx.x & 63;
  for (int base = blockIdx.x * 256 + (threadIdx.x & ~63); base < HW; base += gridDim.x * 256) {
    const int p = base + lane;
    unsigned r = CC_NONE;
    if (p < HW) {
      unsigned x = par[p];
      if (x != CC_NONE) {
        int it = 0;
        for (; it <= HW; ++it) {
          const unsigned up = par[x];
          if (up == x) break;
          x = up;
        }
        if (it > HW) atomicOr(status, (unsigned)ST_FINISH_FIND);
        r = x;
        par[p] = r;      // (a racing walker reads the old ancestor or the root: both lead there)
      }
      lab[p] = r == CC_NONE ? 0u : r + 1u;
    }
    if (EDGE) {
      unsigned e = CC_NONE;
      if (r != CC_NONE) {
        const int y = p / W, xx = p - y * W;
        if (y == 0 || y == H - 1 || xx == 0 || xx == W - 1) e = r;
      }
      or_by_key(are, e, CC_EDGE_BIT, lane);
    }
    add_by_key(are, r, lane);
  }
}

// Zeroes n 32-bit words.  A launch like every other step (the workspaces are cleared by the same
// means in a plain stream and in a replayed graph).
__global__ __launch_bounds__(256) void pp_zero_kernel(unsigned* __restrict__ p, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    p[i] = 0;
}

int pp_zero(void* p, size_t bytes, hipStream_t stream) {
  const size_t n = bytes / sizeof(unsigned);
  const size_t blocks = (n + 1023) / 1024;
  hipLaunchKernelGGL(pp_zero_kernel, dim3((unsigned)(blocks < 1 ? 1 : blocks > 4096 ? 4096 : blocks)),
                     dim3(256), 0, stream, static_cast<unsigned*>(p), n);
  UNET_CHECK_LAUNCH("pp_zero");
  return UNET_OK;
}

int pp_blocks(long long n) {
  const long long blocks = ceil_div64(n, 256ll * 4);
  return (int)(blocks < 1 ? 1 : blocks > PP_BLOCKS ? PP_BLOCKS : blocks);
}

template <int CONN, int MODE>
int cc_launch(const unsigned char* classes, unsigned* parent, unsigned* labels, unsigned* areas,
              unsigned* status, bool edge, int B, int K, int H, int W, hipStream_t stream) {
  const int tiles_x = ceil_div(W, CC_TW), tiles_y = ceil_div(H, CC_TH);
  hipLaunchKernelGGL((cc_tile_kernel<CONN, MODE>), dim3(tiles_x * tiles_y, B), dim3(256), 0,
                     stream, classes, parent, status, K, H, W, tiles_x);
  UNET_CHECK_LAUNCH("cc_tile");
  const int n_h = tiles_y - 1, n_v = tiles_x - 1;
  const long long seam = (long long)n_h * W + (long long)n_v * H;
  if (seam > 0) {
    const long long blocks = ceil_div64(seam, 256);
    hipLaunchKernelGGL((cc_merge_kernel<CONN, MODE>),
                       dim3((unsigned)(blocks > 4096 ? 4096 : blocks), B), dim3(256), 0, stream,
                       classes, parent, status, K, H, W, n_h, n_v);
    UNET_CHECK_LAUNCH("cc_merge");
  }
  const long long HW = (long long)H * W;
  if (int rc = pp_zero(areas, (size_t)B * HW * sizeof(unsigned), stream)) return rc;
  const dim3 grid(pp_blocks(HW), B);
  if (edge)
    hipLaunchKernelGGL(cc_finish_kernel<true>, grid, dim3(256), 0, stream, parent, labels, areas,
                       status, H, W);
  else
    hipLaunchKernelGGL(cc_finish_kernel<false>, grid, dim3(256), 0, stream, parent, labels, areas,
                       status, H, W);
  UNET_CHECK_LAUNCH("cc_finish");
  return UNET_OK;
}

int cc_dispatch(const unsigned char* classes, unsigned* parent, unsigned* labels, unsigned* areas,
                unsigned* status, bool edge, int B, int K, int H, int W, int connectivity, int mode,
                hipStream_t stream) {
#define CC_CASE(C, M)                                                                         \
  if (connectivity == C && mode == M)                                                         \
    return cc_launch<C, M>(classes, parent, labels, areas, status, edge, B, K, H, W, stream);
  CC_CASE(4, MODE_FOREGROUND) CC_CASE(8, MODE_FOREGROUND) CC_CASE(4, MODE_CLASS)
  CC_CASE(8, MODE_CLASS) CC_CASE(4, MODE_BACKGROUND) CC_CASE(8, MODE_BACKGROUND)
#undef CC_CASE
  unet_set_error("cc_label: connectivity %d / mode %d", connectivity, mode);
  return UNET_E_INVALID;
}

// ---- the byte rewrites of the cleanup ----------------------------------------------------------
// All of them: grid (blocks, B), 256 threads, grid-stride over one image's pixels.

// out = in with a byte >= K read as 0 (pointwise: in == out is fine)
__global__ __launch_bounds__(256) void cleanup_copy_kernel(const unsigned char* in,
                                                           unsigned char* out, int K, int HW) {
  const size_t img = (size_t)blockIdx.y * HW;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
    const unsigned char v = in[img + p];
    out[img + p] = v < K ? v : (unsigned char)0;
  }
}

// best[b] = max over the components of (area << 32) | (0xffffffff - root): the largest component,
// ties to the smallest label.  One 64-bit atomicMax per wave.
__global__ __launch_bounds__(256) void cleanup_largest_kernel(const unsigned* __restrict__ areas,
                                                              unsigned long long* __restrict__ best,
                                                              int HW) {
  const unsigned* are = areas + (size_t)blockIdx.y * HW;
  unsigned long long m = 0;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
    const unsigned a = are[p];
    if (a) {
      const unsigned long long v = ((unsigned long long)a << 32) | (0xffffffffu - (unsigned)p);
      m = v > m ? v : m;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(m, off, 64);
    m = o > m ? o : m;
  }
  if ((threadIdx.x & 63) == 0 && m) atomicMax(&best[blockIdx.y], m);
}

// step 1: a component below min_area, or (keep_largest) any but the image's largest, becomes 0
__global__ __launch_bounds__(256) void cleanup_remove_kernel(
    unsigned char* __restrict__ map, const unsigned* __restrict__ labels,
    const unsigned* __restrict__ areas, const unsigned long long* __restrict__ best, int HW,
    unsigned min_area, int keep_largest) {
  const size_t img = (size_t)blockIdx.y * HW;
  const unsigned long long bb = keep_largest ? best[blockIdx.y] : 0ull;
  const unsigned best_root = 0xffffffffu - (unsigned)(bb & 0xffffffffull);
  for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
    const unsigned l = labels[img + p];
    if (l == 0) continue;
    const unsigned root = l - 1;
    const bool keep = areas[img + root] >= min_area && (!keep_largest || (bb && root == best_root));
    if (!keep) map[img + p] = 0;
  }
}

// votes[b][c] = pixels of class c in image b (c >= 1): a workgroup counts in LDS first
__global__ __launch_bounds__(256) void cleanup_image_votes_kernel(
    const unsigned char* __restrict__ map, unsigned* __restrict__ votes, int K, int HW) {
  __shared__ unsigned hist[UNET_MAX_CLASSES];
  if (threadIdx.x < UNET_MAX_CLASSES) hist[threadIdx.x] = 0;
  __syncthreads();
  const unsigned char* m = map + (size_t)blockIdx.y * HW;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
    const unsigned v = m[p];
    if (v != 0 && v < (unsigned)K) atomicAdd(&hist[v], 1u);
  }
  __syncthreads();
  if ((int)threadIdx.x < K && threadIdx.x > 0 && hist[threadIdx.x])
    atomicAdd(&votes[(size_t)blockIdx.y * UNET_MAX_CLASSES + threadIdx.x], hist[threadIdx.x]);
}

// every foreground pixel takes the image's winning class (most pixels, ties to the lower class)
__global__ __launch_bounds__(256) void cleanup_image_apply_kernel(unsigned char* __restrict__ map,
                                                                  const unsigned* __restrict__ votes,
                                                                  int K, int HW) {
  const unsigned* v = votes + (size_t)blockIdx.y * UNET_MAX_CLASSES;
  unsigned best = 0;
  int win = 0;
  for (int c = 1; c < K; ++c)
    if (v[c] > best) { best = v[c]; win = c; }
  if (win == 0) return;       // no foreground
  unsigned char* m = map + (size_t)blockIdx.y * HW;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256)
    if (m[p]) m[p] = (unsigned char)win;
}

// component vote, pass of class c, first half: count[root] += pixels of class c
__global__ __launch_bounds__(256) void cleanup_comp_count_kernel(
    const unsigned char* __restrict__ map, const unsigned* __restrict__ labels,
    unsigned* __restrict__ count, int c, int HW) {
  const size_t img = (size_t)blockIdx.y * HW;
  const int lane = threadIdx.x & 63;
  for (int base = blockIdx.x * 256 + (threadIdx.x & ~63); base < HW; base += gridDim.x * 256) {
    const int p = base + lane;
    unsigned key = CC_NONE;
    if (p < HW && map[img + p] == c) {
      const unsigned l = labels[img + p];
      if (l) key = l - 1;
    }
    add_by_key(count + img, key, lane);
  }
}

// second half, at the root pixels: a strictly larger count takes over (classes come in increasing
// order, so ties stay with the lower class); the counter is zeroed for the next class
__global__ __launch_bounds__(256) void cleanup_comp_update_kernel(
    const unsigned* __restrict__ labels, unsigned* __restrict__ count,
    unsigned* __restrict__ best_count, unsigned* __restrict__ best_class, int c, int HW) {
  const size_t img = (size_t)blockIdx.y * HW;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
    if (labels[img + p] != (unsigned)p + 1u) continue;
    const unsigned n = count[img + p];
    if (n == 0) continue;
    count[img + p] = 0;
    if (n > best_count[img + p]) {
      best_count[img + p] = n;
      best_class[img + p] = (unsigned)c;
    }
  }
}

__global__ __launch_bounds__(256) void cleanup_comp_apply_kernel(
    unsigned char* __restrict__ map, const unsigned* __restrict__ labels,
    const unsigned* __restrict__ best_class, int HW) {
  const size_t img = (size_t)blockIdx.y * HW;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
    if (map[img + p] == 0) continue;
    const unsigned l = labels[img + p];
    if (l) map[img + p] = (unsigned char)best_class[img + l - 1];
  }
}

// step 3: a background component that touches no edge (and is small enough) takes the class of
// the pixel left of its first pixel.  That pixel is foreground (header), and this kernel rewrites
// background pixels only: it is read as it stood before the fill without a second buffer.
__global__ __launch_bounds__(256) void cleanup_fill_kernel(unsigned char* __restrict__ map,
                                                           const unsigned* __restrict__ labels,
                                                           const unsigned* __restrict__ areas,
                                                           int HW, unsigned max_hole_area) {
  const size_t img = (size_t)blockIdx.y * HW;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
    if (map[img + p] != 0) continue;
    const unsigned l = labels[img + p];
    if (l < 2) continue;            // (root 0 is the corner: it touches the edge)
    const unsigned root = l - 1;
    const unsigned a = areas[img + root];
    if (a & CC_EDGE_BIT) continue;
    if (max_hole_area && a > max_hole_area) continue;
    map[img + p] = map[img + root - 1];
  }
}

int check_shape(const char* who, int B, int K, int H, int W) {
  UNET_REQUIRE(B >= 1 && B <= 65535, "%s: B = %d is outside 1..65535", who, B);
  UNET_REQUIRE(K >= 2 && K <= UNET_MAX_CLASSES, "%s: K = %d is outside 2..%d", who, K,
               UNET_MAX_CLASSES);
  UNET_REQUIRE(H >= 1 && H <= PP_MAX_DIM && W >= 1 && W <= PP_MAX_DIM &&
                   (long long)H * W <= PP_MAX_PIXELS,
               "%s: H = %d, W = %d (each 1..16384, H * W <= 2^30)", who, H, W);
  return UNET_OK;
}

bool shape_ok(int B, int H, int W) {
  return B >= 1 && B <= 65535 && H >= 1 && H <= PP_MAX_DIM && W >= 1 && W <= PP_MAX_DIM &&
         (long long)H * W <= PP_MAX_PIXELS;
}

// The status word (+ padding), then - mask_cleanup only - best[B] and votes[B][32], this header
// (zeroed before every call) padded to 256; then one (cc_label: the forest) or four planes.
struct PpWs { unsigned *status, *votes, *plane[4]; unsigned long long* best;
              size_t header, bytes; };
PpWs pp_ws(void* base, int B, int H, int W, bool cleanup) {
  WsLayout l(base);
  PpWs w{};
  w.status = l.take<unsigned>(PP_HEADER / sizeof(unsigned), 1);
  if (cleanup) {
    w.best = l.take<unsigned long long>(B, 1);
    w.votes = l.take<unsigned>((size_t)B * UNET_MAX_CLASSES, 1);
    l.pad(256);
  }
  w.header = l.bytes();
  for (int k = 0; k < (cleanup ? 4 : 1); ++k) w.plane[k] = l.take<unsigned>((size_t)B * H * W, 1);
  w.bytes = l.bytes();
  return w;
}

}  // namespace

extern "C" size_t unet_cc_workspace_bytes(int B, int H, int W) {
  if (!shape_ok(B, H, W)) return 0;
  return pp_ws(nullptr, B, H, W, false).bytes;
}

extern "C" int unet_cc_label_u8(const uint8_t* classes, uint32_t* labels, uint32_t* areas,
                                void* workspace, size_t workspace_bytes, int B, int K, int H,
                                int W, int connectivity, int mode, unet_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  UNET_REQUIRE(classes && labels && areas && workspace, "cc_label: null pointer");
  UNET_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(labels) & 3) == 0 &&
                   (reinterpret_cast<uintptr_t>(areas) & 3) == 0,
               "cc_label: workspace needs 16-byte, labels and areas 4-byte alignment");
  if (int rc = check_shape("cc_label", B, K, H, W)) return rc;
  UNET_REQUIRE(connectivity == 4 || connectivity == 8, "cc_label: connectivity %d is not 4 or 8",
               connectivity);
  UNET_REQUIRE(mode >= UNET_CC_FOREGROUND && mode <= UNET_CC_BACKGROUND,
               "cc_label: unknown mode %d", mode);
  const PpWs ws = pp_ws(workspace, B, H, W, false);
  UNET_REQUIRE(workspace_bytes >= ws.bytes, "cc_label: workspace of %zu bytes, %zu needed",
               workspace_bytes, ws.bytes);
  if (int rc = pp_zero(workspace, ws.header, stream)) return rc;
  return cc_dispatch(classes, ws.plane[0], labels, areas, ws.status, false, B, K, H, W,
                     connectivity, mode, stream);
}

extern "C" size_t unet_mask_cleanup_workspace_bytes(int B, int K, int H, int W) {
  if (!shape_ok(B, H, W) || K < 2 || K > UNET_MAX_CLASSES) return 0;
  return pp_ws(nullptr, B, H, W, true).bytes;
}

extern "C" int unet_mask_cleanup_u8(const uint8_t* classes_in, uint8_t* classes_out,
                                    void* workspace, size_t workspace_bytes, int B, int K, int H,
                                    int W, int connectivity, int vote, int keep_largest,
                                    int min_area, int fill_holes, int max_hole_area,
                                    unet_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  UNET_REQUIRE(classes_in && classes_out && workspace, "mask_cleanup: null pointer");
  UNET_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
               "mask_cleanup: workspace needs 16-byte alignment");
  if (int rc = check_shape("mask_cleanup", B, K, H, W)) return rc;
  UNET_REQUIRE(connectivity == 4 || connectivity == 8,
               "mask_cleanup: connectivity %d is not 4 or 8", connectivity);
  UNET_REQUIRE(vote >= UNET_VOTE_NONE && vote <= UNET_VOTE_COMPONENT,
               "mask_cleanup: unknown vote %d", vote);
  UNET_REQUIRE(min_area >= 0, "mask_cleanup: min_area %d is negative", min_area);
  UNET_REQUIRE(max_hole_area >= 0, "mask_cleanup: max_hole_area %d is negative", max_hole_area);
  const PpWs ws = pp_ws(workspace, B, H, W, true);
  UNET_REQUIRE(workspace_bytes >= ws.bytes, "mask_cleanup: workspace of %zu bytes, %zu needed",
               workspace_bytes, ws.bytes);
  const int HW = H * W;
  const size_t plane = (size_t)B * HW;
  // four planes of one word a pixel: the forest, the labels, the areas, and the component vote's
  // winning class.  The vote's counters reuse the forest and the area planes, which it no longer
  // needs; the background pass of step 3 reuses all three.
  unsigned *const p0 = ws.plane[0], *const p1 = ws.plane[1], *const p2 = ws.plane[2],
           *const p3 = ws.plane[3];
  const dim3 grid(pp_blocks(HW), B), block(256);

  if (int rc = pp_zero(workspace, ws.header, stream)) return rc;
  hipLaunchKernelGGL(cleanup_copy_kernel, grid, block, 0, stream, classes_in, classes_out, K, HW);
  UNET_CHECK_LAUNCH("cleanup_copy");
  uint8_t* map = classes_out;

  const bool removal = keep_largest || min_area > 0;
  bool labelled = false;
  if (removal) {
    if (int rc = cc_dispatch(map, p0, p1, p2, ws.status, false, B, K, H, W, connectivity,
                             MODE_FOREGROUND, stream))
      return rc;
    labelled = true;
    if (keep_largest) {
      hipLaunchKernelGGL(cleanup_largest_kernel, grid, block, 0, stream, p2, ws.best, HW);
      UNET_CHECK_LAUNCH("cleanup_largest");
    }
    hipLaunchKernelGGL(cleanup_remove_kernel, grid, block, 0, stream, map, p1, p2, ws.best, HW,
                       (unsigned)min_area, keep_largest ? 1 : 0);
    UNET_CHECK_LAUNCH("cleanup_remove");
  }
  if (vote == UNET_VOTE_IMAGE) {
    hipLaunchKernelGGL(cleanup_image_votes_kernel, grid, block, 0, stream, map, ws.votes, K, HW);
    UNET_CHECK_LAUNCH("cleanup_image_votes");
    hipLaunchKernelGGL(cleanup_image_apply_kernel, grid, block, 0, stream, map, ws.votes, K, HW);
    UNET_CHECK_LAUNCH("cleanup_image_apply");
  } else if (vote == UNET_VOTE_COMPONENT) {
    if (!labelled)
      if (int rc = cc_dispatch(map, p0, p1, p2, ws.status, false, B, K, H, W, connectivity,
                               MODE_FOREGROUND, stream))
        return rc;
    if (int rc = pp_zero(p0, plane * sizeof(unsigned), stream)) return rc;   // count
    if (int rc = pp_zero(p2, plane * sizeof(unsigned), stream)) return rc;   // ws.best count
    for (int c = 1; c < K; ++c) {
      hipLaunchKernelGGL(cleanup_comp_count_kernel, grid, block, 0, stream, map, p1, p0, c, HW);
      UNET_CHECK_LAUNCH("cleanup_comp_count");
      hipLaunchKernelGGL(cleanup_comp_update_kernel, grid, block, 0, stream, p1, p0, p2, p3, c,
                         HW);
      UNET_CHECK_LAUNCH("cleanup_comp_update");
    }
    hipLaunchKernelGGL(cleanup_comp_apply_kernel, grid, block, 0, stream, map, p1, p3, HW);
    UNET_CHECK_LAUNCH("cleanup_comp_apply");
  }
  if (fill_holes) {
    if (int rc = cc_dispatch(map, p0, p1, p2, ws.status, true, B, K, H, W,
                             connectivity == 8 ? 4 : 8, MODE_BACKGROUND, stream))
      return rc;
    hipLaunchKernelGGL(cleanup_fill_kernel, grid, block, 0, stream, map, p1, p2, HW,
                       (unsigned)max_hole_area);
    UNET_CHECK_LAUNCH("cleanup_fill");
  }
  return UNET_OK;
}
