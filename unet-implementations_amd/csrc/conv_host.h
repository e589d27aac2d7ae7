// conv_host.h — what the forward / data-gradient entry points of conv_igemm.hip assemble a launch
// from: the operand-mode record, one IgemmParams builder per role, the batch-chunk walk and the
// BSTATS binder.  Plain host code without a HIP call (tests/tools/conv_host_check.cpp runs it
// under the host sanitizers).  A new operand or flag of these entry points is threaded through
// here: a field of ConvMode / an argument of ONE builder, not a line in every export.
#pragma once
#include "conv_params.h"

namespace unet_conv {

// ---- operand mode ----------------------------------------------------------------------------
enum class Elem { F32, BF16 };           // storage of the layer tensors in HBM
enum class Cores { F32, BF16, SPLIT };   // matrix cores: fp32, bf16, three-term split bf16

struct ConvMode {
  Elem elem;
  Cores cores;
  const uint16_t* w3;   // the weights pre-split (3 planes) / pre-rounded (1 plane) to bf16, or null
  int planes;

  static ConvMode f32() { return {Elem::F32, Cores::F32, nullptr, 0}; }
  static ConvMode bf16_cores() { return {Elem::F32, Cores::BF16, nullptr, 0}; }
  static ConvMode split(const uint16_t* w3) { return {Elem::F32, Cores::SPLIT, w3, 3}; }
  static ConvMode b16(const uint16_t* wb) { return {Elem::BF16, Cores::BF16, wb, 1}; }
  // the RGB stem (K = 27, HBM-bound) stays on the fp32 matrix cores in every fp32-tensor mode
  ConvMode stem_on_fp32(int C0) const { return C0 == 3 ? f32() : *this; }

  bool b16_tensors() const { return elem == Elem::BF16; }
  bool is_split() const { return cores == Cores::SPLIT; }
  size_t es() const { return elem == Elem::BF16 ? 2 : 4; }   // bytes per tensor element
};

// ---- batch chunks ----------------------------------------------------------------------------
// Images [first, first + count) of a call.  A chunked call has no single tile layout for the
// whole batch, so the statistics / BSTATS epilogues run only in a whole one: their buffers go
// through whole().
struct Batch {
  int first, count;
  bool chunked;
  template <typename T> T* whole(T* epilogue) const { return chunked ? nullptr : epilogue; }
};

// Walks N images in chunks that keep a tensor of per_image_bytes an image inside the 2 GiB
// buffer-descriptor range (batch_chunk; unet_debug_set_chunk_limit lowers it): fn(Batch) per
// chunk, stopping at the first result other than UNET_OK.  who = the caller's name in the error.
template <typename F>
int for_each_chunk(const char* who, int N, long long per_image_bytes, F&& fn) {
  const int nmax = batch_chunk(N, per_image_bytes);
  UNET_REQUIRE(nmax >= 1, "%s: one image exceeds the 2 GiB buffer-descriptor range", who);
  for (int nb = 0; nb < N; nb += nmax) {
    const int rc = fn(Batch{nb, N - nb < nmax ? N - nb : nmax, nmax < N});
    if (rc != UNET_OK) return rc;
  }
  return UNET_OK;
}

// ---- IgemmParams builders --------------------------------------------------------------------
// (IgemmParams is a kernel argument with `float*` members for tensors of either element type; the
// builders are the one place where a `void*` tensor of the mode's type becomes such a member.)
struct ConvSrc { const void* x; int C; const float* alpha; const float* beta; };
inline ConvSrc conv_src(const unet_act_src* s) {
  return s ? ConvSrc{s->x, s->C, s->alpha, s->beta} : ConvSrc{nullptr, 0, nullptr, nullptr};
}

// image `image` of a tensor of image_bytes an image (null stays null)
inline const void* image_at(const void* base, int image, size_t image_bytes) {
  return base ? static_cast<const char*>(base) + (size_t)image * image_bytes : nullptr;
}
inline void* image_at(void* base, int image, size_t image_bytes) {
  return base ? static_cast<char*>(base) + (size_t)image * image_bytes : nullptr;
}

inline void set_w3(IgemmParams& p, const ConvMode& m, int plane) {
  if (!m.w3) return;
  p.w3 = reinterpret_cast<const __bf16*>(m.w3);
  p.w3_plane = plane;
  p.w3_bytes = (unsigned)((long long)m.planes * plane * 2);
}

inline void clear_taps(IgemmParams& p) { p.ntaps = 0; p.tapw[0] = p.tapw[1] = p.tapw[2] = 0; }

// Forward, images b of y[N][Ho][Wo][Cout] = conv_kxk(cat(act(s0), act(s1))) + bias at `stride`
// (pad k / 2): w = packed weights [k*k][Cout][C0 + C1]; a source with alpha is activated on load.
// up: s0 is [N][H/2][W/2][C0] and up-sampled by the loader (stride 1).  The caller sets p.stats.
inline IgemmParams fwd_params(const ConvSrc& s0, const ConvSrc& s1, float slope, const float* w,
                              const float* bias, void* y, Batch b, int H, int W, int Cout,
                              int stride, int ksize, bool up, const ConvMode& m) {
  const size_t es = m.es();
  const int taps = ksize * ksize, Cin = s0.C + s1.C;
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  const size_t img0 = (size_t)(up ? (H / 2) * (W / 2) : H * W) * s0.C * es;
  const size_t img1 = (size_t)H * W * s1.C * es;
  IgemmParams p{};
  p.src0 = static_cast<const float*>(image_at(s0.x, b.first, img0));
  p.src1 = static_cast<const float*>(image_at(s1.x, b.first, img1));
  p.C0 = s0.C; p.C1 = s1.C;
  p.act0_alpha = s0.alpha ? s0.alpha + (size_t)b.first * s0.C : nullptr;
  p.act0_beta = s0.alpha ? s0.beta + (size_t)b.first * s0.C : nullptr;
  p.act1_alpha = s1.alpha ? s1.alpha + (size_t)b.first * s1.C : nullptr;
  p.act1_beta = s1.alpha ? s1.beta + (size_t)b.first * s1.C : nullptr;
  p.slope = slope;
  p.w = w; p.tap_stride = Cout * Cin; p.n_off = 0; p.bias = bias;
  p.src0_bytes = (unsigned)(b.count * img0);
  p.src1_bytes = (unsigned)(b.count * img1);
  p.w_bytes = (unsigned)((long long)taps * Cout * Cin * 4);
  if (taps == 9) set_w3(p, m, 9 * Cout * Cin);
  p.out = static_cast<float*>(image_at(y, b.first, (size_t)Ho * Wo * Cout * es));
  p.ldo = Cout; p.accumulate = 0;
  p.N = b.count; p.Hin = H; p.Win = W;
  p.Hl = p.Hout = Ho; p.Wl = p.Wout = Wo;
  p.Ncols = Cout;
  p.sin = stride; p.sout = 1; p.py = p.px = 0;
  clear_taps(p);
  p.ntaps = taps;
  if (taps == 1) set_tap(p, 0, 0, 0, 0);
  else for (int t = 0; t < 9; ++t) set_tap(p, t, t / 3 - 1, t % 3 - 1, t);
  return p;
}

// Data gradient, images b of dx[N][H][W][Ccols] (+)= dy * wd over the channel slice
// [ci_offset, ci_offset + Ccols) of Cin_total: wd = packed weights [k*k][Cin_total][Cout].
//   ksize 3, stride 1: dy [N][H][W][Cout], the nine flipped taps
//   ksize 3, stride 2: dy [N][H/2][W/2][Cout] on the logical grid H/2 x W/2; the tap table is left
//     empty (set_s2_class_taps for a per-class launch; the one-launch forms carry their own)
//   ksize 1: dy [N][H][W][Cout], one tap
//   channel_taps (the up-sampled operand's gradient at low resolution): dy = D [N][H][W][9 Cout],
//     tap t reads channels [t Cout, (t + 1) Cout) of the same pixel
inline IgemmParams dgrad_params(const void* dy, const float* wd, int Cin_total, int ci_offset,
                                void* dx, Batch b, int H, int W, int Cout, int Ccols, int stride,
                                int ksize, int accumulate, bool channel_taps, const ConvMode& m) {
  const size_t es = m.es();
  const int taps = ksize * ksize;
  const int Hs = (H - 1) / stride + 1, Ws = (W - 1) / stride + 1;
  const size_t img = (size_t)Hs * Ws * (channel_taps ? 9 : 1) * Cout * es;
  IgemmParams p{};
  p.src0 = static_cast<const float*>(image_at(dy, b.first, img));
  p.src1 = nullptr; p.C0 = Cout; p.C1 = 0;
  p.w = wd; p.tap_stride = Cin_total * Cout; p.n_off = ci_offset; p.bias = nullptr;
  p.src0_bytes = (unsigned)(b.count * img);
  p.src1_bytes = 0;
  p.w_bytes = (unsigned)((long long)taps * Cout * Cin_total * 4);
  if (taps == 9) set_w3(p, m, 9 * Cout * Cin_total);
  p.out = static_cast<float*>(image_at(dx, b.first, (size_t)H * W * Ccols * es));
  p.ldo = Ccols; p.accumulate = accumulate;
  p.N = b.count; p.Hin = Hs; p.Win = Ws;
  p.Hl = H / stride; p.Wl = W / stride;
  p.Hout = H; p.Wout = W;
  p.Ncols = Ccols;
  p.sin = 1; p.sout = stride; p.py = p.px = 0;
  clear_taps(p);
  if (channel_taps) {
    p.src0_pitch = 9 * Cout; p.tap_cstride = Cout;
    p.ntaps = 9;
    for (int t = 0; t < 9; ++t) set_tap(p, t, 0, 0, t);
  } else if (taps == 1) {
    p.ntaps = 1;
    set_tap(p, 0, 0, 0, 0);
  } else if (stride == 1) {
    p.ntaps = 9;
    for (int t = 0; t < 9; ++t) set_tap(p, t, 1 - t / 3, 1 - t % 3, t);
  }
  return p;
}

// Stride-2 data gradient, parity class (py, px): dx[2a+py][2b+px] = sum over ky with (py+1-ky)
// even of dy[a + (py+1-ky)/2][..] (and likewise along x)
inline void set_s2_class_taps(IgemmParams& p, int py, int px) {
  p.py = py; p.px = px;
  clear_taps(p);
  for (int ky = 0; ky < 3; ++ky) {
    if ((py + 1 - ky) & 1) continue;
    for (int kx = 0; kx < 3; ++kx) {
      if ((px + 1 - kx) & 1) continue;
      set_tap(p, p.ntaps, (py + 1 - ky) / 2, (px + 1 - kx) / 2, ky * 3 + kx);
      ++p.ntaps;
    }
  }
}

// ---- BSTATS binder ---------------------------------------------------------------------------
// The data gradient g of a launch is final for the layer `bs` describes: binds that layer to the
// launch and turns what the launch reports into bs->tiles_out (0 = no reductions were left).
//   mode_ok   the call site's own condition (the 3x3 form has no epilogue on the bf16 cores over
//             fp32 tensors; the up-sampled form has one in every mode)
//   N, HW     batch and pixels per image of g: the summaries hold at least 64 pixels
class BsBinder {
 public:
  BsBinder(unet_bwd_stats* bs, bool mode_ok, int N, int HW, int Ccols)
      : bs_(bs),
        use_(bs && mode_ok && bs->y && bs->mean && bs->rstd && bs->gamma && bs->beta &&
             bs->partial &&
             bs->partial_bytes >= (size_t)N * ceil_div(HW, 64) * Ccols * sizeof(float2)) {}
  bool use() const { return use_; }
  void bind(IgemmParams& p) const {
    if (!use_) return;
    p.bs_y = bs_->y; p.bs_mean = bs_->mean; p.bs_rstd = bs_->rstd; p.bs_gamma = bs_->gamma;
    p.bs_beta = bs_->beta; p.bs_mask = bs_->mask; p.slope = bs_->slope;
    p.bs_partial = reinterpret_cast<float2*>(bs_->partial);
  }
  // where a launcher reports: null when the epilogue is not wanted
  int* report() { return use_ ? &reported_ : nullptr; }
  int reported() const { return reported_; }
  // the launch reported pixels per reduction tile / reduction tiles per image
  int done_px(int rc, int HW) const { return done_tiles(rc, reported_ > 0 ? HW / reported_ : 0); }
  int done_tiles(int rc, int tiles) const {
    if (rc == UNET_OK && use_ && tiles > 0) bs_->tiles_out = tiles;
    return rc;
  }
  // The four per-class launches of a stride-2 gradient: class c writes its tiles behind those of
  // the classes before it (bs_tile0); one class without the epilogue gives it up for all.
  void begin_class(IgemmParams& p, int cls) {
    reported_ = 0;
    p.bs_tile0 = cls * (class_tiles_ > 0 ? class_tiles_ : 0);
  }
  void end_class(IgemmParams& p, int HlWl) {
    if (!use_) return;
    if (reported_ == 0) { p.bs_partial = nullptr; class_tiles_ = -1; }
    else if (class_tiles_ == 0) class_tiles_ = HlWl / reported_;
  }
  void done_classes(const IgemmParams& p) const {
    if (use_ && class_tiles_ > 0 && p.bs_partial) bs_->tiles_out = 4 * class_tiles_;
  }

 private:
  unet_bwd_stats* bs_;
  bool use_;
  int reported_ = 0;
  int class_tiles_ = 0;
};

}  // namespace unet_conv
