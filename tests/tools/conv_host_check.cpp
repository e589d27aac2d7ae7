// Stand-alone check of unet-implementations_amd/csrc/conv_host.h (the chunk walk, the two
// IgemmParams builders and the BSTATS binder): plain host code, no HIP call, no GPU.  Built with
// the host sanitizers and run by tests/test_conv_host_cpu.py:
//   hipcc -std=c++17 -Xarch_host -fsanitize=address,undefined -I<csrc> -I<include> \
//         tests/tools/conv_host_check.cpp -o conv_host_check && ./conv_host_check
// The walk runs over N = 1, 3, 8 with limits that give one, two and three chunks and a remainder;
// the visited image ranges and the byte offsets of every advanced pointer are compared with a
// straightforward loop.
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "conv_host.h"

static long long g_limit = (1LL << 31) - 1;
static char g_error[256];
long long& unet_conv::chunk_limit_bytes() { return g_limit; }
void unet_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof g_error, fmt, ap);
  va_end(ap);
}

using namespace unet_conv;

static int g_failed = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) { printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
  } while (0)

static ptrdiff_t bytes_from(const void* p, const void* base) {
  return static_cast<const char*>(p) - static_cast<const char*>(base);
}

struct Range { int first, count; bool chunked; };

// what the walk must visit: chunks of floor(limit / per_image) images, the last one shorter
static std::vector<Range> expected(int N, long long per_image, long long limit) {
  std::vector<Range> r;
  const long long fit = limit / per_image;
  const int nmax = (int)(fit < N ? fit : N);
  for (int nb = 0; nb < N; nb += nmax) r.push_back({nb, N - nb < nmax ? N - nb : nmax, nmax < N});
  return r;
}

static void check_walk(int N, int images_per_chunk, size_t es) {
  const int H = 6, W = 10, C0 = 32, C1 = 64, Cout = 96, stride = 2;
  const int Ho = 3, Wo = 5;
  const long long per_image = (long long)H * W * C1 * (long long)es;
  g_limit = per_image * images_per_chunk + per_image / 2;   // (not a multiple: floor is exercised)
  const std::vector<Range> want = expected(N, per_image, g_limit);
  // the tensors are only addressed, never read: a buffer of the full size keeps ASan honest
  std::vector<char> x0((size_t)N * H * W * C0 * es), x1((size_t)N * H * W * C1 * es),
      y((size_t)N * Ho * Wo * Cout * es);
  std::vector<float> alpha((size_t)N * C1), beta((size_t)N * C1), w(9 * Cout * (C0 + C1));
  std::vector<float2> stats(16);
  const ConvMode m = es == 2 ? ConvMode::b16(nullptr) : ConvMode::f32();
  std::vector<Range> got;
  const int rc = for_each_chunk("check", N, per_image, [&](Batch b) {
    got.push_back({b.first, b.count, b.chunked});
    const IgemmParams p =
        fwd_params({x0.data(), C0, nullptr, nullptr}, {x1.data(), C1, alpha.data(), beta.data()},
                   0.01f, w.data(), nullptr, y.data(), b, H, W, Cout, stride, 3, false, m);
    CHECK(bytes_from(p.src0, x0.data()) == (ptrdiff_t)((size_t)b.first * H * W * C0 * es));
    CHECK(bytes_from(p.src1, x1.data()) == (ptrdiff_t)((size_t)b.first * H * W * C1 * es));
    CHECK(bytes_from(p.out, y.data()) == (ptrdiff_t)((size_t)b.first * Ho * Wo * Cout * es));
    CHECK(p.act1_alpha == alpha.data() + (size_t)b.first * C1);
    CHECK(p.act1_beta == beta.data() + (size_t)b.first * C1);
    CHECK(p.act0_alpha == nullptr && p.act0_beta == nullptr);
    CHECK(p.src0_bytes == (unsigned)((size_t)b.count * H * W * C0 * es));
    CHECK(p.src1_bytes == (unsigned)((size_t)b.count * H * W * C1 * es));
    CHECK((long long)p.src1_bytes <= g_limit);
    CHECK(bytes_from(p.src1, x1.data()) + p.src1_bytes <= (ptrdiff_t)x1.size());
    CHECK(bytes_from(p.out, y.data()) + (ptrdiff_t)((size_t)b.count * Ho * Wo * Cout * es) <=
          (ptrdiff_t)y.size());
    CHECK(p.N == b.count && p.Hl == Ho && p.Wl == Wo && p.sin == stride && p.ntaps == 9);
    // the epilogue buffers survive in a whole call only
    CHECK(b.whole(stats.data()) == (b.chunked ? nullptr : stats.data()));
    return UNET_OK;
  });
  CHECK(rc == UNET_OK);
  CHECK(got.size() == want.size());
  for (size_t i = 0; i < got.size() && i < want.size(); ++i)
    CHECK(got[i].first == want[i].first && got[i].count == want[i].count &&
          got[i].chunked == want[i].chunked);

  // the data gradient over the same split: dy at the strided size, dx at the full one
  std::vector<char> dy((size_t)N * Ho * Wo * Cout * es), dx((size_t)N * H * W * C0 * es);
  std::vector<float> wd(9 * (C0 + C1) * Cout);
  int visited = 0;
  CHECK(for_each_chunk("check", N, per_image, [&](Batch b) {
          IgemmParams p = dgrad_params(dy.data(), wd.data(), C0 + C1, C1, dx.data(), b, H, W, Cout,
                                       C0, stride, 3, 1, false, m);
          CHECK(bytes_from(p.src0, dy.data()) == (ptrdiff_t)((size_t)b.first * Ho * Wo * Cout * es));
          CHECK(bytes_from(p.out, dx.data()) == (ptrdiff_t)((size_t)b.first * H * W * C0 * es));
          CHECK(p.src0_bytes == (unsigned)((size_t)b.count * Ho * Wo * Cout * es));
          CHECK(p.n_off == C1 && p.ldo == C0 && p.Ncols == C0 && p.accumulate == 1);
          CHECK(p.Hl == H / 2 && p.Wl == W / 2 && p.sout == 2 && p.ntaps == 0);
          int taps = 0;
          for (int cls = 0; cls < 4; ++cls) { set_s2_class_taps(p, cls >> 1, cls & 1); taps += p.ntaps; }
          CHECK(taps == 9);
          visited += b.count;
          return UNET_OK;
        }) == UNET_OK);
  CHECK(visited == N);
}

static void check_too_large_and_stop() {
  g_limit = 100;
  int calls = 0;
  CHECK(for_each_chunk("conv_x", 4, 101, [&](Batch) { ++calls; return UNET_OK; }) == UNET_E_INVALID);
  CHECK(calls == 0);
  CHECK(std::string(g_error) == "conv_x: one image exceeds the 2 GiB buffer-descriptor range");
  // a failing chunk ends the walk with its code
  CHECK(for_each_chunk("conv_x", 4, 50, [&](Batch b) {
          ++calls;
          return b.first == 2 ? UNET_E_LAUNCH : UNET_OK;
        }) == UNET_E_LAUNCH);
  CHECK(calls == 2);
  g_limit = (1LL << 31) - 1;
}

static void check_variants() {
  std::vector<char> D(2 * 4 * 4 * 9 * 32 * 2), g(2 * 4 * 4 * 64 * 2);
  std::vector<float> wd(9 * 64 * 32);
  std::vector<uint16_t> wb(9 * 64 * 32);
  const Batch whole{0, 2, false};
  IgemmParams p = dgrad_params(D.data(), wd.data(), 64, 0, g.data(), whole, 4, 4, 32, 64, 1, 3, 0,
                               true, ConvMode::b16(wb.data()));
  CHECK(p.tap_cstride == 32 && p.src0_pitch == 9 * 32 && p.ntaps == 9 && p.Hin == 4 && p.sout == 1);
  CHECK(p.src0_bytes == D.size() && p.w3_plane == 9 * 64 * 32 && p.w3_bytes == 2u * 9 * 64 * 32);
  p = dgrad_params(D.data(), wd.data(), 64, 32, g.data(), whole, 4, 4, 32, 32, 1, 1, 0, false,
                   ConvMode::f32());
  CHECK(p.ntaps == 1 && p.w_bytes == 4u * 64 * 32 && p.w3 == nullptr && p.n_off == 32);
  // the fused up-sampling forward: source 0 at half resolution
  std::vector<float> low(2 * 2 * 2 * 32), skip(2 * 4 * 4 * 32), y(2 * 4 * 4 * 32), w(9 * 32 * 64);
  std::vector<uint16_t> w3(3 * 9 * 32 * 64);
  p = fwd_params({low.data(), 32, nullptr, nullptr}, {skip.data(), 32, nullptr, nullptr}, 0.f,
                 w.data(), nullptr, y.data(), whole, 4, 4, 32, 1, 3, true, ConvMode::split(w3.data()));
  CHECK(p.src0_bytes == low.size() * 4 && p.src1_bytes == skip.size() * 4 && p.Hin == 4);
  CHECK(p.w3_bytes == w3.size() * 2 && p.w3_plane == 9 * 32 * 64);
  CHECK(ConvMode::split(w3.data()).stem_on_fp32(3).w3 == nullptr);
  CHECK(ConvMode::bf16_cores().stem_on_fp32(32).cores == Cores::BF16);
}

static void check_bs_binder() {
  float buf[8];
  const int N = 2, HW = 256, C = 32;
  unet_bwd_stats bs{};
  bs.y = bs.mean = bs.rstd = bs.gamma = bs.beta = buf;
  bs.partial = buf;
  bs.partial_bytes = (size_t)N * (HW / 64) * C * sizeof(float2);
  bs.slope = 0.25f;
  bs.tiles_out = 0;
  IgemmParams p{};
  {
    BsBinder b(&bs, true, N, HW, C);
    CHECK(b.use() && b.report() != nullptr);
    b.bind(p);
    CHECK(p.bs_y == buf && p.bs_partial == reinterpret_cast<float2*>(buf) && p.slope == 0.25f);
    *b.report() = 128;
    CHECK(b.done_px(UNET_E_LAUNCH, HW) == UNET_E_LAUNCH && bs.tiles_out == 0);
    CHECK(b.done_px(UNET_OK, HW) == UNET_OK && bs.tiles_out == 2);
  }
  bs.tiles_out = 0;
  CHECK(!BsBinder(&bs, false, N, HW, C).use());       // a mode without the epilogue
  CHECK(!BsBinder(nullptr, true, N, HW, C).use());    // nothing asked for (or a chunked call)
  bs.partial_bytes -= 1;
  CHECK(!BsBinder(&bs, true, N, HW, C).use());        // the summaries do not fit
  bs.partial_bytes += 1;
  {   // four per-class launches of 2 tiles each
    BsBinder b(&bs, true, N, HW, C);
    IgemmParams q{};
    b.bind(q);
    for (int cls = 0; cls < 4; ++cls) {
      b.begin_class(q, cls);
      CHECK(q.bs_tile0 == (cls == 0 ? 0 : cls * 2));
      *b.report() = 32;
      b.end_class(q, HW / 4);
    }
    b.done_classes(q);
    CHECK(bs.tiles_out == 8);
  }
  bs.tiles_out = 0;
  {   // one class reports no epilogue: given up for all
    BsBinder b(&bs, true, N, HW, C);
    IgemmParams q{};
    b.bind(q);
    for (int cls = 0; cls < 4; ++cls) {
      b.begin_class(q, cls);
      if (cls != 1) *b.report() = 32;
      b.end_class(q, HW / 4);
    }
    b.done_classes(q);
    CHECK(bs.tiles_out == 0 && q.bs_partial == nullptr);
  }
}

int main() {
  for (size_t es : {(size_t)4, (size_t)2})
    for (int N : {1, 3, 8})
      for (int per_chunk : {8, 4, 3, 2, 1}) check_walk(N, per_chunk, es);
  check_too_large_and_stop();
  check_variants();
  check_bs_binder();
  printf(g_failed ? "%d checks failed\n" : "conv_host_check: ok\n", g_failed);
  return g_failed ? 1 : 0;
}
