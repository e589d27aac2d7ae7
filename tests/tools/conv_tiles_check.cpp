// Stand-alone run of the tile choosers of unet-implementations_amd/csrc/conv_tiles.h (plain host
// code, no HIP call, no GPU) on IgemmParams built by the conv_host.h builders.  Built with the
// host sanitizers and fed by tests/test_conv_tiles_cpu.py, which holds every answer to the
// kernel instantiation recorded on the GPU for the same call (tests/data/conv_host_gpu.json):
//   hipcc -std=c++17 -Xarch_host -fsanitize=address,undefined -I<csrc> -I<include> \
//         tests/tools/conv_tiles_check.cpp -o conv_tiles_check && ./conv_tiles_check < queries
// A query is one line "id chooser kind N H W A B C stride ksize es w3 act0 act1":
//   kind fwd / up   forward (up: source 0 at half resolution): C0 = A, C1 = B, Cout = C
//   kind dgrad      data gradient: Cout = A, Ccols = B, Cin_total = C
//   es              bytes per tensor element; w3: the bf16 weight plane(s) are given
// The answer "id chooser pick": the tile as "BN WM WN TH" (patch) or "BM BN WM WN KG"
// (gather-GEMM), "none" (no rung of the ladder), "n/a" (the shape does not apply to the family).
#include <cstdio>
#include <cstring>
#include <string>

#include "conv_host.h"
#include "conv_tiles.h"

static long long g_limit = (1LL << 31) - 1;
long long& unet_conv::chunk_limit_bytes() { return g_limit; }
void unet_set_error(const char*, ...) {}

using namespace unet_conv;

// the tensors are only addressed, never read: one 16-byte aligned object stands for all of them
alignas(16) static float g_buf[4];

template <size_t N>
static std::string patch_pick(const PatchRule (&rules)[N], int idx) {
  if (idx == kNoRule) return "none";
  if (idx < 0 || idx >= (int)N) return "out of range";
  const PatchRule& r = rules[idx];
  char s[64];
  snprintf(s, sizeof s, "%d %d %d %d", r.bn, r.wm, r.wn, r.th);
  return s;
}

static std::string gemm_pick(const IgemmParams& p, bool k_groups) {
  const GemmTile t = gemm_tile(p);
  char s[64];
  // (with_gemm_tile_kg is what the launchers instantiate from: ask it, not a copy of its table)
  with_gemm_tile_kg(t, p, [&](auto shape, auto groups) {
    using S = decltype(shape);
    snprintf(s, sizeof s, "%d %d %d %d %d", S::BM, S::BN, S::WM, S::WN,
             k_groups ? (int)decltype(groups)::value : 1);
    return 0;
  });
  return s;
}

static std::string answer(const std::string& chooser, const IgemmParams& p) {
  if (chooser == "f32")
    return patch_f32_applicable(p) ? patch_pick(kPatchF32, pick_patch_f32(p)) : "n/a";
  if (chooser == "up")
    return patch_up_applicable(p) ? patch_pick(kPatchF32, pick_patch_up(p)) : "n/a";
  if (chooser == "s2")
    return patch_s2_applicable(p) ? patch_pick(kPatchS2, pick_patch_s2(p)) : "n/a";
  if (chooser == "dgrad_s2") return patch_pick(kDgradS2, pick_dgrad_s2_patch(p));
  if (chooser == "b16") return patch_pick(kPatchB16, pick_patch_b16(p));
  if (chooser == "b16_up") return patch_pick(kPatchB16Up, pick_patch_b16_up(p));
  if (chooser == "b16_s2") return patch_pick(kPatchB16S2, pick_patch_b16_s2(p));
  if (chooser == "split_fused")
    return patch_split_applicable(p) ? patch_pick(kPatchSplitFused, pick_patch_split_fused(p))
                                     : "n/a";
  if (chooser == "split")
    return patch_split_applicable(p) ? patch_pick(kPatchSplit, pick_patch_split(p)) : "n/a";
  if (chooser == "gemm_kg") return gemm_pick(p, true);
  if (chooser == "gemm") return gemm_pick(p, false);
  return "unknown chooser";
}

int main() {
  char chooser[32], kind[32];
  int id, N, H, W, A, B, C, stride, ksize, es, w3, act0, act1, answered = 0;
  while (scanf("%d %31s %31s %d %d %d %d %d %d %d %d %d %d %d %d", &id, chooser, kind, &N, &H, &W,
               &A, &B, &C, &stride, &ksize, &es, &w3, &act0, &act1) == 15) {
    const uint16_t* planes = w3 ? reinterpret_cast<const uint16_t*>(g_buf) : nullptr;
    const ConvMode m = es == 2 ? ConvMode::b16(planes) : w3 ? ConvMode::split(planes) : ConvMode::f32();
    const Batch whole{0, N, false};
    IgemmParams p;
    if (!strcmp(kind, "dgrad")) {
      p = dgrad_params(g_buf, g_buf, C, 0, g_buf, whole, H, W, A, B, stride, ksize, 0, false, m);
    } else {
      const ConvSrc s0{g_buf, A, act0 ? g_buf : nullptr, act0 ? g_buf : nullptr};
      const ConvSrc s1{B ? g_buf : nullptr, B, act1 ? g_buf : nullptr, act1 ? g_buf : nullptr};
      p = fwd_params(s0, s1, 0.01f, g_buf, g_buf, g_buf, whole, H, W, C, stride, ksize,
                     !strcmp(kind, "up"), m);
    }
    printf("%d %s %s\n", id, chooser, answer(chooser, p).c_str());
    ++answered;
  }
  printf("conv_tiles_check: %d answers\n", answered);
  return 0;
}
