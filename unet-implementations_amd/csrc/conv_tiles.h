// conv_tiles.h — which kernel instantiation a forward / data-gradient launch gets: the
// gather-GEMM ladder, the patch ladders as tables of rule rows, the applicability tests in front
// of them and the epilogue binder.  Plain host code without a HIP call
// (tests/tools/conv_tiles_check.cpp runs the choosers under the host sanitizers).
// A new tile is a row of a table here: the launchers instantiate their kernels from the rows
// (with_patch_rule), so the ladder and the instantiation list cannot drift.
#pragma once
#include "conv_params.h"

#include <iterator>
#include <utility>

namespace unet_conv {

// ---- gather-GEMM ladder ----------------------------------------------------------------------
// Largest tile that still yields >= 256 workgroups (one per CU); layers of at most 128 x 256
// rows take the 64 x 64 tile (K groups: deep_k_groups, for the families that have them).
enum class GemmTile { M128N128, M128N64, M64N64, M128N32 };
inline GemmTile gemm_tile(long long M, int nc) {
  if (nc % 128 == 0 && ceil_div64(M, 128) * (nc / 128) >= 256) return GemmTile::M128N128;
  if (nc % 64 == 0 && ceil_div64(M, 128) * (nc / 64) >= 256) return GemmTile::M128N64;
  if (nc % 64 == 0 && M <= 128 * 256) return GemmTile::M64N64;
  return GemmTile::M128N32;
}
inline GemmTile gemm_tile(const IgemmParams& p) {
  return gemm_tile((long long)p.N * p.Hl * p.Wl, p.Ncols);
}
// the two rungs of 128 rows (a family's extra rungs sit behind them, before 64 x 64)
inline bool fills_128_rows(GemmTile t) { return t == GemmTile::M128N128 || t == GemmTile::M128N64; }

template <int BM_, int BN_, int WM_, int WN_>
struct GemmShape { static constexpr int BM = BM_, BN = BN_, WM = WM_, WN = WN_; };
// f(GemmShape<...>{}) for the tile class t
template <typename F>
int with_gemm_tile(GemmTile t, F&& f) {
  switch (t) {
    case GemmTile::M128N128: return f(GemmShape<128, 128, 64, 64>{});
    case GemmTile::M128N64: return f(GemmShape<128, 64, 64, 32>{});
    case GemmTile::M64N64: return f(GemmShape<64, 64, 32, 32>{});
    default: return f(GemmShape<128, 32, 32, 32>{});
  }
}
// f(GemmShape<...>{}, integral_constant<int, KG>{}) for the families with K groups: the 64 x 64
// tile of a deep layer is shared by deep_k_groups(p) groups of four waves, every other tile by one
template <typename F>
int with_gemm_tile_kg(GemmTile t, const IgemmParams& p, F&& f) {
  using One = std::integral_constant<int, 1>;
  if (t != GemmTile::M64N64) return with_gemm_tile(t, [&](auto shape) { return f(shape, One{}); });
  const int kg = deep_k_groups(p);
  using Deep = GemmShape<64, 64, 32, 32>;
  return kg == 4   ? f(Deep{}, std::integral_constant<int, 4>{})
         : kg == 2 ? f(Deep{}, std::integral_constant<int, 2>{})
                   : f(Deep{}, One{});
}

// ---- applicability ---------------------------------------------------------------------------
// stride-1 3x3 over an image that tiles as 4 x 32 pixels, 16-channel chunks
inline bool patch_split_applicable(const IgemmParams& p) {
  return p.ntaps == 9 && p.sin == 1 && p.sout == 1 && p.Hl == p.Hin && p.Wl == p.Win &&
         p.Hl == p.Hout && p.Wl == p.Wout && p.Hin % 4 == 0 && p.Win % 32 == 0 &&
         p.C0 % 16 == 0 && p.C1 % 16 == 0;
}
// the same with 32-channel chunks (fp32 form)
inline bool patch_f32_applicable(const IgemmParams& p) {
  return p.ntaps == 9 && p.tap_cstride == 0 && p.sin == 1 && p.sout == 1 &&
         p.Hl == p.Hin && p.Wl == p.Win && p.Hl == p.Hout && p.Wl == p.Wout && p.Hin % 4 == 0 &&
         p.Win % 32 == 0 && p.C0 % 32 == 0 && p.C1 % 32 == 0;
}
// stride-2 3x3 forward whose OUTPUT tiles as 4 x 32 pixels, 16-channel chunks, standard taps
inline bool patch_s2_applicable(const IgemmParams& p) {
  IgemmParams std_taps{};
  for (int t = 0; t < 9; ++t) set_tap(std_taps, t, t / 3 - 1, t % 3 - 1, t);
  return p.ntaps == 9 && p.tap_cstride == 0 && p.src0_pitch == 0 && p.sin == 2 &&
         p.sout == 1 && p.Hin == 2 * p.Hl && p.Win == 2 * p.Wl && p.Hl == p.Hout &&
         p.Wl == p.Wout && p.Hl % 4 == 0 && p.Wl % 32 == 0 && p.C0 % 16 == 0 && p.C1 % 16 == 0 &&
         !p.accumulate && p.tapw[0] == std_taps.tapw[0] && p.tapw[1] == std_taps.tapw[1] &&
         p.tapw[2] == std_taps.tapw[2];
}

// ---- patch ladders ---------------------------------------------------------------------------
// A rung: output tile of th x 32 pixels by bn columns, four waves of wm pixels x wn columns.  It
// is taken when the column rule holds, the image has whole tiles of th rows (`tall`: the ladders
// are entered with H % 4 == 0, so only the 8-row rungs and the stride-2 gradient ask), the bf16
// weight plane is there if the rung needs it, and the launch has at least `floor` tiles.
enum class Cols { MultipleOfBN, Exactly32 };
struct PatchRule {
  int bn, wm, wn, th;
  Cols cols;
  bool tall;
  bool w3;
  int floor;
  constexpr int px() const { return th * 32; }   // pixels of a statistics / reduction tile
};
constexpr int kNoRule = -1;

// first rung of `rules` for M output pixels in images of H rows and nc columns, or kNoRule
template <size_t N>
constexpr int first_patch_rule(const PatchRule (&rules)[N], long long M, int nc, int H, bool w3) {
  for (size_t i = 0; i < N; ++i) {
    const PatchRule& r = rules[i];
    if (r.cols == Cols::MultipleOfBN ? nc % r.bn != 0 : nc != 32) continue;
    if (r.tall && H % r.th != 0) continue;
    if (r.w3 && !w3) continue;
    if ((M / r.px()) * (nc / r.bn) >= r.floor) return (int)i;
  }
  return kNoRule;
}
constexpr Cols kMul = Cols::MultipleOfBN, k32 = Cols::Exactly32;
//                                             bn   wm  wn th cols  tall   w3     floor
// fp32 (conv_patch_f32_kernel): measured +5..19 % over the gather-GEMM at 64 and 128 columns,
// +8 % at 32 columns when K > 32.  The same tile choice with the up-sampling in the loader
// (conv_patch_up_kernel), where the Winograd kernel of the (64 up + 32) -> 32 layer is an
// explicit rung of the launcher in front of row kPatchUpWinoBefore.
inline constexpr PatchRule kPatchF32[] = {{128, 64, 64, 4, kMul, false, false, 512},
                                          {64, 64, 32, 4, kMul, false, false, 512},
                                          {32, 64, 32, 8, k32, true, false, 512}};
constexpr int kPatchUpWinoBefore = 2;
// fp32 stride-2 forward (conv_patch_s2_kernel)
inline constexpr PatchRule kPatchS2[] = {{128, 64, 64, 4, kMul, false, false, 512},
                                         {64, 64, 32, 4, kMul, false, false, 512}};
// stride-2 data gradient (conv_dgrad_s2_patch_kernel and its bf16 twin)
inline constexpr PatchRule kDgradS2[] = {{64, 32, 64, 4, kMul, true, false, 256},
                                         {32, 64, 32, 8, k32, true, false, 256}};
// bf16 tensors (conv_patch_b16_kernel).  8 x 32-pixel tiles of 64 columns where they still give
// two workgroups per CU: half the weight-panel traffic (L2 -> LDS) per output of the 4 x 32
// tiles; measured -2..-16 % per launch on the 64..256-channel layers, -0.13 ms per step
// (profiles/r04_bf16_experiments.txt).  That tile exists for the pre-rounded panels only: its
// fused form with fp32 panels spills.
inline constexpr PatchRule kPatchB16[] = {{64, 64, 64, 8, kMul, true, true, 512},
                                          {128, 64, 64, 4, kMul, false, false, 256},
                                          {64, 64, 32, 4, kMul, false, false, 256},
                                          {32, 64, 32, 8, k32, true, false, 256}};
// ... with the up-sampling in the loader (UP; the weight plane is required up front)
inline constexpr PatchRule kPatchB16Up[] = {{64, 64, 64, 8, kMul, true, true, 512},
                                            {64, 64, 32, 4, kMul, false, true, 256},
                                            {32, 64, 32, 8, k32, true, true, 256}};
// ... stride-2 fused forward (SD = 2)
inline constexpr PatchRule kPatchB16S2[] = {{64, 64, 32, 4, kMul, false, true, 512}};
// split-bf16, fused pipeline (conv_patch_split_kernel with an epilogue).  Narrow outputs: taller
// tiles (two or four patch rows per wave) cut the LDS reads per MFMA
inline constexpr PatchRule kPatchSplitFused[] = {{128, 64, 64, 4, kMul, false, false, 512},
                                                 {64, 128, 32, 8, kMul, true, false, 512},
                                                 {64, 64, 32, 4, kMul, false, false, 256},
                                                 {32, 64, 32, 8, k32, true, false, 512}};
// split-bf16, plain: every shape that applies gets a tile (two rungs without a floor)
inline constexpr PatchRule kPatchSplit[] = {{128, 64, 64, 4, kMul, false, false, 512},
                                            {64, 128, 32, 8, kMul, true, false, 512},
                                            {64, 64, 32, 4, kMul, false, false, 0},
                                            {32, 64, 32, 8, kMul, true, false, 512},
                                            {32, 32, 32, 4, kMul, false, false, 0}};

// Row I of a table as compile-time constants: what a launcher instantiates its kernel from
// (with_patch_rule names every row, so the assertion covers the whole table).
template <const auto& Rules, size_t I>
struct PatchTile {
  static constexpr PatchRule rule = Rules[I];
  static constexpr int BN = rule.bn, WM = rule.wm, WN = rule.wn, TH = rule.th, PX = rule.px();
  static constexpr bool W3 = rule.w3;
  static_assert((PX / WM) * (BN / WN) == 4, "a rung is four waves of WM pixels x WN columns");
};
template <const auto& Rules, typename F, size_t... I>
int with_patch_rule_impl(int idx, F&& f, std::index_sequence<I...>) {
  int rc = kNoTileFits;
  (void)((idx == (int)I && (rc = f(PatchTile<Rules, I>{}), true)) || ...);
  return rc;
}
// f(PatchTile<Rules, idx>{}) for a run-time row index; kNoTileFits for kNoRule
template <const auto& Rules, typename F>
int with_patch_rule(int idx, F&& f) {
  return with_patch_rule_impl<Rules>(idx, f, std::make_index_sequence<std::size(Rules)>{});
}

// ---- the choosers: a family's conditions in front of its table --------------------------------
inline long long out_pixels(const IgemmParams& p) { return (long long)p.N * p.Hl * p.Wl; }

inline int pick_patch_f32(const IgemmParams& p) {   // (callers test patch_f32_applicable)
  return first_patch_rule(kPatchF32, out_pixels(p), p.Ncols, p.Hin, false);
}
inline bool patch_up_applicable(const IgemmParams& p) {
  return p.Hin % 4 == 0 && p.Win % 32 == 0 && p.C0 % 32 == 0 && p.C1 % 32 == 0 && p.C0 >= 32;
}
inline int pick_patch_up(const IgemmParams& p) {    // (callers test patch_up_applicable)
  return pick_patch_f32(p);
}
inline int pick_patch_s2(const IgemmParams& p) {    // (callers test patch_s2_applicable)
  return first_patch_rule(kPatchS2, out_pixels(p), p.Ncols, p.Hl, false);
}
// p describes the dy grid (Hl x Wl, K = C0) and dx = (2 Hl) x (2 Wl) x Ncols
inline int pick_dgrad_s2_patch(const IgemmParams& p) {
  if (p.Wl % 32 != 0 || p.C0 % 32 != 0 || p.Hout != 2 * p.Hl || p.Wout != 2 * p.Wl)
    return kNoRule;
  return first_patch_rule(kDgradS2, out_pixels(p), p.Ncols, p.Hl, false);
}
inline int pick_patch_b16(const IgemmParams& p) {
  if (!patch_f32_applicable(p) || p.src0_pitch) return kNoRule;
  return first_patch_rule(kPatchB16, out_pixels(p), p.Ncols, p.Hin, p.w3 != nullptr);
}
inline bool b16_out_aligned(const IgemmParams& p) {   // 16-byte rows of the output tile
  return !(p.ldo & 7) && !(reinterpret_cast<uintptr_t>(p.out) & 15);
}
inline int pick_patch_b16_up(const IgemmParams& p) {
  if (p.Hin % 4 || p.Win % 32 || p.C0 % 32 || p.C1 % 32 || p.C0 < 32 || !p.act0_alpha ||
      (p.C1 && !p.act1_alpha) || p.accumulate || !b16_out_aligned(p))
    return kNoRule;
  return first_patch_rule(kPatchB16Up, (long long)p.N * p.Hin * p.Win, p.Ncols, p.Hin,
                          p.w3 != nullptr);
}
inline int pick_patch_b16_s2(const IgemmParams& p) {
  if (!patch_s2_applicable(p) || p.C0 % 32 || p.C1 % 32 || !b16_out_aligned(p)) return kNoRule;
  return first_patch_rule(kPatchB16S2, out_pixels(p), p.Ncols, p.Hl, p.w3 != nullptr);
}
inline int pick_patch_split_fused(const IgemmParams& p) {   // (patch_split_applicable)
  return first_patch_rule(kPatchSplitFused, out_pixels(p), p.Ncols, p.Hin, false);
}
inline int pick_patch_split(const IgemmParams& p) {         // (patch_split_applicable)
  return first_patch_rule(kPatchSplit, out_pixels(p), p.Ncols, p.Hin, false);
}

// ---- epilogue binder -------------------------------------------------------------------------
// What a patch launch does besides the convolution.  The kernels with ACT / STATS / BSTATS flags
// read p.stats only under STATS and p.bs_partial only under BSTATS, and the kernels without the
// flags read only the pointer of their own role, so the pointer of the other role is always
// nulled here.
enum class Epilogue {
  Plain,      // no epilogue
  FusedFwd,   // statistics of the output into p.stats; *report = pixels per statistics tile
  DgradBs     // BSTATS reductions into p.bs_partial; *report = pixels per reduction tile
};
// the role of a launcher called with (stats_px, bs_px)
inline Epilogue patch_role(const IgemmParams& p, const int* stats_px, const int* bs_px) {
  return stats_px ? Epilogue::FusedFwd : bs_px && p.bs_partial ? Epilogue::DgradBs : Epilogue::Plain;
}
// f(fused, bstats) as compile-time bools: the ACT / STATS and BSTATS flags of a role's kernel
template <typename F>
int with_role(Epilogue role, F&& f) {
  switch (role) {
    case Epilogue::FusedFwd: return f(std::true_type{}, std::false_type{});
    case Epilogue::DgradBs: return f(std::false_type{}, std::true_type{});
    default: return f(std::false_type{}, std::false_type{});
  }
}
// tiles of px pixels, tiles_per_image of them; report may be null for DgradBs (no reductions
// wanted) and is not written for Plain
inline void bind_epilogue(IgemmParams& p, Epilogue role, int px, int tiles_per_image, int* report) {
  switch (role) {
    case Epilogue::FusedFwd:
      *report = p.stats ? px : 0;
      p.stats_tiles = tiles_per_image;
      p.bs_partial = nullptr;
      return;
    case Epilogue::DgradBs:
      p.stats = nullptr;
      if (report && p.bs_partial) { *report = px; p.bs_tiles = tiles_per_image; p.bs_tile0 = 0; }
      else { if (report) *report = 0; p.bs_partial = nullptr; }
      return;
    case Epilogue::Plain:
      p.stats = nullptr;
      p.bs_partial = nullptr;
      return;
  }
}

// The gather-GEMM kernels emit their epilogue only where every BM-row tile lies inside one image:
// the fused forward (stats_px) reports BM pixels per statistics tile or 0 (the caller then runs
// the stand-alone statistics kernel), a data gradient with bs_px the same for its reductions
// (the four per-class launches of a stride-2 gradient pass bs_tile0 themselves).
inline void bind_gemm_epilogue(IgemmParams& p, int BM, int* stats_px, int* bs_px) {
  const int HlWl = p.Hl * p.Wl;
  const bool whole = HlWl % BM == 0;
  if (stats_px) {
    const bool direct = p.sout == 1 && p.Hl == p.Hout && p.Wl == p.Wout;
    if (direct && p.stats && whole) { *stats_px = BM; p.stats_tiles = HlWl / BM; }
    else { *stats_px = 0; p.stats = nullptr; }
    p.bs_partial = nullptr;
  } else if (bs_px && p.bs_partial && whole) {
    *bs_px = BM; p.bs_tiles = HlWl / BM * (p.sout * p.sout);
  } else {
    if (bs_px) *bs_px = 0;
    p.bs_partial = nullptr;
  }
}

}  // namespace unet_conv
