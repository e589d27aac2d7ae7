// augment_common.h — what augment.hip, augment_post.hip and augment_light.hip share: the shape limits, the host-side
// argument checks, Philox4x32-10 and the two pixel helpers of the stages behind the gather.
#pragma once
#include "common.h"

namespace {

constexpr int AUG_MAX_DIM = 32768;             // (float)H, (float)W exact; indices fit int
constexpr long long AUG_MAX_PIXELS = 1ll << 30;

// Philox4x32-10 (Salmon et al., SC'11): counter c[4], key k[2] -> four random words.
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3,
                                              unsigned k0, unsigned k1, unsigned (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__device__ __forceinline__ unsigned char to_byte(float v) {
  return (unsigned char)fminf(fmaxf(rintf(v), 0.f), 255.f);       // fmaxf(NaN, 0) = 0
}

// -t -> t, size - 1 + t -> size - 1 - t, then into 0 .. size - 1 whatever x was
__device__ __forceinline__ int reflect(int x, int size) {
  if (x < 0) x = -x;
  if (x > size - 1) x = 2 * (size - 1) - x;
  return min(max(x, 0), size - 1);
}

bool aug_aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
bool aug_aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

// [a, a + an) and [b, b + bn) share a byte
bool aug_overlap(const void* a, size_t an, const void* b, size_t bn) {
  if (!a || !b) return false;
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + bn && y < x + an;
}

bool aug_shape_ok(int N, int H, int W) {
  return N > 0 && N <= 65535 && H > 0 && W > 0 && H <= AUG_MAX_DIM && W <= AUG_MAX_DIM &&
         (long long)H * W <= AUG_MAX_PIXELS;
}

// The host checks every entry point of a stage behind the gather makes (augment_post.hip, augment_light.hip).  `name`
// is the entry point; `record` names the stage's record ("post": [N][per_sample] floats at `rec`) and `reader` what
// reads a neighbourhood ("blur"); `need` is unet_augment_<record>_workspace_bytes(N); image_out may be null unless
// `apply`.
int aug_stage_check(const char* name, const char* record, const char* reader, bool apply, const uint8_t* image,
                    const uint8_t* image_out, const float* rec, int per_sample, const uint32_t* rng,
                    const void* workspace, size_t workspace_bytes, size_t need, int N, int H, int W) {
  UNET_REQUIRE(image && rec && (image_out || !apply), "%s: null pointer (image, image_out, %s)", name, record);
  UNET_REQUIRE(aug_shape_ok(N, H, W),
               "%s: bad shape (N in 1..65535, H, W in 1..32768, H * W <= 2^30)", name);
  UNET_REQUIRE(workspace && workspace_bytes >= need,
               "%s: workspace is null or smaller than unet_augment_%s_workspace_bytes(N) = %zu", name, record, need);
  UNET_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "%s: workspace is not 16-byte aligned", name);
  const size_t bytes = (size_t)N * H * W * 3;
  const void* ins[4] = {image, rec, rng, workspace};
  const size_t in_bytes[4] = {bytes, (size_t)N * per_sample * sizeof(float), (size_t)N * 4 * sizeof(uint32_t), need};
  for (int i = 0; i < 4; ++i)
    UNET_REQUIRE(!aug_overlap(image_out, bytes, ins[i], in_bytes[i]),
                 "%s: image_out overlaps image, %s, rng or workspace (the %s reads a neighbourhood; it cannot run "
                 "in place)", name, record, reader);
  for (int i = 0; i < 3; ++i)
    UNET_REQUIRE(!aug_overlap(workspace, need, ins[i], in_bytes[i]), "%s: workspace overlaps image, %s or rng", name,
                 record);
  return UNET_OK;
}

}  // namespace
