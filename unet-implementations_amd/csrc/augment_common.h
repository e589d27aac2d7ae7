// augment_common.h — what augment.hip, augment_post.hip and augment_light.hip share: the shape limits, the host-side
// argument checks and Philox4x32-10.
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

}  // namespace
