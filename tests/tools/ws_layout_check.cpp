// ws_layout_check: csrc/ws_layout.h in a program of its own, for a host sanitizer build
// (AddressSanitizer + UBSan, tests/test_workspace_layout_cpu.py).  Region lists over element sizes
// 1, 4, 8 and 16, roundings 1, 16 and 256 and counts that include 0 are measured over a null
// base, allocated with exactly the measured size, carved, and checked: the carve advances as the
// measure did, the regions lie in order, disjoint and inside the block, and every byte of every
// region is written.  A byte past the block is AddressSanitizer's to report.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ws_layout.h"

namespace {

struct E16 { unsigned char b[16]; };
struct Region { int elem; size_t count, round; };
struct Span { char* p; size_t bytes; };

// the list's take() calls, in order (plus a pad() where round is 0: count is then its rounding)
size_t layout(void* base, const Region* r, int n, Span* out) {
  WsLayout l(base);
  for (int i = 0; i < n; ++i) {
    void* p = nullptr;
    if (r[i].round == 0) { l.pad(r[i].count); out[i] = Span{nullptr, 0}; continue; }
    switch (r[i].elem) {
      case 1: p = l.take<unsigned char>(r[i].count, r[i].round); break;
      case 4: p = l.take<uint32_t>(r[i].count, r[i].round); break;
      case 8: p = l.take<uint64_t>(r[i].count, r[i].round); break;
      default: p = l.take<E16>(r[i].count, r[i].round); break;
    }
    out[i] = Span{static_cast<char*>(p), r[i].count * (size_t)r[i].elem};
  }
  return l.bytes();
}

uint32_t rng_state = 12345u;
uint32_t rnd() { return rng_state = rng_state * 1664525u + 1013904223u; }

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      printf("ws_layout_check: list %d: %s fails\n", list, #cond);           \
      return 1;                                                              \
    }                                                                        \
  } while (0)

}  // namespace

int main() {
  static const int kElems[4] = {1, 4, 8, 16};
  static const size_t kRounds[3] = {1, 16, 256};
  static const size_t kCounts[8] = {0, 1, 3, 16, 17, 255, 256, 1000};
  const int kLists = 400, kMaxRegions = 8;
  size_t most = 0;
  for (int list = 0; list < kLists; ++list) {
    Region r[kMaxRegions];
    Span none[kMaxRegions], got[kMaxRegions];
    const int n = 1 + (int)(rnd() >> 8) % kMaxRegions;
    for (int i = 0; i < n; ++i) {
      // the first twelve lists walk element size x rounding with one region of 17 elements
      r[i].elem = list < 12 ? kElems[list % 4] : kElems[(rnd() >> 8) % 4];
      r[i].round = list < 12 ? kRounds[list / 4] : kRounds[(rnd() >> 8) % 3];
      r[i].count = list < 12 ? 17 : kCounts[(rnd() >> 8) % 8];
      if (list >= 12 && (rnd() >> 8) % 16 == 0) { r[i].round = 0; r[i].count = 256; }   // pad()
    }
    const size_t bytes = layout(nullptr, r, n, none);
    for (int i = 0; i < n; ++i) CHECK(none[i].p == nullptr);
    char* block = static_cast<char*>(malloc(bytes ? bytes : 1));
    CHECK(block != nullptr);
    CHECK(layout(block, r, n, got) == bytes);
    char* at = block;
    size_t sum = 0;
    for (int i = 0; i < n; ++i) {
      if (r[i].round == 0) {
        const size_t off = (size_t)(at - block);
        at = block + (off + 255) / 256 * 256;
        continue;
      }
      CHECK(got[i].p == at);                                   // in order, disjoint
      CHECK((size_t)(got[i].p - block) + got[i].bytes <= bytes);   // inside the block
      memset(got[i].p, 0xA5, got[i].bytes);
      const size_t adv = (got[i].bytes + r[i].round - 1) / r[i].round * r[i].round;
      CHECK(adv >= got[i].bytes && adv < got[i].bytes + r[i].round);
      at += adv;
      sum += got[i].bytes;
    }
    CHECK((size_t)(at - block) == bytes);
    CHECK(sum <= bytes);
    if (bytes > most) most = bytes;
    free(block);
  }
  printf("ws_layout_check ok: %d lists, largest block %zu bytes\n", kLists, most);
  return 0;
}
