// ws_layout.h — a caller-allocated workspace described once (plain host code, no HIP): ONE
// function per workspace calls take() once per region, in order, into a struct of typed pointers
// that ends with bytes().  Over a null base it only measures, so export, check and carve agree.
#pragma once
#include <stddef.h>

class WsLayout {
 public:
  explicit WsLayout(void* base) : base_(static_cast<char*>(base)) {}
  // the next region: `count` elements of T, its size rounded up to `round` bytes
  template <typename T>
  T* take(size_t count, size_t round) {
    T* const p = base_ ? reinterpret_cast<T*>(base_ + off_) : nullptr;
    off_ += (count * sizeof(T) + round - 1) / round * round;
    return p;
  }
  void pad(size_t round) { off_ = (off_ + round - 1) / round * round; }   // a header's end
  size_t bytes() const { return off_; }
 private:
  char* base_;
  size_t off_ = 0;
};
