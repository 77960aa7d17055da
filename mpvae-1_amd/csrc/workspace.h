// The one workspace carver.  A family lists its pieces once, in a function that
// takes a Workspace: over a null base that list is the sizing pass
// (*_workspace_bytes), over the caller's buffer it hands out the pointers the
// kernels get, so the size and the pointers cannot disagree.
//
// Every piece starts at a multiple of 256 B from the base and owns its bytes
// up to the next multiple of 256, so bytes() is a multiple of 256 too.  A
// layout that cannot be expressed (a negative count, a product or a sum that
// does not fit size_t) is refused: bytes() is 0 from then on, which every
// *_workspace_bytes returns as "no such shape" and every entry point answers
// with MPV_EINVAL.  No HIP here: tests/host/workspace_check.cpp builds this
// header alone.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace mpv {

class Workspace {
 public:
  static constexpr size_t kAlign = 256;

  explicit Workspace(void* base) : base_(static_cast<char*>(base)) {}

  // The next piece: n * more... elements of T (0 elements: no space, nullptr).
  // nullptr also from the sizing pass and from a refused layout.
  template <typename T, typename... More>
  T* take(int64_t n, More... more) {
    size_t bytes = sizeof(T), end;
    const int64_t factors[] = {n, (int64_t)more...};
    for (int64_t f : factors)
      if (f < 0 || __builtin_mul_overflow(bytes, (size_t)f, &bytes)) return refuse<T>();
    if (__builtin_add_overflow(bytes, kAlign - 1, &bytes) ||
        __builtin_add_overflow(end_, bytes / kAlign * kAlign, &end))
      return refuse<T>();
    char* at = base_ != nullptr && end != end_ && !refused_ ? base_ + end_ : nullptr;
    end_ = end;
    return reinterpret_cast<T*>(at);
  }

  // The end of the last piece; 0 once a take was refused.
  size_t bytes() const { return refused_ ? 0 : end_; }

  // Whether the caller's `have` bytes at a non-null base hold a non-empty layout.
  bool fits(size_t have) const { return base_ != nullptr && bytes() != 0 && have >= bytes(); }

 private:
  template <typename T>
  T* refuse() {
    refused_ = true;
    return nullptr;
  }

  char* base_;
  size_t end_ = 0;
  bool refused_ = false;
};

// The sizing pass of a family's layout function `list(ws, args...)`.
template <typename List, typename... Args>
size_t layout_bytes(List list, const Args&... args) {
  Workspace sizing(nullptr);
  list(sizing, args...);
  return sizing.bytes();
}

}  // namespace mpv
