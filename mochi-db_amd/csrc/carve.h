// carve.h — the scratch layout cursor of the host code.  Plain C++ (no HIP), so a
// host program can check the layout functions alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace mochi {

// Cursor over one call's scratch.  Each user has ONE layout function that takes
// its arrays from a Carve in order: run on a null base it only counts (bytes()
// is what to allocate), run on the allocation it hands out the same arrays, so
// the size and the pointers cannot disagree.  Every array starts on an `align`
// boundary (a power of two) and owns whole `align` units -- none for a count of 0,
// which shares its address with the next take; arrays taken one after the other
// are adjacent up to that rounding.
class Carve {
 public:
  explicit Carve(void* base, size_t align = 16)
      : base_(base ? (uint8_t*)(((uintptr_t)base + align - 1) & ~(uintptr_t)(align - 1)) : nullptr), align_(align) {}
  template <class T>
  T* take(size_t count) {
    const size_t at = used_;
    used_ += (count * sizeof(T) + align_ - 1) & ~(align_ - 1);
    return base_ ? (T*)(base_ + at) : nullptr;
  }
  // the arrays taken so far, plus the `align` bytes that aligning the base may skip
  size_t bytes() const { return used_ + align_; }

 private:
  uint8_t* base_;
  size_t align_, used_ = 0;
};

}  // namespace mochi
