// chunk_plan.h — planning of the chunked host pipeline (host_path.cpp): which units
// go into which chunk, the bytes of the blob a chunk reads, and where each array sits
// in a staging buffer.  Plain C++ (no HIP), so a host program can check it alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace mochi {

// Cuts n units (certificates, messages) into chunks and calls chunk(u0, u1) for each
// in order: whole groups of 32 (so every chunk's accept bits start on a word) until
// the chunk's weight reaches target.  step_weight(lo, hi) is the weight of the units
// [lo, hi) of one group.  An empty batch is one empty chunk.
template <class StepWeight, class Chunk>
void plan_chunks(uint32_t n, uint64_t target, StepWeight step_weight, Chunk chunk) {
  uint32_t u0 = 0;
  do {
    uint32_t u1 = u0;
    uint64_t weight = 0;
    do {
      const uint32_t next = n - u1 > 32 ? u1 + 32 : n;
      weight += step_weight(u1, next);
      u1 = next;
    } while (u1 < n && weight < target);
    chunk(u0, u1);
    u0 = u1;
  } while (u0 < n);
}

// Bytes [lo, hi) of a blob that a chunk reads; lo = hi = 0 while it reads nothing.
struct ByteRange {
  uint64_t lo = 0, hi = 0;
  bool none = true;
  // ... and the slices (off[i], len[i]) for i in [i0, i1) as well
  template <class Len>
  void add(const uint64_t* off, const Len* len, uint32_t i0, uint32_t i1) {
    if (i0 >= i1) return;
    uint64_t l = none ? UINT64_MAX : lo, h = hi;  // locals: a plain min / max loop over millions of grants
    for (uint32_t i = i0; i < i1; i++) {
      const uint64_t end = off[i] + len[i];
      l = off[i] < l ? off[i] : l;
      h = end > h ? end : h;
    }
    lo = l, hi = h, none = false;
  }
};

// Hands out offsets into one buffer, each on a 256-byte boundary.
struct Carve256 {
  size_t total = 0;  // bytes to allocate for what was taken so far
  size_t take(size_t bytes) {
    const size_t off = total;
    total = (total + bytes + 255) / 256 * 256;
    return off;
  }
};

}  // namespace mochi
