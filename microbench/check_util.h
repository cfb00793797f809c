// check_util.h — what the stand-alone *_check programs share: the CHECK macro, the
// builders of protobuf wire bytes, and heap buffers of exactly the size asked for, so
// that under the address sanitizer a read or write one byte past a slice stops the run.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int g_failed = 0;
#define CHECK(cond, ...)                   \
  do {                                     \
    if (!(cond)) {                         \
      g_failed++;                          \
      fprintf(stderr, "FAIL %s: ", #cond); \
      fprintf(stderr, __VA_ARGS__);        \
      fprintf(stderr, "\n");               \
    }                                      \
  } while (0)

using Bytes = std::string;

static inline Bytes varint(uint64_t v) {
  Bytes o;
  while (v >= 0x80) {
    o.push_back((char)((v & 0x7F) | 0x80));
    v >>= 7;
  }
  o.push_back((char)v);
  return o;
}
// a length-delimited field; `tag` is the whole tag (field << 3 | 2), one byte below field 16
static inline Bytes ld(uint32_t tag, const Bytes& p) { return varint(tag) + varint(p.size()) + p; }
// a map entry: key in field 1, value in field 2
static inline Bytes entry(uint32_t tag, const Bytes& k, const Bytes& v) { return ld(tag, ld(0x0A, k) + ld(0x12, v)); }

template <class T>
struct Exact {  // a heap array of exactly n elements (never empty: a valid address)
  T* p;
  explicit Exact(size_t n) : p((T*)malloc(n ? n * sizeof(T) : 1)) {}
  Exact(const Exact&) = delete;
  ~Exact() { free(p); }
};
// `lead` bytes, then the body, ending the allocation: no byte after the body is readable
struct Wire : Exact<uint8_t> {
  size_t n;
  explicit Wire(const Bytes& body, size_t lead = 0) : Exact<uint8_t>(lead + body.size()), n(lead + body.size()) {
    memset(p, 0x5A, lead);
    if (body.size()) memcpy(p + lead, body.data(), body.size());
  }
};

// every truncation and every single-bit flip of b: fn(mutant, flip, k), with k the bytes
// kept (flip false) or index + bit of the bit flipped (flip true), for the callers to vary
// the lead and the kind with
template <class F>
static inline void for_mutants(const Bytes& b, F&& fn) {
  for (size_t n = 0; n <= b.size(); n++) fn(b.substr(0, n), false, n);
  for (size_t i = 0; i < b.size(); i++)
    for (int bit = 0; bit < 8; bit++) {
      Bytes m = b;
      m[i] = (char)(m[i] ^ (1 << bit));
      fn(m, true, i + bit);
    }
}
