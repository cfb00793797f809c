// wire_put.h — protobuf byte writers and the bounds predicate of the encoders'
// host twins (w2_encode_host.cpp, w1_issue_host.cpp, w1_reply_host.cpp, result_encode_host.cpp).
#pragma once
#include <cstdint>
#include <cstring>

namespace mochi_host {

inline uint8_t* put_varint(uint8_t* o, uint64_t v) {
  while (v >= 0x80) {
    *o++ = (uint8_t)(v | 0x80);
    v >>= 7;
  }
  *o++ = (uint8_t)v;
  return o;
}
// tag, length varint, payload
inline uint8_t* put_ld(uint8_t* o, uint8_t tag, const uint8_t* p, uint64_t n) {
  *o++ = tag;
  o = put_varint(o, n);
  if (n) memcpy(o, p, n);
  return o + n;
}
// does [off, off + len) lie inside a blob of `blob` bytes
inline bool inside(uint64_t off, uint32_t len, uint64_t blob) { return off <= blob && len <= blob - off; }

}  // namespace mochi_host
