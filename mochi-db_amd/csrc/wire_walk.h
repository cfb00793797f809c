// wire_walk.h — the one pointer walk over protobuf wire bytes, shared by the
// host and device forms of every codec but the verify path: the Write1 reply,
// Write1 request and result decoders, the answer encoder's plan, the envelope
// codec and the host Write2 encoder.  It includes nothing from any codec.
//
// Everything under `namespace wire` is __host__ __device__ and reads through
// (base pointer, offsets below an explicit end) alone: a host form and its
// kernels run the same walk over the same bytes, so they cannot disagree, and
// the stand-alone programs microbench/*_check.cpp check under a sanitizer that
// no read leaves the slice.
//
// The rules are protobuf-java 3.16.3's: varints of at most ten bytes whose bits
// past 64 are dropped, lengths read as readRawVarint32 (negative: malformed),
// unknown fields and foreign wire types skipped, groups to depth 100, proto3
// strings strict UTF-8 (Utf8.isValidUtf8).
//
// The verify path (kernels.hip, w2_decode.hip, the device encoders' Grant
// parse) walks with proto_dev.h's word-cached ByteReader instead: the same
// rules, shaped for that path's speed.  The two are not merged on purpose.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIP_DEVICE_COMPILE__)
#define WIRE_NOINLINE __noinline__
#else
#define WIRE_NOINLINE
#endif
#define WIRE_HD __host__ __device__ inline

namespace mochi {
namespace wire {

constexpr uint32_t kGroupDepth = 100;  // CodedInputStream's default recursion limit
constexpr uint32_t kBad = 0xFFFFFFFFu;

struct Fld {
  uint32_t field, wt;
  uint64_t v;
  uint32_t off, len;  // wire type 2 payload
};

WIRE_HD bool vint(const uint8_t* p, uint32_t& pos, uint32_t end, uint64_t& v) {
  uint64_t x = 0;
  for (int i = 0; i < 10; i++) {
    if (pos >= end) return false;
    const uint32_t c = p[pos++];
    x |= (uint64_t)(c & 0x7F) << (7 * i);
    if (!(c & 0x80)) {
      v = x;
      return true;
    }
  }
  return false;
}

WIRE_HD bool vlen(const uint8_t* p, uint32_t& pos, uint32_t end, uint32_t& len) {
  uint64_t l;
  if (!vint(p, pos, end, l)) return false;
  const int32_t l32 = (int32_t)(uint32_t)l;  // readRawVarint32
  if (l32 < 0 || (uint32_t)l32 > end - pos) return false;
  len = (uint32_t)l32;
  return true;
}

// Skip the unknown group opened by `field`; the position after it, or kBad.
// Out of line on the device: its stack lives in scratch memory.
__host__ __device__ WIRE_NOINLINE inline uint32_t skip_group(const uint8_t* p, uint32_t pos, uint32_t end, uint32_t field) {
  uint32_t stack[kGroupDepth];
  uint32_t depth = 1;
  stack[0] = field;
  while (depth > 0) {
    uint64_t t64;
    if (!vint(p, pos, end, t64)) return kBad;
    const uint32_t t = (uint32_t)t64, f = t >> 3, wt = t & 7;
    if (f == 0) return kBad;
    uint32_t l;
    uint64_t v;
    switch (wt) {
      case 0:
        if (!vint(p, pos, end, v)) return kBad;
        break;
      case 1:
        if (end - pos < 8) return kBad;
        pos += 8;
        break;
      case 2:
        if (!vlen(p, pos, end, l)) return kBad;
        pos += l;
        break;
      case 3:
        if (depth >= kGroupDepth) return kBad;
        stack[depth++] = f;
        break;
      case 4:
        if (stack[depth - 1] != f) return kBad;
        depth--;
        break;
      case 5:
        if (end - pos < 4) return kBad;
        pos += 4;
        break;
      default:
        return kBad;
    }
  }
  return pos;
}

// Next field in [pos, end): 1 field, 0 end, -1 malformed.
WIRE_HD int next_fld(const uint8_t* p, uint32_t& pos, uint32_t end, Fld& f) {
  if (pos >= end) return 0;
  uint64_t t64;
  if (!vint(p, pos, end, t64)) return -1;
  const uint32_t t = (uint32_t)t64;
  f.field = t >> 3;
  f.wt = t & 7;
  f.off = f.len = 0;
  f.v = 0;
  if (f.field == 0) return -1;
  switch (f.wt) {
    case 0:
      return vint(p, pos, end, f.v) ? 1 : -1;
    case 1:
      if (end - pos < 8) return -1;
      pos += 8;
      return 1;
    case 2:
      if (!vlen(p, pos, end, f.len)) return -1;
      f.off = pos;
      pos += f.len;
      return 1;
    case 3: {
      const uint32_t np = skip_group(p, pos, end, f.field);
      if (np == kBad) return -1;
      pos = np;
      return 1;
    }
    case 5:
      if (end - pos < 4) return -1;
      pos += 4;
      return 1;
    default:
      return -1;  // END_GROUP at message level, wire types 6 and 7
  }
}

// Utf8.isValidUtf8: no overlong forms, no surrogates, nothing above U+10FFFF
WIRE_HD bool valid_utf8(const uint8_t* p, uint32_t off, uint32_t n) {
  uint32_t i = 0;
  while (i < n) {
    // ASCII runs (keys, ids, the 128-character hex transactionHash) a word per step
    // once the position is 4-byte aligned: the word lies inside the string
    if (i + 4 <= n && ((uintptr_t)(p + off + i) & 3) == 0) {
      uint32_t w;
      __builtin_memcpy(&w, __builtin_assume_aligned(p + off + i, 4), 4);
      if ((w & 0x80808080u) == 0) {
        i += 4;
        continue;
      }
    }
    const uint32_t c = p[off + i];
    if (c < 0x80) {
      i++;
    } else if (c < 0xC2) {
      return false;
    } else if (c < 0xE0) {
      if (i + 1 >= n || (p[off + i + 1] & 0xC0) != 0x80) return false;
      i += 2;
    } else if (c < 0xF0) {
      if (i + 2 >= n) return false;
      const uint32_t c1 = p[off + i + 1], c2 = p[off + i + 2];
      if ((c1 & 0xC0) != 0x80 || (c2 & 0xC0) != 0x80) return false;
      if (c == 0xE0 && c1 < 0xA0) return false;
      if (c == 0xED && c1 >= 0xA0) return false;
      i += 3;
    } else if (c < 0xF5) {
      if (i + 3 >= n) return false;
      const uint32_t c1 = p[off + i + 1], c2 = p[off + i + 2], c3 = p[off + i + 3];
      if ((c1 & 0xC0) != 0x80 || (c2 & 0xC0) != 0x80 || (c3 & 0xC0) != 0x80) return false;
      if (c == 0xF0 && c1 < 0x90) return false;
      if (c == 0xF4 && c1 >= 0x90) return false;
      i += 4;
    } else {
      return false;
    }
  }
  return true;
}

WIRE_HD bool bytes_eq(const uint8_t* a, const uint8_t* b, uint32_t n) {
  for (uint32_t i = 0; i < n; i++)
    if (a[i] != b[i]) return false;
  return true;
}
// FNV-1a over the bytes, then a finalizer (murmur3's) so that strings that differ in
// their last byte alone spread over a table: the slot hash of the claim tables
// (w1_request.hip's key table, envelope.hip's msgId table).  It decides no output.
WIRE_HD uint32_t bytes_hash(const uint8_t* k, uint32_t n) {
  uint32_t h = 0x811C9DC5u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (uint32_t i = 0; i < n; i++) h = (h ^ k[i]) * 0x01000193u;
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}
WIRE_HD bool key_eq(const uint8_t* p, uint32_t a, uint32_t al, uint32_t b, uint32_t bl) {
  return al == bl && (a == b || bytes_eq(p + a, p + b, al));
}

// bytes of the minimal varint encoding of v: the one host/device loop, for the
// canonical check below and for every encoder's size arithmetic (w2_encode.h)
WIRE_HD uint32_t varint_size(uint64_t v) {
  uint32_t n = 1;
  while (v >= 0x80) {
    v >>= 7;
    n++;
  }
  return n;
}

// The Grant at [off, off+len) (proto_dev.h's parse_grant_t with CANON): does it
// parse, what does it hold, and are its bytes exactly Grant.toByteArray() of
// what they parse to (fields 1..5 in order, each at most once, none at its
// default, one-byte tags, minimal varints, no unknown fields, status an int32).
struct Grant {
  int64_t ts;
  int32_t status;
  uint32_t oid_off, oid_len;
  bool canon;
};
WIRE_HD bool parse_grant(const uint8_t* p, uint32_t off, uint32_t len, Grant& g) {
  uint32_t pos = off, last = 0;
  const uint32_t end = off + len;
  g.ts = 0;
  g.status = 0;
  g.oid_off = g.oid_len = 0;
  bool cn = true;
  while (pos < end) {
    const uint32_t p0 = pos;
    uint64_t t64;
    if (!vint(p, pos, end, t64)) return false;
    const uint32_t tag = (uint32_t)t64, field = tag >> 3, wt = tag & 7;
    if (field == 0) return false;
    cn = cn && pos - p0 == 1 && field > last;
    last = field;
    if (tag == 10 || tag == 34) {
      const uint32_t p1 = pos;
      uint32_t l;
      if (!vlen(p, pos, end, l) || !valid_utf8(p, pos, l)) return false;
      cn = cn && l != 0 && pos - p1 == varint_size(l);
      if (tag == 10) {
        g.oid_off = pos;
        g.oid_len = l;
      }
      pos += l;
      continue;
    }
    if (tag == 16 || tag == 24 || tag == 40) {
      const uint32_t p1 = pos;
      uint64_t v;
      if (!vint(p, pos, end, v)) return false;
      if (tag == 16) g.ts = (int64_t)v;
      if (tag == 40) g.status = (int32_t)(uint32_t)v;  // readEnum: the low 32 bits
      // a 10-byte varint carries bit 63 alone in its last byte
      cn = cn && v != 0 && pos - p1 == varint_size(v) && (pos - p1 < 10 || p[pos - 1] == 1) &&
           (tag != 40 || (int64_t)v == (int64_t)(int32_t)(uint32_t)v);
      continue;
    }
    cn = false;  // an unknown field, a known one with a foreign wire type, or a group
    uint32_t l;
    uint64_t v;
    switch (wt) {
      case 0:
        if (!vint(p, pos, end, v)) return false;
        break;
      case 1:
        if (end - pos < 8) return false;
        pos += 8;
        break;
      case 2:
        if (!vlen(p, pos, end, l)) return false;
        pos += l;
        break;
      case 3:
        pos = skip_group(p, pos, end, field);
        if (pos == kBad) return false;
        break;
      case 5:
        if (end - pos < 4) return false;
        pos += 4;
        break;
      default:
        return false;
    }
  }
  g.canon = cn;
  return true;
}

// ---- not a walk, but shared by the decoders built on it ------------------------
// status bits a decoder's lanes OR together: the Write1 reply, Write1 request and result decoders
constexpr uint32_t kStMal = 1u, kStFb = 2u;
// responses per call of the Write1 reply and result decoders (at most 65 entries each below a response: every total stays below 2^32)
constexpr uint32_t kMaxResps = 1u << 24;

// Grant.status / OperationResult.status as a classifier reads it, the value or 0xFF outside 0..254: the Write1 reply and result decoders
WIRE_HD uint8_t status_u8(int32_t s) { return s >= 0 && s < 255 ? (uint8_t)s : (uint8_t)0xFF; }

// the row of element p in a CSR of Q rows (the last q with off[q] <= p): the request of a response in the
// Write1 reply and result decoders, the request of an operation in the Write1 request decoder's join
WIRE_HD uint32_t request_of(const uint32_t* req_resp_off, uint32_t Q, uint32_t p) {
  uint32_t lo = 0, hi = Q;  // the last q with req_resp_off[q] <= p
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (req_resp_off[mid] <= p) lo = mid;
    else hi = mid;
  }
  return lo;
}

}  // namespace wire
}  // namespace mochi
