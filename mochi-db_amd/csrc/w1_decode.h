// w1_decode.h — the Write1 reply decoder: launch interface between the C-ABI
// layer (capi.cpp) and the device kernels (w1_decode.hip), the host twin
// (w1_decode_host.cpp), and the parsing both share.  Semantics:
// include/mochi_hip.h (mochi_write1_replies / mochi_write1_decoded).
//
// Everything under `namespace w1d` is __host__ __device__ and reads the body
// through (base pointer, offsets below the body length) alone: the host form
// and every kernel run the same walk over the same bytes, so they cannot
// disagree, and a stand-alone host program (microbench/w1_decode_check.cpp)
// checks under a sanitizer that no read leaves the slice.
//
// Wire layout (MochiProtocol.proto:107-161 + MultiGrant.grantSignatures = 5),
// parsed as protobuf-java 3.16.3 parses it -- the rules of w2_decode.hip:
// singular fields last-wins, unknown fields and foreign wire types skipped
// (groups to depth 100), proto3 strings and map keys strict UTF-8, map entries
// into a LinkedHashMap (a repeated key keeps its first position and takes its
// last value), every Grant / WriteCertificate value parsed even when a later
// entry replaces it.
//   Write1OkFromServer / Write1RefusedFromServer
//     = [0A MultiGrant] { 12 ( 0A objectId  12 WriteCertificate ) } [1A clientId] [22 hash]
//   MultiGrant       = { 0A ( 0A key 12 Grant ) } [12 clientId] [1A hash] [22 serverId] { 2A ( 0A key 12 sig ) }
//   WriteCertificate = { 0A ( 0A serverId 12 MultiGrant ) }
//   Grant            = [0A objectId] [10 timestamp] [18 configstamp] [22 transactionHash] [28 status]
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mochi_hip.h"
#include "carve.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define W1D_NOINLINE __noinline__
#else
#define W1D_NOINLINE
#endif
#define W1D_HD __host__ __device__ inline

namespace mochi {
namespace w1d {

constexpr uint32_t kMaxEntries = 64;   // grants / grantSignatures / currentCertificates wire entries per decoded response
constexpr uint32_t kGroupDepth = 100;  // CodedInputStream's default recursion limit
constexpr uint32_t kStMal = 1u, kStFb = 2u;
constexpr uint32_t kBad = 0xFFFFFFFFu;
constexpr uint32_t kMaxResps = 1u << 24;  // 65 level-2 entries each: every total stays below 2^32

struct Fld {
  uint32_t field, wt;
  uint64_t v;
  uint32_t off, len;  // wire type 2 payload
};

W1D_HD bool vint(const uint8_t* p, uint32_t& pos, uint32_t end, uint64_t& v) {
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

W1D_HD bool vlen(const uint8_t* p, uint32_t& pos, uint32_t end, uint32_t& len) {
  uint64_t l;
  if (!vint(p, pos, end, l)) return false;
  const int32_t l32 = (int32_t)(uint32_t)l;  // readRawVarint32
  if (l32 < 0 || (uint32_t)l32 > end - pos) return false;
  len = (uint32_t)l32;
  return true;
}

// Skip the unknown group opened by `field`; the position after it, or kBad.
// Out of line on the device: its stack lives in scratch memory.
__host__ __device__ W1D_NOINLINE inline uint32_t skip_group(const uint8_t* p, uint32_t pos, uint32_t end, uint32_t field) {
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
W1D_HD int next_fld(const uint8_t* p, uint32_t& pos, uint32_t end, Fld& f) {
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
W1D_HD bool valid_utf8(const uint8_t* p, uint32_t off, uint32_t n) {
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

W1D_HD bool bytes_eq(const uint8_t* a, const uint8_t* b, uint32_t n) {
  for (uint32_t i = 0; i < n; i++)
    if (a[i] != b[i]) return false;
  return true;
}
// FNV-1a over the bytes, then a finalizer (murmur3's) so that strings that differ in
// their last byte alone spread over a table: the slot hash of the claim tables
// (w1_request.hip's key table, envelope.hip's msgId table).  It decides no output.
W1D_HD uint32_t bytes_hash(const uint8_t* k, uint32_t n) {
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
W1D_HD bool key_eq(const uint8_t* p, uint32_t a, uint32_t al, uint32_t b, uint32_t bl) {
  return al == bl && (a == b || bytes_eq(p + a, p + b, al));
}

W1D_HD uint32_t varint_size(uint64_t v) {
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
W1D_HD bool parse_grant(const uint8_t* p, uint32_t off, uint32_t len, Grant& g) {
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

// map<string, V> entry: key and value as MapEntry reads them (last occurrence of each; default empty)
struct Entry {
  uint32_t koff, klen, voff, vlen, nval;
};
// validates the framing and the key; kind 1: every value is a Grant that must parse
W1D_HD bool read_entry(const uint8_t* p, uint32_t off, uint32_t len, int kind, bool check, Entry& e) {
  e.koff = e.klen = e.voff = e.vlen = e.nval = 0;
  uint32_t pos = off;
  const uint32_t end = off + len;
  Fld f;
  int rc;
  while ((rc = next_fld(p, pos, end, f)) > 0) {
    if (f.wt != 2) continue;
    if (f.field == 1) {
      if (check && !valid_utf8(p, f.off, f.len)) return false;
      e.koff = f.off;
      e.klen = f.len;
    } else if (f.field == 2) {
      Grant g;
      if (check && kind == 1 && !parse_grant(p, f.off, f.len, g)) return false;
      e.voff = f.off;
      e.vlen = f.len;
      e.nval++;
    }
  }
  return rc == 0;
}

// One walk of a MultiGrant value: validity (what protobuf-java's parser checks),
// the wire entry counts, whether a grants entry carries its value twice, and
// the last clientId / serverId.
struct MGScan {
  uint32_t nge, nse;
  bool twice;
  uint32_t sid_off, sid_len, cl_off, cl_len;
};
W1D_HD bool scan_multigrant(const uint8_t* p, uint32_t off, uint32_t len, MGScan& m) {
  m.nge = m.nse = 0;
  m.twice = false;
  m.sid_off = m.sid_len = m.cl_off = m.cl_len = 0;
  uint32_t pos = off;
  const uint32_t end = off + len;
  Fld f;
  int rc;
  while ((rc = next_fld(p, pos, end, f)) > 0) {
    if (f.wt != 2) continue;
    Entry e;
    if (f.field == 1) {
      m.nge++;
      if (!read_entry(p, f.off, f.len, 1, true, e)) return false;
      if (e.nval > 1) m.twice = true;
    } else if (f.field >= 2 && f.field <= 4) {
      if (!valid_utf8(p, f.off, f.len)) return false;
      if (f.field == 2) {
        m.cl_off = f.off;
        m.cl_len = f.len;
      } else if (f.field == 4) {
        m.sid_off = f.off;
        m.sid_len = f.len;
      }
    } else if (f.field == 5) {
      m.nse++;
      if (!read_entry(p, f.off, f.len, 0, true, e)) return false;
    }
  }
  return rc == 0;
}

// a WriteCertificate, all the way down
W1D_HD bool valid_writecert(const uint8_t* p, uint32_t off, uint32_t len) {
  uint32_t pos = off;
  const uint32_t end = off + len;
  Fld f;
  int rc;
  while ((rc = next_fld(p, pos, end, f)) > 0) {
    if (f.field != 1 || f.wt != 2) continue;
    uint32_t p2 = f.off;
    const uint32_t e2 = f.off + f.len;
    Fld g;
    int rc2;
    while ((rc2 = next_fld(p, p2, e2, g)) > 0) {
      if (g.wt != 2) continue;
      if (g.field == 1 && !valid_utf8(p, g.off, g.len)) return false;
      MGScan m;
      if (g.field == 2 && !scan_multigrant(p, g.off, g.len, m)) return false;
    }
    if (rc2 < 0) return false;
  }
  return rc == 0;
}

// a whole reply body (the shapes level 1 declines are validated here by its lane)
W1D_HD bool valid_reply(const uint8_t* p, uint32_t len) {
  uint32_t pos = 0;
  Fld f;
  int rc;
  while ((rc = next_fld(p, pos, len, f)) > 0) {
    if (f.wt != 2) continue;
    MGScan m;
    if (f.field == 1 && !scan_multigrant(p, f.off, f.len, m)) return false;
    if (f.field == 2) {
      uint32_t p2 = f.off;
      const uint32_t e2 = f.off + f.len;
      Fld g;
      int rc2;
      while ((rc2 = next_fld(p, p2, e2, g)) > 0) {
        if (g.wt != 2) continue;
        if (g.field == 1 && !valid_utf8(p, g.off, g.len)) return false;
        if (g.field == 2 && !valid_writecert(p, g.off, g.len)) return false;
      }
      if (rc2 < 0) return false;
    }
    if ((f.field == 3 || f.field == 4) && !valid_utf8(p, f.off, f.len)) return false;
  }
  return rc == 0;
}

// Walk the entries of map field `field` of the VALID message [off, off+len) in
// wire order; for each entry that is the first of its key, fn(index among the
// distinct keys, that entry, the entry holding the key's final value).
template <typename F>
W1D_HD void for_map(const uint8_t* p, uint32_t off, uint32_t len, uint32_t field, F&& fn) {
  uint32_t pos = off, idx = 0;
  const uint32_t end = off + len;
  Fld f;
  while (next_fld(p, pos, end, f) > 0) {
    if (f.field != field || f.wt != 2) continue;
    Entry e, x;
    read_entry(p, f.off, f.len, 0, false, e);
    bool first = true;
    uint32_t p2 = off;
    Fld g;
    while (first && p2 < f.off && next_fld(p, p2, end, g) > 0) {
      if (g.field != field || g.wt != 2 || g.off >= f.off) continue;
      read_entry(p, g.off, g.len, 0, false, x);
      if (key_eq(p, x.koff, x.klen, e.koff, e.klen)) first = false;
    }
    if (!first) continue;
    Entry last = e;
    p2 = pos;
    while (next_fld(p, p2, end, g) > 0) {
      if (g.field != field || g.wt != 2) continue;
      read_entry(p, g.off, g.len, 0, false, x);
      if (key_eq(p, x.koff, x.klen, e.koff, e.klen)) last = x;
    }
    fn(idx++, e, last);
  }
}

// ---- level 1, per response: the top level -------------------------------------
struct Level1 {
  uint32_t mg_off, mg_len;  // the multiGrant value (absent: the empty default)
  uint32_t n_ce;            // currentCertificates entries on the wire
  uint32_t n_keys;          // ... distinct keys among them
};
// Returns status bits.  With bits set nothing of `o` is to be used.
W1D_HD uint32_t resp_level(const uint8_t* p, uint32_t len, Level1& o) {
  o.mg_off = o.mg_len = o.n_ce = o.n_keys = 0;
  uint32_t n_mg = 0, pos = 0;
  bool whole = false;
  Fld f;
  int rc;
  while ((rc = next_fld(p, pos, len, f)) > 0) {
    if (f.wt != 2) continue;
    if (f.field == 1) {
      if (++n_mg > 1) whole = true;  // a second multiGrant merges into the first
      o.mg_off = f.off;
      o.mg_len = f.len;
    } else if (f.field == 2) {
      if (++o.n_ce > kMaxEntries) whole = true;
      Entry e;
      if (!read_entry(p, f.off, f.len, 0, true, e)) return kStMal;
      if (e.nval > 1) whole = true;  // a second WriteCertificate value merges into the first
    } else if (f.field == 3 || f.field == 4) {
      if (!valid_utf8(p, f.off, f.len)) return kStMal;
    }
  }
  if (rc < 0) return kStMal;
  if (whole) return valid_reply(p, len) ? kStFb : kStMal;
  for_map(p, 0, len, 2, [&](uint32_t, const Entry&, const Entry&) { o.n_keys++; });
  return 0;
}

// value slice of the j-th currentCertificates entry on the wire (level 1 accepted the body)
W1D_HD void cert_entry_value(const uint8_t* p, uint32_t len, uint32_t j, uint32_t& voff, uint32_t& vlen) {
  uint32_t pos = 0, i = 0;
  Fld f;
  voff = vlen = 0;
  while (next_fld(p, pos, len, f) > 0) {
    if (f.field != 2 || f.wt != 2) continue;
    if (i++ == j) {
      Entry e;
      read_entry(p, f.off, f.len, 0, false, e);
      voff = e.voff;
      vlen = e.vlen;
      return;
    }
  }
}

// ---- level 2, the MultiGrant of a response ---------------------------------------
struct Level2 {
  uint32_t ng;  // distinct grants
  uint32_t sid_off, sid_len, cl_off, cl_len;
};
W1D_HD uint32_t mg_level(const uint8_t* p, uint32_t off, uint32_t len, Level2& o) {
  MGScan m;
  o.ng = o.sid_off = o.sid_len = o.cl_off = o.cl_len = 0;
  if (!scan_multigrant(p, off, len, m)) return kStMal;
  if (m.twice || m.nge > kMaxEntries || m.nse > kMaxEntries) return kStFb;
  bool canon = true;
  uint32_t ng = 0;
  for_map(p, off, len, 1, [&](uint32_t, const Entry&, const Entry& v) {
    Grant g;
    parse_grant(p, v.voff, v.vlen, g);  // an entry without a value: the default Grant, empty and canonical
    canon = canon && g.canon;
    ng++;
  });
  if (!canon) return kStFb;
  o.ng = ng;
  o.sid_off = m.sid_off;
  o.sid_len = m.sid_len;
  o.cl_off = m.cl_off;
  o.cl_len = m.cl_len;
  return 0;
}

// index of the first table id equal to the serverId, 0xFFFF if none
W1D_HD uint16_t find_server(const uint8_t* sid, uint32_t sl, const uint8_t* ids, const uint32_t* id_off, uint32_t n_ids) {
  for (uint32_t k = 0; k < n_ids && k < 0xFFFFu; k++)
    if (id_off[k + 1] - id_off[k] == sl && bytes_eq(ids + id_off[k], sid, sl)) return (uint16_t)k;
  return 0xFFFF;
}

// Grant.status as the classifier reads it: the value, or 0xFF for anything outside 0..254
W1D_HD uint8_t status_u8(int32_t s) { return s >= 0 && s < 255 ? (uint8_t)s : (uint8_t)0xFF; }

// What the decoder reads and writes: host pointers in the host form, device pointers in the kernels.
struct View {
  mochi_write1_replies in;
  const uint8_t* ids;
  const uint32_t* id_off;
  uint32_t n_ids;
  mochi_write1_decoded out;
  uint64_t* sig_src;  // [n_grants] wire offset of each signature, ~0 = none (device: scratch; host: null, copies at once)
};

// request of response p: req_resp_off is a CSR over the responses
W1D_HD uint32_t request_of(const uint32_t* req_resp_off, uint32_t Q, uint32_t p) {
  uint32_t lo = 0, hi = Q;  // the last q with req_resp_off[q] <= p
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (req_resp_off[mid] <= p) lo = mid;
    else hi = mid;
  }
  return lo;
}

// ---- emit, per decoded response: its grants and certificate entries -----------
// g0 / c0: the response's first grant / certificate slot.
W1D_HD void emit_resp(const View& v, uint32_t p, const uint32_t mg_off, const uint32_t mg_len, uint32_t g0, uint32_t c0) {
  const mochi_write1_replies& in = v.in;
  const mochi_write1_decoded& out = v.out;
  const uint64_t base = in.resp_off[p];
  const uint8_t* b = in.wire + base;
  const uint32_t len = in.resp_len[p];
  uint32_t o0 = 0, o1 = 0;
  if (in.n_reqs) {
    const uint32_t q = request_of(in.req_resp_off, in.n_reqs, p);
    o0 = in.req_op_off[q];
    o1 = in.req_op_off[q + 1];
    if (o1 - o0 > MOCHI_MAX_OPS_PER_CERT) o1 = o0 + MOCHI_MAX_OPS_PER_CERT;
  }
  for_map(b, mg_off, mg_len, 1, [&](uint32_t i, const Entry& k, const Entry& val) {
    const uint32_t g = g0 + i;
    Grant gr;
    parse_grant(b, val.voff, val.vlen, gr);
    out.grant_off[g] = base + val.voff;
    out.grant_len[g] = val.vlen;
    out.grant_ts[g] = gr.ts;
    out.grant_status[g] = status_u8(gr.status);
    uint8_t slot = 0xFF;
    for (uint32_t o = o0; o < o1 && slot == 0xFF; o++)
      if (in.op_key_len[o] == k.klen && bytes_eq(in.strings + in.op_key_off[o], b + k.koff, k.klen)) slot = (uint8_t)(o - o0);
    out.grant_key[g] = slot;
    // grantSignatures[key]: the last entry with this key, its last value
    bool have = false;
    uint32_t s_off = 0, s_len = 0, pos = mg_off;
    Fld f;
    while (next_fld(b, pos, mg_off + mg_len, f) > 0) {
      if (f.field != 5 || f.wt != 2) continue;
      Entry se;
      read_entry(b, f.off, f.len, 0, false, se);
      if (key_eq(b, se.koff, se.klen, k.koff, k.klen)) {
        have = true;
        s_off = se.voff;
        s_len = se.vlen;
      }
    }
    const bool sig = have && s_len == MOCHI_RSA_BYTES;
    const bool differs = !(k.klen == gr.oid_len && bytes_eq(b + k.koff, b + gr.oid_off, k.klen));
    out.grant_flags[g] = (uint8_t)((sig ? MOCHI_W1G_HAS_SIG : 0) | (differs ? MOCHI_W1G_KEY_DIFFERS : 0));
    if (v.sig_src) {
      v.sig_src[g] = sig ? base + s_off : ~0ull;
    } else if (out.sig) {
      uint8_t* d = out.sig + (size_t)g * MOCHI_RSA_BYTES;
      for (uint32_t t = 0; t < MOCHI_RSA_BYTES; t++) d[t] = sig ? b[s_off + t] : (uint8_t)0;
    }
  });
  for_map(b, 0, len, 2, [&](uint32_t i, const Entry& k, const Entry& val) {
    const uint32_t c = c0 + i;
    out.cert_key_off[c] = base + k.koff;
    out.cert_key_len[c] = k.klen;
    out.cert_val_off[c] = base + val.voff;
    out.cert_val_len[c] = val.vlen;
  });
}

// is a response of this kind parsed at all
W1D_HD bool parsed_kind(uint8_t kind) { return kind == MOCHI_W1_OK || kind == MOCHI_W1_REFUSED; }

}  // namespace w1d

// Device pointers; the context's scratch, laid out by w1d_layout.
struct W1DecArgs {
  w1d::View v;
  uint32_t P;
  // scratch
  uint32_t* st_bits;   // [P] kStMal / kStFb, OR-ed in by the level-2 lanes
  uint32_t* l1;        // [P][4] w1d::Level1
  uint32_t* l2;        // [P][4] the MultiGrant lane's serverId and clientId slices
  uint32_t* ng;        // [P] distinct grants of the response's MultiGrant
  uint64_t* cnt_e;     // [P+1] level-2 entries per response (1 + certificate entries; scan input)
  uint64_t* e_base;    // [P+1] their exclusive scan; e_base[P] = the entry total
  uint64_t* cnt64;     // [P+1] decoded grants | certificates << 32 per response (one packed scan)
  uint64_t* off64;     // [P+1] its exclusive scan; off64[P] = the two totals
  void* scan_temp;
  size_t scan_temp_bytes;
  // per-kernel timing or null: kW1DecEvents events, recorded before k_w1d_resp, after
  // it, after the entry scan, after k_w1d_level2, after k_w1d_final + the packed scan +
  // k_w1d_offsets; before k_w1d_emit, after it, after the signature gather
  hipEvent_t* ev;
};
constexpr int kW1DecEvents = 8;
constexpr int kW1DecStages = 6;  // k_w1d_resp, entry scan, k_w1d_level2, final + packed scan + offsets, k_w1d_emit, signatures
// The per-call scratch layout (a.P set; every array 16-byte aligned): on a null base it
// only counts and returns the bytes to allocate; on that allocation it sets a's
// scratch pointers.
inline size_t w1d_layout(W1DecArgs& a, void* base) {
  const size_t P = a.P, p1 = P + 1;
  Carve c(base);
  a.st_bits = c.take<uint32_t>(P);
  a.l1 = c.take<uint32_t>(4 * P);
  a.l2 = c.take<uint32_t>(4 * P);
  a.ng = c.take<uint32_t>(P);
  a.cnt_e = c.take<uint64_t>(p1);
  a.e_base = c.take<uint64_t>(p1);
  a.cnt64 = c.take<uint64_t>(p1);
  a.off64 = c.take<uint64_t>(p1);
  return c.bytes();
}
// levels 1 and 2, statuses, per-response outputs, both CSRs; off64[P] = the totals
hipError_t launch_w1d_count(const W1DecArgs& a, hipStream_t stream);
// per-grant and per-certificate arrays (a.v.sig_src set when signatures are wanted), n_grants from the totals
hipError_t launch_w1d_emit(const W1DecArgs& a, uint32_t n_grants, hipStream_t stream);

}  // namespace mochi

namespace mochi_host {
// mochi_write1_reply_decode without the null checks of the C layer; `err` names
// an inconsistent input (MOCHI_EINVAL).  MOCHI_EINVAL with *err == nullptr: a
// capacity is too small (out->n_grants / n_certs hold the counts needed).
int write1_reply_decode(const mochi_write1_replies* in, const uint8_t* ids, const uint32_t* id_off, uint32_t n_ids,
                        mochi_write1_decoded* out, const char** err);
}  // namespace mochi_host
