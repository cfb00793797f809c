// w1_decode.h — the Write1 reply decoder: launch interface between the C-ABI
// layer (capi.cpp) and the device kernels (w1_decode.hip), the host twin
// (w1_decode_host.cpp), and the parsing both share.  Semantics:
// include/mochi_hip.h (mochi_write1_replies / mochi_write1_decoded).
//
// Everything under `namespace w1d` is __host__ __device__, built on the pointer
// walk of wire_walk.h, and reads the body through (base pointer, offsets below
// the body length) alone: the host form and every kernel run the same walk
// over the same bytes, so they cannot disagree, and a stand-alone host program
// (microbench/w1_decode_check.cpp) checks under a sanitizer that no read
// leaves the slice.  Only what is about Write1 replies (MultiGrant,
// WriteCertificate, the reply's levels) lives here.
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
#include "wire_walk.h"

namespace mochi {
namespace w1d {

using namespace wire;

constexpr uint32_t kMaxEntries = 64;   // grants / grantSignatures / currentCertificates wire entries per decoded response

// map<string, V> entry: key and value as MapEntry reads them (last occurrence of each; default empty)
struct Entry {
  uint32_t koff, klen, voff, vlen, nval;
};
// validates the framing and the key; kind 1: every value is a Grant that must parse
WIRE_HD bool read_entry(const uint8_t* p, uint32_t off, uint32_t len, int kind, bool check, Entry& e) {
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
WIRE_HD bool scan_multigrant(const uint8_t* p, uint32_t off, uint32_t len, MGScan& m) {
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

// a WriteCertificate, all the way down (the result decoder validates OperationResult.currentCertificate with it too)
WIRE_HD bool valid_writecert(const uint8_t* p, uint32_t off, uint32_t len) {
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
WIRE_HD bool valid_reply(const uint8_t* p, uint32_t len) {
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
WIRE_HD void for_map(const uint8_t* p, uint32_t off, uint32_t len, uint32_t field, F&& fn) {
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
WIRE_HD uint32_t resp_level(const uint8_t* p, uint32_t len, Level1& o) {
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
WIRE_HD void cert_entry_value(const uint8_t* p, uint32_t len, uint32_t j, uint32_t& voff, uint32_t& vlen) {
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
WIRE_HD uint32_t mg_level(const uint8_t* p, uint32_t off, uint32_t len, Level2& o) {
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
WIRE_HD uint16_t find_server(const uint8_t* sid, uint32_t sl, const uint8_t* ids, const uint32_t* id_off, uint32_t n_ids) {
  for (uint32_t k = 0; k < n_ids && k < 0xFFFFu; k++)
    if (id_off[k + 1] - id_off[k] == sl && bytes_eq(ids + id_off[k], sid, sl)) return (uint16_t)k;
  return 0xFFFF;
}

// What the decoder reads and writes: host pointers in the host form, device pointers in the kernels.
struct View {
  mochi_write1_replies in;
  const uint8_t* ids;
  const uint32_t* id_off;
  uint32_t n_ids;
  mochi_write1_decoded out;
  uint64_t* sig_src;  // [n_grants] wire offset of each signature, ~0 = none (device: scratch; host: null, copies at once)
};

// ---- emit, per decoded response: its grants and certificate entries -----------
// g0 / c0: the response's first grant / certificate slot.
WIRE_HD void emit_resp(const View& v, uint32_t p, const uint32_t mg_off, const uint32_t mg_len, uint32_t g0, uint32_t c0) {
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
WIRE_HD bool parsed_kind(uint8_t kind) { return kind == MOCHI_W1_OK || kind == MOCHI_W1_REFUSED; }

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
