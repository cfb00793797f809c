// result_decode.h — the decoder of the answers that close a transaction
// (Write2AnsFromServer / ReadFromServer) and the coalescing step behind the
// response tally: launch interface between the C-ABI layer (capi.cpp) and the
// device kernels (result_decode.hip), the host twin (result_decode_host.cpp),
// and the parsing both share.  Semantics: include/mochi_hip.h
// (mochi_result_replies / mochi_result_decoded).
//
// Everything under `namespace rrd` is __host__ __device__, built on the field
// walk of wire_walk.h (next_fld, valid_utf8, status_u8) and reads a body
// through (base pointer, offsets below the body length) alone.  It includes
// w1_decode.h for one Write1 structure it really decodes: an OperationResult's
// currentCertificate is a WriteCertificate, validated by w1d::valid_writecert.
// The host form and every kernel call the same functions in the same phases;
// microbench/result_decode_check.cpp runs them under a sanitizer.
//
// Wire layout (MochiProtocol.proto:45-60, 82-87, 102-105), parsed as
// protobuf-java 3.16.3 parses it (the rules of wire_walk.h):
//   Write2AnsFromServer = [0A TransactionResult] [12 rid]
//   ReadFromServer      = [0A TransactionResult] [12 nonce] [1A rid]
//   TransactionResult   = { 0A OperationResult }
//   OperationResult     = [0A result] [12 WriteCertificate] [18 existed] [20 status]
#pragma once
#include "w1_decode.h"

namespace mochi {
namespace rrd {

using w1d::valid_writecert;
using wire::Fld;
using wire::kStFb;
using wire::kStMal;
using wire::next_fld;
using wire::status_u8;
using wire::valid_utf8;

constexpr uint32_t kMaxOps = MOCHI_MAX_OPS_PER_CERT;
constexpr uint32_t kUndecoded = 0xFFFFFFFFu;  // resp_n_ops of a MALFORMED / FALLBACK response: equals no n_ops

// is a response of this kind parsed at all
WIRE_HD bool parsed_kind(uint8_t kind) { return kind == MOCHI_RR_WRITE2_ANS || kind == MOCHI_RR_READ; }
// top-level string fields: 2 in both kinds (rid / nonce), 3 in a ReadFromServer alone (rid)
WIRE_HD bool top_string(uint8_t kind, uint32_t field) { return field == 2 || (field == 3 && kind == MOCHI_RR_READ); }

// One OperationResult, validated all the way down.  Slices are offsets in the
// body; an absent field gives the operation's own offset and length 0.
struct Op {
  uint32_t res_off, res_len, cert_off, cert_len;
  uint32_t n_cert;  // currentCertificate occurrences (a second one merges into the first)
  int32_t status;   // readEnum: the low 32 bits
  bool existed;     // readBool: any non-zero varint
};
WIRE_HD bool read_op(const uint8_t* p, uint32_t off, uint32_t len, Op& o) {
  o.res_off = o.cert_off = off;
  o.res_len = o.cert_len = o.n_cert = 0;
  o.status = 0;
  o.existed = false;
  uint32_t pos = off;
  const uint32_t end = off + len;
  Fld f;
  int rc;
  while ((rc = next_fld(p, pos, end, f)) > 0) {
    if (f.wt == 2 && f.field == 1) {
      if (!valid_utf8(p, f.off, f.len)) return false;
      o.res_off = f.off;
      o.res_len = f.len;
    } else if (f.wt == 2 && f.field == 2) {
      if (!valid_writecert(p, f.off, f.len)) return false;
      o.cert_off = f.off;
      o.cert_len = f.len;
      o.n_cert++;
    } else if (f.wt == 0 && f.field == 3) {
      o.existed = f.v != 0;
    } else if (f.wt == 0 && f.field == 4) {
      o.status = (int32_t)(uint32_t)f.v;
    }
  }
  return rc == 0;
}

// every OperationResult of a TransactionResult value
WIRE_HD bool valid_txresult(const uint8_t* p, uint32_t off, uint32_t len) {
  uint32_t pos = off;
  const uint32_t end = off + len;
  Fld f;
  int rc;
  while ((rc = next_fld(p, pos, end, f)) > 0) {
    Op o;
    if (f.field == 1 && f.wt == 2 && !read_op(p, f.off, f.len, o)) return false;
  }
  return rc == 0;
}

// a whole answer body (the shapes level 1 declines are validated here by its lane)
WIRE_HD bool valid_answer(const uint8_t* p, uint32_t len, uint8_t kind) {
  uint32_t pos = 0;
  Fld f;
  int rc;
  while ((rc = next_fld(p, pos, len, f)) > 0) {
    if (f.wt != 2) continue;
    if (f.field == 1 && !valid_txresult(p, f.off, f.len)) return false;
    if (top_string(kind, f.field) && !valid_utf8(p, f.off, f.len)) return false;
  }
  return rc == 0;
}

// ---- level 1, per response: the top level and the TransactionResult's framing ----
struct Level1 {
  uint32_t tr_off, tr_len;  // the `result` value (absent: the empty default)
  uint32_t n_wire;          // OperationResult entries on the wire: the true count
  uint32_t rid_off, rid_len, nonce_off, nonce_len;  // last occurrences; absent: 0 / 0 in the body
};
// Returns status bits; with bits set only they are to be used.  A response with
// more than kMaxOps entries is validated whole here and keeps its count.
WIRE_HD uint32_t resp_level(const uint8_t* p, uint32_t len, uint8_t kind, Level1& o) {
  o.tr_off = o.tr_len = o.n_wire = o.rid_off = o.rid_len = o.nonce_off = o.nonce_len = 0;
  uint32_t n_res = 0, pos = 0;
  Fld f;
  int rc;
  while ((rc = next_fld(p, pos, len, f)) > 0) {
    if (f.wt != 2) continue;
    if (f.field == 1) {
      n_res++;
      o.tr_off = f.off;
      o.tr_len = f.len;
    } else if (top_string(kind, f.field)) {
      if (!valid_utf8(p, f.off, f.len)) return kStMal;
      if (f.field == 2 && kind == MOCHI_RR_READ) {
        o.nonce_off = f.off;
        o.nonce_len = f.len;
      } else {
        o.rid_off = f.off;
        o.rid_len = f.len;
      }
    }
  }
  if (rc < 0) return kStMal;
  if (n_res > 1) return valid_answer(p, len, kind) ? kStFb : kStMal;  // a second `result` merges: the lists concatenate
  pos = o.tr_off;
  const uint32_t end = o.tr_off + o.tr_len;
  while ((rc = next_fld(p, pos, end, f)) > 0)
    if (f.field == 1 && f.wt == 2) o.n_wire++;
  if (rc < 0) return kStMal;
  if (o.n_wire > kMaxOps && !valid_txresult(p, o.tr_off, o.tr_len)) return kStMal;
  return 0;
}
// operations a response hands to level 3 (the rest was validated by level 1's lane)
WIRE_HD uint32_t level3_ops(uint32_t bits, uint32_t n_wire) { return bits || n_wire > kMaxOps ? 0u : n_wire; }

// payload slice of the j-th OperationResult of the TransactionResult level 1 accepted
WIRE_HD void op_entry(const uint8_t* p, uint32_t tr_off, uint32_t tr_len, uint32_t j, uint32_t& off, uint32_t& len) {
  uint32_t pos = tr_off, i = 0;
  Fld f;
  off = len = 0;
  while (next_fld(p, pos, tr_off + tr_len, f) > 0) {
    if (f.field != 1 || f.wt != 2) continue;
    if (i++ == j) {
      off = f.off;
      len = f.len;
      return;
    }
  }
}

// What the decoder reads and writes: host pointers in the host form, device pointers in the kernels.
struct View {
  mochi_result_replies in;
  mochi_result_decoded out;
};

WIRE_HD void slot_absent(const mochi_result_decoded& out, uint64_t s) {
  out.op_status[s] = 0xFF;
  out.op_existed[s] = 0;
  out.op_flags[s] = 0;
  out.op_result_off[s] = 0;
  out.op_result_len[s] = 0;
  out.op_cert_off[s] = 0;
  out.op_cert_len[s] = 0;
}

// ---- level 3, per OperationResult j of response p (n_ops: its request's count) ----
// Validates the operation; writes its slot if it has one.  Returns status bits.
WIRE_HD uint32_t op_level(const View& v, uint32_t p, uint32_t tr_off, uint32_t tr_len, uint32_t j, uint32_t n_ops) {
  const uint64_t base = v.in.resp_off[p];
  const uint8_t* b = v.in.wire + base;
  uint32_t off, len;
  op_entry(b, tr_off, tr_len, j, off, len);
  Op o;
  if (!read_op(b, off, len, o)) return kStMal;
  if (j >= n_ops) return 0;  // validated; its values go nowhere
  if (o.n_cert > 1) return kStFb;
  const mochi_result_decoded& out = v.out;
  const uint64_t s = v.in.slot_off[p] + j;
  out.op_status[s] = status_u8(o.status);
  out.op_existed[s] = o.existed ? 1 : 0;
  out.op_flags[s] = o.n_cert ? MOCHI_RRO_HAS_CERT : 0;
  out.op_result_off[s] = base + o.res_off;
  out.op_result_len[s] = o.res_len;
  out.op_cert_off[s] = base + o.cert_off;
  out.op_cert_len[s] = o.cert_len;
  return 0;
}

// ---- level 4, per response: status, count, slices, and the slots nobody decoded ----
WIRE_HD void resp_final(const View& v, uint32_t p, uint32_t bits, const Level1& l, uint32_t n_ops) {
  const mochi_result_decoded& out = v.out;
  const uint64_t base = v.in.resp_off[p];
  const bool bad = bits != 0, parsed = !bad && parsed_kind(v.in.resp_kind[p]);
  out.resp_status[p] = bits & kStMal ? MOCHI_RRS_MALFORMED : bits & kStFb ? MOCHI_RRS_FALLBACK : MOCHI_RRS_OK;
  out.resp_n_ops[p] = bad ? kUndecoded : l.n_wire;
  out.resp_rid_off[p] = parsed ? base + l.rid_off : 0;
  out.resp_rid_len[p] = parsed ? l.rid_len : 0;
  out.resp_nonce_off[p] = parsed ? base + l.nonce_off : 0;
  out.resp_nonce_len[p] = parsed ? l.nonce_len : 0;
  const uint32_t done = level3_ops(bits, l.n_wire);
  const uint64_t s0 = v.in.slot_off[p];
  for (uint32_t j = done < n_ops ? done : n_ops; j < n_ops; j++) slot_absent(out, s0 + j);
}

// ---- the coalesced TransactionResult per request (MochiDBClient.java:177-179 / :384-386) ----
WIRE_HD void coalesce_req(const mochi_result_tallied& t, const mochi_result_coalesced& o, uint32_t q) {
  const bool accept = (t.accept_bits[q >> 5] >> (q & 31)) & 1;
  const uint32_t k = t.n_ops[q], p0 = t.req_resp_off[q], np = t.req_resp_off[q + 1] - p0;
  for (uint32_t j = 0; j < k; j++) {
    const uint64_t d = t.out_off[q] + j;
    const int32_t c = accept ? t.chosen[t.chosen_off[q] + j] : -1;
    if (c < 0 || (uint32_t)c >= np) {
      o.resp[d] = 0xFFFFFFFFu;
      o.status[d] = 0xFF;
      o.existed[d] = 0;
      o.flags[d] = 0;
      o.result_off[d] = 0;
      o.result_len[d] = 0;
      o.cert_off[d] = 0;
      o.cert_len[d] = 0;
      continue;
    }
    const uint32_t p = p0 + (uint32_t)c;
    const uint64_t s = t.slot_off[p] + j;
    o.resp[d] = p;
    o.status[d] = t.op_status[s];
    o.existed[d] = t.op_existed[s];
    o.flags[d] = t.op_flags[s];
    o.result_off[d] = t.op_result_off[s];
    o.result_len[d] = t.op_result_len[s];
    o.cert_off[d] = t.op_cert_off[s];
    o.cert_len[d] = t.op_cert_len[s];
  }
}

}  // namespace rrd

// Device pointers; the context's scratch, laid out by rr_layout.
struct RRArgs {
  rrd::View v;
  uint32_t P;
  // scratch
  uint32_t* st_bits;  // [P] kStMal / kStFb, OR-ed in by the level-3 lanes
  uint32_t* l1;       // [P][8] rrd::Level1 and the request's n_ops
  uint64_t* cnt;      // [P+1] level-3 operations per response (scan input)
  uint64_t* e_base;   // [P+1] their exclusive scan; e_base[P] = the operation total
  void* scan_temp;
  size_t scan_temp_bytes;
  // per-kernel timing or null: kRREvents events, recorded before k_rr_resp, after it,
  // after the scan, after k_rr_ops, after k_rr_final
  hipEvent_t* ev;
};
constexpr int kRREvents = 5;
constexpr int kRRStages = 4;  // k_rr_resp, the scan, k_rr_ops, k_rr_final
// The per-call scratch layout (a.P set; every array 16-byte aligned): on a null base it
// only counts and returns the bytes to allocate; on that allocation it sets a's
// scratch pointers.
inline size_t rr_layout(RRArgs& a, void* base) {
  const size_t P = a.P;
  Carve c(base);
  a.st_bits = c.take<uint32_t>(P);
  a.l1 = c.take<uint32_t>(8 * P);
  a.cnt = c.take<uint64_t>(P + 1);
  a.e_base = c.take<uint64_t>(P + 1);
  return c.bytes();
}
// all four levels, enqueued; no host wait
hipError_t launch_rr_decode(const RRArgs& a, hipStream_t stream);
hipError_t launch_rr_coalesce(const mochi_result_tallied& t, const mochi_result_coalesced& o, hipStream_t stream);
// blocks of the grid-stride level-3 kernel at P responses (the operation total is on the device)
uint32_t rr_ops_blocks(uint32_t P);

}  // namespace mochi

namespace mochi_host {
// mochi_result_reply_decode / mochi_result_coalesce without the null checks of the C
// layer; `err` names an inconsistent input (MOCHI_EINVAL).
int result_reply_decode(const mochi_result_replies* in, mochi_result_decoded* out, const char** err);
int result_coalesce(const mochi_result_tallied* in, mochi_result_coalesced* out, const char** err);
}  // namespace mochi_host
