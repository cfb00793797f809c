// read_request.h — the ReadToServer request decoder and the read answer plan: launch
// interface between the C-ABI layer (capi.cpp) and the device kernels
// (read_request.hip), the host twin (read_request_host.cpp), and the parsing both
// share.  Semantics: include/mochi_hip.h (mochi_read_requests_decoded /
// mochi_read_key_state / mochi_read_answer_planned).
//
// The Transaction and Operation walk is w1_request.h's (w1q::tx_count, valid_tx,
// tx_entry, op_level): a read's transaction is the same message.  Only the top level
// (req_level), the per-request outputs and the "takes part in the key numbering"
// predicate are a read's own.  Everything under `namespace rdq` is __host__ __device__
// and reads a body through (base pointer, offsets below the body length) alone; a
// stand-alone host program (microbench/read_request_check.cpp) checks under a sanitizer
// that no read leaves the slice.
//
// Wire layout (MochiProtocol.proto:72-76), parsed as protobuf-java 3.16.3 parses it:
//   ReadToServer = [0A clientId] [12 Transaction] [1A nonce]
#pragma once
#include "w1_request.h"

namespace mochi {
namespace rdq {

using w1q::kMaxOps;
using w1q::kMaxReqs;
using wire::Fld;
using wire::kStFb;
using wire::kStMal;
using wire::next_fld;
using wire::valid_utf8;

// ---- per request: the top level ---------------------------------------------------
struct Level1 {
  uint32_t tx_off, tx_len;  // the transaction value (absent: empty); first, as k_w1q_ops reads them
  uint32_t n_ent;           // its Operation entries
  uint32_t _pad;
  uint32_t cl_off, cl_len, nn_off, nn_len;
};
// Returns status bits, as w1q::req_level: with bits set nothing of `o` is to be used, and a
// request outside the level-by-level shape is validated whole here.
WIRE_HD uint32_t req_level(const uint8_t* p, uint32_t len, Level1& o) {
  o.tx_off = o.tx_len = o.n_ent = o._pad = o.cl_off = o.cl_len = o.nn_off = o.nn_len = 0;
  uint32_t pos = 0, n_tx = 0;
  Fld f;
  int rc;
  while ((rc = next_fld(p, pos, len, f)) > 0) {
    if (f.wt != 2) continue;
    if (f.field == 1 || f.field == 3) {
      if (!valid_utf8(p, f.off, f.len)) return kStMal;
      if (f.field == 1) {
        o.cl_off = f.off;
        o.cl_len = f.len;
      } else {
        o.nn_off = f.off;
        o.nn_len = f.len;
      }
    } else if (f.field == 2) {
      n_tx++;
      o.tx_off = f.off;
      o.tx_len = f.len;
    }
  }
  if (rc < 0) return kStMal;
  if (n_tx > 1) {  // a second transaction merges into the first: every one is parsed
    pos = 0;
    while (next_fld(p, pos, len, f) > 0)
      if (f.wt == 2 && f.field == 2 && !w1q::valid_tx(p, f.off, f.len)) return kStMal;
    return kStFb;
  }
  if (!w1q::tx_count(p, o.tx_off, o.tx_len, o.n_ent)) return kStMal;
  if (o.n_ent > kMaxOps) return w1q::valid_tx(p, o.tx_off, o.tx_len) ? kStFb : kStMal;
  return 0;
}

// What the decoder reads and writes: host pointers in the host form, device pointers in the kernels.
struct View {
  mochi_read_requests in;
  mochi_read_requests_decoded out;
};

// the per-request outputs but req_op_off; returns the request's op count
WIRE_HD uint32_t final_req(const View& v, uint32_t q, uint32_t bits, const Level1& l) {
  const mochi_read_requests_decoded& out = v.out;
  const bool ok = bits == 0;
  const uint64_t base = ok ? v.in.msg_off[q] : 0;
  out.req_status[q] = bits & kStMal ? MOCHI_RDQ_MALFORMED : bits & kStFb ? MOCHI_RDQ_FALLBACK : MOCHI_RDQ_OK;
  out.req_client_off[q] = base + (ok ? l.cl_off : 0);
  out.req_client_len[q] = ok ? l.cl_len : 0;
  out.req_nonce_off[q] = base + (ok ? l.nn_off : 0);
  out.req_nonce_len[q] = ok ? l.nn_len : 0;
  return ok ? l.n_ent : 0;
}

// op o = entry j of OK request q: key slice and flags
WIRE_HD void emit_op(const View& v, uint32_t q, uint32_t tx_off, uint32_t tx_len, uint32_t j, uint32_t o) {
  const uint64_t base = v.in.msg_off[q];
  const uint8_t* b = v.in.wire + base;
  uint32_t eo, el;
  w1q::tx_entry(b, tx_off, tx_len, j, eo, el);
  w1q::Op op;
  w1q::op_level(b, eo, el, false, op);
  v.out.op_key_off[o] = base + op.k_off;
  v.out.op_key_len[o] = op.k_len;
  v.out.op_flags[o] = op.action == 0 ? (uint8_t)MOCHI_RDOP_READ : (uint8_t)0;
}

// ---- the plan, per request ----------------------------------------------------------
struct PlanView {
  uint32_t n_reqs;
  mochi_read_requests_decoded d;  // req_status, req_op_off, op_key_len, op_flags, op_obj
  mochi_read_key_state k;
  mochi_read_answer_planned o;
};
constexpr uint8_t kHeldOk = MOCHI_RDK_PRESENT | MOCHI_RDK_HAS_CERT;
WIRE_HD void plan_req(const PlanView& v, uint32_t q) {
  const uint32_t o0 = v.d.req_op_off[q], o1 = v.d.req_op_off[q + 1];
  const uint8_t rs = v.d.req_status[q];
  uint8_t st = rs == MOCHI_RDQ_OK ? MOCHI_RDA_REPLY : rs == MOCHI_RDQ_FALLBACK ? MOCHI_RDA_HOST : MOCHI_RDA_NO_REPLY;
  for (uint32_t o = o0; st == MOCHI_RDA_REPLY && o < o1; o++) {
    const uint32_t u = v.d.op_obj[o];
    // not a READ (:217), an empty operand1 (:77); such an op has no key number either
    if (!(v.d.op_flags[o] & MOCHI_RDOP_READ) || v.d.op_key_len[o] == 0 || u == MOCHI_W1_NONE) {
      st = MOCHI_RDA_NO_REPLY;
    } else {
      const uint8_t kf = v.k.key_flags[u];
      if ((kf & MOCHI_RDK_LOCAL) && (kf & kHeldOk) != kHeldOk) st = MOCHI_RDA_NO_REPLY;
    }
  }
  for (uint32_t o = o0; o < o1; o++) {
    uint8_t status = 0xFF, existed = 0, flags = 0;
    uint64_t r_off = 0, c_off = 0;
    uint32_t r_len = 0, c_len = 0;
    if (st == MOCHI_RDA_REPLY) {
      const uint32_t u = v.d.op_obj[o];
      const uint8_t kf = v.k.key_flags[u];
      if (!(kf & MOCHI_RDK_LOCAL)) {
        status = 1;  // WRONG_SHARD: the shard check comes before the null checks
      } else {
        status = 0;
        existed = kf & MOCHI_RDK_AVAILABLE ? 1 : 0;
        flags = MOCHI_RAO_RESULT_STORE | MOCHI_RAO_HAS_CERT | MOCHI_RAO_CERT_STORE;
        r_off = v.k.key_value_off[u];
        r_len = v.k.key_value_len[u];
        c_off = v.k.key_cert_off[u];
        c_len = v.k.key_cert_len[u];
      }
    }
    v.o.op_status[o] = status;
    v.o.op_existed[o] = existed;
    v.o.op_flags[o] = flags;
    v.o.op_result_off[o] = r_off;
    v.o.op_result_len[o] = r_len;
    v.o.op_cert_off[o] = c_off;
    v.o.op_cert_len[o] = c_len;
  }
  v.o.plan_status[q] = st;
  v.o.resp_kind[q] = st == MOCHI_RDA_REPLY ? MOCHI_RR_READ : MOCHI_RR_OTHER;
  v.o.resp_n_ops[q] = st == MOCHI_RDA_REPLY ? o1 - o0 : 0;
  v.o.slot_off[q] = o0;
}

}  // namespace rdq

// Device pointers; the context's scratch.  The per-request part (rdq_layout) is laid out
// before the first launch, the per-op part (key_table_layout on k, with k.n_ops and
// k.slots set) once the host knows n_ops.
struct RdReqArgs {
  rdq::View v;
  uint32_t Q;
  uint32_t n_ops;      // set after the host wait
  uint32_t* n_keys;    // the caller's device word
  KeyNumArgs k;        // n_ops, slots and the scratch; launch_rdq_emit fills in the rest
  // per-request scratch
  uint32_t* st_bits;   // [Q] kStMal / kStFb, OR-ed in by the entry lanes
  uint32_t* l1;        // [Q][8] rdq::Level1
  uint64_t* cnt_e;     // [Q+1] Operation entries per request accepted so far (scan input)
  uint64_t* e_base;    // [Q+1] their exclusive scan; e_base[Q] = the entry total
  uint64_t* cnt64;     // [Q+1] ops per request (0 unless OK)
  uint64_t* off64;     // [Q+1] its exclusive scan; off64[Q] = n_ops
  void* scan_temp;
  size_t scan_temp_bytes;
  // per-kernel timing or null: kRdReqEvents events, at the points of W1ReqArgs.ev
  hipEvent_t* ev;
};
constexpr int kRdReqEvents = kW1ReqEvents;
constexpr int kRdReqStages = kW1ReqStages;
// The per-request scratch layout (a.Q set; every array 16-byte aligned): on a null base it
// only counts and returns the bytes to allocate; on that allocation it sets a's pointers.
inline size_t rdq_layout(RdReqArgs& a, void* base) {
  const size_t Q = a.Q, q1 = Q + 1;
  Carve c(base);
  a.st_bits = c.take<uint32_t>(Q);
  a.l1 = c.take<uint32_t>(8 * Q);
  a.cnt_e = c.take<uint64_t>(q1);
  a.e_base = c.take<uint64_t>(q1);
  a.cnt64 = c.take<uint64_t>(q1);
  a.off64 = c.take<uint64_t>(q1);
  return c.bytes();
}
// framing, validation, statuses, per-request outputs and req_op_off; off64[Q] = n_ops
hipError_t launch_rdq_count(const RdReqArgs& a, hipStream_t stream);
// the per-op arrays, the key numbering and *n_keys (a.n_ops <= op_cap checked by the caller)
hipError_t launch_rdq_emit(const RdReqArgs& a, hipStream_t stream);
// k_rda_plan, lane = request
hipError_t launch_rda_plan(const rdq::PlanView& v, hipStream_t stream);

}  // namespace mochi

namespace mochi_host {
// mochi_read_request_decode / mochi_read_answer_plan without the null checks of the C layer;
// `err` names an inconsistent input (MOCHI_EINVAL).  The decoder's MOCHI_EINVAL with *err ==
// nullptr: op_cap is too small (out->n_ops holds the count needed).
int read_request_decode(const mochi_read_requests* in, mochi_read_requests_decoded* out, const char** err);
int read_answer_plan(const mochi::rdq::PlanView* v, const char** err);
}  // namespace mochi_host
