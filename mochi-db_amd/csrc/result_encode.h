// result_encode.h — the ENCODER of the answers that close a transaction
// (Write2AnsFromServer / ReadFromServer, the inverse of result_decode.h) and the
// plan that turns the Write2 verifier's outputs into its input: launch
// interface between the C-ABI layer (capi.cpp) and the kernels
// (result_encode.hip), the host twin (result_encode_host.cpp), and the size
// arithmetic and the Write2 body walk both share.  Semantics:
// include/mochi_hip.h (mochi_result_answers / mochi_write2_answer_source).
//
// Everything under `namespace rae` is __host__ __device__.  The walk is built on
// the field walk of wire_walk.h (next_fld) and reads a body through (base
// pointer, offsets below the body length) alone;
// microbench/result_encode_check.cpp runs it under a sanitizer.
//
// Wire layout written (MochiProtocol.proto:45-60, 82-87, 102-105 as
// protobuf-java writes it):
//   Write2AnsFromServer = 0A len TransactionResult  [12 rid]
//   ReadFromServer      = 0A len TransactionResult  [12 nonce] [1A rid]
//   TransactionResult   = { 0A len OperationResult }
//   OperationResult     = [0A result] [12 len cert] [18 01] [20 status]
// Wire layout walked (w2_encode.h):
//   Write2ToServer = [0A WriteCertificate] [12 Transaction]
//   Transaction    = { 0A Operation }     Operation = [08 action] [12 operand1] [1A operand2]
#pragma once
#include "carve.h"
#include "w2_encode.h"
#include "wire_walk.h"

namespace mochi {
namespace rae {

using wire::Fld;
using wire::next_fld;

constexpr uint32_t kMaxOps = MOCHI_MAX_OPS_PER_CERT;
constexpr uint64_t kNone = ~0ull;
constexpr uint32_t kActionWrite = 2;  // OperationAction.WRITE (MochiProtocol.proto:20-24)

// ---- sizes ---------------------------------------------------------------------
WIRE_HD bool body_kind(uint8_t kind) { return kind == MOCHI_RR_WRITE2_ANS || kind == MOCHI_RR_READ; }

// one OperationResult's body, from its slot
WIRE_HD uint64_t op_body(const mochi_result_answers& a, uint64_t s) {
  const uint8_t st = a.op_status[s];
  return enc_ld_opt_size(a.op_result_len[s]) + (a.op_flags[s] & MOCHI_RAO_HAS_CERT ? enc_ld_size(a.op_cert_len[s]) : 0) +
         (a.op_existed[s] ? 2 : 0) + (st ? 1 + wire::varint_size(st) : 0);
}
WIRE_HD uint32_t rid_len(const mochi_result_answers& a, uint32_t p) { return a.rid_off ? a.rid_len[p] : 0; }
// a Write2 answer has no nonce
WIRE_HD uint32_t nonce_len(const mochi_result_answers& a, uint32_t p) {
  return a.nonce_off && a.resp_kind[p] == MOCHI_RR_READ ? a.nonce_len[p] : 0;
}

struct Sized {
  uint64_t tx;   // TransactionResult body
  uint64_t len;  // the message; 0 unless status is OK and the kind has a body
  uint8_t status;
};
// Response p.  op_rel (may be null) receives, per slot, where the operation's tag
// lies inside the TransactionResult body (meaningful only for an OK message: below 2^31).
WIRE_HD Sized size_resp(const mochi_result_answers& a, uint32_t p, uint32_t* op_rel) {
  Sized z{0, 0, MOCHI_ENC_OK};
  if (!body_kind(a.resp_kind[p])) return z;
  const uint32_t k = a.resp_n_ops[p];
  const uint64_t s0 = a.slot_off[p];
  if (k > kMaxOps || s0 > a.n_slots || k > a.n_slots - s0) {  // the host form refuses these
    z.status = MOCHI_ENC_BAD_OP;
    return z;
  }
  for (uint32_t j = 0; j < k; j++) {
    if (a.op_status[s0 + j] == 0xFF) {
      z.status = MOCHI_ENC_BAD_OP;
      return z;
    }
    if (op_rel) op_rel[s0 + j] = (uint32_t)z.tx;
    z.tx += enc_ld_size(op_body(a, s0 + j));
  }
  z.len = enc_ld_size(z.tx) + enc_ld_opt_size(rid_len(a, p)) + enc_ld_opt_size(nonce_len(a, p));
  if (z.len > kEncMaxMsg) {
    z.status = MOCHI_ENC_TOO_LONG;
    z.len = 0;
  }
  return z;
}

// ---- the walk of a Write2ToServer body -------------------------------------------
struct W2Body {
  uint32_t cert_off, cert_len;  // last length-delimited field 1; absent: 0 / 0
  uint32_t tx_off, tx_len;      // last length-delimited field 2
};
WIRE_HD bool w2_top(const uint8_t* p, uint32_t len, W2Body& o) {
  o.cert_off = o.cert_len = o.tx_off = o.tx_len = 0;
  uint32_t pos = 0;
  Fld f;
  int rc;
  while ((rc = next_fld(p, pos, len, f)) > 0) {
    if (f.wt != 2) continue;
    if (f.field == 1) {
      o.cert_off = f.off;
      o.cert_len = f.len;
    } else if (f.field == 2) {
      o.tx_off = f.off;
      o.tx_len = f.len;
    }
  }
  return rc == 0;
}
struct W2Op {
  uint32_t action;            // last `action` varint, its low 32 bits (readEnum)
  uint32_t op2_off, op2_len;  // last length-delimited field 3; absent: the operation's own offset, 0
};
// The next Operation of the Transaction in [pos, end): 1, 0 at the end, -1 malformed.
WIRE_HD int w2_next_op(const uint8_t* p, uint32_t& pos, uint32_t end, W2Op& o) {
  Fld f;
  int rc;
  while ((rc = next_fld(p, pos, end, f)) > 0) {
    if (f.field != 1 || f.wt != 2) continue;
    o.action = 0;
    o.op2_off = f.off;
    o.op2_len = 0;
    uint32_t q = f.off;
    const uint32_t e = f.off + f.len;
    Fld g;
    int r2;
    while ((r2 = next_fld(p, q, e, g)) > 0) {
      if (g.field == 1 && g.wt == 0) {
        o.action = (uint32_t)g.v;
      } else if (g.field == 3 && g.wt == 2) {
        o.op2_off = g.off;
        o.op2_len = g.len;
      }
    }
    return r2 < 0 ? -1 : 1;
  }
  return rc;
}

// ---- the plan, per message ---------------------------------------------------------
struct PlanView {
  mochi_write2_batch b;
  mochi_write2_answer_source s;
  mochi_write2_answer_planned o;
};
WIRE_HD void slot_put(const mochi_write2_answer_planned& o, uint64_t s, uint8_t status, uint8_t existed, uint8_t flags,
                     uint64_t r_off, uint32_t r_len, uint64_t c_off, uint32_t c_len) {
  o.op_status[s] = status;
  o.op_existed[s] = existed;
  o.op_flags[s] = flags;
  o.op_result_off[s] = r_off;
  o.op_result_len[s] = r_len;
  o.op_cert_off[s] = c_off;
  o.op_cert_len[s] = c_len;
}
WIRE_HD void plan_msg(const PlanView& v, uint32_t m) {
  const mochi_write2_batch& b = v.b;
  const mochi_write2_answer_source& s = v.s;
  const uint32_t o0 = b.op_flags_off[m], o1 = b.op_flags_off[m + 1];
  const uint32_t k = o1 >= o0 ? o1 - o0 : 0;
  const uint64_t s0 = s.slot_off[m];
  // the slots this message may write: its whole run lies below n_slots, or none of it is touched
  const bool run_ok = s0 <= s.n_slots && k <= s.n_slots - s0;
  const uint8_t ms = s.msg_status[m];
  const bool acc = (s.cert_accept_bits[m >> 5] >> (m & 31)) & 1;
  uint8_t st = ms == MOCHI_MSG_FALLBACK ? (acc ? MOCHI_W2A_HOST : MOCHI_W2A_NO_REPLY)
                                        : (ms == MOCHI_MSG_OK && acc ? MOCHI_W2A_REPLY : MOCHI_W2A_NO_REPLY);
  if (st == MOCHI_W2A_REPLY && (k > kMaxOps || !run_ok)) st = MOCHI_W2A_NO_REPLY;
  for (uint32_t j = 0; st == MOCHI_W2A_REPLY && j < k; j++) {
    const uint8_t d = s.op_decision[o0 + j];
    const bool ok = d == MOCHI_OPD_APPLY || d == MOCHI_OPD_WRONG_SHARD ||
                    (d == MOCHI_OPD_READ && !(s.op_store_flags[o0 + j] & MOCHI_W2A_VALUE_NULL));
    if (!ok) st = MOCHI_W2A_NO_REPLY;
  }
  const uint64_t base = b.msg_off[m];
  const uint8_t* p = b.wire + base;
  W2Body t{0, 0, 0, 0};
  if (st == MOCHI_W2A_REPLY) {
    // the operations on the wire must be the k the flags were taken for
    W2Op op;
    uint32_t n = 0, pos = 0;
    int rc = w2_top(p, b.msg_len[m], t) ? 0 : -1;
    if (rc == 0) {
      pos = t.tx_off;
      while ((rc = w2_next_op(p, pos, t.tx_off + t.tx_len, op)) > 0) n++;
    }
    if (rc < 0 || n != k) st = MOCHI_W2A_NO_REPLY;
  }
  if (st == MOCHI_W2A_REPLY) {
    W2Op op;
    uint32_t pos = t.tx_off;
    for (uint32_t j = 0; j < k; j++) {
      (void)w2_next_op(p, pos, t.tx_off + t.tx_len, op);  // counted above: it is there
      const uint32_t i = o0 + j;
      const uint8_t d = s.op_decision[i];
      if (d == MOCHI_OPD_WRONG_SHARD) {
        slot_put(v.o, s0 + j, 1, 0, 0, 0, 0, 0, 0);
      } else if (d == MOCHI_OPD_APPLY) {
        slot_put(v.o, s0 + j, 0, op.action == kActionWrite ? 1 : 0, MOCHI_RAO_HAS_CERT, base + op.op2_off, op.op2_len,
                 base + t.cert_off, t.cert_len);
      } else {
        const bool has = s.op_store_flags[i] & MOCHI_W2A_HAS_STORED_CERT;
        slot_put(v.o, s0 + j, 0, 1,
                 MOCHI_RAO_RESULT_STORE | MOCHI_RAO_CERT_STORE | (has ? MOCHI_RAO_HAS_CERT : 0), s.op_value_off[i],
                 s.op_value_len[i], has ? s.op_stored_cert_off[i] : 0, has ? s.op_stored_cert_len[i] : 0);
      }
    }
  } else if (run_ok) {
    for (uint32_t j = 0; j < k; j++) slot_put(v.o, s0 + j, 0xFF, 0, 0, 0, 0, 0, 0);
  }
  v.o.plan_status[m] = st;
  v.o.resp_kind[m] = st == MOCHI_W2A_REPLY ? MOCHI_RR_WRITE2_ANS : MOCHI_RR_OTHER;
  v.o.resp_n_ops[m] = st == MOCHI_W2A_REPLY ? k : 0;
}

}  // namespace rae

// Device pointers; the context's scratch, laid out by rae_layout.
struct RaeArgs {
  mochi_result_answers in;
  // outputs
  uint8_t* wire;
  uint64_t wire_cap;
  uint64_t* msg_off;  // [P]
  uint32_t* msg_len;  // [P]
  uint8_t* status;    // [P]
  // scratch
  uint32_t* op_rel;   // [S] per slot: the operation's offset inside its TransactionResult body
  uint64_t* op_dst;   // [S][2] wire offsets of the slot's result string and certificate (~0 = none)
  uint32_t* resp_tx;  // [P+1] TransactionResult body length
  uint64_t* len64;    // [P+1] message lengths (scan input), last = 0
  uint64_t* off64;    // [P+1] their exclusive scan; off64[P] = the wire size
  void* scan_temp;
  size_t scan_temp_bytes;
  // per-kernel timing or null: kRaeEvents events, recorded before k_rae_size, after it,
  // after the scan; before k_rae_hdr, after it, after k_rae_copy
  hipEvent_t* ev;
};
constexpr int kRaeEvents = 6;
constexpr int kRaeStages = 4;  // k_rae_size, scan, k_rae_hdr, k_rae_copy
// The per-call scratch layout (a.in.n_resps / n_slots set; every array 16-byte aligned):
// on a null base it only counts and returns the bytes to allocate; on that allocation it
// sets a's scratch pointers.
inline size_t rae_layout(RaeArgs& a, void* base) {
  const size_t p1 = (size_t)a.in.n_resps + 1, S = a.in.n_slots;
  Carve c(base);
  a.op_rel = c.take<uint32_t>(S);
  a.op_dst = c.take<uint64_t>(2 * S);
  a.resp_tx = c.take<uint32_t>(p1);
  a.len64 = c.take<uint64_t>(p1);
  a.off64 = c.take<uint64_t>(p1);
  return c.bytes();
}
// sizes + the 64-bit exclusive scan: fills msg_off / msg_len / status and off64[P]
hipError_t launch_rae_size(const RaeArgs& a, hipStream_t stream);
// headers + payload copy; every kernel writes nothing when off64[P] > wire_cap
hipError_t launch_rae_emit(const RaeArgs& a, hipStream_t stream);
// k_w2a_plan, lane = message
hipError_t launch_w2a_plan(const rae::PlanView& v, hipStream_t stream);

}  // namespace mochi

namespace mochi_host {
// mochi_result_reply_encode / mochi_write2_answer_plan without the null checks of the C
// layer; `err` names an inconsistent input (MOCHI_EINVAL).
int result_reply_encode(const mochi_result_answers* a, uint8_t* wire, uint64_t wire_cap, uint64_t* msg_off,
                        uint32_t* msg_len, uint8_t* status, uint64_t* wire_len, const char** err);
int write2_answer_plan(const mochi_write2_batch* b, const mochi_write2_answer_source* s,
                       mochi_write2_answer_planned* o, const char** err);
}  // namespace mochi_host
