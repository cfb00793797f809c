// w1_request.h — the Write1ToServer request decoder and the key-state join: launch
// interface between the C-ABI layer (capi.cpp) and the device kernels
// (w1_request.hip), the host twin (w1_request_host.cpp), and the parsing both
// share.  Semantics: include/mochi_hip.h (mochi_write1_requests /
// mochi_write1_requests_decoded / mochi_write1_key_state).
//
// Everything under `namespace w1q` is __host__ __device__ and reads a body
// through (base pointer, offsets below the body length) alone, with the field
// walk of wire_walk.h (wire::next_fld and friends): the host form and every
// kernel run the same walk over the same bytes, and a stand-alone host program
// (microbench/w1_request_check.cpp) checks under a sanitizer that no read
// leaves the slice.
//
// Wire layout (MochiProtocol.proto:51-60, :92-97), parsed as protobuf-java
// 3.16.3 parses it (the rules of wire_walk.h):
//   Write1ToServer = [0A clientId] [12 Transaction] [18 seed] [22 transactionHash]
//   Transaction    = { 0A Operation }
//   Operation      = [08 action] [12 operand1] [1A operand2] [22 operand3]
#pragma once
#include "carve.h"
#include "w1_issue.h"
#include "wire_walk.h"

namespace mochi {
namespace w1q {

using wire::Fld;
using wire::kStFb;
using wire::kStMal;
using wire::next_fld;
using wire::valid_utf8;

constexpr uint32_t kMaxReqs = 1u << 24;  // 64 ops each: every total stays below 2^32
constexpr uint32_t kMaxOps = MOCHI_MAX_OPS_PER_CERT;
constexpr uint8_t kWD = MOCHI_W1OP_WRITE | MOCHI_W1OP_DELETE;
constexpr uint8_t kHeld = MOCHI_W1OP_LOCAL | MOCHI_W1OP_HAS_SVOC;

// An Operation at [off, off+len): does it parse (framing, the three strings
// strict UTF-8), its action (the low word of the varint) and operand1, each the
// last occurrence.  An absent operand1 is offset 0, length 0.
struct Op {
  uint32_t action, k_off, k_len;
};
WIRE_HD bool op_level(const uint8_t* p, uint32_t off, uint32_t len, bool check, Op& o) {
  o.action = o.k_off = o.k_len = 0;
  uint32_t pos = off;
  const uint32_t end = off + len;
  Fld f;
  int rc;
  while ((rc = next_fld(p, pos, end, f)) > 0) {
    if (f.field == 1 && f.wt == 0) {
      o.action = (uint32_t)f.v;  // readEnum: readRawVarint32
    } else if (f.wt == 2 && f.field >= 2 && f.field <= 4) {
      if (check && !valid_utf8(p, f.off, f.len)) return false;
      if (f.field == 2) {
        o.k_off = f.off;
        o.k_len = f.len;
      }
    }
  }
  return rc == 0;
}

// the wire half of mochi_write1_batch.op_flags
WIRE_HD uint8_t action_flags(uint32_t action) {
  return action == 2 ? (uint8_t)MOCHI_W1OP_WRITE : action == 1 ? (uint8_t)MOCHI_W1OP_DELETE : (uint8_t)0;
}

// Framing of the Transaction at [off, off+len): its Operation entries counted; false = malformed.
WIRE_HD bool tx_count(const uint8_t* p, uint32_t off, uint32_t len, uint32_t& n_ent) {
  uint32_t pos = off;
  const uint32_t end = off + len;
  Fld f;
  int rc;
  n_ent = 0;
  while ((rc = next_fld(p, pos, end, f)) > 0)
    if (f.field == 1 && f.wt == 2) n_ent++;
  return rc == 0;
}

// ... and every Operation of it, whole
WIRE_HD bool valid_tx(const uint8_t* p, uint32_t off, uint32_t len) {
  uint32_t pos = off;
  const uint32_t end = off + len;
  Fld f;
  int rc;
  while ((rc = next_fld(p, pos, end, f)) > 0) {
    Op o;
    if (f.field == 1 && f.wt == 2 && !op_level(p, f.off, f.len, true, o)) return false;
  }
  return rc == 0;
}

// slice of the j-th Operation entry of a Transaction whose framing tx_count accepted
WIRE_HD void tx_entry(const uint8_t* p, uint32_t off, uint32_t len, uint32_t j, uint32_t& eoff, uint32_t& elen) {
  uint32_t pos = off, i = 0;
  const uint32_t end = off + len;
  Fld f;
  eoff = elen = 0;
  while (next_fld(p, pos, end, f) > 0) {
    if (f.field != 1 || f.wt != 2) continue;
    if (i++ == j) {
      eoff = f.off;
      elen = f.len;
      return;
    }
  }
}

// ---- per request: the top level ---------------------------------------------------
struct Level1 {
  uint32_t tx_off, tx_len;  // the transaction value (absent: empty)
  uint32_t n_ent;           // its Operation entries
  uint32_t seed;
  uint32_t cl_off, cl_len, h_off, h_len;
};
// Returns status bits.  With bits set nothing of `o` is to be used.  A request
// outside the level-by-level shape (a second transaction, more than kMaxOps
// operations) is validated whole here: FALLBACK is never malformed.
WIRE_HD uint32_t req_level(const uint8_t* p, uint32_t len, Level1& o) {
  o.tx_off = o.tx_len = o.n_ent = o.seed = o.cl_off = o.cl_len = o.h_off = o.h_len = 0;
  uint32_t pos = 0, n_tx = 0;
  Fld f;
  int rc;
  while ((rc = next_fld(p, pos, len, f)) > 0) {
    if (f.field == 3 && f.wt == 0) {
      o.seed = (uint32_t)f.v;  // readUInt32: readRawVarint32
    } else if (f.wt == 2 && (f.field == 1 || f.field == 4)) {
      if (!valid_utf8(p, f.off, f.len)) return kStMal;
      if (f.field == 1) {
        o.cl_off = f.off;
        o.cl_len = f.len;
      } else {
        o.h_off = f.off;
        o.h_len = f.len;
      }
    } else if (f.wt == 2 && f.field == 2) {
      n_tx++;
      o.tx_off = f.off;
      o.tx_len = f.len;
    }
  }
  if (rc < 0) return kStMal;
  if (n_tx > 1) {  // a second transaction merges into the first: every one is parsed
    pos = 0;
    while (next_fld(p, pos, len, f) > 0)
      if (f.wt == 2 && f.field == 2 && !valid_tx(p, f.off, f.len)) return kStMal;
    return kStFb;
  }
  if (!tx_count(p, o.tx_off, o.tx_len, o.n_ent)) return kStMal;
  if (o.n_ent > kMaxOps) return valid_tx(p, o.tx_off, o.tx_len) ? kStFb : kStMal;
  return 0;
}

// What the decoder reads and writes: host pointers in the host form, device pointers in the kernels.
struct View {
  mochi_write1_requests in;
  mochi_write1_requests_decoded out;
};

// the per-request outputs but req_op_off; returns the request's op count
WIRE_HD uint32_t final_req(const View& v, uint32_t q, uint32_t bits, const Level1& l) {
  const mochi_write1_requests_decoded& out = v.out;
  const bool ok = bits == 0;
  const uint64_t base = ok ? v.in.msg_off[q] : 0;
  out.req_status[q] = bits & kStMal ? MOCHI_W1Q_MALFORMED : bits & kStFb ? MOCHI_W1Q_FALLBACK : MOCHI_W1Q_OK;
  out.req_seed[q] = ok ? l.seed : 0;
  out.req_hash_off[q] = base + (ok ? l.h_off : 0);
  out.req_hash_len[q] = ok ? l.h_len : 0;
  out.req_client_off[q] = base + (ok ? l.cl_off : 0);
  out.req_client_len[q] = ok ? l.cl_len : 0;
  return ok ? l.n_ent : 0;
}

// op o = entry j of OK request q: key slice and wire flags
WIRE_HD void emit_op(const View& v, uint32_t q, uint32_t tx_off, uint32_t tx_len, uint32_t j, uint32_t o) {
  const uint64_t base = v.in.msg_off[q];
  const uint8_t* b = v.in.wire + base;
  uint32_t eo, el;
  tx_entry(b, tx_off, tx_len, j, eo, el);
  Op op;
  op_level(b, eo, el, false, op);
  v.out.op_key_off[o] = base + op.k_off;
  v.out.op_key_len[o] = op.k_len;
  v.out.op_flags[o] = action_flags(op.action);
}

// does the op take part in the key numbering: one of `part` among its flags and a non-empty key
WIRE_HD bool takes_part(uint8_t flags, uint8_t part, uint32_t key_len) { return (flags & part) && key_len != 0; }
WIRE_HD bool has_key(uint8_t flags, uint32_t key_len) { return takes_part(flags, kWD, key_len); }

// the join, per op (host pointers or device pointers)
struct JoinArgs {
  uint32_t n_reqs, n_ops;
  const uint32_t* req_op_off;
  const uint32_t* req_seed;
  const uint8_t* op_flags_wire;
  const uint32_t* op_obj;
  mochi_write1_key_state ks;
  uint8_t* op_flags;
  int64_t* op_epoch;
  uint32_t* op_stored;
};
WIRE_HD void join_op(const JoinArgs& a, uint32_t o) {
  const uint32_t u = a.op_obj[o];
  uint8_t f = a.op_flags_wire[o];
  int64_t epoch = 0;
  uint32_t stored = MOCHI_W1_NONE;
  if (u != MOCHI_W1_NONE) {
    f |= a.ks.key_flags[u] & kHeld;
    epoch = a.ks.key_epoch[u];
    const int64_t ts = w1_ts(epoch, a.req_seed[wire::request_of(a.req_op_off, a.n_reqs, o)]);
    const uint32_t g1 = a.ks.key_given_off[u + 1];
    for (uint32_t g = a.ks.key_given_off[u]; g < g1; g++)
      if (a.ks.given_ts[g] == ts) {
        stored = a.ks.given_stored[g];
        break;
      }
  }
  a.op_flags[o] = f;
  a.op_epoch[o] = epoch;
  a.op_stored[o] = stored;
}

}  // namespace w1q

// The batch-wide key numbering of a request decoder's ops (this one's and read_request.hip's):
// what k_w1q_claim / k_w1q_rank / k_w1q_number read and write, device pointers.
struct KeyNumArgs {
  const uint8_t* wire;
  const uint64_t* op_key_off;  // [n_ops] into wire
  const uint32_t* op_key_len;
  const uint8_t* op_flags;
  uint8_t part;                // w1q::takes_part's flags
  uint32_t n_ops, slots;       // slots = w1_table_slots(n_ops)
  uint32_t* op_obj;            // [n_ops] out
  uint32_t* key_op;            // [n_keys] out
  uint32_t* n_keys;            // one word, out
  // scratch (key_table_layout)
  uint32_t* tbl_op;    // [slots] the op that claimed the slot, ~0 = empty
  uint32_t* tbl_min;   // [slots] the smallest op index that reached the slot
  uint32_t* op_slot;   // [n_ops] the slot of the op's key, ~0 = the op has no key index
  uint64_t* rep64;     // [n_ops+1] 1 where the op is the first of its key; last = 0
  uint64_t* key_off;   // [n_ops+1] its exclusive scan; key_off[n_ops] = n_keys
  void* scan_temp;
  size_t scan_temp_bytes;
  // per-kernel timing or null: four events, recorded after the table clear + k_w1q_claim,
  // after k_w1q_rank, after the key scan, after k_w1q_number
  hipEvent_t* ev;
};
inline size_t key_table_layout(KeyNumArgs& k, void* base) {
  const size_t o1 = (size_t)k.n_ops + 1;
  Carve c(base);
  k.tbl_op = c.take<uint32_t>(k.slots);  // tbl_op and tbl_min adjacent: one fill
  k.tbl_min = c.take<uint32_t>(k.slots);
  k.op_slot = c.take<uint32_t>(o1);
  k.rep64 = c.take<uint64_t>(o1);
  k.key_off = c.take<uint64_t>(o1);
  return c.bytes();
}
// table clear, claim, rank, scan, number
hipError_t launch_key_number(const KeyNumArgs& k, hipStream_t stream);
// The grid-stride entry kernel (k_w1q_ops) of both request decoders: entry e of the e_base[Q]
// entries is Operation e - e_base[q] of request q's transaction, whose slice is the first two
// words of the request's eight in l1; a malformed one ORs kStMal into st_bits[q].
struct EntryArgs {
  const uint8_t* wire;
  const uint64_t* msg_off;  // [Q]
  uint32_t Q;
  const uint64_t* e_base;   // [Q+1]
  const uint32_t* l1;       // [Q][8]
  uint32_t* st_bits;        // [Q]
};
hipError_t launch_w1q_ops(const EntryArgs& a, hipStream_t stream);
// Device pointers; the signer's scratch.  The per-request part (w1q_layout) is laid
// out before the first launch, the per-op part (key_table_layout on k, with k.n_ops and
// k.slots set) once the host knows n_ops.
struct W1ReqArgs {
  w1q::View v;
  uint32_t Q;
  uint32_t n_ops;      // set after the host wait
  uint32_t* n_keys;    // the caller's device word
  KeyNumArgs k;        // n_ops, slots and the scratch; launch_w1q_emit fills in the rest
  // per-request scratch
  uint32_t* st_bits;   // [Q] kStMal / kStFb, OR-ed in by the entry lanes
  uint32_t* l1;        // [Q][8] w1q::Level1
  uint64_t* cnt_e;     // [Q+1] Operation entries per request accepted so far (scan input)
  uint64_t* e_base;    // [Q+1] their exclusive scan; e_base[Q] = the entry total
  uint64_t* cnt64;     // [Q+1] ops per request (0 unless OK)
  uint64_t* off64;     // [Q+1] its exclusive scan; off64[Q] = n_ops
  void* scan_temp;
  size_t scan_temp_bytes;
  // per-kernel timing or null: kW1ReqEvents events, recorded before k_w1q_req, after it,
  // after the entry scan, after k_w1q_ops, after k_w1q_final + the scan + k_w1q_offsets;
  // before k_w1q_emit, after it, after the table clear + k_w1q_claim, after k_w1q_rank,
  // after the key scan, after k_w1q_number
  hipEvent_t* ev;
};
constexpr int kW1ReqEvents = 11;
constexpr int kW1ReqStages = 9;
// The scratch layouts (a.Q, or k.n_ops and k.slots, set; every array 16-byte aligned): on a
// null base they only count and return the bytes to allocate; on that allocation they
// set the scratch pointers.
inline size_t w1q_layout(W1ReqArgs& a, void* base) {
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
hipError_t launch_w1q_count(const W1ReqArgs& a, hipStream_t stream);
// the per-op arrays, the key numbering and *n_keys (a.n_ops <= op_cap checked by the caller)
hipError_t launch_w1q_emit(const W1ReqArgs& a, hipStream_t stream);
// grid of the grid-stride entry kernel (the entry total is on the device)
inline uint32_t w1q_ops_blocks(uint32_t Q) {
  const uint64_t b = (2 * (uint64_t)Q + 255) / 256;
  return b < 1 ? 1 : b > 4096 ? 4096 : (uint32_t)b;
}
hipError_t launch_w1q_join(const w1q::JoinArgs& a, hipStream_t stream);

}  // namespace mochi

namespace mochi_host {
// mochi_write1_request_decode / mochi_write1_state_join without the null checks of the C
// layer; `err` names an inconsistent input (MOCHI_EINVAL).  MOCHI_EINVAL with *err ==
// nullptr: op_cap is too small (out->n_ops holds the count needed).
int write1_request_decode(const mochi_write1_requests* in, mochi_write1_requests_decoded* out, const char** err);
int write1_state_join(const mochi::w1q::JoinArgs* a, const char** err);
}  // namespace mochi_host
