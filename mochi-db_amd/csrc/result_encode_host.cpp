// result_encode_host.cpp — the host forms of the answer encoder
// (mochi_result_reply_encode) and of the Write2 answer plan
// (mochi_write2_answer_plan): plain C++, no GPU, no context.  They are the CPU
// twins of result_encode.hip (same sizes, same walk and the same per-message
// plan through result_encode.h, same statuses, same bytes) and the ones of the
// two that check their inputs.
#include <cstdint>
#include <cstring>
#include <vector>

#include "result_encode.h"
#include "wire_put.h"

namespace mochi_host {

using namespace mochi::rae;

int result_reply_encode(const mochi_result_answers* a, uint8_t* wire, uint64_t wire_cap, uint64_t* msg_off,
                        uint32_t* msg_len, uint8_t* status, uint64_t* wire_len, const char** err) {
  using namespace mochi;
  const uint32_t P = a->n_resps;
  auto bad = [&](const char* what) {
    *err = what;
    return MOCHI_EINVAL;
  };
  *wire_len = 0;
  for (uint32_t p = 0; p < P; p++) {
    const uint8_t kind = a->resp_kind[p];
    if (kind > MOCHI_RR_OTHER) return bad("resp_kind is no MOCHI_RR_*");
    if (!body_kind(kind)) continue;
    const uint32_t k = a->resp_n_ops[p];
    const uint64_t s0 = a->slot_off[p];
    if (k > kMaxOps) return bad("a response has more than MOCHI_MAX_OPS_PER_CERT ops");
    if (s0 > a->n_slots || k > a->n_slots - s0) return bad("a slot run lies outside n_slots");
    if (a->rid_off && !inside(a->rid_off[p], a->rid_len[p], a->ids_len)) return bad("a rid lies outside ids");
    if (a->nonce_off && kind == MOCHI_RR_READ && !inside(a->nonce_off[p], a->nonce_len[p], a->ids_len))
      return bad("a nonce lies outside ids");
    for (uint64_t s = s0; s < s0 + k; s++) {
      const uint8_t fl = a->op_flags[s];
      if (!inside(a->op_result_off[s], a->op_result_len[s], fl & MOCHI_RAO_RESULT_STORE ? a->store_len : a->wire_len))
        return bad("a result slice lies outside its blob");
      if ((fl & MOCHI_RAO_HAS_CERT) &&
          !inside(a->op_cert_off[s], a->op_cert_len[s], fl & MOCHI_RAO_CERT_STORE ? a->store_len : a->wire_len))
        return bad("a certificate slice lies outside its blob");
    }
  }

  // sizes and offsets
  std::vector<uint64_t> tx(P);
  uint64_t total = 0;
  for (uint32_t p = 0; p < P; p++) {
    const Sized z = size_resp(*a, p, nullptr);
    tx[p] = z.tx;
    status[p] = z.status;
    msg_len[p] = (uint32_t)z.len;
    msg_off[p] = total;
    total += z.len;
  }
  *wire_len = total;
  if (total > wire_cap) return bad("wire_cap is smaller than the encoded size (*wire_len)");

  // emit
  for (uint32_t p = 0; p < P; p++) {
    if (!body_kind(a->resp_kind[p]) || status[p] != MOCHI_ENC_OK) continue;
    const bool read = a->resp_kind[p] == MOCHI_RR_READ;
    uint8_t* o = wire + msg_off[p];
    *o++ = 0x0A;
    o = put_varint(o, tx[p]);
    for (uint64_t s = a->slot_off[p]; s < a->slot_off[p] + a->resp_n_ops[p]; s++) {
      const uint8_t fl = a->op_flags[s], st = a->op_status[s];
      *o++ = 0x0A;
      o = put_varint(o, op_body(*a, s));
      if (a->op_result_len[s])
        o = put_ld(o, 0x0A, (fl & MOCHI_RAO_RESULT_STORE ? a->store : a->wire) + a->op_result_off[s], a->op_result_len[s]);
      if (fl & MOCHI_RAO_HAS_CERT)
        o = put_ld(o, 0x12, (fl & MOCHI_RAO_CERT_STORE ? a->store : a->wire) + a->op_cert_off[s], a->op_cert_len[s]);
      if (a->op_existed[s]) {
        *o++ = 0x18;
        *o++ = 0x01;
      }
      if (st) {
        *o++ = 0x20;
        o = put_varint(o, st);
      }
    }
    const uint32_t rl = rid_len(*a, p), nl = nonce_len(*a, p);
    if (nl) o = put_ld(o, 0x12, a->ids + a->nonce_off[p], nl);
    if (rl) o = put_ld(o, read ? 0x1A : 0x12, a->ids + a->rid_off[p], rl);
    if ((uint64_t)(o - (wire + msg_off[p])) != msg_len[p]) return bad("internal: emitted size differs from computed size");
  }
  return MOCHI_OK;
}

int write2_answer_plan(const mochi_write2_batch* b, const mochi_write2_answer_source* s,
                       mochi_write2_answer_planned* o, const char** err) {
  const uint32_t M = b->n_msgs;
  auto bad = [&](const char* what) {
    *err = what;
    return MOCHI_EINVAL;
  };
  if (b->op_flags_off[0] != 0) return bad("op_flags_off is not a CSR");
  for (uint32_t m = 0; m < M; m++) {
    if (!inside(b->msg_off[m], b->msg_len[m], b->wire_len)) return bad("a message slice lies outside wire");
    const uint32_t o0 = b->op_flags_off[m], o1 = b->op_flags_off[m + 1];
    if (o1 < o0) return bad("op_flags_off is not a CSR");
    if (s->slot_off[m] > s->n_slots || o1 - o0 > s->n_slots - s->slot_off[m]) return bad("a slot run lies outside n_slots");
    for (uint32_t i = o0; i < o1; i++) {
      if (!inside(s->op_value_off[i], s->op_value_len[i], s->store_len)) return bad("a stored value lies outside store_len");
      if ((s->op_store_flags[i] & MOCHI_W2A_HAS_STORED_CERT) &&
          !inside(s->op_stored_cert_off[i], s->op_stored_cert_len[i], s->store_len))
        return bad("a stored certificate lies outside store_len");
    }
  }
  const PlanView v{*b, *s, *o};
  for (uint32_t m = 0; m < M; m++) plan_msg(v, m);
  return MOCHI_OK;
}

}  // namespace mochi_host
