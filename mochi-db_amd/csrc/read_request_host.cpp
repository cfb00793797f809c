// read_request_host.cpp — the host forms of the ReadToServer request decoder and of the
// read answer plan: the walk of read_request.h and w1_request.h (the one the kernels of
// read_request.hip run), request by request, in the same phases.  No GPU, no context.
// The key numbering uses a hash map where the device uses its claim table; both number
// the keys by their first op in op order.
#include <string_view>
#include <unordered_map>
#include <vector>

#include "read_request.h"

namespace mochi_host {

using namespace mochi::rdq;

int read_request_decode(const mochi_read_requests* in, mochi_read_requests_decoded* out, const char** err) {
  *err = nullptr;
  const uint32_t Q = in->n_reqs;
  if (Q > kMaxReqs) {
    *err = "more than 2^24 requests";
    return MOCHI_EINVAL;
  }
  for (uint32_t q = 0; q < Q; q++)
    if (in->msg_off[q] > in->wire_len || in->msg_len[q] > in->wire_len - in->msg_off[q]) {
      *err = "a request slice lies outside wire";
      return MOCHI_EINVAL;
    }
  const View v{*in, *out};
  std::vector<Level1> l1(Q);
  uint32_t n_ops = 0;
  for (uint32_t q = 0; q < Q; q++) {
    const uint8_t* b = in->wire + in->msg_off[q];
    uint32_t bits = req_level(b, in->msg_len[q], l1[q]);
    for (uint32_t j = 0; !bits && j < l1[q].n_ent; j++) {
      uint32_t eo, el;
      mochi::w1q::Op op;
      mochi::w1q::tx_entry(b, l1[q].tx_off, l1[q].tx_len, j, eo, el);
      if (!mochi::w1q::op_level(b, eo, el, true, op)) bits = kStMal;
    }
    out->req_op_off[q] = n_ops;
    n_ops += final_req(v, q, bits, l1[q]);
  }
  out->req_op_off[Q] = out->n_ops = n_ops;
  out->n_keys = 0;
  if (n_ops > out->op_cap) return MOCHI_EINVAL;
  std::unordered_map<std::string_view, uint32_t> keys;
  uint32_t n_keys = 0;
  for (uint32_t q = 0; q < Q; q++)
    for (uint32_t o = out->req_op_off[q]; o < out->req_op_off[q + 1]; o++) {
      emit_op(v, q, l1[q].tx_off, l1[q].tx_len, o - out->req_op_off[q], o);
      uint32_t u = MOCHI_W1_NONE;
      if (mochi::w1q::takes_part(out->op_flags[o], MOCHI_RDOP_READ, out->op_key_len[o])) {
        const auto r = keys.emplace(std::string_view((const char*)in->wire + out->op_key_off[o], out->op_key_len[o]), n_keys);
        u = r.first->second;
        if (r.second) out->key_op[n_keys++] = o;
      }
      out->op_obj[o] = u;
    }
  out->n_keys = n_keys;
  return MOCHI_OK;
}

int read_answer_plan(const PlanView* v, const char** err) {
  *err = nullptr;
  const uint32_t Q = v->n_reqs, O = v->d.n_ops, U = v->k.n_keys;
  const uint64_t S = v->k.store_len;
  if (v->d.req_op_off[0] != 0 || v->d.req_op_off[Q] != O) *err = "req_op_off is not a CSR over n_ops";
  for (uint32_t q = 0; q < Q && !*err; q++)
    if (v->d.req_op_off[q] > v->d.req_op_off[q + 1]) *err = "req_op_off is not a CSR over n_ops";
  for (uint32_t o = 0; o < O && !*err; o++)
    if (v->d.op_obj[o] != MOCHI_W1_NONE && v->d.op_obj[o] >= U) *err = "an op_obj is not below n_keys";
  for (uint32_t u = 0; u < U && !*err; u++)
    if (v->k.key_value_off[u] > S || v->k.key_value_len[u] > S - v->k.key_value_off[u] || v->k.key_cert_off[u] > S ||
        v->k.key_cert_len[u] > S - v->k.key_cert_off[u])
      *err = "a key slice lies outside the store blob";
  if (*err) return MOCHI_EINVAL;
  for (uint32_t q = 0; q < Q; q++) plan_req(*v, q);
  return MOCHI_OK;
}

}  // namespace mochi_host
