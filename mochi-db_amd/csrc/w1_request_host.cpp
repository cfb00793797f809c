// w1_request_host.cpp — the host forms of the Write1 request decoder and of the
// key-state join: the walk of w1_request.h (the one the kernels of w1_request.hip
// run), request by request, in the same phases.  No GPU, no signer.  The key
// numbering uses a hash map where the device uses its claim table; both number the
// keys by their first op in op order.
#include <string_view>
#include <unordered_map>
#include <vector>

#include "w1_request.h"

namespace mochi_host {

using namespace mochi::w1q;

int write1_request_decode(const mochi_write1_requests* in, mochi_write1_requests_decoded* out, const char** err) {
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
      Op op;
      tx_entry(b, l1[q].tx_off, l1[q].tx_len, j, eo, el);
      if (!op_level(b, eo, el, true, op)) bits = mochi::wire::kStMal;
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
      if (has_key(out->op_flags[o], out->op_key_len[o])) {
        const auto r = keys.emplace(std::string_view((const char*)in->wire + out->op_key_off[o], out->op_key_len[o]), n_keys);
        u = r.first->second;
        if (r.second) out->key_op[n_keys++] = o;
      }
      out->op_obj[o] = u;
    }
  out->n_keys = n_keys;
  return MOCHI_OK;
}

int write1_state_join(const JoinArgs* a, const char** err) {
  *err = nullptr;
  const uint32_t Q = a->n_reqs, O = a->n_ops, U = a->ks.n_keys;
  if (a->req_op_off[0] != 0 || a->req_op_off[Q] != O) *err = "req_op_off is not a CSR over n_ops";
  for (uint32_t q = 0; q < Q && !*err; q++)
    if (a->req_op_off[q] > a->req_op_off[q + 1]) *err = "req_op_off is not a CSR over n_ops";
  if (!*err && (a->ks.key_given_off[0] != 0 || a->ks.key_given_off[U] != a->ks.n_given))
    *err = "key_given_off is not a CSR over n_given";
  for (uint32_t u = 0; u < U && !*err; u++)
    if (a->ks.key_given_off[u] > a->ks.key_given_off[u + 1]) *err = "key_given_off is not a CSR over n_given";
  for (uint32_t o = 0; o < O && !*err; o++)
    if (a->op_obj[o] != MOCHI_W1_NONE && a->op_obj[o] >= U) *err = "an op_obj is not below n_keys";
  if (*err) return MOCHI_EINVAL;
  for (uint32_t o = 0; o < O; o++) join_op(*a, o);
  return MOCHI_OK;
}

}  // namespace mochi_host
