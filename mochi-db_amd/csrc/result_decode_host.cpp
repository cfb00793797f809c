// result_decode_host.cpp — the host form of the result reply decoder and of the
// coalescing step: the walk of result_decode.h (the one the kernels of
// result_decode.hip run), response by response, in the same phases.  No GPU, no
// context.
#include "result_decode.h"

namespace mochi_host {

using namespace mochi::rrd;

namespace {

const char* check_input(const mochi_result_replies* in) {
  const uint32_t P = in->n_resps, Q = in->n_reqs;
  if (P > mochi::wire::kMaxResps) return "more than 2^24 responses";
  for (uint32_t p = 0; p < P; p++) {
    if (in->resp_off[p] > in->wire_len || in->resp_len[p] > in->wire_len - in->resp_off[p])
      return "a response slice lies outside wire";
    if (in->resp_kind[p] > MOCHI_RR_OTHER) return "resp_kind is no MOCHI_RR_*";
  }
  if (Q == 0) return P ? "responses without a request" : nullptr;
  if (in->req_resp_off[0] != 0 || in->req_resp_off[Q] != P) return "req_resp_off is not a CSR over n_resps";
  for (uint32_t q = 0; q < Q; q++) {
    if (in->req_resp_off[q] > in->req_resp_off[q + 1]) return "req_resp_off is not a CSR over n_resps";
    if (in->n_ops[q] > kMaxOps) return "a request has more than MOCHI_MAX_OPS_PER_CERT ops";
  }
  return nullptr;
}

}  // namespace

int result_reply_decode(const mochi_result_replies* in, mochi_result_decoded* out, const char** err) {
  *err = check_input(in);
  if (*err) return MOCHI_EINVAL;
  const View v{*in, *out};
  for (uint32_t q = 0; q < in->n_reqs; q++) {
    const uint32_t n_ops = in->n_ops[q];
    for (uint32_t p = in->req_resp_off[q]; p < in->req_resp_off[q + 1]; p++) {
      const uint8_t* b = in->wire + in->resp_off[p];
      const uint8_t kind = in->resp_kind[p];
      // level 1, level 3 over the operations it hands on, level 4
      Level1 l{0, 0, 0, 0, 0, 0, 0};
      uint32_t bits = parsed_kind(kind) ? resp_level(b, in->resp_len[p], kind, l) : 0u;
      const uint32_t n3 = level3_ops(bits, l.n_wire);
      for (uint32_t j = 0; j < n3; j++) bits |= op_level(v, p, l.tr_off, l.tr_len, j, n_ops);
      resp_final(v, p, bits, l, n_ops);
    }
  }
  return MOCHI_OK;
}

int result_coalesce(const mochi_result_tallied* in, mochi_result_coalesced* out, const char** err) {
  *err = nullptr;
  for (uint32_t q = 0; q < in->n_reqs; q++) {
    if (in->req_resp_off[q] > in->req_resp_off[q + 1]) *err = "req_resp_off descends";
    else if (in->n_ops[q] > kMaxOps) *err = "a request has more than MOCHI_MAX_OPS_PER_CERT ops";
    else if ((in->accept_bits[q >> 5] >> (q & 31)) & 1)
      for (uint32_t j = 0; j < in->n_ops[q]; j++) {
        const int32_t c = in->chosen[in->chosen_off[q] + j];
        if (c >= 0 && (uint32_t)c >= in->req_resp_off[q + 1] - in->req_resp_off[q])
          *err = "a chosen index lies past the request's responses";
      }
    if (*err) return MOCHI_EINVAL;
  }
  for (uint32_t q = 0; q < in->n_reqs; q++) coalesce_req(*in, *out, q);
  return MOCHI_OK;
}

}  // namespace mochi_host
