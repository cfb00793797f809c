// w1_decode_host.cpp — the host form of the Write1 reply decoder: the walk of
// w1_decode.h (the one the kernels of w1_decode.hip run), response by response,
// in the same phases.  No GPU, no context.
#include <vector>

#include "w1_decode.h"

namespace mochi_host {

using namespace mochi::w1d;

namespace {

const char* check_input(const mochi_write1_replies* in) {
  const uint32_t P = in->n_resps, Q = in->n_reqs, O = in->n_ops;
  if (P > kMaxResps) return "more than 2^24 responses";
  for (uint32_t p = 0; p < P; p++) {
    if (in->resp_off[p] > in->wire_len || in->resp_len[p] > in->wire_len - in->resp_off[p])
      return "a response slice lies outside wire";
    if (in->resp_kind[p] > MOCHI_W1_OTHER) return "resp_kind is no MOCHI_W1_*";
  }
  if (Q == 0) return P || O ? "responses or ops without a request" : nullptr;
  if (in->req_resp_off[0] != 0 || in->req_resp_off[Q] != P) return "req_resp_off is not a CSR over n_resps";
  if (in->req_op_off[0] != 0 || in->req_op_off[Q] != O) return "req_op_off is not a CSR over n_ops";
  for (uint32_t q = 0; q < Q; q++) {
    if (in->req_resp_off[q] > in->req_resp_off[q + 1]) return "req_resp_off is not a CSR over n_resps";
    if (in->req_op_off[q] > in->req_op_off[q + 1]) return "req_op_off is not a CSR over n_ops";
    if (in->req_op_off[q + 1] - in->req_op_off[q] > MOCHI_MAX_OPS_PER_CERT)
      return "a request has more than MOCHI_MAX_OPS_PER_CERT ops";
  }
  for (uint32_t o = 0; o < O; o++)
    if (in->op_key_off[o] > in->strings_len || in->op_key_len[o] > in->strings_len - in->op_key_off[o])
      return "an operand slice lies outside strings";
  return nullptr;
}

}  // namespace

int write1_reply_decode(const mochi_write1_replies* in, const uint8_t* ids, const uint32_t* id_off, uint32_t n_ids,
                        mochi_write1_decoded* out, const char** err) {
  *err = check_input(in);
  if (*err) return MOCHI_EINVAL;
  const uint32_t P = in->n_resps;
  std::vector<Level1> l1(P);
  uint32_t ng_tot = 0, nc_tot = 0;
  for (uint32_t p = 0; p < P; p++) {
    const uint8_t kind = in->resp_kind[p];
    const uint64_t base = in->resp_off[p];
    const uint8_t* b = in->wire + base;
    uint8_t st = MOCHI_W1R_OK, kind_out = kind;
    uint32_t server = 0x80000000u | p, ng = 0, nc = 0, cl_len = 0;
    uint16_t signer = 0xFFFF;
    uint64_t cl_off = 0;
    l1[p] = Level1{0, 0, 0, 0};
    if (parsed_kind(kind)) {
      // level 1, then level 2 over the MultiGrant and every certificate entry
      uint32_t bits = resp_level(b, in->resp_len[p], l1[p]);
      Level2 l2{0, 0, 0, 0, 0};
      if (!bits) {
        bits |= mg_level(b, l1[p].mg_off, l1[p].mg_len, l2);
        for (uint32_t j = 0; j < l1[p].n_ce; j++) {
          uint32_t vo, vl;
          cert_entry_value(b, in->resp_len[p], j, vo, vl);
          if (!valid_writecert(b, vo, vl)) bits |= kStMal;
        }
      }
      if (bits & kStMal) st = MOCHI_W1R_MALFORMED;
      else if (bits & kStFb) st = MOCHI_W1R_FALLBACK;
      if (st != MOCHI_W1R_OK) {
        kind_out = MOCHI_W1_OTHER;
      } else {
        signer = find_server(b + l2.sid_off, l2.sid_len, ids, id_off, n_ids);
        if (signer == 0xFFFF) st = MOCHI_W1R_UNKNOWN_SERVER;
        else server = signer;
        cl_off = base + l2.cl_off;
        cl_len = l2.cl_len;
        ng = l2.ng;
        nc = l1[p].n_keys;
      }
    }
    out->resp_status[p] = st;
    out->resp_kind_out[p] = kind_out;
    out->resp_server[p] = server;
    out->mg_signer[p] = signer;
    out->resp_client_off[p] = cl_off;
    out->resp_client_len[p] = cl_len;
    out->resp_grant_off[p] = ng_tot;
    out->resp_cert_off[p] = nc_tot;
    ng_tot += ng;
    nc_tot += nc;
  }
  out->resp_grant_off[P] = out->n_grants = ng_tot;
  out->resp_cert_off[P] = out->n_certs = nc_tot;
  if (ng_tot > out->grant_cap || nc_tot > out->cert_cap) return MOCHI_EINVAL;
  View v{*in, ids, id_off, n_ids, *out, nullptr};
  for (uint32_t p = 0; p < P; p++)
    if (out->resp_grant_off[p + 1] != out->resp_grant_off[p] || out->resp_cert_off[p + 1] != out->resp_cert_off[p])
      emit_resp(v, p, l1[p].mg_off, l1[p].mg_len, out->resp_grant_off[p], out->resp_cert_off[p]);
  return MOCHI_OK;
}

}  // namespace mochi_host
