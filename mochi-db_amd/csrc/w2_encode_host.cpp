// w2_encode_host.cpp — the host form of the Write2ToServer encoder
// (mochi_write2_encode): plain C++, no GPU.  It is the CPU twin of
// w2_encode.hip (same sizes through w2_encode.h, same statuses, same bytes) and
// the fallback where no device is at hand.
#include <cstdint>
#include <cstring>
#include <vector>

#include "w2_encode.h"
#include "wire_put.h"

namespace mochi_host {

int write2_encode(const mochi_write2_source* s, const uint8_t* ids, const uint32_t* id_off, uint32_t n_ids,
                  uint8_t* wire, uint64_t wire_cap, uint64_t* msg_off, uint32_t* msg_len, uint8_t* status,
                  uint64_t* wire_len, const char** err) {
  using namespace mochi;
  const uint32_t M = s->n_msgs, NM = s->n_mgs, N = s->n_grants, O = s->n_ops;
  auto bad = [&](const char* what) {
    *err = what;
    return MOCHI_EINVAL;
  };
  auto csr = [](const uint32_t* off, uint32_t n, uint32_t total) {
    if (off[0] != 0 || off[n] != total) return false;
    for (uint32_t i = 0; i < n; i++)
      if (off[i + 1] < off[i]) return false;
    return true;
  };
  if (!csr(s->cert_mg_off, M, NM)) return bad("cert_mg_off is not a CSR over n_mgs");
  if (!csr(s->mg_grant_off, NM, N)) return bad("mg_grant_off is not a CSR over n_grants");
  if (!csr(s->cert_op_off, M, O)) return bad("cert_op_off is not a CSR over n_ops");
  auto in_strings = [&](uint64_t off, uint32_t len) { return inside(off, len, s->strings_len); };
  for (uint32_t o = 0; o < O; o++)
    if (!in_strings(s->op1_off[o], s->op1_len[o]) || (s->op2_off && !in_strings(s->op2_off[o], s->op2_len[o])))
      return bad("an operand lies outside strings");
  if (s->client_off)
    for (uint32_t m = 0; m < M; m++)
      if (!in_strings(s->client_off[m], s->client_len[m])) return bad("a client id lies outside strings");

  // level 1: per grant the objectId slice, per MultiGrant the bytes of its map entries
  std::vector<uint32_t> g_oid(2 * (size_t)N);
  std::vector<uint64_t> mg_gpart(NM);
  std::vector<uint8_t> mg_bad(NM, 0);
  for (uint32_t i = 0; i < NM; i++) {
    uint64_t part = 0;
    for (uint32_t g = s->mg_grant_off[i]; g < s->mg_grant_off[i + 1]; g++) {
      const uint64_t go = s->grant_off[g];
      const uint32_t gl = s->grant_len[g];
      // does the Grant parse, and where is its objectId (the last field 1 given): the
      // pointer walk's parser, which decides as proto_dev.h's does in w2_encode.hip
      wire::Grant gr;
      if (!inside(go, gl, s->grant_bytes_len) || !wire::parse_grant(s->grant_bytes + go, 0, gl, gr)) {
        mg_bad[i] = 1;
        continue;
      }
      const uint32_t ol = gr.oid_len;
      g_oid[2 * (size_t)g] = gr.oid_off;
      g_oid[2 * (size_t)g + 1] = ol;
      part += enc_ld_size(enc_e1_body(ol, gl));
      if (s->sig) part += enc_ld_size(enc_e5_body(ol));
    }
    mg_gpart[i] = part;
  }
  // level 2: per message the certificate, transaction and message lengths; the offsets
  std::vector<uint64_t> wc_len(M), tx_len(M);
  uint64_t total = 0;
  for (uint32_t m = 0; m < M; m++) {
    const uint32_t cl = s->client_off ? s->client_len[m] : 0;
    bool bad_grant = false, bad_signer = false;
    uint64_t wc = 0, tx = 0;
    for (uint32_t i = s->cert_mg_off[m]; i < s->cert_mg_off[m + 1]; i++) {
      bad_grant |= mg_bad[i] != 0;
      const uint32_t sg = s->mg_signer[i];
      if (sg >= n_ids) {
        bad_signer = true;
        continue;
      }
      const uint32_t sl = id_off[sg + 1] - id_off[sg];
      const uint64_t mg = mg_gpart[i] + enc_ld_opt_size(cl) + enc_ld_opt_size(sl);
      wc += enc_ld_size(enc_ld_size(sl) + enc_ld_size(mg));
    }
    for (uint32_t o = s->cert_op_off[m]; o < s->cert_op_off[m + 1]; o++)
      tx += enc_ld_size(enc_op_body(s->op_action[o], s->op1_len[o], s->op2_off ? s->op2_len[o] : 0));
    const uint64_t len = enc_ld_opt_size(wc) + enc_ld_opt_size(tx);
    const uint8_t st = bad_grant ? MOCHI_ENC_BAD_GRANT : bad_signer ? MOCHI_ENC_BAD_SIGNER
                       : len > kEncMaxMsg ? MOCHI_ENC_TOO_LONG : MOCHI_ENC_OK;
    status[m] = st;
    msg_len[m] = st == MOCHI_ENC_OK ? (uint32_t)len : 0;
    msg_off[m] = total;
    total += msg_len[m];
    wc_len[m] = wc;
    tx_len[m] = tx;
  }
  *wire_len = total;
  if (total > wire_cap) return bad("wire_cap is smaller than the encoded size (*wire_len)");
  // emit
  for (uint32_t m = 0; m < M; m++) {
    if (status[m] != MOCHI_ENC_OK) continue;
    uint8_t* o = wire + msg_off[m];
    const uint8_t* cid = s->client_off ? s->strings + s->client_off[m] : nullptr;
    const uint32_t cl = s->client_off ? s->client_len[m] : 0;
    if (wc_len[m]) {
      *o++ = 0x0A;
      o = put_varint(o, wc_len[m]);
      for (uint32_t i = s->cert_mg_off[m]; i < s->cert_mg_off[m + 1]; i++) {
        const uint32_t sg = s->mg_signer[i];
        const uint8_t* sid = ids + id_off[sg];
        const uint32_t sl = id_off[sg + 1] - id_off[sg];
        const uint64_t mg = mg_gpart[i] + enc_ld_opt_size(cl) + enc_ld_opt_size(sl);
        *o++ = 0x0A;
        o = put_varint(o, enc_ld_size(sl) + enc_ld_size(mg));
        o = put_ld(o, 0x0A, sid, sl);
        *o++ = 0x12;
        o = put_varint(o, mg);
        const uint32_t g0 = s->mg_grant_off[i], g1 = s->mg_grant_off[i + 1];
        for (uint32_t g = g0; g < g1; g++) {
          const uint8_t* gb = s->grant_bytes + s->grant_off[g];
          const uint32_t gl = s->grant_len[g], oo = g_oid[2 * (size_t)g], ol = g_oid[2 * (size_t)g + 1];
          *o++ = 0x0A;
          o = put_varint(o, enc_e1_body(ol, gl));
          o = put_ld(o, 0x0A, gb + oo, ol);
          o = put_ld(o, 0x12, gb, gl);
        }
        if (cl) o = put_ld(o, 0x12, cid, cl);
        if (sl) o = put_ld(o, 0x22, sid, sl);
        if (s->sig)
          for (uint32_t g = g0; g < g1; g++) {
            const uint8_t* gb = s->grant_bytes + s->grant_off[g];
            const uint32_t oo = g_oid[2 * (size_t)g], ol = g_oid[2 * (size_t)g + 1];
            *o++ = 0x2A;
            o = put_varint(o, enc_e5_body(ol));
            o = put_ld(o, 0x0A, gb + oo, ol);
            o = put_ld(o, 0x12, s->sig + (size_t)MOCHI_RSA_BYTES * g, MOCHI_RSA_BYTES);
          }
      }
    }
    if (tx_len[m]) {
      *o++ = 0x12;
      o = put_varint(o, tx_len[m]);
      for (uint32_t q = s->cert_op_off[m]; q < s->cert_op_off[m + 1]; q++) {
        const uint32_t act = s->op_action[q], l1 = s->op1_len[q], l2 = s->op2_off ? s->op2_len[q] : 0;
        *o++ = 0x0A;
        o = put_varint(o, enc_op_body(act, l1, l2));
        if (act) {
          *o++ = 0x08;
          o = put_varint(o, act);
        }
        if (l1) o = put_ld(o, 0x12, s->strings + s->op1_off[q], l1);
        if (l2) o = put_ld(o, 0x1A, s->strings + s->op2_off[q], l2);
      }
    }
    if ((uint64_t)(o - (wire + msg_off[m])) != msg_len[m]) return bad("internal: emitted size differs from computed size");
  }
  return MOCHI_OK;
}

}  // namespace mochi_host
