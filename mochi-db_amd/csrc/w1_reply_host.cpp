// w1_reply_host.cpp — the host form of the Write1 reply encoder
// (mochi_write1_reply_encode): plain C++, no GPU, no key.  It is the CPU twin
// of w1_reply.hip (same sizes through w1_reply.h, same statuses, same bytes)
// and the one of the two that checks its inputs.
#include <cstdint>
#include <cstring>
#include <vector>

#include "w1_reply.h"
#include "wire_put.h"

namespace mochi_host {
namespace {

// one listed grant of a reply
struct Entry {
  const uint8_t *key, *grant, *sig, *cert;
  uint32_t key_len, grant_len, cert_len;
};

}  // namespace

int write1_reply_encode(const mochi_write1_batch* b, const mochi_write1_issued* o, const mochi_write1_reply_source* s,
                        uint8_t* wire, uint64_t wire_cap, uint64_t* msg_off, uint32_t* msg_len, uint8_t* status,
                        uint64_t* wire_len, const char** err) {
  using namespace mochi;
  const uint32_t Q = b->n_reqs, O = b->n_ops, S = b->n_stored;
  const bool with_sig = o->sig != nullptr, with_certs = s->op_cert_off != nullptr;
  auto bad = [&](const char* what) {
    *err = what;
    return MOCHI_EINVAL;
  };
  *wire_len = 0;
  if (b->req_op_off[0] != 0 || b->req_op_off[Q] != O) return bad("req_op_off is not a CSR over n_ops");
  if (o->req_grant_off[0] != 0 || o->req_grant_off[Q] > O) return bad("req_grant_off is not a CSR of at most n_ops references");
  for (uint32_t q = 0; q < Q; q++) {
    if (b->req_op_off[q + 1] < b->req_op_off[q]) return bad("req_op_off is not a CSR over n_ops");
    if (o->req_grant_off[q + 1] < o->req_grant_off[q]) return bad("req_grant_off is not a CSR of at most n_ops references");
    if (o->req_kind[q] > MOCHI_W1K_THROWS) return bad("a req_kind is no mochi_w1_req_kind");
    if (s->req_client_off && !inside(s->req_client_off[q], s->req_client_len[q], s->ids_len))
      return bad("a client id lies outside ids");
  }
  if (!inside(s->server_id_off, s->server_id_len, s->ids_len)) return bad("the server id lies outside ids");
  if (with_sig && S && !s->stored_sig) return bad("stored_sig is required when signatures are written and n_stored > 0");

  // the entries of every reply, in req_grant order
  std::vector<Entry> ent(o->req_grant_off[Q]);
  for (uint32_t q = 0; q < Q; q++) {
    const uint32_t o0 = b->req_op_off[q], o1 = b->req_op_off[q + 1];
    const uint8_t kind = o->req_kind[q];
    for (uint32_t e = o->req_grant_off[q]; e < o->req_grant_off[q + 1]; e++) {
      const uint32_t r = o->req_grant[e];
      Entry& t = ent[e];
      if (r & MOCHI_W1_STORED) {
        const uint32_t i = r & ~MOCHI_W1_STORED;
        if (i >= S) return bad("a req_grant reference lies outside n_stored");
        if (!inside(s->stored_off[i], s->stored_len[i], s->stored_bytes_len)) return bad("a stored grant lies outside stored_bytes");
        t.grant = s->stored_bytes + s->stored_off[i];
        t.grant_len = s->stored_len[i];
        t.sig = with_sig ? s->stored_sig + (size_t)MOCHI_RSA_BYTES * i : nullptr;
      } else {
        if (r >= o->n_new) return bad("a req_grant reference lies outside n_new");
        if (!inside(o->grant_off[r], o->grant_len[r], o->grant_bytes_len)) return bad("a new grant lies outside grant_bytes");
        t.grant = o->grant_bytes + o->grant_off[r];
        t.grant_len = o->grant_len[r];
        t.sig = with_sig ? o->sig + (size_t)MOCHI_RSA_BYTES * r : nullptr;
      }
      uint32_t op = o0;
      while (op < o1 && !(o->op_grant[op] == r && w1r_listed(kind, o->op_decision[op]))) op++;
      if (op == o1) return bad("a req_grant reference that no listed op of its request refers to");
      if (!inside(b->op_key_off[op], b->op_key_len[op], b->strings_len)) return bad("a key lies outside strings");
      t.key = b->strings + b->op_key_off[op];
      t.key_len = b->op_key_len[op];
      t.cert = nullptr;
      t.cert_len = 0;
      if (with_certs) {
        if (!inside(s->op_cert_off[op], s->op_cert_len[op], s->certs_len)) return bad("a certificate lies outside certs");
        t.cert = s->certs + s->op_cert_off[op];
        t.cert_len = s->op_cert_len[op];
      }
    }
  }

  // sizes and offsets
  const uint32_t sl = s->server_id_len;
  std::vector<uint64_t> mg_len(Q);
  uint64_t total = 0;
  for (uint32_t q = 0; q < Q; q++) {
    uint64_t len = 0;
    status[q] = MOCHI_ENC_OK;
    if (o->req_kind[q] != MOCHI_W1K_THROWS) {
      uint64_t part = 0, certs = 0;
      for (uint32_t e = o->req_grant_off[q]; e < o->req_grant_off[q + 1]; e++) {
        part += w1r_mg_entry(ent[e].key_len, ent[e].grant_len, with_sig);
        certs += w1r_cert_entry(ent[e].key_len, ent[e].cert_len);
      }
      mg_len[q] = w1r_mg_body(part, s->req_client_off ? s->req_client_len[q] : 0, sl);
      len = w1r_msg_len(mg_len[q], certs);
      if (len > kEncMaxMsg) {
        status[q] = MOCHI_ENC_TOO_LONG;
        len = 0;
      }
    }
    msg_len[q] = (uint32_t)len;
    msg_off[q] = total;
    total += len;
  }
  *wire_len = total;
  if (total > wire_cap) return bad("wire_cap is smaller than the encoded size (*wire_len)");

  // emit
  const uint8_t* sid = s->ids + s->server_id_off;
  for (uint32_t q = 0; q < Q; q++) {
    if (o->req_kind[q] == MOCHI_W1K_THROWS || status[q] != MOCHI_ENC_OK) continue;
    const uint32_t e0 = o->req_grant_off[q], e1 = o->req_grant_off[q + 1];
    const uint32_t cl = s->req_client_off ? s->req_client_len[q] : 0;
    uint8_t* p = wire + msg_off[q];
    *p++ = 0x0A;
    p = put_varint(p, mg_len[q]);
    for (uint32_t e = e0; e < e1; e++) {
      const Entry& t = ent[e];
      *p++ = 0x0A;
      p = put_varint(p, enc_e1_body(t.key_len, t.grant_len));
      p = put_ld(p, 0x0A, t.key, t.key_len);
      p = put_ld(p, 0x12, t.grant, t.grant_len);
    }
    if (cl) p = put_ld(p, 0x12, s->ids + s->req_client_off[q], cl);
    if (sl) p = put_ld(p, 0x22, sid, sl);
    if (with_sig)
      for (uint32_t e = e0; e < e1; e++) {
        const Entry& t = ent[e];
        *p++ = 0x2A;
        p = put_varint(p, enc_e5_body(t.key_len));
        p = put_ld(p, 0x0A, t.key, t.key_len);
        p = put_ld(p, 0x12, t.sig, MOCHI_RSA_BYTES);
      }
    for (uint32_t e = e0; e < e1; e++) {
      const Entry& t = ent[e];
      if (!t.cert_len) continue;
      *p++ = 0x12;
      p = put_varint(p, w1r_cert_body(t.key_len, t.cert_len));
      p = put_ld(p, 0x0A, t.key, t.key_len);
      p = put_ld(p, 0x12, t.cert, t.cert_len);
    }
    if ((uint64_t)(p - (wire + msg_off[q])) != msg_len[q]) return bad("internal: emitted size differs from computed size");
  }
  return MOCHI_OK;
}

}  // namespace mochi_host
