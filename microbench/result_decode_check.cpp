// result_decode_check — host-only memory check of the result reply decoder's walk
// (csrc/result_decode.h through its host form, csrc/result_decode_host.cpp: the code
// the kernels of result_decode.hip run too).  Every truncation and every single-bit
// flip of three answer bodies is decoded from the END of a heap buffer of exactly its
// size, into slot arrays of exactly n_ops entries: `make result_decode_check` builds
// it with the address and undefined-behaviour sanitizers and runs it, so a read past a
// body or a write past a slot run stops it.  It needs no GPU.
#include "../mochi-db_amd/csrc/result_decode.h"
#include "check_util.h"

static Bytes grant(const Bytes& oid, uint64_t ts) {
  return ld(0x0A, oid) + "\x10" + varint(ts) + ld(0x22, Bytes(16, 'a')) + Bytes("\x28\x01", 2);
}
// a WriteCertificate of `n` servers over one key, each MultiGrant with a 16-byte signature
static Bytes cert(int n) {
  Bytes o;
  for (int s = 0; s < n; s++) {
    const Bytes sid = "server-" + std::to_string(s);
    o += entry(0x0A, sid, entry(0x0A, "k\xc3\xa9y", grant("k\xc3\xa9y", 100 + s)) + ld(0x12, "client") + ld(0x22, sid) +
                              entry(0x2A, "k\xc3\xa9y", Bytes(16, '\x7f')));
  }
  return o;
}
static Bytes op(uint64_t status, const Bytes& result, bool existed, const Bytes* c) {
  return (result.empty() ? "" : ld(0x0A, result)) + (c ? ld(0x12, *c) : "") + (existed ? Bytes("\x18\x01", 2) : "") +
         (status ? Bytes("\x20") + varint(status) : "");
}

struct Counts {
  uint32_t status[3] = {0, 0, 0};
  uint64_t calls = 0, slots = 0, certs = 0;
};

// `lead` bytes, then the body, ending the allocation: no byte after the body is readable
static void decode_one(const Bytes& body, uint8_t kind, uint32_t n_ops, size_t lead, Counts& cnt) {
  const Wire wire(body, lead);
  const size_t n = wire.n;
  const uint64_t resp_off[1] = {lead}, slot_off[1] = {0};
  const uint32_t resp_len[1] = {(uint32_t)body.size()}, req_resp_off[2] = {0, 1}, k[1] = {n_ops};
  mochi_result_replies in;
  memset(&in, 0, sizeof in);
  in.n_resps = in.n_reqs = 1;
  in.wire = wire.p;
  in.wire_len = n;
  in.resp_off = resp_off;
  in.resp_len = resp_len;
  in.resp_kind = &kind;
  in.req_resp_off = req_resp_off;
  in.n_ops = k;
  in.slot_off = slot_off;
  uint8_t st;
  uint32_t cnt_ops, rid_len, nonce_len;
  uint64_t rid_off, nonce_off;
  // exactly n_ops entries each, on the heap
  std::vector<uint8_t> o_st(n_ops, 0xA5), o_ex(n_ops, 0xA5), o_fl(n_ops, 0xA5);
  std::vector<uint64_t> r_off(n_ops), c_off(n_ops);
  std::vector<uint32_t> r_len(n_ops), c_len(n_ops);
  mochi_result_decoded out;
  out.resp_status = &st;
  out.resp_n_ops = &cnt_ops;
  out.resp_rid_off = &rid_off;
  out.resp_rid_len = &rid_len;
  out.resp_nonce_off = &nonce_off;
  out.resp_nonce_len = &nonce_len;
  out.op_status = o_st.data();
  out.op_existed = o_ex.data();
  out.op_flags = o_fl.data();
  out.op_result_off = r_off.data();
  out.op_result_len = r_len.data();
  out.op_cert_off = c_off.data();
  out.op_cert_len = c_len.data();
  const char* err = nullptr;
  const int rc = mochi_host::result_reply_decode(&in, &out, &err);
  CHECK(rc == MOCHI_OK && err == nullptr, "input rejected: %s", err ? err : "");
  CHECK(st <= MOCHI_RRS_FALLBACK, "status %u", st);
  CHECK((st == MOCHI_RRS_OK) == (cnt_ops != 0xFFFFFFFFu), "status %u with count %u", st, cnt_ops);
  CHECK(rid_off + rid_len <= n && nonce_off + nonce_len <= n, "a response slice outside the wire");
  const bool values = st == MOCHI_RRS_OK && cnt_ops <= 64;
  for (uint32_t j = 0; j < n_ops; j++) {
    if (values && j < cnt_ops) {
      CHECK(r_off[j] >= lead && r_off[j] + r_len[j] <= n && c_off[j] >= lead && c_off[j] + c_len[j] <= n,
            "slot %u outside the body", j);
      CHECK(o_ex[j] <= 1 && o_fl[j] <= MOCHI_RRO_HAS_CERT, "slot %u flags", j);
      cnt.certs += o_fl[j];
    } else {
      CHECK(o_st[j] == 0xFF && !o_ex[j] && !o_fl[j] && !r_off[j] && !r_len[j] && !c_off[j] && !c_len[j],
            "slot %u of an absent operation holds a value", j);
    }
  }
  cnt.status[st]++;
  cnt.calls++;
  cnt.slots += n_ops;
}

int main() {
  const Bytes c3 = cert(3), c1 = cert(1);
  const Bytes groups = Bytes("\x4b\x4b\x08\x01\x4c\x4c", 6);
  const Bytes ws = Bytes("\x20\x01", 2);
  struct B {
    uint8_t kind;
    uint32_t n_ops;
    Bytes body;
  };
  const std::vector<B> bodies = {
      // a Write2 answer with a certificate, and a WRONG_SHARD operation
      {MOCHI_RR_WRITE2_ANS, 2, ld(0x0A, ld(0x0A, op(0, "value", true, &c3)) + ld(0x0A, ws)) + ld(0x12, "rid-1")},
      // a read answer with nonce and rid, unknown fields and nested groups
      {MOCHI_RR_READ, 2,
       ld(0x0A, ld(0x0A, op(0, "r\xc3\xa9" "ad", true, &c1)) + Bytes("\x10\x01", 2) + ld(0x0A, op(0, "", false, &c1))) +
           ld(0x12, "nonce-2") + groups + ld(0x1A, "rid-2")},
      // one operation more than n_ops
      {MOCHI_RR_WRITE2_ANS, 1, ld(0x0A, ld(0x0A, ws) + ld(0x0A, op(2, "extra", false, &c1))) + ld(0x12, "r")},
  };
  Counts cnt;
  for (const B& b : bodies) {
    for_mutants(b.body, [&](const Bytes& m, bool flip, size_t k) { decode_one(m, b.kind, b.n_ops, flip ? k % 4 : k % 5, cnt); });
  }
  decode_one(Bytes(8, '\xff'), MOCHI_RR_READ, 0, 0, cnt);
  decode_one(Bytes(8, '\xff'), MOCHI_RR_OTHER, 3, 1, cnt);
  // the shapes validated whole: a second result, 65 operations (the last one cut short too), and the
  // merge of two certificates in one operation
  Bytes tx65;
  for (int i = 0; i < 65; i++) tx65 += ld(0x0A, op(0, "r" + std::to_string(i), true, i == 64 ? &c1 : nullptr));
  decode_one(ld(0x0A, ld(0x0A, ws)) + ld(0x0A, ld(0x0A, ws)), MOCHI_RR_WRITE2_ANS, 1, 1, cnt);
  decode_one(ld(0x0A, tx65), MOCHI_RR_WRITE2_ANS, 64, 2, cnt);
  decode_one(ld(0x0A, tx65).substr(0, ld(0x0A, tx65).size() - 1), MOCHI_RR_WRITE2_ANS, 64, 3, cnt);
  decode_one(ld(0x0A, ld(0x0A, ld(0x12, c1) + ld(0x12, c1))), MOCHI_RR_READ, 1, 0, cnt);
  for (int s = 0; s < 3; s++) CHECK(cnt.status[s] > 0, "no body reached status %d", s);
  CHECK(cnt.slots > 0 && cnt.certs > 0, "nothing decoded");
  printf("result_decode_check: %llu bodies (OK %u, MALFORMED %u, FALLBACK %u), %llu slots, %llu certificates, %d failures\n",
         (unsigned long long)cnt.calls, cnt.status[0], cnt.status[1], cnt.status[2], (unsigned long long)cnt.slots,
         (unsigned long long)cnt.certs, g_failed);
  return g_failed ? 1 : 0;
}
