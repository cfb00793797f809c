// read_request_check — host-only memory check of the read request decoder's walk and of
// the read answer plan (csrc/read_request.h through its host forms,
// csrc/read_request_host.cpp: the code the kernels of read_request.hip run too).  Every
// truncation and every single-bit flip of three ReadToServer bodies (one READ op; 64 ops;
// unknown fields and groups around a nonce) is decoded from the END of a heap buffer of
// exactly its size, into output arrays of exactly the sizes the call asks for, and then
// planned against a key state of exactly n_keys entries into exactly n_ops slots: `make
// read_request_check` builds it with the address and undefined-behaviour sanitizers and
// runs it, so a read past a body or a write past a count stops it.  It needs no GPU.
#include "../mochi-db_amd/csrc/read_request.h"
#include "check_util.h"

static Bytes op(uint64_t action, const Bytes& o1, const Bytes& o2 = "", const Bytes& o3 = "") {
  return (action ? Bytes("\x08") + varint(action) : Bytes()) + (o1.empty() ? "" : ld(0x12, o1)) +
         (o2.empty() ? "" : ld(0x1A, o2)) + (o3.empty() ? "" : ld(0x22, o3));
}

struct Counts {
  uint32_t status[3] = {0, 0, 0}, plan[3] = {0, 0, 0};
  uint64_t calls = 0, ops = 0, keys = 0, slots = 0;
};

// `lead` bytes, then the body, ending the allocation: no byte after the body is readable
static void decode_one(const Bytes& body, size_t lead, Counts& cnt) {
  const Wire wire(body, lead);
  const size_t n = wire.n;
  const uint64_t msg_off[1] = {lead};
  const uint32_t msg_len[1] = {(uint32_t)body.size()};
  mochi_read_requests in;
  memset(&in, 0, sizeof in);
  in.n_reqs = 1;
  in.wire = wire.p;
  in.wire_len = n;
  in.msg_off = msg_off;
  in.msg_len = msg_len;
  uint8_t st;
  uint32_t c_len, n_len, op_off[2];
  uint64_t c_off, n_off;
  mochi_read_requests_decoded out;
  memset(&out, 0, sizeof out);
  out.req_status = &st;
  out.req_client_off = &c_off;
  out.req_client_len = &c_len;
  out.req_nonce_off = &n_off;
  out.req_nonce_len = &n_len;
  out.req_op_off = op_off;
  const char* err = nullptr;
  int rc = mochi_host::read_request_decode(&in, &out, &err);
  CHECK(err == nullptr, "input rejected: %s", err ? err : "");
  const uint32_t O = out.n_ops;
  CHECK((rc == MOCHI_OK) == (O == 0), "rc %d with %u ops at capacity 0", rc, O);
  CHECK(O <= 64 && op_off[0] == 0 && op_off[1] == O && st <= MOCHI_RDQ_FALLBACK, "count %u status %u", O, st);
  Exact<uint64_t> k_off(O);
  Exact<uint32_t> k_len(O), obj(O), key_op(O);
  Exact<uint8_t> flags(O);
  out.op_cap = O;
  out.op_key_off = k_off.p;
  out.op_key_len = k_len.p;
  out.op_flags = flags.p;
  out.op_obj = obj.p;
  out.key_op = key_op.p;
  rc = mochi_host::read_request_decode(&in, &out, &err);
  CHECK(rc == MOCHI_OK && out.n_ops == O && out.n_keys <= O, "second call rc %d", rc);
  CHECK(c_off + c_len <= n && n_off + n_len <= n, "a request slice outside the wire");
  for (uint32_t o = 0; o < O; o++) {
    CHECK(k_off.p[o] >= lead && k_off.p[o] + k_len.p[o] <= n, "key %u outside the body", o);
    CHECK(obj.p[o] == MOCHI_W1_NONE || (obj.p[o] < out.n_keys && key_op.p[obj.p[o]] <= o), "op_obj %u", o);
    CHECK((obj.p[o] != MOCHI_W1_NONE) == ((flags.p[o] & MOCHI_RDOP_READ) && k_len.p[o] != 0), "who takes part, op %u", o);
  }
  if (st != MOCHI_RDQ_OK) CHECK(O == 0 && c_len == 0 && n_len == 0, "undecoded");
  // the plan: a key state of exactly n_keys entries, every flag combination in turn
  const uint32_t U = out.n_keys;
  const uint64_t store_len = 64;
  Exact<uint8_t> kf(U);
  Exact<uint64_t> vo(U), co(U);
  Exact<uint32_t> vl(U), cl(U);
  for (uint32_t u = 0; u < U; u++) {
    kf.p[u] = (uint8_t)((u + cnt.calls) % 16 < 3 ? (u + cnt.calls) % 16 : 0x0F);  // mostly LOCAL | PRESENT | AVAILABLE | HAS_CERT
    vo.p[u] = u % 60;
    vl.p[u] = 4;
    co.p[u] = store_len - u % 8;
    cl.p[u] = u % 8;
  }
  uint8_t plan_status, resp_kind;
  uint32_t resp_n_ops;
  uint64_t slot_off;
  Exact<uint8_t> s_status(O), s_existed(O), s_flags(O);
  Exact<uint64_t> r_off(O), ce_off(O);
  Exact<uint32_t> r_len(O), ce_len(O);
  mochi::rdq::PlanView v;
  memset(&v, 0, sizeof v);
  v.n_reqs = 1;
  v.d = out;
  v.k = mochi_read_key_state{U, 0, kf.p, vo.p, vl.p, co.p, cl.p, store_len};
  v.o = mochi_read_answer_planned{&plan_status, &resp_kind, &resp_n_ops, &slot_off, s_status.p, s_existed.p, s_flags.p,
                                  r_off.p,      r_len.p,    ce_off.p,    ce_len.p};
  rc = mochi_host::read_answer_plan(&v, &err);
  CHECK(rc == MOCHI_OK, "plan rc %d: %s", rc, err ? err : "");
  CHECK(plan_status <= MOCHI_RDA_HOST && slot_off == 0, "plan status %u", plan_status);
  CHECK((plan_status == MOCHI_RDA_REPLY) == (resp_kind == MOCHI_RR_READ), "kind %u for plan %u", resp_kind, plan_status);
  CHECK(resp_n_ops == (plan_status == MOCHI_RDA_REPLY ? O : 0), "resp_n_ops %u", resp_n_ops);
  if (st == MOCHI_RDQ_MALFORMED) CHECK(plan_status == MOCHI_RDA_NO_REPLY, "a malformed request replied");
  if (st == MOCHI_RDQ_FALLBACK) CHECK(plan_status == MOCHI_RDA_HOST, "a fallback request was planned");
  for (uint32_t o = 0; o < O; o++) {
    if (plan_status != MOCHI_RDA_REPLY) {
      CHECK(s_status.p[o] == 0xFF && s_flags.p[o] == 0 && r_len.p[o] == 0 && ce_len.p[o] == 0, "slot %u of no reply", o);
    } else {
      CHECK(s_status.p[o] <= 1 && r_off.p[o] + r_len.p[o] <= store_len && ce_off.p[o] + ce_len.p[o] <= store_len, "slot %u", o);
    }
  }
  cnt.status[st]++;
  cnt.plan[plan_status]++;
  cnt.calls++;
  cnt.ops += O;
  cnt.keys += U;
  cnt.slots += resp_n_ops;
}

int main() {
  const Bytes key2 = "k\xc3\xa9y-\xe2\x82\xac-\xf0\x9f\x94\x91";
  const Bytes groups = Bytes("\x4b\x4b\x08\x01\x4c\x4c", 6);
  Bytes tx64;
  for (int i = 0; i < 64; i++) tx64 += ld(0x0A, op(0, "k" + std::to_string(i % 40)));
  std::vector<Bytes> bodies = {
      // one READ op
      ld(0x0A, "client-1") + ld(0x12, ld(0x0A, op(0, key2, "o2", "o3"))) + ld(0x1A, "nonce-1"),
      // 64 ops
      ld(0x0A, "c") + ld(0x12, tx64) + ld(0x1A, "n"),
      // unknown fields and groups around a nonce; field 3 as a varint; field 4; a ten-byte action of low word 0
      Bytes("\x18\x07", 2) + groups + ld(0x1A, "nonce-3") + groups + ld(0x22, "h") + Bytes("\x28\x01", 2) +
          ld(0x12, ld(0x0A, Bytes("\x08\x80\x80\x80\x80\xf0\xff\xff\xff\xff\x01", 11) + ld(0x12, "r")) + Bytes("\x10\x01", 2)),
  };
  Counts cnt;
  for (const Bytes& b : bodies) {
    for_mutants(b, [&](const Bytes& m, bool flip, size_t k) { decode_one(m, flip ? k % 4 : k % 5, cnt); });
  }
  decode_one(Bytes(8, '\xff'), 0, cnt);
  // the shapes validated whole: a second transaction, 65 operations (the last one cut short too)
  const Bytes tx65 = tx64 + ld(0x0A, op(0, "last"));
  decode_one(ld(0x12, ld(0x0A, op(0, "a"))) + ld(0x12, ld(0x0A, op(0, "b"))), 1, cnt);
  decode_one(ld(0x12, tx65), 2, cnt);
  decode_one(ld(0x12, tx65).substr(0, ld(0x12, tx65).size() - 1), 3, cnt);
  for (int s = 0; s < 3; s++) CHECK(cnt.status[s] > 0 && cnt.plan[s] > 0, "no body reached status %d", s);
  CHECK(cnt.ops > 0 && cnt.keys > 0 && cnt.slots > 0, "nothing decoded");
  printf("read_request_check: %llu bodies (OK %u, MALFORMED %u, FALLBACK %u; REPLY %u, NO_REPLY %u, HOST %u), %llu ops, %llu keys, "
         "%llu slots, %d failures\n",
         (unsigned long long)cnt.calls, cnt.status[0], cnt.status[1], cnt.status[2], cnt.plan[0], cnt.plan[1], cnt.plan[2],
         (unsigned long long)cnt.ops, (unsigned long long)cnt.keys, (unsigned long long)cnt.slots, g_failed);
  return g_failed ? 1 : 0;
}
