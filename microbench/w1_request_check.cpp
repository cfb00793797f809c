// w1_request_check — host-only memory check of the Write1 request decoder's walk
// (csrc/w1_request.h through its host form, csrc/w1_request_host.cpp: the code the
// kernels of w1_request.hip run too).  Every truncation and every single-bit flip of
// three Write1ToServer bodies is decoded from the END of a heap buffer of exactly its
// size, into output arrays of exactly the sizes the call asks for: `make
// w1_request_check` builds it with the address and undefined-behaviour sanitizers and
// runs it, so a read past a body or a write past a count stops it.  It needs no GPU.
#include "../mochi-db_amd/csrc/w1_request.h"
#include "check_util.h"

static Bytes op(uint64_t action, const Bytes& o1, const Bytes& o2 = "", const Bytes& o3 = "") {
  return (action ? Bytes("\x08") + varint(action) : Bytes()) + (o1.empty() ? "" : ld(0x12, o1)) +
         (o2.empty() ? "" : ld(0x1A, o2)) + (o3.empty() ? "" : ld(0x22, o3));
}

struct Counts {
  uint32_t status[3] = {0, 0, 0};
  uint64_t calls = 0, ops = 0, keys = 0;
};

// `lead` bytes, then the body, ending the allocation: no byte after the body is readable
static void decode_one(const Bytes& body, size_t lead, Counts& cnt) {
  const Wire wire(body, lead);
  const size_t n = wire.n;
  const uint64_t msg_off[1] = {lead};
  const uint32_t msg_len[1] = {(uint32_t)body.size()};
  mochi_write1_requests in;
  memset(&in, 0, sizeof in);
  in.n_reqs = 1;
  in.wire = wire.p;
  in.wire_len = n;
  in.msg_off = msg_off;
  in.msg_len = msg_len;
  uint8_t st;
  uint32_t seed, h_len, c_len, op_off[2];
  uint64_t h_off, c_off;
  mochi_write1_requests_decoded out;
  memset(&out, 0, sizeof out);
  out.req_status = &st;
  out.req_seed = &seed;
  out.req_hash_off = &h_off;
  out.req_hash_len = &h_len;
  out.req_client_off = &c_off;
  out.req_client_len = &c_len;
  out.req_op_off = op_off;
  const char* err = nullptr;
  int rc = mochi_host::write1_request_decode(&in, &out, &err);
  CHECK(err == nullptr, "input rejected: %s", err ? err : "");
  const uint32_t O = out.n_ops;
  CHECK((rc == MOCHI_OK) == (O == 0), "rc %d with %u ops at capacity 0", rc, O);
  CHECK(O <= 64 && op_off[0] == 0 && op_off[1] == O && st <= MOCHI_W1Q_FALLBACK, "count %u status %u", O, st);
  std::vector<uint64_t> k_off(O);
  std::vector<uint32_t> k_len(O), obj(O), key_op(O);
  std::vector<uint8_t> flags(O);
  out.op_cap = O;
  out.op_key_off = k_off.data();
  out.op_key_len = k_len.data();
  out.op_flags = flags.data();
  out.op_obj = obj.data();
  out.key_op = key_op.data();
  rc = mochi_host::write1_request_decode(&in, &out, &err);
  CHECK(rc == MOCHI_OK && out.n_ops == O && out.n_keys <= O, "second call rc %d", rc);
  CHECK(h_off + h_len <= n && c_off + c_len <= n, "a request slice outside the wire");
  for (uint32_t o = 0; o < O; o++) {
    CHECK(k_off[o] >= lead && k_off[o] + k_len[o] <= n, "key %u outside the body", o);
    CHECK(obj[o] == MOCHI_W1_NONE || (obj[o] < out.n_keys && key_op[obj[o]] <= o), "op_obj %u", o);
  }
  if (st != MOCHI_W1Q_OK) CHECK(O == 0 && seed == 0 && h_len == 0 && c_len == 0, "undecoded");
  cnt.status[st]++;
  cnt.calls++;
  cnt.ops += O;
  cnt.keys += out.n_keys;
}

int main() {
  const Bytes key2 = "k\xc3\xa9y-\xe2\x82\xac-\xf0\x9f\x94\x91";
  const Bytes groups = Bytes("\x4b\x4b\x08\x01\x4c\x4c", 6);
  const Bytes ten2 = Bytes("\x82", 1) + Bytes(8, '\xff') + Bytes("\x01", 1);
  std::vector<Bytes> bodies = {
      ld(0x0A, "client-1") + ld(0x12, ld(0x0A, op(2, "alpha", "value", "third")) + ld(0x0A, op(1, key2))) + "\x18" +
          varint(300) + ld(0x22, Bytes(16, 'a')),
      // unknown fields in the transaction, nested groups, a READ op, fields out of order
      ld(0x12, ld(0x0A, op(0, "r")) + ld(0x0A, op(2, "k")) + Bytes("\x10\x01", 2)) + Bytes("\x18\x07", 2) + groups +
          ld(0x0A, "c2") + ld(0x22, "h"),
      // ten-byte varints for the seed and the action, operand1 = operand2
      Bytes("\x18") + ten2 + ld(0x12, ld(0x0A, Bytes("\x08") + ten2 + ld(0x12, key2) + ld(0x1A, key2))),
  };
  Counts cnt;
  for (const Bytes& b : bodies) {
    for_mutants(b, [&](const Bytes& m, bool flip, size_t k) { decode_one(m, flip ? k % 4 : k % 5, cnt); });
  }
  decode_one(Bytes(8, '\xff'), 0, cnt);
  // the shapes validated whole: a second transaction, 65 operations (the last one cut short too)
  Bytes tx65;
  for (int i = 0; i < 65; i++) tx65 += ld(0x0A, op(2, "k" + std::to_string(i)));
  decode_one(ld(0x12, ld(0x0A, op(2, "a"))) + ld(0x12, ld(0x0A, op(1, "b"))), 1, cnt);
  decode_one(ld(0x12, tx65), 2, cnt);
  decode_one(ld(0x12, tx65).substr(0, ld(0x12, tx65).size() - 1), 3, cnt);
  for (int s = 0; s < 3; s++) CHECK(cnt.status[s] > 0, "no body reached status %d", s);
  CHECK(cnt.ops > 0 && cnt.keys > 0, "nothing decoded");
  printf("w1_request_check: %llu bodies (OK %u, MALFORMED %u, FALLBACK %u), %llu ops, %llu keys, %d failures\n",
         (unsigned long long)cnt.calls, cnt.status[0], cnt.status[1], cnt.status[2], (unsigned long long)cnt.ops,
         (unsigned long long)cnt.keys, g_failed);
  return g_failed ? 1 : 0;
}
