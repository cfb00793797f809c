// w1_decode_check — host-only memory check of the Write1 reply decoder's walk
// (csrc/w1_decode.h through its host form, csrc/w1_decode_host.cpp: the code the
// kernels of w1_decode.hip run too).  Every truncation and every single-bit flip of
// three reply bodies is decoded from a heap buffer of exactly its size, into output
// arrays of exactly the sizes the call asks for: `make w1_decode_check` builds it with
// the address and undefined-behaviour sanitizers and runs it, so a read past a body or
// a write past a count stops it.  A second block runs the Grant parser of
// csrc/wire_walk.h alone over a grant corpus.  It needs no GPU.
#include "../mochi-db_amd/csrc/w1_decode.h"
#include "check_util.h"

static Bytes grant(const Bytes& oid, uint64_t ts, int status = 0) {
  return ld(0x0A, oid) + "\x10" + varint(ts) + ld(0x22, Bytes(32, 'a')) + (status ? Bytes("\x28") + varint(status) : "");
}
static Bytes sig(char c) { return Bytes(256, c); }
static Bytes multigrant(const std::vector<std::pair<Bytes, Bytes>>& grants, const Bytes& server, bool sigs) {
  Bytes o;
  for (auto& g : grants) o += entry(0x0A, g.first, g.second);
  o += ld(0x12, "client-1") + ld(0x22, server);
  if (sigs)
    for (auto& g : grants) o += entry(0x2A, g.first, sig('s'));
  return o;
}
static Bytes writecert(const Bytes& key) {
  Bytes o;
  for (int s = 0; s < 3; s++) {
    const Bytes id = "server-" + std::to_string(s);
    o += entry(0x0A, id, multigrant({{key, grant(key, 100 + s)}}, id, false));
  }
  return o;
}

struct Counts {
  uint32_t status[4] = {0, 0, 0, 0};
  uint64_t calls = 0, grants = 0, certs = 0;
};

// one body from an exact-size heap buffer; ops: the request's operands
static void decode_one(const Bytes& body, uint8_t kind, Counts& cnt) {
  const Bytes ids = "server-0server-1";
  const uint32_t id_off[3] = {0, 8, 16};
  const Bytes strings = "alphabeta";
  const Wire wire(body), str(strings);  // exact: no byte after the body is readable
  const uint64_t resp_off[1] = {0}, op_key_off[2] = {0, 5};
  const uint32_t resp_len[1] = {(uint32_t)body.size()}, req_resp_off[2] = {0, 1}, req_op_off[2] = {0, 2},
                 op_key_len[2] = {5, 4};
  mochi_write1_replies in;
  memset(&in, 0, sizeof in);
  in.n_resps = 1;
  in.n_reqs = 1;
  in.n_ops = 2;
  in.wire = wire.p;
  in.wire_len = body.size();
  in.resp_off = resp_off;
  in.resp_len = resp_len;
  in.resp_kind = &kind;
  in.req_resp_off = req_resp_off;
  in.strings = str.p;
  in.strings_len = strings.size();
  in.req_op_off = req_op_off;
  in.op_key_off = op_key_off;
  in.op_key_len = op_key_len;
  uint8_t st, ko;
  uint32_t server, cl_len, goff[2], coff[2];
  uint16_t signer;
  uint64_t cl_off;
  mochi_write1_decoded out;
  memset(&out, 0, sizeof out);
  out.resp_status = &st;
  out.resp_kind_out = &ko;
  out.resp_server = &server;
  out.mg_signer = &signer;
  out.resp_client_off = &cl_off;
  out.resp_client_len = &cl_len;
  out.resp_grant_off = goff;
  out.resp_cert_off = coff;
  const char* err = nullptr;
  int rc = mochi_host::write1_reply_decode(&in, (const uint8_t*)ids.data(), id_off, 2, &out, &err);
  CHECK(err == nullptr, "input rejected: %s", err ? err : "");
  const uint32_t N = out.n_grants, C = out.n_certs;
  CHECK((rc == MOCHI_OK) == (N == 0 && C == 0), "rc %d with %u grants, %u certificates at capacity 0", rc, N, C);
  CHECK(N <= 64 && C <= 64 && goff[1] == N && coff[1] == C, "counts %u %u", N, C);
  CHECK(st <= MOCHI_W1R_UNKNOWN_SERVER, "status %u", st);
  std::vector<uint64_t> g_off(N), ck_off(C), cv_off(C);
  std::vector<uint32_t> g_len(N), ck_len(C), cv_len(C);
  std::vector<uint8_t> g_key(N), g_st(N), g_fl(N), sigs((size_t)N * 256);
  std::vector<int64_t> g_ts(N);
  out.grant_cap = N;
  out.cert_cap = C;
  out.grant_off = g_off.data();
  out.grant_len = g_len.data();
  out.grant_key = g_key.data();
  out.grant_ts = g_ts.data();
  out.grant_status = g_st.data();
  out.grant_flags = g_fl.data();
  out.sig = sigs.data();
  out.cert_key_off = ck_off.data();
  out.cert_key_len = ck_len.data();
  out.cert_val_off = cv_off.data();
  out.cert_val_len = cv_len.data();
  rc = mochi_host::write1_reply_decode(&in, (const uint8_t*)ids.data(), id_off, 2, &out, &err);
  CHECK(rc == MOCHI_OK && out.n_grants == N && out.n_certs == C, "second call rc %d", rc);
  for (uint32_t g = 0; g < N; g++)
    CHECK(g_off[g] <= body.size() && g_len[g] <= body.size() - g_off[g], "grant %u outside the body", g);
  for (uint32_t c = 0; c < C; c++)
    CHECK(ck_off[c] + ck_len[c] <= body.size() && cv_off[c] + cv_len[c] <= body.size(), "certificate %u outside", c);
  if (st == MOCHI_W1R_MALFORMED || st == MOCHI_W1R_FALLBACK) CHECK(N == 0 && C == 0 && ko == MOCHI_W1_OTHER, "undecoded");
  cnt.status[st]++;
  cnt.calls++;
  cnt.grants += N;
  cnt.certs += C;
}

// wire::parse_grant alone (the Grant parser of this decoder and of the host Write2
// encoder), over every truncation and bit flip of three grants -- the demo grant; one
// with multi-byte UTF-8, all five fields, fixed32 / fixed64 unknowns and a second
// objectId; one with unknown groups nested 1, 15, 16 and 17 deep -- and over groups
// nested 99, 100 and 101 deep: each grant ends an exact-size heap buffer.
static Bytes groups(int depth) { return Bytes(depth, '\x4b') + Bytes(depth, '\x4c'); }
static void grant_corpus() {
  const Bytes utf8 = "k\xc3\xa9y-\xe2\x82\xac-\xf0\x9f\x94\x91";
  const std::vector<Bytes> grants = {
      ld(0x0A, "DEMO_KEY_1") + "\x10" + varint(1342) + ld(0x22, Bytes(128, 'a')),
      ld(0x0A, utf8) + "\x10" + varint(1700000000000ull) + Bytes("\x18\x07", 2) + ld(0x22, "h\xc3\xa4sh" + Bytes(27, 'b')) +
          Bytes("\x28\x01", 2) + Bytes("\x4d\x01\x02\x03\x04", 5) + Bytes("\x49\x01\x02\x03\x04\x05\x06\x07\x08", 9) +
          ld(0x0A, "second"),
      ld(0x0A, "grp") + groups(1) + groups(15) + groups(16) + groups(17) + Bytes("\x10\x05", 2),
  };
  uint32_t n = 0, ok = 0;
  auto one = [&](const Bytes& m, size_t lead) {
    const Wire w(m, lead);
    mochi::wire::Grant g;
    n++;
    if (!mochi::wire::parse_grant(w.p, (uint32_t)lead, (uint32_t)m.size(), g)) return;
    ok++;
    CHECK(g.oid_len == 0 || (g.oid_off >= lead && g.oid_off + g.oid_len <= w.n), "objectId outside the grant");
  };
  for (const Bytes& b : grants) for_mutants(b, [&](const Bytes& m, bool flip, size_t k) { one(m, flip ? k % 4 : k % 5); });
  for (int d = 99; d <= 101; d++) one(ld(0x0A, "deep") + groups(d), d % 4);
  CHECK(ok > 0 && ok < n, "grants accepted: %u of %u", ok, n);
  printf("w1_decode_check: %u grants through wire::parse_grant, %u accepted\n", n, ok);
}

int main() {
  grant_corpus();
  const Bytes g1 = grant("alpha", 11), g2 = grant("beta", 12, 1);
  std::vector<Bytes> bodies = {
      ld(0x0A, multigrant({{"alpha", g1}}, "server-1", true)) + entry(0x12, "alpha", writecert("alpha")),
      // two grants, a repeated key, unknown fields and nested groups, fields 3 and 4, a repeated certificate key
      ld(0x0A, multigrant({{"alpha", g1}, {"beta", g2}, {"alpha", grant("alpha", 13)}}, "server-0", true) +
                   Bytes("\x48\x07\x5b\x08\x01\x5b\x5c\x5c", 8)) +
          entry(0x12, "beta", writecert("beta")) + ld(0x1A, "cid") + ld(0x22, "hash") + entry(0x12, "alpha", "") +
          entry(0x12, "beta", writecert("alpha")),
      // no multiGrant, a certificate entry without a value
      ld(0x12, ld(0x0A, "gamma")) + Bytes("\x08\x01", 2),
  };
  Counts cnt;
  for (const Bytes& b : bodies) {
    for_mutants(b, [&](const Bytes& m, bool flip, size_t k) {
      decode_one(m, !flip || k % 2 ? MOCHI_W1_OK : MOCHI_W1_REFUSED, cnt);
    });
  }
  decode_one(Bytes(8, '\xff'), MOCHI_W1_OK, cnt);
  decode_one(bodies[0], MOCHI_W1_REQUEST_FAILED, cnt);
  for (int s = 0; s < 4; s++) CHECK(cnt.status[s] > 0, "no body reached status %d", s);
  CHECK(cnt.grants > 0 && cnt.certs > 0, "nothing decoded");
  printf("w1_decode_check: %llu bodies (OK %u, MALFORMED %u, FALLBACK %u, UNKNOWN_SERVER %u), %llu grants, %llu "
         "certificates, %d failures\n",
         (unsigned long long)cnt.calls, cnt.status[0], cnt.status[1], cnt.status[2], cnt.status[3],
         (unsigned long long)cnt.grants, (unsigned long long)cnt.certs, g_failed);
  return g_failed ? 1 : 0;
}
