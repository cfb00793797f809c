// envelope_check — host-only memory check of the envelope codec's walk (csrc/envelope.h
// through its host forms, csrc/envelope_host.cpp: the code the kernels of envelope.hip run
// too).  Every truncation and every single-bit flip of three ProtocolMessage frames is
// decoded from the END of a heap buffer of exactly its size into output arrays of exactly
// one element, then routed, joined against a one-entry table and, when it is OK, wrapped
// again into a buffer of exactly the size asked for: `make envelope_check` builds it with
// the address and undefined-behaviour sanitizers and runs it, so a read past a frame or a
// write past a count stops it.  It needs no GPU.
#include "../mochi-db_amd/csrc/envelope.h"
#include "check_util.h"

// a length-delimited field by its number (the payload fields take two tag bytes)
static Bytes fld(uint32_t field, const Bytes& p) { return ld(field << 3 | 2, p); }

struct Counts {
  uint32_t status[3] = {0, 0, 0};
  uint64_t calls = 0, matched = 0, wrapped = 0;
};

static const Bytes kId = "123e4567-e89b-12d3-a456-426614174000";

// `lead` bytes, then the frame, ending the allocation: no byte after the frame is readable
static void one(const Bytes& frame, size_t lead, Counts& cnt) {
  const Wire wire(frame, lead);
  const size_t n = wire.n;
  Exact<uint64_t> f_off(1), b_off(1), s_off(1), m_off(1), r_off(1);
  Exact<uint32_t> f_len(1), b_len(1), s_len(1), m_len(1), r_len(1);
  Exact<uint8_t> st(1), kind(1);
  Exact<int64_t> ts(1);
  f_off.p[0] = lead;
  f_len.p[0] = (uint32_t)frame.size();
  const mochi_envelope_frames in{1, 0, wire.p, n, f_off.p, f_len.p};
  mochi_envelope_decoded dec{st.p, kind.p, b_off.p, b_len.p, ts.p, s_off.p, s_len.p, m_off.p, m_len.p, r_off.p, r_len.p};
  const char* err = nullptr;
  int rc = mochi_host::envelope_decode(&in, &dec, &err);
  CHECK(rc == MOCHI_OK && err == nullptr, "decode rejected: %s", err ? err : "");
  const uint8_t s = st.p[0];
  CHECK(s <= MOCHI_ENV_FALLBACK && kind.p[0] < MOCHI_ENV_KINDS, "status %u kind %u", s, kind.p[0]);
  for (auto sl : {std::make_pair(b_off.p[0], b_len.p[0]), std::make_pair(s_off.p[0], s_len.p[0]),
                  std::make_pair(m_off.p[0], m_len.p[0]), std::make_pair(r_off.p[0], r_len.p[0])})
    CHECK(sl.first >= lead && sl.first + sl.second <= n, "a slice outside the frame");
  if (s != MOCHI_ENV_OK) CHECK(kind.p[0] == 0 && ts.p[0] == 0 && !b_len.p[0] && !s_len.p[0] && !m_len.p[0] && !r_len.p[0], "undecoded");

  // route: one frame, outputs of one element
  Exact<uint32_t> kind_off(MOCHI_ENV_KINDS + 1), order(1), rb_len(1);
  Exact<uint64_t> rb_off(1);
  const mochi::env::RouteView rv{1, st.p, kind.p, b_off.p, b_len.p, {kind_off.p, order.p, rb_off.p, rb_len.p}};
  rc = mochi_host::envelope_route(&rv, &err);
  CHECK(rc == MOCHI_OK && kind_off.p[MOCHI_ENV_KINDS] == (s == MOCHI_ENV_OK ? 1u : 0u), "route");

  // join against the one id the base frames reply to
  Exact<uint8_t> ids(kId.size());
  memcpy(ids.p, kId.data(), kId.size());
  Exact<uint64_t> id_off(1), j_off(1);
  Exact<uint32_t> id_len(1), frame_req(1), rro(2), resp_frame(1), j_len(1);
  Exact<uint8_t> k1(1), k2(1);
  id_off.p[0] = 0;
  id_len.p[0] = (uint32_t)kId.size();
  const mochi::env::JoinView jv{{1, 0, ids.p, kId.size(), id_off.p, id_len.p}, in, dec,
                                {frame_req.p, rro.p, resp_frame.p, j_off.p, j_len.p, k1.p, k2.p}};
  uint32_t P = 9;
  rc = mochi_host::envelope_join(&jv, &P, &err);
  CHECK(rc == MOCHI_OK && P <= 1 && rro.p[0] == 0 && rro.p[1] == P, "join rc %d P %u", rc, P);
  CHECK((frame_req.p[0] == 0) == (P == 1), "frame_req %u", frame_req.p[0]);
  cnt.matched += P;

  // wrap what was decoded (bodies and ids: the received wire), into exactly the size asked for
  if (s == MOCHI_ENV_OK) {
    for (uint32_t flags = 0; flags <= MOCHI_ENV_LENGTH_PREFIX; flags++) {
      const mochi_envelope_source src{1, flags, wire.p, n, wire.p, n, kind.p, b_off.p, b_len.p, ts.p,
                                      m_off.p, m_len.p, r_off.p, r_len.p, s_off.p, s_len.p};
      Exact<uint64_t> o_off(1);
      Exact<uint32_t> o_len(1);
      Exact<uint8_t> o_st(1);
      uint64_t need = 0;
      rc = mochi_host::envelope_encode(&src, nullptr, 0, o_off.p, o_len.p, o_st.p, &need, &err);
      CHECK((rc == MOCHI_OK) == (need == 0), "sizing rc %d need %llu", rc, (unsigned long long)need);
      Exact<uint8_t> out(need);
      rc = mochi_host::envelope_encode(&src, out.p, need, o_off.p, o_len.p, o_st.p, &need, &err);
      CHECK(rc == MOCHI_OK && o_st.p[0] == MOCHI_ENC_OK && o_off.p[0] + o_len.p[0] == need, "encode rc %d: %s", rc, err ? err : "");
      CHECK(o_len.p[0] <= frame.size(), "the canonical form is longer than the frame");  // a writer adds nothing
      cnt.wrapped++;
    }
  }
  cnt.status[s]++;
  cnt.calls++;
}

int main() {
  const Bytes groups = Bytes("\x4b\x4b\x08\x01\x4c\x4c", 6);
  const Bytes ten = Bytes(9, '\xff') + Bytes("\x01", 1);
  std::vector<Bytes> frames = {
      // a canonical request and a canonical reply
      Bytes("\x28") + varint(1700000000000ull) + fld(6, "server-1") + fld(7, kId) + fld(107, fld(1, "client") + Bytes("\x18\x07", 2)),
      Bytes("\x28") + ten + fld(6, "s\xc3\xa9rv-\xe2\x82\xac-\xf0\x9f\x94\x91") + fld(7, "reply-id") + fld(8, kId) + fld(108, fld(1, "grant")),
      // unknown fields and groups between the known ones, fields out of order, an overlong tag, no payload
      fld(8, kId) + groups + Bytes("\xBA\x00\x02id", 5) + fld(9, "unknown") + Bytes("\x28\x05", 2) + Bytes("\x65\x01\x02\x03\x04", 5) + fld(6, "s"),
  };
  Counts cnt;
  for (const Bytes& b : frames) {
    for_mutants(b, [&](const Bytes& m, bool flip, size_t k) { one(m, flip ? k % 4 : k % 5, cnt); });
  }
  one(Bytes(8, '\xff'), 0, cnt);
  // the oneof rule, and a second payload behind a truncated one
  one(fld(107, "a") + fld(107, "b"), 1, cnt);
  one(fld(107, "a") + fld(110, "b") + fld(8, kId), 2, cnt);
  one(fld(107, "a") + fld(108, "b") + Bytes("\x3A\x05id", 4), 3, cnt);
  for (int s = 0; s < 3; s++) CHECK(cnt.status[s] > 0, "no frame reached status %d", s);
  CHECK(cnt.matched > 0 && cnt.wrapped > 0, "nothing matched or wrapped");
  printf("envelope_check: %llu frames (OK %u, MALFORMED %u, FALLBACK %u), %llu matched, %llu wrapped, %d failures\n",
         (unsigned long long)cnt.calls, cnt.status[0], cnt.status[1], cnt.status[2], (unsigned long long)cnt.matched,
         (unsigned long long)cnt.wrapped, g_failed);
  return g_failed ? 1 : 0;
}
