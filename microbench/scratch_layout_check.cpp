// scratch_layout_check — host-only check of the scratch layout functions (verify_layout in
// csrc/kernels.h, w2_count_layout / w2_emit_layout in csrc/w2.h) and of the Carve cursor
// under them (csrc/carve.h): `make scratch_layout_check` builds it with the address and
// undefined-behaviour sanitizers and runs it; it makes no HIP call and needs no GPU.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../mochi-db_amd/csrc/kernels.h"
#include "../mochi-db_amd/csrc/w2.h"

using namespace mochi;

static int g_failed = 0;
#define CHECK(cond, ...)                        \
  do {                                          \
    if (!(cond)) {                              \
      g_failed++;                               \
      fprintf(stderr, "FAIL %s: ", #cond);      \
      fprintf(stderr, __VA_ARGS__);             \
      fprintf(stderr, "\n");                    \
    }                                           \
  } while (0)

// One array a layout handed out, and the bytes its kernels may touch: the size the array
// had while it was an allocation of its own, restated here and not taken from the layout.
struct Arr {
  const char* name;
  void* p;
  size_t need;
};

// Runs `layout` (fills `arrs` from the pointers it set) on null, then on a block of exactly
// the counted bytes whose base is `off` bytes past what malloc returned.
template <class Layout>
static void check_layout(const char* what, size_t off, Layout layout) {
  std::vector<Arr> arrs;
  const size_t bytes = layout(nullptr, arrs);
  for (const Arr& a : arrs) CHECK(a.p == nullptr, "%s: %s on a null base", what, a.name);
  uint8_t* block = (uint8_t*)malloc(off + bytes);
  uint8_t *base = block + off, *end = base + bytes;
  arrs.clear();
  CHECK(layout(base, arrs) == bytes, "%s: the count depends on the base", what);
  std::stable_sort(arrs.begin(), arrs.end(), [](const Arr& x, const Arr& y) {
    return x.p != y.p ? (uintptr_t)x.p < (uintptr_t)y.p : x.need < y.need;
  });
  for (size_t i = 0; i < arrs.size(); i++) {
    const Arr& a = arrs[i];
    uint8_t* p = (uint8_t*)a.p;
    CHECK((uintptr_t)p % 256 == 0, "%s: %s at %p", what, a.name, a.p);
    CHECK(p >= base && p + a.need <= end, "%s: %s [%p, +%zu) outside the block of %zu", what, a.name, a.p, a.need, bytes);
    if (i + 1 < arrs.size())
      CHECK(p + a.need <= (uint8_t*)arrs[i + 1].p, "%s: %s (%zu bytes) runs into %s", what, a.name, a.need,
            arrs[i + 1].name);
    memset(p, 0xA5, a.need);  // past the block: the address sanitizer stops the run
  }
  free(block);
}

static const size_t kBaseOff[] = {0, 1, 16, 255};

static void check_verify(uint32_t N, uint32_t C, uint32_t K) {
  const uint64_t S = (uint64_t)N + 512 * (uint64_t)(K < N ? K : N);
  CHECK(slot_capacity(N, K) == S, "slot_capacity(%u, %u)", N, K);
  const size_t ND = (size_t)N + C;
  for (size_t off : kBaseOff)
    check_layout("verify", off, [&](void* base, std::vector<Arr>& out) {
      LaunchArgs a;
      memset(&a, 0, sizeof a);
      a.n_grants = N, a.n_certs = C, a.n_keys = K, a.n_slots = (uint32_t)S;
      const size_t bytes = verify_layout(a, base);
      CHECK(a.n_dist == N + C, "n_dist %u for %u + %u", a.n_dist, N, C);
      out = {{"digest", a.digest, 32 * ND}, {"rare", a.rare, N},           {"ts", a.ts, 8 * (size_t)N},
             {"hash_off", a.hash_off, 8 * ND}, {"hash_len", a.hash_len, 4 * ND}, {"flags", a.flags, N},
             {"lead", a.lead, 4 * (size_t)N},  {"count", a.count, 4 * (size_t)K}, {"cursor", a.cursor, 4 * (size_t)K},
             {"total", a.total, 4 * 4},        {"perm", a.perm, 4 * (size_t)S},   {"xbuf", a.xbuf, 4 * 74 * (size_t)S}};
      return bytes;
    });
}

static void check_count(uint32_t M) {
  const size_t m1 = (size_t)M + 1;
  for (size_t off : kBaseOff)
    check_layout("w2 count", off, [&](void* base, std::vector<Arr>& out) {
      W2Args a;
      memset(&a, 0, sizeof a);
      a.M = M;
      const size_t bytes = w2_count_layout(a, base);
      CHECK(a.ce_cap == 32 * m1, "ce_cap %u for %zu messages", a.ce_cap, m1);
      // cnt_ce: the seven arrays msg_view reads at stride m1, one run; ce: ce_view's kW2CeArrays arrays of ce_cap
      out = {{"cnt_g", a.cnt_g, 4 * m1},
             {"cnt_o", a.cnt_o, 4 * m1},
             {"cnt_m", a.cnt_m, 4 * m1},
             {"cert_grant_off", a.cert_grant_off, 4 * m1},
             {"cert_op_off", a.cert_op_off, 4 * m1},
             {"cert_mg_off", a.cert_mg_off, 4 * m1},
             {"cnt_ce", a.cnt_ce, 4 * 7 * m1},
             {"ce", a.ce, 4 * (size_t)kW2CeArrays * a.ce_cap},
             {"inl", a.inl, 4 * 4 * 4 * m1},
             {"inl_ops", a.inl_ops, 4 * 2 * 4 * m1},
             {"cnt4", a.cnt4, 16 * m1},
             {"off4", a.off4, 16 * m1}};
      if (base)
        CHECK((uintptr_t)a.inl % 16 == 0 && (uintptr_t)a.cnt4 % 16 == 0 && (uintptr_t)a.off4 % 16 == 0,
              "inl / cnt4 / off4 of %u messages are read as uint4", M);
      return bytes;
    });
}

static void check_emit(uint32_t N, uint32_t O, uint32_t NM) {
  for (size_t off : kBaseOff)
    check_layout("w2 emit", off, [&](void* base, std::vector<Arr>& out) {
      W2Args a;
      memset(&a, 0, sizeof a);
      a.N = N;
      const size_t bytes = w2_emit_layout(a, O, NM, base);
      const size_t n = N, o = O;
      out = {{"grant_off", a.grant_off, 8 * n},
             {"grant_len", a.grant_len, 4 * n},
             {"sig", a.sig, 256 * n},
             {"signer", a.signer, 2 * n},
             {"grant_key", a.grant_key, n},
             {"op_key", a.op_key, o},
             {"op_flags", a.op_flags, o},
             {"sig_src", a.sig_src, 8 * n},
             {"mg_grant_off", a.mg_grant_off, 4 * ((size_t)NM + 1)},
             {"op_object_ts", a.op_object_ts, 8 * o},
             {"op_key_off", a.op_key_off, 8 * o},
             {"op_key_len", a.op_key_len, 4 * o},
             {"grant_same", a.grant_same, 4 * n}};
      return bytes;
    });
}

// The wire encoders' layout functions sit beside their kernels (w2_encode.hip, w1_issue.hip,
// w1_reply.hip), in files of kernels that a host compiler cannot build, so their byte counts at
// the parent cannot be recorded here.  They use Carve with its default alignment, so what is
// checked instead is that cursor: for a take sequence, the offsets and the count of
// the rule the encoders were laid out by -- the base rounded up to 16, every array rounded
// up to 16 bytes, 16 bytes of slack in the count.
static void check_carve16(const std::vector<std::pair<size_t, size_t>>& takes /* element size, count */) {
  alignas(16) static uint8_t buf[64];
  for (size_t off : {0, 1, 8, 15}) {
    uint8_t* base = buf + off;
    Carve counted(nullptr), placed(base);
    size_t used = 0;
    const uintptr_t start = ((uintptr_t)base + 15) / 16 * 16;
    for (auto [size, count] : takes) {
      void *n = nullptr, *p = nullptr;
      switch (size) {
        case 1: n = counted.take<uint8_t>(count), p = placed.take<uint8_t>(count); break;
        case 2: n = counted.take<uint16_t>(count), p = placed.take<uint16_t>(count); break;
        case 4: n = counted.take<uint32_t>(count), p = placed.take<uint32_t>(count); break;
        default: n = counted.take<uint64_t>(count), p = placed.take<uint64_t>(count); break;
      }
      CHECK(n == nullptr, "take on a null base");
      CHECK((uintptr_t)p == start + used, "take of %zu x %zu at +%zu, not +%zu", count, size, (size_t)((uintptr_t)p - start), used);
      used += (size * count + 15) / 16 * 16;
      CHECK(counted.bytes() == used + 16 && placed.bytes() == used + 16, "count %zu after %zu bytes", counted.bytes(), used);
    }
  }
}

int main() {
  int shapes = 0;
  const uint32_t kM[] = {0, 1, 2, 31, 32, 33, 1023, 1024, 1025};
  const uint32_t kN[] = {0, 1, 15, 16, 17, 511, 512, 4096, 4097};
  for (uint32_t N : kN)
    for (uint32_t C : {0u, 1u, N})
      for (uint32_t K : {1u, 4u, 7u, N + 1}) check_verify(N, C, K), shapes++;
  for (uint32_t M : kM) check_count(M), shapes++;
  for (uint32_t N : kN)
    for (uint32_t M : kM)
      for (uint32_t O : {0u, 1u, 3 * M})
        for (uint32_t NM : {0u, 1u, 3 * M}) check_emit(N, O, NM), shapes++;
  for (size_t n : {0, 1, 2, 3, 15, 16, 17, 255, 1000, 4097})
    for (int form = 0; form < 3; form++) {
      const size_t m = form == 0 ? n : form == 1 ? 3 * n + 1 : n / 2;  // three sequences a size, as three encoders
      shapes++;
      check_carve16({{4, n}, {8, n + 1}, {1, m}, {2, n}, {8, m}, {4, 4}, {1, 0}, {4, 2 * m + 1}, {2, 7 * n}});
    }
  printf("scratch_layout_check: %d shapes, %d failed checks\n", shapes, g_failed);
  return g_failed ? 1 : 0;
}
