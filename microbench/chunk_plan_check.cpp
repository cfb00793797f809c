// chunk_plan_check — host-only check of the host pipeline's planning (csrc/chunk_plan.h)
// over random shapes and the edges: `make chunk_plan_check` builds it with the address
// and undefined-behaviour sanitizers and runs it; it needs no GPU.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../mochi-db_amd/csrc/chunk_plan.h"

using namespace mochi;

struct UnitRange {
  uint32_t u0, u1;
};
template <class W>
static std::vector<UnitRange> plan(uint32_t n, uint64_t target, W w) {
  std::vector<UnitRange> out;
  plan_chunks(n, target, w, [&](uint32_t u0, uint32_t u1) { out.push_back({u0, u1}); });
  return out;
}

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

// weight[i] of unit i; the two ways the callers state the weight of a step must agree
static void check_plan(const std::vector<uint32_t>& weight, uint64_t target) {
  const uint32_t n = (uint32_t)weight.size();
  std::vector<uint32_t> prefix(n + 1, 0);  // the SoA path's cert_grant_off
  for (uint32_t i = 0; i < n; i++) prefix[i + 1] = prefix[i] + weight[i];
  const auto plan = ::plan(n, target, [&](uint32_t lo, uint32_t hi) {  // the wire path's sum of msg_len
    CHECK(lo <= hi && hi <= n && hi - lo <= 32 && lo % 32 == 0, "step [%u, %u) of %u", lo, hi, n);
    uint64_t s = 0;
    for (uint32_t i = lo; i < hi; i++) s += weight[i];
    return s;
  });
  const auto by_prefix = ::plan(n, target, [&](uint32_t lo, uint32_t hi) { return prefix[hi] - prefix[lo]; });
  CHECK(plan.size() == by_prefix.size(), "n=%u target=%llu", n, (unsigned long long)target);
  auto sum = [&](uint32_t lo, uint32_t hi) { return (uint64_t)prefix[hi] - prefix[lo]; };
  CHECK(!plan.empty() && plan.front().u0 == 0 && plan.back().u1 == n, "chunks do not span [0, %u)", n);
  if (n == 0) CHECK(plan.size() == 1 && plan[0].u1 == 0, "empty batch: %zu chunks", plan.size());
  for (size_t j = 0; j < plan.size(); j++) {
    const UnitRange k = plan[j];
    const bool last = j + 1 == plan.size();
    CHECK(j >= by_prefix.size() || (by_prefix[j].u0 == k.u0 && by_prefix[j].u1 == k.u1), "chunk %zu differs by weight form", j);
    if (j) CHECK(k.u0 == plan[j - 1].u1, "chunk %zu starts at %u, the one before ends at %u", j, k.u0, plan[j - 1].u1);
    CHECK(n == 0 || k.u0 < k.u1, "chunk %zu is empty", j);
    if (!last) CHECK(k.u1 % 32 == 0, "boundary %u", k.u1);
    if (!last) CHECK(sum(k.u0, k.u1) >= target, "chunk %zu stops short of the target", j);
    const uint32_t last_group = k.u1 > k.u0 ? (k.u1 - 1) / 32 * 32 : k.u0;  // start of the chunk's last group
    if (last_group > k.u0) CHECK(sum(k.u0, last_group) < target, "chunk %zu reaches the target a group early", j);
  }
}

static void check_carve(std::mt19937_64& rng) {
  Carve256 cv;
  const int n = (int)(rng() % 40);
  size_t prev_end = 0, rounded = 0;
  for (int i = 0; i < n; i++) {
    const size_t bytes = rng() % 4 == 0 ? 0 : rng() % 3 == 0 ? 256 * (rng() % 5) : rng() % 5000;
    const size_t off = cv.take(bytes);
    CHECK(off % 256 == 0, "offset %zu", off);
    CHECK(off >= prev_end, "slice at %zu overlaps the one ending at %zu", off, prev_end);
    CHECK(off + bytes <= cv.total, "slice [%zu, %zu) past the total %zu", off, off + bytes, cv.total);
    prev_end = off + bytes;
    rounded += (bytes + 255) / 256 * 256;
  }
  CHECK(cv.total == rounded && cv.total % 256 == 0, "total %zu, slices rounded up %zu", cv.total, rounded);
}

static void check_byte_range(std::mt19937_64& rng) {
  const uint32_t n = (uint32_t)(rng() % 50);
  std::vector<uint64_t> off(n), off2(n);
  std::vector<uint32_t> len(n), len2(n);
  for (uint32_t i = 0; i < n; i++) {
    off[i] = rng() % 100000, len[i] = (uint32_t)(rng() % 3 ? rng() % 70000 : 0);
    off2[i] = rng() % 100000, len2[i] = (uint32_t)(rng() % 300);
  }
  const uint32_t i0 = n ? (uint32_t)(rng() % n) : 0, i1 = i0 + (n ? (uint32_t)(rng() % (n - i0 + 1)) : 0);
  const bool second = rng() % 2;
  ByteRange r;
  r.add(off.data(), len.data(), i0, i1);
  if (second) r.add(off2.data(), len2.data(), i0, i1);
  uint64_t lo = UINT64_MAX, hi = 0;
  for (uint32_t i = i0; i < i1; i++) {
    lo = off[i] < lo ? off[i] : lo;
    hi = off[i] + len[i] > hi ? off[i] + len[i] : hi;
    if (second) {
      lo = off2[i] < lo ? off2[i] : lo;
      hi = off2[i] + len2[i] > hi ? off2[i] + len2[i] : hi;
    }
  }
  if (i0 == i1) lo = hi = 0;
  CHECK(r.lo == lo && r.hi == hi && r.none == (i0 == i1), "[%llu, %llu) for [%llu, %llu)", (unsigned long long)r.lo,
        (unsigned long long)r.hi, (unsigned long long)lo, (unsigned long long)hi);
}

int main() {
  std::mt19937_64 rng(20240607);
  int shapes = 0;
  const uint64_t edge_targets[] = {0, 1, UINT64_MAX};
  for (uint32_t n : {0u, 1u, 31u, 32u, 33u, 64u})
    for (uint64_t target : edge_targets)
      for (uint32_t w : {0u, 1u, 1000u}) {
        check_plan(std::vector<uint32_t>(n, w), target);
        shapes++;
      }
  for (int it = 0; it < 600; it++) {
    const uint32_t n = (uint32_t)(it % 3 == 0 ? rng() % 70 : rng() % 1500);
    static const uint32_t kWeightMax[] = {1, 4, 300, 100000};
    const uint32_t wmax = kWeightMax[rng() % 4];
    std::vector<uint32_t> weight(n);
    for (auto& w : weight) w = rng() % 5 == 0 ? 0 : (uint32_t)(rng() % (wmax + 1));
    uint64_t total = 0;
    for (uint32_t w : weight) total += w;
    const uint64_t targets[] = {0, 1, rng() % (total / 8 + 2), rng() % (total + 2), total + 1, UINT64_MAX};
    check_plan(weight, targets[rng() % 6]);
    check_carve(rng);
    check_byte_range(rng);
    shapes++;
  }
  printf("chunk_plan_check: %d shapes, %d failed checks\n", shapes, g_failed);
  return g_failed ? 1 : 0;
}
