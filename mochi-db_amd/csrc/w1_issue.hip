// w1_issue.hip — Write1 grant issuance on the device (gfx950): which grants
// this server gives to a batch of Write1ToServer requests, and their Grant
// bytes (semantics: include/mochi_hip.h mochi_write1_batch; layout:
// w1_issue.h).  The reference decides one request at a time under locks
// (InMemoryDataStore.java:105-155, :233-310); here contention for a free
// (object, timestamp) slot inside the batch is resolved by the smallest op
// index, which is what the sequential order gives.
//   k_w1_pre     lane = request  owning request of each op; ops behind an empty key
//   k_w1_claim   lane = op       free-slot ops put (object, seed) into an open-addressing
//                                table in HBM: a 64-bit compare-and-swap takes the key
//                                word, a 32-bit atomicMin keeps the smallest op index
//   k_w1_decide  lane = op       (a launch of its own: every claim must have landed)
//                                winner lookup, hash compares, decision, NEW flag and size
//   k_w1_reply   lane = request  kind; distinct grant references of the reply (count, then write)
//   64-bit exclusive scans of new-grant counts, grant bytes and reply sizes
//                                (hipcub; one block below w2_small's line)
//   k_w1_emit    16 lanes per op Grant headers (lane 0), key and hash payloads (all lanes)
// Header bytes and payload bytes go out as in the Write2 encoder (enc_dev.h):
// whole dwords / 16-byte chunks where every byte is the lane's own, byte and
// short stores at the ends.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "enc_dev.h"
#include "enc_launch.h"
#include "prep_dev.h"
#include "w1_issue.h"
#include "w2.h"

namespace mochi {
namespace {

constexpr uint64_t kEmpty = ~0ull;
constexpr uint8_t kWD = MOCHI_W1OP_WRITE | MOCHI_W1OP_DELETE;
constexpr uint8_t kHeld = MOCHI_W1OP_LOCAL | MOCHI_W1OP_HAS_SVOC;

// splitmix64's finalizer: sequential, strided and all-equal-but-seed keys all spread
__device__ __forceinline__ uint32_t slot_of(uint64_t key, uint32_t mask) {
  key = (key ^ (key >> 30)) * 0xBF58476D1CE4E5B9ull;
  key = (key ^ (key >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)(key ^ (key >> 31)) & mask;
}

__device__ __forceinline__ bool slices_equal(const uint8_t* __restrict__ s, uint64_t ao, uint32_t al, uint64_t bo,
                                             uint32_t bl) {
  return al == bl && (ao == bo || bytes_equal(s + ao, s + bo, al));
}

// does this op reach a free slot (and so take part in the claim)?
__device__ __forceinline__ bool claims(const mochi_write1_batch& b, uint32_t o, const uint8_t* __restrict__ op_dead) {
  const uint8_t f = b.op_flags[o];
  return (f & kWD) && !op_dead[o] && b.op_key_len[o] != 0 && (f & kHeld) == kHeld && b.op_stored[o] == MOCHI_W1_NONE;
}

// ---- lane = request: owning request, ops behind an empty key -----------------
__global__ __launch_bounds__(256) void k_w1_pre(mochi_write1_batch b, uint32_t* __restrict__ op_req,
                                                uint8_t* __restrict__ op_dead) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= b.n_reqs) return;
  bool dead = false;
  const uint32_t o1 = b.req_op_off[q + 1];
#pragma unroll 1
  for (uint32_t o = b.req_op_off[q]; o < o1; o++) {
    op_req[o] = q;
    op_dead[o] = dead;
    if ((b.op_flags[o] & kWD) && b.op_key_len[o] == 0) dead = true;
  }
}

// ---- lane = op: claim the free slots ------------------------------------------
__global__ __launch_bounds__(256) void k_w1_claim(mochi_write1_batch b, const uint32_t* __restrict__ op_req,
                                                  const uint8_t* __restrict__ op_dead,
                                                  unsigned long long* __restrict__ tbl_key,
                                                  uint32_t* __restrict__ tbl_val, uint32_t mask) {
  const uint32_t o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= b.n_ops || !claims(b, o, op_dead)) return;
  const uint64_t key = (uint64_t)b.op_obj[o] << 32 | b.req_seed[op_req[o]];
  uint32_t h = slot_of(key, mask);
  // at most n_ops keys in >= 2 * n_ops slots: a free or equal slot is met within `mask` steps
#pragma unroll 1
  for (uint32_t n = 0; n <= mask; n++, h = (h + 1) & mask) {
    const uint64_t prev = atomicCAS(&tbl_key[h], (unsigned long long)kEmpty, (unsigned long long)key);
    if (prev == kEmpty || prev == key) {
      atomicMin(&tbl_val[h], o);
      return;
    }
  }
}

// ---- lane = op: decisions -------------------------------------------------------
__global__ __launch_bounds__(256) void k_w1_decide(mochi_write1_batch b, const uint32_t* __restrict__ op_req,
                                                   const uint8_t* __restrict__ op_dead,
                                                   const uint64_t* __restrict__ tbl_key,
                                                   const uint32_t* __restrict__ tbl_val, uint32_t mask,
                                                   uint8_t* __restrict__ op_decision, uint32_t* __restrict__ op_ref,
                                                   uint64_t* __restrict__ cnt64, uint64_t* __restrict__ len64) {
  const uint32_t o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o > b.n_ops) return;
  if (o == b.n_ops) {  // the scans' last element
    cnt64[o] = 0;
    len64[o] = 0;
    return;
  }
  const uint8_t f = b.op_flags[o];
  const uint32_t kl = b.op_key_len[o];
  uint8_t d;
  uint32_t ref = MOCHI_W1_NONE;
  bool makes = false;
  uint64_t size = 0;
  if (!(f & kWD)) {
    d = MOCHI_W1D_SKIP;
  } else if (op_dead[o]) {
    d = MOCHI_W1D_SKIPPED;
  } else if (kl == 0) {
    d = MOCHI_W1D_FAILED;
  } else {
    const uint32_t q = op_req[o];
    const uint64_t ho = b.req_hash_off[q];
    const uint32_t hl = b.req_hash_len[q];
    if (!(f & MOCHI_W1OP_LOCAL)) {
      d = MOCHI_W1D_WRONG_SHARD;
      ref = o;
      // an earlier non-local op of the request on a byte-equal key already made the grant
      // (no earlier op is the empty-key one: this op would be SKIPPED)
      const uint64_t ko = b.op_key_off[o];
#pragma unroll 1
      for (uint32_t e = b.req_op_off[q]; e < o; e++) {
        const uint8_t fe = b.op_flags[e];
        if ((fe & kWD) && !(fe & MOCHI_W1OP_LOCAL) && slices_equal(b.strings, b.op_key_off[e], b.op_key_len[e], ko, kl)) {
          ref = e;
          break;
        }
      }
      makes = ref == o;
      size = w1_grant_size(kl, hl, 0, true);
    } else if (!(f & MOCHI_W1OP_HAS_SVOC)) {
      d = MOCHI_W1D_FAILED;
    } else if (b.op_stored[o] != MOCHI_W1_NONE) {
      const uint32_t s = b.op_stored[o];
      d = slices_equal(b.strings, ho, hl, b.stored_hash_off[s], b.stored_hash_len[s]) ? MOCHI_W1D_RETRY
                                                                                        : MOCHI_W1D_REFUSED;
      ref = MOCHI_W1_STORED | s;
    } else {
      const uint32_t seed = b.req_seed[q];
      const uint64_t key = (uint64_t)b.op_obj[o] << 32 | seed;
      uint32_t h = slot_of(key, mask), w = o;
      // this op claimed the key, so the probe meets it before an empty slot
#pragma unroll 1
      for (uint32_t n = 0; n <= mask; n++, h = (h + 1) & mask) {
        const uint64_t k = tbl_key[h];
        if (k == key) {
          w = tbl_val[h];
          break;
        }
        if (k == kEmpty) break;
      }
      ref = w;
      if (w == o) {
        d = MOCHI_W1D_NEW;
        makes = true;
        size = w1_grant_size(kl, hl, w1_ts(b.op_epoch[o], seed), false);
      } else {
        const uint32_t qw = op_req[w];
        d = qw == q || slices_equal(b.strings, ho, hl, b.req_hash_off[qw], b.req_hash_len[qw]) ? MOCHI_W1D_RETRY
                                                                                                 : MOCHI_W1D_REFUSED;
      }
    }
  }
  op_decision[o] = d;
  op_ref[o] = ref;
  cnt64[o] = makes ? 1 : 0;
  len64[o] = makes ? size : 0;
}

// ---- lane = request: kind and the reply's distinct grant references ------------
__device__ __forceinline__ bool listed(uint8_t kind, uint8_t d) {
  return kind == MOCHI_W1K_OK ? d == MOCHI_W1D_NEW || d == MOCHI_W1D_RETRY || d == MOCHI_W1D_WRONG_SHARD
                              : kind == MOCHI_W1K_REFUSED && d == MOCHI_W1D_REFUSED;
}

// kWrite = false: req_kind and the number of references (ref64, the scan's input);
// kWrite = true: req_grant from the scanned offsets and the new-grant numbering
template <bool kWrite>
__global__ __launch_bounds__(256) void k_w1_reply(mochi_write1_batch b, const uint8_t* __restrict__ op_decision,
                                                  const uint32_t* __restrict__ op_ref, uint8_t* __restrict__ req_kind,
                                                  uint64_t* __restrict__ ref64, const uint64_t* __restrict__ ref_off,
                                                  const uint64_t* __restrict__ cnt_off,
                                                  uint32_t* __restrict__ req_grant) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q > b.n_reqs) return;
  if (q == b.n_reqs) {
    if (!kWrite) ref64[q] = 0;
    return;
  }
  const uint32_t o0 = b.req_op_off[q], o1 = b.req_op_off[q + 1];
  uint8_t kind;
  if (kWrite) {
    kind = req_kind[q];
  } else {
    bool failed = false, refused = false;
#pragma unroll 1
    for (uint32_t o = o0; o < o1; o++) {
      const uint8_t d = op_decision[o];
      failed |= d == MOCHI_W1D_FAILED;
      refused |= d == MOCHI_W1D_REFUSED;
    }
    kind = failed ? MOCHI_W1K_THROWS : refused ? MOCHI_W1K_REFUSED : MOCHI_W1K_OK;
    req_kind[q] = kind;
  }
  uint64_t n = 0;
  const uint64_t at = kWrite ? ref_off[q] : 0;
  if (kind != MOCHI_W1K_THROWS) {
#pragma unroll 1
    for (uint32_t o = o0; o < o1; o++) {
      if (!listed(kind, op_decision[o])) continue;
      const uint32_t r = op_ref[o];
      bool first = true;
#pragma unroll 1
      for (uint32_t e = o0; e < o && first; e++) first = !(op_ref[e] == r && listed(kind, op_decision[e]));
      if (!first) continue;
      if (kWrite) req_grant[at + n] = r & MOCHI_W1_STORED ? r : (uint32_t)cnt_off[r];
      n++;
    }
  }
  if (!kWrite) ref64[q] = n;
}

// ---- the scans -------------------------------------------------------------------
// one block of 1024 lanes: O < 1024 and Q < 1024
__global__ __launch_bounds__(1024) void k_w1_scan_small(uint32_t O, uint32_t Q, const uint64_t* __restrict__ cnt64,
                                                        const uint64_t* __restrict__ len64,
                                                        const uint64_t* __restrict__ ref64,
                                                        uint64_t* __restrict__ cnt_off, uint64_t* __restrict__ len_off,
                                                        uint64_t* __restrict__ ref_off) {
  using Scan = hipcub::BlockScan<uint64_t, 1024>;
  __shared__ typename Scan::TempStorage tmp;
  const uint32_t t = threadIdx.x;
  uint64_t off;
  Scan(tmp).ExclusiveSum(t <= O ? cnt64[t] : 0, off);
  if (t <= O) cnt_off[t] = off;
  __syncthreads();
  Scan(tmp).ExclusiveSum(t <= O ? len64[t] : 0, off);
  if (t <= O) len_off[t] = off;
  __syncthreads();
  Scan(tmp).ExclusiveSum(t <= Q ? ref64[t] : 0, off);
  if (t <= Q) ref_off[t] = off;
}

// req_grant_off from the scanned reply sizes; the two totals the host waits for
__global__ __launch_bounds__(256) void k_w1_totals(uint32_t O, uint32_t Q, const uint64_t* __restrict__ cnt_off,
                                                   const uint64_t* __restrict__ len_off,
                                                   const uint64_t* __restrict__ ref_off,
                                                   uint32_t* __restrict__ req_grant_off, uint64_t* __restrict__ totals) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q <= Q) req_grant_off[q] = (uint32_t)ref_off[q];
  if (q == 0) {
    totals[0] = cnt_off[O];
    totals[1] = len_off[O];
  }
}

// ---- 16 lanes per op: the new grants ---------------------------------------------
__global__ __launch_bounds__(256) void k_w1_emit(mochi_write1_batch b, mochi_write1_issued out,
                                                 const uint32_t* __restrict__ op_req,
                                                 const uint32_t* __restrict__ op_ref,
                                                 const uint64_t* __restrict__ cnt64,
                                                 const uint64_t* __restrict__ cnt_off,
                                                 const uint64_t* __restrict__ len_off) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t o64 = t >> 4;
  const uint32_t l = (uint32_t)(t & 15);
  if (o64 >= b.n_ops) return;
  const uint32_t o = (uint32_t)o64;
  if (l == 0) {
    const uint32_t r = op_ref[o];
    out.op_grant[o] = r == MOCHI_W1_NONE || (r & MOCHI_W1_STORED) ? r : (uint32_t)cnt_off[r];
  }
  if (!cnt64[o]) return;
  const uint32_t q = op_req[o];
  const bool ws = out.op_decision[o] == MOCHI_W1D_WRONG_SHARD;
  const int64_t ts = ws ? 0 : w1_ts(b.op_epoch[o], b.req_seed[q]);
  const uint32_t kl = b.op_key_len[o], hl = b.req_hash_len[q];
  const uint64_t pos = len_off[o];
  uint8_t* const dst = out.grant_bytes + pos;
  const uint32_t ts_bytes = ts ? 1 + wire::varint_size((uint64_t)ts) : 0;
  const uintptr_t d_key = (uintptr_t)dst + 1 + wire::varint_size(kl);
  const uintptr_t d_hash = d_key + kl + ts_bytes + 1 + wire::varint_size(hl);  // meaningful when hl != 0
  if (l == 0) {
    Put p(dst);
    p.byte(0x0A);
    p.varint(kl);
    p.skip(kl);
    if (ts) {
      p.byte(0x10);
      p.varint((uint64_t)ts);
    }
    if (hl) {
      p.byte(0x22);
      p.varint(hl);
      p.skip(hl);
    }
    if (ws) {
      p.byte(0x28);
      p.byte(kW1WrongShard);
    }
    p.flush();
    const uint64_t g = cnt_off[o];
    out.grant_off[g] = pos;
    out.grant_len[g] = (uint32_t)(p.p - dst);
    out.grant_op[g] = o;
    out.grant_ts[g] = ts;
  }
  const uint32_t c = copy_run(l, d_key, b.strings + b.op_key_off[o], kl);
  if (!hl) return;
  copy_run(c, d_hash, b.strings + b.req_hash_off[q], hl);
}

inline bool w1_small(uint32_t Q, uint32_t O) { return w2_small(O) && w2_small(Q); }

}  // namespace

size_t w1_layout(W1Args& a, void* base) {
  const size_t o1 = (size_t)a.b.n_ops + 1, q1 = (size_t)a.b.n_reqs + 1;
  Carve c(base);
  a.tbl_key = c.take<uint64_t>(a.slots);  // tbl_key and tbl_val adjacent: one fill (launch_w1_decide)
  a.tbl_val = c.take<uint32_t>(a.slots);
  a.op_req = c.take<uint32_t>(o1);
  a.op_ref = c.take<uint32_t>(o1);
  a.op_dead = c.take<uint8_t>(o1);
  a.cnt64 = c.take<uint64_t>(o1);
  a.len64 = c.take<uint64_t>(o1);
  a.cnt_off = c.take<uint64_t>(o1);
  a.len_off = c.take<uint64_t>(o1);
  a.ref64 = c.take<uint64_t>(q1);
  a.ref_off = c.take<uint64_t>(q1);
  a.totals = c.take<uint64_t>(2);
  return c.bytes();
}

hipError_t launch_w1_decide(const W1Args& a, hipStream_t st) {
  const mochi_write1_batch& b = a.b;
  const uint32_t O = b.n_ops, Q = b.n_reqs, mask = a.slots - 1;
  const Stamps stamp{a.ev, st};
  hipError_t e = stamp(0);
  if (e != hipSuccess) return e;
  // every key word empty, every value word "no op"
  const size_t fill = (size_t)((uint8_t*)(a.tbl_val + a.slots) - (uint8_t*)a.tbl_key);
  if ((e = hipMemsetAsync(a.tbl_key, 0xFF, fill, st)) != hipSuccess) return e;
  if (Q) hipLaunchKernelGGL(k_w1_pre, dim3(cdiv(Q, 256)), dim3(256), 0, st, b, a.op_req, a.op_dead);
  if ((e = stamp(1)) != hipSuccess) return e;
  if (O)
    hipLaunchKernelGGL(k_w1_claim, dim3(cdiv(O, 256)), dim3(256), 0, st, b, a.op_req, a.op_dead,
                       (unsigned long long*)a.tbl_key, a.tbl_val, mask);
  if ((e = stamp(2)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_w1_decide, dim3(cdiv((uint64_t)O + 1, 256)), dim3(256), 0, st, b, a.op_req, a.op_dead, a.tbl_key,
                     a.tbl_val, mask, a.o.op_decision, a.op_ref, a.cnt64, a.len64);
  if ((e = stamp(3)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_w1_reply<false>, dim3(cdiv((uint64_t)Q + 1, 256)), dim3(256), 0, st, b, a.o.op_decision, a.op_ref,
                     a.o.req_kind, a.ref64, a.ref_off, a.cnt_off, a.o.req_grant);
  if ((e = hipGetLastError()) != hipSuccess || (e = stamp(4)) != hipSuccess) return e;
  if (w1_small(Q, O)) {
    hipLaunchKernelGGL(k_w1_scan_small, dim3(1), dim3(1024), 0, st, O, Q, a.cnt64, a.len64, a.ref64, a.cnt_off, a.len_off,
                       a.ref_off);
  } else {
    if ((e = enc_scan64(a.scan_temp, a.scan_temp_bytes, a.cnt64, a.cnt_off, O + 1, st)) != hipSuccess ||
        (e = enc_scan64(a.scan_temp, a.scan_temp_bytes, a.len64, a.len_off, O + 1, st)) != hipSuccess ||
        (e = enc_scan64(a.scan_temp, a.scan_temp_bytes, a.ref64, a.ref_off, Q + 1, st)) != hipSuccess)
      return e;
  }
  hipLaunchKernelGGL(k_w1_totals, dim3(cdiv((uint64_t)Q + 1, 256)), dim3(256), 0, st, O, Q, a.cnt_off, a.len_off, a.ref_off,
                     a.o.req_grant_off, a.totals);
  e = hipGetLastError();
  return e != hipSuccess ? e : stamp(5);
}

hipError_t launch_w1_emit(const W1Args& a, hipStream_t st) {
  const mochi_write1_batch& b = a.b;
  const uint32_t O = b.n_ops, Q = b.n_reqs;
  const Stamps stamp{a.ev, st};
  hipError_t e = stamp(6);
  if (e != hipSuccess) return e;
  if (O)
    hipLaunchKernelGGL(k_w1_emit, dim3(cdiv((uint64_t)O * 16, 256)), dim3(256), 0, st, b, a.o, a.op_req, a.op_ref, a.cnt64,
                       a.cnt_off, a.len_off);
  if ((e = stamp(7)) != hipSuccess) return e;
  if (Q)
    hipLaunchKernelGGL(k_w1_reply<true>, dim3(cdiv((uint64_t)Q + 1, 256)), dim3(256), 0, st, b, a.o.op_decision, a.op_ref,
                       a.o.req_kind, a.ref64, a.ref_off, a.cnt_off, a.o.req_grant);
  e = hipGetLastError();
  return e != hipSuccess ? e : stamp(8);
}

}  // namespace mochi
