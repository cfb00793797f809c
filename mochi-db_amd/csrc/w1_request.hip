// w1_request.hip — Write1ToServer bodies -> the wire half of mochi_write1_batch on
// the device, with the batch-wide key numbering, and the key-state join.  Level by
// level, so no lane validates a whole request with its values:
//
//   k_w1q_req      lane = request: top-level framing, UTF-8 of clientId and hash, the
//                  transaction's framing and its Operation entries counted; requests
//                  outside the level-by-level shape are validated whole here
//   (scan)         entry offsets (64-bit)
//   k_w1q_ops      lane = Operation entry, grid-stride over the device-side total:
//                  finds its entry by re-walking the transaction's framing (at most
//                  64 tags) and validates the Operation whole
//   k_w1q_final    lane = request: status, per-request outputs, the op count
//   (scan)         op offsets; k_w1q_offsets writes req_op_off.  The one host wait.
//   k_w1q_emit     lane = op: key slice and wire flags.  The entry total is not known
//                  on the host before the wait, so nothing per entry is kept in scratch:
//                  the lane re-walks to its Operation (valid by now; no UTF-8 pass)
//   k_w1q_claim    lane = op: open-addressing table in HBM, >= 2 * n_ops slots; the
//                  slot from a hash of the key bytes; a 32-bit compare-and-swap installs
//                  the claiming op's index, a probe that meets an occupied slot
//                  byte-compares its key with the claimer's slice and joins or goes on;
//                  a 32-bit atomicMin beside the slot keeps the smallest op index
//                  (k_w1_claim's pattern, the key compare done through the claimer)
//   k_w1q_rank     lane = op (a launch of its own: every claim must have landed): its
//                  key's first op; flags the ops that are one
//   (scan)         key numbers
//   k_w1q_number   op_obj, key_op, *n_keys
//   k_w1q_join     lane = op: the key's state onto the op (mochi_write1_state_join_device)
//
// k_w1q_ops and the key numbering (k_w1q_claim, k_w1q_rank, k_w1q_number) take narrow
// argument structs (EntryArgs, KeyNumArgs): the ReadToServer decoder (read_request.hip)
// launches the same kernels through launch_w1q_ops and launch_key_number.
//
// The hash decides no output: keys are numbered by their first op in op order.  The
// walk itself is w1_request.h's, shared with the host form.  Every read of a body goes
// through its (base, length): lengths are the sender's.
#include "enc_launch.h"
#include "w1_request.h"

namespace mochi {
namespace {

using namespace w1q;

constexpr uint32_t kNone = 0xFFFFFFFFu;

__device__ __forceinline__ void store_l1(uint32_t* l1, uint32_t q, const Level1& o) {
  ((uint4*)l1)[2 * q] = make_uint4(o.tx_off, o.tx_len, o.n_ent, o.seed);
  ((uint4*)l1)[2 * q + 1] = make_uint4(o.cl_off, o.cl_len, o.h_off, o.h_len);
}

__global__ __launch_bounds__(256) void k_w1q_req(W1ReqArgs a) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q > a.Q) return;
  if (q == a.Q) {
    a.cnt_e[q] = 0;
    return;
  }
  const mochi_write1_requests& in = a.v.in;
  Level1 o;
  const uint32_t bits = req_level(in.wire + in.msg_off[q], in.msg_len[q], o);
  a.st_bits[q] = bits;
  store_l1(a.l1, q, o);
  a.cnt_e[q] = bits ? 0 : o.n_ent;
}

__global__ __launch_bounds__(256) void k_w1q_ops(EntryArgs a) {
  const uint64_t total = a.e_base[a.Q];
#pragma unroll 1
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t lo = 0, hi = a.Q;  // the last request whose entries begin at or before e and that has entries
#pragma unroll 1
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (a.e_base[mid] <= e) lo = mid;
      else hi = mid;
    }
    const uint32_t q = lo, j = (uint32_t)(e - a.e_base[q]);
    const uint8_t* b = a.wire + a.msg_off[q];
    const uint4 l = ((const uint4*)a.l1)[2 * q];
    uint32_t eo, el;
    tx_entry(b, l.x, l.y, j, eo, el);
    Op op;
    if (!op_level(b, eo, el, true, op)) atomicOr(a.st_bits + q, kStMal);
  }
}

__global__ __launch_bounds__(256) void k_w1q_final(W1ReqArgs a) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q > a.Q) return;
  if (q == a.Q) {
    a.cnt64[q] = 0;
    return;
  }
  const uint4 l0 = ((const uint4*)a.l1)[2 * q], l1 = ((const uint4*)a.l1)[2 * q + 1];
  const Level1 l{l0.x, l0.y, l0.z, l0.w, l1.x, l1.y, l1.z, l1.w};
  a.cnt64[q] = final_req(a.v, q, a.st_bits[q], l);
}

__global__ __launch_bounds__(256) void k_w1q_offsets(W1ReqArgs a) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q <= a.Q) a.v.out.req_op_off[q] = (uint32_t)a.off64[q];
}

__global__ __launch_bounds__(256) void k_w1q_emit(W1ReqArgs a) {
  const uint32_t o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= a.n_ops) return;
  uint32_t lo = 0, hi = a.Q;  // the last request whose ops begin at or before o: the one that has it
#pragma unroll 1
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (a.off64[mid] <= o) lo = mid;
    else hi = mid;
  }
  const uint4 l = ((const uint4*)a.l1)[2 * lo];
  emit_op(a.v, lo, l.x, l.y, o - (uint32_t)a.off64[lo], o);
}

// the slot a key's probe starts at (wire_walk.h bytes_hash: keys that differ in their
// last byte alone spread over the table)
__device__ __forceinline__ uint32_t key_slot(const uint8_t* __restrict__ k, uint32_t n, uint32_t mask) {
  return wire::bytes_hash(k, n) & mask;
}

__global__ __launch_bounds__(256) void k_w1q_claim(KeyNumArgs a) {
  const uint32_t o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= a.n_ops) return;
  const uint32_t kl = a.op_key_len[o], mask = a.slots - 1;
  uint32_t slot = kNone;
  if (takes_part(a.op_flags[o], a.part, kl)) {
    const uint8_t* k = a.wire + a.op_key_off[o];
    uint32_t h = key_slot(k, kl, mask);
    // at most n_ops keys in >= 2 * n_ops slots: a free or equal slot is met within `mask` steps
#pragma unroll 1
    for (uint32_t n = 0; n <= mask; n++, h = (h + 1) & mask) {
      const uint32_t prev = atomicCAS(&a.tbl_op[h], kNone, o);
      // the claimer's slice was written by the emit kernel, a launch ago
      if (prev == kNone || prev == o ||
          (a.op_key_len[prev] == kl && wire::bytes_eq(a.wire + a.op_key_off[prev], k, kl))) {
        atomicMin(&a.tbl_min[h], o);
        slot = h;
        break;
      }
    }
  }
  a.op_slot[o] = slot;
}

__global__ __launch_bounds__(256) void k_w1q_rank(KeyNumArgs a) {
  const uint32_t o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o > a.n_ops) return;
  if (o == a.n_ops) {
    a.rep64[o] = 0;
    return;
  }
  const uint32_t s = a.op_slot[o];
  a.rep64[o] = s != kNone && a.tbl_min[s] == o ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_w1q_number(KeyNumArgs a) {
  const uint32_t o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o == 0) *a.n_keys = (uint32_t)a.key_off[a.n_ops];
  if (o >= a.n_ops) return;
  const uint32_t s = a.op_slot[o];
  uint32_t u = MOCHI_W1_NONE;
  if (s != kNone) {
    const uint32_t rep = a.tbl_min[s];
    u = (uint32_t)a.key_off[rep];
    if (rep == o) a.key_op[u] = o;
  }
  a.op_obj[o] = u;
}

__global__ __launch_bounds__(256) void k_w1q_join(JoinArgs a) {
  const uint32_t o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o < a.n_ops) join_op(a, o);
}

}  // namespace

hipError_t launch_w1q_count(const W1ReqArgs& a, hipStream_t st) {
  const Stamps stamp{a.ev, st};
  const uint32_t g1 = cdiv((uint64_t)a.Q + 1, 256);
  hipError_t e;
  if ((e = stamp(0)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_w1q_req, dim3(g1), dim3(256), 0, st, a);
  if ((e = hipGetLastError()) != hipSuccess || (e = stamp(1)) != hipSuccess) return e;
  if ((e = enc_scan64(a.scan_temp, a.scan_temp_bytes, a.cnt_e, a.e_base, a.Q + 1, st)) != hipSuccess ||
      (e = stamp(2)) != hipSuccess)
    return e;
  if ((e = launch_w1q_ops(EntryArgs{a.v.in.wire, a.v.in.msg_off, a.Q, a.e_base, a.l1, a.st_bits}, st)) != hipSuccess ||
      (e = stamp(3)) != hipSuccess)
    return e;
  hipLaunchKernelGGL(k_w1q_final, dim3(g1), dim3(256), 0, st, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = enc_scan64(a.scan_temp, a.scan_temp_bytes, a.cnt64, a.off64, a.Q + 1, st)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_w1q_offsets, dim3(g1), dim3(256), 0, st, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return stamp(4);
}

hipError_t launch_w1q_ops(const EntryArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_w1q_ops, dim3(w1q_ops_blocks(a.Q)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_key_number(const KeyNumArgs& a, hipStream_t st) {
  const Stamps stamp{a.ev, st};
  const uint32_t O = a.n_ops, g0 = cdiv(O, 256), g1 = cdiv((uint64_t)O + 1, 256);
  hipError_t e;
  // every slot empty, every minimum "no op"
  if ((e = hipMemsetAsync(a.tbl_op, 0xFF, (size_t)((uint8_t*)(a.tbl_min + a.slots) - (uint8_t*)a.tbl_op), st)) != hipSuccess)
    return e;
  if (O) hipLaunchKernelGGL(k_w1q_claim, dim3(g0), dim3(256), 0, st, a);
  if ((e = hipGetLastError()) != hipSuccess || (e = stamp(0)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_w1q_rank, dim3(g1), dim3(256), 0, st, a);
  if ((e = hipGetLastError()) != hipSuccess || (e = stamp(1)) != hipSuccess) return e;
  if ((e = enc_scan64(a.scan_temp, a.scan_temp_bytes, a.rep64, a.key_off, O + 1, st)) != hipSuccess ||
      (e = stamp(2)) != hipSuccess)
    return e;
  hipLaunchKernelGGL(k_w1q_number, dim3(g1), dim3(256), 0, st, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return stamp(3);
}

hipError_t launch_w1q_emit(const W1ReqArgs& a, hipStream_t st) {
  const Stamps stamp{a.ev, st};
  const uint32_t O = a.n_ops;
  hipError_t e;
  if ((e = stamp(5)) != hipSuccess) return e;
  if (O) hipLaunchKernelGGL(k_w1q_emit, dim3(cdiv(O, 256)), dim3(256), 0, st, a);
  if ((e = hipGetLastError()) != hipSuccess || (e = stamp(6)) != hipSuccess) return e;
  const mochi_write1_requests_decoded& out = a.v.out;
  KeyNumArgs k = a.k;  // n_ops, slots and the table from the caller
  k.wire = a.v.in.wire;
  k.op_key_off = out.op_key_off;
  k.op_key_len = out.op_key_len;
  k.op_flags = out.op_flags;
  k.part = kWD;
  k.op_obj = out.op_obj;
  k.key_op = out.key_op;
  k.n_keys = a.n_keys;
  k.scan_temp = a.scan_temp;
  k.scan_temp_bytes = a.scan_temp_bytes;
  k.ev = a.ev ? a.ev + 7 : nullptr;
  return launch_key_number(k, st);
}

hipError_t launch_w1q_join(const JoinArgs& a, hipStream_t st) {
  if (a.n_ops) hipLaunchKernelGGL(k_w1q_join, dim3(cdiv(a.n_ops, 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace mochi
