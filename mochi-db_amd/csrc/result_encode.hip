// result_encode.hip — the answer ENCODER on the device (gfx950): the
// Write2AnsFromServer / ReadFromServer bodies of a batch from the caller's
// per-response and per-slot arrays (layout and sizes: result_encode.h), packed
// back to back with 64-bit offsets, and the plan kernel that fills those arrays
// from the Write2 verifier's outputs.  Built like w1_reply.hip:
//   k_rae_size   lane = response    per slot where its operation lies in the TransactionResult
//                                   (op_rel); TransactionResult / message length, status
//   exclusive scan of the message lengths in 64 bits (hipcub; inside k_rae_size's
//                single block for a small batch, where w2_small draws the line)
//   k_rae_hdr    lane = (response, op), grid-stride; op 0's lane is also the response's:
//                every tag, length, existed, status, rid and nonce; per slot where
//                its two payloads go (op_dst)
//   k_rae_copy   the payloads: 16 lanes per slot for the `result` string, one wave
//                per slot for the certificate (k_w1r_copy's split: ~2.9 KB at R = 4,
//                three rounds of one dwordx4 store per lane, a contiguous 1 KiB each)
//   k_w2a_plan   lane = message     rae::plan_msg, the walk the host twin runs
// The header kernel leaves the payload bytes alone; the copy kernel writes only
// payload bytes (enc_dev.h).  Both read the scanned total first and write
// nothing when it exceeds wire_cap: the capacity rule without a host wait.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "enc_dev.h"
#include "enc_launch.h"
#include "result_encode.h"
#include "w2.h"

namespace mochi {
namespace {

using rae::kNone;

// ---- sizes: lane = response ------------------------------------------------------
// kSmall: one block of 1024 lanes, P < 1024; the 64-bit scan runs in the block.
template <bool kSmall>
__global__ __launch_bounds__(kSmall ? 1024 : 256) void k_rae_size(mochi_result_answers a, uint32_t* __restrict__ op_rel,
                                                                  uint32_t* __restrict__ resp_tx,
                                                                  uint32_t* __restrict__ msg_len,
                                                                  uint8_t* __restrict__ status,
                                                                  uint64_t* __restrict__ len64,
                                                                  uint64_t* __restrict__ off64,
                                                                  uint64_t* __restrict__ msg_off) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t P = a.n_resps;
  uint64_t mine = 0;
  if (p < P) {
    const rae::Sized z = rae::size_resp(a, p, op_rel);
    mine = z.len;
    status[p] = z.status;
    msg_len[p] = (uint32_t)z.len;
    resp_tx[p] = (uint32_t)z.tx;
  }
  enc_place<kSmall>(p, P, mine, len64, off64, msg_off);
}

// ---- headers: lane = (response, op) ------------------------------------------------
__global__ __launch_bounds__(256) void k_rae_hdr(mochi_result_answers a, const uint32_t* __restrict__ op_rel,
                                                 const uint32_t* __restrict__ resp_tx,
                                                 const uint32_t* __restrict__ msg_len,
                                                 const uint64_t* __restrict__ msg_off,
                                                 const uint64_t* __restrict__ total, uint64_t wire_cap,
                                                 uint8_t* __restrict__ wire, uint64_t* __restrict__ op_dst) {
  if (*total > wire_cap) return;  // op_dst stays ~0 everywhere (the launch cleared it)
  const uint64_t n = (uint64_t)a.n_resps * rae::kMaxOps;
#pragma unroll 1
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t p = (uint32_t)(t / rae::kMaxOps), j = (uint32_t)(t % rae::kMaxOps);
    const uint32_t len = msg_len[p];
    // a response without a body, or one that is not OK; a response with a body has at least 0A 00
    if (len == 0) continue;
    const uint32_t tx = resp_tx[p];
    uint8_t* m0 = wire + msg_off[p];
    const uint32_t tx_at = 1 + wire::varint_size(tx);
    if (j == 0) {
      Put h(m0);
      h.byte(0x0A);
      h.varint(tx);
      h.flush();
      const uint32_t rl = rae::rid_len(a, p), nl = rae::nonce_len(a, p);
      Put q(m0 + tx_at + tx);
      if (nl) q.ld(0x12, a.ids + a.nonce_off[p], nl);
      if (rl) q.ld(a.resp_kind[p] == MOCHI_RR_READ ? 0x1A : 0x12, a.ids + a.rid_off[p], rl);
      q.flush();
    }
    if (j >= a.resp_n_ops[p]) continue;
    const uint64_t s = a.slot_off[p] + j;
    const uint32_t rl = a.op_result_len[s], cl = a.op_cert_len[s];
    const uint8_t fl = a.op_flags[s], st = a.op_status[s];
    Put o(m0 + tx_at + op_rel[s]);
    o.byte(0x0A);
    o.varint(rae::op_body(a, s));
    uint64_t dr = kNone, dc = kNone;
    if (rl) {
      o.byte(0x0A);
      o.varint(rl);
      dr = (uint64_t)(o.p - wire);
      o.skip(rl);
    }
    if (fl & MOCHI_RAO_HAS_CERT) {
      o.byte(0x12);
      o.varint(cl);
      if (cl) dc = (uint64_t)(o.p - wire);
      o.skip(cl);
    }
    if (a.op_existed[s]) {
      o.byte(0x18);
      o.byte(0x01);
    }
    if (st) {
      o.byte(0x20);
      o.varint(st);
    }
    o.flush();
    op_dst[2 * s] = dr;
    op_dst[2 * s + 1] = dc;
  }
}

// ---- payload copy (enc_dev.h copy_chunk) --------------------------------------------
// blocks [0, small_blocks): 16 lanes per slot, its `result` string; the blocks after
// them: one wave per slot, its certificate
__global__ __launch_bounds__(256) void k_rae_copy(mochi_result_answers a, const uint64_t* __restrict__ op_dst,
                                                  const uint64_t* __restrict__ total, uint64_t wire_cap,
                                                  uint32_t small_blocks, uint8_t* __restrict__ wire) {
  if (*total > wire_cap) return;
  const uint64_t S = a.n_slots;
  if (blockIdx.x < small_blocks) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t s = t >> 4;
    if (s >= S) return;
    const uint64_t d = op_dst[2 * s];
    if (d == kNone) return;
    const uint8_t* src = (a.op_flags[s] & MOCHI_RAO_RESULT_STORE ? a.store : a.wire) + a.op_result_off[s];
    copy_run((uint32_t)(t & 15), (uintptr_t)(wire + d), src, a.op_result_len[s]);
    return;
  }
  const uint64_t s = ((uint64_t)(blockIdx.x - small_blocks) * blockDim.x + threadIdx.x) >> 6;
  if (s >= S) return;
  const uint64_t d = op_dst[2 * s + 1];
  if (d == kNone) return;
  const uint32_t cl = a.op_cert_len[s];
  const uint8_t* cert = (a.op_flags[s] & MOCHI_RAO_CERT_STORE ? a.store : a.wire) + a.op_cert_off[s];
  const uintptr_t d0 = (uintptr_t)(wire + d);
  const uint32_t n = run_chunks(d0, cl);
#pragma unroll 1
  for (uint32_t c = threadIdx.x & 63; c < n; c += 64) copy_chunk(d0, cert, cl, c);
}

// ---- the plan: lane = message ----------------------------------------------------------
__global__ __launch_bounds__(256) void k_w2a_plan(rae::PlanView v) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m < v.b.n_msgs) rae::plan_msg(v, m);
}

}  // namespace

hipError_t launch_rae_size(const RaeArgs& a, hipStream_t st) {
  const uint32_t P = a.in.n_resps;
  const Stamps stamp{a.ev, st};
  hipError_t e = stamp(0);
  if (e != hipSuccess) return e;
  if (w2_small(P)) {
    hipLaunchKernelGGL(k_rae_size<true>, dim3(1), dim3(1024), 0, st, a.in, a.op_rel, a.resp_tx, a.msg_len, a.status,
                       a.len64, a.off64, a.msg_off);
    if ((e = stamp(1)) != hipSuccess || (e = stamp(2)) != hipSuccess) return e;
    return hipGetLastError();
  }
  hipLaunchKernelGGL(k_rae_size<false>, dim3(cdiv((uint64_t)P + 1, 256)), dim3(256), 0, st, a.in, a.op_rel, a.resp_tx,
                     a.msg_len, a.status, a.len64, a.off64, a.msg_off);
  e = hipGetLastError();
  if (e != hipSuccess || (e = stamp(1)) != hipSuccess) return e;
  e = enc_scan_offsets(a.scan_temp, a.scan_temp_bytes, a.len64, a.off64, a.msg_off, P, st);
  return e != hipSuccess ? e : stamp(2);
}

hipError_t launch_rae_emit(const RaeArgs& a, hipStream_t st) {
  const uint32_t P = a.in.n_resps;
  const uint64_t S = a.in.n_slots;
  const uint64_t* total = a.off64 + P;
  const Stamps stamp{a.ev, st};
  hipError_t e = stamp(3);
  if (e != hipSuccess) return e;
  if (S) {
    // a slot no response with a body owns has no payload: ~0 until k_rae_hdr says otherwise
    if ((e = hipMemsetAsync(a.op_dst, 0xFF, 16 * S, st)) != hipSuccess) return e;
  }
  if (P) {
    // grid-stride over P * 64 (response, op) pairs; 64 consecutive lanes share a response
    const uint64_t pairs = (uint64_t)P * rae::kMaxOps;
    const uint32_t blocks = pairs / 256 > 16384 ? 16384 : cdiv(pairs, 256);
    hipLaunchKernelGGL(k_rae_hdr, dim3(blocks), dim3(256), 0, st, a.in, a.op_rel, a.resp_tx, a.msg_len, a.msg_off, total,
                       a.wire_cap, a.wire, a.op_dst);
  }
  if ((e = stamp(4)) != hipSuccess) return e;
  if (S) {
    const uint32_t small_blocks = cdiv(S * 16, 256), cert_blocks = cdiv(S * 64, 256);
    hipLaunchKernelGGL(k_rae_copy, dim3(small_blocks + cert_blocks), dim3(256), 0, st, a.in, a.op_dst, total, a.wire_cap,
                       small_blocks, a.wire);
  }
  e = hipGetLastError();
  return e != hipSuccess ? e : stamp(5);
}

hipError_t launch_w2a_plan(const rae::PlanView& v, hipStream_t st) {
  hipLaunchKernelGGL(k_w2a_plan, dim3(cdiv(v.b.n_msgs, 256)), dim3(256), 0, st, v);
  return hipGetLastError();
}

}  // namespace mochi
