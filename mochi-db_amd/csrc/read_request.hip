// read_request.hip — ReadToServer bodies -> SoA arrays with the batch-wide key numbering
// on the device, and the read answer plan.  Level by level, the shape of w1_request.hip:
//
//   k_rdq_req      lane = request: top-level framing, UTF-8 of clientId and nonce, the
//                  transaction's framing and its Operation entries counted; requests
//                  outside the level-by-level shape are validated whole here
//   (scan)         entry offsets (64-bit)
//   k_w1q_ops      w1_request.hip's entry kernel (launch_w1q_ops, grid w1q_ops_blocks):
//                  lane = Operation entry, grid-stride, validates the Operation whole
//   k_rdq_final    lane = request: status, per-request outputs, the op count
//   (scan)         op offsets; k_rdq_offsets writes req_op_off.  The one host wait.
//   k_rdq_emit     lane = op: key slice and MOCHI_RDOP_READ (the lane re-walks to its
//                  Operation, valid by now; no UTF-8 pass)
//   key numbering  w1_request.hip's k_w1q_claim / k_w1q_rank / (scan) / k_w1q_number
//                  (launch_key_number) with READ as the takes-part flag
//   k_rda_plan     lane = request (at most 64 ops each): mochi_read_answer_plan_device
//
// The walk is read_request.h's and w1_request.h's, shared with the host form.  Every
// read of a body goes through its (base, length): lengths are the sender's.
#include "enc_launch.h"
#include "read_request.h"

namespace mochi {
namespace {

using namespace rdq;

__global__ __launch_bounds__(256) void k_rdq_req(RdReqArgs a) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q > a.Q) return;
  if (q == a.Q) {
    a.cnt_e[q] = 0;
    return;
  }
  const mochi_read_requests& in = a.v.in;
  Level1 o;
  const uint32_t bits = req_level(in.wire + in.msg_off[q], in.msg_len[q], o);
  a.st_bits[q] = bits;
  ((uint4*)a.l1)[2 * q] = make_uint4(o.tx_off, o.tx_len, o.n_ent, 0);
  ((uint4*)a.l1)[2 * q + 1] = make_uint4(o.cl_off, o.cl_len, o.nn_off, o.nn_len);
  a.cnt_e[q] = bits ? 0 : o.n_ent;
}

__global__ __launch_bounds__(256) void k_rdq_final(RdReqArgs a) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q > a.Q) return;
  if (q == a.Q) {
    a.cnt64[q] = 0;
    return;
  }
  const uint4 l0 = ((const uint4*)a.l1)[2 * q], l1 = ((const uint4*)a.l1)[2 * q + 1];
  const Level1 l{l0.x, l0.y, l0.z, 0, l1.x, l1.y, l1.z, l1.w};
  a.cnt64[q] = final_req(a.v, q, a.st_bits[q], l);
}

__global__ __launch_bounds__(256) void k_rdq_offsets(RdReqArgs a) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q <= a.Q) a.v.out.req_op_off[q] = (uint32_t)a.off64[q];
}

__global__ __launch_bounds__(256) void k_rdq_emit(RdReqArgs a) {
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

__global__ __launch_bounds__(256) void k_rda_plan(PlanView v) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < v.n_reqs) plan_req(v, q);
}

}  // namespace

hipError_t launch_rdq_count(const RdReqArgs& a, hipStream_t st) {
  const Stamps stamp{a.ev, st};
  const uint32_t g1 = cdiv((uint64_t)a.Q + 1, 256);
  hipError_t e;
  if ((e = stamp(0)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_rdq_req, dim3(g1), dim3(256), 0, st, a);
  if ((e = hipGetLastError()) != hipSuccess || (e = stamp(1)) != hipSuccess) return e;
  if ((e = enc_scan64(a.scan_temp, a.scan_temp_bytes, a.cnt_e, a.e_base, a.Q + 1, st)) != hipSuccess ||
      (e = stamp(2)) != hipSuccess)
    return e;
  if ((e = launch_w1q_ops(EntryArgs{a.v.in.wire, a.v.in.msg_off, a.Q, a.e_base, a.l1, a.st_bits}, st)) != hipSuccess ||
      (e = stamp(3)) != hipSuccess)
    return e;
  hipLaunchKernelGGL(k_rdq_final, dim3(g1), dim3(256), 0, st, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = enc_scan64(a.scan_temp, a.scan_temp_bytes, a.cnt64, a.off64, a.Q + 1, st)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_rdq_offsets, dim3(g1), dim3(256), 0, st, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return stamp(4);
}

hipError_t launch_rdq_emit(const RdReqArgs& a, hipStream_t st) {
  const Stamps stamp{a.ev, st};
  const uint32_t O = a.n_ops;
  hipError_t e;
  if ((e = stamp(5)) != hipSuccess) return e;
  if (O) hipLaunchKernelGGL(k_rdq_emit, dim3(cdiv(O, 256)), dim3(256), 0, st, a);
  if ((e = hipGetLastError()) != hipSuccess || (e = stamp(6)) != hipSuccess) return e;
  const mochi_read_requests_decoded& out = a.v.out;
  KeyNumArgs k = a.k;  // n_ops, slots and the table from the caller
  k.wire = a.v.in.wire;
  k.op_key_off = out.op_key_off;
  k.op_key_len = out.op_key_len;
  k.op_flags = out.op_flags;
  k.part = MOCHI_RDOP_READ;
  k.op_obj = out.op_obj;
  k.key_op = out.key_op;
  k.n_keys = a.n_keys;
  k.scan_temp = a.scan_temp;
  k.scan_temp_bytes = a.scan_temp_bytes;
  k.ev = a.ev ? a.ev + 7 : nullptr;
  return launch_key_number(k, st);
}

hipError_t launch_rda_plan(const PlanView& v, hipStream_t st) {
  if (v.n_reqs) hipLaunchKernelGGL(k_rda_plan, dim3(cdiv(v.n_reqs, 256)), dim3(256), 0, st, v);
  return hipGetLastError();
}

}  // namespace mochi
