// result_decode.hip — Write2AnsFromServer / ReadFromServer bodies -> the arrays
// the response tally reads and the per-operation values it coalesces, on the
// device.  Level by level, so no lane walks a whole answer (one multi-kilobyte
// WriteCertificate per operation) with dependent loads:
//
//   k_rr_resp   level 1, lane = response: top-level framing, the kind's
//               strings, the TransactionResult's framing and entry count;
//               bodies outside the level-by-level shape (a repeated `result`,
//               more than 64 entries) are validated whole here
//   (scan)      operation offsets (64-bit)
//   k_rr_ops    level 3, lane = one OperationResult on the wire, grid-stride
//               over the device-side total: validates `result` and the
//               certificate all the way down, writes its slot if it is below
//               the request's count, ORs its status bits into its response
//   k_rr_final  level 4, lane = response: status, count, rid / nonce, and the
//               slots no operation filled
//   k_rr_coalesce  lane = request: the chosen response's values per op
//
// Every output size follows from the caller's arrays: nothing waits on the
// host.  The walk itself is result_decode.h's, shared with the host form.
// Every read of a body goes through its (base, length): lengths are the
// sender's.
#include "enc_launch.h"
#include "result_decode.h"

namespace mochi {
namespace {

using namespace rrd;

__global__ __launch_bounds__(256) void k_rr_resp(RRArgs a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p > a.P) return;
  if (p == a.P) {
    a.cnt[p] = 0;
    return;
  }
  const mochi_result_replies& in = a.v.in;
  Level1 o{0, 0, 0, 0, 0, 0, 0};
  const uint8_t kind = in.resp_kind[p];
  uint32_t bits = 0;
  if (parsed_kind(kind)) bits = resp_level(in.wire + in.resp_off[p], in.resp_len[p], kind, o);
  const uint32_t n_ops = in.n_ops[wire::request_of(in.req_resp_off, in.n_reqs, p)];
  a.st_bits[p] = bits;
  ((uint4*)a.l1)[2 * p] = make_uint4(o.tr_off, o.tr_len, o.n_wire, n_ops);
  ((uint4*)a.l1)[2 * p + 1] = make_uint4(o.rid_off, o.rid_len, o.nonce_off, o.nonce_len);
  a.cnt[p] = level3_ops(bits, o.n_wire);
}

__global__ __launch_bounds__(256) void k_rr_ops(RRArgs a) {
  const uint64_t total = a.e_base[a.P];
#pragma unroll 1
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t lo = 0, hi = a.P;  // the last response whose operations begin at or before e and that has any
#pragma unroll 1
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (a.e_base[mid] <= e) lo = mid;
      else hi = mid;
    }
    const uint32_t p = lo, j = (uint32_t)(e - a.e_base[p]);
    const uint4 l1 = ((const uint4*)a.l1)[2 * p];
    const uint32_t bits = op_level(a.v, p, l1.x, l1.y, j, l1.w);
    if (bits) atomicOr(a.st_bits + p, bits);
  }
}

__global__ __launch_bounds__(256) void k_rr_final(RRArgs a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.P) return;
  const uint4 x = ((const uint4*)a.l1)[2 * p], y = ((const uint4*)a.l1)[2 * p + 1];
  const Level1 l{x.x, x.y, x.z, y.x, y.y, y.z, y.w};
  resp_final(a.v, p, a.st_bits[p], l, x.w);
}

__global__ __launch_bounds__(256) void k_rr_coalesce(mochi_result_tallied t, mochi_result_coalesced o) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < t.n_reqs) coalesce_req(t, o, q);
}

}  // namespace

// two operations per response at full occupancy is the common shape; more take further strides
uint32_t rr_ops_blocks(uint32_t P) {
  const uint32_t b = cdiv(2 * (uint64_t)P, 256);
  return b < 1 ? 1 : b > 4096 ? 4096 : b;
}

hipError_t launch_rr_decode(const RRArgs& a, hipStream_t st) {
  const Stamps stamp{a.ev, st};
  hipError_t e;
  if ((e = stamp(0)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_rr_resp, dim3(cdiv((uint64_t)a.P + 1, 256)), dim3(256), 0, st, a);
  if ((e = hipGetLastError()) != hipSuccess || (e = stamp(1)) != hipSuccess) return e;
  if ((e = enc_scan64(a.scan_temp, a.scan_temp_bytes, a.cnt, a.e_base, a.P + 1, st)) != hipSuccess ||
      (e = stamp(2)) != hipSuccess)
    return e;
  hipLaunchKernelGGL(k_rr_ops, dim3(rr_ops_blocks(a.P)), dim3(256), 0, st, a);
  if ((e = hipGetLastError()) != hipSuccess || (e = stamp(3)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_rr_final, dim3(cdiv(a.P, 256)), dim3(256), 0, st, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return stamp(4);
}

hipError_t launch_rr_coalesce(const mochi_result_tallied& t, const mochi_result_coalesced& o, hipStream_t st) {
  hipLaunchKernelGGL(k_rr_coalesce, dim3(cdiv(t.n_reqs, 256)), dim3(256), 0, st, t, o);
  return hipGetLastError();
}

}  // namespace mochi
