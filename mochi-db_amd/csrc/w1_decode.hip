// w1_decode.hip — Write1OkFromServer / Write1RefusedFromServer bodies -> the
// SoA arrays the Write1 classifier and the Write2 encoder read, on the device.
// Level by level, so no lane walks a whole reply (a MultiGrant plus one
// multi-kilobyte WriteCertificate per key) with dependent loads:
//
//   k_w1d_resp     level 1, lane = response: top-level framing, the certificate
//                  entries' framing and keys (UTF-8, distinct keys); bodies
//                  outside the level-by-level shape are validated whole here
//   (scan)         level-2 entry offsets (64-bit)
//   k_w1d_level2   level 2, lane = the MultiGrant or one certificate entry of a
//                  response, grid-stride over the device-side total: validates
//                  the value all the way down; the MultiGrant lane also resolves
//                  the grants map, checks the decoded grants canonical and finds
//                  the server
//   k_w1d_final    lane = response: status, kind, server, client id, counts
//   (scan)         grants | certificates << 32 in one packed 64-bit scan
//   k_w1d_offsets  both CSRs from the packed scan
//   k_w1d_emit     lane = decoded response: its grants (zero copy into the wire
//                  blob) and certificate entries
//   k_w2_sig       the signatures, 16 lanes each (w2_decode.hip's gather)
//
// The walk itself is w1_decode.h's, shared with the host form.  Every read of
// a body goes through its (base, length): lengths are the sender's.
#include "enc_launch.h"
#include "w1_decode.h"
#include "w2.h"

namespace mochi {
namespace {

using namespace w1d;

__global__ __launch_bounds__(256) void k_w1d_resp(W1DecArgs a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p > a.P) return;
  if (p == a.P) {
    a.cnt_e[p] = 0;
    return;
  }
  const mochi_write1_replies& in = a.v.in;
  Level1 o{0, 0, 0, 0};
  uint32_t bits = 0, ne = 0;
  if (parsed_kind(in.resp_kind[p])) {
    bits = resp_level(in.wire + in.resp_off[p], in.resp_len[p], o);
    if (!bits) ne = 1 + o.n_ce;
  }
  a.st_bits[p] = bits;
  a.ng[p] = 0;
  ((uint4*)a.l1)[p] = make_uint4(o.mg_off, o.mg_len, o.n_ce, o.n_keys);
  ((uint4*)a.l2)[p] = make_uint4(0, 0, 0, 0);
  a.cnt_e[p] = ne;
}

__global__ __launch_bounds__(256) void k_w1d_level2(W1DecArgs a) {
  const mochi_write1_replies& in = a.v.in;
  const uint64_t total = a.e_base[a.P];
#pragma unroll 1
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t lo = 0, hi = a.P;  // the last response whose entries begin at or before e and that has entries
#pragma unroll 1
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (a.e_base[mid] <= e) lo = mid;
      else hi = mid;
    }
    const uint32_t p = lo, j = (uint32_t)(e - a.e_base[p]);
    const uint8_t* b = in.wire + in.resp_off[p];
    const uint4 l1 = ((const uint4*)a.l1)[p];
    uint32_t bits;
    if (j == 0) {
      Level2 o;
      bits = mg_level(b, l1.x, l1.y, o);
      a.ng[p] = o.ng;
      ((uint4*)a.l2)[p] = make_uint4(o.sid_off, o.sid_len, o.cl_off, o.cl_len);
    } else {
      uint32_t vo, vl;
      cert_entry_value(b, in.resp_len[p], j - 1, vo, vl);
      bits = valid_writecert(b, vo, vl) ? 0u : kStMal;
    }
    if (bits) atomicOr(a.st_bits + p, bits);
  }
}

__global__ __launch_bounds__(256) void k_w1d_final(W1DecArgs a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p > a.P) return;
  if (p == a.P) {
    a.cnt64[p] = 0;
    return;
  }
  const mochi_write1_replies& in = a.v.in;
  const mochi_write1_decoded& out = a.v.out;
  const uint8_t kind = in.resp_kind[p];
  const uint32_t bits = a.st_bits[p];
  uint8_t st = MOCHI_W1R_OK, kind_out = kind;
  uint32_t server = 0x80000000u | p, ng = 0, nc = 0;
  uint16_t signer = 0xFFFF;
  uint64_t cl_off = 0;
  uint32_t cl_len = 0;
  if (bits & kStMal) st = MOCHI_W1R_MALFORMED;
  else if (bits & kStFb) st = MOCHI_W1R_FALLBACK;
  if (st != MOCHI_W1R_OK) {
    kind_out = MOCHI_W1_OTHER;
  } else if (parsed_kind(kind)) {
    const uint64_t base = in.resp_off[p];
    const uint4 l2 = ((const uint4*)a.l2)[p];
    signer = find_server(in.wire + base + l2.x, l2.y, a.v.ids, a.v.id_off, a.v.n_ids);
    if (signer == 0xFFFF) st = MOCHI_W1R_UNKNOWN_SERVER;
    else server = signer;
    cl_off = base + l2.z;
    cl_len = l2.w;
    ng = a.ng[p];
    nc = ((const uint4*)a.l1)[p].w;
  }
  out.resp_status[p] = st;
  out.resp_kind_out[p] = kind_out;
  out.resp_server[p] = server;
  out.mg_signer[p] = signer;
  out.resp_client_off[p] = cl_off;
  out.resp_client_len[p] = cl_len;
  a.cnt64[p] = (uint64_t)ng | (uint64_t)nc << 32;
}

__global__ __launch_bounds__(256) void k_w1d_offsets(W1DecArgs a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p > a.P) return;
  const uint64_t o = a.off64[p];
  a.v.out.resp_grant_off[p] = (uint32_t)o;
  a.v.out.resp_cert_off[p] = (uint32_t)(o >> 32);
}

__global__ __launch_bounds__(256) void k_w1d_emit(W1DecArgs a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.P) return;
  const uint64_t o = a.off64[p];
  if (a.off64[p + 1] == o) return;  // nothing decoded from this response
  const uint4 l1 = ((const uint4*)a.l1)[p];
  emit_resp(a.v, p, l1.x, l1.y, (uint32_t)o, (uint32_t)(o >> 32));
}

// grid of the grid-stride level-2 kernel (the entry total is on the device)
inline uint32_t l2_blocks(uint32_t P) {
  const uint32_t b = cdiv(2 * (uint64_t)P, 256);
  return b < 1 ? 1 : b > 4096 ? 4096 : b;
}

}  // namespace

hipError_t launch_w1d_count(const W1DecArgs& a, hipStream_t st) {
  const Stamps stamp{a.ev, st};
  const uint32_t g1 = cdiv((uint64_t)a.P + 1, 256);
  hipError_t e;
  if ((e = stamp(0)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_w1d_resp, dim3(g1), dim3(256), 0, st, a);
  if ((e = hipGetLastError()) != hipSuccess || (e = stamp(1)) != hipSuccess) return e;
  if ((e = enc_scan64(a.scan_temp, a.scan_temp_bytes, a.cnt_e, a.e_base, a.P + 1, st)) != hipSuccess ||
      (e = stamp(2)) != hipSuccess)
    return e;
  hipLaunchKernelGGL(k_w1d_level2, dim3(l2_blocks(a.P)), dim3(256), 0, st, a);
  if ((e = hipGetLastError()) != hipSuccess || (e = stamp(3)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_w1d_final, dim3(g1), dim3(256), 0, st, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = enc_scan64(a.scan_temp, a.scan_temp_bytes, a.cnt64, a.off64, a.P + 1, st)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_w1d_offsets, dim3(g1), dim3(256), 0, st, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return stamp(4);
}

hipError_t launch_w1d_emit(const W1DecArgs& a, uint32_t n_grants, hipStream_t st) {
  const Stamps stamp{a.ev, st};
  hipError_t e;
  if ((e = stamp(5)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_w1d_emit, dim3(cdiv(a.P, 256)), dim3(256), 0, st, a);
  if ((e = hipGetLastError()) != hipSuccess || (e = stamp(6)) != hipSuccess) return e;
  if (a.v.sig_src && n_grants &&
      (e = launch_w2_sig(a.v.in.wire, a.v.sig_src, n_grants, a.v.out.sig, st)) != hipSuccess)
    return e;
  return stamp(7);
}

}  // namespace mochi
