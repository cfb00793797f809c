// enc_launch.h — host-side launch helpers shared by the wire encoders
// (w2_encode.hip, w1_issue.hip, w1_reply.hip, result_encode.hip): grid arithmetic, the scratch
// layout cursor (carve.h), the per-kernel profiling stamps and the 64-bit hipcub scans.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stddef.h>
#include <stdint.h>

#include "carve.h"

namespace mochi {

inline uint32_t cdiv(uint64_t a, uint32_t b) { return (uint32_t)((a + b - 1) / b); }

// per-kernel timing: records event i on the stream when the call is profiled (ev != null)
struct Stamps {
  hipEvent_t* ev;
  hipStream_t st;
  hipError_t operator()(int i) const { return ev ? hipEventRecord(ev[i], st) : hipSuccess; }
};

// 64-bit exclusive sum of in[0, n) into out (hipcub); temp: enc_scan_temp_bytes(n) bytes or more (w2_encode.h/.hip)
inline hipError_t enc_scan64(void* temp, size_t temp_bytes, const uint64_t* in, uint64_t* out, uint32_t n,
                             hipStream_t st) {
  return hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, in, out, (int)n, st);
}

// the large-batch end of a size phase: off64[0, n] = exclusive sum of len64[0, n]
// (off64[n] = the total), and the first n offsets into the caller's msg_off
inline hipError_t enc_scan_offsets(void* temp, size_t temp_bytes, const uint64_t* len64, uint64_t* off64,
                                   uint64_t* msg_off, uint32_t n, hipStream_t st) {
  const hipError_t e = enc_scan64(temp, temp_bytes, len64, off64, n + 1, st);
  return e != hipSuccess ? e : hipMemcpyAsync(msg_off, off64, 8 * (size_t)n, hipMemcpyDeviceToDevice, st);
}

}  // namespace mochi
