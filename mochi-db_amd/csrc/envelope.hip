// envelope.hip — the ProtocolMessage envelope codec on the device (gfx950): frames in
// HBM to the inputs of the body decoders, and bodies in HBM to frames (layout, walk and
// sizes: envelope.h, shared with the host twin).
//
//   decode   k_env_decode   lane = frame: env::decode_frame.  The top level of a frame is
//                           short (a canonical one has at most five fields), so one
//                           serial walk per lane; no scratch.
//   route    k_env_hist     block of 256 frames: per bin (kind 0..12, 13 = takes no place)
//                           the block's count, from one ballot per bin and wave
//            (scan)         over the counts bin-major: the base of every (bin, block)
//            k_env_scatter  the block's ballots again: a frame's place is that base + the
//                           frames of its bin in the block's earlier waves + the lanes
//                           of its bin below it.  No rank comes from arrival at an atomic.
//   join     k_env_claim    lane = request: the msgId table, k_w1q_claim's open addressing
//                           (w1_request.hip): a 32-bit compare-and-swap installs the
//                           claiming request, an occupied slot is byte-compared with the
//                           claimer's id, a 32-bit atomicMin keeps the smallest index
//            k_env_lookup   lane = frame (a launch of its own: every claim has landed):
//                           probes for its replyToMsgId; frame_req and the sort key
//            (sort)         stable radix sort of (request, frame) by request
//            k_env_group    req_resp_off by a binary search per request, the grouped
//                           per-response arrays, *n_resps
//   encode   k_env_size     lane = message: status, length, prefix
//            (scan)         frame offsets in 64 bits (inside k_env_size's single block
//                           for a small batch, where w2_small draws the line)
//            k_env_hdr      lane = message: msg_off; prefix, scalars, the payload's tag and
//                           length; where the body goes
//            k_env_copy     the bodies with enc_dev.h's chunk copy: 16 lanes per body of
//                           at most kShortBody bytes, one wave per longer one
// The hash decides no output.  Every read of a frame goes through its (base, length).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "enc_dev.h"
#include "enc_launch.h"
#include "envelope.h"
#include "w2.h"

namespace mochi {
namespace {

using namespace env;

constexpr uint32_t kBins = kKinds + 1;
constexpr uint32_t kShortBody = 256;  // 16 lanes x one dwordx4 each

// ---- decode ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_env_decode(DecView v) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f < v.in.n_frames) decode_frame(v, f);
}

// ---- route -------------------------------------------------------------------------------
// Per wave and bin the count of the wave's lanes in that bin (into cnt[wave][bin]); returns
// how many lanes of this lane's bin lie below it in its wave.
__device__ __forceinline__ uint32_t wave_bins(uint32_t bin, uint32_t (*cnt)[kBins]) {
  const uint32_t w = threadIdx.x >> 6;
  uint32_t below = 0;
#pragma unroll
  for (uint32_t k = 0; k < kBins; k++) {
    const uint64_t m = __ballot(bin == k);
    if ((threadIdx.x & 63) == 0) cnt[w][k] = (uint32_t)__popcll(m);
    if (bin == k) below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
  }
  return below;
}

__global__ __launch_bounds__(256) void k_env_hist(EnvRouteArgs a) {
  __shared__ uint32_t cnt[4][kBins];
  const uint32_t f = blockIdx.x * 256 + threadIdx.x;
  // a lane past n is in no bin
  const uint32_t bin = f < a.v.n ? route_bin(a.v.status[f], a.v.kind[f]) : kBins;
  (void)wave_bins(bin, cnt);
  __syncthreads();
  if (threadIdx.x < kBins)
    a.hist64[(uint64_t)threadIdx.x * a.blocks + blockIdx.x] =
        (uint64_t)cnt[0][threadIdx.x] + cnt[1][threadIdx.x] + cnt[2][threadIdx.x] + cnt[3][threadIdx.x];
  if (blockIdx.x == 0 && threadIdx.x == 0) a.hist64[(uint64_t)kBins * a.blocks] = 0;
}

__global__ __launch_bounds__(256) void k_env_scatter(EnvRouteArgs a) {
  __shared__ uint32_t cnt[4][kBins];
  const uint32_t f = blockIdx.x * 256 + threadIdx.x;
  const uint32_t bin = f < a.v.n ? route_bin(a.v.status[f], a.v.kind[f]) : kBins;
  const uint32_t below = wave_bins(bin, cnt);
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x < kBins) a.v.out.kind_off[threadIdx.x] = (uint32_t)a.base64[(uint64_t)threadIdx.x * a.blocks];
  if (bin >= kKinds) return;
  uint32_t i = (uint32_t)a.base64[(uint64_t)bin * a.blocks + blockIdx.x] + below;
  for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) i += cnt[w][bin];
  a.v.out.order[i] = f;
  a.v.out.body_off[i] = a.v.body_off[f];
  a.v.out.body_len[i] = a.v.body_len[f];
}

// ---- join --------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_env_claim(EnvJoinArgs a) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  const mochi_envelope_requests& rq = a.v.rq;
  if (q >= rq.n_reqs) return;
  const uint32_t kl = rq.id_len[q], mask = a.slots - 1;
  if (!kl) return;  // an empty id is matched by nothing
  const uint8_t* k = rq.ids + rq.id_off[q];
  uint32_t h = wire::bytes_hash(k, kl) & mask;
  // at most Q ids in >= 2 * Q slots: a free or equal slot is met within `mask` steps
#pragma unroll 1
  for (uint32_t n = 0; n <= mask; n++, h = (h + 1) & mask) {
    const uint32_t prev = atomicCAS(&a.tbl_req[h], kNone, q);
    if (prev == kNone || prev == q || (rq.id_len[prev] == kl && wire::bytes_eq(rq.ids + rq.id_off[prev], k, kl))) {
      atomicMin(&a.tbl_min[h], q);
      break;
    }
  }
}

__global__ __launch_bounds__(256) void k_env_lookup(EnvJoinArgs a) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= a.v.fr.n_frames) return;
  const mochi_envelope_requests& rq = a.v.rq;
  uint32_t q = kNone;
  if (join_asks(a.v, f)) {
    const uint32_t kl = a.v.dec.reply_to_len[f], mask = a.slots - 1;
    const uint8_t* k = a.v.fr.wire + a.v.dec.reply_to_off[f];
    uint32_t h = wire::bytes_hash(k, kl) & mask;
#pragma unroll 1
    for (uint32_t n = 0; n <= mask; n++, h = (h + 1) & mask) {
      const uint32_t c = a.tbl_req[h];
      if (c == kNone) break;  // the probe chain of this id ends here: no request has it
      if (rq.id_len[c] == kl && wire::bytes_eq(rq.ids + rq.id_off[c], k, kl)) {
        q = a.tbl_min[h];
        break;
      }
    }
  }
  a.v.out.frame_req[f] = q;
  a.key_in[f] = q == kNone ? rq.n_reqs : q;
  a.val_in[f] = f;
}

__global__ __launch_bounds__(256) void k_env_group(EnvJoinArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t n = a.v.fr.n_frames, Q = a.v.rq.n_reqs;
  if (i <= Q) {
    uint32_t lo = 0, hi = n;  // the first sorted position whose request is i or above
#pragma unroll 1
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (a.key_out[mid] < i) lo = mid + 1;
      else hi = mid;
    }
    a.v.out.req_resp_off[i] = lo;
    if (i == Q) *a.n_resps = lo;
  }
  if (i < n && a.key_out[i] < Q) join_emit(a.v, i, a.val_out[i]);
}

// ---- encode ------------------------------------------------------------------------------
template <bool kSmall>
__global__ __launch_bounds__(kSmall ? 1024 : 256) void k_env_size(mochi_envelope_source s, uint32_t* __restrict__ msg_len,
                                                                  uint8_t* __restrict__ status,
                                                                  uint64_t* __restrict__ len64,
                                                                  uint64_t* __restrict__ off64,
                                                                  uint64_t* __restrict__ frm_off) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t M = s.n_msgs;
  uint64_t mine = 0;
  if (m < M) {
    const Sized z = size_msg(s, m);
    mine = z.prefix + z.len;
    status[m] = z.status;
    msg_len[m] = (uint32_t)z.len;
  }
  enc_place<kSmall>(m, M, mine, len64, off64, frm_off);
}

__global__ __launch_bounds__(256) void k_env_hdr(mochi_envelope_source s, const uint32_t* __restrict__ msg_len,
                                                 const uint8_t* __restrict__ status,
                                                 const uint64_t* __restrict__ frm_off,
                                                 const uint64_t* __restrict__ total, uint64_t wire_cap,
                                                 uint8_t* __restrict__ wire, uint64_t* __restrict__ msg_off,
                                                 uint64_t* __restrict__ body_dst) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= s.n_msgs) return;
  const uint32_t len = msg_len[m];
  const uint32_t prefix = s.flags & MOCHI_ENV_LENGTH_PREFIX ? wire::varint_size(len) : 0;
  msg_off[m] = frm_off[m] + prefix;
  uint64_t dst = ~0ull;
  if (*total <= wire_cap) {
    Put h(wire + frm_off[m]);
    if (prefix) h.varint(len);
    if (status[m] == MOCHI_ENC_OK) {
      const uint64_t ts = (uint64_t)s.msg_timestamp[m];
      if (ts) {
        h.byte(0x28);
        h.varint(ts);
      }
      if (const uint32_t l = len_or_0(s.server_id_off, s.server_id_len, m)) h.ld(0x32, s.ids + s.server_id_off[m], l);
      if (const uint32_t l = len_or_0(s.msg_id_off, s.msg_id_len, m)) h.ld(0x3A, s.ids + s.msg_id_off[m], l);
      if (const uint32_t l = len_or_0(s.reply_to_off, s.reply_to_len, m)) h.ld(0x42, s.ids + s.reply_to_off[m], l);
      if (const uint32_t k = s.kind[m]) {
        h.varint(payload_tag(k));
        h.varint(s.body_len[m]);
        if (s.body_len[m]) dst = (uint64_t)(h.p - wire);
      }
    }
    h.flush();
  }
  body_dst[m] = dst;
}

// blocks [0, short_blocks): 16 lanes per message, a body of at most kShortBody bytes; the
// blocks after them: one wave per message, a longer body
__global__ __launch_bounds__(256) void k_env_copy(mochi_envelope_source s, const uint64_t* __restrict__ body_dst,
                                                  uint32_t short_blocks, uint8_t* __restrict__ wire) {
  const bool small = blockIdx.x < short_blocks;
  const uint64_t t = (uint64_t)(small ? blockIdx.x : blockIdx.x - short_blocks) * blockDim.x + threadIdx.x;
  const uint64_t m = small ? t >> 4 : t >> 6;
  if (m >= s.n_msgs) return;
  const uint64_t d = body_dst[m];
  if (d == ~0ull) return;
  const uint32_t len = s.body_len[m];
  if ((len <= kShortBody) != small) return;
  const uint8_t* src = s.bodies + s.body_off[m];
  const uintptr_t d0 = (uintptr_t)(wire + d);
  if (small) {
    copy_run((uint32_t)(t & 15), d0, src, len);
    return;
  }
  const uint32_t n = run_chunks(d0, len);
#pragma unroll 1
  for (uint32_t c = threadIdx.x & 63; c < n; c += 64) copy_chunk(d0, src, len, c);
}

}  // namespace

hipError_t launch_env_decode(const EnvDecArgs& a, hipStream_t st) {
  const Stamps stamp{a.ev, st};
  hipError_t e = stamp(0);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_env_decode, dim3(cdiv(a.v.in.n_frames, 256)), dim3(256), 0, st, a.v);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return stamp(1);
}

hipError_t launch_env_route(const EnvRouteArgs& a, hipStream_t st) {
  const Stamps stamp{a.ev, st};
  hipError_t e = stamp(0);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_env_hist, dim3(a.blocks), dim3(256), 0, st, a);
  if ((e = hipGetLastError()) != hipSuccess || (e = stamp(1)) != hipSuccess) return e;
  if ((e = enc_scan64(a.scan_temp, a.scan_temp_bytes, a.hist64, a.base64, env_route_scan_n(a.blocks), st)) != hipSuccess ||
      (e = stamp(2)) != hipSuccess)
    return e;
  hipLaunchKernelGGL(k_env_scatter, dim3(a.blocks), dim3(256), 0, st, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return stamp(3);
}

hipError_t env_sort_temp_bytes(uint32_t n, int key_bits, size_t* bytes) {
  *bytes = 0;
  return hipcub::DeviceRadixSort::SortPairs(nullptr, *bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                            (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n, 0, key_bits);
}

hipError_t launch_env_join(const EnvJoinArgs& a, hipStream_t st) {
  const Stamps stamp{a.ev, st};
  const uint32_t n = a.v.fr.n_frames, Q = a.v.rq.n_reqs;
  hipError_t e = stamp(0);
  if (e != hipSuccess) return e;
  // every slot empty, every minimum "no request"
  if ((e = hipMemsetAsync(a.tbl_req, 0xFF, (size_t)((uint8_t*)(a.tbl_min + a.slots) - (uint8_t*)a.tbl_req), st)) != hipSuccess)
    return e;
  if (Q) hipLaunchKernelGGL(k_env_claim, dim3(cdiv(Q, 256)), dim3(256), 0, st, a);
  if ((e = hipGetLastError()) != hipSuccess || (e = stamp(1)) != hipSuccess) return e;
  if (n) hipLaunchKernelGGL(k_env_lookup, dim3(cdiv(n, 256)), dim3(256), 0, st, a);
  if ((e = hipGetLastError()) != hipSuccess || (e = stamp(2)) != hipSuccess) return e;
  if (n) {
    size_t bytes = a.scan_temp_bytes;
    if ((e = hipcub::DeviceRadixSort::SortPairs(a.scan_temp, bytes, (const uint32_t*)a.key_in, a.key_out,
                                                (const uint32_t*)a.val_in, a.val_out, (int)n, 0, a.key_bits, st)) != hipSuccess)
      return e;
  }
  if ((e = stamp(3)) != hipSuccess) return e;
  const uint64_t lanes = (uint64_t)(n > Q ? n : Q) + 1;
  hipLaunchKernelGGL(k_env_group, dim3(cdiv(lanes, 256)), dim3(256), 0, st, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return stamp(4);
}

hipError_t launch_env_size(const EnvEncArgs& a, hipStream_t st) {
  const uint32_t M = a.in.n_msgs;
  const Stamps stamp{a.ev, st};
  hipError_t e = stamp(0);
  if (e != hipSuccess) return e;
  if (w2_small(M)) {
    hipLaunchKernelGGL(k_env_size<true>, dim3(1), dim3(1024), 0, st, a.in, a.msg_len, a.status, a.len64, a.off64, a.frm_off);
    if ((e = stamp(1)) != hipSuccess || (e = stamp(2)) != hipSuccess) return e;
    return hipGetLastError();
  }
  hipLaunchKernelGGL(k_env_size<false>, dim3(cdiv((uint64_t)M + 1, 256)), dim3(256), 0, st, a.in, a.msg_len, a.status,
                     a.len64, a.off64, a.frm_off);
  e = hipGetLastError();
  if (e != hipSuccess || (e = stamp(1)) != hipSuccess) return e;
  e = enc_scan_offsets(a.scan_temp, a.scan_temp_bytes, a.len64, a.off64, a.frm_off, M, st);
  return e != hipSuccess ? e : stamp(2);
}

hipError_t launch_env_emit(const EnvEncArgs& a, bool copy, hipStream_t st) {
  const uint32_t M = a.in.n_msgs;
  const Stamps stamp{a.ev, st};
  hipError_t e = stamp(3);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_env_hdr, dim3(cdiv(M, 256)), dim3(256), 0, st, a.in, a.msg_len, a.status, a.frm_off, a.off64 + M,
                     a.wire_cap, a.wire, a.msg_off, a.body_dst);
  if ((e = hipGetLastError()) != hipSuccess || (e = stamp(4)) != hipSuccess) return e;
  if (copy) {
    const uint32_t short_blocks = cdiv((uint64_t)M * 16, 256), long_blocks = cdiv((uint64_t)M * 64, 256);
    hipLaunchKernelGGL(k_env_copy, dim3(short_blocks + long_blocks), dim3(256), 0, st, a.in, a.body_dst, short_blocks, a.wire);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return stamp(5);
}

}  // namespace mochi
