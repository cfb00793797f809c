// w2_encode.hip — Write2ToServer wire ENCODER on the device (gfx950): the
// inverse of w2_decode.hip.  An SoA certificate batch in HBM becomes the
// message bodies protobuf-java would write (layout: w2_encode.h), packed back
// to back with 64-bit offsets.
//
// Sizes nest (a message's length varint depends on its MultiGrants', which
// depend on their grants'), so the work goes level by level and no lane walks a
// whole message with dependent accesses:
//   k_enc_mg       lane = MultiGrant  parse each grant once (objectId slice kept), entry sizes
//   k_enc_msg      lane = message     certificate / transaction / message length, status
//   exclusive scan of the message lengths in 64 bits (hipcub; inside k_enc_msg's
//                  single block for a small batch, where w2_small draws the line)
//   k_enc_hdr_mg   lane = MultiGrant  every tag, length, map key, server id, client id of its entry
//   k_enc_hdr_msg  lane = message     top-level headers and the operations
//   k_enc_copy     16 lanes per grant the grant bytes and signatures (~90 % of the output)
// The header kernels write the short runs between the payloads (whole dwords
// where all four bytes are the lane's own, byte stores at a run's ends) and
// leave the payload bytes alone; the copy kernel writes only payload bytes.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "enc_dev.h"
#include "enc_launch.h"
#include "proto_dev.h"
#include "w2.h"
#include "w2_encode.h"

namespace mochi {
namespace {

constexpr uint64_t kNone = ~0ull;

// ---- level 1: lane = MultiGrant --------------------------------------------
__global__ __launch_bounds__(256) void k_enc_mg(mochi_write2_source s, uint32_t* __restrict__ g_oid,
                                                uint64_t* __restrict__ mg_gpart, uint8_t* __restrict__ mg_bad) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= s.n_mgs) return;
  uint64_t part = 0;
  uint32_t bad = 0;
  const uint32_t g1 = s.mg_grant_off[i + 1];
#pragma unroll 1
  for (uint32_t g = s.mg_grant_off[i]; g < g1; g++) {
    const uint64_t go = s.grant_off[g];
    const uint32_t gl = s.grant_len[g];
    uint32_t oo = 0, ol = 0;
    bool ok = go <= s.grant_bytes_len && gl <= s.grant_bytes_len - go;
    if (ok) {
      ByteReader r;
      r.init(s.grant_bytes + go, gl);
      int64_t ts;
      uint32_t ho, hl;
      ok = parse_grant(r, ts, ho, hl, oo, ol);
    }
    if (!ok) {
      bad = 1;
      continue;
    }
    g_oid[2 * (size_t)g] = oo;
    g_oid[2 * (size_t)g + 1] = ol;
    part += enc_ld_size(enc_e1_body(ol, gl));
    if (s.sig) part += enc_ld_size(enc_e5_body(ol));
  }
  mg_gpart[i] = part;
  mg_bad[i] = (uint8_t)bad;
}

// ---- level 2: lane = message -----------------------------------------------
// kSmall: one block of 1024 lanes, M < 1024; the 64-bit scan runs in the block.
template <bool kSmall>
__global__ __launch_bounds__(kSmall ? 1024 : 256) void k_enc_msg(mochi_write2_source s,
                                                                 const uint32_t* __restrict__ id_off, uint32_t n_ids,
                                                                 const uint64_t* __restrict__ mg_gpart,
                                                                 const uint8_t* __restrict__ mg_bad,
                                                                 uint32_t* __restrict__ mg_msg,
                                                                 uint32_t* __restrict__ mg_rel,
                                                                 uint32_t* __restrict__ msg_wc,
                                                                 uint32_t* __restrict__ msg_tx,
                                                                 uint32_t* __restrict__ msg_len,
                                                                 uint8_t* __restrict__ status,
                                                                 uint64_t* __restrict__ len64,
                                                                 uint64_t* __restrict__ off64,
                                                                 uint64_t* __restrict__ msg_off) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t M = s.n_msgs;
  uint64_t mine = 0;
  if (m < M) {
    const uint32_t cl = s.client_off ? s.client_len[m] : 0;
    bool bad_grant = false, bad_signer = false;
    uint64_t wc = 0, tx = 0;
    const uint32_t i1 = s.cert_mg_off[m + 1];
#pragma unroll 1
    for (uint32_t i = s.cert_mg_off[m]; i < i1; i++) {
      mg_msg[i] = m;
      mg_rel[i] = (uint32_t)wc;
      bad_grant |= mg_bad[i] != 0;
      const uint32_t sg = s.mg_signer[i];
      if (sg >= n_ids) {
        bad_signer = true;
        continue;
      }
      const uint32_t sl = id_off[sg + 1] - id_off[sg];
      const uint64_t mg = mg_gpart[i] + enc_ld_opt_size(cl) + enc_ld_opt_size(sl);
      wc += enc_ld_size(enc_ld_size(sl) + enc_ld_size(mg));
    }
    const uint32_t o1 = s.cert_op_off[m + 1];
#pragma unroll 1
    for (uint32_t o = s.cert_op_off[m]; o < o1; o++)
      tx += enc_ld_size(enc_op_body(s.op_action[o], s.op1_len[o], s.op2_off ? s.op2_len[o] : 0));
    const uint64_t len = enc_ld_opt_size(wc) + enc_ld_opt_size(tx);
    const uint8_t st = bad_grant ? MOCHI_ENC_BAD_GRANT : bad_signer ? MOCHI_ENC_BAD_SIGNER
                       : len > kEncMaxMsg ? MOCHI_ENC_TOO_LONG : MOCHI_ENC_OK;
    mine = st == MOCHI_ENC_OK ? len : 0;
    status[m] = st;
    msg_len[m] = (uint32_t)mine;
    msg_wc[m] = (uint32_t)wc;
    msg_tx[m] = (uint32_t)tx;
  }
  enc_place<kSmall>(m, M, mine, len64, off64, msg_off);
}

// ---- headers: lane = MultiGrant --------------------------------------------
__global__ __launch_bounds__(256) void k_enc_hdr_mg(mochi_write2_source s, const uint8_t* __restrict__ ids,
                                                    const uint32_t* __restrict__ id_off,
                                                    const uint32_t* __restrict__ g_oid,
                                                    const uint64_t* __restrict__ mg_gpart,
                                                    const uint32_t* __restrict__ mg_msg,
                                                    const uint32_t* __restrict__ mg_rel,
                                                    const uint32_t* __restrict__ msg_wc,
                                                    const uint64_t* __restrict__ msg_off,
                                                    const uint8_t* __restrict__ status, uint8_t* __restrict__ wire,
                                                    uint64_t* __restrict__ g_dst) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= s.n_mgs) return;
  const uint32_t m = mg_msg[i];
  if (m == 0xFFFFFFFFu || status[m] != MOCHI_ENC_OK) return;  // g_dst stays kNone: nothing to copy
  const uint32_t cl = s.client_off ? s.client_len[m] : 0;
  const uint32_t sg = s.mg_signer[i];
  const uint8_t* sid = ids + id_off[sg];
  const uint32_t sl = id_off[sg + 1] - id_off[sg];
  const uint64_t mg = mg_gpart[i] + enc_ld_opt_size(cl) + enc_ld_opt_size(sl);
  uint8_t* const base = wire + msg_off[m];
  Put o(base + 1 + wire::varint_size(msg_wc[m]) + mg_rel[i]);
  o.byte(0x0A);
  o.varint(enc_ld_size(sl) + enc_ld_size(mg));
  o.ld(0x0A, sid, sl);
  o.byte(0x12);
  o.varint(mg);
  const uint32_t g0 = s.mg_grant_off[i], g1 = s.mg_grant_off[i + 1];
#pragma unroll 1
  for (uint32_t g = g0; g < g1; g++) {
    const uint8_t* gb = s.grant_bytes + s.grant_off[g];
    const uint32_t gl = s.grant_len[g], oo = g_oid[2 * (size_t)g], ol = g_oid[2 * (size_t)g + 1];
    o.byte(0x0A);
    o.varint(enc_e1_body(ol, gl));
    o.ld(0x0A, gb + oo, ol);
    o.byte(0x12);
    o.varint(gl);
    g_dst[2 * (size_t)g] = (uint64_t)(o.p - wire);
    o.skip(gl);
  }
  if (cl) o.ld(0x12, s.strings + s.client_off[m], cl);
  if (sl) o.ld(0x22, sid, sl);
  if (s.sig) {
#pragma unroll 1
    for (uint32_t g = g0; g < g1; g++) {
      const uint8_t* gb = s.grant_bytes + s.grant_off[g];
      const uint32_t oo = g_oid[2 * (size_t)g], ol = g_oid[2 * (size_t)g + 1];
      o.byte(0x2A);
      o.varint(enc_e5_body(ol));
      o.ld(0x0A, gb + oo, ol);
      o.byte(0x12);
      o.byte(0x80);
      o.byte(0x02);
      g_dst[2 * (size_t)g + 1] = (uint64_t)(o.p - wire);
      o.skip(MOCHI_RSA_BYTES);
    }
  }
  o.flush();
}

// ---- headers: lane = message (top level + the operations) -------------------
__global__ __launch_bounds__(256) void k_enc_hdr_msg(mochi_write2_source s, const uint32_t* __restrict__ msg_wc,
                                                     const uint32_t* __restrict__ msg_tx,
                                                     const uint64_t* __restrict__ msg_off,
                                                     const uint8_t* __restrict__ status, uint8_t* __restrict__ wire) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= s.n_msgs || status[m] != MOCHI_ENC_OK) return;
  Put o(wire + msg_off[m]);
  const uint32_t wc = msg_wc[m], tx = msg_tx[m];
  if (wc) {
    o.byte(0x0A);
    o.varint(wc);
    o.skip(wc);
  }
  if (!tx) return;
  o.byte(0x12);
  o.varint(tx);
  const uint32_t q1 = s.cert_op_off[m + 1];
#pragma unroll 1
  for (uint32_t q = s.cert_op_off[m]; q < q1; q++) {
    const uint32_t act = s.op_action[q], l1 = s.op1_len[q], l2 = s.op2_off ? s.op2_len[q] : 0;
    o.byte(0x0A);
    o.varint(enc_op_body(act, l1, l2));
    if (act) {
      o.byte(0x08);
      o.varint(act);
    }
    if (l1) o.ld(0x12, s.strings + s.op1_off[q], l1);
    if (l2) o.ld(0x1A, s.strings + s.op2_off[q], l2);
  }
  o.flush();
}

// ---- payload copy (enc_dev.h copy_chunk) --------------------------------------

// 16 lanes per grant: its bytes, then its signature, as one list of chunks
__global__ __launch_bounds__(256) void k_enc_copy(mochi_write2_source s, const uint64_t* __restrict__ g_dst,
                                                  uint8_t* __restrict__ wire) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t g = t >> 4;
  const uint32_t q = (uint32_t)(t & 15);
  if (g >= s.n_grants) return;
  const uint64_t dg = g_dst[2 * g], ds = g_dst[2 * g + 1];
  if (dg == kNone) return;  // a grant of no emitted message
  const uint32_t c = copy_run(q, (uintptr_t)(wire + dg), s.grant_bytes + s.grant_off[g], s.grant_len[g]);
  if (ds == kNone) return;
  copy_run(c, (uintptr_t)(wire + ds), s.sig + (size_t)MOCHI_RSA_BYTES * g, MOCHI_RSA_BYTES);
}

}  // namespace

size_t w2_enc_layout(W2EncArgs& a, void* base) {
  const size_t m1 = (size_t)a.src.n_msgs + 1, nm = a.src.n_mgs, n = a.src.n_grants;
  Carve c(base);
  a.g_dst = c.take<uint64_t>(2 * n);  // g_dst and mg_msg adjacent: one fill (launch_w2_enc_size)
  a.mg_msg = c.take<uint32_t>(nm);
  a.g_oid = c.take<uint32_t>(2 * n);
  a.mg_gpart = c.take<uint64_t>(nm);
  a.mg_rel = c.take<uint32_t>(nm);
  a.mg_bad = c.take<uint8_t>(nm);
  a.msg_wc = c.take<uint32_t>(m1);
  a.msg_tx = c.take<uint32_t>(m1);
  a.len64 = c.take<uint64_t>(m1);
  a.off64 = c.take<uint64_t>(m1);
  return c.bytes();
}

// declared in w2_encode.h for capi.cpp, which cannot include hipcub
hipError_t enc_scan_temp_bytes(uint32_t n, size_t* bytes) {
  return hipcub::DeviceScan::ExclusiveSum(nullptr, *bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (int)n);
}

hipError_t launch_w2_enc_size(const W2EncArgs& a, hipStream_t st) {
  const mochi_write2_source& s = a.src;
  const uint32_t M = s.n_msgs;
  const Stamps stamp{a.ev, st};
  hipError_t e = stamp(0);
  if (e != hipSuccess) return e;
  // "no destination" / "no message" until the header kernels say otherwise
  const size_t fill = (size_t)((uint8_t*)(a.mg_msg + s.n_mgs) - (uint8_t*)a.g_dst);
  if (fill && (e = hipMemsetAsync(a.g_dst, 0xFF, fill, st)) != hipSuccess) return e;
  if (s.n_mgs) hipLaunchKernelGGL(k_enc_mg, dim3(cdiv(s.n_mgs, 256)), dim3(256), 0, st, s, a.g_oid, a.mg_gpart, a.mg_bad);
  if ((e = stamp(1)) != hipSuccess) return e;
  if (w2_small(M)) {
    hipLaunchKernelGGL(k_enc_msg<true>, dim3(1), dim3(1024), 0, st, s, a.id_off, a.n_ids, a.mg_gpart, a.mg_bad, a.mg_msg,
                       a.mg_rel, a.msg_wc, a.msg_tx, a.msg_len, a.status, a.len64, a.off64, a.msg_off);
    if ((e = stamp(2)) != hipSuccess || (e = stamp(3)) != hipSuccess) return e;
    return hipGetLastError();
  }
  hipLaunchKernelGGL(k_enc_msg<false>, dim3(cdiv((uint64_t)M + 1, 256)), dim3(256), 0, st, s, a.id_off, a.n_ids,
                     a.mg_gpart, a.mg_bad, a.mg_msg, a.mg_rel, a.msg_wc, a.msg_tx, a.msg_len, a.status, a.len64,
                     a.off64, a.msg_off);
  e = hipGetLastError();
  if (e != hipSuccess || (e = stamp(2)) != hipSuccess) return e;
  e = enc_scan_offsets(a.scan_temp, a.scan_temp_bytes, a.len64, a.off64, a.msg_off, M, st);
  return e != hipSuccess ? e : stamp(3);
}

hipError_t launch_w2_enc_emit(const W2EncArgs& a, hipStream_t st) {
  const mochi_write2_source& s = a.src;
  const Stamps stamp{a.ev, st};
  hipError_t e = stamp(4);
  if (e != hipSuccess) return e;
  if (s.n_mgs)
    hipLaunchKernelGGL(k_enc_hdr_mg, dim3(cdiv(s.n_mgs, 256)), dim3(256), 0, st, s, a.ids, a.id_off, a.g_oid, a.mg_gpart,
                       a.mg_msg, a.mg_rel, a.msg_wc, a.msg_off, a.status, a.wire, a.g_dst);
  if ((e = stamp(5)) != hipSuccess) return e;
  if (s.n_msgs)
    hipLaunchKernelGGL(k_enc_hdr_msg, dim3(cdiv(s.n_msgs, 256)), dim3(256), 0, st, s, a.msg_wc, a.msg_tx, a.msg_off,
                       a.status, a.wire);
  if ((e = stamp(6)) != hipSuccess) return e;
  if (s.n_grants)
    hipLaunchKernelGGL(k_enc_copy, dim3(cdiv((uint64_t)s.n_grants * 16, 256)), dim3(256), 0, st, s, a.g_dst, a.wire);
  e = hipGetLastError();
  return e != hipSuccess ? e : stamp(7);
}

}  // namespace mochi
