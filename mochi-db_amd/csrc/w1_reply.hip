// w1_reply.hip — Write1 reply ENCODER on the device (gfx950): the
// Write1OkFromServer / Write1RefusedFromServer bodies of a batch, from the
// arrays mochi_write1_issue_device left in HBM (layout: w1_reply.h), packed
// back to back with 64-bit offsets.  Built like w2_encode.hip, level by level:
//   k_w1r_size   lane = request     per req_grant entry the first listed op that refers to it
//                                   (kept in ent_op); MultiGrant / message length, status
//   exclusive scan of the message lengths in 64 bits (hipcub; inside k_w1r_size's
//                single block for a small batch, where w2_small draws the line)
//   k_w1r_hdr    lane = request     every tag, length, map key, client id and server id;
//                                   per entry where its three payloads go (ent_dst)
//   k_w1r_copy   the payloads: 16 lanes per entry for the grant bytes and the signature
//                (k_enc_copy's split), one wave per entry for the certificate
// A certificate is ~2.9 KB at R = 4 (182 destination chunks of 16 bytes) against
// ~150 B of grant and 256 B of signature, so it gets 64 lanes: three rounds of
// one dwordx4 store per lane, every round a contiguous 1 KiB of the wire, where
// 16 lanes would loop twelve times.  The two roles are block ranges of one
// launch (no kernel boundary between them, no divergence inside a block).
// The header kernel leaves the payload bytes alone; the copy kernel writes only
// payload bytes (enc_dev.h).  Both read the scanned total first and write
// nothing when it exceeds wire_cap: the capacity rule without a host wait.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "enc_dev.h"
#include "enc_launch.h"
#include "w1_reply.h"
#include "w2.h"

namespace mochi {
namespace {

constexpr uint64_t kNone = ~0ull;
constexpr uint32_t kNoOp = 0xFFFFFFFFu;

// the grant a reference names: length and (src != null) address; a reference outside
// n_new / n_stored (the host form refuses it) reads as an empty grant
__device__ __forceinline__ uint32_t ref_grant(const mochi_write1_issued& o, const mochi_write1_reply_source& s,
                                              uint32_t n_stored, uint32_t r, const uint8_t** src,
                                              const uint8_t** sig) {
  if (r & MOCHI_W1_STORED) {
    const uint32_t i = r & ~MOCHI_W1_STORED;
    if (i >= n_stored) return 0;
    if (src) *src = s.stored_bytes + s.stored_off[i];
    if (sig) *sig = s.stored_sig + (size_t)MOCHI_RSA_BYTES * i;
    return s.stored_len[i];
  }
  if (r >= o.n_new) return 0;
  if (src) *src = o.grant_bytes + o.grant_off[r];
  if (sig) *sig = o.sig + (size_t)MOCHI_RSA_BYTES * r;
  return o.grant_len[r];
}

// ---- sizes: lane = request ----------------------------------------------------
// kSmall: one block of 1024 lanes, Q < 1024; the 64-bit scan runs in the block.
template <bool kSmall>
__global__ __launch_bounds__(kSmall ? 1024 : 256) void k_w1r_size(mochi_write1_batch b, mochi_write1_issued o,
                                                                  mochi_write1_reply_source s,
                                                                  uint32_t* __restrict__ ent_op,
                                                                  uint32_t* __restrict__ req_mg,
                                                                  uint32_t* __restrict__ msg_len,
                                                                  uint8_t* __restrict__ status,
                                                                  uint64_t* __restrict__ len64,
                                                                  uint64_t* __restrict__ off64,
                                                                  uint64_t* __restrict__ msg_off) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t Q = b.n_reqs;
  uint64_t mine = 0;
  if (q < Q) {
    const uint8_t kind = o.req_kind[q];
    const uint32_t o0 = b.req_op_off[q], o1 = b.req_op_off[q + 1];
    const uint32_t e1 = o.req_grant_off[q + 1];
    const bool with_sig = o.sig != nullptr;
    uint64_t part = 0, certs = 0;
#pragma unroll 1
    for (uint32_t e = o.req_grant_off[q]; e < e1; e++) {
      const uint32_t r = o.req_grant[e];
      uint32_t op = o0;
#pragma unroll 1
      while (op < o1 && !(o.op_grant[op] == r && w1r_listed(kind, o.op_decision[op]))) op++;
      if (op == o1) op = kNoOp;  // the host form refuses this batch; here the entry has no key and no certificate
      ent_op[e] = op;
      const uint32_t kl = op != kNoOp ? b.op_key_len[op] : 0;
      const uint32_t cl = op != kNoOp && s.op_cert_off ? s.op_cert_len[op] : 0;
      part += w1r_mg_entry(kl, ref_grant(o, s, b.n_stored, r, nullptr, nullptr), with_sig);
      certs += w1r_cert_entry(kl, cl);
    }
    uint8_t st = MOCHI_ENC_OK;
    uint64_t mg = 0;
    if (kind == MOCHI_W1K_OK || kind == MOCHI_W1K_REFUSED) {
      mg = w1r_mg_body(part, s.req_client_off ? s.req_client_len[q] : 0, s.server_id_len);
      mine = w1r_msg_len(mg, certs);
      if (mine > kEncMaxMsg) {
        st = MOCHI_ENC_TOO_LONG;
        mine = 0;
      }
    }
    status[q] = st;
    msg_len[q] = (uint32_t)mine;
    req_mg[q] = (uint32_t)mg;
  }
  enc_place<kSmall>(q, Q, mine, len64, off64, msg_off);
}

// ---- headers: lane = request ----------------------------------------------------
__global__ __launch_bounds__(256) void k_w1r_hdr(mochi_write1_batch b, mochi_write1_issued o,
                                                 mochi_write1_reply_source s, const uint32_t* __restrict__ ent_op,
                                                 const uint32_t* __restrict__ req_mg,
                                                 const uint32_t* __restrict__ msg_len,
                                                 const uint64_t* __restrict__ msg_off,
                                                 const uint64_t* __restrict__ total, uint64_t wire_cap,
                                                 uint8_t* __restrict__ wire, uint64_t* __restrict__ ent_dst) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= b.n_reqs) return;
  const uint32_t e0 = o.req_grant_off[q], e1 = o.req_grant_off[q + 1];
  const uint8_t kind = o.req_kind[q];
  const uint32_t len = msg_len[q];
  // a THROWS request has no body; a request with a body has at least the two bytes 0A 00
  if (*total > wire_cap || !(kind == MOCHI_W1K_OK || kind == MOCHI_W1K_REFUSED) || len == 0) {
#pragma unroll 1
    for (uint64_t e = e0; e < e1; e++) ent_dst[3 * e] = ent_dst[3 * e + 1] = ent_dst[3 * e + 2] = kNone;
    return;
  }
  const bool with_sig = o.sig != nullptr;
  Put p(wire + msg_off[q]);
  p.byte(0x0A);
  p.varint(req_mg[q]);
#pragma unroll 1
  for (uint64_t e = e0; e < e1; e++) {
    const uint32_t op = ent_op[e];
    const uint32_t kl = op != kNoOp ? b.op_key_len[op] : 0;
    const uint32_t gl = ref_grant(o, s, b.n_stored, o.req_grant[e], nullptr, nullptr);
    p.byte(0x0A);
    p.varint(enc_e1_body(kl, gl));
    p.ld(0x0A, kl ? b.strings + b.op_key_off[op] : nullptr, kl);
    p.byte(0x12);
    p.varint(gl);
    ent_dst[3 * e] = gl ? (uint64_t)(p.p - wire) : kNone;
    p.skip(gl);
  }
  const uint32_t cl = s.req_client_off ? s.req_client_len[q] : 0;
  if (cl) p.ld(0x12, s.ids + s.req_client_off[q], cl);
  if (s.server_id_len) p.ld(0x22, s.ids + s.server_id_off, s.server_id_len);
#pragma unroll 1
  for (uint64_t e = e0; e < e1; e++) {
    if (!with_sig) {
      ent_dst[3 * e + 1] = kNone;
      continue;
    }
    const uint32_t op = ent_op[e];
    const uint32_t kl = op != kNoOp ? b.op_key_len[op] : 0;
    p.byte(0x2A);
    p.varint(enc_e5_body(kl));
    p.ld(0x0A, kl ? b.strings + b.op_key_off[op] : nullptr, kl);
    p.byte(0x12);
    p.byte(0x80);
    p.byte(0x02);
    ent_dst[3 * e + 1] = (uint64_t)(p.p - wire);
    p.skip(MOCHI_RSA_BYTES);
  }
#pragma unroll 1
  for (uint64_t e = e0; e < e1; e++) {
    const uint32_t op = ent_op[e];
    const uint32_t cert = op != kNoOp && s.op_cert_off ? s.op_cert_len[op] : 0;
    if (!cert) {
      ent_dst[3 * e + 2] = kNone;
      continue;
    }
    const uint32_t kl = b.op_key_len[op];
    p.byte(0x12);
    p.varint(w1r_cert_body(kl, cert));
    p.ld(0x0A, kl ? b.strings + b.op_key_off[op] : nullptr, kl);
    p.byte(0x12);
    p.varint(cert);
    ent_dst[3 * e + 2] = (uint64_t)(p.p - wire);
    p.skip(cert);
  }
  p.flush();
}

// ---- payload copy (enc_dev.h copy_chunk) ------------------------------------------
// blocks [0, small_blocks): 16 lanes per entry, its grant bytes then its signature as one
// list of chunks; the blocks after them: one wave per entry, its certificate
__global__ __launch_bounds__(256) void k_w1r_copy(mochi_write1_batch b, mochi_write1_issued o,
                                                  mochi_write1_reply_source s, const uint32_t* __restrict__ ent_op,
                                                  const uint64_t* __restrict__ ent_dst,
                                                  const uint64_t* __restrict__ total, uint64_t wire_cap,
                                                  uint32_t small_blocks, uint8_t* __restrict__ wire) {
  if (*total > wire_cap) return;
  const uint64_t n_ent = o.req_grant_off[b.n_reqs];
  if (blockIdx.x < small_blocks) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t e = t >> 4;
    const uint32_t l = (uint32_t)(t & 15);
    if (e >= n_ent) return;
    const uint64_t dg = ent_dst[3 * e], ds = ent_dst[3 * e + 1];
    const uint8_t *src = nullptr, *sig = nullptr;
    const uint32_t gl = ref_grant(o, s, b.n_stored, o.req_grant[e], &src, &sig);
    uint32_t c = l;
    if (dg != kNone && gl) c = copy_run(c, (uintptr_t)(wire + dg), src, gl);
    if (ds == kNone || !sig) return;
    copy_run(c, (uintptr_t)(wire + ds), sig, MOCHI_RSA_BYTES);
    return;
  }
  const uint64_t e = ((uint64_t)(blockIdx.x - small_blocks) * blockDim.x + threadIdx.x) >> 6;
  if (e >= n_ent) return;
  const uint64_t dc = ent_dst[3 * e + 2];
  if (dc == kNone) return;
  const uint32_t op = ent_op[e];
  const uint32_t cl = s.op_cert_len[op];  // dc is set: the op exists and certificates are given
  const uint8_t* cert = s.certs + s.op_cert_off[op];
  const uintptr_t d0 = (uintptr_t)(wire + dc);
  const uint32_t n = run_chunks(d0, cl);
#pragma unroll 1
  for (uint32_t c = threadIdx.x & 63; c < n; c += 64) copy_chunk(d0, cert, cl, c);
}

}  // namespace

size_t w1r_layout(W1ReplyArgs& a, void* base) {
  const size_t q1 = (size_t)a.b.n_reqs + 1, n = a.b.n_ops;
  Carve c(base);
  a.ent_op = c.take<uint32_t>(n);
  a.ent_dst = c.take<uint64_t>(3 * n);
  a.req_mg = c.take<uint32_t>(q1);
  a.len64 = c.take<uint64_t>(q1);
  a.off64 = c.take<uint64_t>(q1);
  return c.bytes();
}

hipError_t launch_w1r_size(const W1ReplyArgs& a, hipStream_t st) {
  const uint32_t Q = a.b.n_reqs;
  const Stamps stamp{a.ev, st};
  hipError_t e = stamp(0);
  if (e != hipSuccess) return e;
  if (w2_small(Q)) {
    hipLaunchKernelGGL(k_w1r_size<true>, dim3(1), dim3(1024), 0, st, a.b, a.o, a.src, a.ent_op, a.req_mg, a.msg_len,
                       a.status, a.len64, a.off64, a.msg_off);
    if ((e = stamp(1)) != hipSuccess || (e = stamp(2)) != hipSuccess) return e;
    return hipGetLastError();
  }
  hipLaunchKernelGGL(k_w1r_size<false>, dim3(cdiv((uint64_t)Q + 1, 256)), dim3(256), 0, st, a.b, a.o, a.src, a.ent_op,
                     a.req_mg, a.msg_len, a.status, a.len64, a.off64, a.msg_off);
  e = hipGetLastError();
  if (e != hipSuccess || (e = stamp(1)) != hipSuccess) return e;
  e = enc_scan_offsets(a.scan_temp, a.scan_temp_bytes, a.len64, a.off64, a.msg_off, Q, st);
  return e != hipSuccess ? e : stamp(2);
}

hipError_t launch_w1r_emit(const W1ReplyArgs& a, hipStream_t st) {
  const uint32_t Q = a.b.n_reqs, O = a.b.n_ops;
  const uint64_t* total = a.off64 + Q;
  const Stamps stamp{a.ev, st};
  hipError_t e = stamp(3);
  if (e != hipSuccess) return e;
  if (Q)
    hipLaunchKernelGGL(k_w1r_hdr, dim3(cdiv(Q, 256)), dim3(256), 0, st, a.b, a.o, a.src, a.ent_op, a.req_mg, a.msg_len,
                       a.msg_off, total, a.wire_cap, a.wire, a.ent_dst);
  if ((e = stamp(4)) != hipSuccess) return e;
  if (O) {
    // the number of entries is known on the device only (req_grant_off[Q] <= O)
    const uint32_t small_blocks = cdiv((uint64_t)O * 16, 256);
    const uint32_t cert_blocks = a.src.op_cert_off ? cdiv((uint64_t)O * 64, 256) : 0;
    hipLaunchKernelGGL(k_w1r_copy, dim3(small_blocks + cert_blocks), dim3(256), 0, st, a.b, a.o, a.src, a.ent_op,
                       a.ent_dst, total, a.wire_cap, small_blocks, a.wire);
  }
  e = hipGetLastError();
  return e != hipSuccess ? e : stamp(5);
}

}  // namespace mochi
