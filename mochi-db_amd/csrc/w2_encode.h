// w2_encode.h — launch interface between the C-ABI layer (capi.cpp) and the
// Write2ToServer wire encoder (w2_encode.hip), its host twin
// (w2_encode_host.cpp), and the size arithmetic both share.
//
// Wire layout (MochiProtocol.proto:107-147 as protobuf-java writes it, with
// INTEGRATION.md's grantSignatures map):
//   Write2ToServer  = [0A len WriteCertificate] [12 len Transaction]   (each iff non-empty)
//   WriteCertificate = { 0A len ( 0A len serverId  12 len MultiGrant ) }    per MultiGrant
//   MultiGrant      = { 0A len ( 0A len objectId  12 len Grant ) }          per grant
//                     [12 len clientId] [22 len serverId]                   (each iff non-empty)
//                     { 2A len ( 0A len objectId  12 80 02 sig[256] ) }     per grant, iff signatures
//   Transaction     = { 0A len Operation }
//   Operation       = [08 action] [12 len operand1] [1A len operand2]       (each iff non-default)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mochi_hip.h"
#include "wire_walk.h"

namespace mochi {

// sizes on wire::varint_size, the bytes of a minimal varint (wire_walk.h):
// tag (one byte: every field number here is below 16) + length varint + payload
__host__ __device__ inline uint64_t enc_ld_size(uint64_t payload) { return 1 + wire::varint_size(payload) + payload; }
// the same, omitted when empty (proto3 default)
__host__ __device__ inline uint64_t enc_ld_opt_size(uint64_t payload) { return payload ? enc_ld_size(payload) : 0; }
// body of a grants-map entry: key objectId + value Grant
__host__ __device__ inline uint64_t enc_e1_body(uint32_t oid_len, uint32_t grant_len) {
  return enc_ld_size(oid_len) + enc_ld_size(grant_len);
}
// body of a grantSignatures entry: key objectId + 256 signature bytes
__host__ __device__ inline uint64_t enc_e5_body(uint32_t oid_len) { return enc_ld_size(oid_len) + 3 + MOCHI_RSA_BYTES; }
// one Operation's body
__host__ __device__ inline uint64_t enc_op_body(uint32_t action, uint32_t l1, uint32_t l2) {
  return (action ? 1 + wire::varint_size(action) : 0) + enc_ld_opt_size(l1) + enc_ld_opt_size(l2);
}
constexpr uint64_t kEncMaxMsg = 0x7FFFFFFFull;  // a message of 2^31 bytes or more is MOCHI_ENC_TOO_LONG

// Device pointers.
struct W2EncArgs {
  mochi_write2_source src;
  const uint8_t* ids;  // server-id table
  const uint32_t* id_off;
  uint32_t n_ids;
  // outputs
  uint8_t* wire;
  uint64_t* msg_off;  // [M]
  uint32_t* msg_len;  // [M]
  uint8_t* status;    // [M]
  // scratch
  uint32_t* g_oid;      // [N][2] objectId slice of each grant (offset inside the grant, length)
  uint64_t* g_dst;      // [N][2] wire offsets of the grant's bytes and of its signature (~0 = none)
  uint64_t* mg_gpart;   // [n_mgs] bytes of the MultiGrant's grants + grantSignatures entries
  uint32_t* mg_msg;     // [n_mgs] owning message (~0 = none)
  uint32_t* mg_rel;     // [n_mgs] offset of the certificate entry inside its message
  uint8_t* mg_bad;      // [n_mgs] a grant of it does not parse
  uint32_t* msg_wc;     // [M] WriteCertificate body length
  uint32_t* msg_tx;     // [M] Transaction body length
  uint64_t* len64;      // [M+1] message lengths (scan input), last = 0
  uint64_t* off64;      // [M+1] their exclusive scan; off64[M] = the wire size
  void* scan_temp;
  size_t scan_temp_bytes;
  // per-kernel timing (mochi_ctx_set_profiling) or null: kW2EncEvents events, recorded
  // before k_enc_mg, after it, after k_enc_msg, after the scan; before k_enc_hdr_mg,
  // after it, after k_enc_hdr_msg, after k_enc_copy
  hipEvent_t* ev;
};
constexpr int kW2EncEvents = 8;
constexpr int kW2EncStages = 6;  // k_enc_mg, k_enc_msg, scan, k_enc_hdr_mg, k_enc_hdr_msg, k_enc_copy
// The per-batch scratch layout (a.src set; every array 16-byte aligned): on a null base
// it only counts and returns the bytes to allocate; on that allocation it sets a's
// scratch pointers.
size_t w2_enc_layout(W2EncArgs& a, void* base);
// temp bytes of a 64-bit device scan over n elements; one function for the three
// encoders (w2_encode.hip, w1_issue.hip, w1_reply.hip), see enc_launch.h
hipError_t enc_scan_temp_bytes(uint32_t n, size_t* bytes);
// sizes + the 64-bit exclusive scan: fills msg_off / msg_len / status and off64[M]
hipError_t launch_w2_enc_size(const W2EncArgs& a, hipStream_t stream);
// headers + payload copy (after the caller has checked off64[M] against the capacity)
hipError_t launch_w2_enc_emit(const W2EncArgs& a, hipStream_t stream);

}  // namespace mochi

namespace mochi_host {
// mochi_write2_encode without the argument checks of the C layer; `err` names
// an inconsistent input (MOCHI_EINVAL).
int write2_encode(const mochi_write2_source* s, const uint8_t* ids, const uint32_t* id_off, uint32_t n_ids,
                  uint8_t* wire, uint64_t wire_cap, uint64_t* msg_off, uint32_t* msg_len, uint8_t* status,
                  uint64_t* wire_len, const char** err);
}  // namespace mochi_host
