// w1_reply.h — launch interface between the C-ABI layer (capi.cpp) and the
// Write1 reply encoder (w1_reply.hip), its host twin (w1_reply_host.cpp), and
// the size arithmetic both share.  Semantics: include/mochi_hip.h
// (mochi_write1_reply_source).
//
// Wire layout (MochiProtocol.proto:117-161 as protobuf-java writes it, with
// INTEGRATION.md's grantSignatures map; InMemoryDataStore.java:283-308):
//   Write1OkFromServer / Write1RefusedFromServer
//     = 0A len MultiGrant                                        always, also when the body is empty (0A 00)
//       { 12 len ( 0A len objectId  12 len WriteCertificate ) }  per listed grant whose container has a currentC
//   MultiGrant = { 0A len ( 0A len objectId  12 len Grant ) }    per listed grant
//                [12 len clientId] [22 len serverId]             (each iff non-empty)
//                { 2A len ( 0A len objectId  12 80 02 sig[256] ) }  per listed grant, iff signatures
//   RequestFailedFromServer{OLD_REQUEST} = empty body
// The listed grants of request q are req_grant[req_grant_off[q] .. req_grant_off[q+1]);
// the map key and the certificate of an entry are those of the first listed op
// of the request that refers to the grant.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mochi_hip.h"
#include "w2_encode.h"

namespace mochi {

// is op decision d part of the reply of a request of this kind (w1_issue.hip listed())
__host__ __device__ inline bool w1r_listed(uint8_t kind, uint8_t d) {
  return kind == MOCHI_W1K_OK ? d == MOCHI_W1D_NEW || d == MOCHI_W1D_RETRY || d == MOCHI_W1D_WRONG_SHARD
                              : kind == MOCHI_W1K_REFUSED && d == MOCHI_W1D_REFUSED;
}
// bytes one listed grant adds to the MultiGrant body: its grants entry and, with signatures, its grantSignatures entry
__host__ __device__ inline uint64_t w1r_mg_entry(uint32_t key_len, uint32_t grant_len, bool with_sig) {
  return enc_ld_size(enc_e1_body(key_len, grant_len)) + (with_sig ? enc_ld_size(enc_e5_body(key_len)) : 0);
}
// body of a currentCertificates entry: key objectId + value WriteCertificate
__host__ __device__ inline uint64_t w1r_cert_body(uint32_t key_len, uint32_t cert_len) {
  return enc_ld_size(key_len) + enc_ld_size(cert_len);
}
// bytes one listed grant adds after the MultiGrant: its currentCertificates entry (none without a certificate)
__host__ __device__ inline uint64_t w1r_cert_entry(uint32_t key_len, uint32_t cert_len) {
  return cert_len ? enc_ld_size(w1r_cert_body(key_len, cert_len)) : 0;
}
// MultiGrant body from the sum of its entries
__host__ __device__ inline uint64_t w1r_mg_body(uint64_t entries, uint32_t client_len, uint32_t server_len) {
  return entries + enc_ld_opt_size(client_len) + enc_ld_opt_size(server_len);
}
// the message: multiGrant is always present
__host__ __device__ inline uint64_t w1r_msg_len(uint64_t mg_body, uint64_t cert_entries) {
  return enc_ld_size(mg_body) + cert_entries;
}

// Device pointers.
struct W1ReplyArgs {
  mochi_write1_batch b;
  mochi_write1_issued o;  // n_new as the issue call left it
  mochi_write1_reply_source src;
  // outputs
  uint8_t* wire;
  uint64_t wire_cap;
  uint64_t* msg_off;  // [Q]
  uint32_t* msg_len;  // [Q]
  uint8_t* status;    // [Q]
  // scratch
  uint32_t* ent_op;    // [O] per req_grant entry: the first listed op of its request that refers to it (~0 = none)
  uint64_t* ent_dst;   // [O][3] wire offsets of the entry's grant bytes, signature and certificate (~0 = none)
  uint32_t* req_mg;    // [Q+1] MultiGrant body length
  uint64_t* len64;     // [Q+1] message lengths (scan input), last = 0
  uint64_t* off64;     // [Q+1] their exclusive scan; off64[Q] = the wire size
  void* scan_temp;
  size_t scan_temp_bytes;
  // per-kernel timing or null: kW1ReplyEvents events, recorded before k_w1r_size,
  // after it, after the scan; before k_w1r_hdr, after it, after k_w1r_copy
  hipEvent_t* ev;
};
constexpr int kW1ReplyEvents = 6;
constexpr int kW1ReplyStages = 4;  // k_w1r_size, scan, k_w1r_hdr, k_w1r_copy
// The per-call scratch layout (a.b set; every array 16-byte aligned): on a null base it
// only counts and returns the bytes to allocate; on that allocation it sets a's
// scratch pointers.
size_t w1r_layout(W1ReplyArgs& a, void* base);
// sizes + the 64-bit exclusive scan: fills msg_off / msg_len / status and off64[Q]
hipError_t launch_w1r_size(const W1ReplyArgs& a, hipStream_t stream);
// headers + payload copy; every kernel writes nothing when off64[Q] > wire_cap
hipError_t launch_w1r_emit(const W1ReplyArgs& a, hipStream_t stream);

}  // namespace mochi

namespace mochi_host {
// mochi_write1_reply_encode without the null checks of the C layer; `err` names
// an inconsistent input (MOCHI_EINVAL).
int write1_reply_encode(const mochi_write1_batch* b, const mochi_write1_issued* o, const mochi_write1_reply_source* s,
                        uint8_t* wire, uint64_t wire_cap, uint64_t* msg_off, uint32_t* msg_len, uint8_t* status,
                        uint64_t* wire_len, const char** err);
}  // namespace mochi_host
