// w1_issue.h — launch interface between the C-ABI layer (capi.cpp) and the
// Write1 grant issuance (w1_issue.hip), its host twin (w1_issue_host.cpp), and
// the size arithmetic both share.  Semantics: include/mochi_hip.h
// (mochi_write1_batch).
//
// Grant wire layout (MochiProtocol.proto Grant as protobuf-java writes it,
// proto3 defaults omitted, fields in number order):
//   [0A len objectId] [10 varint timestamp] [22 len transactionHash] [28 varint status]
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mochi_hip.h"
#include "w2_encode.h"

namespace mochi {

constexpr uint32_t kW1WrongShard = 1;  // OperationResultStatus.WRONG_SHARD

// ts = epoch + seed as Java adds a long and an int widened from an unsigned seed: wrapping
__host__ __device__ inline int64_t w1_ts(int64_t epoch, uint32_t seed) { return (int64_t)((uint64_t)epoch + seed); }
// bytes of a new Grant (the key is never empty: an empty key FAILED)
__host__ __device__ inline uint64_t w1_grant_size(uint32_t key_len, uint32_t hash_len, int64_t ts, bool wrong_shard) {
  return enc_ld_size(key_len) + (wrong_shard || ts == 0 ? 0 : 1 + wire::varint_size((uint64_t)ts)) +
         enc_ld_opt_size(hash_len) + (wrong_shard ? 2 : 0);
}
// slots of the claim table: a power of two >= 2 * n_ops (load factor <= 1/2)
inline uint64_t w1_table_slots(uint32_t n_ops) {
  uint64_t c = 16;
  while (c < 2 * (uint64_t)n_ops) c <<= 1;
  return c;
}

// Device pointers.
struct W1Args {
  mochi_write1_batch b;
  mochi_write1_issued o;
  // scratch
  uint64_t* tbl_key;   // [slots] (op_obj << 32 | seed), ~0 = empty
  uint32_t* tbl_val;   // [slots] smallest op index that reached the slot
  uint32_t slots;      // w1_table_slots(n_ops)
  uint32_t* op_req;    // [O] owning request
  uint8_t* op_dead;    // [O] an earlier WRITE / DELETE op of the request had an empty key
  uint32_t* op_ref;    // [O] the op whose new grant this op refers to, MOCHI_W1_STORED | index, or NONE
  uint64_t* cnt64;     // [O+1] 1 where the op makes a grant; last = 0
  uint64_t* len64;     // [O+1] that grant's size; last = 0
  uint64_t* ref64;     // [Q+1] grant references in the request's reply; last = 0
  uint64_t* cnt_off;   // [O+1] exclusive scans; cnt_off[O] = n_new, len_off[O] = the byte total
  uint64_t* len_off;   // [O+1]
  uint64_t* ref_off;   // [Q+1]
  uint64_t* totals;    // [2] n_new, byte total (copied to the host)
  void* scan_temp;
  size_t scan_temp_bytes;
  // per-kernel timing or null: kW1Events events, recorded before k_w1_pre (with
  // the table clear), after it, after k_w1_claim, k_w1_decide, k_w1_reply
  // (count), the scans; before k_w1_emit, after it, after k_w1_reply (write)
  hipEvent_t* ev;
};
constexpr int kW1Events = 10;  // the last one is recorded by the caller after signing
constexpr int kW1Stages = 8;
// The per-call scratch layout (a.b and a.slots set; every array 16-byte aligned): on a
// null base it only counts and returns the bytes to allocate; on that allocation it
// sets a's scratch pointers.
size_t w1_layout(W1Args& a, void* base);
// decisions, kinds, reply sizes and the scans: fills op_decision / req_kind /
// req_grant_off and totals[2]
hipError_t launch_w1_decide(const W1Args& a, hipStream_t stream);
// grant bytes and every remaining output (after the caller has checked totals
// against the capacity)
hipError_t launch_w1_emit(const W1Args& a, hipStream_t stream);

}  // namespace mochi

namespace mochi_host {
// mochi_write1_issue without the argument checks of the C layer; `err` names
// an inconsistent input (MOCHI_EINVAL).
int write1_issue(const mochi_write1_batch* b, mochi_write1_issued* out, const char** err);
}  // namespace mochi_host
