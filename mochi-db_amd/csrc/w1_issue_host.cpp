// w1_issue_host.cpp — the host form of Write1 grant issuance
// (mochi_write1_issue): plain C++, no GPU, no key.  It is the CPU twin of
// w1_issue.hip (same decisions, numbering, views and bytes; sizes through
// w1_issue.h) and walks the batch the way the reference walks one request
// after another (InMemoryDataStore.java:105-155, :233-310).
#include <cstdint>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "w1_issue.h"
#include "wire_put.h"

namespace mochi_host {

int write1_issue(const mochi_write1_batch* b, mochi_write1_issued* out, const char** err) {
  using namespace mochi;
  const uint32_t Q = b->n_reqs, O = b->n_ops, S = b->n_stored;
  auto bad = [&](const char* what) {
    *err = what;
    return MOCHI_EINVAL;
  };
  constexpr uint8_t kWD = MOCHI_W1OP_WRITE | MOCHI_W1OP_DELETE, kHeld = MOCHI_W1OP_LOCAL | MOCHI_W1OP_HAS_SVOC;
  if (b->req_op_off[0] != 0 || b->req_op_off[Q] != O) return bad("req_op_off is not a CSR over n_ops");
  for (uint32_t q = 0; q < Q; q++) {
    if (b->req_op_off[q + 1] < b->req_op_off[q]) return bad("req_op_off is not a CSR over n_ops");
    if (b->req_op_off[q + 1] - b->req_op_off[q] > MOCHI_MAX_OPS_PER_CERT)
      return bad("a request has more than MOCHI_MAX_OPS_PER_CERT ops");
  }
  auto in_strings = [&](uint64_t off, uint32_t len) { return inside(off, len, b->strings_len); };
  for (uint32_t q = 0; q < Q; q++)
    if (!in_strings(b->req_hash_off[q], b->req_hash_len[q])) return bad("a transactionHash lies outside strings");
  for (uint32_t s = 0; s < S; s++)
    if (!in_strings(b->stored_hash_off[s], b->stored_hash_len[s])) return bad("a stored hash lies outside strings");
  std::unordered_map<uint32_t, int64_t> epoch_of;
  for (uint32_t o = 0; o < O; o++) {
    if (!in_strings(b->op_key_off[o], b->op_key_len[o])) return bad("a key lies outside strings");
    if ((b->op_flags[o] & kHeld) != kHeld) continue;
    if (b->op_stored[o] != MOCHI_W1_NONE && b->op_stored[o] >= S) return bad("an op_stored index is outside n_stored");
    if (b->op_obj[o] == 0xFFFFFFFFu) return bad("op_obj 0xFFFFFFFF is reserved");
    const auto it = epoch_of.emplace(b->op_obj[o], b->op_epoch[o]).first;
    if (it->second != b->op_epoch[o]) return bad("equal op_obj with different op_epoch");
  }

  auto hash_eq = [&](uint64_t ao, uint32_t al, uint64_t bo, uint32_t bl) {
    return al == bl && (al == 0 || memcmp(b->strings + ao, b->strings + bo, al) == 0);
  };
  // one request after another, its ops in order
  std::vector<uint32_t> op_req(O), op_ref(O, MOCHI_W1_NONE);
  std::vector<uint8_t> makes(O, 0);
  std::unordered_map<uint64_t, uint32_t> given;  // (object, seed) -> the op that took the free slot
  for (uint32_t q = 0; q < Q; q++) {
    bool dead = false;
    const uint32_t o0 = b->req_op_off[q], o1 = b->req_op_off[q + 1];
    for (uint32_t o = o0; o < o1; o++) {
      op_req[o] = q;
      const uint8_t f = b->op_flags[o];
      uint8_t d;
      if (!(f & kWD)) {
        d = MOCHI_W1D_SKIP;
      } else if (dead) {
        d = MOCHI_W1D_SKIPPED;
      } else if (b->op_key_len[o] == 0) {
        d = MOCHI_W1D_FAILED;
        dead = true;
      } else if (!(f & MOCHI_W1OP_LOCAL)) {
        d = MOCHI_W1D_WRONG_SHARD;
        op_ref[o] = o;
        for (uint32_t e = o0; e < o; e++)
          if (out->op_decision[e] == MOCHI_W1D_WRONG_SHARD &&
              hash_eq(b->op_key_off[e], b->op_key_len[e], b->op_key_off[o], b->op_key_len[o])) {
            op_ref[o] = op_ref[e];
            break;
          }
        makes[o] = op_ref[o] == o;
      } else if (!(f & MOCHI_W1OP_HAS_SVOC)) {
        d = MOCHI_W1D_FAILED;
      } else if (b->op_stored[o] != MOCHI_W1_NONE) {
        const uint32_t s = b->op_stored[o];
        d = hash_eq(b->req_hash_off[q], b->req_hash_len[q], b->stored_hash_off[s], b->stored_hash_len[s])
                ? MOCHI_W1D_RETRY : MOCHI_W1D_REFUSED;
        op_ref[o] = MOCHI_W1_STORED | s;
      } else {
        const auto ins = given.emplace((uint64_t)b->op_obj[o] << 32 | b->req_seed[q], o);
        const uint32_t w = ins.first->second;
        op_ref[o] = w;
        if (ins.second) {
          d = MOCHI_W1D_NEW;
          makes[o] = 1;
        } else {
          const uint32_t qw = op_req[w];
          d = hash_eq(b->req_hash_off[q], b->req_hash_len[q], b->req_hash_off[qw], b->req_hash_len[qw])
                  ? MOCHI_W1D_RETRY : MOCHI_W1D_REFUSED;
        }
      }
      out->op_decision[o] = d;
    }
  }
  // kinds and reply sizes
  auto listed = [&](uint8_t kind, uint8_t d) {
    return kind == MOCHI_W1K_OK ? d == MOCHI_W1D_NEW || d == MOCHI_W1D_RETRY || d == MOCHI_W1D_WRONG_SHARD
                                : kind == MOCHI_W1K_REFUSED && d == MOCHI_W1D_REFUSED;
  };
  auto first_ref = [&](uint32_t o0, uint32_t o, uint8_t kind) {
    for (uint32_t e = o0; e < o; e++)
      if (listed(kind, out->op_decision[e]) && op_ref[e] == op_ref[o]) return false;
    return true;
  };
  uint32_t n_ref = 0;
  for (uint32_t q = 0; q < Q; q++) {
    const uint32_t o0 = b->req_op_off[q], o1 = b->req_op_off[q + 1];
    bool failed = false, refused = false;
    for (uint32_t o = o0; o < o1; o++) {
      failed |= out->op_decision[o] == MOCHI_W1D_FAILED;
      refused |= out->op_decision[o] == MOCHI_W1D_REFUSED;
    }
    const uint8_t kind = failed ? MOCHI_W1K_THROWS : refused ? MOCHI_W1K_REFUSED : MOCHI_W1K_OK;
    out->req_kind[q] = kind;
    out->req_grant_off[q] = n_ref;
    for (uint32_t o = o0; o < o1; o++)
      if (listed(kind, out->op_decision[o]) && first_ref(o0, o, kind)) n_ref++;
  }
  out->req_grant_off[Q] = n_ref;
  // new grants in the order of the ops that made them
  std::vector<uint32_t> index_of(O, MOCHI_W1_NONE);
  uint32_t n_new = 0;
  uint64_t total = 0;
  auto size_of = [&](uint32_t o) {
    const uint32_t q = op_req[o];
    return w1_grant_size(b->op_key_len[o], b->req_hash_len[q], w1_ts(b->op_epoch[o], b->req_seed[q]),
                         out->op_decision[o] == MOCHI_W1D_WRONG_SHARD);
  };
  for (uint32_t o = 0; o < O; o++)
    if (makes[o]) {
      index_of[o] = n_new++;
      total += size_of(o);
    }
  out->n_new = n_new;
  out->grant_bytes_len = total;
  if (total > out->grant_cap) return bad("grant_cap is smaller than the size needed (grant_bytes_len)");
  // emit
  uint64_t pos = 0;
  for (uint32_t o = 0; o < O; o++) {
    const uint32_t r = op_ref[o];
    out->op_grant[o] = r == MOCHI_W1_NONE || (r & MOCHI_W1_STORED) ? r : index_of[r];
    if (!makes[o]) continue;
    const uint32_t g = index_of[o], q = op_req[o];
    const bool ws = out->op_decision[o] == MOCHI_W1D_WRONG_SHARD;
    const int64_t ts = ws ? 0 : w1_ts(b->op_epoch[o], b->req_seed[q]);
    uint8_t* p = out->grant_bytes + pos;
    p = put_ld(p, 0x0A, b->strings + b->op_key_off[o], b->op_key_len[o]);
    if (ts) {
      *p++ = 0x10;
      p = put_varint(p, (uint64_t)ts);
    }
    if (b->req_hash_len[q]) p = put_ld(p, 0x22, b->strings + b->req_hash_off[q], b->req_hash_len[q]);
    if (ws) {
      *p++ = 0x28;
      *p++ = (uint8_t)kW1WrongShard;
    }
    const uint64_t len = (uint64_t)(p - (out->grant_bytes + pos));
    if (len != size_of(o)) return bad("internal: emitted size differs from computed size");
    out->grant_off[g] = pos;
    out->grant_len[g] = (uint32_t)len;
    out->grant_op[g] = o;
    out->grant_ts[g] = ts;
    pos += len;
  }
  for (uint32_t q = 0; q < Q; q++) {
    const uint32_t o0 = b->req_op_off[q], o1 = b->req_op_off[q + 1];
    uint32_t at = out->req_grant_off[q];
    for (uint32_t o = o0; o < o1; o++)
      if (listed(out->req_kind[q], out->op_decision[o]) && first_ref(o0, o, out->req_kind[q]))
        out->req_grant[at++] = out->op_grant[o];
  }
  return MOCHI_OK;
}

}  // namespace mochi_host
