// envelope.h — the ProtocolMessage envelope codec (decode, route, join, wrap): launch
// interface between the C-ABI layer (capi.cpp) and the device kernels (envelope.hip),
// the host twin (envelope_host.cpp), and the walk, the hash and the size arithmetic
// both share.  Semantics: include/mochi_hip.h (mochi_envelope_frames and what follows).
//
// Everything under `namespace env` is __host__ __device__ and reads a frame through
// (base pointer, offsets below the frame length) alone, with the field walk of
// wire_walk.h (wire::next_fld and friends): the host form and every kernel run the
// same walk over the same bytes, and a stand-alone host program
// (microbench/envelope_check.cpp) checks under a sanitizer that no read leaves the
// slice.
//
// Wire layout (MochiProtocol.proto:194-213), parsed as protobuf-java 3.16.3 parses it
// (the rules of wire_walk.h) and written as it writes it:
//   ProtocolMessage = [28 msgTimestamp] [32 serverId] [3A msgId] [42 replyToMsgId]
//                     [payload: field 101..112, length-delimited]
#pragma once
#include "carve.h"
#include "w2_encode.h"
#include "wire_walk.h"

namespace mochi {
namespace env {

using wire::Fld;
using wire::next_fld;
using wire::valid_utf8;

constexpr uint32_t kMaxFrames = 1u << 24;
constexpr uint32_t kKinds = 13;  // PAYLOAD_NOT_SET and the cases 101..112
constexpr uint32_t kNone = 0xFFFFFFFFu;

// ---- decode: the top level of one frame ----------------------------------------------
struct Top {
  uint32_t kind, body_off, body_len;
  uint64_t ts;
  uint32_t sid_off, sid_len, mid_off, mid_len, rto_off, rto_len;
};
// Returns enum mochi_env_status.  Unless it is OK nothing of `o` is to be used.  The
// envelope level is validated whole before the oneof rule is applied: a frame with two
// payload fields whose own framing or strings are bad is MALFORMED, not FALLBACK.
WIRE_HD uint32_t frame_level(const uint8_t* p, uint32_t len, Top& o) {
  o.kind = o.body_off = o.body_len = 0;
  o.ts = 0;
  o.sid_off = o.sid_len = o.mid_off = o.mid_len = o.rto_off = o.rto_len = 0;
  uint32_t pos = 0, n_pay = 0;
  Fld f;
  int rc;
  while ((rc = next_fld(p, pos, len, f)) > 0) {
    if (f.field == 5 && f.wt == 0) {
      o.ts = f.v;  // readInt64: the low 64 bits
    } else if (f.wt == 2 && f.field >= 6 && f.field <= 8) {
      if (!valid_utf8(p, f.off, f.len)) return MOCHI_ENV_MALFORMED;  // every occurrence is read as a string
      if (f.field == 6) {
        o.sid_off = f.off;
        o.sid_len = f.len;
      } else if (f.field == 7) {
        o.mid_off = f.off;
        o.mid_len = f.len;
      } else {
        o.rto_off = f.off;
        o.rto_len = f.len;
      }
    } else if (f.wt == 2 && f.field >= 101 && f.field <= 112) {
      n_pay++;
      o.kind = f.field - 100;
      o.body_off = f.off;
      o.body_len = f.len;
    }
  }
  if (rc < 0) return MOCHI_ENV_MALFORMED;
  return n_pay > 1 ? MOCHI_ENV_FALLBACK : MOCHI_ENV_OK;
}

// What the decoder reads and writes: host pointers in the host form, device pointers in the kernel.
struct DecView {
  mochi_envelope_frames in;
  mochi_envelope_decoded out;
};
WIRE_HD void decode_frame(const DecView& v, uint32_t f) {
  const uint64_t base = v.in.frame_off[f];
  Top t;
  const uint32_t st = frame_level(v.in.wire + base, v.in.frame_len[f], t);
  const bool ok = st == MOCHI_ENV_OK;
  const mochi_envelope_decoded& o = v.out;
  o.status[f] = (uint8_t)st;
  o.kind[f] = ok ? (uint8_t)t.kind : (uint8_t)0;
  o.body_off[f] = base + (ok ? t.body_off : 0);
  o.body_len[f] = ok ? t.body_len : 0;
  o.msg_timestamp[f] = ok ? (int64_t)t.ts : 0;
  o.server_id_off[f] = base + (ok ? t.sid_off : 0);
  o.server_id_len[f] = ok ? t.sid_len : 0;
  o.msg_id_off[f] = base + (ok ? t.mid_off : 0);
  o.msg_id_len[f] = ok ? t.mid_len : 0;
  o.reply_to_off[f] = base + (ok ? t.rto_off : 0);
  o.reply_to_len[f] = ok ? t.rto_len : 0;
}

// ---- route -----------------------------------------------------------------------------
// the bin of a frame: its kind, or kKinds for a frame that takes no place
WIRE_HD uint32_t route_bin(uint8_t status, uint8_t kind) {
  return status == MOCHI_ENV_OK && kind < kKinds ? (uint32_t)kind : kKinds;
}
struct RouteView {
  uint32_t n;
  const uint8_t* status;
  const uint8_t* kind;
  const uint64_t* body_off;
  const uint32_t* body_len;
  mochi_envelope_routed out;
};

// ---- join -------------------------------------------------------------------------------
// The msgId table is k_w1q_claim's (w1_request.hip): open addressing, the slot from
// wire::bytes_hash, the smallest claimant wins.  Its slots: a power of two, at least 2 * Q
inline uint32_t join_slots(uint32_t Q) {
  uint32_t s = 16;
  while (s < 2 * (uint64_t)Q) s <<= 1;
  return s;
}
// bits of the grouping sort's keys: the request index, Q for a frame in no run
inline int join_key_bits(uint32_t Q) {
  int b = 1;
  while (b < 32 && (Q >> b)) b++;
  return b;
}
WIRE_HD uint8_t w1_kind_of(uint8_t kind) {
  return kind == 8 ? MOCHI_W1_OK : kind == 9 ? MOCHI_W1_REFUSED : kind == 12 ? MOCHI_W1_REQUEST_FAILED : MOCHI_W1_OTHER;
}
WIRE_HD uint8_t rr_kind_of(uint8_t kind) {
  return kind == 11 ? MOCHI_RR_WRITE2_ANS : kind == 6 ? MOCHI_RR_READ : MOCHI_RR_OTHER;
}
struct JoinView {
  mochi_envelope_requests rq;
  mochi_envelope_frames fr;
  mochi_envelope_decoded dec;  // read, not written
  mochi_envelope_joined out;
};
// does frame f look for a request at all
WIRE_HD bool join_asks(const JoinView& v, uint32_t f) { return v.dec.status[f] == MOCHI_ENV_OK && v.dec.reply_to_len[f] != 0; }
// slot i of the grouped outputs <- frame f
WIRE_HD void join_emit(const JoinView& v, uint32_t i, uint32_t f) {
  const uint8_t k = v.dec.kind[f];
  v.out.resp_frame[i] = f;
  v.out.resp_off[i] = v.dec.body_off[f];
  v.out.resp_len[i] = v.dec.body_len[f];
  v.out.resp_w1_kind[i] = w1_kind_of(k);
  v.out.resp_rr_kind[i] = rr_kind_of(k);
}

// ---- wrap: sizes ------------------------------------------------------------------------
WIRE_HD uint32_t len_or_0(const uint64_t* off, const uint32_t* len, uint32_t m) { return off ? len[m] : 0; }
struct Sized {
  uint64_t len;     // the message; 0 unless status is OK
  uint32_t prefix;  // bytes of the length prefix before it (0 without MOCHI_ENV_LENGTH_PREFIX)
  uint8_t status;
};
WIRE_HD Sized size_msg(const mochi_envelope_source& s, uint32_t m) {
  Sized z{0, 0, MOCHI_ENC_OK};
  const uint8_t k = s.kind[m];
  if (k >= kKinds) {
    z.status = MOCHI_ENC_BAD_KIND;
  } else {
    const uint32_t sl = len_or_0(s.server_id_off, s.server_id_len, m), ml = len_or_0(s.msg_id_off, s.msg_id_len, m),
                   rl = len_or_0(s.reply_to_off, s.reply_to_len, m);
    if ((sl && !valid_utf8(s.ids + s.server_id_off[m], 0, sl)) || (ml && !valid_utf8(s.ids + s.msg_id_off[m], 0, ml)) ||
        (rl && !valid_utf8(s.ids + s.reply_to_off[m], 0, rl))) {
      z.status = MOCHI_ENC_BAD_ID;
    } else {
      const uint64_t ts = (uint64_t)s.msg_timestamp[m];
      z.len = (ts ? 1 + wire::varint_size(ts) : 0) + enc_ld_opt_size(sl) + enc_ld_opt_size(ml) + enc_ld_opt_size(rl) +
              (k ? 2 + wire::varint_size(s.body_len[m]) + (uint64_t)s.body_len[m] : 0);  // the payload tag takes two bytes
      if (z.len > kEncMaxMsg) {
        z.status = MOCHI_ENC_TOO_LONG;
        z.len = 0;
      }
    }
  }
  // a message that is not OK is emitted empty; with the prefix flag its frame is the one byte 00
  z.prefix = s.flags & MOCHI_ENV_LENGTH_PREFIX ? wire::varint_size(z.len) : 0;
  return z;
}
// the two tag bytes of payload case k (1..12): field 100 + k, length-delimited
WIRE_HD uint32_t payload_tag(uint32_t k) { return ((100 + k) << 3) | 2; }

}  // namespace env

// ---- device side: arguments and scratch ------------------------------------------------
// Device pointers throughout.  Each call lays its scratch out with its one layout
// function (every array 16-byte aligned): on a null base it only counts and returns the
// bytes to allocate; on that allocation it sets the scratch pointers.
struct EnvDecArgs {
  env::DecView v;
  hipEvent_t* ev;  // per-kernel timing or null: before and after k_env_decode
};
constexpr int kEnvDecEvents = 2, kEnvDecStages = 1;  // the decoder has no scratch
hipError_t launch_env_decode(const EnvDecArgs& a, hipStream_t stream);

struct EnvRouteArgs {
  env::RouteView v;
  uint32_t blocks;   // cdiv(n, 256)
  uint64_t* hist64;  // [14 * blocks + 1] per (bin, block) count, bin-major; last = 0
  uint64_t* base64;  // [14 * blocks + 1] its exclusive scan
  void* scan_temp;
  size_t scan_temp_bytes;
  hipEvent_t* ev;  // before k_env_hist, after it, after the scan, after k_env_scatter
};
constexpr int kEnvRouteEvents = 4, kEnvRouteStages = 3;
inline uint32_t env_route_scan_n(uint32_t blocks) { return (env::kKinds + 1) * blocks + 1; }
inline size_t env_route_layout(EnvRouteArgs& a, void* base) {
  Carve c(base);
  a.hist64 = c.take<uint64_t>(env_route_scan_n(a.blocks));
  a.base64 = c.take<uint64_t>(env_route_scan_n(a.blocks));
  return c.bytes();
}
hipError_t launch_env_route(const EnvRouteArgs& a, hipStream_t stream);

struct EnvJoinArgs {
  env::JoinView v;
  uint32_t slots;     // env::join_slots(Q)
  int key_bits;       // env::join_key_bits(Q)
  uint32_t* n_resps;  // the caller's device word
  uint32_t* tbl_req;  // [slots] the request that claimed the slot, ~0 = empty
  uint32_t* tbl_min;  // [slots] the smallest request index that reached the slot
  uint32_t* key_in;   // [n] the frame's request, Q = none (sort input)
  uint32_t* key_out;  // [n] sorted
  uint32_t* val_in;   // [n] frame indices 0..n-1
  uint32_t* val_out;  // [n] the frames grouped by request, frame order inside a request
  void* scan_temp;    // the radix sort's temp
  size_t scan_temp_bytes;
  hipEvent_t* ev;  // before the table clear, after k_env_claim, after k_env_lookup, after the sort, after k_env_group
};
constexpr int kEnvJoinEvents = 5, kEnvJoinStages = 4;
inline size_t env_join_layout(EnvJoinArgs& a, void* base) {
  const size_t n = a.v.fr.n_frames;
  Carve c(base);
  a.tbl_req = c.take<uint32_t>(a.slots);  // tbl_req and tbl_min adjacent: one fill
  a.tbl_min = c.take<uint32_t>(a.slots);
  a.key_in = c.take<uint32_t>(n);
  a.key_out = c.take<uint32_t>(n);
  a.val_in = c.take<uint32_t>(n);
  a.val_out = c.take<uint32_t>(n);
  return c.bytes();
}
hipError_t env_sort_temp_bytes(uint32_t n, int key_bits, size_t* bytes);
hipError_t launch_env_join(const EnvJoinArgs& a, hipStream_t stream);

struct EnvEncArgs {
  mochi_envelope_source in;
  // outputs
  uint8_t* wire;
  uint64_t wire_cap;
  uint64_t* msg_off;  // [M]
  uint32_t* msg_len;  // [M]
  uint8_t* status;    // [M]
  // scratch
  uint64_t* frm_off;  // [M] where the frame begins: its prefix, or the message itself
  uint64_t* body_dst; // [M] wire offset of the body's bytes, ~0 = none
  uint64_t* len64;    // [M+1] frame lengths (scan input), last = 0
  uint64_t* off64;    // [M+1] their exclusive scan; off64[M] = the wire size
  void* scan_temp;
  size_t scan_temp_bytes;
  hipEvent_t* ev;  // before k_env_size, after it, after the scan; before k_env_hdr, after it, after k_env_copy
};
constexpr int kEnvEncEvents = 6, kEnvEncStages = 4;
inline size_t env_enc_layout(EnvEncArgs& a, void* base) {
  const size_t M = a.in.n_msgs;
  Carve c(base);
  a.frm_off = c.take<uint64_t>(M);
  a.body_dst = c.take<uint64_t>(M);
  a.len64 = c.take<uint64_t>(M + 1);
  a.off64 = c.take<uint64_t>(M + 1);
  return c.bytes();
}
// sizes + the 64-bit exclusive scan: fills msg_len / status, frm_off and off64[M]
hipError_t launch_env_size(const EnvEncArgs& a, hipStream_t stream);
// msg_off and the headers (nothing of `wire` when off64[M] > wire_cap); with copy: the bodies
hipError_t launch_env_emit(const EnvEncArgs& a, bool copy, hipStream_t stream);

}  // namespace mochi

namespace mochi_host {
// the four host forms without the null checks of the C layer; `err` names an
// inconsistent input (MOCHI_EINVAL)
int envelope_decode(const mochi_envelope_frames* in, mochi_envelope_decoded* out, const char** err);
int envelope_route(const mochi::env::RouteView* v, const char** err);
int envelope_join(const mochi::env::JoinView* v, uint32_t* n_resps, const char** err);
int envelope_encode(const mochi_envelope_source* s, uint8_t* wire, uint64_t wire_cap, uint64_t* msg_off, uint32_t* msg_len,
                    uint8_t* status, uint64_t* wire_len, const char** err);
}  // namespace mochi_host
