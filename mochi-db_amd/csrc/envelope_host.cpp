// envelope_host.cpp — the host forms of the envelope codec (mochi_envelope_decode /
// _route / _join / _encode): the walk and the size arithmetic of envelope.h (the ones
// the kernels of envelope.hip run), frame by frame.  No GPU, no context.  The join uses
// a hash map where the device uses its claim table, the partition and the grouping a
// counting pass where the device uses ballots, scans and a radix sort: both are stable,
// so the results are equal array for array.
#include <string_view>
#include <unordered_map>
#include <vector>

#include "envelope.h"
#include "wire_put.h"

namespace mochi_host {

using namespace mochi::env;

int envelope_decode(const mochi_envelope_frames* in, mochi_envelope_decoded* out, const char** err) {
  *err = nullptr;
  const uint32_t n = in->n_frames;
  for (uint32_t f = 0; f < n; f++)
    if (!inside(in->frame_off[f], in->frame_len[f], in->wire_len)) {
      *err = "a frame slice lies outside wire";
      return MOCHI_EINVAL;
    }
  const DecView v{*in, *out};
  for (uint32_t f = 0; f < n; f++) decode_frame(v, f);
  return MOCHI_OK;
}

int envelope_route(const RouteView* v, const char** err) {
  *err = nullptr;
  uint32_t cnt[kKinds + 1] = {0};
  for (uint32_t f = 0; f < v->n; f++) cnt[route_bin(v->status[f], v->kind[f])]++;
  uint32_t at[kKinds + 1];
  for (uint32_t k = 0, sum = 0; k <= kKinds; k++) {
    v->out.kind_off[k] = at[k] = sum;
    sum += cnt[k];
  }
  for (uint32_t f = 0; f < v->n; f++) {
    const uint32_t b = route_bin(v->status[f], v->kind[f]);
    if (b == kKinds) continue;
    const uint32_t i = at[b]++;
    v->out.order[i] = f;
    v->out.body_off[i] = v->body_off[f];
    v->out.body_len[i] = v->body_len[f];
  }
  return MOCHI_OK;
}

int envelope_join(const JoinView* v, uint32_t* n_resps, const char** err) {
  *err = nullptr;
  *n_resps = 0;
  const uint32_t Q = v->rq.n_reqs, n = v->fr.n_frames;
  for (uint32_t q = 0; q < Q; q++)
    if (!inside(v->rq.id_off[q], v->rq.id_len[q], v->rq.ids_len)) {
      *err = "a request id lies outside ids";
      return MOCHI_EINVAL;
    }
  for (uint32_t f = 0; f < n; f++)
    if (join_asks(*v, f) && !inside(v->dec.reply_to_off[f], v->dec.reply_to_len[f], v->fr.wire_len)) {
      *err = "a replyToMsgId lies outside wire";
      return MOCHI_EINVAL;
    }
  std::unordered_map<std::string_view, uint32_t> table;
  for (uint32_t q = 0; q < Q; q++)  // emplace keeps the first: the smaller request index
    if (v->rq.id_len[q]) table.emplace(std::string_view((const char*)v->rq.ids + v->rq.id_off[q], v->rq.id_len[q]), q);
  std::vector<uint32_t> cnt(Q + 1, 0);
  for (uint32_t f = 0; f < n; f++) {
    uint32_t q = kNone;
    if (join_asks(*v, f)) {
      const auto it = table.find(std::string_view((const char*)v->fr.wire + v->dec.reply_to_off[f], v->dec.reply_to_len[f]));
      if (it != table.end()) q = it->second;
    }
    v->out.frame_req[f] = q;
    if (q != kNone) cnt[q]++;
  }
  uint32_t sum = 0;
  for (uint32_t q = 0; q <= Q; q++) {
    v->out.req_resp_off[q] = sum;
    const uint32_t c = cnt[q];
    cnt[q] = sum;
    sum += c;
  }
  for (uint32_t f = 0; f < n; f++)
    if (v->out.frame_req[f] != kNone) join_emit(*v, cnt[v->out.frame_req[f]]++, f);
  *n_resps = sum;
  return MOCHI_OK;
}

int envelope_encode(const mochi_envelope_source* s, uint8_t* wire, uint64_t wire_cap, uint64_t* msg_off, uint32_t* msg_len,
                    uint8_t* status, uint64_t* wire_len, const char** err) {
  using namespace mochi;
  const uint32_t M = s->n_msgs;
  auto bad = [&](const char* what) {
    *err = what;
    return MOCHI_EINVAL;
  };
  *wire_len = 0;
  for (uint32_t m = 0; m < M; m++) {
    if (s->kind[m] >= kKinds) return bad("a kind is above 12");
    if (s->kind[m] && !inside(s->body_off[m], s->body_len[m], s->bodies_len)) return bad("a body slice lies outside bodies");
    if (s->msg_id_off && !inside(s->msg_id_off[m], s->msg_id_len[m], s->ids_len)) return bad("a msgId lies outside ids");
    if (s->reply_to_off && !inside(s->reply_to_off[m], s->reply_to_len[m], s->ids_len))
      return bad("a replyToMsgId lies outside ids");
    if (s->server_id_off && !inside(s->server_id_off[m], s->server_id_len[m], s->ids_len))
      return bad("a serverId lies outside ids");
  }
  uint64_t total = 0;
  for (uint32_t m = 0; m < M; m++) {
    const Sized z = size_msg(*s, m);
    if (z.status == MOCHI_ENC_BAD_ID) return bad("an id is not UTF-8");
    status[m] = z.status;
    msg_len[m] = (uint32_t)z.len;
    msg_off[m] = total + z.prefix;
    total += z.prefix + z.len;
  }
  *wire_len = total;
  if (total > wire_cap) return bad("wire_cap is smaller than the encoded size (*wire_len)");
  for (uint32_t m = 0; m < M; m++) {
    uint8_t* o = wire + msg_off[m];
    if (s->flags & MOCHI_ENV_LENGTH_PREFIX) put_varint(o - wire::varint_size(msg_len[m]), msg_len[m]);
    if (status[m] != MOCHI_ENC_OK) continue;
    const uint64_t ts = (uint64_t)s->msg_timestamp[m];
    if (ts) {
      *o++ = 0x28;
      o = put_varint(o, ts);
    }
    if (const uint32_t l = len_or_0(s->server_id_off, s->server_id_len, m)) o = put_ld(o, 0x32, s->ids + s->server_id_off[m], l);
    if (const uint32_t l = len_or_0(s->msg_id_off, s->msg_id_len, m)) o = put_ld(o, 0x3A, s->ids + s->msg_id_off[m], l);
    if (const uint32_t l = len_or_0(s->reply_to_off, s->reply_to_len, m)) o = put_ld(o, 0x42, s->ids + s->reply_to_off[m], l);
    if (const uint32_t k = s->kind[m]) {
      o = put_varint(o, payload_tag(k));
      o = put_varint(o, s->body_len[m]);
      if (s->body_len[m]) memcpy(o, s->bodies + s->body_off[m], s->body_len[m]);
      o += s->body_len[m];
    }
    if ((uint64_t)(o - (wire + msg_off[m])) != msg_len[m]) return bad("internal: emitted size differs from computed size");
  }
  return MOCHI_OK;
}

}  // namespace mochi_host
