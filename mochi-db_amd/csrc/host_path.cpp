// host_path.cpp — the entry points that take their arrays in host memory
// (mochi_verify_batch, mochi_verify_write2, mochi_write2_decode): both cut the
// batch into chunks (chunk_plan.h) and drive them through one upload / compute /
// download pipeline (HostPipe) around the device-side steps of capi.cpp.
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <thread>

#include "chunk_plan.h"
#include "ctx.h"
#include "w2_host.h"

using namespace mochi;

namespace {

bool copy_streams() {
  static const bool v = [] {
    const char* e = getenv("MOCHI_COPY_STREAMS");
    return e && atoi(e) != 0;
  }();
  return v;
}

// Host-side consistency checks (host path only; the device path trusts the caller's device arrays).
int check_batch_host(const mochi_batch* b) {
  if (b->cert_grant_off[0] != 0 || b->cert_grant_off[b->n_certs] != b->n_grants)
    return fail(MOCHI_EINVAL, "cert_grant_off must start at 0 and end at n_grants");
  if (b->cert_op_off[0] != 0 || b->cert_op_off[b->n_certs] != b->n_ops)
    return fail(MOCHI_EINVAL, "cert_op_off must start at 0 and end at n_ops");
  for (uint32_t c = 0; c < b->n_certs; c++) {
    if (b->cert_grant_off[c + 1] < b->cert_grant_off[c] || b->cert_op_off[c + 1] < b->cert_op_off[c])
      return fail(MOCHI_EINVAL, "CSR offsets must be non-decreasing (cert %u)", c);
    if (b->cert_op_off[c + 1] - b->cert_op_off[c] > MOCHI_MAX_OPS_PER_CERT)
      return fail(MOCHI_EINVAL, "cert %u has more than %d ops", c, MOCHI_MAX_OPS_PER_CERT);
  }
  for (uint32_t i = 0; i < b->n_grants; i++) {
    if (b->grant_len[i] > 65536) return fail(MOCHI_EINVAL, "grant %u longer than 65536 bytes", i);
    if (b->grant_off[i] > b->grant_bytes_len || b->grant_len[i] > b->grant_bytes_len - b->grant_off[i])
      return fail(MOCHI_EINVAL, "grant %u lies outside grant_bytes", i);
  }
  for (uint32_t o = 0; o < b->n_ops; o++) {
    if (b->op_key[o] >= MOCHI_MAX_OPS_PER_CERT) return fail(MOCHI_EINVAL, "op_key[%u] >= %d", o, MOCHI_MAX_OPS_PER_CERT);
    if (b->op_key_off && (b->op_key_off[o] > b->grant_bytes_len || b->op_key_len[o] > b->grant_bytes_len - b->op_key_off[o]))
      return fail(MOCHI_EINVAL, "op key %u lies outside grant_bytes", o);
  }
  if (b->cert_mg_off) {
    if (b->cert_mg_off[0] != 0 || b->cert_mg_off[b->n_certs] != b->n_mgs)
      return fail(MOCHI_EINVAL, "cert_mg_off must start at 0 and end at n_mgs");
    if (b->mg_grant_off[0] != 0 || b->mg_grant_off[b->n_mgs] != b->n_grants)
      return fail(MOCHI_EINVAL, "mg_grant_off must start at 0 and end at n_grants");
    for (uint32_t m = 0; m < b->n_mgs; m++)
      if (b->mg_grant_off[m + 1] < b->mg_grant_off[m]) return fail(MOCHI_EINVAL, "mg_grant_off decreases at %u", m);
    for (uint32_t c = 0; c < b->n_certs; c++)
      if (b->cert_mg_off[c + 1] < b->cert_mg_off[c] || b->mg_grant_off[b->cert_mg_off[c]] != b->cert_grant_off[c])
        return fail(MOCHI_EINVAL, "MultiGrants of cert %u do not cover its grants", c);
  }
  return MOCHI_OK;
}

// ---- host path: chunked H2D / compute / D2H pipeline ------------------------
//
// The batch is cut at certificate boundaries (multiples of 32 certificates, so
// every chunk's accept bits start on a word) into chunks of ~kChunkGrants
// grants.  Chunk j's inputs go up on the copy-in stream, its kernels run on the
// context stream once they have landed, and its verdicts come down on the
// copy-out stream while chunk j+1 computes.  Every chunk has its own input
// region on the device and writes disjoint output slices, so the only
// cross-stream ordering is one event per hand-off.  Sources that are already
// pinned (mochi_host_alloc) are DMA'd in place; others are staged through the
// context's pinned buffer with a parallel memcpy.
bool is_pinned(const void* ptr) {
  if (!ptr) return false;
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, ptr) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeHost;
}

int ensure_events(std::vector<hipEvent_t>& ev, size_t n) {
  while (ev.size() < n) {
    hipEvent_t e;
    HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    ev.push_back(e);
  }
  return MOCHI_OK;
}

// One input array of one chunk.  A null src with bytes set is an array the caller
// writes into its staging slot itself (a CSR array rebased to the chunk).
struct SegIn {
  size_t bytes;
  const void* src;
  size_t off = 0;  // in pin_in and dev_in
};

// What an output slice is indexed by.  kPerCert: certificates or messages; kAccWord:
// words of 32 of those; kWhole: one unit that only the last chunk completes.
enum Unit { kPerGrant, kPerCert, kPerOp, kAccWord, kWhole, kNumUnit };

// One whole-batch output array; every chunk writes its own range of it.  It comes down
// from the device and is copied to dst when the caller gave a dst, or when `always`.
struct OutSlice {
  void* dst;
  size_t per_unit;  // bytes
  Unit unit;
  bool always = false;
  size_t reserve = 0;  // bytes the device writes whether it comes down or not
  size_t off = 0;      // in dev_out and pin_out
  bool wanted() const { return dst || always; }
};

// What mochi_verify_batch and mochi_verify_write2 share.  The caller carves every
// chunk's segments from `in`, sets the mode flags, then: start, per chunk upload / its own
// launches / download in the order it needs, and end.
struct HostPipe {
  mochi_ctx* c;
  int nseg;
  OutSlice* out;
  int nout;
  size_t units[kNumUnit];  // of the whole batch: grants, certificates, ops, accept words, 1
  Carve256 in, dn;  // pin_in / dev_in and dev_out / pin_out
  // one copy of the staged segments up; one of the whole output region down; both on the launch stream
  bool one_up = false, one_down = false, on_st = false;
  bool pinned[16] = {};  // the segment's source is DMA'd in place

  hipStream_t s_in() const { return on_st ? c->stream : c->s_in; }
  hipStream_t s_out() const { return on_st ? c->stream : c->s_out; }
  uint8_t* stage(const SegIn& s) const { return (uint8_t*)c->pin_in.p + s.off; }
  uint8_t* dev(const SegIn& s) const { return c->dev_in.as<uint8_t>() + s.off; }
  uint8_t* dev_out(int i) const { return c->dev_out.as<uint8_t>() + out[i].off; }
  size_t bytes(const OutSlice& s) const { return s.per_unit * units[s.unit]; }

  HostPipe(mochi_ctx* ctx, int n_seg, OutSlice* slices, int n_out, size_t grants, size_t certs, size_t ops)
      : c(ctx), nseg(n_seg), out(slices), nout(n_out), units{grants, certs, ops, (certs + 31) / 32, 1} {
    for (int i = 0; i < nout; i++) {  // the output slices at 256-byte steps
      const size_t want = out[i].wanted() ? bytes(out[i]) : 0;
      out[i].off = dn.take(want > out[i].reserve ? want : out[i].reserve);
    }
  }

  // The four buffers and the hand-off events; sources already pinned (mochi_host_alloc)
  // are DMA'd in place, judged once by chunk 0's; the call's span begins
  int start(size_t nch, const SegIn* chunk0) {
    int rc;
    if ((rc = c->pin_in.ensure(in.total)) || (rc = c->dev_in.ensure(in.total)) || (rc = c->pin_out.ensure(dn.total)) ||
        (rc = c->dev_out.ensure(dn.total)) || (rc = ensure_events(c->chunk_ev, 2 * nch)))
      return rc;
    for (int i = 0; i < nseg; i++) pinned[i] = !one_up && is_pinned(chunk0[i].src);
    c->ev_set ^= 1;  // this call's span events: the other set keeps the last call's
    c->ev = c->evs[c->ev_set];
    HIP_TRY(hipEventRecord(c->ev[0], s_in()));
    return MOCHI_OK;
  }

  // Chunk j's segments go up and the launch stream waits for them
  int upload(size_t j, const SegIn* seg) {
    size_t staged_end = 0;
    for (int i = 0; i < nseg; i++) {
      const SegIn& s = seg[i];
      if (!s.bytes) continue;
      const void* src = stage(s);
      if (pinned[i]) src = s.src;
      else if (s.src) par_memcpy(stage(s), s.src, s.bytes);
      if (one_up) staged_end = s.off + s.bytes > staged_end ? s.off + s.bytes : staged_end;
      else HIP_TRY(hipMemcpyAsync(dev(s), src, s.bytes, hipMemcpyHostToDevice, s_in()));
    }
    if (staged_end) HIP_TRY(hipMemcpyAsync(c->dev_in.p, c->pin_in.p, staged_end, hipMemcpyHostToDevice, s_in()));
    if (!on_st) {
      HIP_TRY(hipEventRecord(c->chunk_ev[2 * j], s_in()));
      HIP_TRY(hipStreamWaitEvent(c->stream, c->chunk_ev[2 * j], 0));
    }
    if (j == 0) HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    return MOCHI_OK;
  }

  int down(size_t off, size_t n) {
    if (n) HIP_TRY(hipMemcpyAsync((uint8_t*)c->pin_out.p + off, c->dev_out.as<uint8_t>() + off, n,
                                  hipMemcpyDeviceToHost, s_out()));
    return MOCHI_OK;
  }

  // Chunk j's launches are enqueued: its range of every wanted slice comes down
  // (u: its units [first, end) by kPerGrant, kPerCert, kPerOp)
  int download(size_t j, bool last, const uint32_t (&u)[3][2]) {
    if (last) HIP_TRY(hipEventRecord(c->ev[2], c->stream));
    if (!on_st) {
      HIP_TRY(hipEventRecord(c->chunk_ev[2 * j + 1], c->stream));
      HIP_TRY(hipStreamWaitEvent(s_out(), c->chunk_ev[2 * j + 1], 0));
    }
    if (one_down) return down(0, dn.total);
    // accept words: whole ones but for the batch's last; kWhole: with the last chunk
    const size_t w0 = u[kPerCert][0] / 32, w1 = last ? units[kAccWord] : w0 + (u[kPerCert][1] - u[kPerCert][0]) / 32;
    const size_t r[kNumUnit][2] = {{u[0][0], u[0][1]}, {u[1][0], u[1][1]}, {u[2][0], u[2][1]}, {w0, w1}, {0, last}};
    int rc = MOCHI_OK;
    for (const OutSlice* s = out; s < out + nout && !rc; s++)
      if (s->wanted()) rc = down(s->off + s->per_unit * r[s->unit][0], s->per_unit * (r[s->unit][1] - r[s->unit][0]));
    return rc;
  }

  // Waits for the last download and hands every slice to the caller.  The spans (first
  // upload, compute, last download, whole call) are read from the events when asked.
  int end() {
    HIP_TRY(hipEventRecord(c->ev[3], s_out()));
    HIP_TRY(hipStreamSynchronize(s_out()));
    c->ev_done = c->ev_set;
    c->timing_pending = true;
    c->acc_words = (uint32_t)units[kAccWord];
    for (int i = 0; i < nout; i++) {
      const OutSlice& s = out[i];
      if (s.dst && bytes(s)) memcpy(s.dst, (uint8_t*)c->pin_out.p + s.off, bytes(s));
      if (s.unit == kAccWord) c->acc_dev = (const uint32_t*)dev_out(i);
    }
    return MOCHI_OK;
  }
};

// Input segments of one chunk, in mochi_batch order.  The CSR arrays (6, 7,
// 11, 12) are rebased per chunk and therefore always staged.
enum Seg {
  kBlob, kGrantOff, kGrantLen, kSig, kSigner, kGrantKey, kCertGrantOff, kCertOpOff, kOpKey, kOpFlags, kExpHash,
  kCertMgOff, kMgGrantOff, kOpObjTs, kOpKeyOff, kOpKeyLen, kNumSeg
};
static_assert(kNumSeg <= sizeof HostPipe::pinned, "HostPipe::pinned");
// Output slices, in download order
enum Out { kOutFlags, kOutTs, kOutAcc, kOutReason, kOutFail, kOutDec, kOutG0, kOutOpTs, kOutGrantBits, kNumOut };

int run_host_pipeline(mochi_ctx* c, const mochi_batch* b, const mochi_params* p, mochi_verdicts* o) {
  const uint32_t N = b->n_grants, C = b->n_certs, O = b->n_ops;
  c->acc_dev = nullptr;
  c->acc_words = 0;
  const bool mg = b->cert_mg_off != nullptr;
  const uint32_t *cgo = b->cert_grant_off, *coo = b->cert_op_off, *cmo = b->cert_mg_off;
  OutSlice out[kNumOut] = {{o->grant_flags, 1, kPerGrant, false, N},  // the kernels always write them
                           {o->grant_ts, sizeof(int64_t), kPerGrant},
                           {o->cert_accept_bits, 4, kAccWord},
                           {o->cert_reason, 1, kPerCert},
                           {o->cert_fail_op, 1, kPerCert},
                           {o->op_decision, 1, kPerOp},
                           {o->op_g0, sizeof(uint32_t), kPerOp},
                           {o->op_ts, sizeof(int64_t), kPerOp},
                           {o->grant_valid_bits, ((size_t)N + 31) / 32 * 4, kWhole}};
  HostPipe hp(c, kNumSeg, out, kNumOut, N, C, O);
  struct Chunk {
    uint32_t c0, c1, g0, g1, o0, o1, m0, m1;
    ByteRange blob;  // of grant_bytes
    SegIn seg[kNumSeg];
  };
  std::vector<Chunk> ch;
  uint32_t max_grants = 0, max_certs = 0;
  auto weight = [&](uint32_t lo, uint32_t hi) { return cgo[hi] - cgo[lo]; };
  plan_chunks(C, c->chunk_grants, weight, [&](uint32_t c0, uint32_t c1) {
    ch.push_back({c0, c1, cgo[c0], cgo[c1], coo[c0], coo[c1], mg ? cmo[c0] : 0, mg ? cmo[c1] : 0, {}, {}});
    Chunk& k = ch.back();
    k.blob.add(b->grant_off, b->grant_len, k.g0, k.g1);
    if (b->op_key_off) k.blob.add(b->op_key_off, b->op_key_len, k.o0, k.o1);  // MOCHI_Q_BIND reads the op keys too
    const size_t ng = k.g1 - k.g0, nc = c1 - c0, no = k.o1 - k.o0, nm = k.m1 - k.m0;
    if (ng > max_grants) max_grants = (uint32_t)ng;
    if (nc > max_certs) max_certs = (uint32_t)nc;
    SegIn* s = k.seg;
    s[kBlob] = {(size_t)(k.blob.hi - k.blob.lo), b->grant_bytes + k.blob.lo};
    s[kGrantOff] = {sizeof(uint64_t) * ng, b->grant_off + k.g0};
    s[kGrantLen] = {sizeof(uint32_t) * ng, b->grant_len + k.g0};
    s[kSig] = {(size_t)MOCHI_RSA_BYTES * ng, b->sig + (size_t)MOCHI_RSA_BYTES * k.g0};
    s[kSigner] = {sizeof(uint16_t) * ng, b->signer + k.g0};
    s[kGrantKey] = {ng, b->grant_key + k.g0};
    s[kCertGrantOff] = s[kCertOpOff] = {sizeof(uint32_t) * (nc + 1), nullptr};
    s[kOpKey] = {no, b->op_key + k.o0};
    s[kOpFlags] = {no, b->op_flags + k.o0};
    s[kExpHash] = {(size_t)MOCHI_TXN_HASH_BYTES * nc, b->expected_hash + (size_t)MOCHI_TXN_HASH_BYTES * c0};
    s[kCertMgOff] = {mg ? sizeof(uint32_t) * (nc + 1) : 0, nullptr};
    s[kMgGrantOff] = {mg ? sizeof(uint32_t) * (nm + 1) : 0, nullptr};
    s[kOpObjTs] = {b->op_object_ts ? sizeof(int64_t) * no : 0, b->op_object_ts ? b->op_object_ts + k.o0 : nullptr};
    s[kOpKeyOff] = {b->op_key_off ? sizeof(uint64_t) * no : 0, b->op_key_off ? b->op_key_off + k.o0 : nullptr};
    s[kOpKeyLen] = {b->op_key_len ? sizeof(uint32_t) * no : 0, b->op_key_len ? b->op_key_len + k.o0 : nullptr};
    for (SegIn& x : k.seg) x.off = hp.in.take(x.bytes);
  });
  const size_t nchunks = ch.size();
  hp.one_down = nchunks == 1 && hp.dn.total <= (4u << 20);  // one small chunk: one download of the whole region
  int rc;
  if ((rc = ensure_scratch(c, max_grants, max_certs)) || (rc = hp.start(nchunks, ch[0].seg))) return rc;
  for (size_t j = 0; j < nchunks; j++) {
    const Chunk& k = ch[j];
    const SegIn* s = k.seg;
    uint32_t* cg = (uint32_t*)hp.stage(s[kCertGrantOff]);
    uint32_t* co = (uint32_t*)hp.stage(s[kCertOpOff]);
    for (uint32_t x = k.c0; x <= k.c1; x++) {
      cg[x - k.c0] = cgo[x] - k.g0;
      co[x - k.c0] = coo[x] - k.o0;
    }
    if (mg) {
      uint32_t* cm = (uint32_t*)hp.stage(s[kCertMgOff]);
      uint32_t* mo = (uint32_t*)hp.stage(s[kMgGrantOff]);
      for (uint32_t x = k.c0; x <= k.c1; x++) cm[x - k.c0] = cmo[x] - k.m0;
      for (uint32_t x = k.m0; x <= k.m1; x++) mo[x - k.m0] = b->mg_grant_off[x] - k.g0;
    }
    if ((rc = hp.upload(j, s))) return rc;
    auto at = [&](int i) -> const void* { return s[i].bytes ? hp.dev(s[i]) : nullptr; };
    mochi_batch db;
    memset(&db, 0, sizeof db);
    db.n_grants = k.g1 - k.g0;
    db.n_certs = k.c1 - k.c0;
    db.n_ops = k.o1 - k.o0;
    db.n_mgs = k.m1 - k.m0;
    db.grant_bytes_len = k.blob.hi;
    db.grant_bytes = hp.dev(s[kBlob]) - k.blob.lo;  // kernels add the absolute grant_off / op_key_off
    db.grant_off = (const uint64_t*)hp.dev(s[kGrantOff]);
    db.grant_len = (const uint32_t*)hp.dev(s[kGrantLen]);
    db.sig = hp.dev(s[kSig]);
    db.signer = (const uint16_t*)hp.dev(s[kSigner]);
    db.grant_key = hp.dev(s[kGrantKey]);
    db.cert_grant_off = (const uint32_t*)hp.dev(s[kCertGrantOff]);
    db.cert_op_off = (const uint32_t*)hp.dev(s[kCertOpOff]);
    db.op_key = hp.dev(s[kOpKey]);
    db.op_flags = hp.dev(s[kOpFlags]);
    db.expected_hash = hp.dev(s[kExpHash]);
    db.cert_mg_off = (const uint32_t*)at(kCertMgOff);
    db.mg_grant_off = (const uint32_t*)at(kMgGrantOff);
    db.op_object_ts = (const int64_t*)at(kOpObjTs);
    db.op_key_off = (const uint64_t*)at(kOpKeyOff);
    db.op_key_len = (const uint32_t*)at(kOpKeyLen);
    mochi_verdicts dv;
    memset(&dv, 0, sizeof dv);
    dv.grant_flags = (uint8_t*)hp.dev_out(kOutFlags) + k.g0;
    dv.grant_ts = o->grant_ts ? (int64_t*)hp.dev_out(kOutTs) + k.g0 : nullptr;
    dv.cert_accept_bits = (uint32_t*)hp.dev_out(kOutAcc) + k.c0 / 32;
    dv.cert_reason = o->cert_reason ? (uint8_t*)hp.dev_out(kOutReason) + k.c0 : nullptr;
    dv.cert_fail_op = o->cert_fail_op ? (uint8_t*)hp.dev_out(kOutFail) + k.c0 : nullptr;
    dv.op_decision = o->op_decision ? (uint8_t*)hp.dev_out(kOutDec) + k.o0 : nullptr;
    dv.op_g0 = o->op_g0 ? (uint32_t*)hp.dev_out(kOutG0) + k.o0 : nullptr;
    dv.op_ts = o->op_ts ? (int64_t*)hp.dev_out(kOutOpTs) + k.o0 : nullptr;
    if ((rc = run_device(c, &db, p, &dv, c->stream))) return rc;
    if (j + 1 == nchunks && o->grant_valid_bits && N)
      HIP_TRY(mochi::launch_pack_bits((uint8_t*)hp.dev_out(kOutFlags), N, MOCHI_GRANT_SIG_OK,
                                      (uint32_t*)hp.dev_out(kOutGrantBits), c->stream));
    const uint32_t units[3][2] = {{k.g0, k.g1}, {k.c0, k.c1}, {k.o0, k.o1}};
    if ((rc = hp.download(j, j + 1 == nchunks, units))) return rc;
  }
  return hp.end();
}

}  // namespace

void mochi::par_memcpy(void* dst, const void* src, size_t n) {
  constexpr size_t kPar = 8u << 20;
  if (n < kPar) {
    memcpy(dst, src, n);
    return;
  }
  const unsigned hw = std::thread::hardware_concurrency();
  const unsigned nt = hw < 2 ? 1 : hw > 8 ? 8 : hw;
  const size_t per = (n + nt - 1) / nt;
  std::vector<std::thread> th;
  for (unsigned t = 1; t < nt; t++) {
    const size_t lo = t * per;
    if (lo >= n) break;
    const size_t len = per < n - lo ? per : n - lo;
    th.emplace_back([=] { memcpy((char*)dst + lo, (const char*)src + lo, len); });
  }
  memcpy(dst, src, per < n ? per : n);
  for (auto& x : th) x.join();
}

extern "C" {

int mochi_verify_batch(mochi_ctx* c, const mochi_batch* b, const mochi_params* p, mochi_verdicts* o) {
  int rc = check_batch_header(c, b, p, o);
  if (rc) return rc;
  if ((rc = check_batch_host(b))) return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard dev(c->device);
  if (!dev.ok) return fail(MOCHI_EHIP, "hipSetDevice(%d)", c->device);
  new_call(c);
  return run_host_pipeline(c, b, p, o);
}

// ---- Write2 wire path: the messages the device decoder declines -------------
//
// MOCHI_MSG_FALLBACK messages (repeated / merged fields, non-canonical Grant
// bytes, more than 32 MultiGrants or 64 grants per MultiGrant) are decoded on
// the host with full protobuf-java semantics (w2_host.cpp) into an SoA batch and
// verified through the same device path as every other certificate; their
// verdicts replace the UNDECIDED placeholder.  Messages the host decoder cannot
// express (more than MOCHI_MAX_OPS_PER_CERT operations, a grant over 64 KiB,
// op_flags_off disagreeing with the operation count) stay UNDECIDED.
static int decide_fallback(mochi_ctx* c, const mochi_write2_batch* w, const mochi_params* p, mochi_verdicts* o,
                           const std::vector<uint32_t>& msgs) {
  const uint32_t* ofo = w->op_flags_off;
  std::vector<uint32_t> take;
  std::vector<mochi_host::Message> dec;
  for (uint32_t m : msgs) {
    mochi_host::Message d;
    if (mochi_host::decode_full(w->wire + w->msg_off[m], w->msg_len[m], c->server_ids, d) != MOCHI_MSG_OK) continue;
    if (ofo && ofo[m + 1] - ofo[m] != d.ops.size()) continue;
    bool fits = true;
    for (auto& mg : d.mgs)
      for (auto& g : mg.grants) fits &= g.bytes.size() <= 65536;
    if (!fits) continue;
    take.push_back(m);
    dec.push_back(std::move(d));
  }
  if (take.empty()) return MOCHI_OK;
  std::vector<uint8_t> blob, sig, gkey, opk, opf, hashes;
  std::vector<uint64_t> goff, okoff;
  std::vector<uint32_t> glen, cgo{0}, coo{0}, cmo{0}, mgo{0}, oklen;
  std::vector<uint16_t> signer;
  std::vector<int64_t> ots;
  for (size_t i = 0; i < take.size(); i++) {
    const uint32_t m = take[i];
    const mochi_host::Message& d = dec[i];
    for (auto& mg : d.mgs) {
      for (auto& g : mg.grants) {
        goff.push_back(blob.size());
        glen.push_back((uint32_t)g.bytes.size());
        blob.insert(blob.end(), g.bytes.begin(), g.bytes.end());
        sig.insert(sig.end(), g.sig, g.sig + MOCHI_RSA_BYTES);
        signer.push_back(mg.signer);
        gkey.push_back(g.slot);
      }
      mgo.push_back((uint32_t)goff.size());
    }
    cmo.push_back((uint32_t)mgo.size() - 1);
    cgo.push_back((uint32_t)goff.size());
    for (size_t j = 0; j < d.ops.size(); j++) {
      const auto& op = d.ops[j];
      opk.push_back(op.slot);
      const uint8_t fl = ofo ? w->op_flags[ofo[m] + j] : (uint8_t)(MOCHI_OP_LOCAL | MOCHI_OP_HAS_SVOC);
      opf.push_back((uint8_t)(fl | (op.not_write ? MOCHI_OP_NOT_WRITE : 0)));
      ots.push_back(ofo && w->op_object_ts ? w->op_object_ts[ofo[m] + j] : 0);
      okoff.push_back(blob.size());
      oklen.push_back((uint32_t)op.key_bytes.size());
      blob.insert(blob.end(), op.key_bytes.begin(), op.key_bytes.end());
    }
    coo.push_back((uint32_t)opk.size());
    hashes.insert(hashes.end(), w->expected_hash + (size_t)m * MOCHI_TXN_HASH_BYTES,
                  w->expected_hash + (size_t)(m + 1) * MOCHI_TXN_HASH_BYTES);
  }
  if (blob.empty()) blob.push_back(0);
  mochi_batch b;
  memset(&b, 0, sizeof b);
  b.n_grants = (uint32_t)goff.size();
  b.n_certs = (uint32_t)take.size();
  b.n_ops = (uint32_t)opk.size();
  b.n_mgs = (uint32_t)mgo.size() - 1;
  b.grant_bytes_len = blob.size();
  b.grant_bytes = blob.data();
  b.grant_off = goff.data();
  b.grant_len = glen.data();
  b.sig = sig.data();
  b.signer = signer.data();
  b.grant_key = gkey.data();
  b.cert_grant_off = cgo.data();
  b.cert_op_off = coo.data();
  b.op_key = opk.data();
  b.op_flags = opf.data();
  b.expected_hash = hashes.data();
  b.cert_mg_off = cmo.data();
  b.mg_grant_off = mgo.data();
  b.op_object_ts = ots.data();
  b.op_key_off = okoff.data();
  b.op_key_len = oklen.data();
  const size_t C = take.size(), O = opk.size();
  std::vector<uint32_t> acc((C + 31) / 32), og0(O + 1);
  std::vector<uint8_t> reason(C), fail(C), odec(O + 1);
  std::vector<int64_t> ots_out(O + 1);
  mochi_verdicts v;
  memset(&v, 0, sizeof v);
  v.cert_accept_bits = acc.data();
  v.cert_reason = reason.data();
  v.cert_fail_op = fail.data();
  v.op_decision = odec.data();
  v.op_g0 = og0.data();
  v.op_ts = ots_out.data();
  resolve_timing(c);
  float saved[4] = {c->last_ms[0], c->last_ms[1], c->last_ms[2], c->last_total_ms};
  const int rc = run_host_pipeline(c, &b, p, &v);
  c->last_ms[0] = saved[0], c->last_ms[1] = saved[1], c->last_ms[2] = saved[2], c->last_total_ms = saved[3];
  c->timing_pending = false;
  if (rc) return rc;
  for (size_t i = 0; i < C; i++) {
    const uint32_t m = take[i];
    const bool a = (acc[i >> 5] >> (i & 31)) & 1u;
    if (a) o->cert_accept_bits[m >> 5] |= 1u << (m & 31);
    else o->cert_accept_bits[m >> 5] &= ~(1u << (m & 31));
    if (o->cert_reason) o->cert_reason[m] = reason[i];
    if (o->cert_fail_op) o->cert_fail_op[m] = fail[i];
    if (ofo)
      for (uint32_t j = 0; j < coo[i + 1] - coo[i]; j++) {
        const size_t src = coo[i] + j, dst = ofo[m] + j;
        if (o->op_decision) o->op_decision[dst] = odec[src];
        if (o->op_g0) o->op_g0[dst] = og0[src];
        if (o->op_ts) o->op_ts[dst] = ots_out[src];
      }
  }
  return MOCHI_OK;
}

// ---- Write2 wire path, host memory: chunked pipeline -------------------------
//
// Messages are cut into chunks of whole messages (multiples of 32, so each
// chunk's accept bits start on a word) of ~chunk_grants * 256 wire bytes.
// For chunk j:
// stage + upload (copy-in stream), then on the context stream the decode count
// phase and its totals; chunk j-2's emit + verify + fix-up is enqueued once ITS
// totals are on the host, so the host waits only for count kernels while the
// device verifies earlier chunks and the copy engines move the next one.
// Verdicts come down per chunk on the copy-out stream.
//
// Input segments of one chunk (op_flags_off is rebased per chunk, so always staged)
// and the output slices in download order.
enum W2Seg { kW2Wire, kW2MsgOff, kW2MsgLen, kW2OpFlagsOff, kW2OpFlags, kW2OpObjTs, kW2ExpHash, kNumW2Seg };
enum W2Out { kW2Acc, kW2Reason, kW2Fail, kW2Status, kW2Dec, kW2G0, kW2OpTs, kNumW2Out };

static int verify_write2_host(mochi_ctx* c, const mochi_write2_batch* w, const mochi_params* p, mochi_verdicts* o,
                              uint8_t* msg_status, mochi_write2_decoded* dec, uint32_t** same = nullptr) {
  constexpr size_t kW2Lag = 2;  // chunks counted ahead of the one being verified
  int rc;
  const uint32_t M = w->n_msgs;
  for (uint32_t m = 0; m < M; m++)
    if (w->msg_off[m] > w->wire_len || w->msg_len[m] > w->wire_len - w->msg_off[m])
      return fail(MOCHI_EINVAL, "message %u lies outside wire", m);
  if (w->op_flags_off) {  // the device trusts these offsets: validate them here
    if (w->op_flags_off[0] != 0) return fail(MOCHI_EINVAL, "op_flags_off[0] must be 0");
    for (uint32_t m = 0; m < M; m++)
      if (w->op_flags_off[m + 1] < w->op_flags_off[m]) return fail(MOCHI_EINVAL, "op_flags_off decreases at %u", m);
  }
  if (c->n_ids != c->n_keys) return fail(MOCHI_EINVAL, "server ids not set (mochi_ctx_set_server_ids)");
  std::lock_guard<std::mutex> lk(c->mu);
  new_call(c);
  DeviceGuard dev(c->device);
  if (!dev.ok) return fail(MOCHI_EHIP, "hipSetDevice(%d)", c->device);
  const uint32_t* ofo = w->op_flags_off;
  const size_t O_in = ofo ? ofo[M] : 0;
  // ~67 MB of wire bytes per chunk at the default chunk_grants (measured on one
  // box, 250k messages: 45.5 GB/s at 67 MB, 43.5 at 134 MB, 40.3 at 34 MB; a
  // ramp of smaller chunks at fill and drain measured 37.7: every chunk pays
  // the verify path's latency floor, ~0.6 ms, whatever its size)
  const uint64_t target = dec ? UINT64_MAX : (uint64_t)c->chunk_grants * 256;
  // reason, fail-op and status always come down (the status decides the fallback)
  OutSlice out[kNumW2Out] = {{o->cert_accept_bits, 4, kAccWord},
                             {o->cert_reason, 1, kPerCert, true},
                             {o->cert_fail_op, 1, kPerCert, true},
                             {msg_status, 1, kPerCert, true, 1},
                             {o->op_decision, 1, kPerOp},
                             {o->op_g0, 4, kPerOp},
                             {o->op_ts, 8, kPerOp}};
  HostPipe hp(c, kNumW2Seg, out, kNumW2Out, 0, M, O_in);
  struct Chunk {
    uint32_t m0, m1;
    ByteRange wire;
    size_t cnt;  // its decode scratch, bytes into w2_cnt
    SegIn seg[kNumW2Seg];
    mochi_write2_batch dw;  // the chunk on the device
    mochi::W2Args args;
  };
  std::vector<Chunk> ch;
  size_t cnt_total = 0;
  auto weight = [&](uint32_t lo, uint32_t hi) {
    return std::accumulate(w->msg_len + lo, w->msg_len + hi, uint64_t{0});
  };
  plan_chunks(M, target, weight, [&](uint32_t m0, uint32_t m1) {
    ch.push_back({m0, m1, {}, cnt_total, {}, {}, {}});
    Chunk& k = ch.back();
    k.wire.add(w->msg_off, w->msg_len, m0, m1);
    k.args.M = m1 - m0;
    cnt_total += mochi::w2_count_layout(k.args, nullptr);
    const size_t nm = m1 - m0, no = ofo ? ofo[m1] - ofo[m0] : 0;
    const bool ots = ofo && w->op_object_ts;
    SegIn* s = k.seg;
    s[kW2Wire] = {(size_t)(k.wire.hi - k.wire.lo), w->wire + k.wire.lo};
    s[kW2MsgOff] = {8 * nm, w->msg_off + m0};
    s[kW2MsgLen] = {4 * nm, w->msg_len + m0};
    s[kW2OpFlagsOff] = {ofo ? 4 * (nm + 1) : 0, nullptr};
    s[kW2OpFlags] = {no, ofo ? w->op_flags + ofo[m0] : nullptr};
    s[kW2OpObjTs] = {ots ? 8 * no : 0, ots ? w->op_object_ts + ofo[m0] : nullptr};
    s[kW2ExpHash] = {(size_t)MOCHI_TXN_HASH_BYTES * nm, w->expected_hash + (size_t)MOCHI_TXN_HASH_BYTES * m0};
    for (SegIn& x : k.seg) x.off = hp.in.take(x.bytes);
  });
  const size_t nch = ch.size();
  if ((rc = c->w2_cnt.ensure(cnt_total)) || (rc = c->w2_tot.ensure(16 * nch)) ||
      (rc = ensure_events(c->tot_ev, nch)))
    return rc;
  uint32_t* tot = (uint32_t*)c->w2_tot.p;
  hipStream_t st = c->stream;
  // One small chunk (a batcher flush): every segment staged and ONE upload and
  // ONE download of the whole region -- a copy costs ~5 us of its own on the
  // GPU whatever its size, and a 2-message batch moved 5 + 7 of them.
  hp.one_up = hp.one_down = nch == 1 && hp.in.total <= (4u << 20);
  // ... and both copies on the launch stream: nothing to overlap them with, and
  // a cross-stream hand-off is one more event record, wait and barrier packet
  hp.on_st = hp.one_up && !copy_streams();  // MOCHI_COPY_STREAMS=1 (A/B): the copy streams anyway
  HIP_TRY(scratch_acquire(c, st));
  if ((rc = hp.start(nch, ch[0].seg))) return rc;
  // phase 2 + download of chunk j (its totals must be on the host)
  auto finish = [&](size_t j) -> int {
    Chunk& k = ch[j];
    HIP_TRY(hipEventSynchronize(c->tot_ev[j]));
    const uint32_t* t = tot + 4 * j;
    const uint32_t o0 = ofo ? ofo[k.m0] : 0;
    mochi_verdicts dv;
    memset(&dv, 0, sizeof dv);
    dv.cert_accept_bits = (uint32_t*)hp.dev_out(kW2Acc) + k.m0 / 32;
    dv.cert_reason = (uint8_t*)hp.dev_out(kW2Reason) + k.m0;
    dv.cert_fail_op = (uint8_t*)hp.dev_out(kW2Fail) + k.m0;
    dv.op_decision = o->op_decision ? (uint8_t*)hp.dev_out(kW2Dec) + o0 : nullptr;
    dv.op_g0 = o->op_g0 ? (uint32_t*)hp.dev_out(kW2G0) + o0 : nullptr;
    dv.op_ts = o->op_ts ? (int64_t*)hp.dev_out(kW2OpTs) + o0 : nullptr;
    int r = w2_verify(c, &k.dw, p, &dv, k.args, t[0], t[1], t[2], k.dw.op_flags_off, st, dec != nullptr);
    if (r) return r;
    if (dec) return MOCHI_OK;
    const uint32_t units[3][2] = {{0, 0}, {k.m0, k.m1}, {o0, ofo ? ofo[k.m1] : 0}};
    return hp.download(j, j + 1 == nch, units);
  };
  for (size_t j = 0; j < nch; j++) {
    Chunk& k = ch[j];
    const SegIn* s = k.seg;
    if (ofo) {
      uint32_t* f = (uint32_t*)hp.stage(s[kW2OpFlagsOff]);
      for (uint32_t m = k.m0; m <= k.m1; m++) f[m - k.m0] = ofo[m] - ofo[k.m0];
    }
    if ((rc = hp.upload(j, s))) return rc;
    mochi_write2_batch& dw = k.dw;
    dw.n_msgs = k.m1 - k.m0;
    dw.wire_len = k.wire.hi;
    dw.wire = hp.dev(s[kW2Wire]) - k.wire.lo;  // message offsets stay absolute
    dw.msg_off = (const uint64_t*)hp.dev(s[kW2MsgOff]);
    dw.msg_len = (const uint32_t*)hp.dev(s[kW2MsgLen]);
    dw.op_flags_off = ofo ? (const uint32_t*)hp.dev(s[kW2OpFlagsOff]) : nullptr;
    dw.op_flags = ofo ? hp.dev(s[kW2OpFlags]) : nullptr;
    dw.op_object_ts = s[kW2OpObjTs].bytes ? (const int64_t*)hp.dev(s[kW2OpObjTs]) : nullptr;
    dw.expected_hash = hp.dev(s[kW2ExpHash]);
    if ((rc = w2_count(c, &dw, (uint8_t*)hp.dev_out(kW2Status) + k.m0, c->w2_cnt.as<uint8_t>() + k.cnt, tot + 4 * j,
                       c->tot_ev[j], st, &k.args)))
      return rc;
    // the verify of chunk j - kW2Lag: its totals are read on the host, so the
    // host waits for its count; with two chunks of lag the stream still holds
    // work while it waits
    if (j >= kW2Lag && (rc = finish(j - kW2Lag))) return rc;
  }
  for (size_t j = nch > kW2Lag ? nch - kW2Lag : 0; j < nch; j++)
    if ((rc = finish(j))) return rc;
  HIP_TRY(scratch_release(c, st));
  if (dec) {
    // decode-only (one chunk): copy the decoded SoA back (tests / inspection)
    const mochi::W2Args& da = ch[0].args;
    const uint32_t N = tot[0], O = tot[1], NM = tot[2];
    dec->n_msgs = M;
    dec->n_grants = N;
    dec->n_ops = O;
    dec->n_mgs = NM;
    dec->grant_off = (uint64_t*)malloc(8 * (size_t)N + 8);
    dec->grant_len = (uint32_t*)malloc(4 * (size_t)N + 4);
    dec->sig = (uint8_t*)malloc((size_t)MOCHI_RSA_BYTES * N + 1);
    dec->signer = (uint16_t*)malloc(2 * (size_t)N + 2);
    dec->grant_key = (uint8_t*)malloc((size_t)N + 1);
    dec->cert_grant_off = (uint32_t*)malloc(4 * ((size_t)M + 1));
    dec->cert_op_off = (uint32_t*)malloc(4 * ((size_t)M + 1));
    dec->op_key = (uint8_t*)malloc((size_t)O + 1);
    dec->op_flags = (uint8_t*)malloc((size_t)O + 1);
    dec->msg_status = (uint8_t*)malloc((size_t)M + 1);
    dec->cert_mg_off = (uint32_t*)malloc(4 * ((size_t)M + 1));
    dec->mg_grant_off = (uint32_t*)malloc(4 * ((size_t)NM + 1));
    dec->op_key_off = (uint64_t*)malloc(8 * (size_t)O + 8);
    dec->op_key_len = (uint32_t*)malloc(4 * (size_t)O + 4);
    struct {
      void* dst;
      const void* src;
      size_t n;
    } cp[] = {{dec->grant_off, da.grant_off, 8 * (size_t)N},     {dec->grant_len, da.grant_len, 4 * (size_t)N},
              {dec->sig, da.sig, (size_t)MOCHI_RSA_BYTES * N},   {dec->signer, da.signer, 2 * (size_t)N},
              {dec->grant_key, da.grant_key, N},                 {dec->cert_grant_off, da.cert_grant_off, 4 * ((size_t)M + 1)},
              {dec->cert_op_off, da.cert_op_off, 4 * ((size_t)M + 1)}, {dec->op_key, da.op_key, O},
              {dec->op_flags, da.op_flags, O},                   {dec->msg_status, da.status, M},
              {dec->cert_mg_off, da.cert_mg_off, 4 * ((size_t)M + 1)}, {dec->mg_grant_off, da.mg_grant_off, 4 * ((size_t)NM + 1)},
              {dec->op_key_off, da.op_key_off, 8 * (size_t)O},   {dec->op_key_len, da.op_key_len, 4 * (size_t)O}};
    for (auto& x : cp)
      if (x.n) HIP_TRY(hipMemcpyAsync(x.dst, x.src, x.n, hipMemcpyDeviceToHost, st));
    if (same) {
      // the first-grant hint as prep reads it: indices relative to the launch, and the
      // decode-only call is one launch (target above), so they are batch-global as they are
      *same = (uint32_t*)malloc(4 * (size_t)N + 4);
      if (N) HIP_TRY(hipMemcpyAsync(*same, da.grant_same, 4 * (size_t)N, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return MOCHI_OK;
  }
  if ((rc = hp.end())) return rc;
  std::vector<uint32_t> fallback;
  const uint8_t* status = (const uint8_t*)c->pin_out.p + out[kW2Status].off;
  for (uint32_t m = 0; m < M; m++)
    if (status[m] == MOCHI_MSG_FALLBACK) fallback.push_back(m);
  if (fallback.empty()) return MOCHI_OK;
  rc = decide_fallback(c, w, p, o, fallback);
  c->acc_dev = nullptr;  // the host decided some verdicts (and the fallback batch reused dev_out)
  c->acc_words = 0;
  return rc;
}

int mochi_verify_write2(mochi_ctx* c, const mochi_write2_batch* w, const mochi_params* p, mochi_verdicts* o,
                        uint8_t* msg_status) {
  int rc = check_write2_header(c, w, p, o);
  if (rc) return rc;
  return verify_write2_host(c, w, p, o, msg_status, nullptr);
}

int mochi_write2_decode(mochi_ctx* c, const mochi_write2_batch* w, mochi_write2_decoded* out) {
  return mochi_write2_decode_same(c, w, out, nullptr);
}

int mochi_write2_decode_same(mochi_ctx* c, const mochi_write2_batch* w, mochi_write2_decoded* out,
                             uint32_t** grant_same) {
  if (!out) return fail(MOCHI_EINVAL, "null argument");
  memset(out, 0, sizeof *out);
  if (grant_same) *grant_same = nullptr;
  mochi_params p = {1, 1, 0, 0};
  mochi_verdicts o;
  memset(&o, 0, sizeof o);
  uint32_t dummy = 0;
  o.cert_accept_bits = &dummy;
  int rc = check_write2_header(c, w, &p, &o);
  if (rc) return rc;
  return verify_write2_host(c, w, &p, &o, nullptr, out, grant_same);
}

void mochi_write2_same_free(uint32_t* grant_same) { free(grant_same); }

void mochi_write2_decoded_free(mochi_write2_decoded* d) {
  if (!d) return;
  free(d->grant_off);
  free(d->grant_len);
  free(d->sig);
  free(d->signer);
  free(d->grant_key);
  free(d->cert_grant_off);
  free(d->cert_op_off);
  free(d->op_key);
  free(d->op_flags);
  free(d->msg_status);
  free(d->cert_mg_off);
  free(d->mg_grant_off);
  free(d->op_key_off);
  free(d->op_key_len);
  memset(d, 0, sizeof *d);
}

}  // extern "C"
