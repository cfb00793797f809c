// ctx.h — what capi.cpp and host_path.cpp share: the error slot, growable device and
// pinned buffers, the context itself, and the device-side steps the host paths drive.
#pragma once
#include <mutex>
#include <string>
#include <vector>

#include "kernels.h"
#include "w2.h"
#include "w2_encode.h"

namespace mochi {

// sets this thread's mochi_last_error text; returns code
int fail(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                                               \
  do {                                                                                              \
    hipError_t e_ = (expr);                                                                         \
    if (e_ != hipSuccess) return mochi::fail(MOCHI_EHIP, "%s: %s", #expr, hipGetErrorString(e_));   \
  } while (0)

// Growable device allocation.
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  int ensure(size_t bytes) {
    if (bytes <= cap) return MOCHI_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    size_t want = bytes < 256 ? 256 : bytes;
    if (hipMalloc(&p, want) != hipSuccess) return fail(MOCHI_ENOMEM, "hipMalloc(%zu) failed", want);
    cap = want;
    return MOCHI_OK;
  }
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  template <typename T>
  T* as() const {
    return static_cast<T*>(p);
  }
};

struct PinnedBuf {
  void* p = nullptr;
  size_t cap = 0;
  int ensure(size_t bytes) {
    if (bytes <= cap) return MOCHI_OK;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    size_t want = bytes < 4096 ? 4096 : bytes + bytes / 4;
    if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess)
      return fail(MOCHI_ENOMEM, "hipHostMalloc(%zu) failed", want);
    cap = want;
    return MOCHI_OK;
  }
  ~PinnedBuf() {
    if (p) (void)hipHostFree(p);
  }
};

// What one wire encoder (w2_encode.hip, w1_issue.hip, w1_reply.hip, result_encode.hip) keeps between calls.
struct EncState {
  DevBuf scratch, scan;        // per-call scratch; temp of the device-wide scan
  PinnedBuf tot;               // the totals the host waits for
  std::vector<hipEvent_t> ev;  // per-kernel events of the last call made while profiling, created on first use
  bool ev_valid = false;       // ev holds a whole call: read_profile may read it
  // scan_n: elements of the device-wide 64-bit scan, 0 on the single-block path (no temp)
  int prepare(size_t scratch_bytes, uint32_t scan_n, size_t tot_bytes) {
    size_t scan_bytes = 0;
    if (scan_n) HIP_TRY(mochi::enc_scan_temp_bytes(scan_n, &scan_bytes));
    int rc;
    if ((rc = scratch.ensure(scratch_bytes)) || (rc = scan.ensure(scan_bytes))) return rc;
    return tot.ensure(tot_bytes);
  }
  // *out = n events to stamp while profiling, null otherwise
  int events(bool profiling, int n, hipEvent_t** out) {
    ev_valid = false;
    *out = nullptr;
    while (profiling && ev.size() < (size_t)n) {
      hipEvent_t e;
      HIP_TRY(hipEventCreate(&e));
      ev.push_back(e);
    }
    if (profiling) *out = ev.data();
    return MOCHI_OK;
  }
  // all a call needs before its first launch: the buffers, a's scratch pointers through the
  // encoder's one layout function, its scan temp and its events
  template <class Args>
  int begin(Args& a, size_t (*layout)(Args&, void*), uint32_t scan_n, size_t tot_bytes, bool profiling, int n_ev) {
    int rc;
    if ((rc = prepare(layout(a, nullptr), scan_n, tot_bytes)) || (rc = events(profiling, n_ev, &a.ev))) return rc;
    a.scan_temp = scan.p;
    a.scan_temp_bytes = scan.cap;
    layout(a, scratch.p);
    return MOCHI_OK;
  }
  // the totals the size phase left at `dev`, in tot.p once this returns
  int fetch_totals(const void* dev, size_t bytes, hipEvent_t ev_tot, hipStream_t st) {
    HIP_TRY(hipMemcpyAsync(tot.p, dev, bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(ev_tot, st));
    HIP_TRY(hipEventSynchronize(ev_tot));
    return MOCHI_OK;
  }
  // kernel_ms[i] = time between events span[i][0] and span[i][1] of the last profiled call
  int read_profile(const int (*span)[2], int n_stages, float* kernel_ms, uint32_t n, const char* none_msg) {
    if (!ev_valid) return fail(MOCHI_EINVAL, "%s", none_msg);
    if (hipEventSynchronize(ev.back()) != hipSuccess) return fail(MOCHI_EHIP, "hipEventSynchronize failed");
    for (uint32_t i = 0; i < n; i++) {
      kernel_ms[i] = 0.f;
      if (i < (uint32_t)n_stages) (void)hipEventElapsedTime(&kernel_ms[i], ev[span[i][0]], ev[span[i][1]]);
    }
    return MOCHI_OK;
  }
  ~EncState() {
    for (auto e : ev) (void)hipEventDestroy(e);
  }
};

// Scratch ordering across calls and streams: every launch that uses its owner's scratch
// waits for the previous one to be done with it (the device entry points are async on a
// caller-chosen stream, so two calls on different streams would otherwise race on it).
struct ScratchOrder {
  hipEvent_t ev = nullptr;  // created and destroyed by the owner
  bool used = false;
  hipStream_t st = nullptr;  // the stream ev was last recorded on
  hipError_t acquire(hipStream_t s) {
    // on the stream that last released the scratch, stream order already holds
    // (a wait there is one more API call and barrier packet per small batch)
    return used && st != s ? hipStreamWaitEvent(s, ev, 0) : hipSuccess;
  }
  hipError_t release(hipStream_t s) {
    used = true;
    st = s;
    return hipEventRecord(ev, s);
  }
};

// the device of a context or signer for one call; the caller's device again on return
struct DeviceGuard {
  int save = 0;
  bool ok;
  explicit DeviceGuard(int device) {
    (void)hipGetDevice(&save);
    ok = hipSetDevice(device) == hipSuccess;
  }
  ~DeviceGuard() {
    if (ok) (void)hipSetDevice(save);
  }
};

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

}  // namespace mochi

struct mochi_ctx {
  // batchers built on this context (mochi_batcher_create*) hold it until they
  // are freed -- a batcher destroyed from its own callback is freed later by
  // its last flusher thread, which still uses the context's streams and pinned
  // buffers until then.  mochi_ctx_destroy with a holder left never blocks: it
  // marks the context and the last holder's release frees it.
  std::mutex ref_mu;
  int batcher_refs = 0;
  bool destroy_pending = false;
  int device = 0;
  hipStream_t stream = nullptr;
  uint32_t n_keys = 0;
  mochi::KeyEntry* d_keys = nullptr;
  mochi::FoldKey* d_fold = nullptr;  // per-key k_rsa_pow fold matrices (~101 KB each)
  std::mutex mu;
  mochi::DevBuf scratch;  // verify scratch (verify_layout, kernels.h)
  // host-path device copies
  mochi::DevBuf dev_in, dev_out;
  mochi::PinnedBuf pin_in, pin_out;
  hipStream_t s_in = nullptr, s_out = nullptr;  // host-path copy streams
  hipStream_t aux = nullptr;                     // grant prep (high priority), beside k_rsa_pow
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  mochi::ScratchOrder order;  // over scratch and the decode and encode buffers
  std::vector<hipEvent_t> chunk_ev;              // host-path chunk hand-offs
  std::vector<hipEvent_t> tot_ev;                // wire host path: per-chunk decode totals on the host
  // two sets of the host-path call's span events: a call records into one while
  // the other keeps the last completed call's, read only when asked
  hipEvent_t evs[2][4] = {{nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr}};
  hipEvent_t* ev = evs[0];   // the set of the call in progress
  int ev_set = 0, ev_done = 0;  // ev's set; the last completed call's
  float last_ms[3] = {0, 0, 0};  // first upload, compute span, last download of the last host-path call
  float last_total_ms = 0;       // whole pipelined host-path call (first H2D start -> last D2H end)
  bool timing_pending = false;   // ev[0..3] recorded, last_ms not yet read from them (resolve_timing)
  uint32_t chunk_grants = 0;     // host-path chunk target (grants), mochi_ctx_set_chunk_grants
  uint32_t small_grants = 4096;  // small-batch launch sequence up to this many grants (mochi_ctx_set_small_batch)
  // Write2 wire path: server-id table + decode scratch
  mochi::DevBuf ids, id_off;
  uint32_t n_ids = 0;
  std::vector<std::string> server_ids;  // host copy for the fallback decoder (w2_host.cpp)
  mochi::DevBuf w2_cnt, w2_status, w2_scan, w2_out;  // w2_cnt: w2_count_layout per chunk; w2_out: w2_emit_layout
  mochi::PinnedBuf w2_tot;
  hipEvent_t ev_tot = nullptr;
  mochi::EncState w2e;  // Write2 encoder (w2_encode.hip); its total is the wire size
  mochi::EncState w1d;  // Write1 reply decoder (w1_decode.hip); its totals are the grant and certificate counts
  mochi::DevBuf w1d_sig;  // ... and its signature sources, sized once the grant total is known
  mochi::EncState rr;   // result reply decoder (result_decode.hip); it waits for no total
  mochi::EncState rae;  // answer encoder (result_encode.hip); its total is the wire size
  // read request decoder (read_request.hip): the per-request scratch, its total is n_ops; the
  // per-op scratch (claim table, key numbering) is sized once n_ops is known
  mochi::EncState rdq;
  mochi::DevBuf rdq_tab;
  // envelope codec (envelope.hip), one state per call so that each keeps its last profile:
  // decode (events alone), route, join (its `scan` is the radix sort's temp), encode
  mochi::EncState env_dec, env_route, env_join, env_enc;
  // the last host-path call's certificate accept bitmap on the device (a slice
  // of dev_out, valid until the next call on this context; nullptr when the
  // device copy is not the final verdict, e.g. after host fallback decisions):
  // multi.cpp all-gathers it in place of re-uploading the host bits
  const uint32_t* acc_dev = nullptr;
  uint32_t acc_words = 0;
  uint64_t gen = 0;  // bumped (under mu) by every call that may rewrite dev_out / scratch
  // per-stage profiling (mochi_ctx_set_profiling): one event set per verify call
  bool profiling = false;
  std::vector<std::vector<hipEvent_t>> prof_sets;
};

namespace mochi {

// every entry point that launches on the context's buffers, with c->mu held
void new_call(mochi_ctx* c);
void resolve_timing(mochi_ctx* c);
// Scratch ordering across calls and streams (ScratchOrder).
inline hipError_t scratch_acquire(mochi_ctx* c, hipStream_t st) { return c->order.acquire(st); }
inline hipError_t scratch_release(mochi_ctx* c, hipStream_t st) { return c->order.release(st); }
int check_batch_header(const mochi_ctx* c, const mochi_batch* b, const mochi_params* p, const mochi_verdicts* o);
int check_write2_header(const mochi_ctx* c, const mochi_write2_batch* w, const mochi_params* p,
                        const mochi_verdicts* o);
int ensure_scratch(mochi_ctx* c, uint32_t N, uint32_t C);
int run_device(mochi_ctx* c, const mochi_batch* b, const mochi_params* p, mochi_verdicts* o, hipStream_t st,
               const uint32_t* op_out_off = nullptr, const uint32_t* grant_same = nullptr,
               const uint8_t* msg_status = nullptr);
int w2_count(mochi_ctx* c, const mochi_write2_batch* w, uint8_t* status, void* cnt, uint32_t* tot_host,
             hipEvent_t ev_tot, hipStream_t st, W2Args* a);
int w2_verify(mochi_ctx* c, const mochi_write2_batch* w, const mochi_params* p, mochi_verdicts* o, W2Args& a,
              uint32_t N, uint32_t O, uint32_t NM, const uint32_t* op_out_off, hipStream_t st, bool decode_only);
// host_path.cpp
void par_memcpy(void* dst, const void* src, size_t n);

}  // namespace mochi
