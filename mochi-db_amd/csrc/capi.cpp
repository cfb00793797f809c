// capi.cpp — libmochi_hip C ABI (include/mochi_hip.h): contexts, key tables,
// device scratch, host<->device staging, and the client-side tally.
//
// The verify path it drives replaces, in the reference,
//   InMemoryDataStore.processWrite2ToServer  (InMemoryDataStore.java:641-666)
// with one batched call over many certificates.
#include <openssl/bn.h>
#include <openssl/core_names.h>
#include <openssl/evp.h>
#include <openssl/pem.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "ctx.h"
#include "envelope.h"
#include "mont.h"
#include "read_request.h"
#include "result_decode.h"
#include "result_encode.h"
#include "w1_decode.h"
#include "w1_issue.h"
#include "w1_reply.h"
#include "w1_request.h"
#include "wire_walk.h"

using namespace mochi;

static thread_local std::string g_err;

int mochi::fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

namespace {

bool prep_serial() {
  static const bool v = [] {
    const char* e = getenv("MOCHI_PREP_SERIAL");
    return e && atoi(e) != 0;
  }();
  return v;
}

bool fixup_kernel() {
  static const bool v = [] {
    const char* e = getenv("MOCHI_W2_FIXUP_KERNEL");
    return e && atoi(e) != 0;
  }();
  return v;
}

uint32_t default_chunk_grants() {
  const char* e = getenv("MOCHI_CHUNK_GRANTS");
  const long x = e ? atol(e) : 0;
  return (uint32_t)(x > 0 ? x : 262144);
}

int capacity_error(const char* cap_name, uint64_t cap, const char* need_name, uint64_t need) {
  return fail(MOCHI_EINVAL, "%s (%llu) is smaller than the %s (%llu)", cap_name, (unsigned long long)cap, need_name,
              (unsigned long long)need);
}

// ---- host-side key precompute (OpenSSL BN, setup only) --------------------

// Cpad = EMSA-PKCS1-v1_5 encoding (RFC 8017 §9.2) of SHA-256 with an all-zero
// digest: 00 01 FF..FF 00 || DigestInfo(SHA-256) || 32 zero bytes.
void pkcs1_cpad(uint8_t cpad[256]) {
  static const uint8_t kDigestInfo[19] = {0x30, 0x31, 0x30, 0x0d, 0x06, 0x09, 0x60, 0x86, 0x48, 0x01,
                                          0x65, 0x03, 0x04, 0x02, 0x01, 0x05, 0x00, 0x04, 0x20};
  memset(cpad, 0xFF, 256);
  cpad[0] = 0x00;
  cpad[1] = 0x01;
  cpad[256 - 32 - 19 - 1] = 0x00;
  memcpy(cpad + 256 - 32 - 19, kDigestInfo, 19);
  memset(cpad + 256 - 32, 0, 32);
}

int make_key_entry(const uint8_t* n_be, mochi::KeyEntry* e) {
  using namespace mochi;
  memset(e, 0, sizeof *e);
  if (!(n_be[0] & 0x80)) return fail(MOCHI_EINVAL, "modulus is not 2048 bits (top bit clear)");
  if (!(n_be[255] & 1)) return fail(MOCHI_EINVAL, "modulus is even");
  // 32-bit words, little-endian word order
  for (int i = 0; i < 64; i++) {
    const uint8_t* b = n_be + 256 - 4 * (i + 1);
    e->n32[i] = (uint32_t)b[0] << 24 | (uint32_t)b[1] << 16 | (uint32_t)b[2] << 8 | b[3];
  }
  auto to_limbs = [](const uint32_t* w, uint32_t* x) {
    for (int j = 0; j < kL; j++) {
      const int bit = j * kLimbBits, wi = bit >> 5, sh = bit & 31;
      const uint64_t lo = wi < 64 ? w[wi] : 0, hi = wi + 1 < 64 ? w[wi + 1] : 0;
      x[j] = (uint32_t)(((hi << 32) | lo) >> sh) & kLimbMask;
    }
  };
  to_limbs(e->n32, e->n);
  // n0inv = -n^{-1} mod 2^28 (Newton iteration on 32 bits)
  uint32_t inv = 1;
  for (int i = 0; i < 6; i++) inv *= 2u - e->n32[0] * inv;
  e->n0inv = (0u - inv) & kLimbMask;
  // Per-key constants (R = 2^(28*74)); k_rsa_pow leaves z = s^(2^16) mod n:
  //   kfix = R^2 mod n                           (k_rsa_raw: MontMul(MontMul(z, K), s) = s^65537)
  //   q    = R^-1 mod n                          (k_rsa_final: MontMul(z, s) = s^65537 * q)
  //   a2   = (Cpad * q mod n) + 2n               (k_rsa_final: target EM*q = Cpad*q + H*q)
  uint8_t cpad[256];
  pkcs1_cpad(cpad);
  BN_CTX* ctx = BN_CTX_new();
  BIGNUM *n = BN_bin2bn(n_be, 256, nullptr), *r = BN_new(), *k = BN_new(), *ex = BN_new(), *t = BN_new(),
         *q = BN_new(), *a2 = BN_new(), *cp = BN_bin2bn(cpad, 256, nullptr), *n2 = BN_new();
  int ok = ctx && n && r && k && ex && t && q && a2 && cp && n2;
  ok = ok && BN_set_bit(r, kL * kLimbBits) && BN_mod(r, r, n, ctx);
  ok = ok && BN_mod_mul(k, r, r, n, ctx);
  ok = ok && BN_copy(t, r) && BN_mod_inverse(q, t, n, ctx) != nullptr;
  ok = ok && BN_mod_mul(a2, cp, q, n, ctx) && BN_lshift1(n2, n) && BN_add(a2, a2, n2);
  auto to_limbs_bn = [](const BIGNUM* v, uint32_t* x) {
    uint8_t le[264];
    if (BN_bn2lebinpad(v, le, sizeof le) != (int)sizeof le) return 0;
    for (int j = 0; j < kL; j++) {
      const int bit = j * kLimbBits, by = bit >> 3, sh = bit & 7;
      uint64_t w = 0;
      for (int b = 0; b < 5; b++) w |= (uint64_t)le[by + b] << (8 * b);
      x[j] = (uint32_t)(w >> sh) & kLimbMask;
    }
    return 1;
  };
  ok = ok && to_limbs_bn(k, e->kfix) && to_limbs_bn(q, e->q) && to_limbs_bn(a2, e->a2);
  for (BIGNUM* b : {n, r, k, ex, t, q, a2, cp, n2}) BN_free(b);
  BN_CTX_free(ctx);
  if (!ok) return fail(MOCHI_EINVAL, "key precompute failed");
  return MOCHI_OK;
}

// Fold matrix of k_rsa_pow (fold.h): R_{j,b} = 2^(28(73+j)+8b) mod n as balanced
// mixed-radix digits (8, 8, 8, 4 bits per 28-bit limb), laid out as MFMA A fragments.
int make_fold_key(const uint8_t* n_be, mochi::FoldKey* f) {
  using namespace mochi;
  memset(f, 0, sizeof *f);
  static thread_local std::vector<int8_t> W;  // [296 rows][300 k]
  constexpr int kRows = kFoldLimbs * 4, kK = kFoldNH * 4;
  W.assign((size_t)kRows * kK, 0);
  BN_CTX* ctx = BN_CTX_new();
  BIGNUM *n = BN_bin2bn(n_be, 256, nullptr), *r = BN_new(), *sum = BN_new();
  int ok = ctx && n && r && sum;
  if (ok) BN_zero(sum);
  ok = ok && BN_set_bit(r, kLimbBits * kFoldF) && BN_mod(r, r, n, ctx);
  uint8_t le[264];
  for (int k = 0; k < kK && ok; k++) {
    if (k) ok = BN_lshift(r, r, (k & 3) ? 8 : 4) && BN_mod(r, r, n, ctx);  // limb = 8 + 8 + 8 + 4 bits
    if ((k & 3) != 3) ok = ok && BN_add(sum, sum, r);  // bytes 0..2 are biased, byte 3 is a signed digit
    ok = ok && BN_bn2lebinpad(r, le, sizeof le) == (int)sizeof le;
    int carry = 0;
    for (int row = 0; row < kRows && ok; row++) {
      const int bit = 28 * (row >> 2) + 8 * (row & 3), w = (row & 3) == 3 ? 4 : 8;
      const int field = (int)((((uint32_t)le[bit >> 3] | (uint32_t)le[(bit >> 3) + 1] << 8) >> (bit & 7)) & ((1u << w) - 1));
      int d = field + carry;
      carry = d >= (1 << (w - 1));
      if (carry) d -= 1 << w;
      W[(size_t)row * kK + k] = (int8_t)d;
    }
    ok = ok && carry == 0;
  }
  // cadd = 128 * sum_{j, b<3} R_{j,b} + kFoldOffN * n (fold.h) and cnc = cadd + n - Cpad
  // (k_rsa_final) as 74 limbs of 28 bits
  auto limbs = [&](const BIGNUM* v, uint32_t* out) {
    if (BN_num_bits(v) > kLimbBits * kFoldLimbs || BN_bn2lebinpad(v, le, sizeof le) != (int)sizeof le) return 0;
    for (int q = 0; q < kFoldLimbs; q++) {
      const int bit = q * kLimbBits, by = bit >> 3;
      uint64_t w = 0;
      for (int b = 0; b < 5 && by + b < (int)sizeof le; b++) w |= (uint64_t)le[by + b] << (8 * b);
      out[q] = (uint32_t)(w >> (bit & 7)) & kLimbMask;
    }
    return 1;
  };
  uint8_t cpad[256];
  pkcs1_cpad(cpad);
  BIGNUM* cp = BN_bin2bn(cpad, 256, nullptr);
  BIGNUM* off = BN_new();
  ok = ok && cp && off && BN_lshift(sum, sum, 7) && BN_set_word(off, kFoldOffN) && BN_mul(off, off, n, ctx) &&
       BN_add(sum, sum, off) && limbs(sum, f->cadd);
  BN_free(off);
  ok = ok && BN_add(sum, sum, n) && BN_sub(sum, sum, cp) && !BN_is_negative(sum) && limbs(sum, f->cnc);
  BN_free(cp);
  BN_free(n);
  BN_free(r);
  BN_free(sum);
  BN_CTX_free(ctx);
  if (!ok) return fail(MOCHI_EINVAL, "fold matrix precompute failed");
  for (int mt = 0; mt < kFoldMT; mt++)
    for (int ks = 0; ks < kFoldKS; ks++)
      for (int lane = 0; lane < 64; lane++)
        for (int jj = 0; jj < 16; jj++) {
          const int row = 32 * mt + (lane & 31), limb = 8 * ks + 4 * (lane >> 5) + jj / 4;
          if (row < kRows && limb < kFoldNH)
            f->img[((mt * kFoldKS + ks) * 64 + lane) * 16 + jj] = W[(size_t)row * kK + 4 * limb + jj % 4];
        }
  return MOCHI_OK;
}

}  // namespace

namespace mochi {
// multi.cpp: the device accept bitmap of the context's last host-path call
const uint32_t* ctx_last_accept_dev(mochi_ctx* c, uint32_t* words, int* device, hipStream_t* stream);
int set_error(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
}  // namespace mochi

namespace mochi {
// batcher.cpp: a batcher holds each of its contexts from create to its free
void ctx_hold(mochi_ctx* c) {
  std::lock_guard<std::mutex> lk(c->ref_mu);
  c->batcher_refs++;
}
void ctx_free(mochi_ctx* c);
// Nothing touches c after the unlock unless this release is the one that frees
// it (refs reached 0 with a destroy pending: no other thread may still use c).
void ctx_release(mochi_ctx* c) {
  bool free_now;
  {
    std::lock_guard<std::mutex> lk(c->ref_mu);
    free_now = --c->batcher_refs == 0 && c->destroy_pending;
  }
  if (free_now) ctx_free(c);
}

// the generation of the last context call made by this thread (multi.cpp reads it
// right after its mochi_verify_* returns, on the same thread)
thread_local uint64_t t_ctx_gen = 0;
uint64_t ctx_call_gen() { return t_ctx_gen; }

// Copies the certificate accept bitmap of context call `gen` from the device
// (where that call left it) into dst on `st`, holding the context's lock until
// the copy is done, so no later call can grow or overwrite dev_out under it.
// 1 = not available (a later call ran, the call's device bitmap is not final,
// or it lives on another device): the caller uploads its host bits instead.
int ctx_copy_accept_dev(mochi_ctx* c, uint64_t gen, int device, uint32_t* dst, uint32_t need, hipStream_t st) {
  std::lock_guard<std::mutex> lk(c->mu);
  if (c->gen != gen || !c->acc_dev || c->device != device || c->acc_words < need) return 1;
  if (hipMemcpyAsync(dst, c->acc_dev, 4 * (size_t)need, hipMemcpyDeviceToDevice, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return MOCHI_EHIP;
  return MOCHI_OK;
}
}  // namespace mochi

void mochi::new_call(mochi_ctx* c) {
  c->gen++;
  c->acc_dev = nullptr;
  c->acc_words = 0;
  mochi::t_ctx_gen = c->gen;
}

extern "C" {

int mochi_abi_version(void) { return MOCHI_ABI_VERSION; }

const char* mochi_last_error(void) { return g_err.c_str(); }

int mochi_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// The grant-prep stream runs at the highest priority, so its blocks take each
// CU the moment k_rsa_pow's block there retires (kernels.hip:launch_verify).
static hipError_t create_prep_stream(hipStream_t* s) {
  int least = 0, greatest = 0;
  if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess)
    return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
  return hipStreamCreateWithPriority(s, hipStreamNonBlocking, greatest);
}

mochi_ctx* mochi_ctx_create(int device, const uint8_t* moduli_be, uint32_t n_keys, uint32_t key_bytes,
                            uint32_t public_exponent) {
  if (!moduli_be || n_keys == 0 || n_keys > MOCHI_MAX_KEYS) {
    fail(MOCHI_EINVAL, "n_keys must be in [1, %d]", MOCHI_MAX_KEYS);
    return nullptr;
  }
  if (key_bytes != MOCHI_RSA_BYTES) {
    fail(MOCHI_EINVAL, "key_bytes must be %d (RSA-2048)", MOCHI_RSA_BYTES);
    return nullptr;
  }
  if (public_exponent != MOCHI_RSA_E) {
    fail(MOCHI_EINVAL, "public_exponent must be 65537");
    return nullptr;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    fail(MOCHI_ENODEV, "no HIP device visible");
    return nullptr;
  }
  if (device < 0 || device >= ndev) {
    fail(MOCHI_ENODEV, "device %d out of range (%d visible)", device, ndev);
    return nullptr;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    fail(MOCHI_ENODEV, "device %d is not gfx950 (%s)", device, prop.gcnArchName);
    return nullptr;
  }
  std::vector<mochi::KeyEntry> table(n_keys);
  std::vector<mochi::FoldKey> fold(n_keys);
  for (uint32_t k = 0; k < n_keys; k++)
    if (make_key_entry(moduli_be + (size_t)k * MOCHI_RSA_BYTES, &table[k]) != MOCHI_OK ||
        make_fold_key(moduli_be + (size_t)k * MOCHI_RSA_BYTES, &fold[k]) != MOCHI_OK)
      return nullptr;
  mochi_ctx* c = new mochi_ctx;
  c->device = device;
  c->n_keys = n_keys;
  c->chunk_grants = default_chunk_grants();
  DeviceGuard dev(device);
  bool ok = dev.ok && hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess &&
            hipStreamCreateWithFlags(&c->s_in, hipStreamNonBlocking) == hipSuccess &&
            create_prep_stream(&c->aux) == hipSuccess &&
            hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&c->order.ev, hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&c->ev_tot, hipEventDisableTiming) == hipSuccess &&
            hipStreamCreateWithFlags(&c->s_out, hipStreamNonBlocking) == hipSuccess &&
            hipMalloc(&c->d_keys, sizeof(mochi::KeyEntry) * n_keys) == hipSuccess &&
            hipMemcpy(c->d_keys, table.data(), sizeof(mochi::KeyEntry) * n_keys, hipMemcpyHostToDevice) == hipSuccess &&
            hipMalloc(&c->d_fold, sizeof(mochi::FoldKey) * n_keys) == hipSuccess &&
            hipMemcpy(c->d_fold, fold.data(), sizeof(mochi::FoldKey) * n_keys, hipMemcpyHostToDevice) == hipSuccess;
  for (int i = 0; i < 8 && ok; i++) ok = hipEventCreate(&c->evs[i / 4][i % 4]) == hipSuccess;
  if (!ok) {
    fail(MOCHI_EHIP, "context setup failed on device %d", device);
    mochi_ctx_destroy(c);
    return nullptr;
  }
  return c;
}

void mochi_ctx_destroy(mochi_ctx* c) {
  if (!c) return;
  {  // a batcher on this context still alive (its deferred teardown not yet done, or
     // the caller closed the context before the batcher): the last release frees it
    std::lock_guard<std::mutex> lk(c->ref_mu);
    if (c->batcher_refs > 0) {
      c->destroy_pending = true;
      return;
    }
  }
  mochi::ctx_free(c);
}

}  // extern "C"

void mochi::ctx_free(mochi_ctx* c) {
  DeviceGuard dev(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->s_out) (void)hipStreamSynchronize(c->s_out);
  for (auto& set : c->evs)
    for (auto& e : set)
      if (e) (void)hipEventDestroy(e);
  for (auto& e : c->chunk_ev) (void)hipEventDestroy(e);
  for (auto& e : c->tot_ev) (void)hipEventDestroy(e);
  if (c->aux) (void)hipStreamSynchronize(c->aux);
  if (c->s_in) (void)hipStreamDestroy(c->s_in);
  if (c->aux) (void)hipStreamDestroy(c->aux);
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  if (c->ev_join) (void)hipEventDestroy(c->ev_join);
  if (c->order.ev) (void)hipEventDestroy(c->order.ev);
  if (c->ev_tot) (void)hipEventDestroy(c->ev_tot);
  if (c->s_out) (void)hipStreamDestroy(c->s_out);
  if (c->d_keys) (void)hipFree(c->d_keys);
  if (c->d_fold) (void)hipFree(c->d_fold);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

namespace mochi {

int check_batch_header(const mochi_ctx* c, const mochi_batch* b, const mochi_params* p, const mochi_verdicts* o) {
  if (!c || !b || !p || !o) return fail(MOCHI_EINVAL, "null argument");
  if (!o->cert_accept_bits && b->n_certs) return fail(MOCHI_EINVAL, "cert_accept_bits is required");
  if (p->replication_factor == 0) return fail(MOCHI_EINVAL, "replication_factor must be > 0");
  if (b->n_grants && (!b->grant_bytes || !b->grant_off || !b->grant_len || !b->sig || !b->signer || !b->grant_key))
    return fail(MOCHI_EINVAL, "grant arrays must be non-null when n_grants > 0");
  if (!b->cert_grant_off || !b->cert_op_off) return fail(MOCHI_EINVAL, "cert_grant_off / cert_op_off required");
  if (b->n_certs && !b->expected_hash) return fail(MOCHI_EINVAL, "expected_hash required");
  if (b->n_ops && (!b->op_key || !b->op_flags)) return fail(MOCHI_EINVAL, "op arrays required");
  if ((b->cert_mg_off == nullptr) != (b->mg_grant_off == nullptr))
    return fail(MOCHI_EINVAL, "cert_mg_off and mg_grant_off go together");
  if (!b->cert_mg_off && b->n_mgs) return fail(MOCHI_EINVAL, "n_mgs must be 0 without cert_mg_off");
  if ((p->quorum_mode & MOCHI_Q_BIND) && b->n_ops && (!b->op_key_off || !b->op_key_len))
    return fail(MOCHI_EINVAL, "MOCHI_Q_BIND needs op_key_off / op_key_len");
  if (p->quorum_mode & ~(uint32_t)(MOCHI_Q_DISTINCT_SIGNERS | MOCHI_Q_BIND))
    return fail(MOCHI_EINVAL, "unknown quorum_mode bits 0x%x", p->quorum_mode);
  return MOCHI_OK;
}

// The last host-path call's spans, from its events (recorded during the call,
// read only when asked).
void resolve_timing(mochi_ctx* c) {
  if (!c->timing_pending) return;
  c->timing_pending = false;
  hipEvent_t* e = c->evs[c->ev_done];
  (void)hipEventElapsedTime(&c->last_ms[0], e[0], e[1]);
  (void)hipEventElapsedTime(&c->last_ms[1], e[1], e[2]);
  (void)hipEventElapsedTime(&c->last_ms[2], e[2], e[3]);
  (void)hipEventElapsedTime(&c->last_total_ms, e[0], e[3]);
}

static_assert(mochi::kFoldLimbs == mochi::kL, "verify_layout sizes a slot of xbuf by kFoldLimbs");
// a's batch fields for N grants of C certificates and its scratch pointers from `base`; the scratch bytes
static size_t lay_out(mochi::LaunchArgs& a, const mochi_ctx* c, uint32_t N, uint32_t C, void* base) {
  a.n_grants = N;
  a.n_certs = C;
  a.n_keys = c->n_keys;
  a.n_slots = (uint32_t)mochi::slot_capacity(N, c->n_keys);
  return mochi::verify_layout(a, base);
}
// the scratch bytes of N grants of C certificates; 0: the batch is too large
static size_t verify_bytes(const mochi_ctx* c, uint32_t N, uint32_t C) {
  if (mochi::slot_capacity(N, c->n_keys) > 0xFFFFFFF0ull || (uint64_t)N + C > 0xFFFFFFF0ull) return 0;
  mochi::LaunchArgs a;
  return lay_out(a, c, N, C, nullptr);
}
// The one place that grows the verify scratch.
int ensure_scratch(mochi_ctx* c, uint32_t N, uint32_t C) {
  const size_t bytes = verify_bytes(c, N, C);
  return bytes ? c->scratch.ensure(bytes) : fail(MOCHI_EINVAL, "batch too large");
}

int run_device(mochi_ctx* c, const mochi_batch* b, const mochi_params* p, mochi_verdicts* o, hipStream_t st,
               const uint32_t* op_out_off, const uint32_t* grant_same, const uint8_t* msg_status) {
  const uint32_t N = b->n_grants, C = b->n_certs;
  int rc;
  if ((rc = ensure_scratch(c, N, C))) return rc;
  mochi::LaunchArgs a;
  memset(&a, 0, sizeof a);
  lay_out(a, c, N, C, c->scratch.p);
  a.blob = b->grant_bytes;
  a.grant_off = b->grant_off;
  a.grant_len = b->grant_len;
  a.sig = b->sig;
  a.signer = b->signer;
  a.grant_key = b->grant_key;
  a.cert_grant_off = b->cert_grant_off;
  a.cert_op_off = b->cert_op_off;
  a.op_key = b->op_key;
  a.op_flags = b->op_flags;
  a.expected_hash = b->expected_hash;
  a.cert_mg_off = b->cert_mg_off;
  a.mg_grant_off = b->mg_grant_off;
  a.op_object_ts = b->op_object_ts;
  a.op_key_off = b->op_key_off;
  a.op_key_len = b->op_key_len;
  a.quorum_mode = p->quorum_mode;
  const uint32_t R = p->replication_factor;
  a.majority = 2 * (R / 3) + 1;  // ClusterConfiguration.getServerMajority  ClusterConfiguration.java:264-267
  a.strict_gt = p->strict_gt ? 1 : 0;
  a.keys = c->d_keys;
  a.fold = c->d_fold;
  if (o->grant_ts) a.ts = o->grant_ts;
  if (o->grant_flags) a.flags = o->grant_flags;
  a.small_grants = c->small_grants;
  a.grant_same = grant_same;
  a.grant_valid_bits = o->grant_valid_bits;
  a.cert_accept_bits = o->cert_accept_bits;
  a.cert_reason = o->cert_reason;
  a.cert_fail_op = o->cert_fail_op;
  a.op_decision = o->op_decision;
  a.op_g0 = o->op_g0;
  a.op_ts = o->op_ts;
  a.op_out_off = op_out_off;
  a.msg_status = msg_status;
  a.aux = prep_serial() ? nullptr : c->aux;  // MOCHI_PREP_SERIAL=1: prep on the launch stream (A/B)
  a.ev_fork = c->ev_fork;
  a.ev_join = c->ev_join;
  if (c->profiling) {
    std::vector<hipEvent_t> evs(2 * mochi::kProfStages, nullptr);
    for (auto& e : evs) HIP_TRY(hipEventCreate(&e));
    c->prof_sets.push_back(evs);
    a.prof_events = c->prof_sets.back().data();
  }
  HIP_TRY(scratch_acquire(c, st));
  HIP_TRY(mochi::launch_verify(a, st));
  HIP_TRY(scratch_release(c, st));
  return MOCHI_OK;
}

// ---- Write2ToServer wire path -------------------------------------------------
// Decode on the device (w2_decode.hip), then the ordinary verify path over the
// decoded batch, then the per-message status fix-up.  All pointers device.
// Decode, phase 1 (w2_decode.hip): validate + count + CSR scans for the M
// messages of `w`.  cnt: this batch's w2_count_layout bytes on the device;
// the totals (N, O, n_mgs) land in tot_host (pinned) once ev_tot completes.
int w2_count(mochi_ctx* c, const mochi_write2_batch* w, uint8_t* status, void* cnt, uint32_t* tot_host,
             hipEvent_t ev_tot, hipStream_t st, mochi::W2Args* a) {
  const uint32_t M = w->n_msgs;
  size_t scan_bytes = 0;  // a small batch needs none (and the size query is ~7 host API calls)
  if (!mochi::w2_small(M)) HIP_TRY(mochi::w2_scan_temp_bytes(M + 1, &scan_bytes));
  if (scan_bytes > c->w2_scan.cap) {
    HIP_TRY(hipStreamSynchronize(st));  // the scan scratch may be in use by an earlier chunk
    int rc = c->w2_scan.ensure(scan_bytes);
    if (rc) return rc;
  }
  memset(a, 0, sizeof *a);
  a->wire = w->wire;
  a->msg_off = w->msg_off;
  a->msg_len = w->msg_len;
  a->M = M;
  a->flags_off = w->op_flags_off;
  a->flags_in = w->op_flags;
  a->ots_in = w->op_object_ts;
  a->ids = c->ids.as<uint8_t>();
  a->id_off = c->id_off.as<uint32_t>();
  a->n_ids = c->n_ids;
  mochi::w2_count_layout(*a, cnt);
  a->status = status;
  a->scan_temp = c->w2_scan.p;
  a->scan_temp_bytes = c->w2_scan.cap;
  HIP_TRY(mochi::launch_w2_count(*a, st));
  // decoded grants, ops and MultiGrants: the packed scan's last element
  HIP_TRY(hipMemcpyAsync(tot_host, a->off4 + 4 * (size_t)M, 12, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipEventRecord(ev_tot, st));
  return MOCHI_OK;
}

// Decode, phase 2: emit the SoA batch (N grants, O ops, NM MultiGrants from
// phase 1), then the verify path and the per-message status fix-up.  Per-op
// outputs follow the caller's op_flags_off layout (`op_out_off`, device).
int w2_verify(mochi_ctx* c, const mochi_write2_batch* w, const mochi_params* p, mochi_verdicts* o,
              mochi::W2Args& a, uint32_t N, uint32_t O, uint32_t NM, const uint32_t* op_out_off, hipStream_t st,
              bool decode_only) {
  a.N = N;
  const size_t out_bytes = mochi::w2_emit_layout(a, O, NM, nullptr);
  const size_t ver_bytes = decode_only ? 0 : verify_bytes(c, N, a.M);  // 0 too where ensure_scratch refuses the batch
  // a buffer that must be reallocated: first let the stream drain (an earlier chunk's kernels may still use it)
  if (out_bytes > c->w2_out.cap || ver_bytes > c->scratch.cap) HIP_TRY(hipStreamSynchronize(st));
  int rc;
  if ((rc = c->w2_out.ensure(out_bytes)) || (!decode_only && (rc = ensure_scratch(c, N, a.M)))) return rc;
  mochi::w2_emit_layout(a, O, NM, c->w2_out.p);
  HIP_TRY(mochi::launch_w2_emit(a, st));
  if (decode_only) return MOCHI_OK;
  mochi_batch db;
  memset(&db, 0, sizeof db);
  db.n_grants = N;
  db.n_certs = a.M;
  db.n_ops = O;
  db.n_mgs = NM;
  db.grant_bytes_len = w->wire_len;
  db.grant_bytes = w->wire;
  db.grant_off = a.grant_off;
  db.grant_len = a.grant_len;
  db.sig = a.sig;
  db.signer = a.signer;
  db.grant_key = a.grant_key;
  db.cert_grant_off = a.cert_grant_off;
  db.cert_op_off = a.cert_op_off;
  db.op_key = a.op_key;
  db.op_flags = a.op_flags;
  db.expected_hash = w->expected_hash;
  db.cert_mg_off = a.cert_mg_off;
  db.mg_grant_off = a.mg_grant_off;
  db.op_object_ts = a.op_object_ts;
  db.op_key_off = a.op_key_off;
  db.op_key_len = a.op_key_len;
  mochi_verdicts dv;
  memset(&dv, 0, sizeof dv);
  dv.cert_accept_bits = o->cert_accept_bits;
  dv.cert_reason = o->cert_reason;
  dv.cert_fail_op = o->cert_fail_op;
  dv.op_decision = o->op_decision;
  dv.op_g0 = o->op_g0;
  dv.op_ts = o->op_ts;
  // the status fix-up of undecoded messages runs inside k_tally (one launch
  // fewer at the end of the call); MOCHI_W2_FIXUP_KERNEL=1 (A/B): as its own kernel
  const bool fused = !fixup_kernel();
  if ((rc = run_device(c, &db, p, &dv, st, op_out_off, a.grant_same, fused ? a.status : nullptr))) return rc;
  if (!fused)
    HIP_TRY(mochi::launch_w2_fixup(a, o->cert_accept_bits, o->cert_reason, o->cert_fail_op, o->op_decision, o->op_g0,
                                   o->op_ts, st));
  return MOCHI_OK;
}

// Device-resident wire batch, one shot (mochi_verify_write2_device).
static int run_write2_device(mochi_ctx* c, const mochi_write2_batch* w, const mochi_params* p, mochi_verdicts* o,
                             uint8_t* status, hipStream_t st) {
  const uint32_t M = w->n_msgs;
  if (c->n_ids != c->n_keys) return fail(MOCHI_EINVAL, "server ids not set (mochi_ctx_set_server_ids)");
  int rc;
  mochi::W2Args a;
  a.M = M;
  if ((rc = c->w2_cnt.ensure(mochi::w2_count_layout(a, nullptr))) || (rc = c->w2_tot.ensure(16)) ||
      (!status && (rc = c->w2_status.ensure(M ? M : 1))))
    return rc;
  HIP_TRY(scratch_acquire(c, st));
  uint32_t* tot = (uint32_t*)c->w2_tot.p;
  if ((rc = w2_count(c, w, status ? status : c->w2_status.as<uint8_t>(), c->w2_cnt.p, tot, c->ev_tot, st, &a)))
    return rc;
  HIP_TRY(hipEventSynchronize(c->ev_tot));
  if ((rc = w2_verify(c, w, p, o, a, tot[0], tot[1], tot[2], w->op_flags_off, st, false))) return rc;
  HIP_TRY(scratch_release(c, st));
  return MOCHI_OK;
}

int check_write2_header(const mochi_ctx* c, const mochi_write2_batch* w, const mochi_params* p,
                        const mochi_verdicts* o) {
  if (!c || !w || !p || !o) return fail(MOCHI_EINVAL, "null argument");
  if (o->grant_valid_bits || o->grant_flags || o->grant_ts)
    return fail(MOCHI_EINVAL, "grant-level outputs are not produced on the Write2 wire path");
  if (w->n_msgs && (!o->cert_accept_bits || !w->wire || !w->msg_off || !w->msg_len || !w->expected_hash))
    return fail(MOCHI_EINVAL, "wire / msg_off / msg_len / expected_hash / cert_accept_bits required");
  if (w->op_flags_off && !w->op_flags) return fail(MOCHI_EINVAL, "op_flags required with op_flags_off");
  if ((o->op_decision || o->op_g0 || o->op_ts) && !w->op_flags_off)
    return fail(MOCHI_EINVAL, "per-op outputs on the wire path need op_flags_off (their layout)");
  if (w->op_object_ts && !w->op_flags_off) return fail(MOCHI_EINVAL, "op_object_ts needs op_flags_off");
  if ((p->quorum_mode & ~(uint32_t)(MOCHI_Q_DISTINCT_SIGNERS | MOCHI_Q_BIND)) != 0)
    return fail(MOCHI_EINVAL, "unknown quorum_mode bits 0x%x", p->quorum_mode);
  if (p->replication_factor == 0) return fail(MOCHI_EINVAL, "replication_factor must be > 0");
  return MOCHI_OK;
}

}  // namespace mochi

extern "C" {

int mochi_verify_batch_device(mochi_ctx* c, const mochi_batch* b, const mochi_params* p, mochi_verdicts* o,
                              void* stream) {
  int rc = check_batch_header(c, b, p, o);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard dev(c->device);
  if (!dev.ok) return fail(MOCHI_EHIP, "hipSetDevice(%d)", c->device);
  new_call(c);
  return run_device(c, b, p, o, (hipStream_t)stream);  // NULL = the null stream, as in HIP
}

void* mochi_host_alloc(uint64_t bytes) {
  void* ptr = nullptr;
  if (hipHostMalloc(&ptr, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
    fail(MOCHI_ENOMEM, "hipHostMalloc(%llu) failed", (unsigned long long)bytes);
    return nullptr;
  }
  return ptr;
}

void mochi_host_free(void* ptr) {
  if (ptr) (void)hipHostFree(ptr);
}

int mochi_ctx_set_small_batch(mochi_ctx* c, uint32_t grants) {
  if (!c) return fail(MOCHI_EINVAL, "null context");
  std::lock_guard<std::mutex> lk(c->mu);
  c->small_grants = grants;
  return MOCHI_OK;
}

int mochi_ctx_set_chunk_grants(mochi_ctx* c, uint32_t grants) {
  if (!c) return fail(MOCHI_EINVAL, "null context");
  std::lock_guard<std::mutex> lk(c->mu);
  c->chunk_grants = grants ? grants : default_chunk_grants();
  return MOCHI_OK;
}

int mochi_ctx_last_total_ms(mochi_ctx* c, float* total_ms) {
  if (!c || !total_ms) return fail(MOCHI_EINVAL, "null argument");
  resolve_timing(c);
  *total_ms = c->last_total_ms;
  return MOCHI_OK;
}

int mochi_ctx_set_server_ids(mochi_ctx* c, const uint8_t* ids, const uint32_t* id_off, uint32_t n_ids) {
  if (!c || !ids || !id_off) return fail(MOCHI_EINVAL, "null argument");
  if (n_ids != c->n_keys) return fail(MOCHI_EINVAL, "n_ids (%u) must equal the key count (%u)", n_ids, c->n_keys);
  if (id_off[0] != 0) return fail(MOCHI_EINVAL, "id_off[0] must be 0");
  for (uint32_t i = 0; i < n_ids; i++)
    if (id_off[i + 1] < id_off[i] || id_off[i + 1] - id_off[i] > 256)
      return fail(MOCHI_EINVAL, "server id %u: bad length", i);
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard dev(c->device);
  if (!dev.ok) return fail(MOCHI_EHIP, "hipSetDevice(%d)", c->device);
  const size_t nb = id_off[n_ids];
  int rc = c->ids.ensure(nb ? nb : 1);
  if (!rc) rc = c->id_off.ensure(4 * ((size_t)n_ids + 1));
  if (!rc && nb && hipMemcpy(c->ids.p, ids, nb, hipMemcpyHostToDevice) != hipSuccess) rc = fail(MOCHI_EHIP, "copy ids");
  if (!rc && hipMemcpy(c->id_off.p, id_off, 4 * ((size_t)n_ids + 1), hipMemcpyHostToDevice) != hipSuccess)
    rc = fail(MOCHI_EHIP, "copy id_off");
  if (!rc) {
    c->n_ids = n_ids;
    c->server_ids.clear();
    for (uint32_t i = 0; i < n_ids; i++) c->server_ids.emplace_back((const char*)ids + id_off[i], id_off[i + 1] - id_off[i]);
  }
  return rc;
}

int mochi_verify_write2_device(mochi_ctx* c, const mochi_write2_batch* w, const mochi_params* p, mochi_verdicts* o,
                               uint8_t* msg_status, void* stream) {
  int rc = check_write2_header(c, w, p, o);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard dev(c->device);
  if (!dev.ok) return fail(MOCHI_EHIP, "hipSetDevice(%d)", c->device);
  new_call(c);
  return run_write2_device(c, w, p, o, msg_status, (hipStream_t)stream);
}

// ---- Write2 encode (client certificate assembly) ----------------------------

namespace {

int check_write2_source(const mochi_write2_source* s, const uint64_t* msg_off, const uint32_t* msg_len,
                        const uint8_t* status, const uint64_t* wire_len) {
  if (!s || !wire_len) return fail(MOCHI_EINVAL, "null argument");
  if (s->n_msgs && (!msg_off || !msg_len || !status)) return fail(MOCHI_EINVAL, "msg_off / msg_len / status required");
  if (!s->cert_mg_off || !s->mg_grant_off || !s->cert_op_off)
    return fail(MOCHI_EINVAL, "cert_mg_off / mg_grant_off / cert_op_off required");
  if (s->n_mgs && !s->mg_signer) return fail(MOCHI_EINVAL, "mg_signer required");
  if (s->n_grants && (!s->grant_off || !s->grant_len || (!s->grant_bytes && s->grant_bytes_len)))
    return fail(MOCHI_EINVAL, "grant_bytes / grant_off / grant_len required");
  if (s->n_ops && (!s->op_action || !s->op1_off || !s->op1_len)) return fail(MOCHI_EINVAL, "op_action / op1_off / op1_len required");
  if (!s->op2_off != !s->op2_len) return fail(MOCHI_EINVAL, "op2_off and op2_len go together");
  if (!s->client_off != !s->client_len) return fail(MOCHI_EINVAL, "client_off and client_len go together");
  if (s->n_msgs == 0xFFFFFFFFu) return fail(MOCHI_EINVAL, "batch too large");
  return MOCHI_OK;
}

int run_write2_encode_device(mochi_ctx* c, const mochi_write2_source* s, uint8_t* wire, uint64_t wire_cap,
                             uint64_t* msg_off, uint32_t* msg_len, uint8_t* status, uint64_t* wire_len,
                             hipStream_t st) {
  if (c->n_ids != c->n_keys) return fail(MOCHI_EINVAL, "server ids not set (mochi_ctx_set_server_ids)");
  *wire_len = 0;
  const uint32_t M = s->n_msgs;
  if (M == 0) return MOCHI_OK;
  EncState& x = c->w2e;
  mochi::W2EncArgs a;
  memset(&a, 0, sizeof a);
  a.src = *s;
  a.ids = c->ids.as<uint8_t>();
  a.id_off = c->id_off.as<uint32_t>();
  a.n_ids = c->n_ids;
  a.wire = wire;
  a.msg_off = msg_off;
  a.msg_len = msg_len;
  a.status = status;
  int rc = x.begin(a, mochi::w2_enc_layout, mochi::w2_small(M) ? 0 : M + 1, 8, c->profiling, mochi::kW2EncEvents);
  if (rc) return rc;
  HIP_TRY(c->order.acquire(st));
  HIP_TRY(mochi::launch_w2_enc_size(a, st));
  if ((rc = x.fetch_totals(a.off64 + M, 8, c->ev_tot, st))) return rc;
  const uint64_t need = *wire_len = *(const uint64_t*)x.tot.p;
  const bool fits = need <= wire_cap;
  if (fits) HIP_TRY(mochi::launch_w2_enc_emit(a, st));
  x.ev_valid = a.ev && fits;
  HIP_TRY(c->order.release(st));
  return fits ? MOCHI_OK : capacity_error("wire_cap", wire_cap, "encoded size", need);
}

}  // namespace

uint64_t mochi_write2_encode_bound(const mochi_write2_source* s, uint32_t max_id_len) {
  if (!s) return 0;
  // every grant at grant_bytes_len (grants may share bytes) with its objectId
  // twice, every string at strings_len, five-byte length varints throughout
  const unsigned __int128 gb = s->grant_bytes_len, sb = s->strings_len;
  unsigned __int128 t = (unsigned __int128)s->n_grants * (3 * gb + MOCHI_RSA_BYTES + 40) +
                        (unsigned __int128)s->n_mgs * (2 * (unsigned __int128)max_id_len + sb + 32) +
                        (unsigned __int128)s->n_ops * (2 * sb + 24) + (unsigned __int128)s->n_msgs * 12;
  const unsigned __int128 cap = (unsigned __int128)s->n_msgs * mochi::kEncMaxMsg;  // longer messages are emitted empty
  if (t > cap) t = cap;
  return (uint64_t)t;
}

int mochi_write2_encode(const mochi_write2_source* s, const uint8_t* ids, const uint32_t* id_off, uint32_t n_ids,
                        uint8_t* wire, uint64_t wire_cap, uint64_t* msg_off, uint32_t* msg_len, uint8_t* status,
                        uint64_t* wire_len) {
  int rc = check_write2_source(s, msg_off, msg_len, status, wire_len);
  if (rc) return rc;
  if (n_ids && (!ids || !id_off)) return fail(MOCHI_EINVAL, "ids / id_off required");
  if (wire_cap && !wire) return fail(MOCHI_EINVAL, "wire required");
  if (s->n_grants && s->grant_bytes_len && !s->grant_bytes) return fail(MOCHI_EINVAL, "grant_bytes required");
  if (s->strings_len && !s->strings) return fail(MOCHI_EINVAL, "strings required");
  const char* err = "";
  rc = mochi_host::write2_encode(s, ids, id_off, n_ids, wire, wire_cap, msg_off, msg_len, status, wire_len, &err);
  return rc ? fail(rc, "mochi_write2_encode: %s", err) : MOCHI_OK;
}

int mochi_write2_encode_device(mochi_ctx* c, const mochi_write2_source* s, uint8_t* wire, uint64_t wire_cap,
                               uint64_t* msg_off, uint32_t* msg_len, uint8_t* status, uint64_t* wire_len,
                               void* stream) {
  if (!c) return fail(MOCHI_EINVAL, "null context");
  int rc = check_write2_source(s, msg_off, msg_len, status, wire_len);
  if (rc) return rc;
  if (wire_cap && !wire) return fail(MOCHI_EINVAL, "wire required");
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard dev(c->device);
  if (!dev.ok) return fail(MOCHI_EHIP, "hipSetDevice(%d)", c->device);
  new_call(c);
  return run_write2_encode_device(c, s, wire, wire_cap, msg_off, msg_len, status, wire_len, (hipStream_t)stream);
}

}  // extern "C"

// ---- Write1 reply decode (the client's round) --------------------------------

namespace {

int check_write1_replies(const mochi_write1_replies* r, const mochi_write1_decoded* o) {
  if (!r || !o) return fail(MOCHI_EINVAL, "null argument");
  if (!o->resp_grant_off || !o->resp_cert_off) return fail(MOCHI_EINVAL, "resp_grant_off / resp_cert_off required");
  if (r->n_resps && (!r->resp_off || !r->resp_len || !r->resp_kind || (!r->wire && r->wire_len)))
    return fail(MOCHI_EINVAL, "wire / resp_off / resp_len / resp_kind required");
  if (r->n_resps && (!o->resp_status || !o->resp_kind_out || !o->resp_server || !o->mg_signer || !o->resp_client_off ||
                     !o->resp_client_len))
    return fail(MOCHI_EINVAL, "the per-response outputs are required");
  if (r->n_resps && !r->n_reqs) return fail(MOCHI_EINVAL, "responses without a request");
  if (r->n_reqs && (!r->req_resp_off || !r->req_op_off)) return fail(MOCHI_EINVAL, "req_resp_off / req_op_off required");
  if (r->n_ops && (!r->op_key_off || !r->op_key_len || (!r->strings && r->strings_len)))
    return fail(MOCHI_EINVAL, "strings / op_key_off / op_key_len required");
  if (r->n_resps > mochi::wire::kMaxResps) return fail(MOCHI_EINVAL, "more than 2^24 responses");
  if (o->grant_cap && (!o->grant_off || !o->grant_len || !o->grant_key || !o->grant_ts || !o->grant_status ||
                       !o->grant_flags))
    return fail(MOCHI_EINVAL, "the per-grant outputs are required (grant_cap > 0)");
  if (o->cert_cap && (!o->cert_key_off || !o->cert_key_len || !o->cert_val_off || !o->cert_val_len))
    return fail(MOCHI_EINVAL, "the per-certificate outputs are required (cert_cap > 0)");
  return MOCHI_OK;
}

int w1d_capacity_error(const mochi_write1_decoded* o) {
  return fail(MOCHI_EINVAL, "grant_cap (%u) / cert_cap (%u) smaller than the decoded grants (%u) / certificates (%u)",
              o->grant_cap, o->cert_cap, o->n_grants, o->n_certs);
}

int run_write1_decode_device(mochi_ctx* c, const mochi_write1_replies* r, mochi_write1_decoded* o, hipStream_t st) {
  if (c->n_ids != c->n_keys) return fail(MOCHI_EINVAL, "server ids not set (mochi_ctx_set_server_ids)");
  o->n_grants = o->n_certs = 0;
  const uint32_t P = r->n_resps;
  EncState& x = c->w1d;
  if (P == 0) {  // both CSRs hold their one element
    x.ev_valid = false;
    HIP_TRY(hipMemsetAsync(o->resp_grant_off, 0, 4, st));
    HIP_TRY(hipMemsetAsync(o->resp_cert_off, 0, 4, st));
    return MOCHI_OK;
  }
  mochi::W1DecArgs a;
  memset(&a, 0, sizeof a);
  a.v.in = *r;
  a.v.ids = c->ids.as<uint8_t>();
  a.v.id_off = c->id_off.as<uint32_t>();
  a.v.n_ids = c->n_ids;
  a.v.out = *o;
  a.P = P;
  int rc = x.begin(a, mochi::w1d_layout, P + 1, 8, c->profiling, mochi::kW1DecEvents);
  if (rc) return rc;
  HIP_TRY(c->order.acquire(st));
  HIP_TRY(mochi::launch_w1d_count(a, st));
  if ((rc = x.fetch_totals(a.off64 + P, 8, c->ev_tot, st))) return rc;
  const uint64_t tot = *(const uint64_t*)x.tot.p;
  o->n_grants = (uint32_t)tot;
  o->n_certs = (uint32_t)(tot >> 32);
  const bool fits = o->n_grants <= o->grant_cap && o->n_certs <= o->cert_cap;
  if (fits) {
    if (o->sig && o->n_grants) {
      if ((rc = c->w1d_sig.ensure(8 * (size_t)o->n_grants))) return rc;
      a.v.sig_src = c->w1d_sig.as<uint64_t>();
    }
    HIP_TRY(mochi::launch_w1d_emit(a, o->n_grants, st));
  }
  x.ev_valid = a.ev && fits;
  HIP_TRY(c->order.release(st));
  return fits ? MOCHI_OK : w1d_capacity_error(o);
}

}  // namespace

extern "C" {

void mochi_write1_reply_decode_bound(uint64_t wire_len, uint32_t n_resps, uint64_t* grants, uint64_t* certs) {
  const uint64_t per = wire_len / 2 < mochi::w1d::kMaxEntries ? wire_len / 2 : mochi::w1d::kMaxEntries;
  if (grants) *grants = per * n_resps;
  if (certs) *certs = per * n_resps;
}

int mochi_write1_reply_decode(const mochi_write1_replies* r, const uint8_t* ids, const uint32_t* id_off, uint32_t n_ids,
                              mochi_write1_decoded* o) {
  int rc = check_write1_replies(r, o);
  if (rc) return rc;
  if (n_ids && (!ids || !id_off)) return fail(MOCHI_EINVAL, "ids / id_off required");
  const char* err = nullptr;
  rc = mochi_host::write1_reply_decode(r, ids, id_off, n_ids, o, &err);
  if (rc && err) return fail(rc, "mochi_write1_reply_decode: %s", err);
  return rc ? w1d_capacity_error(o) : MOCHI_OK;
}

int mochi_write1_reply_decode_device(mochi_ctx* c, const mochi_write1_replies* r, mochi_write1_decoded* o,
                                     void* stream) {
  if (!c) return fail(MOCHI_EINVAL, "null context");
  int rc = check_write1_replies(r, o);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard dev(c->device);
  if (!dev.ok) return fail(MOCHI_EHIP, "hipSetDevice(%d)", c->device);
  new_call(c);
  return run_write1_decode_device(c, r, o, (hipStream_t)stream);
}

int mochi_ctx_read_w1_decode_profile(mochi_ctx* c, float* kernel_ms, uint32_t n_kernels) {
  if (!c || !kernel_ms) return fail(MOCHI_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(c->mu);
  static const int kSpan[mochi::kW1DecStages][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {5, 6}, {6, 7}};
  return c->w1d.read_profile(kSpan, mochi::kW1DecStages, kernel_ms, n_kernels,
                             "no Write1 reply decode call was made while profiling was on");
}

int mochi_fold_matrix(const uint8_t* modulus_be, int8_t* img, uint32_t* cadd) {
  if (!modulus_be || !img || !cadd) return fail(MOCHI_EINVAL, "null argument");
  if (!(modulus_be[0] & 0x80) || !(modulus_be[255] & 1)) return fail(MOCHI_EINVAL, "modulus must be odd, 2048 bits");
  std::vector<mochi::FoldKey> f(1);
  int rc = make_fold_key(modulus_be, f.data());
  if (rc) return rc;
  memcpy(img, f[0].img, sizeof f[0].img);
  memcpy(cadd, f[0].cadd, sizeof f[0].cadd);
  return MOCHI_OK;
}

int mochi_rsa_public_op(mochi_ctx* c, uint32_t n, const uint8_t* sig_be, const uint16_t* signer, uint8_t* out_be,
                        uint32_t* out_z) {
  if (!c || (n && (!sig_be || !signer || !out_be))) return fail(MOCHI_EINVAL, "null argument");
  for (uint32_t i = 0; i < n; i++)
    if (signer[i] >= c->n_keys) return fail(MOCHI_EINVAL, "signer[%u] out of range", i);
  if (n == 0) return MOCHI_OK;
  std::lock_guard<std::mutex> lk(c->mu);
  new_call(c);
  DeviceGuard dev(c->device);
  if (!dev.ok) return fail(MOCHI_EHIP, "hipSetDevice(%d)", c->device);
  const size_t sig_bytes = (size_t)MOCHI_RSA_BYTES * n, y_bytes = sizeof(uint32_t) * 64 * (size_t)n;
  int rc;
  if ((rc = c->dev_in.ensure(align_up(sig_bytes, 256) + sizeof(uint16_t) * n)) || (rc = c->dev_out.ensure(y_bytes)) ||
      (rc = ensure_scratch(c, n, 0)))
    return rc;
  hipStream_t st = c->stream;
  uint8_t* din = c->dev_in.as<uint8_t>();
  uint16_t* dsigner = (uint16_t*)(din + align_up(sig_bytes, 256));
  mochi::LaunchArgs a;
  memset(&a, 0, sizeof a);
  lay_out(a, c, n, 0, c->scratch.p);
  const uint64_t slots = a.n_slots;
  a.sig = din;
  a.signer = dsigner;
  a.keys = c->d_keys;
  a.fold = c->d_fold;
  a.dbg_y = c->dev_out.as<uint32_t>();
  a.skip_prep_tally = true;
  // the context's small-batch setting picks the launch sequence as in the verify
  // calls (k_bucket_small + k_rsa_pow_lat); prep stays off, so k_bucket_small
  // never reads the zeroed PrepArgs, and dbg_y keeps the final on k_rsa_raw
  a.small_grants = c->small_grants;
  std::vector<uint32_t> y(64 * (size_t)n), perm, z;
  bool ok = hipMemcpyAsync(din, sig_be, sig_bytes, hipMemcpyHostToDevice, st) == hipSuccess &&
            hipMemcpyAsync(dsigner, signer, sizeof(uint16_t) * n, hipMemcpyHostToDevice, st) == hipSuccess &&
            hipMemsetAsync(a.digest, 0, sizeof(uint32_t) * 8 * (size_t)n, st) == hipSuccess &&
            hipMemsetAsync(a.flags, 0, n, st) == hipSuccess && mochi::launch_verify(a, st) == hipSuccess &&
            hipMemcpyAsync(y.data(), a.dbg_y, y_bytes, hipMemcpyDeviceToHost, st) == hipSuccess;
  if (ok && out_z) {
    perm.resize(slots);
    z.resize((size_t)mochi::kL * slots);
    ok = hipMemcpyAsync(perm.data(), a.perm, sizeof(uint32_t) * slots, hipMemcpyDeviceToHost, st) == hipSuccess &&
         hipMemcpyAsync(z.data(), a.xbuf, sizeof(uint32_t) * z.size(), hipMemcpyDeviceToHost, st) == hipSuccess;
  }
  ok = ok && hipStreamSynchronize(st) == hipSuccess;
  if (!ok) return fail(MOCHI_EHIP, "rsa_public_op failed: %s", hipGetErrorString(hipGetLastError()));
  for (uint32_t g = 0; g < n; g++)
    for (int i = 0; i < 64; i++) {
      const uint32_t w = y[(size_t)g * 64 + i];
      uint8_t* o = out_be + (size_t)g * 256 + 256 - 4 * (i + 1);
      o[0] = (uint8_t)(w >> 24);
      o[1] = (uint8_t)(w >> 16);
      o[2] = (uint8_t)(w >> 8);
      o[3] = (uint8_t)w;
    }
  if (out_z)
    for (uint64_t sl = 0; sl < slots; sl++) {
      const uint32_t g = perm[sl];
      if (g == 0xFFFFFFFFu) continue;
      for (int j = 0; j < mochi::kL; j++) out_z[(size_t)g * mochi::kL + j] = z[(size_t)j * slots + sl];
    }
  return MOCHI_OK;
}

int mochi_ctx_set_profiling(mochi_ctx* c, int on) {
  if (!c) return fail(MOCHI_EINVAL, "null ctx");
  std::lock_guard<std::mutex> lk(c->mu);
  c->profiling = on != 0;
  return MOCHI_OK;
}

int mochi_ctx_read_profile(mochi_ctx* c, float* stage_ms, uint32_t n_stages, uint32_t* n_calls) {
  if (!c || !stage_ms) return fail(MOCHI_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(c->mu);
  for (uint32_t i = 0; i < n_stages; i++) stage_ms[i] = 0.f;
  uint32_t calls = 0;
  for (auto& evs : c->prof_sets) {
    for (auto e : evs)
      if (hipEventSynchronize(e) != hipSuccess) return fail(MOCHI_EHIP, "hipEventSynchronize failed");
    for (uint32_t i = 0; i < n_stages && i < (uint32_t)mochi::kProfStages; i++) {
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, evs[2 * i], evs[2 * i + 1]);  // (start, end) of stage i
      stage_ms[i] += ms;
    }
    for (auto e : evs) (void)hipEventDestroy(e);
    calls++;
  }
  c->prof_sets.clear();
  if (n_calls) *n_calls = calls;
  return MOCHI_OK;
}

int mochi_ctx_read_encode_profile(mochi_ctx* c, float* kernel_ms, uint32_t n_kernels) {
  if (!c || !kernel_ms) return fail(MOCHI_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(c->mu);
  static const int kSpan[mochi::kW2EncStages][2] = {{0, 1}, {1, 2}, {2, 3}, {4, 5}, {5, 6}, {6, 7}};
  return c->w2e.read_profile(kSpan, mochi::kW2EncStages, kernel_ms, n_kernels,
                             "no encode call was made while profiling was on");
}

int mochi_ctx_last_timing(mochi_ctx* c, float* h2d_ms, float* kernels_ms, float* d2h_ms) {
  if (!c) return fail(MOCHI_EINVAL, "null ctx");
  resolve_timing(c);
  if (h2d_ms) *h2d_ms = c->last_ms[0];
  if (kernels_ms) *kernels_ms = c->last_ms[1];
  if (d2h_ms) *d2h_ms = c->last_ms[2];
  return MOCHI_OK;
}

// Client-side aggregation: MochiDBClient.java:148-175 (reads) / 355-382 (Write2).
int mochi_tally_responses(uint32_t n_requests, const uint32_t* resp_off, const uint32_t* n_ops,
                          const uint32_t* resp_n_ops, const uint64_t* status_off, const uint8_t* status,
                          const uint64_t* chosen_off, uint32_t replication_factor, int32_t* chosen, uint8_t* reason,
                          uint32_t* accept_bits) {
  // the device form's rule: an argument nobody reads is not required
  if (!n_requests) return MOCHI_OK;
  if (!resp_off || !n_ops || !resp_n_ops || !status_off || !status || !accept_bits || (chosen && !chosen_off))
    return fail(MOCHI_EINVAL, "null argument");
  const uint32_t M = 2 * (replication_factor / 3) + 1;  // getServerMajority
  memset(accept_bits, 0, ((size_t)n_requests + 31) / 32 * 4);
  std::vector<uint32_t> cnt;
  for (uint32_t r = 0; r < n_requests; r++) {
    const uint32_t k = n_ops[r];
    cnt.assign(k, 0);
    int32_t* ch = chosen ? chosen + chosen_off[r] : nullptr;
    if (ch)
      for (uint32_t j = 0; j < k; j++) ch[j] = -1;
    uint8_t why = 0;
    for (uint32_t q = resp_off[r]; q < resp_off[r + 1]; q++) {
      if (resp_n_ops[q] != k) {  // operations.size() != transactionOps.size()
        why = 1;
        break;
      }
      const uint8_t* st = status + status_off[q];
      for (uint32_t j = 0; j < k; j++)
        if (st[j] != 1) {  // != WRONG_SHARD
          cnt[j]++;
          if (ch) ch[j] = (int32_t)(q - resp_off[r]);
        }
    }
    for (uint32_t j = 0; j < k && !why; j++)
      if (cnt[j] < M) why = 2;  // consistentTRCount[index] < getServerMajority()
    if (reason) reason[r] = why;
    if (!why) accept_bits[r >> 5] |= 1u << (r & 31);
  }
  return MOCHI_OK;
}

int mochi_write1_classify(uint32_t n_requests, const uint32_t* resp_off, const uint8_t* resp_kind,
                          const uint32_t* resp_server, const uint32_t* resp_grant_off, const uint8_t* grant_key,
                          const int64_t* grant_ts, const uint8_t* grant_status, uint8_t* decision) {
  if (!n_requests) return MOCHI_OK;
  if (!resp_off || !resp_kind || !resp_server || !resp_grant_off || !decision)
    return fail(MOCHI_EINVAL, "null argument");
  if (resp_grant_off[resp_off[n_requests]] > resp_grant_off[0] && (!grant_key || !grant_ts || !grant_status))
    return fail(MOCHI_EINVAL, "null grant arrays");
  std::vector<uint32_t> ok_servers;
  for (uint32_t r = 0; r < n_requests; r++) {
    const uint32_t q0 = resp_off[r], q1 = resp_off[r + 1];
    if (q1 < q0) return fail(MOCHI_EINVAL, "resp_off not monotone at request %u", r);
    // one pass: REQUESTFAILED dominates, then any WRONG_SHARD grant in an OK/REFUSED multigrant
    bool failed = false, wrong_shard = false, all_ok = true;
    for (uint32_t q = q0; q < q1; q++) {
      const uint8_t kind = resp_kind[q];
      all_ok &= kind == MOCHI_W1_OK;
      failed |= kind == MOCHI_W1_REQUEST_FAILED;
      if (kind == MOCHI_W1_OK || kind == MOCHI_W1_REFUSED)
        for (uint32_t g = resp_grant_off[q]; g < resp_grant_off[q + 1]; g++) wrong_shard |= grant_status[g] == 1;
    }
    uint8_t d;
    if (failed) d = MOCHI_W1_THROW_FAILED;
    else if (wrong_shard) d = MOCHI_W1_THROW_UNSUPPORTED;
    else {
      // uniformity over the surviving OK multigrant of every serverId (the
      // last one, HashMap.put): walk backwards, skip ids already taken
      int64_t ts0[256];
      uint8_t seen[256];
      memset(seen, 0, sizeof seen);
      ok_servers.clear();
      bool uniform = true;
      for (uint32_t q = q1; q-- > q0 && uniform;) {
        if (resp_kind[q] != MOCHI_W1_OK) continue;
        bool dup = false;
        for (uint32_t sid : ok_servers) dup |= sid == resp_server[q];
        if (dup) continue;
        ok_servers.push_back(resp_server[q]);
        for (uint32_t g = resp_grant_off[q]; g < resp_grant_off[q + 1]; g++) {
          const uint8_t k = grant_key[g];
          if (k == 0xFF) continue;
          if (!seen[k]) {
            seen[k] = 1;
            ts0[k] = grant_ts[g];
          } else if (ts0[k] != grant_ts[g]) {
            uniform = false;
            break;
          }
        }
      }
      d = !uniform ? MOCHI_W1_RETRY : all_ok ? MOCHI_W1_PROCEED : MOCHI_W1_THROW_REFUSED;
    }
    decision[r] = d;
  }
  return MOCHI_OK;
}

}  // extern "C"

// ---- device signer (rsa_sign.hip) --------------------------------------------
struct mochi_signer {
  int device = 0;
  hipStream_t stream = nullptr;
  void* d_key = nullptr;
  std::mutex mu;
  DevBuf dev_in, dev_sig;
  PinnedBuf pin_in, pin_out;
  // fault check: the verify path under the signer's own public key
  mochi_ctx* check = nullptr;
  DevBuf zeros, flags, misc;  // signer index / key slot zeros, SIG_OK flags, [0] rejected [1..] CSR zeros
  uint32_t fault_idx = 0xFFFFFFFFu;
  EncState w1;  // Write1 issuance (w1_issue.hip); its totals are n_new and the grant bytes
  // Write1 reply encoder (w1_reply.hip): scratch of its own, so that it can run behind an
  // issue call whose kernels are still using w1.scratch
  EncState w1r;
  // Write1 request decoder (w1_request.hip): the per-request scratch, its total is n_ops;
  // the per-op scratch (claim table, key numbering) is sized once n_ops is known
  EncState w1q;
  DevBuf w1q_tab;
  hipEvent_t ev_tot = nullptr;  // totals landed
  ScratchOrder order;           // one for the encoders and the request decoder
  bool profiling = false;
};

namespace {

int bn_limbs(const BIGNUM* v, uint32_t* x, int n_limbs) {
  std::vector<uint8_t> le((size_t)n_limbs * 28 / 8 + 8, 0);
  if (BN_num_bytes(v) > (int)le.size() - 8 || BN_bn2lebinpad(v, le.data(), (int)le.size()) < 0) return 0;
  for (int j = 0; j < n_limbs; j++) {
    const int bit = j * 28, by = bit >> 3, sh = bit & 7;
    uint64_t w = 0;
    for (int b = 0; b < 5; b++) w |= (uint64_t)le[by + b] << (8 * b);
    x[j] = (uint32_t)(w >> sh) & 0x0FFFFFFFu;
  }
  return 1;
}

// -m^{-1} mod 2^28 from m's lowest 28-bit limb (odd): Newton on 32 bits
uint32_t neg_inv28(uint32_t lo) {
  uint32_t inv = 1;
  for (int i = 0; i < 6; i++) inv *= 2u - lo * inv;
  return (0u - inv) & 0x0FFFFFFFu;
}

}  // namespace

extern "C" {

mochi_signer* mochi_signer_create(int device, const char* pem) {
  if (!pem) {
    fail(MOCHI_EINVAL, "null key");
    return nullptr;
  }
  BIO* bio = BIO_new_mem_buf(pem, -1);
  EVP_PKEY* pk = bio ? PEM_read_bio_PrivateKey(bio, nullptr, nullptr, nullptr) : nullptr;
  if (bio) BIO_free(bio);
  BIGNUM *p = nullptr, *q = nullptr, *dp = nullptr, *dq = nullptr, *qi = nullptr;
  bool ok = pk && EVP_PKEY_get_bits(pk) == 2048 && EVP_PKEY_get_bn_param(pk, OSSL_PKEY_PARAM_RSA_FACTOR1, &p) &&
            EVP_PKEY_get_bn_param(pk, OSSL_PKEY_PARAM_RSA_FACTOR2, &q) &&
            EVP_PKEY_get_bn_param(pk, OSSL_PKEY_PARAM_RSA_EXPONENT1, &dp) &&
            EVP_PKEY_get_bn_param(pk, OSSL_PKEY_PARAM_RSA_EXPONENT2, &dq) &&
            EVP_PKEY_get_bn_param(pk, OSSL_PKEY_PARAM_RSA_COEFFICIENT1, &qi);
  if (pk) EVP_PKEY_free(pk);
  ok = ok && BN_num_bits(p) <= 1024 && BN_num_bits(q) <= 1024 && BN_num_bits(dp) <= 1024 && BN_num_bits(dq) <= 1024 &&
       BN_num_bits(dp) >= 2 && BN_num_bits(dq) >= 2;
  constexpr int kLh = 37;
  uint32_t lp[kLh], lq[kLh], r3p[kLh], r3q[kLh], qir[kLh], wdp[32], wdq[32], cpad[74];
  BN_CTX* bc = BN_CTX_new();
  BIGNUM *R = BN_new(), *t = BN_new(), *three = BN_new(), *cp = nullptr;
  uint8_t cb[256];
  memset(cb, 0xFF, sizeof cb);
  static const uint8_t kDigestInfo[19] = {0x30, 0x31, 0x30, 0x0d, 0x06, 0x09, 0x60, 0x86, 0x48, 0x01,
                                          0x65, 0x03, 0x04, 0x02, 0x01, 0x05, 0x00, 0x04, 0x20};
  cb[0] = 0x00;
  cb[1] = 0x01;
  cb[256 - 32 - 19 - 1] = 0x00;
  memcpy(cb + 256 - 32 - 19, kDigestInfo, 19);
  memset(cb + 256 - 32, 0, 32);
  cp = BN_bin2bn(cb, 256, nullptr);
  ok = ok && bc && R && t && three && cp && BN_set_bit(R, 28 * kLh) && BN_set_word(three, 3);
  ok = ok && bn_limbs(p, lp, kLh) && bn_limbs(q, lq, kLh);
  ok = ok && BN_mod_exp(t, R, three, p, bc) && bn_limbs(t, r3p, kLh);
  ok = ok && BN_mod_exp(t, R, three, q, bc) && bn_limbs(t, r3q, kLh);
  ok = ok && BN_mod_mul(t, qi, R, p, bc) && bn_limbs(t, qir, kLh);
  ok = ok && bn_limbs(cp, cpad, 74);
  uint8_t le[128];
  ok = ok && BN_bn2lebinpad(dp, le, 128) == 128;
  if (ok)
    for (int i = 0; i < 32; i++) wdp[i] = (uint32_t)le[4 * i] | (uint32_t)le[4 * i + 1] << 8 | (uint32_t)le[4 * i + 2] << 16 | (uint32_t)le[4 * i + 3] << 24;
  ok = ok && BN_bn2lebinpad(dq, le, 128) == 128;
  if (ok)
    for (int i = 0; i < 32; i++) wdq[i] = (uint32_t)le[4 * i] | (uint32_t)le[4 * i + 1] << 8 | (uint32_t)le[4 * i + 2] << 16 | (uint32_t)le[4 * i + 3] << 24;
  std::vector<uint8_t> host(mochi::sign_key_bytes());
  if (ok)
    mochi::sign_key_set(host.data(), lp, lq, r3p, r3q, qir, wdp, wdq, cpad, neg_inv28(lp[0]), neg_inv28(lq[0]),
                        (uint32_t)BN_num_bits(dp), (uint32_t)BN_num_bits(dq));
  for (BIGNUM* b : {p, q, dp, dq, qi, R, t, three, cp}) BN_clear_free(b);
  BN_CTX_free(bc);
  if (!ok) {
    fail(MOCHI_EINVAL, "not an RSA-2048 private key with CRT parameters");
    return nullptr;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
    fail(MOCHI_ENODEV, "device %d not available", device);
    return nullptr;
  }
  mochi_signer* s = new mochi_signer;
  s->device = device;
  {
    DeviceGuard dev(device);
    ok = dev.ok && hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) == hipSuccess &&
         hipEventCreateWithFlags(&s->ev_tot, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&s->order.ev, hipEventDisableTiming) == hipSuccess &&
         hipMalloc(&s->d_key, host.size()) == hipSuccess &&
         hipMemcpy(s->d_key, host.data(), host.size(), hipMemcpyHostToDevice) == hipSuccess;
  }
  memset(host.data(), 0, host.size());
  if (!ok) {
    fail(MOCHI_EHIP, "signer setup failed");
    mochi_signer_destroy(s);
    return nullptr;
  }
  uint8_t n_be[MOCHI_RSA_BYTES];
  if (mochi_pem_modulus(pem, n_be) != MOCHI_OK ||
      !(s->check = mochi_ctx_create(device, n_be, 1, MOCHI_RSA_BYTES, MOCHI_RSA_E))) {
    fail(MOCHI_EINVAL, "signer: public-key check context failed");
    mochi_signer_destroy(s);
    return nullptr;
  }
  if (s->misc.ensure(256) || hipMemset(s->misc.p, 0, 256) != hipSuccess) {
    fail(MOCHI_EHIP, "signer scratch");
    mochi_signer_destroy(s);
    return nullptr;
  }
  return s;
}

void mochi_signer_destroy(mochi_signer* s) {
  if (!s) return;
  DeviceGuard dev(s->device);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  if (s->d_key) {
    (void)hipMemset(s->d_key, 0, mochi::sign_key_bytes());  // private key material
    (void)hipFree(s->d_key);
  }
  if (s->stream) (void)hipStreamDestroy(s->stream);
  if (s->ev_tot) (void)hipEventDestroy(s->ev_tot);
  if (s->order.ev) (void)hipEventDestroy(s->order.ev);
  if (s->check) mochi_ctx_destroy(s->check);
  delete s;
}

}  // extern "C"

namespace {
// Verify n freshly made signatures with the signer's public key on the same
// stream (k_grant_prep + k_rsa_pow + k_rsa_final, ~1/50 of the signing work)
// and withhold every one that fails (RSA-CRT fault attack, Boneh-DeMillo-Lipton).
int signer_check(mochi_signer* s, const uint8_t* grant_bytes, const uint64_t* grant_off, const uint32_t* grant_len,
                 uint32_t n, uint8_t* sig, hipStream_t st) {
  if (!n) return MOCHI_OK;
  int rc;
  if ((rc = s->zeros.ensure(2 * (size_t)n)) || (rc = s->flags.ensure(n))) return rc;
  HIP_TRY(hipMemsetAsync(s->zeros.p, 0, 2 * (size_t)n, st));
  mochi_batch db;
  memset(&db, 0, sizeof db);
  db.n_grants = n;
  db.grant_bytes = grant_bytes;
  db.grant_off = grant_off;
  db.grant_len = grant_len;
  db.sig = sig;
  db.signer = s->zeros.as<uint16_t>();
  db.grant_key = s->zeros.as<uint8_t>();
  uint32_t* misc = s->misc.as<uint32_t>();
  db.cert_grant_off = misc + 1;  // one zero: no certificates
  db.cert_op_off = misc + 1;
  mochi_params p = {1, 1, 0, 0};
  mochi_verdicts dv;
  memset(&dv, 0, sizeof dv);
  dv.grant_flags = s->flags.as<uint8_t>();
  dv.cert_accept_bits = misc + 2;
  if ((rc = run_device(s->check, &db, &p, &dv, st))) return rc;
  HIP_TRY(mochi::launch_withhold(s->flags.as<uint8_t>(), n, sig, misc, st));
  return MOCHI_OK;
}
}  // namespace

extern "C" {

int mochi_signer_set_fault(mochi_signer* s, uint32_t grant_index) {
  if (!s) return fail(MOCHI_EINVAL, "null signer");
  std::lock_guard<std::mutex> lk(s->mu);
  s->fault_idx = grant_index;
  return MOCHI_OK;
}

int mochi_signer_rejected(mochi_signer* s, uint64_t* rejected) {
  if (!s || !rejected) return fail(MOCHI_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard dev(s->device);
  uint32_t v = 0;
  const bool ok = dev.ok && hipDeviceSynchronize() == hipSuccess &&
                  hipMemcpy(&v, s->misc.p, 4, hipMemcpyDeviceToHost) == hipSuccess &&
                  hipMemset(s->misc.p, 0, 4) == hipSuccess;
  if (!ok) return fail(MOCHI_EHIP, "signer counter read failed");
  *rejected = v;
  return MOCHI_OK;
}

int mochi_sign_batch_device(mochi_signer* s, const uint8_t* grant_bytes, const uint64_t* grant_off,
                            const uint32_t* grant_len, uint32_t n, uint8_t* sig_out, void* stream) {
  if (!s || (n && (!grant_bytes || !grant_off || !grant_len || !sig_out))) return fail(MOCHI_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard dev(s->device);
  if (!dev.ok) return fail(MOCHI_EHIP, "hipSetDevice");
  const hipError_t e = mochi::launch_rsa_sign(grant_bytes, grant_off, grant_len, n, s->d_key, sig_out, s->fault_idx,
                                              (hipStream_t)stream);
  int rc = e == hipSuccess ? MOCHI_OK : fail(MOCHI_EHIP, "k_rsa_sign: %s", hipGetErrorString(e));
  if (!rc) {
    std::lock_guard<std::mutex> ck(s->check->mu);
    rc = signer_check(s, grant_bytes, grant_off, grant_len, n, sig_out, (hipStream_t)stream);
  }
  return rc;
}

int mochi_sign_batch(mochi_signer* s, const uint8_t* grant_bytes, uint64_t grant_bytes_len, const uint64_t* grant_off,
                     const uint32_t* grant_len, uint32_t n, uint8_t* sig_out) {
  if (!s || (n && (!grant_bytes || !grant_off || !grant_len || !sig_out))) return fail(MOCHI_EINVAL, "null argument");
  for (uint32_t i = 0; i < n; i++)
    if (grant_off[i] > grant_bytes_len || grant_len[i] > grant_bytes_len - grant_off[i])
      return fail(MOCHI_EINVAL, "grant %u lies outside grant_bytes", i);
  if (n == 0) return MOCHI_OK;
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard dev(s->device);
  if (!dev.ok) return fail(MOCHI_EHIP, "hipSetDevice");
  const size_t o_off = align_up(grant_bytes_len, 256), o_len = o_off + align_up(8 * (size_t)n, 256),
               total = o_len + align_up(4 * (size_t)n, 256), sig_bytes = (size_t)MOCHI_RSA_BYTES * n;
  int rc;
  if ((rc = s->pin_in.ensure(total)) || (rc = s->dev_in.ensure(total)) || (rc = s->pin_out.ensure(sig_bytes)) ||
      (rc = s->dev_sig.ensure(sig_bytes)))
    return rc;
  uint8_t* pin = (uint8_t*)s->pin_in.p;
  par_memcpy(pin, grant_bytes, grant_bytes_len);
  memcpy(pin + o_off, grant_off, 8 * (size_t)n);
  memcpy(pin + o_len, grant_len, 4 * (size_t)n);
  uint8_t* din = s->dev_in.as<uint8_t>();
  hipStream_t st = s->stream;
  hipError_t e = hipMemcpyAsync(din, pin, total, hipMemcpyHostToDevice, st);
  if (e == hipSuccess)
    e = mochi::launch_rsa_sign(din, (const uint64_t*)(din + o_off), (const uint32_t*)(din + o_len), n, s->d_key,
                               s->dev_sig.as<uint8_t>(), s->fault_idx, st);
  if (e == hipSuccess) {
    std::lock_guard<std::mutex> ck(s->check->mu);
    if (signer_check(s, din, (const uint64_t*)(din + o_off), (const uint32_t*)(din + o_len), n,
                     s->dev_sig.as<uint8_t>(), st) != MOCHI_OK)
      e = hipErrorUnknown;
  }
  if (e == hipSuccess) e = hipMemcpyAsync(s->pin_out.p, s->dev_sig.p, sig_bytes, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess) memcpy(sig_out, s->pin_out.p, sig_bytes);
  return e == hipSuccess ? MOCHI_OK : fail(MOCHI_EHIP, "sign batch: %s", hipGetErrorString(e));
}

}  // extern "C"

// ---- Write1 grant issuance (w1_issue.hip / w1_issue_host.cpp) ------------------
namespace {

int check_write1(const mochi_write1_batch* b, const mochi_write1_issued* o) {
  if (!b || !o) return fail(MOCHI_EINVAL, "null argument");
  if (b->n_ops >= (1u << 30) || b->n_stored >= MOCHI_W1_STORED || b->n_reqs == 0xFFFFFFFFu)
    return fail(MOCHI_EINVAL, "batch too large");
  if (!b->req_op_off || !o->req_grant_off) return fail(MOCHI_EINVAL, "req_op_off / req_grant_off required");
  if (b->n_reqs && (!b->req_seed || !b->req_hash_off || !b->req_hash_len || !o->req_kind))
    return fail(MOCHI_EINVAL, "req_seed / req_hash_off / req_hash_len / req_kind required");
  if (b->n_ops && (!b->op_key_off || !b->op_key_len || !b->op_flags || !b->op_obj || !b->op_epoch || !b->op_stored ||
                   !o->op_decision || !o->op_grant || !o->req_grant || !o->grant_off || !o->grant_len || !o->grant_op ||
                   !o->grant_ts))
    return fail(MOCHI_EINVAL, "an op or grant array is missing");
  if (b->n_stored && (!b->stored_hash_off || !b->stored_hash_len))
    return fail(MOCHI_EINVAL, "stored_hash_off / stored_hash_len required");
  if (b->strings_len && !b->strings) return fail(MOCHI_EINVAL, "strings required");
  if (o->grant_cap && !o->grant_bytes) return fail(MOCHI_EINVAL, "grant_bytes required");
  return MOCHI_OK;
}

int run_write1_issue_device(mochi_signer* s, const mochi_write1_batch* b, mochi_write1_issued* o, hipStream_t st) {
  const uint32_t Q = b->n_reqs, O = b->n_ops;
  EncState& x = s->w1;
  mochi::W1Args a;
  memset(&a, 0, sizeof a);
  a.b = *b;
  a.o = *o;
  a.slots = (uint32_t)mochi::w1_table_slots(O);
  const uint32_t scan_n = mochi::w2_small(O) && mochi::w2_small(Q) ? 0 : (O > Q ? O : Q) + 1;
  int rc = x.begin(a, mochi::w1_layout, scan_n, 16, s->profiling, mochi::kW1Events);
  if (rc) return rc;
  // one scratch per signer: a call on another stream waits for the last call's kernels
  HIP_TRY(s->order.acquire(st));
  HIP_TRY(mochi::launch_w1_decide(a, st));
  if ((rc = x.fetch_totals(a.totals, 16, s->ev_tot, st))) return rc;
  const uint64_t* tot = (const uint64_t*)x.tot.p;
  o->n_new = (uint32_t)tot[0];
  o->grant_bytes_len = tot[1];
  const bool fits = tot[1] <= o->grant_cap;
  if (fits) {
    HIP_TRY(mochi::launch_w1_emit(a, st));
    if (o->sig && o->n_new) {
      HIP_TRY(mochi::launch_rsa_sign(o->grant_bytes, o->grant_off, o->grant_len, o->n_new, s->d_key, o->sig,
                                     s->fault_idx, st));
      std::lock_guard<std::mutex> ck(s->check->mu);
      if ((rc = signer_check(s, o->grant_bytes, o->grant_off, o->grant_len, o->n_new, o->sig, st))) return rc;
    }
    if (a.ev) HIP_TRY(hipEventRecord(a.ev[mochi::kW1Events - 1], st));
  }
  x.ev_valid = a.ev && fits;
  HIP_TRY(s->order.release(st));
  return fits ? MOCHI_OK : capacity_error("grant_cap", o->grant_cap, "size needed", tot[1]);
}

}  // namespace

extern "C" {

uint64_t mochi_write1_issue_bound(const mochi_write1_batch* b) {
  if (!b) return 0;
  // every op a new grant: key and hash at strings_len each, ten-byte varints throughout
  const unsigned __int128 t = (unsigned __int128)b->n_ops * (2 * (unsigned __int128)b->strings_len + 40);
  return t > ~0ull ? ~0ull : (uint64_t)t;
}

int mochi_write1_issue(const mochi_write1_batch* b, mochi_write1_issued* o, uint64_t* bytes_needed) {
  if (bytes_needed) *bytes_needed = 0;
  int rc = check_write1(b, o);
  if (rc) return rc;
  o->n_new = 0;
  o->grant_bytes_len = 0;
  const char* err = "";
  rc = mochi_host::write1_issue(b, o, &err);
  if (bytes_needed) *bytes_needed = o->grant_bytes_len;
  return rc ? fail(rc, "mochi_write1_issue: %s", err) : MOCHI_OK;
}

int mochi_write1_issue_device(mochi_signer* s, const mochi_write1_batch* b, mochi_write1_issued* o, void* stream) {
  if (!s) return fail(MOCHI_EINVAL, "null signer");
  int rc = check_write1(b, o);
  if (rc) return rc;
  o->n_new = 0;
  o->grant_bytes_len = 0;
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard dev(s->device);
  if (!dev.ok) return fail(MOCHI_EHIP, "hipSetDevice(%d)", s->device);
  return run_write1_issue_device(s, b, o, (hipStream_t)stream);
}

int mochi_signer_set_profiling(mochi_signer* s, int on) {
  if (!s) return fail(MOCHI_EINVAL, "null signer");
  std::lock_guard<std::mutex> lk(s->mu);
  s->profiling = on != 0;
  return MOCHI_OK;
}

int mochi_signer_read_issue_profile(mochi_signer* s, float* kernel_ms, uint32_t n) {
  if (!s || !kernel_ms) return fail(MOCHI_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(s->mu);
  static const int kSpan[mochi::kW1Stages][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {4, 5}, {6, 7}, {7, 8}, {8, 9}};
  return s->w1.read_profile(kSpan, mochi::kW1Stages, kernel_ms, n, "no issue call was made while profiling was on");
}

}  // extern "C"

// ---- Write1 reply encoder (w1_reply.hip / w1_reply_host.cpp) --------------------
namespace {

int check_write1_reply(const mochi_write1_batch* b, const mochi_write1_issued* o, const mochi_write1_reply_source* s,
                       const uint8_t* wire, uint64_t wire_cap, const uint64_t* msg_off, const uint32_t* msg_len,
                       const uint8_t* status) {
  if (!b || !o || !s) return fail(MOCHI_EINVAL, "null argument");
  if (b->n_ops >= (1u << 30) || b->n_stored >= MOCHI_W1_STORED || b->n_reqs == 0xFFFFFFFFu)
    return fail(MOCHI_EINVAL, "batch too large");
  if (!b->req_op_off || !o->req_grant_off) return fail(MOCHI_EINVAL, "req_op_off / req_grant_off required");
  if (b->n_reqs && (!o->req_kind || !msg_off || !msg_len || !status))
    return fail(MOCHI_EINVAL, "req_kind / msg_off / msg_len / status required");
  if (b->n_ops && (!b->op_key_off || !b->op_key_len || !o->op_decision || !o->op_grant || !o->req_grant))
    return fail(MOCHI_EINVAL, "op_key_off / op_key_len / op_decision / op_grant / req_grant required");
  if (o->n_new > b->n_ops) return fail(MOCHI_EINVAL, "n_new exceeds n_ops");
  if (o->n_new && (!o->grant_bytes || !o->grant_off || !o->grant_len))
    return fail(MOCHI_EINVAL, "grant_bytes / grant_off / grant_len required");
  if (b->strings_len && !b->strings) return fail(MOCHI_EINVAL, "strings required");
  if (s->ids_len && !s->ids) return fail(MOCHI_EINVAL, "ids required");
  if (!s->req_client_off != !s->req_client_len) return fail(MOCHI_EINVAL, "req_client_off and req_client_len go together");
  if (b->n_stored && (!s->stored_off || !s->stored_len || (s->stored_bytes_len && !s->stored_bytes)))
    return fail(MOCHI_EINVAL, "stored_bytes / stored_off / stored_len required");
  if (o->sig && b->n_stored && !s->stored_sig)
    return fail(MOCHI_EINVAL, "stored_sig is required when signatures are written and n_stored > 0");
  if (!s->op_cert_off != !s->op_cert_len) return fail(MOCHI_EINVAL, "op_cert_off and op_cert_len go together");
  if (s->op_cert_off && s->certs_len && !s->certs) return fail(MOCHI_EINVAL, "certs required");
  if (wire_cap && !wire) return fail(MOCHI_EINVAL, "wire required");
  return MOCHI_OK;
}

int run_write1_reply_device(mochi_signer* s, const mochi_write1_batch* b, const mochi_write1_issued* o,
                            const mochi_write1_reply_source* src, uint8_t* wire, uint64_t wire_cap, uint64_t* msg_off,
                            uint32_t* msg_len, uint8_t* status, uint64_t* wire_len, uint64_t* wire_len_dev,
                            hipStream_t st) {
  const uint32_t Q = b->n_reqs;
  EncState& x = s->w1r;
  if (wire_len) *wire_len = 0;
  x.ev_valid = false;
  if (Q == 0) {
    if (!wire_len) HIP_TRY(hipMemsetAsync(wire_len_dev, 0, 8, st));
    return MOCHI_OK;
  }
  mochi::W1ReplyArgs a;
  memset(&a, 0, sizeof a);
  a.b = *b;
  a.o = *o;
  a.src = *src;
  a.wire = wire;
  a.wire_cap = wire_cap;
  a.msg_off = msg_off;
  a.msg_len = msg_len;
  a.status = status;
  int rc = x.begin(a, mochi::w1r_layout, mochi::w2_small(Q) ? 0 : Q + 1, 8, s->profiling, mochi::kW1ReplyEvents);
  if (rc) return rc;
  // one scratch per signer: a call on another stream waits for the last call's kernels
  // (an issue call's included: its outputs are this call's inputs)
  HIP_TRY(s->order.acquire(st));
  HIP_TRY(mochi::launch_w1r_size(a, st));
  bool fits = true;
  uint64_t need = 0;
  if (wire_len) {
    if ((rc = x.fetch_totals(a.off64 + Q, 8, s->ev_tot, st))) return rc;
    *wire_len = need = *(const uint64_t*)x.tot.p;
    fits = need <= wire_cap;
  } else {
    HIP_TRY(hipMemcpyAsync(wire_len_dev, a.off64 + Q, 8, hipMemcpyDeviceToDevice, st));
  }
  if (fits) HIP_TRY(mochi::launch_w1r_emit(a, st));
  x.ev_valid = a.ev && fits;
  HIP_TRY(s->order.release(st));
  return fits ? MOCHI_OK : capacity_error("wire_cap", wire_cap, "encoded size", need);
}

}  // namespace

extern "C" {

uint64_t mochi_write1_reply_bound(uint32_t n_reqs, uint32_t n_ops, uint64_t strings_len, uint64_t ids_len,
                                  uint64_t grant_bytes_len, uint64_t stored_bytes_len, uint64_t certs_len,
                                  int with_signatures) {
  // every op an entry of all three maps (its key three times), five-byte length varints throughout
  const unsigned __int128 g = grant_bytes_len > stored_bytes_len ? grant_bytes_len : stored_bytes_len;
  unsigned __int128 t = (unsigned __int128)n_ops * (3 * (unsigned __int128)strings_len + g + certs_len + 64 +
                                                    (with_signatures ? MOCHI_RSA_BYTES : 0)) +
                        (unsigned __int128)n_reqs * (2 * (unsigned __int128)ids_len + 24);
  const unsigned __int128 cap = (unsigned __int128)n_reqs * mochi::kEncMaxMsg;  // longer bodies are emitted empty
  if (t > cap) t = cap;
  return (uint64_t)t;
}

int mochi_write1_reply_encode(const mochi_write1_batch* b, const mochi_write1_issued* o,
                              const mochi_write1_reply_source* src, uint8_t* wire, uint64_t wire_cap, uint64_t* msg_off,
                              uint32_t* msg_len, uint8_t* status, uint64_t* wire_len) {
  if (!wire_len) return fail(MOCHI_EINVAL, "wire_len required");
  *wire_len = 0;
  int rc = check_write1_reply(b, o, src, wire, wire_cap, msg_off, msg_len, status);
  if (rc) return rc;
  const char* err = "";
  rc = mochi_host::write1_reply_encode(b, o, src, wire, wire_cap, msg_off, msg_len, status, wire_len, &err);
  return rc ? fail(rc, "mochi_write1_reply_encode: %s", err) : MOCHI_OK;
}

int mochi_write1_reply_encode_device(mochi_signer* s, const mochi_write1_batch* b, const mochi_write1_issued* o,
                                     const mochi_write1_reply_source* src, uint8_t* wire, uint64_t wire_cap,
                                     uint64_t* msg_off, uint32_t* msg_len, uint8_t* status, uint64_t* wire_len,
                                     uint64_t* wire_len_dev, void* stream) {
  if (!s) return fail(MOCHI_EINVAL, "null signer");
  if (!wire_len && !wire_len_dev) return fail(MOCHI_EINVAL, "wire_len or wire_len_dev required");
  int rc = check_write1_reply(b, o, src, wire, wire_cap, msg_off, msg_len, status);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard dev(s->device);
  if (!dev.ok) return fail(MOCHI_EHIP, "hipSetDevice(%d)", s->device);
  return run_write1_reply_device(s, b, o, src, wire, wire_cap, msg_off, msg_len, status, wire_len, wire_len_dev,
                                 (hipStream_t)stream);
}

int mochi_signer_read_reply_profile(mochi_signer* s, float* kernel_ms, uint32_t n) {
  if (!s || !kernel_ms) return fail(MOCHI_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(s->mu);
  static const int kSpan[mochi::kW1ReplyStages][2] = {{0, 1}, {1, 2}, {3, 4}, {4, 5}};
  return s->w1r.read_profile(kSpan, mochi::kW1ReplyStages, kernel_ms, n,
                             "no reply encode call was made while profiling was on");
}

}  // extern "C"

// ---- Write1 request decoder and key-state join (w1_request.hip / w1_request_host.cpp) ----
namespace {

int check_write1_requests(const mochi_write1_requests* r, const mochi_write1_requests_decoded* o) {
  if (!r || !o) return fail(MOCHI_EINVAL, "null argument");
  if (!o->req_op_off) return fail(MOCHI_EINVAL, "req_op_off required");
  if (r->n_reqs && (!r->msg_off || !r->msg_len || (!r->wire && r->wire_len)))
    return fail(MOCHI_EINVAL, "wire / msg_off / msg_len required");
  if (r->n_reqs && (!o->req_status || !o->req_seed || !o->req_hash_off || !o->req_hash_len || !o->req_client_off ||
                    !o->req_client_len))
    return fail(MOCHI_EINVAL, "the per-request outputs are required");
  if (r->n_reqs > mochi::w1q::kMaxReqs) return fail(MOCHI_EINVAL, "more than 2^24 requests");
  if (o->op_cap && (!o->op_key_off || !o->op_key_len || !o->op_flags || !o->op_obj || !o->key_op))
    return fail(MOCHI_EINVAL, "the per-op outputs and key_op are required (op_cap > 0)");
  return MOCHI_OK;
}

int w1q_capacity_error(const mochi_write1_requests_decoded* o) {
  return capacity_error("op_cap", o->op_cap, "decoded ops", o->n_ops);
}

int run_write1_request_device(mochi_signer* s, const mochi_write1_requests* r, mochi_write1_requests_decoded* o,
                              uint32_t* n_keys_dev, hipStream_t st) {
  const uint32_t Q = r->n_reqs;
  EncState& x = s->w1q;
  o->n_ops = o->n_keys = 0;
  mochi::W1ReqArgs a;
  memset(&a, 0, sizeof a);
  a.v.in = *r;
  a.v.out = *o;
  a.Q = Q;
  a.n_keys = n_keys_dev;
  int rc = x.begin(a, mochi::w1q_layout, Q + 1, 8, s->profiling, mochi::kW1ReqEvents);
  if (rc) return rc;
  // one scratch per signer: a call on another stream waits for the last call's kernels
  HIP_TRY(s->order.acquire(st));
  HIP_TRY(mochi::launch_w1q_count(a, st));
  if ((rc = x.fetch_totals(a.off64 + Q, 8, s->ev_tot, st))) return rc;
  const uint64_t tot = *(const uint64_t*)x.tot.p;
  o->n_ops = a.n_ops = (uint32_t)tot;
  const bool fits = o->n_ops <= o->op_cap;
  if (fits) {
    a.k.n_ops = a.n_ops;
    a.k.slots = (uint32_t)mochi::w1_table_slots(a.n_ops);
    size_t scan_bytes = 0;
    HIP_TRY(mochi::enc_scan_temp_bytes(a.n_ops + 1, &scan_bytes));
    if ((rc = s->w1q_tab.ensure(mochi::key_table_layout(a.k, nullptr))) || (rc = x.scan.ensure(scan_bytes))) return rc;
    mochi::key_table_layout(a.k, s->w1q_tab.p);
    a.scan_temp = x.scan.p;
    a.scan_temp_bytes = x.scan.cap;
    HIP_TRY(mochi::launch_w1q_emit(a, st));
  }
  x.ev_valid = a.ev && fits;
  HIP_TRY(s->order.release(st));
  return fits ? MOCHI_OK : w1q_capacity_error(o);
}

int check_write1_join(uint32_t n_ops, const uint32_t* req_op_off, const uint32_t* req_seed, const uint8_t* op_flags_wire,
                      const uint32_t* op_obj, const mochi_write1_key_state* k, const uint8_t* op_flags,
                      const int64_t* op_epoch, const uint32_t* op_stored) {
  if (!k || !req_op_off) return fail(MOCHI_EINVAL, "null argument");
  if (n_ops && (!req_seed || !op_flags_wire || !op_obj || !op_flags || !op_epoch || !op_stored))
    return fail(MOCHI_EINVAL, "an op array or req_seed is missing");
  if (!k->key_given_off || (k->n_keys && (!k->key_flags || !k->key_epoch)) ||
      (k->n_given && (!k->given_ts || !k->given_stored)))
    return fail(MOCHI_EINVAL, "a key state array is missing");
  return MOCHI_OK;
}

}  // namespace

extern "C" {

uint64_t mochi_write1_request_decode_bound(uint64_t wire_len, uint32_t n_reqs) {
  const uint64_t per = wire_len / 2 < mochi::w1q::kMaxOps ? wire_len / 2 : mochi::w1q::kMaxOps;
  return per * n_reqs;
}

int mochi_write1_request_decode(const mochi_write1_requests* r, mochi_write1_requests_decoded* o) {
  int rc = check_write1_requests(r, o);
  if (rc) return rc;
  const char* err = nullptr;
  rc = mochi_host::write1_request_decode(r, o, &err);
  if (rc && err) return fail(rc, "mochi_write1_request_decode: %s", err);
  return rc ? w1q_capacity_error(o) : MOCHI_OK;
}

int mochi_write1_request_decode_device(mochi_signer* s, const mochi_write1_requests* r, mochi_write1_requests_decoded* o,
                                       uint32_t* n_keys_dev, void* stream) {
  if (!s) return fail(MOCHI_EINVAL, "null signer");
  if (!n_keys_dev) return fail(MOCHI_EINVAL, "n_keys_dev required");
  int rc = check_write1_requests(r, o);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard dev(s->device);
  if (!dev.ok) return fail(MOCHI_EHIP, "hipSetDevice(%d)", s->device);
  return run_write1_request_device(s, r, o, n_keys_dev, (hipStream_t)stream);
}

int mochi_signer_read_request_profile(mochi_signer* s, float* kernel_ms, uint32_t n) {
  if (!s || !kernel_ms) return fail(MOCHI_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(s->mu);
  static const int kSpan[mochi::kW1ReqStages][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {5, 6}, {6, 7}, {7, 8}, {8, 9}, {9, 10}};
  return s->w1q.read_profile(kSpan, mochi::kW1ReqStages, kernel_ms, n,
                             "no request decode call was made while profiling was on");
}

int mochi_write1_state_join(uint32_t n_reqs, uint32_t n_ops, const uint32_t* req_op_off, const uint32_t* req_seed,
                            const uint8_t* op_flags_wire, const uint32_t* op_obj, const mochi_write1_key_state* keys,
                            uint8_t* op_flags, int64_t* op_epoch, uint32_t* op_stored) {
  int rc = check_write1_join(n_ops, req_op_off, req_seed, op_flags_wire, op_obj, keys, op_flags, op_epoch, op_stored);
  if (rc) return rc;
  const mochi::w1q::JoinArgs a{n_reqs, n_ops, req_op_off, req_seed, op_flags_wire, op_obj, *keys, op_flags, op_epoch, op_stored};
  const char* err = nullptr;
  rc = mochi_host::write1_state_join(&a, &err);
  return rc ? fail(rc, "mochi_write1_state_join: %s", err) : MOCHI_OK;
}

int mochi_write1_state_join_device(mochi_signer* s, uint32_t n_reqs, uint32_t n_ops, const uint32_t* req_op_off,
                                   const uint32_t* req_seed, const uint8_t* op_flags_wire, const uint32_t* op_obj,
                                   const mochi_write1_key_state* keys, uint8_t* op_flags, int64_t* op_epoch,
                                   uint32_t* op_stored, void* stream) {
  if (!s) return fail(MOCHI_EINVAL, "null signer");
  int rc = check_write1_join(n_ops, req_op_off, req_seed, op_flags_wire, op_obj, keys, op_flags, op_epoch, op_stored);
  if (rc) return rc;
  DeviceGuard dev(s->device);
  if (!dev.ok) return fail(MOCHI_EHIP, "hipSetDevice(%d)", s->device);
  const mochi::w1q::JoinArgs a{n_reqs, n_ops, req_op_off, req_seed, op_flags_wire, op_obj, *keys, op_flags, op_epoch, op_stored};
  HIP_TRY(mochi::launch_w1q_join(a, (hipStream_t)stream));
  return MOCHI_OK;
}

}  // extern "C"

// ---- result reply decoder and coalescing (result_decode.hip / result_decode_host.cpp) ----
namespace {

int check_result_replies(const mochi_result_replies* r, const mochi_result_decoded* o) {
  if (!r || !o) return fail(MOCHI_EINVAL, "null argument");
  if (r->n_resps > mochi::wire::kMaxResps) return fail(MOCHI_EINVAL, "more than 2^24 responses");
  if (!r->n_resps) return MOCHI_OK;
  if (!r->n_reqs) return fail(MOCHI_EINVAL, "responses without a request");
  if (!r->resp_off || !r->resp_len || !r->resp_kind || (!r->wire && r->wire_len))
    return fail(MOCHI_EINVAL, "wire / resp_off / resp_len / resp_kind required");
  if (!r->req_resp_off || !r->n_ops || !r->slot_off) return fail(MOCHI_EINVAL, "req_resp_off / n_ops / slot_off required");
  if (!o->resp_status || !o->resp_n_ops || !o->resp_rid_off || !o->resp_rid_len || !o->resp_nonce_off ||
      !o->resp_nonce_len)
    return fail(MOCHI_EINVAL, "the per-response outputs are required");
  if (!o->op_status || !o->op_existed || !o->op_flags || !o->op_result_off || !o->op_result_len || !o->op_cert_off ||
      !o->op_cert_len)
    return fail(MOCHI_EINVAL, "the per-slot outputs are required");
  return MOCHI_OK;
}

int check_result_tallied(const mochi_result_tallied* t, const mochi_result_coalesced* o) {
  if (!t || !o) return fail(MOCHI_EINVAL, "null argument");
  if (!t->n_reqs) return MOCHI_OK;
  if (!t->req_resp_off || !t->n_ops || !t->chosen || !t->chosen_off || !t->accept_bits || !t->slot_off || !t->out_off)
    return fail(MOCHI_EINVAL, "req_resp_off / n_ops / chosen / chosen_off / accept_bits / slot_off / out_off required");
  if (!t->op_status || !t->op_existed || !t->op_flags || !t->op_result_off || !t->op_result_len || !t->op_cert_off ||
      !t->op_cert_len)
    return fail(MOCHI_EINVAL, "the per-slot inputs are required");
  if (!o->resp || !o->status || !o->existed || !o->flags || !o->result_off || !o->result_len || !o->cert_off ||
      !o->cert_len)
    return fail(MOCHI_EINVAL, "the coalesced outputs are required");
  return MOCHI_OK;
}

}  // namespace

extern "C" {

int mochi_result_reply_decode(const mochi_result_replies* r, mochi_result_decoded* o) {
  int rc = check_result_replies(r, o);
  if (rc || !r->n_resps) return rc;
  const char* err = nullptr;
  rc = mochi_host::result_reply_decode(r, o, &err);
  return rc ? fail(rc, "mochi_result_reply_decode: %s", err) : MOCHI_OK;
}

int mochi_result_reply_decode_device(mochi_ctx* c, const mochi_result_replies* r, mochi_result_decoded* o,
                                     void* stream) {
  if (!c) return fail(MOCHI_EINVAL, "null context");
  int rc = check_result_replies(r, o);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard dev(c->device);
  if (!dev.ok) return fail(MOCHI_EHIP, "hipSetDevice(%d)", c->device);
  new_call(c);
  EncState& x = c->rr;
  x.ev_valid = false;
  if (!r->n_resps) return MOCHI_OK;
  hipStream_t st = (hipStream_t)stream;
  mochi::RRArgs a;
  memset(&a, 0, sizeof a);
  a.v.in = *r;
  a.v.out = *o;
  a.P = r->n_resps;
  if ((rc = x.begin(a, mochi::rr_layout, a.P + 1, 0, c->profiling, mochi::kRREvents))) return rc;
  HIP_TRY(c->order.acquire(st));
  HIP_TRY(mochi::launch_rr_decode(a, st));
  x.ev_valid = a.ev != nullptr;
  HIP_TRY(c->order.release(st));
  return MOCHI_OK;
}

int mochi_ctx_read_result_decode_profile(mochi_ctx* c, float* kernel_ms, uint32_t n_kernels) {
  if (!c || !kernel_ms) return fail(MOCHI_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(c->mu);
  static const int kSpan[mochi::kRRStages][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 4}};
  return c->rr.read_profile(kSpan, mochi::kRRStages, kernel_ms, n_kernels,
                            "no result reply decode call was made while profiling was on");
}

int mochi_result_coalesce(const mochi_result_tallied* t, mochi_result_coalesced* o) {
  int rc = check_result_tallied(t, o);
  if (rc || !t->n_reqs) return rc;
  const char* err = nullptr;
  rc = mochi_host::result_coalesce(t, o, &err);
  return rc ? fail(rc, "mochi_result_coalesce: %s", err) : MOCHI_OK;
}

int mochi_result_coalesce_device(const mochi_result_tallied* t, mochi_result_coalesced* o, void* stream) {
  int rc = check_result_tallied(t, o);
  if (rc || !t->n_reqs) return rc;
  HIP_TRY(mochi::launch_rr_coalesce(*t, *o, (hipStream_t)stream));
  return MOCHI_OK;
}

}  // extern "C"

// ---- answer encoder and Write2 answer plan (result_encode.hip / result_encode_host.cpp) ----
namespace {

int check_result_answers(const mochi_result_answers* a, const uint8_t* wire, uint64_t wire_cap, const uint64_t* msg_off,
                         const uint32_t* msg_len, const uint8_t* status) {
  if (!a) return fail(MOCHI_EINVAL, "null argument");
  if (a->n_resps == 0xFFFFFFFFu) return fail(MOCHI_EINVAL, "batch too large");
  if (!a->n_resps) return MOCHI_OK;
  if (!a->resp_kind || !a->resp_n_ops || !a->slot_off || !msg_off || !msg_len || !status)
    return fail(MOCHI_EINVAL, "resp_kind / resp_n_ops / slot_off / msg_off / msg_len / status required");
  if (!a->rid_off != !a->rid_len) return fail(MOCHI_EINVAL, "rid_off and rid_len go together");
  if (!a->nonce_off != !a->nonce_len) return fail(MOCHI_EINVAL, "nonce_off and nonce_len go together");
  if ((a->rid_off || a->nonce_off) && a->ids_len && !a->ids) return fail(MOCHI_EINVAL, "ids required");
  if (a->n_slots && (!a->op_status || !a->op_existed || !a->op_flags || !a->op_result_off || !a->op_result_len ||
                     !a->op_cert_off || !a->op_cert_len))
    return fail(MOCHI_EINVAL, "the per-slot arrays are required");
  if (a->wire_len && !a->wire) return fail(MOCHI_EINVAL, "wire required");
  if (a->store_len && !a->store) return fail(MOCHI_EINVAL, "store required");
  if (wire_cap && !wire) return fail(MOCHI_EINVAL, "wire_out required");
  return MOCHI_OK;
}

int check_write2_answer(const mochi_write2_batch* b, const mochi_write2_answer_source* s,
                        const mochi_write2_answer_planned* o) {
  if (!b || !s || !o) return fail(MOCHI_EINVAL, "null argument");
  if (b->n_msgs == 0xFFFFFFFFu) return fail(MOCHI_EINVAL, "batch too large");
  if (!b->n_msgs) return MOCHI_OK;
  if (!b->msg_off || !b->msg_len || !b->op_flags_off || (!b->wire && b->wire_len))
    return fail(MOCHI_EINVAL, "wire / msg_off / msg_len / op_flags_off required");
  if (!s->msg_status || !s->cert_accept_bits || !s->op_decision || !s->op_value_off || !s->op_value_len ||
      !s->op_stored_cert_off || !s->op_stored_cert_len || !s->op_store_flags || !s->slot_off)
    return fail(MOCHI_EINVAL, "every array of the answer source is required");
  if (!o->plan_status || !o->resp_kind || !o->resp_n_ops || !o->op_status || !o->op_existed || !o->op_flags ||
      !o->op_result_off || !o->op_result_len || !o->op_cert_off || !o->op_cert_len)
    return fail(MOCHI_EINVAL, "every output array is required");
  return MOCHI_OK;
}

int run_result_encode_device(mochi_ctx* c, const mochi_result_answers* in, uint8_t* wire, uint64_t wire_cap,
                             uint64_t* msg_off, uint32_t* msg_len, uint8_t* status, uint64_t* wire_len,
                             uint64_t* wire_len_dev, hipStream_t st) {
  const uint32_t P = in->n_resps;
  EncState& x = c->rae;
  if (wire_len) *wire_len = 0;
  x.ev_valid = false;
  if (P == 0) {
    if (!wire_len) HIP_TRY(hipMemsetAsync(wire_len_dev, 0, 8, st));
    return MOCHI_OK;
  }
  mochi::RaeArgs a;
  memset(&a, 0, sizeof a);
  a.in = *in;
  a.wire = wire;
  a.wire_cap = wire_cap;
  a.msg_off = msg_off;
  a.msg_len = msg_len;
  a.status = status;
  int rc = x.begin(a, mochi::rae_layout, mochi::w2_small(P) ? 0 : P + 1, 8, c->profiling, mochi::kRaeEvents);
  if (rc) return rc;
  // the context's scratch: a call on another stream waits for the last call's kernels
  HIP_TRY(c->order.acquire(st));
  HIP_TRY(mochi::launch_rae_size(a, st));
  bool fits = true;
  uint64_t need = 0;
  if (wire_len) {
    if ((rc = x.fetch_totals(a.off64 + P, 8, c->ev_tot, st))) return rc;
    *wire_len = need = *(const uint64_t*)x.tot.p;
    fits = need <= wire_cap;
  } else {
    HIP_TRY(hipMemcpyAsync(wire_len_dev, a.off64 + P, 8, hipMemcpyDeviceToDevice, st));
  }
  if (fits) HIP_TRY(mochi::launch_rae_emit(a, st));
  x.ev_valid = a.ev && fits;
  HIP_TRY(c->order.release(st));
  return fits ? MOCHI_OK : capacity_error("wire_cap", wire_cap, "encoded size", need);
}

}  // namespace

extern "C" {

uint64_t mochi_result_reply_encode_bound(uint32_t n_resps, uint64_t n_ops, uint64_t wire_len, uint64_t store_len,
                                         uint64_t ids_len) {
  // every op with a result and a certificate as long as the larger blob, every response with
  // rid and nonce at ids_len, five-byte length varints and a two-byte status throughout
  const unsigned __int128 blob = wire_len > store_len ? wire_len : store_len;
  unsigned __int128 t = (unsigned __int128)n_ops * (2 * blob + 24) + (unsigned __int128)n_resps * (2 * (unsigned __int128)ids_len + 18);
  const unsigned __int128 cap = (unsigned __int128)n_resps * mochi::kEncMaxMsg;  // longer bodies are emitted empty
  if (t > cap) t = cap;
  return (uint64_t)t;
}

int mochi_result_reply_encode(const mochi_result_answers* a, uint8_t* wire, uint64_t wire_cap, uint64_t* msg_off,
                              uint32_t* msg_len, uint8_t* status, uint64_t* wire_len) {
  if (!wire_len) return fail(MOCHI_EINVAL, "wire_len required");
  *wire_len = 0;
  int rc = check_result_answers(a, wire, wire_cap, msg_off, msg_len, status);
  if (rc || !a->n_resps) return rc;
  const char* err = "";
  rc = mochi_host::result_reply_encode(a, wire, wire_cap, msg_off, msg_len, status, wire_len, &err);
  return rc ? fail(rc, "mochi_result_reply_encode: %s", err) : MOCHI_OK;
}

int mochi_result_reply_encode_device(mochi_ctx* c, const mochi_result_answers* a, uint8_t* wire, uint64_t wire_cap,
                                     uint64_t* msg_off, uint32_t* msg_len, uint8_t* status, uint64_t* wire_len,
                                     uint64_t* wire_len_dev, void* stream) {
  if (!c) return fail(MOCHI_EINVAL, "null context");
  if (!wire_len && !wire_len_dev) return fail(MOCHI_EINVAL, "wire_len or wire_len_dev required");
  int rc = check_result_answers(a, wire, wire_cap, msg_off, msg_len, status);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard dev(c->device);
  if (!dev.ok) return fail(MOCHI_EHIP, "hipSetDevice(%d)", c->device);
  new_call(c);
  return run_result_encode_device(c, a, wire, wire_cap, msg_off, msg_len, status, wire_len, wire_len_dev,
                                  (hipStream_t)stream);
}

int mochi_ctx_read_result_encode_profile(mochi_ctx* c, float* kernel_ms, uint32_t n_kernels) {
  if (!c || !kernel_ms) return fail(MOCHI_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(c->mu);
  static const int kSpan[mochi::kRaeStages][2] = {{0, 1}, {1, 2}, {3, 4}, {4, 5}};
  return c->rae.read_profile(kSpan, mochi::kRaeStages, kernel_ms, n_kernels,
                             "no answer encode call was made while profiling was on");
}

int mochi_write2_answer_plan(const mochi_write2_batch* b, const mochi_write2_answer_source* s,
                             mochi_write2_answer_planned* o) {
  int rc = check_write2_answer(b, s, o);
  if (rc || !b->n_msgs) return rc;
  const char* err = "";
  rc = mochi_host::write2_answer_plan(b, s, o, &err);
  return rc ? fail(rc, "mochi_write2_answer_plan: %s", err) : MOCHI_OK;
}

int mochi_write2_answer_plan_device(const mochi_write2_batch* b, const mochi_write2_answer_source* s,
                                    mochi_write2_answer_planned* o, void* stream) {
  int rc = check_write2_answer(b, s, o);
  if (rc || !b->n_msgs) return rc;
  const mochi::rae::PlanView v{*b, *s, *o};
  HIP_TRY(mochi::launch_w2a_plan(v, (hipStream_t)stream));
  return MOCHI_OK;
}

}  // extern "C"

// ---- read request decoder and read answer plan (read_request.hip / read_request_host.cpp) ----
namespace {

int check_read_requests(const mochi_read_requests* r, const mochi_read_requests_decoded* o) {
  if (!r || !o) return fail(MOCHI_EINVAL, "null argument");
  if (!o->req_op_off) return fail(MOCHI_EINVAL, "req_op_off required");
  if (r->n_reqs && (!r->msg_off || !r->msg_len || (!r->wire && r->wire_len)))
    return fail(MOCHI_EINVAL, "wire / msg_off / msg_len required");
  if (r->n_reqs && (!o->req_status || !o->req_client_off || !o->req_client_len || !o->req_nonce_off || !o->req_nonce_len))
    return fail(MOCHI_EINVAL, "the per-request outputs are required");
  if (r->n_reqs > mochi::rdq::kMaxReqs) return fail(MOCHI_EINVAL, "more than 2^24 requests");
  if (o->op_cap && (!o->op_key_off || !o->op_key_len || !o->op_flags || !o->op_obj || !o->key_op))
    return fail(MOCHI_EINVAL, "the per-op outputs and key_op are required (op_cap > 0)");
  return MOCHI_OK;
}

int rdq_capacity_error(const mochi_read_requests_decoded* o) {
  return capacity_error("op_cap", o->op_cap, "decoded ops", o->n_ops);
}

int run_read_request_device(mochi_ctx* c, const mochi_read_requests* r, mochi_read_requests_decoded* o,
                            uint32_t* n_keys_dev, hipStream_t st) {
  const uint32_t Q = r->n_reqs;
  EncState& x = c->rdq;
  o->n_ops = o->n_keys = 0;
  mochi::RdReqArgs a;
  memset(&a, 0, sizeof a);
  a.v.in = *r;
  a.v.out = *o;
  a.Q = Q;
  a.n_keys = n_keys_dev;
  int rc = x.begin(a, mochi::rdq_layout, Q + 1, 8, c->profiling, mochi::kRdReqEvents);
  if (rc) return rc;
  // the context's scratch: a call on another stream waits for the last call's kernels
  HIP_TRY(c->order.acquire(st));
  HIP_TRY(mochi::launch_rdq_count(a, st));
  if ((rc = x.fetch_totals(a.off64 + Q, 8, c->ev_tot, st))) return rc;
  o->n_ops = a.n_ops = (uint32_t)*(const uint64_t*)x.tot.p;
  const bool fits = o->n_ops <= o->op_cap;
  if (fits) {
    a.k.n_ops = a.n_ops;
    a.k.slots = (uint32_t)mochi::w1_table_slots(a.n_ops);
    size_t scan_bytes = 0;
    HIP_TRY(mochi::enc_scan_temp_bytes(a.n_ops + 1, &scan_bytes));
    if ((rc = c->rdq_tab.ensure(mochi::key_table_layout(a.k, nullptr))) || (rc = x.scan.ensure(scan_bytes))) return rc;
    mochi::key_table_layout(a.k, c->rdq_tab.p);
    a.scan_temp = x.scan.p;
    a.scan_temp_bytes = x.scan.cap;
    HIP_TRY(mochi::launch_rdq_emit(a, st));
  }
  x.ev_valid = a.ev && fits;
  HIP_TRY(c->order.release(st));
  return fits ? MOCHI_OK : rdq_capacity_error(o);
}

int check_read_plan(uint32_t n_reqs, const mochi_read_requests_decoded* d, const mochi_read_key_state* k,
                    const mochi_read_answer_planned* o) {
  if (!n_reqs) return MOCHI_OK;
  if (!d || !k || !o) return fail(MOCHI_EINVAL, "null argument");
  if (!d->req_status || !d->req_op_off) return fail(MOCHI_EINVAL, "req_status / req_op_off required");
  if (d->n_ops && (!d->op_key_len || !d->op_flags || !d->op_obj)) return fail(MOCHI_EINVAL, "an op array is missing");
  if (k->n_keys && (!k->key_flags || !k->key_value_off || !k->key_value_len || !k->key_cert_off || !k->key_cert_len))
    return fail(MOCHI_EINVAL, "a key state array is missing");
  if (!o->plan_status || !o->resp_kind || !o->resp_n_ops || !o->slot_off)
    return fail(MOCHI_EINVAL, "plan_status / resp_kind / resp_n_ops / slot_off required");
  if (d->n_ops && (!o->op_status || !o->op_existed || !o->op_flags || !o->op_result_off || !o->op_result_len ||
                   !o->op_cert_off || !o->op_cert_len))
    return fail(MOCHI_EINVAL, "the per-slot outputs are required");
  return MOCHI_OK;
}

}  // namespace

extern "C" {

uint64_t mochi_read_request_decode_bound(uint64_t wire_len, uint32_t n_reqs) {
  return mochi_write1_request_decode_bound(wire_len, n_reqs);
}

int mochi_read_request_decode(const mochi_read_requests* r, mochi_read_requests_decoded* o) {
  int rc = check_read_requests(r, o);
  if (rc) return rc;
  const char* err = nullptr;
  rc = mochi_host::read_request_decode(r, o, &err);
  if (rc && err) return fail(rc, "mochi_read_request_decode: %s", err);
  return rc ? rdq_capacity_error(o) : MOCHI_OK;
}

int mochi_read_request_decode_device(mochi_ctx* c, const mochi_read_requests* r, mochi_read_requests_decoded* o,
                                     uint32_t* n_keys_dev, void* stream) {
  if (!c) return fail(MOCHI_EINVAL, "null context");
  if (!n_keys_dev) return fail(MOCHI_EINVAL, "n_keys_dev required");
  int rc = check_read_requests(r, o);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard dev(c->device);
  if (!dev.ok) return fail(MOCHI_EHIP, "hipSetDevice(%d)", c->device);
  new_call(c);
  return run_read_request_device(c, r, o, n_keys_dev, (hipStream_t)stream);
}

int mochi_ctx_read_read_decode_profile(mochi_ctx* c, float* kernel_ms, uint32_t n) {
  if (!c || !kernel_ms) return fail(MOCHI_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(c->mu);
  static const int kSpan[mochi::kRdReqStages][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {5, 6}, {6, 7}, {7, 8}, {8, 9}, {9, 10}};
  return c->rdq.read_profile(kSpan, mochi::kRdReqStages, kernel_ms, n,
                             "no read request decode call was made while profiling was on");
}

int mochi_read_answer_plan(uint32_t n_reqs, const mochi_read_requests_decoded* d, const mochi_read_key_state* k,
                           mochi_read_answer_planned* o) {
  int rc = check_read_plan(n_reqs, d, k, o);
  if (rc || !n_reqs) return rc;
  const mochi::rdq::PlanView v{n_reqs, *d, *k, *o};
  const char* err = "";
  rc = mochi_host::read_answer_plan(&v, &err);
  return rc ? fail(rc, "mochi_read_answer_plan: %s", err) : MOCHI_OK;
}

int mochi_read_answer_plan_device(uint32_t n_reqs, const mochi_read_requests_decoded* d, const mochi_read_key_state* k,
                                  mochi_read_answer_planned* o, void* stream) {
  int rc = check_read_plan(n_reqs, d, k, o);
  if (rc || !n_reqs) return rc;
  const mochi::rdq::PlanView v{n_reqs, *d, *k, *o};
  HIP_TRY(mochi::launch_rda_plan(v, (hipStream_t)stream));
  return MOCHI_OK;
}

}  // extern "C"

// ---- the ProtocolMessage envelope (envelope.hip / envelope_host.cpp) ----
namespace {

int check_env_frames(const mochi_envelope_frames* f) {
  if (!f) return fail(MOCHI_EINVAL, "null argument");
  if (f->n_frames > mochi::env::kMaxFrames) return fail(MOCHI_EINVAL, "more than 2^24 frames");
  if (f->n_frames && (!f->frame_off || !f->frame_len || (!f->wire && f->wire_len)))
    return fail(MOCHI_EINVAL, "wire / frame_off / frame_len required");
  return MOCHI_OK;
}

int check_env_decode(const mochi_envelope_frames* f, const mochi_envelope_decoded* o) {
  int rc = check_env_frames(f);
  if (rc) return rc;
  if (!o) return fail(MOCHI_EINVAL, "null argument");
  if (f->n_frames && (!o->status || !o->kind || !o->body_off || !o->body_len || !o->msg_timestamp || !o->server_id_off ||
                      !o->server_id_len || !o->msg_id_off || !o->msg_id_len || !o->reply_to_off || !o->reply_to_len))
    return fail(MOCHI_EINVAL, "every output array is required");
  return MOCHI_OK;
}

int check_env_route(uint32_t n, const uint8_t* status, const uint8_t* kind, const uint64_t* body_off,
                    const uint32_t* body_len, const mochi_envelope_routed* o) {
  if (!o || !o->kind_off) return fail(MOCHI_EINVAL, "kind_off required");
  if (n > mochi::env::kMaxFrames) return fail(MOCHI_EINVAL, "more than 2^24 frames");
  if (n && (!status || !kind || !body_off || !body_len)) return fail(MOCHI_EINVAL, "status / kind / body_off / body_len required");
  if (n && (!o->order || !o->body_off || !o->body_len)) return fail(MOCHI_EINVAL, "every output array is required");
  return MOCHI_OK;
}

int check_env_join(const mochi_envelope_requests* r, const mochi_envelope_frames* f, const mochi_envelope_decoded* d,
                   const mochi_envelope_joined* o) {
  int rc = check_env_frames(f);
  if (rc) return rc;
  if (!r || !d || !o) return fail(MOCHI_EINVAL, "null argument");
  if (r->n_reqs > mochi::env::kMaxFrames) return fail(MOCHI_EINVAL, "more than 2^24 requests");
  if (r->n_reqs && (!r->id_off || !r->id_len || (!r->ids && r->ids_len))) return fail(MOCHI_EINVAL, "ids / id_off / id_len required");
  if (!o->req_resp_off) return fail(MOCHI_EINVAL, "req_resp_off required");
  if (f->n_frames && (!d->status || !d->kind || !d->body_off || !d->body_len || !d->reply_to_off || !d->reply_to_len))
    return fail(MOCHI_EINVAL, "status / kind / body_off / body_len / reply_to_off / reply_to_len required");
  if (f->n_frames && (!o->frame_req || !o->resp_frame || !o->resp_off || !o->resp_len || !o->resp_w1_kind || !o->resp_rr_kind))
    return fail(MOCHI_EINVAL, "every output array is required");
  return MOCHI_OK;
}

int check_env_source(const mochi_envelope_source* s, const uint8_t* wire, uint64_t wire_cap, const uint64_t* msg_off,
                     const uint32_t* msg_len, const uint8_t* status) {
  if (!s) return fail(MOCHI_EINVAL, "null argument");
  if (s->n_msgs == 0xFFFFFFFFu) return fail(MOCHI_EINVAL, "batch too large");
  if (s->flags & ~(uint32_t)MOCHI_ENV_LENGTH_PREFIX) return fail(MOCHI_EINVAL, "unknown flags");
  if (!s->n_msgs) return MOCHI_OK;
  if (!s->kind || !s->body_off || !s->body_len || !s->msg_timestamp || !msg_off || !msg_len || !status)
    return fail(MOCHI_EINVAL, "kind / body_off / body_len / msg_timestamp / msg_off / msg_len / status required");
  if (!s->msg_id_off != !s->msg_id_len) return fail(MOCHI_EINVAL, "msg_id_off and msg_id_len go together");
  if (!s->reply_to_off != !s->reply_to_len) return fail(MOCHI_EINVAL, "reply_to_off and reply_to_len go together");
  if (!s->server_id_off != !s->server_id_len) return fail(MOCHI_EINVAL, "server_id_off and server_id_len go together");
  if ((s->msg_id_off || s->reply_to_off || s->server_id_off) && s->ids_len && !s->ids) return fail(MOCHI_EINVAL, "ids required");
  if (s->bodies_len && !s->bodies) return fail(MOCHI_EINVAL, "bodies required");
  if (wire_cap && !wire) return fail(MOCHI_EINVAL, "wire_out required");
  return MOCHI_OK;
}

}  // namespace

extern "C" {

int mochi_envelope_decode(const mochi_envelope_frames* f, mochi_envelope_decoded* o) {
  int rc = check_env_decode(f, o);
  if (rc || !f->n_frames) return rc;
  const char* err = "";
  rc = mochi_host::envelope_decode(f, o, &err);
  return rc ? fail(rc, "mochi_envelope_decode: %s", err) : MOCHI_OK;
}

int mochi_envelope_decode_device(mochi_ctx* c, const mochi_envelope_frames* f, mochi_envelope_decoded* o, void* stream) {
  if (!c) return fail(MOCHI_EINVAL, "null context");
  int rc = check_env_decode(f, o);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard dev(c->device);
  if (!dev.ok) return fail(MOCHI_EHIP, "hipSetDevice(%d)", c->device);
  new_call(c);
  EncState& x = c->env_dec;
  x.ev_valid = false;
  if (!f->n_frames) return MOCHI_OK;
  hipStream_t st = (hipStream_t)stream;
  mochi::EnvDecArgs a;
  memset(&a, 0, sizeof a);
  a.v.in = *f;
  a.v.out = *o;
  if ((rc = x.events(c->profiling, mochi::kEnvDecEvents, &a.ev))) return rc;
  // no scratch, but the call still orders itself behind the context's last call on another stream
  HIP_TRY(c->order.acquire(st));
  HIP_TRY(mochi::launch_env_decode(a, st));
  x.ev_valid = a.ev != nullptr;
  HIP_TRY(c->order.release(st));
  return MOCHI_OK;
}

int mochi_envelope_route(uint32_t n, const uint8_t* status, const uint8_t* kind, const uint64_t* body_off,
                         const uint32_t* body_len, mochi_envelope_routed* o) {
  int rc = check_env_route(n, status, kind, body_off, body_len, o);
  if (rc) return rc;
  const mochi::env::RouteView v{n, status, kind, body_off, body_len, *o};
  const char* err = "";
  rc = mochi_host::envelope_route(&v, &err);
  return rc ? fail(rc, "mochi_envelope_route: %s", err) : MOCHI_OK;
}

int mochi_envelope_route_device(mochi_ctx* c, uint32_t n, const uint8_t* status, const uint8_t* kind,
                                const uint64_t* body_off, const uint32_t* body_len, mochi_envelope_routed* o, void* stream) {
  if (!c) return fail(MOCHI_EINVAL, "null context");
  int rc = check_env_route(n, status, kind, body_off, body_len, o);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard dev(c->device);
  if (!dev.ok) return fail(MOCHI_EHIP, "hipSetDevice(%d)", c->device);
  new_call(c);
  EncState& x = c->env_route;
  x.ev_valid = false;
  hipStream_t st = (hipStream_t)stream;
  if (!n) {
    HIP_TRY(hipMemsetAsync(o->kind_off, 0, 4 * (MOCHI_ENV_KINDS + 1), st));
    return MOCHI_OK;
  }
  mochi::EnvRouteArgs a;
  memset(&a, 0, sizeof a);
  a.v = mochi::env::RouteView{n, status, kind, body_off, body_len, *o};
  a.blocks = (n + 255) / 256;
  if ((rc = x.begin(a, mochi::env_route_layout, mochi::env_route_scan_n(a.blocks), 0, c->profiling, mochi::kEnvRouteEvents)))
    return rc;
  HIP_TRY(c->order.acquire(st));
  HIP_TRY(mochi::launch_env_route(a, st));
  x.ev_valid = a.ev != nullptr;
  HIP_TRY(c->order.release(st));
  return MOCHI_OK;
}

int mochi_envelope_join(const mochi_envelope_requests* r, const mochi_envelope_frames* f, const mochi_envelope_decoded* d,
                        mochi_envelope_joined* o, uint32_t* n_resps) {
  if (!n_resps) return fail(MOCHI_EINVAL, "n_resps required");
  *n_resps = 0;
  int rc = check_env_join(r, f, d, o);
  if (rc) return rc;
  const mochi::env::JoinView v{*r, *f, *d, *o};
  const char* err = "";
  rc = mochi_host::envelope_join(&v, n_resps, &err);
  return rc ? fail(rc, "mochi_envelope_join: %s", err) : MOCHI_OK;
}

int mochi_envelope_join_device(mochi_ctx* c, const mochi_envelope_requests* r, const mochi_envelope_frames* f,
                               const mochi_envelope_decoded* d, mochi_envelope_joined* o, uint32_t* n_resps_dev,
                               void* stream) {
  if (!c) return fail(MOCHI_EINVAL, "null context");
  if (!n_resps_dev) return fail(MOCHI_EINVAL, "n_resps_dev required");
  int rc = check_env_join(r, f, d, o);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard dev(c->device);
  if (!dev.ok) return fail(MOCHI_EHIP, "hipSetDevice(%d)", c->device);
  new_call(c);
  EncState& x = c->env_join;
  x.ev_valid = false;
  hipStream_t st = (hipStream_t)stream;
  mochi::EnvJoinArgs a;
  memset(&a, 0, sizeof a);
  a.v = mochi::env::JoinView{*r, *f, *d, *o};
  a.slots = mochi::env::join_slots(r->n_reqs);
  a.key_bits = mochi::env::join_key_bits(r->n_reqs);
  a.n_resps = n_resps_dev;
  if ((rc = x.begin(a, mochi::env_join_layout, 0, 0, c->profiling, mochi::kEnvJoinEvents))) return rc;
  if (f->n_frames) {
    size_t sort_bytes = 0;
    HIP_TRY(mochi::env_sort_temp_bytes(f->n_frames, a.key_bits, &sort_bytes));
    if ((rc = x.scan.ensure(sort_bytes))) return rc;
    a.scan_temp = x.scan.p;
    a.scan_temp_bytes = x.scan.cap;
  }
  HIP_TRY(c->order.acquire(st));
  HIP_TRY(mochi::launch_env_join(a, st));
  x.ev_valid = a.ev != nullptr;
  HIP_TRY(c->order.release(st));
  return MOCHI_OK;
}

uint64_t mochi_envelope_encode_bound(uint32_t n_msgs, uint64_t bodies_len, uint64_t ids_len) {
  // every body at bodies_len and every id at ids_len, five-byte length varints, a ten-byte
  // timestamp and a five-byte prefix throughout
  unsigned __int128 t = (unsigned __int128)n_msgs * ((unsigned __int128)bodies_len + 3 * (unsigned __int128)ids_len + 41);
  const unsigned __int128 cap = (unsigned __int128)n_msgs * (mochi::kEncMaxMsg + 5);  // longer messages are emitted empty
  if (t > cap) t = cap;
  return (uint64_t)t;
}

int mochi_envelope_encode(const mochi_envelope_source* s, uint8_t* wire, uint64_t wire_cap, uint64_t* msg_off,
                          uint32_t* msg_len, uint8_t* status, uint64_t* wire_len) {
  if (!wire_len) return fail(MOCHI_EINVAL, "wire_len required");
  *wire_len = 0;
  int rc = check_env_source(s, wire, wire_cap, msg_off, msg_len, status);
  if (rc || !s->n_msgs) return rc;
  const char* err = "";
  rc = mochi_host::envelope_encode(s, wire, wire_cap, msg_off, msg_len, status, wire_len, &err);
  return rc ? fail(rc, "mochi_envelope_encode: %s", err) : MOCHI_OK;
}

int mochi_envelope_encode_device(mochi_ctx* c, const mochi_envelope_source* s, uint8_t* wire, uint64_t wire_cap,
                                 uint64_t* msg_off, uint32_t* msg_len, uint8_t* status, uint64_t* wire_len,
                                 uint64_t* wire_len_dev, void* stream) {
  if (!c) return fail(MOCHI_EINVAL, "null context");
  if (!wire_len && !wire_len_dev) return fail(MOCHI_EINVAL, "wire_len or wire_len_dev required");
  int rc = check_env_source(s, wire, wire_cap, msg_off, msg_len, status);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard dev(c->device);
  if (!dev.ok) return fail(MOCHI_EHIP, "hipSetDevice(%d)", c->device);
  new_call(c);
  hipStream_t st = (hipStream_t)stream;
  const uint32_t M = s->n_msgs;
  EncState& x = c->env_enc;
  if (wire_len) *wire_len = 0;
  x.ev_valid = false;
  if (M == 0) {
    if (!wire_len) HIP_TRY(hipMemsetAsync(wire_len_dev, 0, 8, st));
    return MOCHI_OK;
  }
  mochi::EnvEncArgs a;
  memset(&a, 0, sizeof a);
  a.in = *s;
  a.wire = wire;
  a.wire_cap = wire_cap;
  a.msg_off = msg_off;
  a.msg_len = msg_len;
  a.status = status;
  if ((rc = x.begin(a, mochi::env_enc_layout, mochi::w2_small(M) ? 0 : M + 1, 8, c->profiling, mochi::kEnvEncEvents))) return rc;
  HIP_TRY(c->order.acquire(st));
  HIP_TRY(mochi::launch_env_size(a, st));
  bool fits = true;
  uint64_t need = 0;
  if (wire_len) {
    if ((rc = x.fetch_totals(a.off64 + M, 8, c->ev_tot, st))) return rc;
    *wire_len = need = *(const uint64_t*)x.tot.p;
    fits = need <= wire_cap;
  } else {
    HIP_TRY(hipMemcpyAsync(wire_len_dev, a.off64 + M, 8, hipMemcpyDeviceToDevice, st));
  }
  // k_env_hdr runs either way: it writes msg_off, and reads the total before it writes a byte of wire
  HIP_TRY(mochi::launch_env_emit(a, fits, st));
  x.ev_valid = a.ev && fits;
  HIP_TRY(c->order.release(st));
  return fits ? MOCHI_OK : capacity_error("wire_cap", wire_cap, "encoded size", need);
}

int mochi_ctx_read_envelope_profile(mochi_ctx* c, int which, float* kernel_ms, uint32_t n_kernels) {
  if (!c || !kernel_ms) return fail(MOCHI_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(c->mu);
  static const int kDec[mochi::kEnvDecStages][2] = {{0, 1}};
  static const int kRoute[mochi::kEnvRouteStages][2] = {{0, 1}, {1, 2}, {2, 3}};
  static const int kJoin[mochi::kEnvJoinStages][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 4}};
  static const int kEnc[mochi::kEnvEncStages][2] = {{0, 1}, {1, 2}, {3, 4}, {4, 5}};
  switch (which) {
    case MOCHI_ENV_PROF_DECODE:
      return c->env_dec.read_profile(kDec, mochi::kEnvDecStages, kernel_ms, n_kernels,
                                     "no envelope decode call was made while profiling was on");
    case MOCHI_ENV_PROF_ROUTE:
      return c->env_route.read_profile(kRoute, mochi::kEnvRouteStages, kernel_ms, n_kernels,
                                       "no envelope route call was made while profiling was on");
    case MOCHI_ENV_PROF_JOIN:
      return c->env_join.read_profile(kJoin, mochi::kEnvJoinStages, kernel_ms, n_kernels,
                                      "no envelope join call was made while profiling was on");
    case MOCHI_ENV_PROF_ENCODE:
      return c->env_enc.read_profile(kEnc, mochi::kEnvEncStages, kernel_ms, n_kernels,
                                     "no envelope encode call was made while profiling was on");
  }
  return fail(MOCHI_EINVAL, "which is no MOCHI_ENV_PROF_*");
}

}  // extern "C"
