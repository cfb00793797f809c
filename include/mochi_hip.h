/*
 * mochi_hip.h — C ABI of libmochi_hip, the MI355X batch verifier for MochiDB's
 * Write2 certificate path.
 *
 * What this replaces in the reference (tomisetsu/mochi-db, Java):
 *
 *   InMemoryDataStore.processWrite2ToServer(Write2ToServer)           InMemoryDataStore.java:641-666
 *     ├ processMultiGrantsFromAllServers(wc.grantsMap, txn)           InMemoryDataStore.java:613-640
 *     └ write2apply(coalesced, msg)  (verdict part only)              InMemoryDataStore.java:576-611
 *   ClusterConfiguration.getServerMajority()                          ClusterConfiguration.java:264-267
 *   MochiDBClient Write2/Read response aggregation                    MochiDBClient.java:148-175, 355-382
 *
 * plus the per-grant signature check the reference leaves as a TODO
 * (MochiProtocol.proto:123 "// TODO: add signature"): SHA-256 over the
 * proto3-encoded Grant (MochiProtocol.java:7556-7574) and an RSA-2048
 * PKCS#1 v1.5 verify (JCA "SHA256withRSA", e = 65537).
 *
 * ABI rules: plain C, plain pointers and sizes, no torch / HIP types in the
 * signatures (a hipStream_t travels as void*).  Every entry point returns an
 * int status: 0 = ok, < 0 = argument / HIP error (text in mochi_last_error()).
 * A verdict is NEVER an error: rejects are bits and reason codes in the
 * output buffers (the reference throws, and RequestHandlerDispatcher.java:74-79
 * swallows, so a reject is observable only as a missing Write2Ans; the Java
 * shim in INTEGRATION.md maps reason codes back to those exception types).
 */
#ifndef MOCHI_HIP_H
#define MOCHI_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOCHI_ABI_VERSION 3
#define MOCHI_RSA_BYTES 256     /* RSA-2048 modulus / signature size            */
#define MOCHI_RSA_E 65537u      /* the only public exponent supported          */
#define MOCHI_TXN_HASH_BYTES 128 /* lowercase-hex SHA-512 (Utils.java:135-153)  */
#define MOCHI_MAX_KEYS 4096     /* key-table entries per context               */
#define MOCHI_MAX_OPS_PER_CERT 64 /* transaction operations per certificate    */

/* Status codes. */
#define MOCHI_OK 0
#define MOCHI_EINVAL (-1)  /* bad argument / inconsistent batch          */
#define MOCHI_EHIP (-2)    /* HIP runtime error                          */
#define MOCHI_ENOMEM (-3)  /* device or pinned-host allocation failed    */
#define MOCHI_ENODEV (-4)  /* no usable gfx950 device                    */

/* Per-certificate verdict reason codes.  Each maps to the exception the
 * reference throws on that branch (see INTEGRATION.md for the Java mapping). */
enum mochi_reason {
  MOCHI_ACCEPT = 0,
  /* processMultiGrantsFromAllServers: a valid grant's timestamp differs from the
   * first valid grant seen for the same key -> UnsupportedOperationException
   * (InMemoryDataStore.java:626-628). */
  MOCHI_REJECT_TS_MISMATCH = 1,
  /* write2apply: no valid grant for a local op's key -> coalescedTxnGrantMap.get()
   * returns null -> NullPointerException (InMemoryDataStore.java:588). */
  MOCHI_REJECT_NO_GRANT = 2,
  /* write2apply: list.size() > getServerMajority() fails -> IllegalStateException
   * via Utils.assertTrue (InMemoryDataStore.java:590, Utils.java:43-47).  With
   * strict_gt = 0 the client predicate ">=" (MochiDBClient.java:172,379) is used. */
  MOCHI_REJECT_BELOW_QUORUM = 3,
  /* write2apply: g0.transactionHash != objectSHA512(txn) ->
   * UnsupportedOperationException (InMemoryDataStore.java:591,605-607). */
  MOCHI_REJECT_HASH_MISMATCH = 4,
  /* write2apply: no StoreValueObjectContainer for the key -> NullPointerException
   * (InMemoryDataStore.java:592-593).  Driven by MOCHI_OP_HAS_SVOC. */
  MOCHI_REJECT_NO_SVOC = 5,
  /* a grant's bytes are not a parseable proto3 Grant (the reference would fail
   * in the Netty protobuf decoder, MochiServerInitializer.java:30-34). */
  MOCHI_REJECT_MALFORMED = 6,
  /* Write2 wire path only: the message is legal protobuf but outside the
   * device decoder's fast path (enum mochi_msg_status MOCHI_MSG_FALLBACK /
   * MOCHI_MSG_OPS_MISMATCH) and the library's host decoder could not decide it
   * either (more than MOCHI_MAX_OPS_PER_CERT operations, or op_flags_off giving a
   * different operation count).  Never accepted. */
  MOCHI_UNDECIDED = 7,
  /* applyOperation: setCurrentC(wc) then getCurrentTimestampFromCurrentCertificate()
   * on the INCOMING certificate (InMemoryDataStore.java:533-534) throws
   * IllegalStateException: some MultiGrant of the certificate has no grant for the
   * op's key (StoreValueObjectContainer.java:186, Utils.assertNotNull) or two of
   * them carry different timestamps (:192-194).  Every MultiGrant counts here,
   * whatever its signatures (the Java loop runs over the stored certificate as
   * received).  Side effect in the reference: currentC is already replaced. */
  MOCHI_REJECT_APPLY_STATE = 8,
  /* write2apply :594: the key's STORED currentC throws in
   * getCurrentTimestampFromCurrentCertificate (op flag MOCHI_OP_CURRENT_C_BAD) ->
   * IllegalStateException. */
  MOCHI_REJECT_STORED_CERT = 9,
  /* readOperation / applyOperation on an op that is not a WRITE/DELETE, or whose
   * key holds no write lock (empty operand1 is never locked,
   * InMemoryDataStore.java:339-358): IllegalStateException (:525-526 / :560-561)
   * or UnsupportedOperationException (:551 / :572).  Op flag MOCHI_OP_NOT_WRITE. */
  MOCHI_REJECT_NOT_WRITE = 10,
};

/* Per-operation outcome of write2apply's loop (InMemoryDataStore.java:581-609),
 * mochi_verdicts.op_decision.  The reference is not atomic: the ops before a
 * failing op have already been applied when it throws. */
enum mochi_op_decision {
  MOCHI_OPD_SKIPPED = 0,     /* not reached (the certificate was rejected earlier)        */
  MOCHI_OPD_APPLY = 1,       /* applyOperation(op, wc) (:597): currentC := wc, ts = op_ts  */
  MOCHI_OPD_READ = 2,        /* readOperation(op) (:596): objectTS > g0.timestamp          */
  MOCHI_OPD_WRONG_SHARD = 3, /* WRONG_SHARD result (:582-587)                              */
  MOCHI_OPD_FAILED = 4,      /* this op's step threw: cert_reason / cert_fail_op          */
};

/* op_flags bits (one byte per transaction operation). */
#define MOCHI_OP_LOCAL 0x01    /* objectBelongsToCurrentShardServer(key)      InMemoryDataStore.java:63-72,582 */
#define MOCHI_OP_HAS_SVOC 0x02 /* getDataMap(key).get(key) != null           InMemoryDataStore.java:592 */
#define MOCHI_OP_HAS_CURRENT_C 0x04 /* the SVOC holds a certificate (currentC != null); its timestamp,
                                       getCurrentTimestampFromCurrentCertificate(), is op_object_ts[o]
                                       (StoreValueObjectContainer.java:175-198, InMemoryDataStore.java:594) */
#define MOCHI_OP_CURRENT_C_BAD 0x08 /* the SVOC's stored currentC makes that call throw (:594)    */
#define MOCHI_OP_NOT_WRITE 0x10     /* action is not WRITE/DELETE, or operand1 is empty (no write
                                       lock): the read/apply step throws.  The wire decoder sets it
                                       itself from Operation.action / operand1. */

/* grant_flags bits (one byte per grant, output). */
#define MOCHI_GRANT_SIG_OK 0x01   /* RSA/SHA-256 signature verified            */
#define MOCHI_GRANT_PARSED 0x02   /* bytes parsed as a Grant                   */

/*
 * A batch of Write2 certificates in struct-of-arrays form.
 *
 * Grants are listed certificate by certificate, in certificate WIRE order
 * (the MultiGrant map iteration order, which decides which grant is "g0",
 * InMemoryDataStore.java:588, MochiDBClient.java:333-338).  A grant's bytes
 * are the exact proto3 encoding that was signed (Grant.toByteArray(),
 * MochiProtocol.java:7556-7574) and may sit anywhere in `grant_bytes`
 * (e.g. as slices of the received Write2ToServer wire buffer: zero copy).
 *
 * All arrays are host pointers for mochi_verify_batch() and device pointers
 * for mochi_verify_batch_device().
 */
typedef struct mochi_batch {
  uint32_t n_grants;              /* N */
  uint32_t n_certs;               /* C */
  uint32_t n_ops;                 /* O = total transaction operations over all certificates */
  uint32_t n_mgs;                 /* total MultiGrants (size of mg_grant_off - 1); 0 with cert_mg_off NULL */
  uint64_t grant_bytes_len;       /* size of grant_bytes                                      */
  const uint8_t* grant_bytes;     /* blob holding every grant's proto3 bytes                  */
  const uint64_t* grant_off;      /* [N] byte offset of grant i in grant_bytes                */
  const uint32_t* grant_len;      /* [N] byte length of grant i (<= 65536)                    */
  const uint8_t* sig;             /* [N * 256] big-endian RSA signatures                      */
  const uint16_t* signer;         /* [N] key-table index of the signing server (MultiGrant.serverId) */
  const uint8_t* grant_key;       /* [N] key slot of the op key this grant is for (< ops in cert) */
  const uint32_t* cert_grant_off; /* [C+1] CSR: grants of cert c are [off[c], off[c+1])        */
  const uint32_t* cert_op_off;    /* [C+1] CSR: ops of cert c are [off[c], off[c+1])           */
  const uint8_t* op_key;          /* [O] key slot of each op (ops on the same key share a slot) */
  const uint8_t* op_flags;        /* [O] MOCHI_OP_* bits                                        */
  const uint8_t* expected_hash;   /* [C * 128] objectSHA512(txn) as lowercase hex (host-computed, §7.1.4) */
  /* --- ABI 2 --- */
  /* MultiGrant boundaries (the certificate map's values, wire order): the
   * MultiGrants of cert c are [cert_mg_off[c], cert_mg_off[c+1]) and the grants of
   * MultiGrant m are [mg_grant_off[m], mg_grant_off[m+1]) (empty MultiGrants
   * allowed); mg_grant_off[cert_mg_off[c]] == cert_grant_off[c].  NULL: every
   * maximal run of consecutive grants with one signer is one MultiGrant. */
  const uint32_t* cert_mg_off;    /* [C+1] or NULL                                              */
  const uint32_t* mg_grant_off;   /* [n_mgs+1] or NULL                                          */
  const int64_t* op_object_ts;    /* [O] stored currentC timestamp, read iff MOCHI_OP_HAS_CURRENT_C; NULL = none */
  /* The op key (Operation.operand1) bytes, as a slice of grant_bytes: needed only
   * by MOCHI_Q_BIND (Grant.objectId must equal it).  NULL otherwise. */
  const uint64_t* op_key_off;     /* [O] offset in grant_bytes                                  */
  const uint32_t* op_key_len;     /* [O]                                                        */
} mochi_batch;

/* mochi_params.quorum_mode bits.  0 = parity with the reference: every
 * signature-valid grant of the certificate counts once per op naming its key
 * (InMemoryDataStore.java:613-640, :590), whoever signed it.  The bits make the
 * new signature layer a Byzantine quorum; a grant they exclude is treated like
 * one with an invalid signature (absent, :622-624). */
#define MOCHI_Q_DISTINCT_SIGNERS 0x1 /* a signer counts at most once per key: only its first valid
                                        grant for the key (wire order) counts.  The honest client keys
                                        the certificate by MultiGrant.serverId (MochiDBClient.java:299,
                                        334), so honest certificates are unaffected. */
#define MOCHI_Q_BIND 0x2             /* a grant counts only if Grant.objectId equals the op key it is
                                        filed under and Grant.transactionHash equals expected_hash
                                        (no replay of a signer's grants for other objects or
                                        transactions).  Needs op_key_off / op_key_len. */

typedef struct mochi_params {
  uint32_t replication_factor; /* R = _CONFIG_BFT_REPLICATION; majority M = 2*(R/3)+1 */
  uint32_t strict_gt;          /* 1: server predicate count > M (InMemoryDataStore.java:590)
                                  0: client predicate count >= M (MochiDBClient.java:172,379) */
  uint32_t quorum_mode;        /* MOCHI_Q_* bits, 0 = reference parity */
  uint32_t _pad;
} mochi_params;

typedef struct mochi_verdicts {
  uint32_t* grant_valid_bits; /* [ceil(N/32)] bit i = grant i signature valid  (may be NULL) */
  uint8_t* grant_flags;       /* [N] MOCHI_GRANT_* bits                          (may be NULL) */
  int64_t* grant_ts;          /* [N] parsed Grant.timestamp                      (may be NULL) */
  uint32_t* cert_accept_bits; /* [ceil(C/32)] bit c = certificate accepted       (required)    */
  uint8_t* cert_reason;       /* [C] enum mochi_reason                           (may be NULL) */
  uint8_t* cert_fail_op;      /* [C] op index of the first failing op, 0xFF if none / n.a. (may be NULL) */
  /* --- ABI 2: per operation, in the batch's op order (may be NULL) --- */
  uint8_t* op_decision;       /* [O] enum mochi_op_decision                                     */
  uint32_t* op_g0;            /* [O] g0 of the op's key: certificate-relative index of the first
                                 counted grant for it (InMemoryDataStore.java:588), 0xFFFFFFFF none */
  int64_t* op_ts;             /* [O] g0's timestamp (the ts applyOperation records), 0 if none   */
} mochi_verdicts;

typedef struct mochi_ctx mochi_ctx;

/* ABI version of the loaded library (== MOCHI_ABI_VERSION). */
int mochi_abi_version(void);

/* Thread-local text of the last error returned on this thread. */
const char* mochi_last_error(void);

/* Number of visible HIP devices (0 when none). */
int mochi_device_count(void);

/*
 * Create a verifier on HIP device `device` with a key table of `n_keys`
 * RSA public keys.  `moduli_be` holds n_keys * key_bytes big-endian moduli
 * (key_bytes must be 256; every modulus exactly 2048 bits and odd);
 * `public_exponent` must be 65537.  Key index = MultiGrant.serverId's position
 * in the table.  Montgomery constants (n0', R^2 mod n) are derived here and
 * the table is uploaded once.  Returns NULL on error (see mochi_last_error()).
 */
mochi_ctx* mochi_ctx_create(int device, const uint8_t* moduli_be, uint32_t n_keys, uint32_t key_bytes,
                            uint32_t public_exponent);
/* Never blocks.  With no batcher holding the context it is freed now; while a
 * batcher built on it is alive (or a batcher destroyed from its own callback is
 * not yet freed by its last flusher) the context is freed by that batcher's
 * release instead.  Either way the handle must not be used after the call. */
void mochi_ctx_destroy(mochi_ctx* ctx);

/*
 * Verify a batch held in HOST memory.  The batch is cut into chunks of whole
 * certificates (~256k grants, env MOCHI_CHUNK_GRANTS); chunk j+1's upload
 * (hipMemcpyAsync on a copy stream; pageable arrays staged through pinned
 * buffers, pinned ones DMA'd in place) overlaps chunk j's kernels (grant prep
 * + RSA verify + certificate tally) and chunk j-1's verdict download.
 * Synchronous.  Thread-safe per context (calls on one context serialize).
 */
int mochi_verify_batch(mochi_ctx* ctx, const mochi_batch* batch, const mochi_params* params,
                       mochi_verdicts* out);

/*
 * Verify a batch already resident in DEVICE memory (every mochi_batch pointer
 * and every non-NULL mochi_verdicts pointer is a device pointer).  Enqueued on
 * `stream` (a hipStream_t; NULL = the null stream, as in every HIP API); asynchronous.  The
 * batch header itself is read on the host.  Scratch is owned by the context.
 */
int mochi_verify_batch_device(mochi_ctx* ctx, const mochi_batch* batch, const mochi_params* params,
                              mochi_verdicts* out, void* stream);

/*
 * The raw RSA public operation y = s^65537 mod n for n signatures (big-endian,
 * 256 bytes each) under key `signer[i]`, on the device, through the same
 * bucketing and squaring-chain kernels as the verify path, then k_rsa_raw.
 * The call follows the context's small-batch setting as the verify calls do
 * (mochi_ctx_set_small_batch): up to that many signatures run k_bucket_small
 * + k_rsa_pow_lat, more run the bucket kernels + k_rsa_pow.  out_be: n * 256
 * bytes.  out_z (optional, n * 74 words): the squaring-chain intermediate
 * z = s^(2^16) mod n in radix-2^28 limbs, not fully reduced (< 2^2064), for
 * tests.  Host memory, synchronous.
 */
int mochi_rsa_public_op(mochi_ctx* ctx, uint32_t n, const uint8_t* sig_be, const uint16_t* signer, uint8_t* out_be,
                        uint32_t* out_z);

/*
 * The k_rsa_pow fold matrix of one RSA-2048 modulus (inspection / tests; the
 * context builds one per key).  img: 102,400 int8 = the MFMA A fragments of
 * R_{j,b} = 2^(28(73+j)+8b) mod n in balanced mixed-radix digits (layout:
 * mochi-db_amd/csrc/fold.h); cadd: the int8 bias correction 128 * sum R_{j,b}
 * as 74 limbs of 28 bits.  Host memory.
 */
int mochi_fold_matrix(const uint8_t* modulus_be, int8_t* img, uint32_t* cadd);

/*
 * Per-stage device timing.  While profiling is on, every verify call records a
 * (start, end) hipEvent pair around each stage on the stream the stage runs
 * on; mochi_ctx_read_profile waits for them and returns the SUM over calls
 * since the last read, per stage: [0] grant prep (parse + SHA-256; it runs on
 * the context's aux stream, concurrently with [1] and [2]), [1] signer
 * bucketing, [2] k_rsa_pow, [3] k_rsa_final (+ bitmap pack), [4] k_tally.
 * n_stages <= 5.
 */
int mochi_ctx_set_profiling(mochi_ctx* ctx, int on);
int mochi_ctx_read_profile(mochi_ctx* ctx, float* stage_ms, uint32_t n_stages, uint32_t* n_calls);

/* Stream-event timings of the last mochi_verify_batch() call on this context
 * (milliseconds).  The host path is a chunked pipeline (uploads, kernels and
 * downloads of consecutive chunks overlap), so: h2d_ms = the first chunk's
 * upload (nothing else runs yet), kernels_ms = first kernel start -> last
 * kernel end, d2h_ms = the last chunk's download; mochi_ctx_last_total_ms
 * gives first upload start -> last download end. */
int mochi_ctx_last_timing(mochi_ctx* ctx, float* h2d_ms, float* kernels_ms, float* d2h_ms);
int mochi_ctx_last_total_ms(mochi_ctx* ctx, float* total_ms);

/* Host-path chunk size target in grants (0 = default: env MOCHI_CHUNK_GRANTS
 * or 262144).  Chunks always hold whole certificates, 32 at a time. */
int mochi_ctx_set_chunk_grants(mochi_ctx* ctx, uint32_t grants);

/* Small-batch launch sequence (a batcher flush of a few messages): a batch of
 * at most `grants` grants is bucketed by one kernel and prepped grant by grant
 * on the launch stream, instead of the large-batch sequence (three bucketing
 * kernels, the certificate-level grant dedup forked beside k_rsa_pow).  Same
 * outputs either way.  Default 4096; 0 = always the large-batch sequence. */
int mochi_ctx_set_small_batch(mochi_ctx* ctx, uint32_t grants);

/*
 * Pinned (page-locked) host memory for building batches in place: arrays of a
 * mochi_batch that live in such memory are DMA'd straight to the device by
 * mochi_verify_batch (no staging copy).  NULL on failure.
 */
void* mochi_host_alloc(uint64_t bytes);
void mochi_host_free(void* ptr);

/*
 * Producer side (the Write1 signing site the reference leaves as a TODO:
 * InMemoryDataStore.java:283-295, MochiProtocol.proto:123): sign SHA-256 of
 * each grant's bytes with an RSA-2048 private key (PEM, PKCS#1 v1.5,
 * "SHA256withRSA"), CPU / OpenSSL, `n_threads` threads.  sig_out: n * 256.
 */
int mochi_sign_grants(const char* pem_private_key, uint32_t n, const uint8_t* grant_bytes, const uint64_t* grant_off,
                      const uint32_t* grant_len, uint8_t* sig_out, int n_threads);

/* Big-endian modulus of a PEM RSA key (private or public) -> n_be_out[256]. */
int mochi_pem_modulus(const char* pem_key, uint8_t* n_be_out);

/*
 * Client-side response aggregation (MochiDBClient.java:148-175 reads,
 * 355-382 Write2): for each request r, responses [resp_off[r], resp_off[r+1])
 * each carry n_ops[r] op statuses (1 byte each, OperationResultStatus: 0 = OK,
 * 1 = WRONG_SHARD) at status + status_off[resp]; resp_n_ops[resp] is the op
 * count that response actually returned.  Request r is accepted iff every
 * response returned n_ops[r] results and, for every op, the number of
 * non-WRONG_SHARD results is >= M = 2*(R/3)+1.  chosen[status_off-aligned]
 * receives, per (request, op), the index of the LAST non-WRONG_SHARD response
 * (MochiDBClient.java:166,373) or -1.  reason[r]: 0 accept, 1 op-count
 * mismatch (InconsistentRead/WriteException at :159-161 / :366-368), 2 below
 * majority (:171-175 / :378-381).  Host memory; pure CPU.
 *
 * Arguments (host and device form alike): an argument nobody reads is not
 * required.  chosen and reason are optional outputs (NULL = not wanted);
 * chosen_off is read only when chosen is given and may be NULL otherwise.
 * With n_requests == 0 every pointer may be NULL and nothing is written.
 * Every other pointer must be non-NULL (MOCHI_EINVAL).  chosen_off and
 * status_off need not be ascending or dense, and responses may share a
 * status slice.  Every word of accept_bits[ceil(n_requests/32)] is written,
 * the bits past n_requests in the last word as 0; for every request all
 * n_ops[r] entries of chosen are written whatever the reason, and nothing
 * else is.
 */
int mochi_tally_responses(uint32_t n_requests, const uint32_t* resp_off, const uint32_t* n_ops,
                          const uint32_t* resp_n_ops, const uint64_t* status_off, const uint8_t* status,
                          const uint64_t* chosen_off, uint32_t replication_factor, int32_t* chosen,
                          uint8_t* reason, uint32_t* accept_bits);

/* The same aggregation on the device, batched across in-flight transactions
 * (every pointer a device pointer; asynchronous on `stream`, a hipStream_t).
 * Lane = request.  accept_bits must hold ceil(n_requests/32) words. */
int mochi_tally_responses_device(uint32_t n_requests, const uint32_t* resp_off, const uint32_t* n_ops,
                                 const uint32_t* resp_n_ops, const uint64_t* status_off, const uint8_t* status,
                                 const uint64_t* chosen_off, uint32_t replication_factor, int32_t* chosen,
                                 uint8_t* reason, uint32_t* accept_bits, void* stream);

/* Write1 response kinds: the ProtocolMessage payload case a Write1ToServer got
 * back (MochiDBClient.java:274-289). */
#define MOCHI_W1_OK 0             /* WRITE1OKFROMSERVER                        */
#define MOCHI_W1_REFUSED 1        /* WRITE1REFUSEDFROMSERVER                   */
#define MOCHI_W1_REQUEST_FAILED 2 /* REQUESTFAILEDFROMSERVER                   */
#define MOCHI_W1_OTHER 3          /* any other payload                         */

/* Write1 round outcomes (MochiDBClient.executeWriteTransactionBL). */
enum mochi_write1_decision {
  MOCHI_W1_PROCEED = 0,           /* every response OK, timestamps uniform -> Write2 (:320-324)      */
  MOCHI_W1_RETRY = 1,             /* OK multigrants disagree on a key's timestamp -> sleep 1 ms and
                                     resend Write1 (isUniformTimeStampInMultiGrants, :195-219, :310-318) */
  MOCHI_W1_THROW_REFUSED = 2,     /* RequestRefusedException (:325-328)                              */
  MOCHI_W1_THROW_FAILED = 3,      /* RequestFailedException (:281-283)                               */
  MOCHI_W1_THROW_UNSUPPORTED = 4, /* a WRONG_SHARD grant in an OK/REFUSED multigrant:
                                     removeWrongShardGrantFromMultiGrant removes from protobuf's
                                     read-only map view -> UnsupportedOperationException (:221-228) */
};

/*
 * Client Write1 round classification (a8 + a9), batched over requests.
 * Request r owns responses [resp_off[r], resp_off[r+1]) in arrival order;
 * response q has payload kind resp_kind[q] (MOCHI_W1_*), the replying
 * MultiGrant.serverId as a small integer resp_server[q], and grants
 * [resp_grant_off[q], resp_grant_off[q+1]) (CSR over all responses).  Grant g:
 * grant_key[g] = slot of its objectId among the transaction's op keys (0xFF if
 * it is no op's key), grant_ts[g] = Grant.timestamp, grant_status[g] =
 * OperationResultStatus (0 OK, 1 WRONG_SHARD).  decision[r] receives an enum
 * mochi_write1_decision.  Host memory; pure CPU.
 */
int mochi_write1_classify(uint32_t n_requests, const uint32_t* resp_off, const uint8_t* resp_kind,
                          const uint32_t* resp_server, const uint32_t* resp_grant_off, const uint8_t* grant_key,
                          const int64_t* grant_ts, const uint8_t* grant_status, uint8_t* decision);
/* The Write1 classification on the device (device pointers, async on `stream`).
 *
 * Arguments (host and device form alike): with n_requests == 0 every pointer
 * may be NULL and nothing is written; otherwise resp_off, resp_kind,
 * resp_server, resp_grant_off and decision must be non-NULL (MOCHI_EINVAL).
 * grant_key / grant_ts / grant_status are read only where a response has
 * grants and may be NULL when none has.  The host form checks that
 * (MOCHI_EINVAL for NULL grant arrays when resp_grant_off spans a grant); the
 * device form cannot validate the grant arrays against resp_grant_off, which
 * lives in device memory: passing NULL grant arrays with a resp_grant_off that
 * spans grants is undefined there. */
int mochi_write1_classify_device(uint32_t n_requests, const uint32_t* resp_off, const uint8_t* resp_kind,
                                 const uint32_t* resp_server, const uint32_t* resp_grant_off, const uint8_t* grant_key,
                                 const int64_t* grant_ts, const uint8_t* grant_status, uint8_t* decision,
                                 void* stream);

/* ------------------------------------------------------------------------
 * Write2ToServer wire path: the device decodes the received protobuf bytes.
 *
 * Replaces the SoA assembly a caller of mochi_verify_batch has to do: it takes
 * the Write2ToServer message bodies exactly as they arrived
 * (MochiProtocol.proto:144-147, field 110 of a
 * ProtocolMessage), decodes them on the device with protobuf-java 3.16.3
 * semantics (map fields keep first-insertion order with last-value-wins,
 * unknown fields skipped, proto3 strings UTF-8 checked, any malformation fails
 * the whole message) and verifies them.  Grant bytes are verified in place
 * (zero copy); each grant's signature is MultiGrant.grantSignatures[objectId]
 * (the field INTEGRATION.md adds as MochiProtocol.proto:123's TODO) and its
 * signer is the key whose server id (mochi_ctx_set_server_ids) equals
 * MultiGrant.serverId.
 * ------------------------------------------------------------------------ */

/* Per-message decode status. */
enum mochi_msg_status {
  MOCHI_MSG_OK = 0,
  /* not a parseable Write2ToServer: protobuf-java's parser would throw
   * InvalidProtocolBufferException in the Netty decoder
   * (MochiServerInitializer.java:30-34) -> reason MOCHI_REJECT_MALFORMED */
  MOCHI_MSG_MALFORMED = 1,
  /* legal, but outside the device decoder's fast path -> reason
   * MOCHI_UNDECIDED: writeCertificate or transaction given more than once; a
   * map entry whose MultiGrant or Grant value is given more than once; a Grant
   * whose bytes are not the canonical encoding Grant.toByteArray() would give
   * (MochiProtocol.java:7556-7574); more than 32 certificate entries, or 64
   * grants or 64 grantSignatures entries in a decoded MultiGrant (counted on the
   * wire, repeated keys included), or more than 64 operations */
  MOCHI_MSG_FALLBACK = 2,
  /* op_flags_off gives a different operation count than the message holds */
  MOCHI_MSG_OPS_MISMATCH = 3,
};

typedef struct mochi_write2_batch {
  uint32_t n_msgs; /* M */
  uint32_t _pad0;
  uint64_t wire_len;              /* size of wire                                             */
  const uint8_t* wire;            /* blob holding every Write2ToServer body                    */
  const uint64_t* msg_off;        /* [M] byte offset of message m in wire                      */
  const uint32_t* msg_len;        /* [M] byte length of message m                              */
  const uint32_t* op_flags_off;   /* [M+1] CSR into op_flags; NULL = every op LOCAL|HAS_SVOC    */
  const uint8_t* op_flags;        /* MOCHI_OP_* per operation, transaction order               */
  const uint8_t* expected_hash;   /* [M * 128] objectSHA512(transaction), lowercase hex         */
  /* --- ABI 2 --- */
  const int64_t* op_object_ts;    /* aligned with op_flags (CSR op_flags_off): stored currentC
                                     timestamp, read iff MOCHI_OP_HAS_CURRENT_C; NULL = none      */
} mochi_write2_batch;

/* Server-id table of the context: key i of the key table belongs to the server
 * whose MultiGrant.serverId is ids[id_off[i], id_off[i+1]).  n_ids must equal
 * the context's key count; ids <= 256 bytes each. */
int mochi_ctx_set_server_ids(mochi_ctx* ctx, const uint8_t* ids, const uint32_t* id_off, uint32_t n_ids);

/* Decode + verify M Write2ToServer messages held in HOST memory.  Only the
 * certificate-level and per-op verdict arrays of `out` are written (grant-level
 * pointers must be NULL); per-op arrays need op_flags_off and follow its layout
 * (ops of messages that were not decoded read MOCHI_OPD_SKIPPED).
 * msg_status[M] receives enum mochi_msg_status.  Messages the device decoder
 * leaves to the host (MOCHI_MSG_FALLBACK: repeated / merged fields, non-canonical
 * Grant bytes, more than 32 MultiGrants or 64 grants per MultiGrant) are decoded
 * by the library's host decoder with full protobuf-java semantics and verified
 * on the device like any other certificate -- signatures are always checked;
 * msg_status still reports MOCHI_MSG_FALLBACK for them.  Synchronous; batches
 * larger than the chunk target are pipelined (upload / decode+verify / download
 * of consecutive chunks overlap). */
int mochi_verify_write2(mochi_ctx* ctx, const mochi_write2_batch* batch, const mochi_params* params,
                        mochi_verdicts* out, uint8_t* msg_status);

/* Same with every pointer of `batch`, `out` and msg_status in DEVICE memory,
 * enqueued on `stream` (hipStream_t; NULL = null stream).  The decoded batch
 * is sized on the device; the call waits for its grant / op totals. */
int mochi_verify_write2_device(mochi_ctx* ctx, const mochi_write2_batch* batch, const mochi_params* params,
                               mochi_verdicts* out, uint8_t* msg_status, void* stream);

/* The device decoder's output for M messages in HOST memory (inspection and
 * tests; mochi_verify_write2 never copies it back).  Arrays are allocated by
 * the library; release them with mochi_write2_decoded_free.  grant_off is
 * relative to the start of `wire`. */
typedef struct mochi_write2_decoded {
  uint32_t n_msgs, n_grants, n_ops, n_mgs;
  uint64_t* grant_off;      /* [N] */
  uint32_t* grant_len;      /* [N] */
  uint8_t* sig;             /* [N * 256] */
  uint16_t* signer;         /* [N] key index, 0xFFFF = unknown serverId */
  uint8_t* grant_key;       /* [N] op key slot, 0xFF = no op names it */
  uint32_t* cert_grant_off; /* [M+1] */
  uint32_t* cert_op_off;    /* [M+1] */
  uint8_t* op_key;          /* [O] */
  uint8_t* op_flags;        /* [O] */
  uint8_t* msg_status;      /* [M] enum mochi_msg_status */
  /* ABI 2 */
  uint32_t* cert_mg_off;    /* [M+1] MultiGrants per message (CSR) */
  uint32_t* mg_grant_off;   /* [n_mgs+1] grants per MultiGrant (CSR) */
  uint64_t* op_key_off;     /* [O] Operation.operand1, offset relative to `wire` */
  uint32_t* op_key_len;     /* [O] */
} mochi_write2_decoded;
int mochi_write2_decode(mochi_ctx* ctx, const mochi_write2_batch* batch, mochi_write2_decoded* out);
void mochi_write2_decoded_free(mochi_write2_decoded* d);

/* mochi_write2_decode, and with it the decoder's first-grant hint (additive; inspection
 * and tests: the verify path hands the hint to grant prep and never copies it back).
 * *grant_same receives [n_grants] indices into the decoded grants of the whole batch,
 * allocated by the library (release with mochi_write2_same_free; NULL on failure):
 * grant_same[g] is g itself, or the first decoded grant of g's message -- then that
 * grant lies before g and its bytes are g's, byte for byte.  A NULL grant_same makes
 * the call mochi_write2_decode. */
int mochi_write2_decode_same(mochi_ctx* ctx, const mochi_write2_batch* batch, mochi_write2_decoded* out,
                             uint32_t** grant_same);
void mochi_write2_same_free(uint32_t* grant_same);

/* ------------------------------------------------------------------------
 * Write2ToServer ENCODE: the inverse of the decoder above, the client's
 * certificate assembly (MochiDBClient.java:333-338).  An SoA batch of the
 * MultiGrants a client collected becomes the Write2ToServer bodies, one blob
 * with msg_off / msg_len, laid out as mochi_write2_batch takes them, byte for
 * byte what protobuf-java writes (MochiProtocol.proto:107-147): fields in
 * number order, every map entry with its key and its value, proto3 defaults
 * omitted, MultiGrant.hash never written.  The key of a grants-map entry and of
 * its grantSignatures entry is the grant's objectId, read from the grant's own
 * bytes; grant bytes are copied as given.  The caller lists MultiGrants and
 * grants in the order it wants on the wire.
 * ------------------------------------------------------------------------ */
typedef struct mochi_write2_source {
  uint32_t n_msgs, n_mgs, n_grants, n_ops;
  const uint8_t*  grant_bytes;  uint64_t grant_bytes_len;
  const uint64_t* grant_off;    /* [N] any alignment                              */
  const uint32_t* grant_len;    /* [N]                                            */
  const uint8_t*  sig;          /* [N*256] or NULL = no grantSignatures entries   */
  const uint32_t* cert_mg_off;  /* [M+1]  MultiGrants per message, wire order     */
  const uint32_t* mg_grant_off; /* [n_mgs+1] grants per MultiGrant, map order     */
  const uint16_t* mg_signer;    /* [n_mgs] key index: MultiGrant.serverId AND the
                                   certificate map key = that key's server id     */
  const uint8_t*  strings;      uint64_t strings_len;  /* operands and client ids */
  const uint32_t* cert_op_off;  /* [M+1] */
  const uint8_t*  op_action;    /* [O] OperationAction value (0 omitted)          */
  const uint64_t* op1_off; const uint32_t* op1_len;   /* [O] operand1 (0 = omitted) */
  const uint64_t* op2_off; const uint32_t* op2_len;   /* [O] or both NULL          */
  const uint64_t* client_off; const uint32_t* client_len; /* [M] MultiGrant.clientId of
                                   every MultiGrant of message m; both NULL = empty */
} mochi_write2_source;

/* Per-message encode status.  A message with a status other than OK is emitted
 * with length 0; the call still succeeds.  With several causes the lowest
 * value is reported. */
enum mochi_enc_status {
  MOCHI_ENC_OK = 0,
  MOCHI_ENC_BAD_GRANT = 1,  /* a grant does not parse (or lies outside grant_bytes) */
  MOCHI_ENC_BAD_SIGNER = 2, /* an mg_signer outside the id table                    */
  MOCHI_ENC_TOO_LONG = 3,   /* the message would be 2^31 bytes or more              */
  MOCHI_ENC_BAD_OP = 4,     /* answer encoder alone: an op slot of the response reads absent
                               (op_status 0xFF); the response's size is then not computed    */
  MOCHI_ENC_BAD_KIND = 5,   /* envelope encoder alone (device form): a kind above 12        */
  MOCHI_ENC_BAD_ID = 6,     /* envelope encoder alone (device form): an id that is not UTF-8 */
};

/* A safe upper bound on the wire size, from the counts and the two blob
 * lengths of `counts_only` alone (no pointer is dereferenced).  Grants may
 * share bytes, so every grant is taken at grant_bytes_len and every string at
 * strings_len, capped by 2^31 - 1 bytes per message: safe, not tight.  A caller
 * that wants the exact size calls the encoder with wire_cap = 0 and reads
 * *wire_len. */
uint64_t mochi_write2_encode_bound(const mochi_write2_source* counts_only, uint32_t max_id_len);

/* Host form: every array in host memory, no context, no GPU (the CPU twin of
 * the device form, as mochi_write1_classify is).  ids / id_off[n_ids+1] is the
 * server-id table (as mochi_ctx_set_server_ids takes it).  Messages are packed
 * back to back: msg_off[m] is the sum of the earlier lengths (64-bit).
 * msg_off[M], msg_len[M] and status[M] are always written; when wire_cap is
 * smaller than the total the call returns MOCHI_EINVAL with *wire_len = the
 * size needed and writes no byte of `wire`.  Inconsistent CSR arrays or a
 * string slice outside `strings` are MOCHI_EINVAL. */
int mochi_write2_encode(const mochi_write2_source* src, const uint8_t* ids, const uint32_t* id_off, uint32_t n_ids,
                        uint8_t* wire, uint64_t wire_cap, uint64_t* msg_off, uint32_t* msg_len, uint8_t* status,
                        uint64_t* wire_len);

/* Device form: every array of `src` and wire / msg_off / msg_len / status in
 * DEVICE memory, wire_len on the host; server ids from mochi_ctx_set_server_ids
 * (MOCHI_EINVAL without them).  The call waits for the total size, then returns
 * with the emit kernels enqueued on `stream` (hipStream_t; NULL = null stream).
 * Same bytes, offsets, statuses and capacity rule as the host form; the CSR
 * arrays and string slices are trusted. */
int mochi_write2_encode_device(mochi_ctx* ctx, const mochi_write2_source* src, uint8_t* wire, uint64_t wire_cap,
                               uint64_t* msg_off, uint32_t* msg_len, uint8_t* status, uint64_t* wire_len,
                               void* stream);
/* Per-kernel device time (ms) of the last mochi_write2_encode_device call made
 * while profiling was on (mochi_ctx_set_profiling): [0] k_enc_mg, [1] k_enc_msg,
 * [2] the 64-bit scan, [3] k_enc_hdr_mg, [4] k_enc_hdr_msg, [5] k_enc_copy.
 * Waits for that call.  n_kernels <= 6. */
int mochi_ctx_read_encode_profile(mochi_ctx* ctx, float* kernel_ms, uint32_t n_kernels);

/* ------------------------------------------------------------------------
 * Producer side on the device: SHA256withRSA over each grant's bytes with ONE
 * server's private key (RSA-2048, CRT), the Write1 signing site
 * (InMemoryDataStore.java:283-295, MochiProtocol.proto:123 TODO).  Output is
 * bit-identical to mochi_sign_grants / OpenSSL (PKCS#1 v1.5 is deterministic).
 * ------------------------------------------------------------------------ */
typedef struct mochi_signer mochi_signer;
mochi_signer* mochi_signer_create(int device, const char* pem_private_key);
void mochi_signer_destroy(mochi_signer* s);
/* Host memory, synchronous; sig_out: n * 256 bytes. */
int mochi_sign_batch(mochi_signer* s, const uint8_t* grant_bytes, uint64_t grant_bytes_len, const uint64_t* grant_off,
                     const uint32_t* grant_len, uint32_t n, uint8_t* sig_out);
/* Device memory, asynchronous on `stream`. */
int mochi_sign_batch_device(mochi_signer* s, const uint8_t* grant_bytes, const uint64_t* grant_off,
                            const uint32_t* grant_len, uint32_t n, uint8_t* sig_out, void* stream);
/* Every signature is verified with the signer's public key before it is
 * released (same stream, ~2 % of the signing cost): a transient fault in one
 * RSA-CRT half would otherwise publish s with gcd(s^e - EM, n) = a prime factor.
 * A failing signature is written as 256 zero bytes (it verifies nowhere).
 * mochi_signer_rejected waits for the device and returns (and clears) the
 * number withheld since the last call. */
int mochi_signer_rejected(mochi_signer* s, uint64_t* rejected);
/* Test hook: corrupt the CRT half m_p of grant `grant_index` of every later call
 * (0xFFFFFFFF = off), to show the fault check withholding it. */
int mochi_signer_set_fault(mochi_signer* s, uint32_t grant_index);

/* ------------------------------------------------------------------------
 * Write1 grant issuance for a batch of Write1ToServer requests: which grants
 * this server gives (InMemoryDataStore.java:105-155 processWrite, :233-310
 * tryProcessWriteRegularly, StoreValueObjectContainer.java:100-133), their
 * Grant bytes, and (device form) their signatures.
 *
 * The result equals processing the requests one after another in batch order,
 * the ops of a request in transaction order, against the caller's state as of
 * batch start (epochs do not move during Write1).  Per op:
 *   action not WRITE / DELETE                          -> SKIP (no grant)
 *   an earlier WRITE / DELETE op of the request had an
 *   empty operand1 (the reference threw there)         -> SKIPPED (claims nothing)
 *   the empty-key op itself                            -> FAILED
 *   not LOCAL                                          -> WRONG_SHARD: a new Grant
 *       {objectId, transactionHash, status = 1}, counted as granted; a later
 *       non-local op of the same request on a byte-equal key refers to it
 *   LOCAL without HAS_SVOC (DELETE of an absent key)   -> FAILED
 *   LOCAL with HAS_SVOC: slot (object, ts), ts = op_epoch + req_seed (64-bit
 *       wrapping, seed unsigned)
 *     op_stored names a stored grant: RETRY (granted) when the request's
 *       transactionHash byte-equals the stored one, else REFUSED; both refer
 *       to the stored grant
 *     slot free: the op with the smallest batch-wide op index among all ops
 *       that reach the slot is NEW (Grant {objectId, timestamp = ts,
 *       transactionHash}; a zero timestamp is omitted, proto3).  Every other
 *       op on it is RETRY when its request's hash equals the winner's
 *       request's, else REFUSED; both refer to the new grant.  A winner stays
 *       the winner whatever becomes of its own request (the reference has
 *       stored the grant by then, :139).
 * Request kind: THROWS if any op FAILED, else REFUSED if any op REFUSED, else
 * OK.  The reply's MultiGrant view lists each distinct grant once, at the first
 * op that refers to it, in op order: the granted ops (NEW / RETRY /
 * WRONG_SHARD) for OK, the REFUSED ops for REFUSED (:283-308), nothing for
 * THROWS.  Java's HashMap iteration order is not reproduced: wire order is the
 * caller's, as in mochi_write2_source.  New grants are numbered in the order of
 * the ops that made them, so the host and device forms give identical arrays.
 * Afterwards the host stores EVERY new grant, whatever its request's kind.
 * ------------------------------------------------------------------------ */
#define MOCHI_W1OP_LOCAL 0x01    /* objectBelongsToCurrentShardServer(operand1)            */
#define MOCHI_W1OP_HAS_SVOC 0x02 /* the key has a container (a caller creates it for a
                                    WRITE before the batch, as getOrCreateStoreValue does) */
#define MOCHI_W1OP_WRITE 0x04    /* action == WRITE                                        */
#define MOCHI_W1OP_DELETE 0x08   /* action == DELETE                                       */
#define MOCHI_W1_NONE 0xFFFFFFFFu   /* op_stored: slot free; op_grant: no grant            */
#define MOCHI_W1_STORED 0x80000000u /* op_grant / req_grant: MOCHI_W1_STORED | stored index */

enum mochi_w1_op_decision {
  MOCHI_W1D_SKIP = 0,
  MOCHI_W1D_SKIPPED = 1,
  MOCHI_W1D_FAILED = 2,
  MOCHI_W1D_WRONG_SHARD = 3,
  MOCHI_W1D_NEW = 4,
  MOCHI_W1D_RETRY = 5,
  MOCHI_W1D_REFUSED = 6,
};
enum mochi_w1_req_kind { MOCHI_W1K_OK = 0, MOCHI_W1K_REFUSED = 1, MOCHI_W1K_THROWS = 2 };

typedef struct mochi_write1_batch {
  uint32_t n_reqs, n_ops, n_stored;         /* n_ops below 2^30, n_stored below 2^31        */
  const uint8_t*  strings; uint64_t strings_len; /* keys and hashes                         */
  const uint32_t* req_op_off;    /* [Q+1] ops per request (at most MOCHI_MAX_OPS_PER_CERT)  */
  const uint32_t* req_seed;      /* [Q]   Write1ToServer.seed                               */
  const uint64_t* req_hash_off; const uint32_t* req_hash_len; /* [Q] transactionHash, any length */
  const uint64_t* op_key_off;   const uint32_t* op_key_len;   /* [O] operand1                */
  const uint8_t*  op_flags;      /* [O] MOCHI_W1OP_*                                        */
  const uint32_t* op_obj;        /* [O] the caller's index of the key's container (LOCAL ops
                                    only; equal keys <=> equal index; 0xFFFFFFFF reserved)  */
  const int64_t*  op_epoch;      /* [O] the container's current epoch                       */
  const uint32_t* op_stored;     /* [O] stored grant at (object, ts), or MOCHI_W1_NONE      */
  const uint64_t* stored_hash_off; const uint32_t* stored_hash_len; /* [S] its transactionHash */
} mochi_write1_batch;

/* Every array is the caller's.  op_* and req_grant, grant_off / grant_len /
 * grant_op / grant_ts (and sig, 256 bytes each) hold n_ops entries (n_new <=
 * n_ops); n_new and grant_bytes_len are written by the call (host fields in
 * both forms).  grant_bytes with grant_off / grant_len is the input layout of
 * mochi_sign_batch_device, and with sig the grant part of mochi_write2_source. */
typedef struct mochi_write1_issued {
  uint8_t*  op_decision;   /* [O] mochi_w1_op_decision                                      */
  uint32_t* op_grant;      /* [O] new-grant index, MOCHI_W1_STORED | stored index, or NONE  */
  uint8_t*  req_kind;      /* [Q] mochi_w1_req_kind                                         */
  uint32_t* req_grant_off; /* [Q+1] the reply's MultiGrant view                             */
  uint32_t* req_grant;     /* [req_grant_off[Q]] grant references (as op_grant)             */
  uint32_t  n_new;         /* out: new grants                                               */
  uint64_t  grant_bytes_len; /* out: bytes of the new grants (the capacity needed)          */
  uint8_t*  grant_bytes;  uint64_t grant_cap;  /* new grants back to back, in index order   */
  uint64_t* grant_off;     /* [n_new]                                                       */
  uint32_t* grant_len;     /* [n_new]                                                       */
  uint32_t* grant_op;      /* [n_new] the op that made the grant                            */
  int64_t*  grant_ts;      /* [n_new] its timestamp (0 for a WRONG_SHARD grant)             */
  uint8_t*  sig;           /* [n_new][256] or NULL = do not sign (device form only)         */
} mochi_write1_issued;

/* A safe upper bound on grant_bytes_len from n_ops and strings_len of
 * `counts_only` alone (no pointer is dereferenced): every op a new grant with a
 * key and a hash of strings_len bytes each. */
uint64_t mochi_write1_issue_bound(const mochi_write1_batch* counts_only);

/* Host form: host arrays, no GPU, no key; `sig` is ignored.  MOCHI_EINVAL for a
 * req_op_off that is not a CSR over n_ops, a slice outside `strings`, more than
 * MOCHI_MAX_OPS_PER_CERT ops in a request, a stored index >= n_stored, or LOCAL
 * ops with equal op_obj and different op_epoch.  When grant_cap is smaller than
 * the size needed the call returns MOCHI_EINVAL with out->grant_bytes_len (and
 * *bytes_needed, which may be NULL) = that size and out->n_new set, having
 * written op_decision, req_kind and req_grant_off and nothing else. */
int mochi_write1_issue(const mochi_write1_batch* batch, mochi_write1_issued* out, uint64_t* bytes_needed);

/* Device form: every array of `batch` and `out` in DEVICE memory (the structs
 * themselves on the host); scratch hangs off the signer.  The call waits once,
 * for n_new and the byte total, then returns with the emit kernels and, when
 * out->sig is not NULL, k_rsa_sign and the public-key check over the new grants
 * enqueued on `stream`.  Same outputs and capacity rule as the host form; the
 * inputs are trusted. */
int mochi_write1_issue_device(mochi_signer* s, const mochi_write1_batch* batch, mochi_write1_issued* out,
                              void* stream);
/* Per-kernel device time (ms) of the last mochi_write1_issue_device call made
 * while profiling was on: [0] table clear + k_w1_pre, [1] k_w1_claim,
 * [2] k_w1_decide, [3] k_w1_reply (count), [4] the 64-bit scans, [5] k_w1_emit,
 * [6] k_w1_reply (write), [7] k_rsa_sign + the public-key check (0 without
 * sig).  Waits for that call.  n <= 8. */
int mochi_signer_set_profiling(mochi_signer* s, int on);
int mochi_signer_read_issue_profile(mochi_signer* s, float* kernel_ms, uint32_t n);

/* ------------------------------------------------------------------------
 * Write1 REPLY ENCODE: the bodies the server answers a Write1 batch with
 * (InMemoryDataStore.java:283-308, MochiProtocol.proto:117-161), one blob with
 * msg_off / msg_len.  Request q's slice is the body of ProtocolMessage field
 * 108 (write1OkFromServer) for req_kind OK, 109 (write1RefusedFromServer) for
 * REFUSED and 112 (requestFailedFromServer, OLD_REQUEST: the empty body) for
 * THROWS; the payload case is req_kind's, so no further output is needed.
 *
 *   Write1OkFromServer / Write1RefusedFromServer (same layout)
 *     = 0A len MultiGrant                      always, also when empty (0A 00)
 *       { 12 len ( 0A len objectId  12 len WriteCertificate ) }
 *                                              per listed grant with a certificate
 *     clientId = 3 and hash = 4 are never set by the reference: never written
 *   MultiGrant as in mochi_write2_source: grants entries, clientId, serverId
 *     (each iff non-empty), grantSignatures entries iff issued->sig is given.
 *
 * The listed grants of request q are req_grant[req_grant_off[q] ..
 * req_grant_off[q+1]) as mochi_write1_issue wrote them; the entries of all
 * three maps are in that order (Java's HashMap order is not reproduced).  The
 * map key of an entry is operand1 of the first listed op of the request that
 * refers to the grant (for a new and for a stored grant this is
 * Grant.objectId; no grant is parsed), and its certificate is the one given
 * for that same op.
 *
 * mochi_write1_reply_source is what the batch and the issue outputs do not
 * hold already.  The server id and the client ids are slices of a blob of
 * their own, `ids` (not of the batch's `strings`).  stored_* are the bytes and
 * signatures of the batch's stored grants (S = batch.n_stored), read only for
 * references MOCHI_W1_STORED | i.  op_cert_* give per op the serialized
 * WriteCertificate of its container (getCurrentC()), opaque bytes copied as
 * given; length 0 = no certificate = no currentCertificates entry (a non-null
 * EMPTY certificate cannot arise: setCurrentC stores only certificates that
 * reached quorum).  Slices of different ops may alias.  op_cert_off and
 * op_cert_len both NULL = no certificates at all.  Signatures are written iff
 * issued->sig is not NULL; stored_sig is then required when n_stored > 0.
 * ------------------------------------------------------------------------ */
typedef struct mochi_write1_reply_source {
  const uint8_t*  ids;          uint64_t ids_len;        /* server id and client ids      */
  uint64_t server_id_off;       uint32_t server_id_len;  /* MochiContext.getServerId()    */
  const uint64_t* req_client_off; const uint32_t* req_client_len; /* [Q] Write1ToServer.clientId;
                                                            both NULL = empty              */
  const uint8_t*  stored_bytes; uint64_t stored_bytes_len;
  const uint64_t* stored_off;   const uint32_t* stored_len; /* [S]                         */
  const uint8_t*  stored_sig;   /* [S][256], or NULL without signatures                    */
  const uint8_t*  certs;        uint64_t certs_len;
  const uint64_t* op_cert_off;  const uint32_t* op_cert_len; /* [O] or both NULL            */
} mochi_write1_reply_source;

/* A safe upper bound on the wire size from counts and blob lengths alone:
 * every op a listed grant whose key is strings_len long, whose grant is the
 * longer of grant_bytes_len (the new grants) and stored_bytes_len, and whose
 * certificate is certs_len long, every id ids_len long, capped by 2^31 - 1
 * bytes per request: safe, not tight (slices may alias).  The exact size comes
 * from the encoder called with wire_cap = 0. */
uint64_t mochi_write1_reply_bound(uint32_t n_reqs, uint32_t n_ops, uint64_t strings_len, uint64_t ids_len,
                                  uint64_t grant_bytes_len, uint64_t stored_bytes_len, uint64_t certs_len,
                                  int with_signatures);

/* Host form: every array in host memory, no GPU, no key; `batch` and `issued`
 * exactly as mochi_write1_issue took and wrote them (n_new set; with a sig
 * array the caller filled for signatures).  Messages are packed back to back;
 * msg_off[Q], msg_len[Q] and status[Q] are always written.  status reuses
 * mochi_enc_status: MOCHI_ENC_OK, or MOCHI_ENC_TOO_LONG for a body of 2^31
 * bytes or more, which gets length 0.  A THROWS request gets length 0 and
 * MOCHI_ENC_OK.  When wire_cap is smaller than the total the call returns
 * MOCHI_EINVAL with *wire_len = the size needed and writes no byte of `wire`.
 * MOCHI_EINVAL also for: req_op_off that is not a CSR over n_ops;
 * req_grant_off that is not a CSR of at most n_ops references; a req_kind
 * that is no mochi_w1_req_kind; a req_grant reference outside n_new /
 * n_stored; a reference that no listed op of its request refers to; an id,
 * key, grant or certificate slice outside its blob; stored_sig missing while
 * signatures are written and n_stored > 0. */
int mochi_write1_reply_encode(const mochi_write1_batch* batch, const mochi_write1_issued* issued,
                              const mochi_write1_reply_source* src, uint8_t* wire, uint64_t wire_cap,
                              uint64_t* msg_off, uint32_t* msg_len, uint8_t* status, uint64_t* wire_len);

/* Device form: every array of the three structs and wire / msg_off / msg_len /
 * status in DEVICE memory, the structs themselves on the host; same bytes,
 * offsets and statuses as the host form; the inputs are trusted.  Scratch
 * hangs off the signer (its own, apart from the issue call's), the call takes
 * the signer's lock and orders itself behind the signer's last call on another
 * stream as mochi_write1_issue_device does.  It may be called on the issuing
 * stream right after mochi_write1_issue_device with no synchronisation in
 * between: it reads op_decision, op_grant, req_*, grant_* and sig in stream
 * order (issued->n_new is the host field that call set).
 *   wire_len != NULL: the call waits once for the total, applies the host
 *     form's capacity rule on the host and returns with the emit kernels
 *     enqueued.  Behind an issue call with sig on the same stream that wait
 *     sits behind the signing kernels.
 *   wire_len == NULL, wire_len_dev a device uint64_t*: no host wait.  The
 *     total goes to *wire_len_dev; every kernel that writes `wire` reads the
 *     total and writes nothing when it exceeds wire_cap (all or nothing, on
 *     the device); msg_off / msg_len / status are written either way and the
 *     call returns MOCHI_OK.  A caller that allocates
 *     mochi_write1_reply_bound bytes never waits for a size. */
int mochi_write1_reply_encode_device(mochi_signer* s, const mochi_write1_batch* batch,
                                     const mochi_write1_issued* issued, const mochi_write1_reply_source* src,
                                     uint8_t* wire, uint64_t wire_cap, uint64_t* msg_off, uint32_t* msg_len,
                                     uint8_t* status, uint64_t* wire_len, uint64_t* wire_len_dev, void* stream);
/* Per-kernel device time (ms) of the last mochi_write1_reply_encode_device call
 * made while profiling was on (mochi_signer_set_profiling) and that emitted:
 * [0] k_w1r_size, [1] the 64-bit scan, [2] k_w1r_hdr, [3] k_w1r_copy.  Waits
 * for that call.  n <= 4. */
int mochi_signer_read_reply_profile(mochi_signer* s, float* kernel_ms, uint32_t n);

/* ------------------------------------------------------------------------
 * Write1 REPLY DECODE: the client's side of the bodies above.  The
 * Write1OkFromServer / Write1RefusedFromServer bytes a client received become
 * the arrays mochi_write1_classify and mochi_write2_source read, with
 * protobuf-java 3.16.3 parsing semantics (as the Write2 decoder: singular
 * fields last-wins, unknown fields and groups to depth 100 skipped, strings
 * and map keys strict UTF-8, maps in LinkedHashMap order -- a repeated key
 * keeps its first position and takes its last value --, every Grant and
 * WriteCertificate value parsed all the way down even where a later entry
 * replaces it).  The bytes are a Byzantine server's: every read stays inside
 * the response's slice (the signature gather reads the 16-byte-aligned chunks
 * that hold a signature byte, as the Write2 decoder's does).
 *
 * Input.  Response p is wire[resp_off[p], +resp_len[p]) (field 108 / 109 of a
 * ProtocolMessage; any alignment; slices may alias) with payload case
 * resp_kind[p] (MOCHI_W1_*), known from the envelope.  Request q owns
 * responses [req_resp_off[q], req_resp_off[q+1]) in arrival order (a CSR over
 * all n_resps) and sent the ops [req_op_off[q], req_op_off[q+1]) (at most
 * MOCHI_MAX_OPS_PER_CERT), op o with operand1 strings[op_key_off[o],
 * +op_key_len[o]).  n_resps is at most 2^24.
 * ------------------------------------------------------------------------ */
typedef struct mochi_write1_replies {
  uint32_t n_resps, n_reqs, n_ops, _pad0;      /* P, Q, O */
  const uint8_t*  wire;    uint64_t wire_len;
  const uint64_t* resp_off;      /* [P] */
  const uint32_t* resp_len;      /* [P] */
  const uint8_t*  resp_kind;     /* [P] MOCHI_W1_* */
  const uint32_t* req_resp_off;  /* [Q+1] */
  const uint8_t*  strings; uint64_t strings_len;
  const uint32_t* req_op_off;    /* [Q+1] */
  const uint64_t* op_key_off;    /* [O] */
  const uint32_t* op_key_len;    /* [O] */
} mochi_write1_replies;

/* Per-response decode status. */
enum mochi_w1r_status {
  MOCHI_W1R_OK = 0,
  /* protobuf-java would throw while parsing the body as its message type */
  MOCHI_W1R_MALFORMED = 1,
  /* well-formed (validated whole, never malformed) but outside the shape this
   * decoder handles, not decoded: multiGrant given more than once (a merge); a
   * grants or currentCertificates entry carrying its value more than once; a
   * decoded Grant whose bytes are not what Grant.toByteArray() would write;
   * more than 64 grants, grantSignatures or currentCertificates entries on the
   * wire (repeated keys included) */
  MOCHI_W1R_FALLBACK = 2,
  /* decoded like an OK one, but MultiGrant.serverId equals no table entry */
  MOCHI_W1R_UNKNOWN_SERVER = 3,
};
#define MOCHI_W1G_HAS_SIG 0x01     /* grantSignatures[map key] exists with exactly 256 bytes */
#define MOCHI_W1G_KEY_DIFFERS 0x02 /* the map key is not Grant.objectId                      */

/* Output; every array is the caller's.  Responses of kind REQUEST_FAILED /
 * OTHER are not parsed: status OK, no grants, no certificates.  A response
 * whose status is MALFORMED or FALLBACK has resp_kind_out MOCHI_W1_OTHER (so
 * that a reply nobody decoded never counts as an empty OK), no grants and no
 * certificates.  A missing multiGrant (an empty body too) is the default
 * MultiGrant: no grants, serverId empty.
 *   resp_server: the key index of MultiGrant.serverId.  Where no table entry
 *     equals it, and for every response that was not decoded, it is
 *     0x80000000 | p: distinct from every key index and from every other
 *     response's value, so such a reply never supersedes another server's in
 *     mochi_write1_classify.
 *   mg_signer: the same index as mochi_write2_source.mg_signer takes it,
 *     0xFFFF if unknown or not decoded.
 *   resp_client_off / _len: MultiGrant.clientId (last occurrence), an offset
 *     into `wire`; 0 / 0 if not decoded.  Here and below, a field that is
 *     absent gives the response's own offset and length 0.
 *   resp_grant_off / resp_cert_off [P+1]: CSRs over the grants / certificates.
 * Per grant, in map order: grant_off / grant_len point into `wire` (zero
 * copy); grant_key = slot of the first op of the response's request whose
 * operand1 byte-equals the MAP KEY (what allGrants.get(op.getOperand1()) finds,
 * MochiDBClient.java:203), 0xFF if none; grant_ts = Grant.timestamp;
 * grant_status = Grant.status, 0xFF for a value outside 0..254; grant_flags =
 * MOCHI_W1G_*; sig[g] (optional, NULL = not wanted) = the 256 signature bytes,
 * zeros without MOCHI_W1G_HAS_SIG.  Per currentCertificates entry, in map
 * order: key and value slices of `wire`; the value has been validated as a
 * WriteCertificate and is otherwise opaque.
 *
 * The arrays of a batch plug into mochi_write1_classify[_device] (resp_off =
 * req_resp_off, resp_kind = resp_kind_out, resp_server, resp_grant_off,
 * grant_key, grant_ts, grant_status) and, for the rounds it answers PROCEED,
 * into mochi_write2_source (grant_bytes = wire, grant_off, grant_len, sig,
 * cert_mg_off = req_resp_off, mg_grant_off = resp_grant_off, mg_signer).
 *
 * Capacity: grant_cap / cert_cap are the entries the per-grant / per-
 * certificate arrays hold.  n_grants and n_certs (host fields) are always
 * written, and so are the per-response arrays and both CSRs; when a capacity
 * is too small the call returns MOCHI_EINVAL with the counts needed and
 * touches no per-grant or per-certificate array. */
typedef struct mochi_write1_decoded {
  uint8_t*  resp_status;      /* [P] enum mochi_w1r_status */
  uint8_t*  resp_kind_out;    /* [P] */
  uint32_t* resp_server;      /* [P] */
  uint16_t* mg_signer;        /* [P] */
  uint64_t* resp_client_off;  /* [P] */
  uint32_t* resp_client_len;  /* [P] */
  uint32_t* resp_grant_off;   /* [P+1] */
  uint32_t* resp_cert_off;    /* [P+1] */
  uint32_t  n_grants, n_certs;   /* out */
  uint32_t  grant_cap, cert_cap; /* in  */
  uint64_t* grant_off;        /* [N] */
  uint32_t* grant_len;        /* [N] */
  uint8_t*  grant_key;        /* [N] */
  int64_t*  grant_ts;         /* [N] */
  uint8_t*  grant_status;     /* [N] */
  uint8_t*  grant_flags;      /* [N] */
  uint8_t*  sig;              /* [N][256] or NULL */
  uint64_t* cert_key_off;     /* [C] */
  uint32_t* cert_key_len;     /* [C] */
  uint64_t* cert_val_off;     /* [C] */
  uint32_t* cert_val_len;     /* [C] */
} mochi_write1_decoded;

/* Safe capacities from wire_len and n_resps alone: slices may alias, so every
 * response is taken at the whole blob; an entry takes two bytes or more and a
 * decoded response holds at most 64 of each kind.  Safe, not tight. */
void mochi_write1_reply_decode_bound(uint64_t wire_len, uint32_t n_resps, uint64_t* grants, uint64_t* certs);

/* Host form: every array in host memory, no context, no GPU; ids / id_off[n_ids+1]
 * is the server-id table as mochi_write2_encode takes it (the first equal entry
 * wins).  MOCHI_EINVAL for a response or operand slice outside its blob, a
 * req_resp_off that is not a CSR over n_resps, a req_op_off that is not a CSR
 * over n_ops or gives a request more than MOCHI_MAX_OPS_PER_CERT ops, a
 * resp_kind that is no MOCHI_W1_*, or more than 2^24 responses. */
int mochi_write1_reply_decode(const mochi_write1_replies* replies, const uint8_t* ids, const uint32_t* id_off,
                              uint32_t n_ids, mochi_write1_decoded* out);

/* Device form: every array of `replies` and `out` in DEVICE memory, the structs
 * themselves on the host; server ids from mochi_ctx_set_server_ids
 * (MOCHI_EINVAL without them); scratch is the context's.  The call waits once,
 * for the two totals, applies the capacity rule on the host and returns with
 * the emit kernels enqueued on `stream` (hipStream_t; NULL = null stream).
 * Same arrays as the host form; the caller's own arrays (CSRs, operand slices,
 * response slices inside `wire`) are trusted, the bytes of `wire` are not. */
int mochi_write1_reply_decode_device(mochi_ctx* ctx, const mochi_write1_replies* replies, mochi_write1_decoded* out,
                                     void* stream);
/* Per-kernel device time (ms) of the last mochi_write1_reply_decode_device call
 * made while profiling was on (mochi_ctx_set_profiling) and that emitted:
 * [0] k_w1d_resp, [1] the entry scan, [2] k_w1d_level2, [3] k_w1d_final + the
 * packed scan + k_w1d_offsets, [4] k_w1d_emit, [5] the signature gather.  Waits
 * for that call.  n_kernels <= 6. */
int mochi_ctx_read_w1_decode_profile(mochi_ctx* ctx, float* kernel_ms, uint32_t n_kernels);

/* ------------------------------------------------------------------------
 * Write1 REQUEST DECODE: the server's side of the Write1 round.  The
 * Write1ToServer bodies a server received (field 107 of a ProtocolMessage,
 * MochiProtocol.proto:92-97) become the wire half of mochi_write1_batch, with
 * protobuf-java 3.16.3 parsing semantics (as the reply decoder: singular
 * fields last-wins, unknown fields and known field numbers with a foreign wire
 * type skipped, groups to depth 100, field number 0 or a bad varint malformed,
 * every string strict UTF-8 -- clientId, transactionHash and operand1 / 2 / 3
 * of every Operation whatever its action --, seed and Operation.action the low
 * 32 bits of their varint).  The bytes are a Byzantine client's: every read
 * stays inside the request's slice.
 *
 *   Write1ToServer = [0A clientId] [12 Transaction] [18 seed] [22 transactionHash]
 *   Transaction    = { 0A Operation }
 *   Operation      = [08 action] [12 operand1] [1A operand2] [22 operand3]
 *
 * Input.  Request q is wire[msg_off[q], +msg_len[q]) (any alignment; slices
 * may alias).  n_reqs is at most 2^24.
 * ------------------------------------------------------------------------ */
typedef struct mochi_write1_requests {
  uint32_t n_reqs, _pad0;        /* Q */
  const uint8_t*  wire;    uint64_t wire_len;
  const uint64_t* msg_off;       /* [Q] */
  const uint32_t* msg_len;       /* [Q] */
} mochi_write1_requests;

/* Per-request decode status. */
enum mochi_w1q_status {
  MOCHI_W1Q_OK = 0,
  /* protobuf-java would throw while parsing the body as a Write1ToServer */
  MOCHI_W1Q_MALFORMED = 1,
  /* well-formed (validated whole, never malformed) but not decoded:
   * `transaction` given more than once (a merge); more than
   * MOCHI_MAX_OPS_PER_CERT operations */
  MOCHI_W1Q_FALLBACK = 2,
};

/* Output; every array is the caller's.  Offsets point into `wire` (zero copy);
 * a field that is absent gives the request's own offset and length 0.  A
 * request whose status is not OK has no ops, seed 0 and slices 0 / 0: the
 * caller sends it no reply.
 *   req_seed: Write1ToServer.seed.  req_hash_*: transactionHash.
 *   req_client_*: clientId.  req_op_off [Q+1]: a CSR over the ops.
 * Per op, in transaction order: op_key_off / op_key_len = operand1; op_flags =
 * MOCHI_W1OP_WRITE for action 2, MOCHI_W1OP_DELETE for action 1 and 0 for any
 * other value (unknown enum values included); op_obj = the index of the op's
 * key among the batch's distinct keys, MOCHI_W1_NONE for an op that has none.
 * Keys are compared byte for byte; only WRITE and DELETE ops with a non-empty
 * operand1 take part (every op here belongs to an OK request); keys are
 * numbered by their first op in op order, so the host and device forms give
 * identical arrays.  key_op[u] = the first op that holds key u (the slice to
 * look the store up with).
 *
 * These arrays are mochi_write1_batch's strings (= wire), req_op_off,
 * req_seed, req_hash_*, op_key_* and op_obj, and the wire half of op_flags
 * (mochi_write1_state_join adds the rest); with ids = wire they are
 * mochi_write1_reply_source.req_client_* too.
 *
 * Capacity: op_cap is the entries the per-op arrays and key_op hold.  n_ops (a
 * host field in both forms) is always written, and so are the per-request
 * arrays and req_op_off; when op_cap < n_ops the call returns MOCHI_EINVAL and
 * touches no per-op array, key_op or n_keys. */
typedef struct mochi_write1_requests_decoded {
  uint8_t*  req_status;       /* [Q] enum mochi_w1q_status */
  uint32_t* req_seed;         /* [Q] */
  uint64_t* req_hash_off;     /* [Q] */
  uint32_t* req_hash_len;     /* [Q] */
  uint64_t* req_client_off;   /* [Q] */
  uint32_t* req_client_len;   /* [Q] */
  uint32_t* req_op_off;       /* [Q+1] */
  uint32_t  n_ops;            /* out */
  uint32_t  n_keys;           /* out (host form; the device form leaves it 0) */
  uint32_t  op_cap, _pad0;    /* in  */
  uint64_t* op_key_off;       /* [O] */
  uint32_t* op_key_len;       /* [O] */
  uint8_t*  op_flags;         /* [O] */
  uint32_t* op_obj;           /* [O] */
  uint32_t* key_op;           /* [op_cap]; n_keys entries written */
} mochi_write1_requests_decoded;

/* A safe op_cap from wire_len and n_reqs alone: slices may alias, so every
 * request is taken at the whole blob; an op takes two bytes or more and a
 * decoded request holds at most MOCHI_MAX_OPS_PER_CERT.  Safe, not tight. */
uint64_t mochi_write1_request_decode_bound(uint64_t wire_len, uint32_t n_reqs);

/* Host form: every array in host memory, no signer, no GPU.  MOCHI_EINVAL for
 * a request slice outside `wire` or more than 2^24 requests. */
int mochi_write1_request_decode(const mochi_write1_requests* requests, mochi_write1_requests_decoded* out);

/* Device form: every array of `requests` and `out` and n_keys_dev (one
 * uint32_t) in DEVICE memory, the structs themselves on the host.  Scratch
 * hangs off the signer (its own, apart from the issue and reply encode
 * calls'); the call takes the signer's lock and orders itself behind the
 * signer's last call on another stream as mochi_write1_reply_encode_device
 * does.  It waits once, for n_ops, applies the capacity rule on the host and
 * returns with the remaining kernels enqueued on `stream` (hipStream_t; NULL =
 * null stream); the number of distinct keys goes to *n_keys_dev.  Same arrays
 * as the host form; the caller's offsets are trusted, the bytes of `wire` are
 * not. */
int mochi_write1_request_decode_device(mochi_signer* s, const mochi_write1_requests* requests,
                                       mochi_write1_requests_decoded* out, uint32_t* n_keys_dev, void* stream);
/* Per-kernel device time (ms) of the last mochi_write1_request_decode_device
 * call made while profiling was on (mochi_signer_set_profiling) and that
 * emitted: [0] k_w1q_req, [1] the entry scan, [2] k_w1q_ops, [3] k_w1q_final +
 * the op scan + k_w1q_offsets, [4] k_w1q_emit, [5] the table clear +
 * k_w1q_claim, [6] k_w1q_rank, [7] the key scan, [8] k_w1q_number.  Waits for
 * that call.  n <= 9. */
int mochi_signer_read_request_profile(mochi_signer* s, float* kernel_ms, uint32_t n);

/* STATE JOIN: from "state per distinct key" to the per-op state arrays of
 * mochi_write1_batch.  The host looks the store up once per distinct key
 * (key_op names an op that holds it) and gives, per key u: key_flags =
 * MOCHI_W1OP_LOCAL | MOCHI_W1OP_HAS_SVOC as they apply; key_epoch = the
 * container's current epoch; key_given_off [U+1], a CSR over the container's
 * given Write1 grants, each with its timestamp given_ts and given_stored, its
 * index among the batch's stored grants. */
typedef struct mochi_write1_key_state {
  uint32_t n_keys, n_given;      /* U, G */
  const uint8_t*  key_flags;     /* [U] */
  const int64_t*  key_epoch;     /* [U] */
  const uint32_t* key_given_off; /* [U+1] */
  const int64_t*  given_ts;      /* [G] */
  const uint32_t* given_stored;  /* [G] */
} mochi_write1_key_state;

/* Per op o of request q with u = op_obj[o] != MOCHI_W1_NONE: op_flags[o] =
 * op_flags_wire[o] | key_flags[u]; op_epoch[o] = key_epoch[u]; op_stored[o] =
 * given_stored of the first entry of u's list whose timestamp equals
 * key_epoch[u] + req_seed[q] (64-bit wrapping, seed unsigned), else
 * MOCHI_W1_NONE (isGivenWrite1GrantsEmpty() || getGrantIfExistsAtTimeStamp(ts)
 * == null, InMemoryDataStore.java:127-128).  An op without a key index keeps
 * its flags and gets epoch 0 and MOCHI_W1_NONE.  op_flags may be
 * op_flags_wire (in place).
 * Host form: MOCHI_EINVAL for a req_op_off that is not a CSR over n_ops, a
 * key_given_off that is not a CSR over n_given, or an op_obj >= n_keys. */
int mochi_write1_state_join(uint32_t n_reqs, uint32_t n_ops, const uint32_t* req_op_off, const uint32_t* req_seed,
                            const uint8_t* op_flags_wire, const uint32_t* op_obj, const mochi_write1_key_state* keys,
                            uint8_t* op_flags, int64_t* op_epoch, uint32_t* op_stored);
/* Device form: every array (those of `keys` too) in DEVICE memory; one kernel
 * on `stream` on the signer's device, no host wait, no scratch; the inputs are
 * trusted. */
int mochi_write1_state_join_device(mochi_signer* s, uint32_t n_reqs, uint32_t n_ops, const uint32_t* req_op_off,
                                   const uint32_t* req_seed, const uint8_t* op_flags_wire, const uint32_t* op_obj,
                                   const mochi_write1_key_state* keys, uint8_t* op_flags, int64_t* op_epoch,
                                   uint32_t* op_stored, void* stream);

/* ------------------------------------------------------------------------
 * RESULT REPLY DECODE: the client's closing round.  The Write2AnsFromServer /
 * ReadFromServer bodies a client received (MochiProtocol.proto:45-60, 82-87,
 * 102-105) become the arrays mochi_tally_responses[_device] reads, and the
 * per-operation values the accepted TransactionResult is coalesced from, with
 * protobuf-java 3.16.3 parsing semantics (as the Write1 reply decoder:
 * singular fields last-wins, unknown fields and known field numbers with a
 * foreign wire type skipped, groups to depth 100, every string strict UTF-8,
 * every currentCertificate validated as a WriteCertificate all the way down,
 * in an operation past the transaction's count too; status the low 32 bits of
 * its varint, existed any non-zero varint).  The bytes are a Byzantine
 * server's: every read stays inside the response's slice.
 *
 *   Write2AnsFromServer = [0A TransactionResult] [12 rid]
 *   ReadFromServer      = [0A TransactionResult] [12 nonce] [1A rid]
 *   TransactionResult   = { 0A OperationResult }
 *   OperationResult     = [0A result] [12 WriteCertificate] [18 existed] [20 status]
 *
 * Field 3 is a string in a ReadFromServer alone: invalid UTF-8 in a length-
 * delimited field 3 makes a read answer MALFORMED and leaves a Write2 answer OK.
 *
 * Input.  Response p is wire[resp_off[p], +resp_len[p]) (any alignment; slices
 * may alias) with payload case resp_kind[p] (MOCHI_RR_*), known from the
 * envelope.  Request q owns responses [req_resp_off[q], req_resp_off[q+1]) in
 * arrival order (a CSR over all n_resps) and sent n_ops[q] operations (at most
 * MOCHI_MAX_OPS_PER_CERT).  Response p of request q owns the n_ops[q] slots
 * [slot_off[p], +n_ops[q]) of the per-slot arrays: slot_off is the array the
 * tally takes as status_off, need not be dense or ascending, and the slot runs
 * of two responses must not overlap here (they are written).  n_resps is at
 * most 2^24.
 * ------------------------------------------------------------------------ */
#define MOCHI_RR_WRITE2_ANS 0 /* WRITE2ANSFROMSERVER */
#define MOCHI_RR_READ 1       /* READFROMSERVER      */
#define MOCHI_RR_OTHER 2      /* any other payload: getWrite2AnsFromServer() / getReadFromServer() give the default
                                 message, 0 operations (MochiDBClient.java:155, :362) */
typedef struct mochi_result_replies {
  uint32_t n_resps, n_reqs;      /* P, Q */
  const uint8_t*  wire;    uint64_t wire_len;
  const uint64_t* resp_off;      /* [P] */
  const uint32_t* resp_len;      /* [P] */
  const uint8_t*  resp_kind;     /* [P] MOCHI_RR_* */
  const uint32_t* req_resp_off;  /* [Q+1] */
  const uint32_t* n_ops;         /* [Q] */
  const uint64_t* slot_off;      /* [P] */
} mochi_result_replies;

/* Per-response decode status. */
enum mochi_rr_status {
  MOCHI_RRS_OK = 0,
  /* protobuf-java would throw while parsing the body as its message type */
  MOCHI_RRS_MALFORMED = 1,
  /* well-formed (validated whole, never malformed) but not decoded: `result`
   * given more than once (a merge concatenates the lists); an OperationResult
   * among the request's first n_ops carrying currentCertificate more than once
   * (the two maps merge: no single slice is the value) */
  MOCHI_RRS_FALLBACK = 2,
};
#define MOCHI_RRO_HAS_CERT 0x01 /* the OperationResult carries a currentCertificate */

/* Output; every array is the caller's.  Offsets point into `wire` (zero copy).
 * Per response:
 *   resp_n_ops: the OperationResult count on the wire, whatever it is (more
 *     than MOCHI_MAX_OPS_PER_CERT too: such a body is validated whole and, as
 *     its count can equal no n_ops, none of its slots holds a value); 0
 *     without a `result` and for kind OTHER (not parsed: status OK);
 *     0xFFFFFFFF for a MALFORMED or FALLBACK response, which so equals no
 *     n_ops, not even 0: a reply nobody decoded never counts as an empty one.
 *   resp_rid_* / resp_nonce_*: last occurrence (a Write2 answer has no nonce);
 *     0 / 0 if not decoded or not parsed.  Here and below, a field that is
 *     absent gives its message's own offset and length 0.
 * Per slot j < n_ops[q] of response p, at slot_off[p] + j: op_status =
 * OperationResult.status (0 OK, 1 WRONG_SHARD), 0xFF for a value outside
 * 0..254 -- the array is mochi_tally_responses' `status` --; op_existed;
 * op_flags = MOCHI_RRO_*; the `result` string and the currentCertificate as
 * slices, the certificate validated and otherwise opaque.  All n_ops[q] slots
 * of every response are written and nothing else is: the slots at or past the
 * response's count, and all slots of a response that is not OK, read absent
 * (status 0xFF, existed 0, flags 0, slices 0 / 0). */
typedef struct mochi_result_decoded {
  uint8_t*  resp_status;     /* [P] enum mochi_rr_status */
  uint32_t* resp_n_ops;      /* [P] */
  uint64_t* resp_rid_off;    /* [P] */
  uint32_t* resp_rid_len;    /* [P] */
  uint64_t* resp_nonce_off;  /* [P] */
  uint32_t* resp_nonce_len;  /* [P] */
  uint8_t*  op_status;       /* per slot */
  uint8_t*  op_existed;
  uint8_t*  op_flags;
  uint64_t* op_result_off;
  uint32_t* op_result_len;
  uint64_t* op_cert_off;
  uint32_t* op_cert_len;
} mochi_result_decoded;

/* Host form: every array in host memory, no context, no GPU.  MOCHI_EINVAL for
 * a response slice outside `wire`, a req_resp_off that is not a CSR over
 * n_resps, an n_ops above MOCHI_MAX_OPS_PER_CERT, a resp_kind that is no
 * MOCHI_RR_*, more than 2^24 responses, responses without a request, or a
 * NULL array (with n_resps > 0 every array of both structs is read or
 * written).  With n_resps == 0 no pointer is needed and nothing is written. */
int mochi_result_reply_decode(const mochi_result_replies* replies, mochi_result_decoded* out);

/* Device form: every array of `replies` and `out` in DEVICE memory, the structs
 * themselves on the host; scratch is the context's.  No host wait: every output
 * size follows from the caller's own arrays, so the call returns with all its
 * kernels enqueued on `stream` (hipStream_t; NULL = null stream), and
 * mochi_tally_responses_device (resp_off = req_resp_off, status_off =
 * slot_off, status = op_status) and mochi_result_coalesce_device may be
 * enqueued behind it at once.  The caller's own arrays are trusted, the bytes
 * of `wire` are not. */
int mochi_result_reply_decode_device(mochi_ctx* ctx, const mochi_result_replies* replies, mochi_result_decoded* out,
                                     void* stream);
/* Per-kernel device time (ms) of the last mochi_result_reply_decode_device call
 * made while profiling was on (mochi_ctx_set_profiling): [0] k_rr_resp, [1] the
 * operation scan, [2] k_rr_ops, [3] k_rr_final.  Waits for that call.
 * n_kernels <= 4. */
int mochi_ctx_read_result_decode_profile(mochi_ctx* ctx, float* kernel_ms, uint32_t n_kernels);

/* COALESCE: the TransactionResult the client returns once the tally accepted
 * (MochiDBClient.java:177-179 / :384-386): per op, the result of the LAST
 * response that did not answer WRONG_SHARD.  Inputs: the decoder's request CSR,
 * n_ops, slot_off and per-slot arrays, and the tally's chosen / chosen_off /
 * accept_bits. */
typedef struct mochi_result_tallied {
  uint32_t n_reqs, _pad0;        /* Q */
  const uint32_t* req_resp_off;  /* [Q+1] */
  const uint32_t* n_ops;         /* [Q] */
  const int32_t*  chosen;        /* the tally's: index among the request's responses, or -1 */
  const uint64_t* chosen_off;    /* [Q] */
  const uint32_t* accept_bits;   /* [ceil(Q/32)] */
  const uint64_t* slot_off;      /* [P] */
  const uint8_t*  op_status;     /* per slot, as mochi_result_decoded */
  const uint8_t*  op_existed;
  const uint8_t*  op_flags;
  const uint64_t* op_result_off;
  const uint32_t* op_result_len;
  const uint64_t* op_cert_off;
  const uint32_t* op_cert_len;
  const uint64_t* out_off;       /* [Q] where request q's n_ops[q] entries start in the outputs */
} mochi_result_tallied;
/* Per (request, op) at out_off[q] + j: resp = the chosen response's index among
 * ALL responses (req_resp_off[q] + chosen), and that response's slot values.  A
 * request whose accept bit is 0 gets resp 0xFFFFFFFF and absent values (status
 * 0xFF, existed 0, flags 0, slices 0 / 0) in all its ops. */
typedef struct mochi_result_coalesced {
  uint32_t* resp;
  uint8_t*  status;
  uint8_t*  existed;
  uint8_t*  flags;
  uint64_t* result_off;
  uint32_t* result_len;
  uint64_t* cert_off;
  uint32_t* cert_len;
} mochi_result_coalesced;
/* Host form.  MOCHI_EINVAL for a NULL array, a req_resp_off that descends, an
 * n_ops above MOCHI_MAX_OPS_PER_CERT, or a chosen index of an accepted request
 * at or past its response count.  With n_reqs == 0 no pointer is needed. */
int mochi_result_coalesce(const mochi_result_tallied* tallied, mochi_result_coalesced* out);
/* Device form: every array in DEVICE memory; one kernel on `stream` on the
 * current device (lane = request), no host wait, no scratch; the inputs are
 * trusted. */
int mochi_result_coalesce_device(const mochi_result_tallied* tallied, mochi_result_coalesced* out, void* stream);

/* ------------------------------------------------------------------------
 * Answer ENCODER (the server's closing round): the inverse of
 * mochi_result_reply_decode.  The Write2AnsFromServer / ReadFromServer bodies
 * of a batch from caller arrays, byte for byte what protobuf-java writes
 * (InMemoryDataStore.java:641-666, :521-574, :582-587, :75-103, :201-231):
 *
 *   Write2AnsFromServer = 0A len TransactionResult   always, also when empty (0A 00: setResult is always called)
 *                         [12 rid]                   iff non-empty
 *   ReadFromServer      = 0A len TransactionResult  [12 nonce] [1A rid]   each string iff non-empty
 *   TransactionResult   = { 0A len OperationResult } one per op, also when empty (0A 00)
 *   OperationResult     = [0A result] iff non-empty
 *                         [12 len cert] iff HAS_CERT, also when empty (12 00: processRead sets the default instance)
 *                         [18 01] iff existed
 *                         [20 varint(status)] iff status != 0
 *
 * Input.  Response p has kind resp_kind[p] (MOCHI_RR_WRITE2_ANS / MOCHI_RR_READ;
 * MOCHI_RR_OTHER: no body, length 0, status OK), resp_n_ops[p] operations (at
 * most MOCHI_MAX_OPS_PER_CERT) in the slots [slot_off[p], +resp_n_ops[p]) of
 * the per-slot arrays, which are n_slots long; slot_off need not be dense or
 * ascending and the slot runs of two responses must not overlap (as in the
 * decoder).  rid and nonce are slices of `ids`; either pair of arrays may be
 * NULL (empty); a Write2 answer has no nonce.  `ids` may be the same pointer as
 * `wire` (a read's nonce is a slice of the request it came in: see
 * mochi_read_answer_plan); the encoder only reads both.  Per slot: op_status 0..254 is
 * written as a varint (128..254 take two bytes), 0xFF -- the decoder's
 * "absent" mark -- makes the response MOCHI_ENC_BAD_OP; op_existed;
 * op_flags = MOCHI_RAO_*; the `result` string and the certificate as slices of
 * `wire` (the received request bytes: an applied op answers with the incoming
 * certificate and its own operand2) or, by flag, of `store` (stored values and
 * certificates).  Slices may alias and have any alignment; certificates are
 * opaque bytes, copied as given.
 * ------------------------------------------------------------------------ */
#define MOCHI_RAO_HAS_CERT 0x01     /* = MOCHI_RRO_HAS_CERT: currentCertificate is written, also when empty */
#define MOCHI_RAO_RESULT_STORE 0x02 /* op_result_off points into `store`, not `wire` */
#define MOCHI_RAO_CERT_STORE 0x04   /* op_cert_off points into `store`, not `wire`   */
typedef struct mochi_result_answers {
  uint32_t n_resps, n_slots;     /* P, S */
  const uint8_t*  wire;    uint64_t wire_len;
  const uint8_t*  store;   uint64_t store_len;
  const uint8_t*  ids;     uint64_t ids_len;
  const uint8_t*  resp_kind;     /* [P] MOCHI_RR_* */
  const uint32_t* resp_n_ops;    /* [P] */
  const uint64_t* slot_off;      /* [P] */
  const uint64_t* rid_off;       /* [P] into ids; NULL with rid_len = every rid empty */
  const uint32_t* rid_len;
  const uint64_t* nonce_off;     /* [P] into ids; NULL with nonce_len = every nonce empty */
  const uint32_t* nonce_len;
  const uint8_t*  op_status;     /* [S] */
  const uint8_t*  op_existed;
  const uint8_t*  op_flags;      /* MOCHI_RAO_* */
  const uint64_t* op_result_off;
  const uint32_t* op_result_len;
  const uint64_t* op_cert_off;
  const uint32_t* op_cert_len;
} mochi_result_answers;

/* A safe wire_cap from counts and blob lengths alone (n_ops: the sum of resp_n_ops). */
uint64_t mochi_result_reply_encode_bound(uint32_t n_resps, uint64_t n_ops, uint64_t wire_len, uint64_t store_len,
                                         uint64_t ids_len);

/* Host form: every array in host memory.  Outputs as mochi_write1_reply_encode:
 * message p is wire_out[msg_off[p], +msg_len[p]), packed back to back in
 * response order with 64-bit offsets; status[p] is enum mochi_enc_status
 * (MOCHI_ENC_TOO_LONG: 2^31 bytes or more; it and MOCHI_ENC_BAD_OP give length
 * 0); *wire_len the total.  MOCHI_EINVAL, with *wire_len set and no byte
 * written, when wire_cap is smaller; MOCHI_EINVAL also for a slice outside its
 * blob, a slot run outside n_slots, a resp_n_ops above MOCHI_MAX_OPS_PER_CERT,
 * a kind that is no MOCHI_RR_*, or a NULL required array.  With n_resps == 0 no
 * pointer but wire_len is needed and nothing is written. */
int mochi_result_reply_encode(const mochi_result_answers* answers, uint8_t* wire_out, uint64_t wire_cap,
                              uint64_t* msg_off, uint32_t* msg_len, uint8_t* status, uint64_t* wire_len);

/* Device form: every array of `answers` and every output in DEVICE memory, the
 * struct itself on the host; scratch is the context's.  The caller's arrays are
 * trusted.  The two capacity modes of mochi_write1_reply_encode_device:
 * wire_len (host) non-NULL: one wait for the total, MOCHI_EINVAL with the needed
 * size and no byte written if it exceeds wire_cap; wire_len NULL and
 * wire_len_dev (device) non-NULL: no host wait, the total goes to *wire_len_dev,
 * and every kernel that writes wire_out reads it first and writes nothing if it
 * exceeds wire_cap (msg_off / msg_len / status are written either way). */
int mochi_result_reply_encode_device(mochi_ctx* ctx, const mochi_result_answers* answers, uint8_t* wire_out,
                                     uint64_t wire_cap, uint64_t* msg_off, uint32_t* msg_len, uint8_t* status,
                                     uint64_t* wire_len, uint64_t* wire_len_dev, void* stream);
/* Per-kernel device time (ms) of the last mochi_result_reply_encode_device call
 * made while profiling was on: [0] k_rae_size, [1] the offset scan, [2]
 * k_rae_hdr, [3] k_rae_copy.  Waits for that call.  n_kernels <= 4. */
int mochi_ctx_read_result_encode_profile(mochi_ctx* ctx, float* kernel_ms, uint32_t n_kernels);

/* ------------------------------------------------------------------------
 * Write2 answer PLAN: from the verifier's outputs to the encoder's input.  Per
 * message of the mochi_write2_batch the verify call took (op_flags_off is
 * required here), from msg_status / cert_accept_bits / op_decision as
 * mochi_verify_write2[_device] left them and the store's side of every op:
 *   MOCHI_W2A_REPLY     msg_status OK, accepted, every decision APPLY, READ or
 *     WRONG_SHARD: resp_kind = MOCHI_RR_WRITE2_ANS, resp_n_ops = the op count.
 *     WRONG_SHARD -> status 1 alone.  APPLY -> status 0, result = the op's
 *     operand2 (a slice of batch->wire), existed = (action == WRITE), HAS_CERT,
 *     certificate = the message's field 1 (a slice of batch->wire; absent:
 *     length 0).  READ -> status 0, existed 1, result = the stored value
 *     (RESULT_STORE), certificate = the stored one (CERT_STORE; HAS_CERT iff
 *     MOCHI_W2A_HAS_STORED_CERT).
 *   MOCHI_W2A_NO_REPLY  the reference threw (not accepted, a FAILED / SKIPPED
 *     decision, msg_status MALFORMED / OPS_MISMATCH, a READ of an op marked
 *     MOCHI_W2A_VALUE_NULL, or a body whose operations the walk cannot match to
 *     op_flags_off): resp_kind = MOCHI_RR_OTHER, every slot absent.
 *   MOCHI_W2A_HOST      msg_status FALLBACK but accepted (merged or repeated
 *     fields have no single slice): resp_kind = MOCHI_RR_OTHER, every slot
 *     absent; the caller builds this answer.
 * The walk takes the last length-delimited field 1 of the body and, per
 * Operation of field 2, the last `action` varint (low 32 bits) and the last
 * length-delimited field 3; every read stays inside the message's slice.  An
 * absent operand2 gives the Operation's own offset and length 0, an absent
 * certificate the message's own offset and length 0; WRONG_SHARD slots and a
 * READ without a stored certificate carry offset 0 / length 0.
 * Message m owns the slots [slot_off[m], +its op count) of the per-slot outputs,
 * which are n_slots long; all of them are written and nothing else is.
 * Dependencies between messages of one batch are the caller's, as for verify.
 * ------------------------------------------------------------------------ */
#define MOCHI_W2A_REPLY 0
#define MOCHI_W2A_NO_REPLY 1
#define MOCHI_W2A_HOST 2
#define MOCHI_W2A_HAS_STORED_CERT 0x01 /* the key's container holds a certificate                      */
#define MOCHI_W2A_VALUE_NULL 0x02      /* getValue() is null: setResult(null) throws (:567), no reply */
typedef struct mochi_write2_answer_source {
  const uint8_t*  msg_status;          /* [M] enum mochi_msg_status */
  const uint32_t* cert_accept_bits;    /* [ceil(M/32)] */
  const uint8_t*  op_decision;         /* [O] enum mochi_op_decision, O = op_flags_off[M] */
  const uint64_t* op_value_off;        /* [O] into the store blob */
  const uint32_t* op_value_len;
  const uint64_t* op_stored_cert_off;  /* [O] into the store blob */
  const uint32_t* op_stored_cert_len;
  const uint8_t*  op_store_flags;      /* [O] MOCHI_W2A_* bits */
  uint64_t store_len;                  /* size of the store blob (the host form checks slices against it) */
  const uint64_t* slot_off;            /* [M] */
  uint32_t n_slots, _pad0;
} mochi_write2_answer_source;
/* The arrays of a mochi_result_answers with n_resps = M (wire = batch->wire,
 * store = the store blob), and the plan's verdict per message. */
typedef struct mochi_write2_answer_planned {
  uint8_t*  plan_status;     /* [M] MOCHI_W2A_* */
  uint8_t*  resp_kind;       /* [M] */
  uint32_t* resp_n_ops;      /* [M] */
  uint8_t*  op_status;       /* [S] */
  uint8_t*  op_existed;
  uint8_t*  op_flags;
  uint64_t* op_result_off;
  uint32_t* op_result_len;
  uint64_t* op_cert_off;
  uint32_t* op_cert_len;
} mochi_write2_answer_planned;
/* Host form.  MOCHI_EINVAL for a NULL array, a message slice outside wire, an
 * op_flags_off that is not a CSR, a slot run outside n_slots, or a stored slice
 * outside store_len.  With n_msgs == 0 no pointer is needed. */
int mochi_write2_answer_plan(const mochi_write2_batch* batch, const mochi_write2_answer_source* src,
                             mochi_write2_answer_planned* out);
/* Device form: every array in DEVICE memory; one kernel (k_w2a_plan, lane =
 * message) on `stream` on the current device, no host wait, no scratch: it may
 * be enqueued right behind mochi_verify_write2_device, and
 * mochi_result_reply_encode_device right behind it.  The caller's own arrays
 * are trusted, the bytes of `wire` are not. */
int mochi_write2_answer_plan_device(const mochi_write2_batch* batch, const mochi_write2_answer_source* src,
                                    mochi_write2_answer_planned* out, void* stream);

/* ------------------------------------------------------------------------
 * Read REQUEST DECODE: the server's side of a read.  The ReadToServer bodies a
 * server received (field 105 of a ProtocolMessage, MochiProtocol.proto:72-76)
 * become SoA arrays, with the parsing semantics of mochi_write1_request_decode
 * (protobuf-java 3.16.3: singular fields last-wins, unknown fields and known
 * field numbers with a foreign wire type skipped -- field 3 as a varint and
 * field 4 of any type are unknown here --, groups to depth 100, field number 0
 * or a bad varint malformed; clientId, nonce and operand1 / 2 / 3 of every
 * Operation strict UTF-8; Operation.action the low 32 bits of its varint).  The
 * bytes are a Byzantine client's: every read stays inside the request's slice.
 *
 *   ReadToServer = [0A clientId] [12 Transaction] [1A nonce]
 *   Transaction  = { 0A Operation }
 *   Operation    = [08 action] [12 operand1] [1A operand2] [22 operand3]
 *
 * Input: as mochi_write1_requests (n_reqs at most 2^24; slices may alias and
 * have any alignment).
 * ------------------------------------------------------------------------ */
typedef mochi_write1_requests mochi_read_requests;

/* Per-request decode status: the values and meanings of mochi_w1q_status. */
enum mochi_rdq_status {
  MOCHI_RDQ_OK = 0,
  MOCHI_RDQ_MALFORMED = 1, /* protobuf-java would throw while parsing the body as a ReadToServer */
  /* well-formed (validated whole, never malformed) but not decoded: `transaction`
   * given more than once; more than MOCHI_MAX_OPS_PER_CERT operations */
  MOCHI_RDQ_FALLBACK = 2,
};
#define MOCHI_RDOP_READ 0x01 /* op_flags: the action is READ (0, an absent action included) */

/* Output; every array is the caller's.  Offsets point into `wire`; a field that
 * is absent gives the request's own offset and length 0.  A request whose
 * status is not OK has no ops and slices 0 / 0.
 *   req_client_*: clientId.  req_nonce_*: nonce (with ids = wire they are the
 *   nonce_off / nonce_len of mochi_result_answers).  req_op_off [Q+1]: a CSR.
 * Per op, in transaction order: op_key_off / op_key_len = operand1; op_flags =
 * MOCHI_RDOP_READ for action 0 and 0 for any other value; op_obj = the index
 * of the op's key among the batch's distinct keys, MOCHI_W1_NONE for an op that
 * has none.  Only READ ops with a non-empty operand1 take part (every op here
 * belongs to an OK request); keys are compared byte for byte and numbered by
 * their first op in op order, so the host and device forms give identical
 * arrays.  key_op[u] = the first op that holds key u.
 * Capacity: n_ops / n_keys / op_cap as in mochi_write1_requests_decoded: n_ops
 * is always written; when op_cap < n_ops the call returns MOCHI_EINVAL and
 * touches no per-op array, key_op or n_keys. */
typedef struct mochi_read_requests_decoded {
  uint8_t*  req_status;       /* [Q] enum mochi_rdq_status */
  uint64_t* req_client_off;   /* [Q] */
  uint32_t* req_client_len;   /* [Q] */
  uint64_t* req_nonce_off;    /* [Q] */
  uint32_t* req_nonce_len;    /* [Q] */
  uint32_t* req_op_off;       /* [Q+1] */
  uint32_t  n_ops;            /* out */
  uint32_t  n_keys;           /* out (host form; the device form leaves it 0) */
  uint32_t  op_cap, _pad0;    /* in  */
  uint64_t* op_key_off;       /* [O] */
  uint32_t* op_key_len;       /* [O] */
  uint8_t*  op_flags;         /* [O] MOCHI_RDOP_* */
  uint32_t* op_obj;           /* [O] */
  uint32_t* key_op;           /* [op_cap]; n_keys entries written */
} mochi_read_requests_decoded;

/* A safe op_cap, as mochi_write1_request_decode_bound. */
uint64_t mochi_read_request_decode_bound(uint64_t wire_len, uint32_t n_reqs);

/* Host form: every array in host memory, no context, no GPU.  MOCHI_EINVAL for
 * a request slice outside `wire` or more than 2^24 requests. */
int mochi_read_request_decode(const mochi_read_requests* requests, mochi_read_requests_decoded* out);

/* Device form: every array of `requests` and `out` and n_keys_dev (one
 * uint32_t) in DEVICE memory, the structs themselves on the host.  A read signs
 * nothing: the call hangs off the context (the answer encoder's owner).  Its
 * scratch is the context's, apart from the other calls'; it takes the context's
 * lock and orders itself behind the context's last call on another stream.  It
 * waits once, for n_ops, applies the capacity rule on the host and returns with
 * the remaining kernels enqueued on `stream` (hipStream_t; NULL = null stream);
 * the number of distinct keys goes to *n_keys_dev.  The caller's offsets are
 * trusted, the bytes of `wire` are not. */
int mochi_read_request_decode_device(mochi_ctx* ctx, const mochi_read_requests* requests,
                                     mochi_read_requests_decoded* out, uint32_t* n_keys_dev, void* stream);
/* Per-kernel device time (ms) of the last mochi_read_request_decode_device call
 * made while profiling was on (mochi_ctx_set_profiling) and that emitted: [0]
 * k_rdq_req, [1] the entry scan, [2] k_w1q_ops, [3] k_rdq_final + the op scan +
 * k_rdq_offsets, [4] k_rdq_emit, [5] the table clear + k_w1q_claim, [6]
 * k_w1q_rank, [7] the key scan, [8] k_w1q_number.  Waits for that call.  n <= 9. */
int mochi_ctx_read_read_decode_profile(mochi_ctx* ctx, float* kernel_ms, uint32_t n);

/* ------------------------------------------------------------------------
 * Read answer PLAN: decoded read requests and the store's state per distinct
 * key to the encoder's input (InMemoryDataStore.processReadRequest :201-231 and
 * processRead :75-103 over arrays).  The host looks the store up once per
 * distinct key (key_op names an op that holds it) and gives, per key u,
 * key_flags and the value and the certificate as slices of a `store` blob (a
 * null value and an empty value both give length 0).
 *
 * Per request q:
 *   MOCHI_RDA_NO_REPLY  the reference threw: req_status MALFORMED; an op
 *     without MOCHI_RDOP_READ (checkAndFailOnReadOnly :217); an op with an empty
 *     operand1 (:77); an op whose key is LOCAL but not PRESENT (:99 dereferences
 *     null); an op whose key is LOCAL and PRESENT without HAS_CERT (:100,
 *     setCurrentCertificate(null) throws).  resp_kind = MOCHI_RR_OTHER,
 *     resp_n_ops = 0, every slot of the request absent (op_status 0xFF, the rest
 *     0, as mochi_write2_answer_plan writes them).
 *   MOCHI_RDA_HOST      req_status FALLBACK: resp_kind = MOCHI_RR_OTHER; the
 *     caller builds this answer.
 *   MOCHI_RDA_REPLY     everything else: resp_kind = MOCHI_RR_READ, resp_n_ops =
 *     the op count (zero ops: an empty TransactionResult).  Per op: key not
 *     LOCAL -> status 1 (WRONG_SHARD) alone; otherwise status 0, result = the
 *     value slice with MOCHI_RAO_RESULT_STORE, existed = AVAILABLE,
 *     MOCHI_RAO_HAS_CERT | MOCHI_RAO_CERT_STORE with the certificate slice (an
 *     empty one is still written, as 12 00).  Every other field of a slot is 0.
 * slot_off[q] = req_op_off[q]: the per-slot outputs are n_ops long and are the
 * seven per-slot arrays of mochi_result_answers (n_slots = n_ops, wire = the
 * requests' wire, store = the store blob).  The nonce goes to the encoder as
 * nonce_off / nonce_len = req_nonce_off / req_nonce_len with ids = wire: `ids`
 * may be the same pointer as `wire`.  A server that wants non-empty rids places
 * them in the same allocation behind wire_len and passes an ids_len that covers
 * them.
 * ------------------------------------------------------------------------ */
#define MOCHI_RDA_REPLY 0
#define MOCHI_RDA_NO_REPLY 1
#define MOCHI_RDA_HOST 2
#define MOCHI_RDK_LOCAL 0x01     /* objectBelongsToCurrentShardServer (the CONFIG_KEY_PREFIX rule is the caller's) */
#define MOCHI_RDK_PRESENT 0x02   /* a container exists */
#define MOCHI_RDK_AVAILABLE 0x04 /* isValueAvailble() */
#define MOCHI_RDK_HAS_CERT 0x08  /* getCurrentC() != null */
typedef struct mochi_read_key_state {
  uint32_t n_keys, _pad0;        /* U */
  const uint8_t*  key_flags;     /* [U] MOCHI_RDK_* */
  const uint64_t* key_value_off; /* [U] into the store blob */
  const uint32_t* key_value_len;
  const uint64_t* key_cert_off;  /* [U] into the store blob */
  const uint32_t* key_cert_len;
  uint64_t store_len;            /* size of the store blob (the host form checks slices against it) */
} mochi_read_key_state;
typedef struct mochi_read_answer_planned {
  uint8_t*  plan_status;     /* [Q] MOCHI_RDA_* */
  uint8_t*  resp_kind;       /* [Q] */
  uint32_t* resp_n_ops;      /* [Q] */
  uint64_t* slot_off;        /* [Q] = req_op_off[q] */
  uint8_t*  op_status;       /* [O] */
  uint8_t*  op_existed;
  uint8_t*  op_flags;
  uint64_t* op_result_off;
  uint32_t* op_result_len;
  uint64_t* op_cert_off;
  uint32_t* op_cert_len;
} mochi_read_answer_planned;
/* Host form.  Of `decoded` it reads req_status, req_op_off, n_ops, op_key_len,
 * op_flags and op_obj.  MOCHI_EINVAL for a NULL array, a req_op_off that is not
 * a CSR over n_ops, an op_obj >= n_keys that is not MOCHI_W1_NONE, or a key
 * slice outside store_len.  With n_reqs == 0 no pointer is needed. */
int mochi_read_answer_plan(uint32_t n_reqs, const mochi_read_requests_decoded* decoded,
                           const mochi_read_key_state* keys, mochi_read_answer_planned* out);
/* Device form: every array in DEVICE memory (decoded->n_ops is the host field
 * the decoder set); one kernel (k_rda_plan, lane = request) on `stream` on the
 * current device, no host wait, no scratch: it may be enqueued right behind
 * mochi_read_request_decode_device, and mochi_result_reply_encode_device right
 * behind it.  The caller's own arrays are trusted. */
int mochi_read_answer_plan_device(uint32_t n_reqs, const mochi_read_requests_decoded* decoded,
                                  const mochi_read_key_state* keys, mochi_read_answer_planned* out, void* stream);

/* ------------------------------------------------------------------------
 * The ProtocolMessage ENVELOPE (MochiProtocol.proto:194-213, one frame of
 * MochiServerInitializer.java:30-33 with Netty's length prefix stripped):
 *
 *   ProtocolMessage = [28 msgTimestamp] [32 serverId] [3A msgId] [42 replyToMsgId]
 *                     [payload: one of the fields 101..112, length-delimited]
 *
 * Four calls, each in a host form (no GPU, no context) and a device form:
 * decode (frames -> status, payload case, body slice, the four scalars), route
 * (the server's side: a stable partition of the OK frames by payload case, whose
 * runs are the msg_off / msg_len of the body decoders), join (the client's side:
 * replies matched to the outstanding requests by replyToMsgId, grouped by
 * request: the resp_off / resp_len / resp_kind / req_resp_off of the reply
 * decoders) and encode (bodies wrapped into frames, the inverse of decode).
 * What stays with the caller: msgId generation (UUIDs), sockets and cutting the
 * byte stream into frames.
 *
 * Frame f is wire[frame_off[f], +frame_len[f]): any alignment, slices may alias,
 * at most 2^24 frames.  The bytes are an untrusted peer's: every read stays
 * inside the frame's slice; the caller's own offsets are trusted (the host form
 * checks them against wire_len).  Parsing is protobuf-java 3.16.3's, as in the
 * body decoders: singular fields last-wins; unknown fields and known field
 * numbers with a foreign wire type are skipped (a payload field that is not
 * length-delimited included), groups to depth 100; field number 0 or a bad
 * varint is malformed; overlong varint tags are accepted; msgTimestamp is the
 * low 64 bits of its varint; serverId, msgId and replyToMsgId are strict UTF-8,
 * every occurrence of them.
 *
 * Status per frame:
 *   MOCHI_ENV_OK         the envelope level parses and holds at most one
 *     length-delimited field among 101..112.
 *   MOCHI_ENV_MALFORMED  protobuf-java throws on the envelope level itself
 *     (framing, a string that is not UTF-8), whatever the payloads are.
 *   MOCHI_ENV_FALLBACK   the envelope level parses, validated whole, and holds
 *     more than one length-delimited field among 101..112.  The generated parser
 *     parses every payload field it meets, merges when the case repeats and
 *     replaces when it changes: such a frame is either a merge, where no single
 *     slice is the value, or has a discarded body that Java still parsed and could
 *     have thrown on.  It is never MALFORMED on account of a body, and it is
 *     not decoded: the caller hands it to protobuf-java.  No canonical writer
 *     produces one.
 * Contract against the body decoders: Java throws on a frame exactly when the
 * envelope is MALFORMED, or it is OK and the decoder of its kind calls the body
 * MALFORMED.  The bodies of kinds 1-4 (the Hello messages) and 12
 * (RequestFailedFromServer) have no decoder here: they are returned as slices
 * and not validated.
 *
 * Outputs per frame, zero-copy offsets into `wire`; an absent field gives the
 * frame's own offset and length 0; a frame that is not OK has kind 0, timestamp
 * 0 and every length 0 (offsets: the frame's own).  kind: 0 = PAYLOAD_NOT_SET,
 * otherwise the field number - 100 (1..12); a present, empty payload has length
 * 0 and its kind.
 * ------------------------------------------------------------------------ */
enum mochi_env_status { MOCHI_ENV_OK = 0, MOCHI_ENV_MALFORMED = 1, MOCHI_ENV_FALLBACK = 2 };
#define MOCHI_ENV_KINDS 13 /* payload cases: 0 = not set, k = field number - 100 */
typedef struct mochi_envelope_frames {
  uint32_t n_frames, _pad0;
  const uint8_t*  wire;    uint64_t wire_len;
  const uint64_t* frame_off;   /* [n] */
  const uint32_t* frame_len;   /* [n] */
} mochi_envelope_frames;
typedef struct mochi_envelope_decoded {
  uint8_t*  status;            /* [n] enum mochi_env_status */
  uint8_t*  kind;              /* [n] 0..12 */
  uint64_t* body_off;          /* [n] the payload's value */
  uint32_t* body_len;
  int64_t*  msg_timestamp;     /* [n] */
  uint64_t* server_id_off;     /* [n] */
  uint32_t* server_id_len;
  uint64_t* msg_id_off;        /* [n] */
  uint32_t* msg_id_len;
  uint64_t* reply_to_off;      /* [n] */
  uint32_t* reply_to_len;
} mochi_envelope_decoded;
/* Host form.  MOCHI_EINVAL for a NULL array, more than 2^24 frames or a frame
 * slice outside wire.  With n_frames == 0 no pointer is needed. */
int mochi_envelope_decode(const mochi_envelope_frames* frames, mochi_envelope_decoded* out);
/* Device form: every array in DEVICE memory, the structs on the host; one
 * kernel (k_env_decode, lane = frame) on `stream`, no host wait, no scratch. */
int mochi_envelope_decode_device(mochi_ctx* ctx, const mochi_envelope_frames* frames, mochi_envelope_decoded* out,
                                 void* stream);

/* ROUTE, the server's side.  From the decode's status / kind / body_off /
 * body_len: kind_off[14], a CSR over the kinds 0..12 (kind_off[13] = the number
 * routed); order[], the indices of the OK frames kind-major, in frame order
 * inside a kind; body_off / body_len gathered in that order.  The run of kind 7
 * is mochi_write1_requests.msg_off / msg_len as it stands (at body_off +
 * kind_off[7], kind_off[8] - kind_off[7] long), the run of kind 10 the Write2
 * batch's, the run of kind 5 the read requests.  Frames that are not OK (or
 * carry a kind above 12) take no place; the entries of order / body_off /
 * body_len from kind_off[13] on are not written. */
typedef struct mochi_envelope_routed {
  uint32_t* kind_off;          /* [14] */
  uint32_t* order;             /* [n] */
  uint64_t* body_off;          /* [n] */
  uint32_t* body_len;          /* [n] */
} mochi_envelope_routed;
/* Host form.  MOCHI_EINVAL for a NULL array or more than 2^24 frames. */
int mochi_envelope_route(uint32_t n_frames, const uint8_t* status, const uint8_t* kind, const uint64_t* body_off,
                         const uint32_t* body_len, mochi_envelope_routed* out);
/* Device form: every array in DEVICE memory, kind_off included; no host wait (a
 * caller copies 14 words when it wants the counts).  The result equals the host
 * form's array for array: ranks come from ballots and a scan over per-block
 * histograms (k_env_hist, the scan, k_env_scatter), not from arrival at an
 * atomic.  Scratch is the context's. */
int mochi_envelope_route_device(mochi_ctx* ctx, uint32_t n_frames, const uint8_t* status, const uint8_t* kind,
                                const uint64_t* body_off, const uint32_t* body_len, mochi_envelope_routed* out,
                                void* stream);

/* JOIN, the client's side.  The outstanding requests' msgIds are slices of
 * `ids`; each OK frame's replyToMsgId is matched byte for byte against them.  An
 * empty replyToMsgId matches nothing (nor does an empty table id); an id that
 * occurs twice in the table resolves to the smaller request index.  Outputs:
 * frame_req[n], the frame's request or MOCHI_W1_NONE; req_resp_off[Q+1];
 * resp_frame[], the matched frames grouped by request, in frame order inside a
 * request; in that order resp_off / resp_len (the body slices) and the payload
 * case as the two reply decoders take it: resp_w1_kind (108 -> MOCHI_W1_OK, 109
 * -> MOCHI_W1_REFUSED, 112 -> MOCHI_W1_REQUEST_FAILED, else MOCHI_W1_OTHER) and
 * resp_rr_kind (111 -> MOCHI_RR_WRITE2_ANS, 106 -> MOCHI_RR_READ, else
 * MOCHI_RR_OTHER); P = req_resp_off[Q], the number of matched frames.  The
 * per-response arrays are n long; their entries from P on are not written.
 * Frames that are MALFORMED, FALLBACK or unmatched appear in no run: a frame
 * whose parse throws never reaches the reference's client either.  The
 * reference's client pairs replies by connection and never reads field 8; the
 * join by field 8 is this library's choice. */
typedef struct mochi_envelope_requests {
  uint32_t n_reqs, _pad0;      /* Q */
  const uint8_t*  ids;     uint64_t ids_len;
  const uint64_t* id_off;      /* [Q] */
  const uint32_t* id_len;      /* [Q] */
} mochi_envelope_requests;
typedef struct mochi_envelope_joined {
  uint32_t* frame_req;         /* [n] */
  uint32_t* req_resp_off;      /* [Q+1] */
  uint32_t* resp_frame;        /* [n], P written */
  uint64_t* resp_off;
  uint32_t* resp_len;
  uint8_t*  resp_w1_kind;
  uint8_t*  resp_rr_kind;
} mochi_envelope_joined;
/* Host form; *n_resps = P.  `decoded` is read (status, kind, body_off, body_len,
 * reply_to_off, reply_to_len; the other arrays may be NULL).  MOCHI_EINVAL for a
 * NULL array, more than 2^24 frames or requests, an id outside ids or a
 * replyToMsgId outside wire. */
int mochi_envelope_join(const mochi_envelope_requests* requests, const mochi_envelope_frames* frames,
                        const mochi_envelope_decoded* decoded, mochi_envelope_joined* out, uint32_t* n_resps);
/* Device form: every array in DEVICE memory; P goes to the device word
 * *n_resps_dev; no host wait.  The msgId table is an open-addressing claim
 * table in the context's scratch (k_w1q_claim's: at least 2 * Q slots, the
 * smallest claimant wins); the grouping is a stable radix sort by request index.
 * Array for array the host form's result. */
int mochi_envelope_join_device(mochi_ctx* ctx, const mochi_envelope_requests* requests,
                               const mochi_envelope_frames* frames, const mochi_envelope_decoded* decoded,
                               mochi_envelope_joined* out, uint32_t* n_resps_dev, void* stream);

/* ENCODE: wrap.  Per message a kind (0..12), a body slice of `bodies` (a body
 * encoder's output in place; ignored for kind 0), msg_timestamp, and msgId /
 * replyToMsgId / serverId as slices of `ids` (any pair of arrays may be NULL:
 * every such string empty).  `ids` may be a received wire: a reply's
 * replyToMsgId is the request's msgId slice, no copy.  Output: exactly the bytes
 * ProtocolMessage.toByteArray() writes: fields in number order 5, 6, 7, 8, then
 * the payload; zero and empty scalars omitted; a set payload written even when
 * empty (DA 06 00 for kind 7); kind 0 writes no payload.  With
 * MOCHI_ENV_LENGTH_PREFIX in `flags` ProtobufVarint32LengthFieldPrepender's
 * varint32 goes in front of each message: msg_off / msg_len still name the
 * message, the prefix lies in the bytes just before it. */
#define MOCHI_ENV_LENGTH_PREFIX 0x1
typedef struct mochi_envelope_source {
  uint32_t n_msgs, flags;      /* M; MOCHI_ENV_* */
  const uint8_t*  bodies;  uint64_t bodies_len;
  const uint8_t*  ids;     uint64_t ids_len;
  const uint8_t*  kind;            /* [M] */
  const uint64_t* body_off;        /* [M] into bodies */
  const uint32_t* body_len;
  const int64_t*  msg_timestamp;   /* [M] */
  const uint64_t* msg_id_off;      /* [M] into ids; NULL with msg_id_len = every msgId empty */
  const uint32_t* msg_id_len;
  const uint64_t* reply_to_off;    /* [M] into ids */
  const uint32_t* reply_to_len;
  const uint64_t* server_id_off;   /* [M] into ids */
  const uint32_t* server_id_len;
} mochi_envelope_source;
/* A safe wire_cap from counts and blob lengths alone. */
uint64_t mochi_envelope_encode_bound(uint32_t n_msgs, uint64_t bodies_len, uint64_t ids_len);
/* Host form.  Outputs, capacity rule and argument order as
 * mochi_result_reply_encode: messages packed back to back in order with 64-bit
 * offsets, status[m] enum mochi_enc_status (MOCHI_ENC_TOO_LONG gives length 0),
 * *wire_len the total; MOCHI_EINVAL with *wire_len set and no byte written when
 * wire_cap is smaller.  MOCHI_EINVAL also for a kind above 12, an id that is
 * not UTF-8, a slice outside its blob, unknown flags or a NULL required array.
 * With n_msgs == 0 no pointer but wire_len is needed. */
int mochi_envelope_encode(const mochi_envelope_source* src, uint8_t* wire_out, uint64_t wire_cap, uint64_t* msg_off,
                          uint32_t* msg_len, uint8_t* status, uint64_t* wire_len);
/* Device form: every array in DEVICE memory, the two capacity modes of
 * mochi_result_reply_encode_device.  The caller's arrays are trusted, their
 * values are not: a kind above 12 is MOCHI_ENC_BAD_KIND and an id that is not
 * UTF-8 MOCHI_ENC_BAD_ID for that message, which is emitted with length 0 (with
 * the prefix flag: the one byte 00), and the call succeeds.  k_env_size, the
 * offset scan, k_env_hdr, and k_env_copy, which copies the bodies with the
 * encoders' shared chunk copy (16 lanes per short body, one wave per long one). */
int mochi_envelope_encode_device(mochi_ctx* ctx, const mochi_envelope_source* src, uint8_t* wire_out,
                                 uint64_t wire_cap, uint64_t* msg_off, uint32_t* msg_len, uint8_t* status,
                                 uint64_t* wire_len, uint64_t* wire_len_dev, void* stream);
/* Per-kernel device time (ms) of the last device call of kind `which` made while
 * profiling was on.  Waits for that call.
 *   MOCHI_ENV_PROF_DECODE  [0] k_env_decode
 *   MOCHI_ENV_PROF_ROUTE   [0] k_env_hist, [1] the scan, [2] k_env_scatter
 *   MOCHI_ENV_PROF_JOIN    [0] table clear + k_env_claim, [1] k_env_lookup, [2] the sort, [3] k_env_group
 *   MOCHI_ENV_PROF_ENCODE  [0] k_env_size, [1] the offset scan, [2] k_env_hdr, [3] k_env_copy
 * n_kernels <= 4; entries past the call's stages are 0. */
#define MOCHI_ENV_PROF_DECODE 0
#define MOCHI_ENV_PROF_ROUTE 1
#define MOCHI_ENV_PROF_JOIN 2
#define MOCHI_ENV_PROF_ENCODE 3
int mochi_ctx_read_envelope_profile(mochi_ctx* ctx, int which, float* kernel_ms, uint32_t n_kernels);

/* ------------------------------------------------------------------------
 * Micro-batcher: the blocking per-request call the Java handler keeps
 * (Write2ToServerRequestHandler.handle -> processWrite2ToServer on a 2..20
 * thread pool, MochiServer.java:36-40), coalesced across threads into one
 * mochi_verify_write2 call by a flusher thread: a batch goes out when
 * max_msgs requests are pending or the oldest has waited max_wait_us.
 * ------------------------------------------------------------------------ */
typedef struct mochi_batcher mochi_batcher;

typedef struct mochi_verdict1 {
  uint8_t accepted;   /* certificate accepted                 */
  uint8_t reason;     /* enum mochi_reason                    */
  uint8_t fail_op;    /* first failing op, 0xFF if none       */
  uint8_t msg_status; /* enum mochi_msg_status                */
} mochi_verdict1;

/* with_op_flags: 1 = every call passes op_flags[n_ops] (MOCHI_OP_* per op, in
 * transaction order); 0 = calls pass NULL / 0 and every op counts as
 * LOCAL|HAS_SVOC.  The batcher borrows `ctx` (one batcher per context). */
mochi_batcher* mochi_batcher_create(mochi_ctx* ctx, const mochi_params* params, uint32_t max_msgs,
                                    uint32_t max_wait_us, int with_op_flags);
/* The same over n_ctx contexts (e.g. two on one GPU): one flusher thread per
 * context takes the next batch while the others are on the GPU, so n batches
 * are in flight.  The batcher borrows the contexts. */
mochi_batcher* mochi_batcher_create_multi(mochi_ctx* const* ctxs, uint32_t n_ctx, const mochi_params* params,
                                          uint32_t max_msgs, uint32_t max_wait_us, int with_op_flags);
typedef void (*mochi_verdict_cb)(void* user, int rc, const mochi_verdict1* verdict);

/* One Write2ToServer request (ABI 3): the message body plus the receiving
 * server's per-op state and optional per-op outputs.  Everything stays owned by
 * the caller and must stay valid until the verdict is delivered. */
typedef struct mochi_write2_request {
  const uint8_t* msg;            /* Write2ToServer body (ProtocolMessage field 110)            */
  uint32_t msg_len;
  uint32_t n_ops;                /* operations in the message's transaction                   */
  const uint8_t* op_flags;       /* [n_ops] MOCHI_OP_* (batcher created with with_op_flags)     */
  const int64_t* op_object_ts;   /* [n_ops] stored currentC timestamp, read iff HAS_CURRENT_C;
                                    NULL = none                                                */
  const uint8_t* expected_hash;  /* [128] objectSHA512(transaction), lowercase hex              */
  uint8_t* op_decision;          /* [n_ops] out: enum mochi_op_decision (NULL = not wanted)     */
  uint32_t* op_g0;               /* [n_ops] out: certificate-relative index of g0               */
  int64_t* op_ts;                /* [n_ops] out: g0's timestamp (what applyOperation records)   */
} mochi_write2_request;

/* Blocks until this request's verdict is in `out` (and its per-op outputs are
 * written).  Thread-safe.  Returns the status of the batch call that carried
 * it.  This is the call a server's Write2 handler makes in place of
 * InMemoryDataStore.processWrite2ToServer (InMemoryDataStore.java:641-666): the
 * per-op decision says which operations applyOperation / readOperation runs.
 * MOCHI_EINVAL (and mochi_last_error) from a completion callback running on
 * this batcher: a callback submits instead. */
int mochi_batcher_verify_request(mochi_batcher* b, const mochi_write2_request* req, mochi_verdict1* out);
/* Non-blocking form: cb(user, rc, &verdict) runs on a flusher thread once the
 * batch is verified, after the per-op outputs are written.  A callback may
 * submit to the batcher running it (e.g. the next stage of a future chain);
 * _verify* from a callback returns MOCHI_EINVAL. */
int mochi_batcher_submit_request(mochi_batcher* b, const mochi_write2_request* req, mochi_verdict_cb cb, void* user);
/* Blocks until this message's verdict is in `out`.  Thread-safe.  Returns the
 * status of the batch call that carried it. */
int mochi_batcher_verify(mochi_batcher* b, const uint8_t* msg, uint32_t msg_len, const uint8_t* op_flags,
                         uint32_t n_ops, const uint8_t* expected_hash, mochi_verdict1* out);
/* Non-blocking form for an event-loop caller (e.g. a Netty handler completing a
 * future): enqueue one message and return; cb(user, rc, &verdict) runs on a
 * flusher thread once its batch is verified (rc = the batch call's status).
 * msg / op_flags / expected_hash must stay valid until the callback.  With
 * thousands of requests in flight the batches grow to max_msgs, so throughput
 * follows the bulk wire path instead of 1 / latency per blocked thread. */
int mochi_batcher_submit(mochi_batcher* b, const uint8_t* msg, uint32_t msg_len, const uint8_t* op_flags,
                         uint32_t n_ops, const uint8_t* expected_hash, mochi_verdict_cb cb, void* user);
int mochi_batcher_stats(mochi_batcher* b, uint64_t* batches, uint64_t* msgs);
/* Drains pending requests, then stops the flushers and frees the batcher once
 * every blocked caller has returned.  From one of the batcher's own callbacks
 * the teardown is deferred instead: later submissions are refused with
 * MOCHI_EINVAL, requests already queued still complete, and the last flusher
 * frees the batcher; the handle must not be used after the call either way.
 * The batcher holds its contexts until it is freed: mochi_ctx_destroy on one of
 * them while a batcher still holds it returns at once and the context is freed
 * by the batcher's release (never while a flusher still uses it), so a caller
 * that tears down right after its last callback -- or closes the context before
 * the batcher -- neither blocks nor frees a context in use.  A process that
 * exits without destroying the contexts must not exit from a callback. */
void mochi_batcher_destroy(mochi_batcher* b);

/* ------------------------------------------------------------------------
 * Cluster configuration (ABI 3): the reference's properties file
 * (ClusterConfiguration.loadInitialConfigurationFromProperties,
 * ClusterConfiguration.java:138-187; config/sample_config): _CONFIG_SERVERS,
 * _CONFIG_BFT_REPLICATION, _CONFIG_SERVER_<id>_URL, _CONFIG_SERVER_<id>_TOKENS.
 * Host only.  Errors (MOCHI_EINVAL + mochi_last_error()) where the reference
 * throws: a server without URL, a token >= 1024 or mapped twice, a token left
 * unassigned, no replication factor, R < 4 or R > the token owners (:182-184).
 * ------------------------------------------------------------------------ */
typedef struct mochi_config mochi_config;
mochi_config* mochi_config_load(const char* path);
/* The same from the properties text itself. */
mochi_config* mochi_config_parse(const char* text, uint64_t len);
void mochi_config_free(mochi_config* c);
/* R (_CONFIG_BFT_REPLICATION) and M = getServerMajority() = 2*(R/3)+1. */
uint32_t mochi_config_replication(const mochi_config* c);
uint32_t mochi_config_majority(const mochi_config* c);
/* Servers in _CONFIG_SERVERS order: id and URL (NUL-terminated, owned by c). */
uint32_t mochi_config_n_servers(const mochi_config* c);
const char* mochi_config_server_id(const mochi_config* c, uint32_t i);
const char* mochi_config_server_url(const mochi_config* c, uint32_t i);
/* getServersForObject(key) (ClusterConfiguration.java:194-226): R indices into
 * the server table, in replica order.  Faithful to the reference, whose loop
 * reads token i instead of ithTokenValue (:215), so every key maps to the
 * owners of tokens 0..R-1; key = UTF-8 bytes (hashed as Java String.hashCode). */
int mochi_config_servers_for_key(const mochi_config* c, const uint8_t* key, uint32_t key_len, uint32_t* idx_out);
/* Server-id table of the replica set of `key` (or of tokens 0..R-1 for key =
 * NULL), laid out for mochi_ctx_set_server_ids: ids_out = the ids back to back,
 * id_off[R+1].  ids_cap = capacity of ids_out; returns the bytes needed (or
 * < 0 on error), writing nothing beyond ids_cap. */
int64_t mochi_config_replica_ids(const mochi_config* c, const uint8_t* key, uint32_t key_len, uint8_t* ids_out,
                                 uint64_t ids_cap, uint32_t* id_off);

/* ------------------------------------------------------------------------
 * Multi-GPU: certificates are independent, so a batch is cut
 * into contiguous certificate ranges, one per GPU, every boundary a multiple of
 * 32 certificates (the per-GPU accept bitmaps then concatenate word by word).
 * The only collective is one RCCL all-gather of those bitmaps over xGMI, after
 * which every GPU holds the whole batch's verdict bitmap.
 * ------------------------------------------------------------------------ */

/* Shard plan: cert_lo[n_shards+1], shard s = [cert_lo[s], cert_lo[s+1]), every
 * inner boundary a multiple of 32, the shards' work as even as that allows
 * (work = grants via cert_grant_off[C+1]; NULL = certificates).  Host only. */
int mochi_shard_plan(uint32_t n_certs, const uint32_t* cert_grant_off, uint32_t n_shards, uint32_t* cert_lo);
/* Words per shard slot of the all-gather (max over shards of ceil(size/32)). */
uint32_t mochi_shard_words(uint32_t n_shards, const uint32_t* cert_lo);
/* The batch's accept bitmap from an all-gathered buffer of n_shards slots of
 * words_per_shard words (slot s = shard s's bitmap, zero-padded). */
int mochi_bits_assemble(uint32_t n_shards, const uint32_t* cert_lo, uint32_t words_per_shard, const uint32_t* gathered,
                        uint32_t* bits_out);

/* One process owning several GPUs (e.g. one JVM server on an 8-GPU node):
 * bit i of device_mask = HIP device i; one context per device, each driven by
 * its own host thread, and an RCCL communicator over them (ncclCommInitAll). */
typedef struct mochi_mctx mochi_mctx;
mochi_mctx* mochi_mctx_create(uint64_t device_mask, const uint8_t* moduli_be, uint32_t n_keys, uint32_t key_bytes,
                              uint32_t public_exponent);
void mochi_mctx_destroy(mochi_mctx* m);
/* Device ids of the context (returns their count). */
int mochi_mctx_devices(mochi_mctx* m, int* devices, int max);
/* The per-device context i (profiling, chunk size, ...); owned by m. */
mochi_ctx* mochi_mctx_context(mochi_mctx* m, int i);
int mochi_mctx_set_server_ids(mochi_mctx* m, const uint8_t* ids, const uint32_t* id_off, uint32_t n_ids);
/* Host batch across the devices: each device runs mochi_verify_batch on its
 * shard (outputs land in their slices of `out`; grant_valid_bits is not
 * supported here, use grant_flags), then each device's accept bitmap is
 * all-gathered from where the verify left it in device memory (no host
 * round trip) and out->cert_accept_bits is assembled from one copy of device
 * 0's gathered buffer.  The per-device contexts must not be used by other
 * threads during the call. */
int mochi_mverify_batch(mochi_mctx* m, const mochi_batch* batch, const mochi_params* params, mochi_verdicts* out);
/* Write2ToServer messages across the devices (shards by wire bytes); as
 * mochi_verify_write2, the grant-level outputs must be NULL (MOCHI_EINVAL). */
int mochi_mverify_write2(mochi_mctx* m, const mochi_write2_batch* batch, const mochi_params* params,
                         mochi_verdicts* out, uint8_t* msg_status);
/* After a call: device i's all-gathered buffer (n_devices slots of
 * words_per_device words, device memory of device i). */
int mochi_mctx_gathered_bits(mochi_mctx* m, int i, const uint32_t** d_bits, uint32_t* words_per_device);

/* One process per GPU (torchrun / MPI style).  Rank 0 makes the 128-byte id,
 * the caller moves it to every rank by any transport, each rank joins. */
#define MOCHI_COMM_ID_BYTES 128
typedef struct mochi_comm mochi_comm;
int mochi_comm_unique_id(uint8_t* id_out /* [128] */);
mochi_comm* mochi_comm_init(const uint8_t* id /* [128] */, int n_ranks, int rank, int device);
/* ncclAllGather of words_per_rank uint32 per rank: d_recv[n_ranks * words_per_rank]
 * (d_send may be d_recv + rank * words_per_rank), async on `stream`. */
int mochi_comm_allgather_bits(mochi_comm* c, const uint32_t* d_send, uint32_t words_per_rank, uint32_t* d_recv,
                              void* stream);
void mochi_comm_destroy(mochi_comm* c);

/* Test hook (host only, no GPU): the per-device protocol mochi_mverify_* use
 * around the all-gather (multi.cpp run_gather), with n simulated devices whose
 * device selection / slot fill / collective enqueue fail per bit of the masks
 * and whose collective is a host rendezvous of all n.  Returns the protocol's
 * status; *entered_collective = devices that enqueued, *timed_out = devices that
 * waited `timeout_ms` for a peer that never came (the hang the protocol must
 * rule out: always 0). */
int mochi_test_gather_protocol(uint32_t n, uint32_t fail_select, uint32_t fail_fill, uint32_t fail_enqueue,
                               uint32_t timeout_ms, uint32_t* entered_collective, uint32_t* timed_out);

#ifdef __cplusplus
}
#endif

#endif /* MOCHI_HIP_H */
