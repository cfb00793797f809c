"""ctypes binding for libmochi_hip (include/mochi_hip.h).

The host-side mirror of the reference's Write2 verification interface for
tests, the benchmark and Python callers.  The product path is the HIP
library; this module never falls back to a CPU implementation: if the shared
library is missing or no gfx950 device is visible, constructing a Verifier
raises.

Reference interface mirrored (tomisetsu/mochi-db):
  DataStore.processWrite2ToServer(Write2ToServer) -> Object
      server/datastrore/DataStore.java:12, InMemoryDataStore.java:641-666
  MochiDBClient read / Write2 aggregation
      client/MochiDBClient.java:148-175, 355-382
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MOCHI_HIP_LIB: an alternative build of the same library (A/B measurements)
LIB_PATH = os.environ.get("MOCHI_HIP_LIB") or os.path.join(_HERE, "libmochi_hip.so")

RSA_BYTES = 256
RSA_E = 65537
TXN_HASH_BYTES = 128
MAX_OPS_PER_CERT = 64

# status codes
OK, EINVAL, EHIP, ENOMEM, ENODEV = 0, -1, -2, -3, -4

# reason codes (enum mochi_reason)
ACCEPT = 0
REJECT_TS_MISMATCH = 1
REJECT_NO_GRANT = 2
REJECT_BELOW_QUORUM = 3
REJECT_HASH_MISMATCH = 4
REJECT_NO_SVOC = 5
REJECT_MALFORMED = 6
REJECT_APPLY_STATE = 8
REJECT_STORED_CERT = 9
REJECT_NOT_WRITE = 10
REASON_NAMES = {
    ACCEPT: "ACCEPT",
    REJECT_TS_MISMATCH: "TS_MISMATCH",
    REJECT_NO_GRANT: "NO_GRANT",
    REJECT_BELOW_QUORUM: "BELOW_QUORUM",
    REJECT_HASH_MISMATCH: "HASH_MISMATCH",
    REJECT_NO_SVOC: "NO_SVOC",
    REJECT_MALFORMED: "MALFORMED",
    REJECT_APPLY_STATE: "APPLY_STATE",
    REJECT_STORED_CERT: "STORED_CERT",
    REJECT_NOT_WRITE: "NOT_WRITE",
}

OP_LOCAL = 0x01
OP_HAS_SVOC = 0x02
OP_HAS_CURRENT_C = 0x04
OP_CURRENT_C_BAD = 0x08
OP_NOT_WRITE = 0x10

# per-op decisions (enum mochi_op_decision)
OPD_SKIPPED, OPD_APPLY, OPD_READ, OPD_WRONG_SHARD, OPD_FAILED = 0, 1, 2, 3, 4

# mochi_params.quorum_mode bits
Q_DISTINCT_SIGNERS = 0x1
Q_BIND = 0x2
GRANT_SIG_OK = 0x01
GRANT_PARSED = 0x02


class MochiError(RuntimeError):
    pass


class Batch_C(ctypes.Structure):
    _fields_ = [
        ("n_grants", ctypes.c_uint32),
        ("n_certs", ctypes.c_uint32),
        ("n_ops", ctypes.c_uint32),
        ("n_mgs", ctypes.c_uint32),
        ("grant_bytes_len", ctypes.c_uint64),
        ("grant_bytes", ctypes.c_void_p),
        ("grant_off", ctypes.c_void_p),
        ("grant_len", ctypes.c_void_p),
        ("sig", ctypes.c_void_p),
        ("signer", ctypes.c_void_p),
        ("grant_key", ctypes.c_void_p),
        ("cert_grant_off", ctypes.c_void_p),
        ("cert_op_off", ctypes.c_void_p),
        ("op_key", ctypes.c_void_p),
        ("op_flags", ctypes.c_void_p),
        ("expected_hash", ctypes.c_void_p),
        ("cert_mg_off", ctypes.c_void_p),
        ("mg_grant_off", ctypes.c_void_p),
        ("op_object_ts", ctypes.c_void_p),
        ("op_key_off", ctypes.c_void_p),
        ("op_key_len", ctypes.c_void_p),
    ]


class Params_C(ctypes.Structure):
    _fields_ = [
        ("replication_factor", ctypes.c_uint32),
        ("strict_gt", ctypes.c_uint32),
        ("quorum_mode", ctypes.c_uint32),
        ("_pad", ctypes.c_uint32),
    ]


def params(replication_factor: int, strict_gt: bool = True, quorum_mode: int = 0) -> "Params_C":
    return Params_C(replication_factor=replication_factor, strict_gt=1 if strict_gt else 0, quorum_mode=quorum_mode)


class Verdicts_C(ctypes.Structure):
    _fields_ = [
        ("grant_valid_bits", ctypes.c_void_p),
        ("grant_flags", ctypes.c_void_p),
        ("grant_ts", ctypes.c_void_p),
        ("cert_accept_bits", ctypes.c_void_p),
        ("cert_reason", ctypes.c_void_p),
        ("cert_fail_op", ctypes.c_void_p),
        ("op_decision", ctypes.c_void_p),
        ("op_g0", ctypes.c_void_p),
        ("op_ts", ctypes.c_void_p),
    ]


_lib = None
ABI_VERSION = 3


def load_library(path: str = LIB_PATH) -> ctypes.CDLL:
    """Load libmochi_hip.so (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise MochiError(f"{path} not built: run `make -C mochi-db_amd` (or __graft_entry__.build())")
    # One HIP runtime per process: when PyTorch-ROCm is present, load it first so
    # that libmochi_hip's libamdhip64.so.7 dependency resolves (by SONAME) to the
    # runtime torch already mapped; device pointers and hipStream_t handles can
    # then cross the boundary.  Loading ours first would make torch map a second
    # runtime, which then sees no GPU.
    try:
        import torch  # noqa: F401  (plumbing only)
    except Exception:
        pass
    lib = ctypes.CDLL(path)
    vp, u32, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32
    lib.mochi_abi_version.restype = ctypes.c_int
    lib.mochi_last_error.restype = ctypes.c_char_p
    lib.mochi_device_count.restype = ctypes.c_int
    lib.mochi_ctx_create.restype = vp
    lib.mochi_ctx_create.argtypes = [ctypes.c_int, vp, u32, u32, u32]
    lib.mochi_ctx_destroy.argtypes = [vp]
    lib.mochi_verify_batch.argtypes = [vp, ctypes.POINTER(Batch_C), ctypes.POINTER(Params_C), ctypes.POINTER(Verdicts_C)]
    lib.mochi_verify_batch_device.argtypes = [vp, ctypes.POINTER(Batch_C), ctypes.POINTER(Params_C),
                                              ctypes.POINTER(Verdicts_C), vp]
    lib.mochi_ctx_last_timing.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float),
                                          ctypes.POINTER(ctypes.c_float)]
    lib.mochi_sign_grants.argtypes = [ctypes.c_char_p, u32, vp, vp, vp, vp, ctypes.c_int]
    lib.mochi_pem_modulus.argtypes = [ctypes.c_char_p, vp]
    lib.mochi_rsa_public_op.argtypes = [vp, u32, vp, vp, vp, vp]
    lib.mochi_fold_matrix.argtypes = [vp, vp, vp]
    lib.mochi_ctx_set_profiling.argtypes = [vp, ctypes.c_int]
    lib.mochi_ctx_read_profile.argtypes = [vp, vp, u32, vp]
    lib.mochi_tally_responses.argtypes = [u32, vp, vp, vp, vp, vp, vp, u32, vp, vp, vp]
    lib.mochi_write1_classify.argtypes = [u32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.mochi_tally_responses_device.argtypes = [u32, vp, vp, vp, vp, vp, vp, u32, vp, vp, vp, vp]
    lib.mochi_write1_classify_device.argtypes = [u32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.mochi_ctx_last_total_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
    lib.mochi_ctx_set_chunk_grants.argtypes = [vp, u32]
    lib.mochi_ctx_set_small_batch.argtypes = [vp, u32]
    lib.mochi_ctx_set_server_ids.argtypes = [vp, vp, vp, u32]
    lib.mochi_verify_write2.argtypes = [vp, vp, vp, vp, vp]
    lib.mochi_verify_write2_device.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.mochi_write2_decode.argtypes = [vp, vp, vp]
    lib.mochi_write2_decoded_free.argtypes = [vp]
    lib.mochi_write2_decode_same.argtypes = [vp, vp, vp, vp]
    lib.mochi_write2_same_free.argtypes = [vp]
    lib.mochi_write2_same_free.restype = None
    lib.mochi_write2_encode_bound.restype = ctypes.c_uint64
    lib.mochi_write2_encode_bound.argtypes = [vp, u32]
    lib.mochi_write2_encode.argtypes = [vp, vp, vp, u32, vp, ctypes.c_uint64, vp, vp, vp, vp]
    lib.mochi_write2_encode_device.argtypes = [vp, vp, vp, ctypes.c_uint64, vp, vp, vp, vp, vp]
    lib.mochi_ctx_read_encode_profile.argtypes = [vp, vp, u32]
    lib.mochi_signer_create.restype = vp
    lib.mochi_signer_create.argtypes = [ctypes.c_int, ctypes.c_char_p]
    lib.mochi_signer_destroy.argtypes = [vp]
    lib.mochi_sign_batch.argtypes = [vp, vp, ctypes.c_uint64, vp, vp, u32, vp]
    lib.mochi_sign_batch_device.argtypes = [vp, vp, vp, vp, u32, vp, vp]
    lib.mochi_signer_rejected.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    lib.mochi_signer_set_fault.argtypes = [vp, u32]
    lib.mochi_write1_issue_bound.restype = ctypes.c_uint64
    lib.mochi_write1_issue_bound.argtypes = [vp]
    lib.mochi_write1_issue.argtypes = [vp, vp, vp]
    lib.mochi_write1_issue_device.argtypes = [vp, vp, vp, vp]
    lib.mochi_signer_set_profiling.argtypes = [vp, ctypes.c_int]
    lib.mochi_signer_read_issue_profile.argtypes = [vp, vp, u32]
    u64 = ctypes.c_uint64
    lib.mochi_write1_reply_bound.restype = u64
    lib.mochi_write1_reply_bound.argtypes = [u32, u32, u64, u64, u64, u64, u64, ctypes.c_int]
    lib.mochi_write1_reply_encode.argtypes = [vp, vp, vp, vp, u64, vp, vp, vp, vp]
    lib.mochi_write1_reply_encode_device.argtypes = [vp, vp, vp, vp, vp, u64, vp, vp, vp, vp, vp, vp]
    lib.mochi_signer_read_reply_profile.argtypes = [vp, vp, u32]
    lib.mochi_write1_reply_decode_bound.restype = None
    lib.mochi_write1_reply_decode_bound.argtypes = [u64, u32, vp, vp]
    lib.mochi_write1_reply_decode.argtypes = [vp, vp, vp, u32, vp]
    lib.mochi_write1_reply_decode_device.argtypes = [vp, vp, vp, vp]
    lib.mochi_ctx_read_w1_decode_profile.argtypes = [vp, vp, u32]
    lib.mochi_write1_request_decode_bound.restype = u64
    lib.mochi_write1_request_decode_bound.argtypes = [u64, u32]
    lib.mochi_write1_request_decode.argtypes = [vp, vp]
    lib.mochi_write1_request_decode_device.argtypes = [vp, vp, vp, vp, vp]
    lib.mochi_signer_read_request_profile.argtypes = [vp, vp, u32]
    lib.mochi_write1_state_join.argtypes = [u32, u32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.mochi_write1_state_join_device.argtypes = [vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.mochi_result_reply_decode.argtypes = [vp, vp]
    lib.mochi_result_reply_decode_device.argtypes = [vp, vp, vp, vp]
    lib.mochi_ctx_read_result_decode_profile.argtypes = [vp, vp, u32]
    lib.mochi_result_coalesce.argtypes = [vp, vp]
    lib.mochi_result_coalesce_device.argtypes = [vp, vp, vp]
    lib.mochi_result_reply_encode_bound.restype = u64
    lib.mochi_result_reply_encode_bound.argtypes = [u32, u64, u64, u64, u64]
    lib.mochi_result_reply_encode.argtypes = [vp, vp, u64, vp, vp, vp, vp]
    lib.mochi_result_reply_encode_device.argtypes = [vp, vp, vp, u64, vp, vp, vp, vp, vp, vp]
    lib.mochi_ctx_read_result_encode_profile.argtypes = [vp, vp, u32]
    lib.mochi_write2_answer_plan.argtypes = [vp, vp, vp]
    lib.mochi_write2_answer_plan_device.argtypes = [vp, vp, vp, vp]
    lib.mochi_read_request_decode_bound.restype = u64
    lib.mochi_read_request_decode_bound.argtypes = [u64, u32]
    lib.mochi_read_request_decode.argtypes = [vp, vp]
    lib.mochi_read_request_decode_device.argtypes = [vp, vp, vp, vp, vp]
    lib.mochi_ctx_read_read_decode_profile.argtypes = [vp, vp, u32]
    lib.mochi_read_answer_plan.argtypes = [u32, vp, vp, vp]
    lib.mochi_read_answer_plan_device.argtypes = [u32, vp, vp, vp, vp]
    lib.mochi_envelope_decode.argtypes = [vp, vp]
    lib.mochi_envelope_decode_device.argtypes = [vp, vp, vp, vp]
    lib.mochi_envelope_route.argtypes = [u32, vp, vp, vp, vp, vp]
    lib.mochi_envelope_route_device.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp]
    lib.mochi_envelope_join.argtypes = [vp, vp, vp, vp, vp]
    lib.mochi_envelope_join_device.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    lib.mochi_envelope_encode_bound.restype = u64
    lib.mochi_envelope_encode_bound.argtypes = [u32, u64, u64]
    lib.mochi_envelope_encode.argtypes = [vp, vp, u64, vp, vp, vp, vp]
    lib.mochi_envelope_encode_device.argtypes = [vp, vp, vp, u64, vp, vp, vp, vp, vp, vp]
    lib.mochi_ctx_read_envelope_profile.argtypes = [vp, ctypes.c_int, vp, u32]
    lib.mochi_batcher_create.restype = vp
    lib.mochi_batcher_create.argtypes = [vp, vp, u32, u32, ctypes.c_int]
    lib.mochi_batcher_create_multi.restype = vp
    lib.mochi_batcher_create_multi.argtypes = [vp, u32, vp, u32, u32, ctypes.c_int]
    lib.mochi_batcher_verify.argtypes = [vp, vp, u32, vp, u32, vp, vp]
    lib.mochi_batcher_submit.argtypes = [vp, vp, u32, vp, u32, vp, VERDICT_CB, vp]
    lib.mochi_batcher_stats.argtypes = [vp, vp, vp]
    lib.mochi_batcher_destroy.argtypes = [vp]
    lib.mochi_shard_plan.argtypes = [u32, vp, u32, vp]
    lib.mochi_shard_words.restype = u32
    lib.mochi_shard_words.argtypes = [u32, vp]
    lib.mochi_bits_assemble.argtypes = [u32, vp, u32, vp, vp]
    lib.mochi_mctx_create.restype = vp
    lib.mochi_mctx_create.argtypes = [ctypes.c_uint64, vp, u32, u32, u32]
    lib.mochi_mctx_destroy.argtypes = [vp]
    lib.mochi_mctx_devices.argtypes = [vp, vp, ctypes.c_int]
    lib.mochi_mctx_context.restype = vp
    lib.mochi_mctx_context.argtypes = [vp, ctypes.c_int]
    lib.mochi_mctx_set_server_ids.argtypes = [vp, vp, vp, u32]
    lib.mochi_mverify_batch.argtypes = [vp, vp, vp, vp]
    lib.mochi_mverify_write2.argtypes = [vp, vp, vp, vp, vp]
    lib.mochi_mctx_gathered_bits.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
                                             ctypes.POINTER(ctypes.c_uint32)]
    lib.mochi_comm_unique_id.argtypes = [vp]
    lib.mochi_comm_init.restype = vp
    lib.mochi_comm_init.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.mochi_comm_allgather_bits.argtypes = [vp, vp, u32, vp, vp]
    lib.mochi_comm_destroy.argtypes = [vp]
    lib.mochi_test_gather_protocol.argtypes = [u32, u32, u32, u32, u32, ctypes.POINTER(u32), ctypes.POINTER(u32)]
    lib.mochi_host_alloc.restype = vp
    lib.mochi_host_alloc.argtypes = [ctypes.c_uint64]
    lib.mochi_host_free.argtypes = [vp]
    # ABI 3: per-request batcher calls with stored state + per-op outputs; cluster config
    lib.mochi_batcher_verify_request.argtypes = [vp, ctypes.POINTER(Write2Request_C), ctypes.POINTER(Verdict1_C)]
    lib.mochi_batcher_submit_request.argtypes = [vp, ctypes.POINTER(Write2Request_C), VERDICT_CB, vp]
    lib.mochi_config_load.restype = vp
    lib.mochi_config_load.argtypes = [ctypes.c_char_p]
    lib.mochi_config_parse.restype = vp
    lib.mochi_config_parse.argtypes = [ctypes.c_char_p, ctypes.c_uint64]
    lib.mochi_config_free.argtypes = [vp]
    lib.mochi_config_replication.restype = u32
    lib.mochi_config_replication.argtypes = [vp]
    lib.mochi_config_majority.restype = u32
    lib.mochi_config_majority.argtypes = [vp]
    lib.mochi_config_n_servers.restype = u32
    lib.mochi_config_n_servers.argtypes = [vp]
    lib.mochi_config_server_id.restype = ctypes.c_char_p
    lib.mochi_config_server_id.argtypes = [vp, u32]
    lib.mochi_config_server_url.restype = ctypes.c_char_p
    lib.mochi_config_server_url.argtypes = [vp, u32]
    lib.mochi_config_servers_for_key.argtypes = [vp, vp, u32, vp]
    lib.mochi_config_replica_ids.restype = ctypes.c_int64
    lib.mochi_config_replica_ids.argtypes = [vp, vp, u32, vp, ctypes.c_uint64, vp]
    if lib.mochi_abi_version() != ABI_VERSION:
        raise MochiError("libmochi_hip ABI mismatch")
    _lib = lib
    return lib


def _ptr(a: Optional[np.ndarray]) -> Optional[int]:
    if a is None:
        return None
    if not a.flags["C_CONTIGUOUS"]:
        raise ValueError("arrays must be C-contiguous")
    return a.ctypes.data


def _err(lib) -> str:
    return (lib.mochi_last_error() or b"").decode(errors="replace")


@dataclass
class Batch:
    """A batch of Write2 certificates, struct-of-arrays (see mochi_batch)."""

    grant_bytes: np.ndarray  # uint8 blob
    grant_off: np.ndarray  # uint64 [N]
    grant_len: np.ndarray  # uint32 [N]
    sig: np.ndarray  # uint8 [N, 256]
    signer: np.ndarray  # uint16 [N]
    grant_key: np.ndarray  # uint8 [N]
    cert_grant_off: np.ndarray  # uint32 [C+1]
    cert_op_off: np.ndarray  # uint32 [C+1]
    op_key: np.ndarray  # uint8 [O]
    op_flags: np.ndarray  # uint8 [O]
    expected_hash: np.ndarray  # uint8 [C, 128]
    # ABI 2 (optional): MultiGrant CSR, stored-certificate timestamps, op key slices
    cert_mg_off: Optional[np.ndarray] = None  # uint32 [C+1]
    mg_grant_off: Optional[np.ndarray] = None  # uint32 [n_mgs+1]
    op_object_ts: Optional[np.ndarray] = None  # int64 [O]
    op_key_off: Optional[np.ndarray] = None  # uint64 [O] into grant_bytes
    op_key_len: Optional[np.ndarray] = None  # uint32 [O]

    OPTIONAL = ("cert_mg_off", "mg_grant_off", "op_object_ts", "op_key_off", "op_key_len")
    OPT_DTYPES = {"cert_mg_off": np.uint32, "mg_grant_off": np.uint32, "op_object_ts": np.int64,
                  "op_key_off": np.uint64, "op_key_len": np.uint32}
    FIELDS = ("grant_bytes", "grant_off", "grant_len", "sig", "signer", "grant_key", "cert_grant_off",
              "cert_op_off", "op_key", "op_flags", "expected_hash")

    @property
    def n_mgs(self) -> int:
        return 0 if self.mg_grant_off is None else int(self.mg_grant_off.shape[0]) - 1

    @property
    def n_grants(self) -> int:
        return int(self.grant_off.shape[0])

    @property
    def n_certs(self) -> int:
        return int(self.cert_grant_off.shape[0]) - 1

    @property
    def n_ops(self) -> int:
        return int(self.op_key.shape[0])

    def normalized(self) -> "Batch":
        return Batch(
            grant_bytes=np.ascontiguousarray(self.grant_bytes, dtype=np.uint8),
            grant_off=np.ascontiguousarray(self.grant_off, dtype=np.uint64),
            grant_len=np.ascontiguousarray(self.grant_len, dtype=np.uint32),
            sig=np.ascontiguousarray(self.sig, dtype=np.uint8).reshape(-1, RSA_BYTES),
            signer=np.ascontiguousarray(self.signer, dtype=np.uint16),
            grant_key=np.ascontiguousarray(self.grant_key, dtype=np.uint8),
            cert_grant_off=np.ascontiguousarray(self.cert_grant_off, dtype=np.uint32),
            cert_op_off=np.ascontiguousarray(self.cert_op_off, dtype=np.uint32),
            op_key=np.ascontiguousarray(self.op_key, dtype=np.uint8),
            op_flags=np.ascontiguousarray(self.op_flags, dtype=np.uint8),
            expected_hash=np.ascontiguousarray(self.expected_hash, dtype=np.uint8).reshape(-1, TXN_HASH_BYTES),
            **{k: (None if getattr(self, k) is None else np.ascontiguousarray(getattr(self, k), dtype=self.OPT_DTYPES[k]))
               for k in self.OPTIONAL},
        )

    def pinned(self) -> "Batch":
        """A copy whose arrays live in one pinned host allocation (mochi_host_alloc):
        mochi_verify_batch DMAs such arrays in place instead of staging them."""
        b = self.normalized()
        names = self.FIELDS + tuple(k for k in self.OPTIONAL if getattr(b, k) is not None)
        arrs = [getattr(b, nm) for nm in names]
        offs, total = [], 0
        for a in arrs:
            offs.append(total)
            total = (total + a.nbytes + 255) // 256 * 256
        buf = PinnedHost(total)
        out = {}
        for nm, a, o in zip(names, arrs, offs):
            v = np.frombuffer(buf.view()[o:o + a.nbytes], dtype=a.dtype).reshape(a.shape)
            v[...] = a
            out[nm] = v
        pb = Batch(**out)
        pb._pinned = buf  # keep the allocation alive with the views
        return pb

    def to_c(self) -> Batch_C:
        b = Batch_C()
        b.n_grants, b.n_certs, b.n_ops = self.n_grants, self.n_certs, self.n_ops
        b.grant_bytes_len = int(self.grant_bytes.nbytes)
        b.grant_bytes = _ptr(self.grant_bytes)
        b.grant_off = _ptr(self.grant_off)
        b.grant_len = _ptr(self.grant_len)
        b.sig = _ptr(self.sig)
        b.signer = _ptr(self.signer)
        b.grant_key = _ptr(self.grant_key)
        b.cert_grant_off = _ptr(self.cert_grant_off)
        b.cert_op_off = _ptr(self.cert_op_off)
        b.op_key = _ptr(self.op_key)
        b.op_flags = _ptr(self.op_flags)
        b.expected_hash = _ptr(self.expected_hash)
        b.n_mgs = self.n_mgs
        for k in self.OPTIONAL:
            setattr(b, k, _ptr(getattr(self, k)))
        return b


class PinnedHost:
    """Pinned host allocation from libmochi_hip (mochi_host_alloc / mochi_host_free)."""

    def __init__(self, nbytes: int):
        self.lib = load_library()
        self.nbytes = max(int(nbytes), 1)
        self.ptr = self.lib.mochi_host_alloc(self.nbytes)
        if not self.ptr:
            raise MochiError(f"mochi_host_alloc: {_err(self.lib)}")

    def view(self) -> np.ndarray:
        return np.ctypeslib.as_array((ctypes.c_uint8 * self.nbytes).from_address(self.ptr))

    def __del__(self):  # pragma: no cover
        if getattr(self, "ptr", None):
            self.lib.mochi_host_free(self.ptr)
            self.ptr = None


@dataclass
class Verdicts:
    grant_valid_bits: np.ndarray
    grant_flags: np.ndarray
    grant_ts: np.ndarray
    cert_accept_bits: np.ndarray
    cert_reason: np.ndarray
    cert_fail_op: np.ndarray
    op_decision: Optional[np.ndarray] = None  # uint8 [O]
    op_g0: Optional[np.ndarray] = None  # uint32 [O]
    op_ts: Optional[np.ndarray] = None  # int64 [O]
    timing_ms: dict = field(default_factory=dict)

    @staticmethod
    def alloc(n_grants: int, n_certs: int, n_ops: int = 0) -> "Verdicts":
        return Verdicts(
            grant_valid_bits=np.zeros((n_grants + 31) // 32, np.uint32),
            grant_flags=np.zeros(n_grants, np.uint8),
            grant_ts=np.zeros(n_grants, np.int64),
            cert_accept_bits=np.zeros((n_certs + 31) // 32, np.uint32),
            cert_reason=np.zeros(n_certs, np.uint8),
            cert_fail_op=np.zeros(n_certs, np.uint8),
            op_decision=np.full(n_ops, 0xEE, np.uint8),
            op_g0=np.zeros(n_ops, np.uint32),
            op_ts=np.zeros(n_ops, np.int64),
        )

    def to_c(self) -> Verdicts_C:
        v = Verdicts_C()
        v.grant_valid_bits = _ptr(self.grant_valid_bits)
        v.grant_flags = _ptr(self.grant_flags)
        v.grant_ts = _ptr(self.grant_ts)
        v.cert_accept_bits = _ptr(self.cert_accept_bits)
        v.cert_reason = _ptr(self.cert_reason)
        v.cert_fail_op = _ptr(self.cert_fail_op)
        # zero-length op arrays still get a pointer (n_ops == 0 reads nothing)
        v.op_decision = _ptr(self.op_decision)
        v.op_g0 = _ptr(self.op_g0)
        v.op_ts = _ptr(self.op_ts)
        return v

    @property
    def grant_valid(self) -> np.ndarray:
        return unpack_bits(self.grant_valid_bits, self.grant_flags.shape[0])

    @property
    def cert_accept(self) -> np.ndarray:
        return unpack_bits(self.cert_accept_bits, self.cert_reason.shape[0])


def unpack_bits(words: np.ndarray, n: int) -> np.ndarray:
    """uint32 little-endian bitmap -> bool[n] (bit i of word i//32)."""
    b = np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little")
    return b[:n].astype(bool)


def majority(replication_factor: int) -> int:
    """ClusterConfiguration.getServerMajority (ClusterConfiguration.java:264-267)."""
    return 2 * (replication_factor // 3) + 1


class Verifier:
    """A libmochi_hip context: one device, one RSA public-key table.

    Key index i corresponds to the i-th server ID of the cluster (the
    MultiGrant.serverId that signed the grant).
    """

    def __init__(self, moduli_be: Sequence[bytes] | np.ndarray, device: int = 0):
        self.lib = load_library()
        mod = np.ascontiguousarray(
            np.frombuffer(b"".join(bytes(m) for m in moduli_be), np.uint8)
            if not isinstance(moduli_be, np.ndarray) else moduli_be.astype(np.uint8).reshape(-1)
        )
        if mod.size % RSA_BYTES:
            raise ValueError("moduli must be 256-byte big-endian values")
        self.n_keys = mod.size // RSA_BYTES
        self._moduli = mod
        self.ctx = self.lib.mochi_ctx_create(int(device), mod.ctypes.data, self.n_keys, RSA_BYTES, RSA_E)
        if not self.ctx:
            raise MochiError(f"mochi_ctx_create failed: {_err(self.lib)}")
        self.device = device

    def set_server_ids(self, server_ids) -> None:
        """Key i of the table belongs to MultiGrant.serverId == server_ids[i] (Write2 wire path)."""
        enc = [x.encode() if isinstance(x, str) else bytes(x) for x in server_ids]
        blob = np.frombuffer(b"".join(enc) or b"\x00", np.uint8).copy()
        off = np.zeros(len(enc) + 1, np.uint32)
        np.cumsum([len(x) for x in enc], out=off[1:])
        if self.lib.mochi_ctx_set_server_ids(self.ctx, _ptr(blob), _ptr(off), len(enc)) != OK:
            raise MochiError(f"mochi_ctx_set_server_ids: {_err(self.lib)}")

    def verify_write2(self, wb, replication_factor: int, strict_gt: bool = True, quorum_mode: int = 0):
        """Write2ToServer messages (workload.WireBatch, host memory) -> (Verdicts with
        certificate-level arrays -- and per-op arrays when wb.op_flags_off is set --,
        msg_status[M])."""
        wc, keep = write2_batch_c(wb)
        M = wb.n_msgs
        O = int(wb.op_flags_off[-1]) if wb.op_flags_off is not None else 0
        out = Verdicts.alloc(0, M, O)
        vc = out.to_c()
        vc.grant_valid_bits = vc.grant_flags = vc.grant_ts = None
        if wb.op_flags_off is None:
            vc.op_decision = vc.op_g0 = vc.op_ts = None
            out.op_decision = out.op_g0 = out.op_ts = None
        p = params(replication_factor, strict_gt, quorum_mode)
        st = np.zeros(max(M, 1), np.uint8)
        rc = self.lib.mochi_verify_write2(self.ctx, ctypes.addressof(wc), ctypes.addressof(p), ctypes.addressof(vc),
                                          _ptr(st))
        if rc != OK:
            raise MochiError(f"mochi_verify_write2 rc={rc}: {_err(self.lib)}")
        t = ctypes.c_float()
        self.lib.mochi_ctx_last_total_ms(self.ctx, ctypes.byref(t))
        out.timing_ms = {"total": t.value}
        return out, st[:M].copy()

    def verify_write2_device(self, dwb: "DeviceWireBatch", out: "DeviceVerdicts", replication_factor: int,
                             strict_gt: bool = True, stream: int = 0, quorum_mode: int = 0) -> None:
        """Device-resident Write2 wire messages -> certificate verdicts (async on `stream`,
        except for one wait on the decoded grant / op totals)."""
        wc = dwb.to_c()
        vc = out.to_c()
        vc.grant_valid_bits = vc.grant_flags = vc.grant_ts = None
        if dwb.op_flags_off is None:
            vc.op_decision = vc.op_g0 = vc.op_ts = None
        p = params(replication_factor, strict_gt, quorum_mode)
        rc = self.lib.mochi_verify_write2_device(self.ctx, ctypes.addressof(wc), ctypes.addressof(p),
                                                 ctypes.addressof(vc), dwb.status.data_ptr(), stream)
        if rc != OK:
            raise MochiError(f"mochi_verify_write2_device rc={rc}: {_err(self.lib)}")

    def encode_write2_device(self, dsrc: "DeviceWrite2Source", wire, msg_off, msg_len, status, stream: int = 0,
                             check: bool = True):
        """Device-resident certificate source -> Write2ToServer bodies in `wire` (torch
        uint8) with msg_off (int64) / msg_len (int32) / status (uint8) [M], all on the
        device (mochi_write2_encode_device).  Waits for the total size, then returns
        (rc, wire_len) with the emit kernels enqueued on `stream`.  rc is EINVAL with
        wire_len = the size needed when `wire` is too small (nothing written);
        check=True raises on any rc but OK."""
        sc = dsrc.to_c()
        n = ctypes.c_uint64(0)
        cap = int(wire.numel()) if wire is not None else 0
        rc = self.lib.mochi_write2_encode_device(self.ctx, ctypes.addressof(sc), wire.data_ptr() if cap else None, cap,
                                                 msg_off.data_ptr(), msg_len.data_ptr(), status.data_ptr(),
                                                 ctypes.addressof(n), stream or None)
        if check and rc != OK:
            raise MochiError(f"mochi_write2_encode_device rc={rc}: {_err(self.lib)}")
        return rc, int(n.value)

    ENCODE_KERNELS = ("k_enc_mg", "k_enc_msg", "scan", "k_enc_hdr_mg", "k_enc_hdr_msg", "k_enc_copy")

    def read_encode_profile(self) -> dict:
        """Per-kernel ms of the last encode_write2_device call made with set_profiling(True)."""
        ms = np.zeros(len(self.ENCODE_KERNELS), np.float32)
        if self.lib.mochi_ctx_read_encode_profile(self.ctx, _ptr(ms), ms.size) != OK:
            raise MochiError(f"mochi_ctx_read_encode_profile: {_err(self.lib)}")
        return dict(zip(self.ENCODE_KERNELS, (float(x) for x in ms)))

    def write1_reply_decode_device(self, dreplies: "DeviceWrite1Replies", out: "DeviceWrite1Decoded", stream: int = 0,
                                   check: bool = True) -> int:
        """mochi_write1_reply_decode_device: device-resident Write1 reply bodies -> the
        arrays of `out` (server ids from set_server_ids).  Waits for the two totals
        (out.n_grants / out.n_certs), then returns the rc with the emit kernels enqueued
        on `stream`: EINVAL when a capacity of `out` is too small (the counts needed are
        set, no per-grant or per-certificate array touched; raises then if `check`)."""
        r, o = dreplies.to_c(), out.to_c()
        rc = self.lib.mochi_write1_reply_decode_device(self.ctx, ctypes.addressof(r), ctypes.addressof(o), stream or None)
        out.n_grants, out.n_certs = int(o.n_grants), int(o.n_certs)
        short = rc == EINVAL and (out.n_grants > out.grant_cap or out.n_certs > out.cert_cap)
        if rc != OK and (check or not short):
            raise MochiError(f"mochi_write1_reply_decode_device rc={rc}: {_err(self.lib)}")
        return rc

    def read_w1_decode_profile(self) -> dict:
        """Per-kernel ms of the last write1_reply_decode_device call made with set_profiling(True)."""
        ms = np.zeros(len(W1_DECODE_STAGES), np.float32)
        if self.lib.mochi_ctx_read_w1_decode_profile(self.ctx, _ptr(ms), ms.size) != OK:
            raise MochiError(f"mochi_ctx_read_w1_decode_profile: {_err(self.lib)}")
        return dict(zip(W1_DECODE_STAGES, (float(x) for x in ms)))

    def result_reply_decode_device(self, dreplies: "DeviceResultReplies", out: "DeviceResultDecoded",
                                   stream: int = 0) -> None:
        """mochi_result_reply_decode_device: device-resident Write2 / read answer bodies -> the
        arrays of `out`.  Returns with everything enqueued on `stream`; it waits for nothing."""
        r, o = dreplies.to_c(), out.to_c()
        rc = self.lib.mochi_result_reply_decode_device(self.ctx, ctypes.addressof(r), ctypes.addressof(o), stream or None)
        if rc != OK:
            raise MochiError(f"mochi_result_reply_decode_device rc={rc}: {_err(self.lib)}")

    def read_result_decode_profile(self) -> dict:
        """Per-kernel ms of the last result_reply_decode_device call made with set_profiling(True)."""
        ms = np.zeros(len(RESULT_DECODE_STAGES), np.float32)
        if self.lib.mochi_ctx_read_result_decode_profile(self.ctx, _ptr(ms), ms.size) != OK:
            raise MochiError(f"mochi_ctx_read_result_decode_profile: {_err(self.lib)}")
        return dict(zip(RESULT_DECODE_STAGES, (float(x) for x in ms)))

    def result_reply_encode_device(self, danswers: "DeviceResultAnswers", wire, msg_off, msg_len, status,
                                   stream: int = 0, wire_len_dev=None, check: bool = True):
        """mochi_result_reply_encode_device: the Write2 / read answer bodies of `danswers` into
        the uint8 tensor `wire` (None = capacity 0), msg_off (int64) / msg_len (int32) / status
        (uint8) [P] on the device.  wire_len_dev None: the call waits for the total; returns
        (rc, total), rc EINVAL when the total exceeds the capacity (raises then if `check`).
        wire_len_dev an int64 tensor of one element: no host wait, the total goes there and
        nothing is written to `wire` when it exceeds the capacity; returns (rc, None)."""
        a = danswers.to_c()
        cap = 0 if wire is None else int(wire.numel())
        need = ctypes.c_uint64(0)
        rc = self.lib.mochi_result_reply_encode_device(
            self.ctx, ctypes.addressof(a), wire.data_ptr() if cap else None, cap, msg_off.data_ptr(),
            msg_len.data_ptr(), status.data_ptr(), ctypes.addressof(need) if wire_len_dev is None else None,
            None if wire_len_dev is None else wire_len_dev.data_ptr(), stream or None)
        short = wire_len_dev is None and rc == EINVAL and int(need.value) > cap
        if rc != OK and (check or not short):
            raise MochiError(f"mochi_result_reply_encode_device rc={rc}: {_err(self.lib)}")
        return rc, (int(need.value) if wire_len_dev is None else None)

    def read_result_encode_profile(self) -> dict:
        """Per-kernel ms of the last result_reply_encode_device call made with set_profiling(True)."""
        ms = np.zeros(len(RESULT_ENCODE_STAGES), np.float32)
        if self.lib.mochi_ctx_read_result_encode_profile(self.ctx, _ptr(ms), ms.size) != OK:
            raise MochiError(f"mochi_ctx_read_result_encode_profile: {_err(self.lib)}")
        return dict(zip(RESULT_ENCODE_STAGES, (float(x) for x in ms)))

    def read_request_decode_device(self, dreqs: "DeviceReadRequests", out: "DeviceReadRequestsDecoded", stream: int = 0,
                                   check: bool = True) -> int:
        """mochi_read_request_decode_device: ReadToServer bodies in device memory to SoA arrays
        with their key numbering, in device memory.  Sets out.n_ops (the key count goes to the
        device word out.n_keys_dev); returns the rc, EINVAL when out.op_cap is too small
        (raises then if `check`)."""
        r, o = dreqs.to_c(), out.to_c()
        rc = self.lib.mochi_read_request_decode_device(self.ctx, ctypes.addressof(r), ctypes.addressof(o),
                                                       out.n_keys_dev.data_ptr(), stream or None)
        out.n_ops = int(o.n_ops)
        short = rc == EINVAL and out.n_ops > out.op_cap
        if rc != OK and (check or not short):
            raise MochiError(f"mochi_read_request_decode_device rc={rc}: {_err(self.lib)}")
        return rc

    def read_read_decode_profile(self) -> dict:
        """Per-kernel ms of the last read_request_decode_device call made with set_profiling(True)."""
        ms = np.zeros(len(READ_REQUEST_STAGES), np.float32)
        if self.lib.mochi_ctx_read_read_decode_profile(self.ctx, _ptr(ms), ms.size) != OK:
            raise MochiError(f"mochi_ctx_read_read_decode_profile: {_err(self.lib)}")
        return dict(zip(READ_REQUEST_STAGES, (float(x) for x in ms)))

    def envelope_decode_device(self, dframes: "DeviceEnvelopeFrames", out: "DeviceEnvelopeDecoded",
                               stream: int = 0) -> None:
        """mochi_envelope_decode_device: device-resident frames -> the arrays of `out`; no wait."""
        f, o = dframes.to_c(), out.to_c()
        rc = self.lib.mochi_envelope_decode_device(self.ctx, ctypes.addressof(f), ctypes.addressof(o), stream or None)
        if rc != OK:
            raise MochiError(f"mochi_envelope_decode_device rc={rc}: {_err(self.lib)}")

    def envelope_route_device(self, dec: "DeviceEnvelopeDecoded", out: "DeviceEnvelopeRouted", stream: int = 0) -> None:
        """mochi_envelope_route_device over the decode's outputs; kind_off stays on the device; no wait."""
        o = out.to_c()
        rc = self.lib.mochi_envelope_route_device(self.ctx, dec.n, dec.status.data_ptr(), dec.kind.data_ptr(),
                                                  dec.body_off.data_ptr(), dec.body_len.data_ptr(), ctypes.addressof(o),
                                                  stream or None)
        if rc != OK:
            raise MochiError(f"mochi_envelope_route_device rc={rc}: {_err(self.lib)}")

    def envelope_join_device(self, dreqs: "DeviceEnvelopeRequests", dframes: "DeviceEnvelopeFrames",
                             dec: "DeviceEnvelopeDecoded", out: "DeviceEnvelopeJoined", stream: int = 0) -> None:
        """mochi_envelope_join_device: the replies of `dframes` grouped by request into `out`
        (out.n_resps: the device word P goes to); no wait."""
        r, f, d, o = dreqs.to_c(), dframes.to_c(), dec.to_c(), out.to_c()
        rc = self.lib.mochi_envelope_join_device(self.ctx, ctypes.addressof(r), ctypes.addressof(f), ctypes.addressof(d),
                                                 ctypes.addressof(o), out.n_resps.data_ptr(), stream or None)
        if rc != OK:
            raise MochiError(f"mochi_envelope_join_device rc={rc}: {_err(self.lib)}")

    def envelope_encode_device(self, dsrc: "DeviceEnvelopeSource", wire, msg_off, msg_len, status, stream: int = 0,
                               wire_len_dev=None, check: bool = True):
        """mochi_envelope_encode_device; arguments and result as result_reply_encode_device."""
        s = dsrc.to_c()
        cap = 0 if wire is None else int(wire.numel())
        need = ctypes.c_uint64(0)
        rc = self.lib.mochi_envelope_encode_device(
            self.ctx, ctypes.addressof(s), wire.data_ptr() if cap else None, cap, msg_off.data_ptr(), msg_len.data_ptr(),
            status.data_ptr(), ctypes.addressof(need) if wire_len_dev is None else None,
            None if wire_len_dev is None else wire_len_dev.data_ptr(), stream or None)
        short = wire_len_dev is None and rc == EINVAL and int(need.value) > cap
        if rc != OK and (check or not short):
            raise MochiError(f"mochi_envelope_encode_device rc={rc}: {_err(self.lib)}")
        return rc, (int(need.value) if wire_len_dev is None else None)

    def read_envelope_profile(self, which: str) -> dict:
        """Per-kernel ms of the last envelope_<which>_device call made with set_profiling(True);
        which: "decode", "route", "join" or "encode"."""
        names = ENVELOPE_STAGES[which]
        ms = np.zeros(len(names), np.float32)
        if self.lib.mochi_ctx_read_envelope_profile(self.ctx, list(ENVELOPE_STAGES).index(which), _ptr(ms), ms.size) != OK:
            raise MochiError(f"mochi_ctx_read_envelope_profile: {_err(self.lib)}")
        return dict(zip(names, (float(x) for x in ms)))

    def decode_write2(self, wb) -> dict:
        """The device decoder's SoA view of the messages (inspection / tests), and under
        "grant_same" its first-grant hint to grant prep ([n_grants], mochi_write2_decode_same)."""
        wc, keep = write2_batch_c(wb)
        d = Write2Decoded_C()
        same = ctypes.c_void_p()
        rc = self.lib.mochi_write2_decode_same(self.ctx, ctypes.addressof(wc), ctypes.addressof(d),
                                               ctypes.addressof(same))
        if rc != OK:
            raise MochiError(f"mochi_write2_decode_same rc={rc}: {_err(self.lib)}")
        N, M, O = d.n_grants, d.n_msgs, d.n_ops

        def arr(ptr, n, dt):
            if n == 0:
                return np.zeros(0, dt)
            return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(np.ctypeslib.as_ctypes_type(dt))),
                                         shape=(n,)).copy()

        out = dict(grant_off=arr(d.grant_off, N, np.uint64), grant_len=arr(d.grant_len, N, np.uint32),
                   sig=arr(d.sig, N * 256, np.uint8).reshape(N, 256), signer=arr(d.signer, N, np.uint16),
                   grant_key=arr(d.grant_key, N, np.uint8), cert_grant_off=arr(d.cert_grant_off, M + 1, np.uint32),
                   cert_op_off=arr(d.cert_op_off, M + 1, np.uint32), op_key=arr(d.op_key, O, np.uint8),
                   op_flags=arr(d.op_flags, O, np.uint8), msg_status=arr(d.msg_status, M, np.uint8),
                   cert_mg_off=arr(d.cert_mg_off, M + 1, np.uint32),
                   mg_grant_off=arr(d.mg_grant_off, d.n_mgs + 1, np.uint32),
                   op_key_off=arr(d.op_key_off, O, np.uint64), op_key_len=arr(d.op_key_len, O, np.uint32),
                   grant_same=arr(same, N, np.uint32))
        self.lib.mochi_write2_decoded_free(ctypes.addressof(d))
        self.lib.mochi_write2_same_free(same)
        return out

    def set_small_batch(self, grants: int) -> None:
        """Batches of at most `grants` grants take the small-batch launch sequence
        (mochi_ctx_set_small_batch); 0 = never."""
        if self.lib.mochi_ctx_set_small_batch(self.ctx, int(grants)) != OK:
            raise MochiError(_err(self.lib))

    def set_chunk_grants(self, grants: int) -> None:
        """Host-path pipeline chunk target (grants); 0 restores the default."""
        if self.lib.mochi_ctx_set_chunk_grants(self.ctx, int(grants)) != OK:
            raise MochiError(_err(self.lib))

    def close(self) -> None:
        if getattr(self, "ctx", None):
            self.lib.mochi_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def verify(self, batch: Batch, replication_factor: int, strict_gt: bool = True, quorum_mode: int = 0) -> Verdicts:
        """Host-memory batch -> verdicts (pinned staging, synchronous)."""
        b = batch.normalized()
        out = Verdicts.alloc(b.n_grants, b.n_certs, b.n_ops)
        bc, vc = b.to_c(), out.to_c()
        p = params(replication_factor, strict_gt, quorum_mode)
        rc = self.lib.mochi_verify_batch(self.ctx, ctypes.byref(bc), ctypes.byref(p), ctypes.byref(vc))
        if rc != OK:
            raise MochiError(f"mochi_verify_batch rc={rc}: {_err(self.lib)}")
        h, k, d, t = ctypes.c_float(), ctypes.c_float(), ctypes.c_float(), ctypes.c_float()
        self.lib.mochi_ctx_last_timing(self.ctx, ctypes.byref(h), ctypes.byref(k), ctypes.byref(d))
        self.lib.mochi_ctx_last_total_ms(self.ctx, ctypes.byref(t))
        out.timing_ms = {"h2d": h.value, "kernels": k.value, "d2h": d.value, "total": t.value}
        return out

    STAGES = ("prep_sha256", "bucket", "rsa_pow", "rsa_final", "tally")

    def set_profiling(self, on: bool) -> None:
        self.lib.mochi_ctx_set_profiling(self.ctx, 1 if on else 0)

    def read_profile(self) -> dict:
        """Mean per-call stage times (ms) since the last read; waits for the device."""
        arr = (ctypes.c_float * len(self.STAGES))()
        n = ctypes.c_uint32()
        rc = self.lib.mochi_ctx_read_profile(self.ctx, arr, len(self.STAGES), ctypes.byref(n))
        if rc != OK:
            raise MochiError(f"mochi_ctx_read_profile rc={rc}: {_err(self.lib)}")
        calls = max(1, n.value)
        out = {name: arr[i] / calls for i, name in enumerate(self.STAGES)}
        out["calls"] = n.value
        return out

    def verify_device(self, dev: "DeviceBatch", out: "DeviceVerdicts", replication_factor: int,
                      strict_gt: bool = True, stream: int = 0, quorum_mode: int = 0) -> None:
        """Device-resident batch (torch tensors) -> device verdicts; async on `stream`."""
        p = params(replication_factor, strict_gt, quorum_mode)
        bc, vc = dev.to_c(), out.to_c()
        rc = self.lib.mochi_verify_batch_device(self.ctx, ctypes.byref(bc), ctypes.byref(p), ctypes.byref(vc),
                                                stream or None)
        if rc != OK:
            raise MochiError(f"mochi_verify_batch_device rc={rc}: {_err(self.lib)}")


def fold_matrix(modulus_be: bytes):
    """The k_rsa_pow fold matrix of one modulus (mochi_fold_matrix): int8 image
    [10 M-tiles][10 K-steps][64 lanes][16] and the bias correction cadd uint32[74]."""
    lib = load_library()
    m = np.frombuffer(bytes(modulus_be), np.uint8)
    img = np.zeros((10, 10, 64, 16), np.int8)
    cadd = np.zeros(74, np.uint32)
    rc = lib.mochi_fold_matrix(_ptr(m), _ptr(img), _ptr(cadd))
    if rc != OK:
        raise MochiError(f"mochi_fold_matrix rc={rc}: {_err(lib)}")
    return img, cadd


def rsa_public_op(verifier: "Verifier", sigs: np.ndarray, signer: np.ndarray, want_z: bool = False):
    """y = s^65537 mod n on the device (big-endian bytes); optionally the chain intermediate z."""
    lib = verifier.lib
    s = np.ascontiguousarray(sigs, np.uint8).reshape(-1, RSA_BYTES)
    sg = np.ascontiguousarray(signer, np.uint16)
    n = s.shape[0]
    out = np.zeros((n, RSA_BYTES), np.uint8)
    z = np.zeros((n, 74), np.uint32) if want_z else None
    rc = lib.mochi_rsa_public_op(verifier.ctx, n, _ptr(s), _ptr(sg), _ptr(out), _ptr(z) if want_z else None)
    if rc != OK:
        raise MochiError(f"mochi_rsa_public_op rc={rc}: {_err(lib)}")
    return (out, z) if want_z else out


class DeviceBatch:
    """A Batch copied into device memory with torch (plumbing only)."""

    def __init__(self, batch: Batch, device: int = 0):
        import torch

        b = batch.normalized()
        dev = torch.device("cuda", device)

        def t(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

        self.n_grants, self.n_certs, self.n_ops = b.n_grants, b.n_certs, b.n_ops
        self.grant_bytes = t(b.grant_bytes)
        self.grant_off = t(b.grant_off.view(np.int64))
        self.grant_len = t(b.grant_len.view(np.int32))
        self.sig = t(b.sig)
        self.signer = t(b.signer.view(np.int16))
        self.grant_key = t(b.grant_key)
        self.cert_grant_off = t(b.cert_grant_off.view(np.int32))
        self.cert_op_off = t(b.cert_op_off.view(np.int32))
        self.op_key = t(b.op_key)
        self.op_flags = t(b.op_flags)
        self.expected_hash = t(b.expected_hash)
        self.n_mgs = b.n_mgs
        sv = {np.uint32: np.int32, np.uint64: np.int64, np.int64: np.int64}
        for k in Batch.OPTIONAL:
            a = getattr(b, k)
            setattr(self, k, None if a is None else t(a.view(sv[Batch.OPT_DTYPES[k]])))

    def to_c(self) -> Batch_C:
        b = Batch_C()
        b.n_grants, b.n_certs, b.n_ops, b.n_mgs = self.n_grants, self.n_certs, self.n_ops, self.n_mgs
        b.grant_bytes_len = int(self.grant_bytes.numel())
        for name in Batch.FIELDS:
            setattr(b, name, getattr(self, name).data_ptr())
        for name in Batch.OPTIONAL:
            a = getattr(self, name)
            setattr(b, name, None if a is None else a.data_ptr())
        return b


class DeviceWireBatch:
    """A workload.WireBatch copied into device memory with torch (plumbing only)."""

    def __init__(self, wb, device: int = 0):
        import torch

        dev = torch.device("cuda", device)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.n_msgs = wb.n_msgs
        self.wire = t(wb.wire)
        self.msg_off = t(np.ascontiguousarray(wb.msg_off, np.uint64).view(np.int64))
        self.msg_len = t(np.ascontiguousarray(wb.msg_len, np.uint32).view(np.int32))
        self.op_flags_off = None if wb.op_flags_off is None else t(np.ascontiguousarray(wb.op_flags_off, np.uint32).view(np.int32))
        self.op_flags = t(wb.op_flags if wb.op_flags.size else np.zeros(1, np.uint8))
        self.expected_hash = t(np.ascontiguousarray(wb.expected_hash, np.uint8).reshape(-1))
        ots = getattr(wb, "op_object_ts", None)
        self.op_object_ts = None if ots is None or wb.op_flags_off is None else t(np.ascontiguousarray(ots, np.int64))
        self.status = torch.zeros(max(self.n_msgs, 1), dtype=torch.uint8, device=dev)

    @classmethod
    def from_encoded(cls, wire, msg_off, msg_len, n_msgs: int, expected_hash, op_flags_off=None, op_flags=None,
                     op_object_ts=None) -> "DeviceWireBatch":
        """The device outputs of Verifier.encode_write2_device (wire / msg_off /
        msg_len tensors, used as they are: no copy, no host round trip) as the input
        of verify_write2_device.  expected_hash [M, 128] and the optional per-op
        arrays may be numpy arrays or tensors on the same device."""
        import torch

        dev = wire.device
        t = lambda a, dt: a.to(dev) if isinstance(a, torch.Tensor) else torch.from_numpy(
            np.ascontiguousarray(a).view(dt)).to(dev)
        self = cls.__new__(cls)
        self.n_msgs = int(n_msgs)
        self.wire, self.msg_off, self.msg_len = wire, msg_off, msg_len
        self.op_flags_off = None if op_flags_off is None else t(op_flags_off, np.int32)
        self.op_flags = (torch.zeros(1, dtype=torch.uint8, device=dev) if op_flags is None or len(op_flags) == 0
                         else t(op_flags, np.uint8))
        self.expected_hash = t(expected_hash, np.uint8).reshape(-1)
        self.op_object_ts = None if op_object_ts is None or op_flags_off is None else t(op_object_ts, np.int64)
        self.status = torch.zeros(max(self.n_msgs, 1), dtype=torch.uint8, device=dev)
        return self

    def to_c(self) -> "Write2Batch_C":
        c = Write2Batch_C()
        c.n_msgs = self.n_msgs
        c.wire_len = int(self.wire.numel())
        c.wire, c.msg_off, c.msg_len = self.wire.data_ptr(), self.msg_off.data_ptr(), self.msg_len.data_ptr()
        c.op_flags_off = None if self.op_flags_off is None else self.op_flags_off.data_ptr()
        c.op_flags, c.expected_hash = self.op_flags.data_ptr(), self.expected_hash.data_ptr()
        c.op_object_ts = None if self.op_object_ts is None else self.op_object_ts.data_ptr()
        return c


class DeviceVerdicts:
    def __init__(self, n_grants: int, n_certs: int, device: int = 0, full: bool = True, n_ops: int = 0):
        import torch

        dev = torch.device("cuda", device)
        self.n_grants, self.n_certs = n_grants, n_certs
        self.cert_accept_bits = torch.zeros((n_certs + 31) // 32, dtype=torch.int32, device=dev)
        self.grant_valid_bits = torch.zeros((n_grants + 31) // 32, dtype=torch.int32, device=dev)
        self.grant_flags = torch.zeros(n_grants, dtype=torch.uint8, device=dev) if full else None
        self.grant_ts = torch.zeros(n_grants, dtype=torch.int64, device=dev) if full else None
        self.cert_reason = torch.zeros(n_certs, dtype=torch.uint8, device=dev) if full else None
        self.cert_fail_op = torch.zeros(n_certs, dtype=torch.uint8, device=dev) if full else None
        op = full and n_ops > 0
        self.op_decision = torch.zeros(n_ops, dtype=torch.uint8, device=dev) if op else None
        self.op_g0 = torch.zeros(n_ops, dtype=torch.int32, device=dev) if op else None
        self.op_ts = torch.zeros(n_ops, dtype=torch.int64, device=dev) if op else None

    NAMES = ("grant_valid_bits", "grant_flags", "grant_ts", "cert_accept_bits", "cert_reason", "cert_fail_op",
             "op_decision", "op_g0", "op_ts")

    def to_c(self) -> Verdicts_C:
        v = Verdicts_C()
        for name in self.NAMES:
            t = getattr(self, name)
            setattr(v, name, t.data_ptr() if t is not None else None)
        return v

    def to_host(self) -> Verdicts:
        def h(t, dt):
            return t.cpu().numpy().view(dt) if t is not None else None

        return Verdicts(
            grant_valid_bits=h(self.grant_valid_bits, np.uint32),
            grant_flags=h(self.grant_flags, np.uint8),
            grant_ts=h(self.grant_ts, np.int64),
            cert_accept_bits=h(self.cert_accept_bits, np.uint32),
            cert_reason=h(self.cert_reason, np.uint8),
            cert_fail_op=h(self.cert_fail_op, np.uint8),
            op_decision=h(self.op_decision, np.uint8),
            op_g0=h(self.op_g0, np.uint32),
            op_ts=h(self.op_ts, np.int64),
        )


def sign_grants(pem_private_key: bytes, grant_bytes: np.ndarray, grant_off: np.ndarray, grant_len: np.ndarray,
                n_threads: int = 8) -> np.ndarray:
    """Producer-side SHA256withRSA signing of grants (libmochi_hip, OpenSSL)."""
    lib = load_library()
    blob = np.ascontiguousarray(grant_bytes, np.uint8)
    off = np.ascontiguousarray(grant_off, np.uint64)
    ln = np.ascontiguousarray(grant_len, np.uint32)
    n = off.shape[0]
    out = np.zeros((n, RSA_BYTES), np.uint8)
    rc = lib.mochi_sign_grants(pem_private_key, n, _ptr(blob), _ptr(off), _ptr(ln), _ptr(out), int(n_threads))
    if rc != OK:
        raise MochiError(f"mochi_sign_grants rc={rc}")
    return out


def pem_modulus(pem: bytes) -> bytes:
    lib = load_library()
    out = np.zeros(RSA_BYTES, np.uint8)
    if lib.mochi_pem_modulus(pem, _ptr(out)) != OK:
        raise MochiError("not an RSA-2048 PEM key")
    return out.tobytes()


def tally_responses(responses: Sequence[Sequence[Sequence[int]]], n_ops: Sequence[int], replication_factor: int):
    """Client aggregation (MochiDBClient.java:148-175 / 355-382) via libmochi_hip.

    responses[r] = list of per-response status lists.  Returns (accept[bool],
    reason[uint8], chosen[list of int arrays]).
    """
    lib = load_library()
    nreq = len(responses)
    resp_off = np.zeros(nreq + 1, np.uint32)
    resp_n_ops, status_off, status, chosen_off = [], [], [], np.zeros(nreq, np.uint64)
    pos = 0
    cpos = 0
    for r, resps in enumerate(responses):
        resp_off[r + 1] = resp_off[r] + len(resps)
        chosen_off[r] = cpos
        cpos += n_ops[r]
        for st in resps:
            resp_n_ops.append(len(st))
            status_off.append(pos)
            status.extend(st)
            pos += len(st)
    n_ops_a = np.asarray(n_ops, np.uint32)
    resp_n_ops_a = np.asarray(resp_n_ops if resp_n_ops else [0], np.uint32)
    status_off_a = np.asarray(status_off if status_off else [0], np.uint64)
    status_a = np.asarray(status if status else [0], np.uint8)
    chosen = np.full(max(cpos, 1), -1, np.int32)
    reason = np.zeros(max(nreq, 1), np.uint8)
    bits = np.zeros(max((nreq + 31) // 32, 1), np.uint32)
    rc = lib.mochi_tally_responses(nreq, _ptr(resp_off), _ptr(n_ops_a), _ptr(resp_n_ops_a), _ptr(status_off_a),
                                   _ptr(status_a), _ptr(chosen_off), replication_factor, _ptr(chosen), _ptr(reason),
                                   _ptr(bits))
    if rc != OK:
        raise MochiError(f"mochi_tally_responses rc={rc}: {_err(lib)}")
    acc = unpack_bits(bits, nreq)
    ch = [chosen[int(chosen_off[r]):int(chosen_off[r]) + n_ops[r]].copy() for r in range(nreq)]
    return acc, reason[:nreq].copy(), ch


def _pack_responses(responses, n_ops):
    nreq = len(responses)
    resp_off = np.zeros(nreq + 1, np.uint32)
    resp_n_ops, status_off, status, chosen_off = [], [], [], np.zeros(max(nreq, 1), np.uint64)
    pos = cpos = 0
    for r, resps in enumerate(responses):
        resp_off[r + 1] = resp_off[r] + len(resps)
        chosen_off[r] = cpos
        cpos += n_ops[r]
        for st in resps:
            resp_n_ops.append(len(st))
            status_off.append(pos)
            status.extend(st)
            pos += len(st)
    return (resp_off, np.asarray(n_ops if len(n_ops) else [0], np.uint32),
            np.asarray(resp_n_ops if resp_n_ops else [0], np.uint32),
            np.asarray(status_off if status_off else [0], np.uint64), np.asarray(status if status else [0], np.uint8),
            chosen_off, max(cpos, 1))


def tally_responses_device(responses, n_ops, replication_factor: int, device: int = 0):
    """Client aggregation on the device (mochi_tally_responses_device), batched over
    requests; same results as tally_responses.  torch moves the arrays (plumbing)."""
    import torch

    lib = load_library()
    nreq = len(responses)
    resp_off, n_ops_a, rn, so, st, co, nch = _pack_responses(responses, n_ops)
    d = torch.device("cuda", device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view({1: np.uint8, 2: np.int16, 4: np.int32,
                                                                 8: np.int64}[a.dtype.itemsize])).to(d)
    ts = [t(x) for x in (resp_off, n_ops_a, rn, so, st, co)]
    chosen = torch.full((nch,), -1, dtype=torch.int32, device=d)
    reason = torch.zeros(max(nreq, 1), dtype=torch.uint8, device=d)
    bits = torch.zeros(max((nreq + 31) // 32, 1), dtype=torch.int32, device=d)
    rc = lib.mochi_tally_responses_device(nreq, *[x.data_ptr() for x in ts[:6]], replication_factor,
                                          chosen.data_ptr(), reason.data_ptr(), bits.data_ptr(),
                                          torch.cuda.current_stream(d).cuda_stream)
    if rc != OK:
        raise MochiError(f"mochi_tally_responses_device rc={rc}")
    torch.cuda.synchronize(d)
    acc = unpack_bits(bits.cpu().numpy().view(np.uint32), nreq)
    ch_h = chosen.cpu().numpy()
    ch = [ch_h[int(co[r]):int(co[r]) + n_ops[r]].copy() for r in range(nreq)]
    return acc, reason.cpu().numpy()[:nreq].copy(), ch


def write1_classify_device(requests, device: int = 0) -> np.ndarray:
    """Client Write1 round outcome per request on the device (mochi_write1_classify_device)."""
    import torch

    lib = load_library()
    a = pack_write1(requests)
    d = torch.device("cuda", device)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x).view({1: np.uint8, 4: np.int32,
                                                                 8: np.int64}[x.dtype.itemsize])).to(d)
    ts = [t(x) for x in a]
    out = torch.zeros(max(len(requests), 1), dtype=torch.uint8, device=d)
    rc = lib.mochi_write1_classify_device(len(requests), *[x.data_ptr() for x in ts], out.data_ptr(),
                                          torch.cuda.current_stream(d).cuda_stream)
    if rc != OK:
        raise MochiError(f"mochi_write1_classify_device rc={rc}")
    torch.cuda.synchronize(d)
    return out.cpu().numpy()[:len(requests)].copy()


# Write1 response kinds / round decisions (include/mochi_hip.h)
W1_OK, W1_REFUSED, W1_REQUEST_FAILED, W1_OTHER = 0, 1, 2, 3
W1_PROCEED, W1_RETRY, W1_THROW_REFUSED, W1_THROW_FAILED, W1_THROW_UNSUPPORTED = 0, 1, 2, 3, 4


def pack_write1(requests):
    """requests[r] = list of responses (kind, server_id, [(key_slot, ts, status), ...])
    -> the CSR arrays of mochi_write1_classify."""
    resp_off = np.zeros(len(requests) + 1, np.uint32)
    kinds, servers, goff, keys, tss, sts = [], [], [0], [], [], []
    for r, resps in enumerate(requests):
        resp_off[r + 1] = resp_off[r] + len(resps)
        for kind, sid, grants in resps:
            kinds.append(kind)
            servers.append(sid)
            for key, ts, st in grants:
                keys.append(key)
                tss.append(ts)
                sts.append(st)
            goff.append(len(keys))
    arr = lambda v, dt: np.asarray(v if v else [0], dt)
    return (resp_off, arr(kinds, np.uint8), arr(servers, np.uint32), np.asarray(goff, np.uint32),
            arr(keys, np.uint8), arr(tss, np.int64), arr(sts, np.uint8))


def write1_classify(requests) -> np.ndarray:
    """Client Write1 round outcome per request (MochiDBClient.java:236-332) via libmochi_hip."""
    lib = load_library()
    a = pack_write1(requests)
    out = np.zeros(max(len(requests), 1), np.uint8)
    rc = lib.mochi_write1_classify(len(requests), *[_ptr(x) for x in a], _ptr(out))
    if rc != OK:
        raise MochiError(f"mochi_write1_classify: {_err(lib)}")
    return out[:len(requests)].copy()


class Write2Batch_C(ctypes.Structure):
    _fields_ = [
        ("n_msgs", ctypes.c_uint32),
        ("_pad0", ctypes.c_uint32),
        ("wire_len", ctypes.c_uint64),
        ("wire", ctypes.c_void_p),
        ("msg_off", ctypes.c_void_p),
        ("msg_len", ctypes.c_void_p),
        ("op_flags_off", ctypes.c_void_p),
        ("op_flags", ctypes.c_void_p),
        ("expected_hash", ctypes.c_void_p),
        ("op_object_ts", ctypes.c_void_p),
    ]


MSG_OK, MSG_MALFORMED, MSG_FALLBACK, MSG_OPS_MISMATCH = 0, 1, 2, 3
UNDECIDED = 7
REASON_NAMES[UNDECIDED] = "UNDECIDED"


def write2_batch_c(wb):
    """workload.WireBatch (host arrays) -> (Write2Batch_C, keep-alive list)."""
    arrs = [np.ascontiguousarray(wb.wire, np.uint8), np.ascontiguousarray(wb.msg_off, np.uint64),
            np.ascontiguousarray(wb.msg_len, np.uint32),
            None if wb.op_flags_off is None else np.ascontiguousarray(wb.op_flags_off, np.uint32),
            np.ascontiguousarray(wb.op_flags if wb.op_flags.size else np.zeros(1, np.uint8), np.uint8),
            np.ascontiguousarray(wb.expected_hash, np.uint8).reshape(-1)]
    ots = getattr(wb, "op_object_ts", None)
    arrs.append(None if ots is None or wb.op_flags_off is None else np.ascontiguousarray(ots, np.int64))
    c = Write2Batch_C()
    c.n_msgs = int(arrs[1].shape[0])
    c.wire_len = int(arrs[0].nbytes)
    c.wire, c.msg_off, c.msg_len = _ptr(arrs[0]), _ptr(arrs[1]), _ptr(arrs[2])
    c.op_flags_off, c.op_flags, c.expected_hash = _ptr(arrs[3]), _ptr(arrs[4]), _ptr(arrs[5])
    c.op_object_ts = _ptr(arrs[6])
    return c, arrs



# ---------------------------------------------------------------------------
# Write2ToServer encode (client certificate assembly, MochiDBClient.java:333-338)
# ---------------------------------------------------------------------------
ENC_OK, ENC_BAD_GRANT, ENC_BAD_SIGNER, ENC_TOO_LONG = 0, 1, 2, 3


class Write2Source_C(ctypes.Structure):
    _fields_ = [("n_msgs", ctypes.c_uint32), ("n_mgs", ctypes.c_uint32), ("n_grants", ctypes.c_uint32),
                ("n_ops", ctypes.c_uint32),
                ("grant_bytes", ctypes.c_void_p), ("grant_bytes_len", ctypes.c_uint64),
                ("grant_off", ctypes.c_void_p), ("grant_len", ctypes.c_void_p), ("sig", ctypes.c_void_p),
                ("cert_mg_off", ctypes.c_void_p), ("mg_grant_off", ctypes.c_void_p), ("mg_signer", ctypes.c_void_p),
                ("strings", ctypes.c_void_p), ("strings_len", ctypes.c_uint64),
                ("cert_op_off", ctypes.c_void_p), ("op_action", ctypes.c_void_p),
                ("op1_off", ctypes.c_void_p), ("op1_len", ctypes.c_void_p),
                ("op2_off", ctypes.c_void_p), ("op2_len", ctypes.c_void_p),
                ("client_off", ctypes.c_void_p), ("client_len", ctypes.c_void_p)]


@dataclass
class Write2Source:
    """SoA source of M Write2ToServer messages (mochi_write2_source, host arrays)."""

    grant_bytes: np.ndarray  # uint8
    grant_off: np.ndarray  # uint64 [N]
    grant_len: np.ndarray  # uint32 [N]
    sig: Optional[np.ndarray]  # uint8 [N, 256] or None = no grantSignatures entries
    cert_mg_off: np.ndarray  # uint32 [M+1]
    mg_grant_off: np.ndarray  # uint32 [n_mgs+1]
    mg_signer: np.ndarray  # uint16 [n_mgs]
    strings: np.ndarray  # uint8: operands and client ids
    cert_op_off: np.ndarray  # uint32 [M+1]
    op_action: np.ndarray  # uint8 [O]
    op1_off: np.ndarray  # uint64 [O]
    op1_len: np.ndarray  # uint32 [O]
    op2_off: Optional[np.ndarray] = None
    op2_len: Optional[np.ndarray] = None
    client_off: Optional[np.ndarray] = None  # uint64 [M]
    client_len: Optional[np.ndarray] = None  # uint32 [M]

    DTYPES = dict(grant_bytes=np.uint8, grant_off=np.uint64, grant_len=np.uint32, sig=np.uint8, cert_mg_off=np.uint32,
                  mg_grant_off=np.uint32, mg_signer=np.uint16, strings=np.uint8, cert_op_off=np.uint32,
                  op_action=np.uint8, op1_off=np.uint64, op1_len=np.uint32, op2_off=np.uint64, op2_len=np.uint32,
                  client_off=np.uint64, client_len=np.uint32)

    @property
    def n_msgs(self) -> int:
        return int(self.cert_mg_off.shape[0]) - 1

    @property
    def n_mgs(self) -> int:
        return int(self.mg_signer.shape[0])

    @property
    def n_grants(self) -> int:
        return int(self.grant_off.shape[0])

    @property
    def n_ops(self) -> int:
        return int(self.op_action.shape[0])

    def arrays(self) -> dict:
        """Every array C-contiguous in its ABI dtype (None stays None)."""
        out = {}
        for k, dt in self.DTYPES.items():
            a = getattr(self, k)
            out[k] = None if a is None else np.ascontiguousarray(a, dt).reshape(-1)
        return out

    def to_c(self):
        arrs = self.arrays()
        c = Write2Source_C()
        c.n_msgs, c.n_mgs, c.n_grants, c.n_ops = self.n_msgs, self.n_mgs, self.n_grants, self.n_ops
        c.grant_bytes_len = int(arrs["grant_bytes"].nbytes)
        c.strings_len = int(arrs["strings"].nbytes)
        for k, a in arrs.items():
            # an empty array still gets a valid address (the library reads none of it)
            setattr(c, k, None if a is None else _ptr(a if a.size else np.zeros(1, a.dtype)))
        return c, arrs


def _id_table(server_ids):
    enc = [x.encode() if isinstance(x, str) else bytes(x) for x in server_ids]
    blob = np.frombuffer(b"".join(enc) or b"\x00", np.uint8).copy()
    off = np.zeros(len(enc) + 1, np.uint32)
    np.cumsum([len(x) for x in enc], out=off[1:])
    return blob, off, len(enc)


def write2_encode_bound(src: "Write2Source", max_id_len: int) -> int:
    """mochi_write2_encode_bound: a safe (not tight) upper bound on the wire size."""
    c, keep = src.to_c()
    return int(load_library().mochi_write2_encode_bound(ctypes.addressof(c), int(max_id_len)))


def encode_write2_into(src: "Write2Source", server_ids, wire: Optional[np.ndarray]):
    """mochi_write2_encode into the caller's buffer (uint8; None = capacity 0).
    Returns (rc, wire_len, msg_off, msg_len, status); rc is EINVAL with wire_len =
    the size needed when the buffer is too small (no byte of it written)."""
    lib = load_library()
    c, keep = src.to_c()
    ids, id_off, n_ids = _id_table(server_ids)
    M = src.n_msgs
    msg_off = np.zeros(max(M, 1), np.uint64)
    msg_len = np.zeros(max(M, 1), np.uint32)
    status = np.zeros(max(M, 1), np.uint8)
    n = ctypes.c_uint64(0)
    cap = 0 if wire is None else int(wire.nbytes)
    rc = lib.mochi_write2_encode(ctypes.addressof(c), _ptr(ids), _ptr(id_off), n_ids, _ptr(wire) if cap else None, cap,
                                 _ptr(msg_off), _ptr(msg_len), _ptr(status), ctypes.addressof(n))
    return rc, int(n.value), msg_off[:M], msg_len[:M], status[:M]


def encode_write2(src: "Write2Source", server_ids):
    """Host form of the Write2ToServer encoder: (wire uint8 [wire_len], msg_off
    uint64 [M], msg_len uint32 [M], status uint8 [M]) for the source's messages,
    laid out as mochi_write2_batch takes them.  server_ids[i] = the id of key i."""
    lib = load_library()
    rc, need, msg_off, msg_len, status = encode_write2_into(src, server_ids, None)  # sizes only
    if rc != OK and need == 0:
        raise MochiError(f"mochi_write2_encode rc={rc}: {_err(lib)}")
    wire = np.zeros(max(need, 1), np.uint8)
    rc, n, msg_off, msg_len, status = encode_write2_into(src, server_ids, wire)
    if rc != OK:
        raise MochiError(f"mochi_write2_encode rc={rc}: {_err(lib)}")
    return wire[:n], msg_off, msg_len, status


class DeviceWrite2Source:
    """A Write2Source copied into device memory with torch (plumbing only)."""

    def __init__(self, src: "Write2Source", device: int = 0):
        import torch

        dev = torch.device("cuda", device)
        sv = {np.uint8: np.uint8, np.uint16: np.int16, np.uint32: np.int32, np.uint64: np.int64}
        self.n_msgs, self.n_mgs, self.n_grants, self.n_ops = src.n_msgs, src.n_mgs, src.n_grants, src.n_ops
        for k, a in src.arrays().items():
            if a is not None and a.size == 0:
                a = np.zeros(1, a.dtype)
            setattr(self, k, None if a is None else torch.from_numpy(a.view(sv[Write2Source.DTYPES[k]])).to(dev))
        self.grant_bytes_len = int(np.asarray(src.grant_bytes).size)
        self.strings_len = int(np.asarray(src.strings).size)

    @classmethod
    def from_tensors(cls, n_msgs: int, n_mgs: int, n_grants: int, n_ops: int, **tensors) -> "DeviceWrite2Source":
        """A source whose arrays are already on the device (used as they are: no
        copy, no host round trip), e.g. the grant_bytes / grant_off / grant_len /
        sig a DeviceSigner.issue_device call wrote.  Every Write2Source field is a
        torch tensor of the ABI width or None."""
        self = cls.__new__(cls)
        self.n_msgs, self.n_mgs, self.n_grants, self.n_ops = int(n_msgs), int(n_mgs), int(n_grants), int(n_ops)
        for k in Write2Source.DTYPES:
            setattr(self, k, tensors.get(k))
        self.grant_bytes_len = int(self.grant_bytes.numel())
        self.strings_len = int(self.strings.numel())
        return self

    def to_c(self) -> Write2Source_C:
        c = Write2Source_C()
        c.n_msgs, c.n_mgs, c.n_grants, c.n_ops = self.n_msgs, self.n_mgs, self.n_grants, self.n_ops
        c.grant_bytes_len, c.strings_len = self.grant_bytes_len, self.strings_len
        for k in Write2Source.DTYPES:
            t = getattr(self, k)
            setattr(c, k, None if t is None else t.data_ptr())
        return c


class Write2Decoded_C(ctypes.Structure):
    _fields_ = [("n_msgs", ctypes.c_uint32), ("n_grants", ctypes.c_uint32), ("n_ops", ctypes.c_uint32),
                ("n_mgs", ctypes.c_uint32), ("grant_off", ctypes.c_void_p), ("grant_len", ctypes.c_void_p),
                ("sig", ctypes.c_void_p), ("signer", ctypes.c_void_p), ("grant_key", ctypes.c_void_p),
                ("cert_grant_off", ctypes.c_void_p), ("cert_op_off", ctypes.c_void_p), ("op_key", ctypes.c_void_p),
                ("op_flags", ctypes.c_void_p), ("msg_status", ctypes.c_void_p), ("cert_mg_off", ctypes.c_void_p),
                ("mg_grant_off", ctypes.c_void_p), ("op_key_off", ctypes.c_void_p), ("op_key_len", ctypes.c_void_p)]


class Verdict1_C(ctypes.Structure):
    _fields_ = [("accepted", ctypes.c_uint8), ("reason", ctypes.c_uint8), ("fail_op", ctypes.c_uint8),
                ("msg_status", ctypes.c_uint8)]


VERDICT_CB = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Verdict1_C))


class Write2Request_C(ctypes.Structure):
    """mochi_write2_request (ABI 3)."""
    _fields_ = [("msg", ctypes.c_void_p), ("msg_len", ctypes.c_uint32), ("n_ops", ctypes.c_uint32),
                ("op_flags", ctypes.c_void_p), ("op_object_ts", ctypes.c_void_p), ("expected_hash", ctypes.c_void_p),
                ("op_decision", ctypes.c_void_p), ("op_g0", ctypes.c_void_p), ("op_ts", ctypes.c_void_p)]


class Write2Request:
    """One Write2ToServer as a server receives it, with its per-op state
    (MOCHI_OP_* flags, stored-certificate timestamps) and per-op outputs
    (decision, g0, g0's timestamp) — the buffers live as long as this object."""

    def __init__(self, msg: bytes, expected_hash: bytes, op_flags: Optional[Sequence[int]] = None,
                 op_object_ts: Optional[Sequence[int]] = None, want_ops: bool = True):
        self.msg = np.frombuffer(bytes(msg) or b"\x00", np.uint8).copy()
        self.msg_len = len(msg)
        self.expected_hash = np.frombuffer(bytes(expected_hash), np.uint8).copy()
        assert self.expected_hash.shape[0] == TXN_HASH_BYTES
        n = 0 if op_flags is None else len(op_flags)
        self.op_flags = None if op_flags is None else np.asarray(op_flags, np.uint8).copy()
        self.op_object_ts = None if op_object_ts is None else np.asarray(op_object_ts, np.int64).copy()
        if self.op_object_ts is not None:
            assert self.op_object_ts.shape[0] == n
        self.op_decision = np.zeros(max(n, 1), np.uint8) if want_ops and n else None
        self.op_g0 = np.zeros(max(n, 1), np.uint32) if want_ops and n else None
        self.op_ts = np.zeros(max(n, 1), np.int64) if want_ops and n else None
        self.c = Write2Request_C(_ptr(self.msg), self.msg_len, n, _ptr(self.op_flags), _ptr(self.op_object_ts),
                                 _ptr(self.expected_hash), _ptr(self.op_decision), _ptr(self.op_g0), _ptr(self.op_ts))
        self.result = None  # (rc, accepted, reason, fail_op, msg_status) once delivered

    def ops(self):
        """[(decision, g0, ts)] per op (after the verdict)."""
        if self.op_decision is None:
            return []
        n = self.c.n_ops
        return [(int(self.op_decision[i]), int(self.op_g0[i]), int(self.op_ts[i])) for i in range(n)]


class Batcher:
    """mochi_batcher: blocking per-request verify, coalesced across calling threads.
    (ctypes drops the GIL during the call, so Python threads block concurrently.)"""

    def __init__(self, verifier, replication_factor: int, strict_gt: bool = True, max_msgs: int = 4096,
                 max_wait_us: int = 200, with_op_flags: bool = False):
        # verifier: a Verifier, or a list of them (one flusher, i.e. one batch in
        # flight, per context: mochi_batcher_create_multi)
        vers = list(verifier) if isinstance(verifier, (list, tuple)) else [verifier]
        self.lib = vers[0].lib
        self._ver = vers
        self._p = params(replication_factor, strict_gt)
        self.with_op_flags = with_op_flags
        self._ctxs = (ctypes.c_void_p * len(vers))(*[v.ctx for v in vers])
        self.h = self.lib.mochi_batcher_create_multi(self._ctxs, len(vers), ctypes.addressof(self._p), max_msgs,
                                                     max_wait_us, 1 if with_op_flags else 0)
        if not self.h:
            raise MochiError("mochi_batcher_create failed")
        # mochi_batcher_submit: requests in flight keyed by the callback's user word
        import itertools

        self._seq = itertools.count(1)
        self._pending = {}
        self._cb = VERDICT_CB(self._on_done)

    def _on_done(self, user, rc, v):
        _, _, _, done = self._pending.pop(user)
        d = v.contents
        done(rc, bool(d.accepted), d.reason, d.fail_op, d.msg_status)

    def submit(self, msg: bytes, expected_hash: bytes, done, op_flags: Optional[bytes] = None):
        """Non-blocking (mochi_batcher_submit): done(rc, accepted, reason, fail_op,
        msg_status) runs on a flusher thread once the message's batch is verified."""
        if not self.h:
            raise MochiError("batcher closed")
        key = next(self._seq)
        self._pending[key] = (msg, expected_hash, op_flags, done)  # alive until the callback
        fl = op_flags if op_flags is not None else None
        rc = self.lib.mochi_batcher_submit(self.h, msg, len(msg), fl, len(fl) if fl else 0, expected_hash, self._cb,
                                           key)
        if rc != OK:
            self._pending.pop(key, None)
            raise MochiError(f"mochi_batcher_submit rc={rc}")

    def verify(self, msg: bytes, expected_hash: bytes, op_flags: Optional[bytes] = None):
        out = Verdict1_C()
        fl = op_flags if op_flags is not None else None
        rc = self.lib.mochi_batcher_verify(self.h, msg, len(msg), fl, len(fl) if fl else 0, expected_hash,
                                           ctypes.byref(out))
        if rc != OK:
            raise MochiError(f"mochi_batcher_verify rc={rc}: {_err(self.lib)}")
        return bool(out.accepted), out.reason, out.fail_op, out.msg_status

    def verify_request(self, req: "Write2Request"):
        """mochi_batcher_verify_request: blocks; fills req's per-op outputs."""
        out = Verdict1_C()
        rc = self.lib.mochi_batcher_verify_request(self.h, ctypes.byref(req.c), ctypes.byref(out))
        if rc != OK:
            raise MochiError(f"mochi_batcher_verify_request rc={rc}: {_err(self.lib)}")
        req.result = (rc, bool(out.accepted), out.reason, out.fail_op, out.msg_status)
        return req.result[1:]

    def submit_request(self, req: "Write2Request", done):
        """mochi_batcher_submit_request: done(req) runs on a flusher thread once
        req.result and its per-op outputs are set."""
        key = next(self._seq)

        def fin(rc, accepted, reason, fail_op, msg_status):
            req.result = (rc, accepted, reason, fail_op, msg_status)
            done(req)

        self._pending[key] = (req, None, None, fin)
        rc = self.lib.mochi_batcher_submit_request(self.h, ctypes.byref(req.c), self._cb, key)
        if rc != OK:
            self._pending.pop(key, None)
            raise MochiError(f"mochi_batcher_submit_request rc={rc}")

    def stats(self):
        b, m = ctypes.c_uint64(), ctypes.c_uint64()
        self.lib.mochi_batcher_stats(self.h, ctypes.byref(b), ctypes.byref(m))
        return b.value, m.value

    def close(self):
        """mochi_batcher_destroy, once.  From one of this batcher's callbacks the
        library defers the teardown (queued requests still complete; its last
        flusher frees it); the handle is dropped here either way, so a later
        close() / __del__ cannot free the batcher a second time.  The library
        holds the contexts until the batcher is freed (a mochi_ctx_destroy before that
        returns at once and the batcher's release frees the context)."""
        h, self.h = self.h, None
        if h:
            self.lib.mochi_batcher_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 -- interpreter teardown
            pass


class DeviceSigner:
    """Producer-side SHA256withRSA on the device with one server's private key
    (mochi_signer_*; bit-identical to sign_grants / OpenSSL)."""

    def __init__(self, pem_private_key: bytes, device: int = 0):
        self.lib = load_library()
        self.h = self.lib.mochi_signer_create(int(device), pem_private_key)
        if not self.h:
            raise MochiError(f"mochi_signer_create: {_err(self.lib)}")

    def sign(self, grant_bytes: np.ndarray, grant_off: np.ndarray, grant_len: np.ndarray) -> np.ndarray:
        blob = np.ascontiguousarray(grant_bytes, np.uint8)
        off = np.ascontiguousarray(grant_off, np.uint64)
        ln = np.ascontiguousarray(grant_len, np.uint32)
        n = int(off.shape[0])
        out = np.zeros((n, RSA_BYTES), np.uint8)
        rc = self.lib.mochi_sign_batch(self.h, _ptr(blob), blob.nbytes, _ptr(off), _ptr(ln), n, _ptr(out))
        if rc != OK:
            raise MochiError(f"mochi_sign_batch rc={rc}: {_err(self.lib)}")
        return out

    def sign_device(self, blob_t, off_t, len_t, n: int, sig_t, stream: int = 0) -> None:
        rc = self.lib.mochi_sign_batch_device(self.h, blob_t.data_ptr(), off_t.data_ptr(), len_t.data_ptr(), n,
                                              sig_t.data_ptr(), stream)
        if rc != OK:
            raise MochiError(f"mochi_sign_batch_device rc={rc}: {_err(self.lib)}")

    def rejected(self) -> int:
        """Signatures withheld by the public-key fault check since the last call."""
        v = ctypes.c_uint64()
        if self.lib.mochi_signer_rejected(self.h, ctypes.byref(v)) != OK:
            raise MochiError(f"mochi_signer_rejected: {_err(self.lib)}")
        return v.value

    def set_fault(self, grant_index: int) -> None:
        """Test hook: corrupt one CRT half of grant `grant_index` (-1 = off)."""
        self.lib.mochi_signer_set_fault(self.h, grant_index & 0xFFFFFFFF)

    def issue_device(self, dbatch: "DeviceWrite1Batch", out: "DeviceWrite1Issued", stream: int = 0) -> int:
        """mochi_write1_issue_device: decide, encode and (out.sig given) sign the
        new grants of the batch, everything in device memory.  Returns the rc:
        EINVAL when out.grant_bytes is too small (out.grant_bytes_len = the size
        needed, out.n_new set)."""
        b, o = dbatch.to_c(), out.to_c()
        rc = self.lib.mochi_write1_issue_device(self.h, ctypes.addressof(b), ctypes.addressof(o), stream)
        out.n_new, out.grant_bytes_len = int(o.n_new), int(o.grant_bytes_len)
        if rc != OK and not (rc == EINVAL and out.grant_bytes_len > out.grant_cap):
            raise MochiError(f"mochi_write1_issue_device rc={rc}: {_err(self.lib)}")
        return rc

    def set_profiling(self, on: bool) -> None:
        self.lib.mochi_signer_set_profiling(self.h, 1 if on else 0)

    def read_issue_profile(self) -> dict:
        """Per-kernel device ms of the last issue_device call made while profiling was on."""
        ms = (ctypes.c_float * len(W1_ISSUE_STAGES))()
        if self.lib.mochi_signer_read_issue_profile(self.h, ms, len(W1_ISSUE_STAGES)) != OK:
            raise MochiError(f"mochi_signer_read_issue_profile: {_err(self.lib)}")
        return dict(zip(W1_ISSUE_STAGES, (float(x) for x in ms)))

    def reply_encode_device(self, dbatch: "DeviceWrite1Batch", out: "DeviceWrite1Issued",
                            dsrc: "DeviceWrite1ReplySource", wire, msg_off, msg_len, status, stream: int = 0,
                            wire_len_dev=None, check: bool = True):
        """mochi_write1_reply_encode_device: the reply bodies of the batch `out`
        was issued for, into the uint8 tensor `wire` (None = capacity 0).  May
        follow issue_device on the same stream with no synchronisation.
        wire_len_dev None: the call waits for the total; returns (rc, total),
        rc EINVAL when the total exceeds the capacity (raises then if `check`).
        wire_len_dev an int64 tensor of one element: no host wait, the total
        goes there and nothing is written when it exceeds the capacity;
        returns (rc, None)."""
        b, o, s = dbatch.to_c(), out.to_c(), dsrc.to_c()
        o.n_new, o.grant_bytes_len = out.n_new, out.grant_bytes_len
        cap = 0 if wire is None else int(wire.numel())
        need = ctypes.c_uint64(0)
        rc = self.lib.mochi_write1_reply_encode_device(
            self.h, ctypes.addressof(b), ctypes.addressof(o), ctypes.addressof(s), wire.data_ptr() if cap else None, cap,
            msg_off.data_ptr(), msg_len.data_ptr(), status.data_ptr(),
            ctypes.addressof(need) if wire_len_dev is None else None,
            None if wire_len_dev is None else wire_len_dev.data_ptr(), stream)
        short = wire_len_dev is None and rc == EINVAL and int(need.value) > cap
        if rc != OK and (check or not short):
            raise MochiError(f"mochi_write1_reply_encode_device rc={rc}: {_err(self.lib)}")
        return rc, (int(need.value) if wire_len_dev is None else None)

    def read_reply_profile(self) -> dict:
        """Per-kernel device ms of the last reply_encode_device call made while profiling was on."""
        ms = (ctypes.c_float * len(W1_REPLY_STAGES))()
        if self.lib.mochi_signer_read_reply_profile(self.h, ms, len(W1_REPLY_STAGES)) != OK:
            raise MochiError(f"mochi_signer_read_reply_profile: {_err(self.lib)}")
        return dict(zip(W1_REPLY_STAGES, (float(x) for x in ms)))

    def request_decode_device(self, dreqs: "DeviceWrite1Requests", out: "DeviceWrite1RequestsDecoded", stream: int = 0,
                              check: bool = True) -> int:
        """mochi_write1_request_decode_device: Write1ToServer bodies in device memory to
        the wire half of a Write1 batch with its key numbering, in device memory.  Sets
        out.n_ops (the key count goes to the device word out.n_keys_dev); returns the rc,
        EINVAL when out.op_cap is too small (raises then if `check`)."""
        r, o = dreqs.to_c(), out.to_c()
        rc = self.lib.mochi_write1_request_decode_device(self.h, ctypes.addressof(r), ctypes.addressof(o),
                                                         out.n_keys_dev.data_ptr(), stream)
        out.n_ops = int(o.n_ops)
        short = rc == EINVAL and out.n_ops > out.op_cap
        if rc != OK and (check or not short):
            raise MochiError(f"mochi_write1_request_decode_device rc={rc}: {_err(self.lib)}")
        return rc

    def read_request_profile(self) -> dict:
        """Per-kernel device ms of the last request_decode_device call made while profiling was on."""
        ms = (ctypes.c_float * len(W1_REQUEST_STAGES))()
        if self.lib.mochi_signer_read_request_profile(self.h, ms, len(W1_REQUEST_STAGES)) != OK:
            raise MochiError(f"mochi_signer_read_request_profile: {_err(self.lib)}")
        return dict(zip(W1_REQUEST_STAGES, (float(x) for x in ms)))

    def state_join_device(self, n_reqs: int, n_ops: int, req_op_off, req_seed, op_flags_wire, op_obj,
                          dkeys: "DeviceWrite1KeyState", op_flags, op_epoch, op_stored, stream: int = 0) -> None:
        """mochi_write1_state_join_device over device tensors (op_flags may be op_flags_wire)."""
        k = dkeys.to_c()
        rc = self.lib.mochi_write1_state_join_device(
            self.h, n_reqs, n_ops, req_op_off.data_ptr(), req_seed.data_ptr(), op_flags_wire.data_ptr(),
            op_obj.data_ptr(), ctypes.addressof(k), op_flags.data_ptr(), op_epoch.data_ptr(), op_stored.data_ptr(), stream)
        if rc != OK:
            raise MochiError(f"mochi_write1_state_join_device rc={rc}: {_err(self.lib)}")

    def close(self):
        if self.h:
            self.lib.mochi_signer_destroy(self.h)
            self.h = None


GpuSigner = DeviceSigner

# ---------------------------------------------------------------------------
# Write1 grant issuance (InMemoryDataStore.java:105-155, :233-310): decide,
# encode and sign the grants of a batch of Write1ToServer requests
# ---------------------------------------------------------------------------
W1OP_LOCAL, W1OP_HAS_SVOC, W1OP_WRITE, W1OP_DELETE = 0x01, 0x02, 0x04, 0x08
W1_NONE, W1_STORED = 0xFFFFFFFF, 0x80000000
W1D_SKIP, W1D_SKIPPED, W1D_FAILED, W1D_WRONG_SHARD, W1D_NEW, W1D_RETRY, W1D_REFUSED = range(7)
W1K_OK, W1K_REFUSED, W1K_THROWS = 0, 1, 2
W1_ISSUE_STAGES = ("k_w1_pre", "k_w1_claim", "k_w1_decide", "k_w1_reply_count", "scan", "k_w1_emit", "k_w1_reply_write",
                   "sign")


class Write1Batch_C(ctypes.Structure):
    _fields_ = [("n_reqs", ctypes.c_uint32), ("n_ops", ctypes.c_uint32), ("n_stored", ctypes.c_uint32),
                ("strings", ctypes.c_void_p), ("strings_len", ctypes.c_uint64),
                ("req_op_off", ctypes.c_void_p), ("req_seed", ctypes.c_void_p),
                ("req_hash_off", ctypes.c_void_p), ("req_hash_len", ctypes.c_void_p),
                ("op_key_off", ctypes.c_void_p), ("op_key_len", ctypes.c_void_p),
                ("op_flags", ctypes.c_void_p), ("op_obj", ctypes.c_void_p), ("op_epoch", ctypes.c_void_p),
                ("op_stored", ctypes.c_void_p),
                ("stored_hash_off", ctypes.c_void_p), ("stored_hash_len", ctypes.c_void_p)]


class Write1Issued_C(ctypes.Structure):
    _fields_ = [("op_decision", ctypes.c_void_p), ("op_grant", ctypes.c_void_p), ("req_kind", ctypes.c_void_p),
                ("req_grant_off", ctypes.c_void_p), ("req_grant", ctypes.c_void_p),
                ("n_new", ctypes.c_uint32), ("grant_bytes_len", ctypes.c_uint64),
                ("grant_bytes", ctypes.c_void_p), ("grant_cap", ctypes.c_uint64),
                ("grant_off", ctypes.c_void_p), ("grant_len", ctypes.c_void_p), ("grant_op", ctypes.c_void_p),
                ("grant_ts", ctypes.c_void_p), ("sig", ctypes.c_void_p)]


_W1_OUT_DTYPES = dict(op_decision=np.uint8, op_grant=np.uint32, req_kind=np.uint8, req_grant_off=np.uint32,
                      req_grant=np.uint32, grant_off=np.uint64, grant_len=np.uint32, grant_op=np.uint32,
                      grant_ts=np.int64)


@dataclass
class Write1Batch:
    """SoA batch of Q Write1ToServer requests (mochi_write1_batch, host arrays)."""

    strings: np.ndarray  # uint8: keys and hashes
    req_op_off: np.ndarray  # uint32 [Q+1]
    req_seed: np.ndarray  # uint32 [Q]
    req_hash_off: np.ndarray  # uint64 [Q]
    req_hash_len: np.ndarray  # uint32 [Q]
    op_key_off: np.ndarray  # uint64 [O]
    op_key_len: np.ndarray  # uint32 [O]
    op_flags: np.ndarray  # uint8 [O] W1OP_*
    op_obj: np.ndarray  # uint32 [O]
    op_epoch: np.ndarray  # int64 [O]
    op_stored: np.ndarray  # uint32 [O] stored-grant index or W1_NONE
    stored_hash_off: np.ndarray  # uint64 [S]
    stored_hash_len: np.ndarray  # uint32 [S]

    DTYPES = dict(strings=np.uint8, req_op_off=np.uint32, req_seed=np.uint32, req_hash_off=np.uint64,
                  req_hash_len=np.uint32, op_key_off=np.uint64, op_key_len=np.uint32, op_flags=np.uint8,
                  op_obj=np.uint32, op_epoch=np.int64, op_stored=np.uint32, stored_hash_off=np.uint64,
                  stored_hash_len=np.uint32)

    @property
    def n_reqs(self) -> int:
        return int(self.req_op_off.shape[0]) - 1

    @property
    def n_ops(self) -> int:
        return int(self.op_flags.shape[0])

    @property
    def n_stored(self) -> int:
        return int(self.stored_hash_off.shape[0])

    def arrays(self) -> dict:
        """Every array C-contiguous in its ABI dtype."""
        return {k: np.ascontiguousarray(getattr(self, k), dt).reshape(-1) for k, dt in self.DTYPES.items()}

    def to_c(self):
        arrs = self.arrays()
        c = Write1Batch_C()
        c.n_reqs, c.n_ops, c.n_stored = self.n_reqs, self.n_ops, self.n_stored
        c.strings_len = int(arrs["strings"].nbytes)
        for k, a in arrs.items():
            if a.size == 0:  # an empty array still gets a valid address (the library reads none of it)
                a = arrs[k] = np.zeros(1, a.dtype)
            setattr(c, k, _ptr(a))
        return c, arrs


@dataclass
class Write1Issued:
    """Outputs of write1_issue (mochi_write1_issued), trimmed to their lengths."""

    rc: int
    op_decision: np.ndarray  # uint8 [O] W1D_*
    op_grant: np.ndarray  # uint32 [O]
    req_kind: np.ndarray  # uint8 [Q] W1K_*
    req_grant_off: np.ndarray  # uint32 [Q+1]
    req_grant: np.ndarray  # uint32
    n_new: int
    grant_bytes_len: int
    grant_bytes: np.ndarray  # uint8 (the caller's buffer, whole)
    grant_off: np.ndarray  # uint64 [n_new]
    grant_len: np.ndarray  # uint32 [n_new]
    grant_op: np.ndarray  # uint32 [n_new]
    grant_ts: np.ndarray  # int64 [n_new]
    sig: Optional[np.ndarray] = None  # uint8 [n_new, 256] (device form)

    def grant(self, g: int) -> bytes:
        o = int(self.grant_off[g])
        return self.grant_bytes[o:o + int(self.grant_len[g])].tobytes()


def write1_issue_bound(batch: "Write1Batch") -> int:
    """mochi_write1_issue_bound: a safe (not tight) upper bound on the grant bytes."""
    c, keep = batch.to_c()
    lib = load_library()
    return int(lib.mochi_write1_issue_bound(ctypes.addressof(c)))


def write1_issue_into(batch: "Write1Batch", grant_bytes: Optional[np.ndarray]) -> "Write1Issued":
    """mochi_write1_issue into the caller's buffer (uint8; None = capacity 0).
    rc is EINVAL with grant_bytes_len = the size needed when the buffer is too
    small (no byte of it written); any other failure raises."""
    lib = load_library()
    c, keep = batch.to_c()
    Q, O = batch.n_reqs, batch.n_ops
    n = dict(op_decision=O, op_grant=O, req_kind=Q, req_grant_off=Q + 1, req_grant=O, grant_off=O, grant_len=O,
             grant_op=O, grant_ts=O)
    arr = {k: np.zeros(max(n[k], 1), dt) for k, dt in _W1_OUT_DTYPES.items()}
    o = Write1Issued_C()
    for k, a in arr.items():
        setattr(o, k, _ptr(a))
    cap = 0 if grant_bytes is None else int(grant_bytes.nbytes)
    o.grant_bytes, o.grant_cap = (_ptr(grant_bytes) if cap else None), cap
    need = ctypes.c_uint64(0)
    rc = lib.mochi_write1_issue(ctypes.addressof(c), ctypes.addressof(o), ctypes.addressof(need))
    if rc != OK and not (rc == EINVAL and int(need.value) > cap):
        raise MochiError(f"mochi_write1_issue rc={rc}: {_err(lib)}")
    assert int(need.value) == int(o.grant_bytes_len)
    nn = int(o.n_new) if rc == OK else 0
    nr = int(arr["req_grant_off"][Q]) if rc == OK else 0
    return Write1Issued(rc=rc, op_decision=arr["op_decision"][:O], op_grant=arr["op_grant"][:O],
                        req_kind=arr["req_kind"][:Q], req_grant_off=arr["req_grant_off"][:Q + 1],
                        req_grant=arr["req_grant"][:nr], n_new=int(o.n_new), grant_bytes_len=int(o.grant_bytes_len),
                        grant_bytes=grant_bytes if cap else np.zeros(0, np.uint8), grant_off=arr["grant_off"][:nn],
                        grant_len=arr["grant_len"][:nn], grant_op=arr["grant_op"][:nn], grant_ts=arr["grant_ts"][:nn])


def write1_issue(batch: "Write1Batch") -> "Write1Issued":
    """Host form of Write1 grant issuance: sizes first, then the grants into a
    buffer of exactly the size needed."""
    first = write1_issue_into(batch, None)
    if first.rc == OK:  # no new grant has a byte
        return first
    return write1_issue_into(batch, np.zeros(first.grant_bytes_len, np.uint8))


class DeviceWrite1Batch:
    """A Write1Batch copied into device memory with torch (plumbing only)."""

    def __init__(self, batch: "Write1Batch", device: int = 0):
        import torch

        dev = torch.device("cuda", device)
        sv = {np.uint8: np.uint8, np.uint32: np.int32, np.uint64: np.int64, np.int64: np.int64}
        self.n_reqs, self.n_ops, self.n_stored = batch.n_reqs, batch.n_ops, batch.n_stored
        for k, a in batch.arrays().items():
            if a.size == 0:
                a = np.zeros(1, a.dtype)
            setattr(self, k, torch.from_numpy(a.view(sv[Write1Batch.DTYPES[k]])).to(dev))
        self.strings_len = int(np.asarray(batch.strings).size)

    def to_c(self) -> Write1Batch_C:
        c = Write1Batch_C()
        c.n_reqs, c.n_ops, c.n_stored, c.strings_len = self.n_reqs, self.n_ops, self.n_stored, self.strings_len
        for k in Write1Batch.DTYPES:
            setattr(c, k, getattr(self, k).data_ptr())
        return c


class DeviceWrite1Issued:
    """Device buffers for the outputs of DeviceSigner.issue_device.  grant_cap
    bytes of grant_bytes (prefilled with `fill`), sign=True adds the signature
    rows.  n_new / grant_bytes_len are set by the call."""

    def __init__(self, n_reqs: int, n_ops: int, grant_cap: int, sign: bool = False, device: int = 0, fill: int = 0):
        import torch

        dev = torch.device("cuda", device)
        sv = {np.uint8: torch.uint8, np.uint32: torch.int32, np.uint64: torch.int64, np.int64: torch.int64}
        self.n_reqs, self.n_ops, self.grant_cap = n_reqs, n_ops, int(grant_cap)
        n = dict(op_decision=n_ops, op_grant=n_ops, req_kind=n_reqs, req_grant_off=n_reqs + 1, req_grant=n_ops,
                 grant_off=n_ops, grant_len=n_ops, grant_op=n_ops, grant_ts=n_ops)
        for k, dt in _W1_OUT_DTYPES.items():
            setattr(self, k, torch.zeros(max(n[k], 1), dtype=sv[dt], device=dev))
        self.grant_bytes = torch.full((max(self.grant_cap, 1),), fill, dtype=torch.uint8, device=dev)
        self.sig = torch.zeros((max(n_ops, 1), RSA_BYTES), dtype=torch.uint8, device=dev) if sign else None
        self.n_new = 0
        self.grant_bytes_len = 0

    def to_c(self) -> Write1Issued_C:
        o = Write1Issued_C()
        for k in _W1_OUT_DTYPES:
            setattr(o, k, getattr(self, k).data_ptr())
        o.grant_bytes, o.grant_cap = self.grant_bytes.data_ptr(), self.grant_cap
        o.sig = None if self.sig is None else self.sig.data_ptr()
        return o

    def to_host(self, rc: int = OK) -> "Write1Issued":
        """The outputs on the host, trimmed as write1_issue trims them."""
        Q, O = self.n_reqs, self.n_ops
        h = {k: getattr(self, k).cpu().numpy().view(dt) for k, dt in _W1_OUT_DTYPES.items()}
        nn = self.n_new if rc == OK else 0
        nr = int(h["req_grant_off"][Q]) if rc == OK else 0
        return Write1Issued(rc=rc, op_decision=h["op_decision"][:O], op_grant=h["op_grant"][:O], req_kind=h["req_kind"][:Q],
                            req_grant_off=h["req_grant_off"][:Q + 1], req_grant=h["req_grant"][:nr], n_new=self.n_new,
                            grant_bytes_len=self.grant_bytes_len, grant_bytes=self.grant_bytes.cpu().numpy()[:self.grant_cap],
                            grant_off=h["grant_off"][:nn], grant_len=h["grant_len"][:nn], grant_op=h["grant_op"][:nn],
                            grant_ts=h["grant_ts"][:nn],
                            sig=None if self.sig is None else self.sig.cpu().numpy()[:nn])


# ---------------------------------------------------------------------------
# Write1 reply bodies (InMemoryDataStore.java:283-308): Write1OkFromServer /
# Write1RefusedFromServer from the issue outputs, one blob with offsets
# ---------------------------------------------------------------------------
W1_REPLY_STAGES = ("k_w1r_size", "scan", "k_w1r_hdr", "k_w1r_copy")


class Write1ReplySource_C(ctypes.Structure):
    _fields_ = [("ids", ctypes.c_void_p), ("ids_len", ctypes.c_uint64),
                ("server_id_off", ctypes.c_uint64), ("server_id_len", ctypes.c_uint32),
                ("req_client_off", ctypes.c_void_p), ("req_client_len", ctypes.c_void_p),
                ("stored_bytes", ctypes.c_void_p), ("stored_bytes_len", ctypes.c_uint64),
                ("stored_off", ctypes.c_void_p), ("stored_len", ctypes.c_void_p), ("stored_sig", ctypes.c_void_p),
                ("certs", ctypes.c_void_p), ("certs_len", ctypes.c_uint64),
                ("op_cert_off", ctypes.c_void_p), ("op_cert_len", ctypes.c_void_p)]


@dataclass
class Write1ReplySource:
    """What a Write1 reply needs beyond the batch and the issue outputs
    (mochi_write1_reply_source, host arrays)."""

    ids: np.ndarray  # uint8: the server id and the client ids
    server_id_off: int
    server_id_len: int
    req_client_off: Optional[np.ndarray]  # uint64 [Q] or None = no client ids
    req_client_len: Optional[np.ndarray]  # uint32 [Q]
    stored_bytes: np.ndarray  # uint8: the batch's stored grants
    stored_off: np.ndarray  # uint64 [S]
    stored_len: np.ndarray  # uint32 [S]
    stored_sig: Optional[np.ndarray]  # uint8 [S, 256] or None
    certs: np.ndarray  # uint8: serialized WriteCertificates
    op_cert_off: Optional[np.ndarray]  # uint64 [O] or None = no certificates
    op_cert_len: Optional[np.ndarray]  # uint32 [O] (0 = none for this op)

    DTYPES = dict(ids=np.uint8, req_client_off=np.uint64, req_client_len=np.uint32, stored_bytes=np.uint8,
                  stored_off=np.uint64, stored_len=np.uint32, stored_sig=np.uint8, certs=np.uint8,
                  op_cert_off=np.uint64, op_cert_len=np.uint32)

    def arrays(self) -> dict:
        """Every given array C-contiguous in its ABI dtype (None stays None)."""
        return {k: None if getattr(self, k) is None else np.ascontiguousarray(getattr(self, k), dt).reshape(-1)
                for k, dt in self.DTYPES.items()}

    def to_c(self):
        arrs = self.arrays()
        c = Write1ReplySource_C()
        c.server_id_off, c.server_id_len = int(self.server_id_off), int(self.server_id_len)
        c.ids_len, c.stored_bytes_len, c.certs_len = (int(arrs[k].size) for k in ("ids", "stored_bytes", "certs"))
        for k, a in arrs.items():
            if a is not None and a.size == 0:  # an empty array still gets a valid address
                a = arrs[k] = np.zeros(1, a.dtype)
            setattr(c, k, _ptr(a))
        return c, arrs


def _issued_c(issued: "Write1Issued"):
    """mochi_write1_issued over the host arrays of a Write1Issued (reply encoder input)."""
    o = Write1Issued_C()
    keep = {}
    for k, dt in _W1_OUT_DTYPES.items():
        a = np.ascontiguousarray(getattr(issued, k), dt).reshape(-1)
        keep[k] = a if a.size else np.zeros(1, dt)
        setattr(o, k, _ptr(keep[k]))
    gb = np.ascontiguousarray(issued.grant_bytes, np.uint8).reshape(-1)
    keep["grant_bytes"] = gb if gb.size else np.zeros(1, np.uint8)
    o.grant_bytes, o.grant_cap = _ptr(keep["grant_bytes"]), int(gb.size)
    o.n_new, o.grant_bytes_len = int(issued.n_new), int(issued.grant_bytes_len)
    if issued.sig is not None:
        sg = np.ascontiguousarray(issued.sig, np.uint8).reshape(-1)
        keep["sig"] = sg if sg.size else np.zeros(RSA_BYTES, np.uint8)
        o.sig = _ptr(keep["sig"])
    return o, keep


def write1_reply_bound(batch, src, grant_bytes_len: int, with_signatures: bool) -> int:
    """mochi_write1_reply_bound: a safe (not tight) upper bound on the reply bytes
    of a batch whose new grants take at most grant_bytes_len bytes (after the
    issue call its grant_bytes_len; before it, write1_issue_bound).  `batch` and
    `src` may be the host or the device classes."""
    lib = load_library()
    size = lambda o, k: int(getattr(o, k + "_len")) if hasattr(o, k + "_len") else int(np.asarray(getattr(o, k)).size)
    return int(lib.mochi_write1_reply_bound(
        batch.n_reqs, batch.n_ops, size(batch, "strings"), size(src, "ids"), int(grant_bytes_len),
        size(src, "stored_bytes"), size(src, "certs") if src.op_cert_off is not None else 0, 1 if with_signatures else 0))


def write1_reply_encode_into(batch: "Write1Batch", issued: "Write1Issued", src: "Write1ReplySource",
                             wire: Optional[np.ndarray]):
    """mochi_write1_reply_encode into the caller's buffer (uint8; None = capacity
    0).  Returns (rc, wire_len, msg_off, msg_len, status); rc is EINVAL with
    wire_len = the size needed when the buffer is too small (no byte of it
    written); any other failure raises."""
    lib = load_library()
    b, keep_b = batch.to_c()
    o, keep_o = _issued_c(issued)
    s, keep_s = src.to_c()
    Q = batch.n_reqs
    off, ln, st = np.zeros(max(Q, 1), np.uint64), np.zeros(max(Q, 1), np.uint32), np.zeros(max(Q, 1), np.uint8)
    cap = 0 if wire is None else int(wire.nbytes)
    need = ctypes.c_uint64(0)
    rc = lib.mochi_write1_reply_encode(ctypes.addressof(b), ctypes.addressof(o), ctypes.addressof(s),
                                       _ptr(wire) if cap else None, cap, _ptr(off), _ptr(ln), _ptr(st),
                                       ctypes.addressof(need))
    if rc != OK and not (rc == EINVAL and int(need.value) > cap):
        raise MochiError(f"mochi_write1_reply_encode rc={rc}: {_err(lib)}")
    return rc, int(need.value), off[:Q], ln[:Q], st[:Q]


def write1_reply_encode(batch: "Write1Batch", issued: "Write1Issued", src: "Write1ReplySource"):
    """Host form of the Write1 reply encoder: sizes first, then the bodies into
    a buffer of exactly the size needed.  Returns (wire, msg_off, msg_len, status)."""
    rc, need, off, ln, st = write1_reply_encode_into(batch, issued, src, None)
    wire = np.zeros(need, np.uint8)
    if need:
        rc, need, off, ln, st = write1_reply_encode_into(batch, issued, src, wire)
    assert rc == OK
    return wire, off, ln, st


class DeviceWrite1ReplySource:
    """A Write1ReplySource copied into device memory with torch (plumbing only)."""

    def __init__(self, src: "Write1ReplySource", device: int = 0):
        import torch

        dev = torch.device("cuda", device)
        sv = {np.uint8: np.uint8, np.uint32: np.int32, np.uint64: np.int64}
        self.server_id_off, self.server_id_len = int(src.server_id_off), int(src.server_id_len)
        for k, a in src.arrays().items():
            if a is not None:
                if k in ("ids", "stored_bytes", "certs"):
                    setattr(self, k + "_len", int(a.size))
                a = torch.from_numpy((a if a.size else np.zeros(1, a.dtype)).view(sv[Write1ReplySource.DTYPES[k]])).to(dev)
            setattr(self, k, a)

    @classmethod
    def from_tensors(cls, server_id_off: int, server_id_len: int, **tensors) -> "DeviceWrite1ReplySource":
        """Arrays already on the device (uint64 as int64, uint32 as int32); absent = None."""
        self = cls.__new__(cls)
        self.server_id_off, self.server_id_len = int(server_id_off), int(server_id_len)
        for k in Write1ReplySource.DTYPES:
            t = tensors.get(k)
            setattr(self, k, t)
            if k in ("ids", "stored_bytes", "certs"):
                setattr(self, k + "_len", 0 if t is None else int(t.numel()))
        return self

    def to_c(self) -> Write1ReplySource_C:
        c = Write1ReplySource_C()
        c.server_id_off, c.server_id_len = self.server_id_off, self.server_id_len
        c.ids_len, c.stored_bytes_len, c.certs_len = self.ids_len, self.stored_bytes_len, self.certs_len
        for k in Write1ReplySource.DTYPES:
            t = getattr(self, k)
            setattr(c, k, None if t is None else t.data_ptr())
        return c



# ---------------------------------------------------------------------------
# Write1 reply decode (the client's round): Write1OkFromServer /
# Write1RefusedFromServer bodies -> the arrays write1_classify and Write2Source read
# ---------------------------------------------------------------------------
W1R_OK, W1R_MALFORMED, W1R_FALLBACK, W1R_UNKNOWN_SERVER = range(4)
W1G_HAS_SIG, W1G_KEY_DIFFERS = 0x01, 0x02
W1_DECODE_STAGES = ("k_w1d_resp", "entry_scan", "k_w1d_level2", "final_scan_offsets", "k_w1d_emit", "signatures")


class Write1Replies_C(ctypes.Structure):
    _fields_ = [("n_resps", ctypes.c_uint32), ("n_reqs", ctypes.c_uint32), ("n_ops", ctypes.c_uint32),
                ("_pad0", ctypes.c_uint32), ("wire", ctypes.c_void_p), ("wire_len", ctypes.c_uint64),
                ("resp_off", ctypes.c_void_p), ("resp_len", ctypes.c_void_p), ("resp_kind", ctypes.c_void_p),
                ("req_resp_off", ctypes.c_void_p), ("strings", ctypes.c_void_p), ("strings_len", ctypes.c_uint64),
                ("req_op_off", ctypes.c_void_p), ("op_key_off", ctypes.c_void_p), ("op_key_len", ctypes.c_void_p)]


class Write1Decoded_C(ctypes.Structure):
    _fields_ = [("resp_status", ctypes.c_void_p), ("resp_kind_out", ctypes.c_void_p), ("resp_server", ctypes.c_void_p),
                ("mg_signer", ctypes.c_void_p), ("resp_client_off", ctypes.c_void_p),
                ("resp_client_len", ctypes.c_void_p), ("resp_grant_off", ctypes.c_void_p),
                ("resp_cert_off", ctypes.c_void_p), ("n_grants", ctypes.c_uint32), ("n_certs", ctypes.c_uint32),
                ("grant_cap", ctypes.c_uint32), ("cert_cap", ctypes.c_uint32), ("grant_off", ctypes.c_void_p),
                ("grant_len", ctypes.c_void_p), ("grant_key", ctypes.c_void_p), ("grant_ts", ctypes.c_void_p),
                ("grant_status", ctypes.c_void_p), ("grant_flags", ctypes.c_void_p), ("sig", ctypes.c_void_p),
                ("cert_key_off", ctypes.c_void_p), ("cert_key_len", ctypes.c_void_p),
                ("cert_val_off", ctypes.c_void_p), ("cert_val_len", ctypes.c_void_p)]


# output arrays by what they are indexed with: "P" responses, "P1" the CSRs, "N" grants, "C" certificates
_W1D_OUT = dict(resp_status=(np.uint8, "P"), resp_kind_out=(np.uint8, "P"), resp_server=(np.uint32, "P"),
                mg_signer=(np.uint16, "P"), resp_client_off=(np.uint64, "P"), resp_client_len=(np.uint32, "P"),
                resp_grant_off=(np.uint32, "P1"), resp_cert_off=(np.uint32, "P1"),
                grant_off=(np.uint64, "N"), grant_len=(np.uint32, "N"), grant_key=(np.uint8, "N"),
                grant_ts=(np.int64, "N"), grant_status=(np.uint8, "N"), grant_flags=(np.uint8, "N"),
                cert_key_off=(np.uint64, "C"), cert_key_len=(np.uint32, "C"), cert_val_off=(np.uint64, "C"),
                cert_val_len=(np.uint32, "C"))


@dataclass
class Write1Replies:
    """The Write1 reply bodies a client received (mochi_write1_replies, host arrays)."""

    wire: np.ndarray  # uint8
    resp_off: np.ndarray  # uint64 [P]
    resp_len: np.ndarray  # uint32 [P]
    resp_kind: np.ndarray  # uint8 [P] W1_*
    req_resp_off: np.ndarray  # uint32 [Q+1]
    strings: np.ndarray  # uint8: the operands the client sent
    req_op_off: np.ndarray  # uint32 [Q+1]
    op_key_off: np.ndarray  # uint64 [O]
    op_key_len: np.ndarray  # uint32 [O]

    DTYPES = dict(wire=np.uint8, resp_off=np.uint64, resp_len=np.uint32, resp_kind=np.uint8, req_resp_off=np.uint32,
                  strings=np.uint8, req_op_off=np.uint32, op_key_off=np.uint64, op_key_len=np.uint32)

    @property
    def n_resps(self) -> int:
        return int(np.asarray(self.resp_off).shape[0])

    @property
    def n_reqs(self) -> int:
        return int(np.asarray(self.req_resp_off).shape[0]) - 1

    @property
    def n_ops(self) -> int:
        return int(np.asarray(self.op_key_off).shape[0])

    def arrays(self) -> dict:
        return {k: np.ascontiguousarray(getattr(self, k), dt).reshape(-1) for k, dt in self.DTYPES.items()}

    def to_c(self):
        arrs = self.arrays()
        c = Write1Replies_C()
        c.n_resps, c.n_reqs, c.n_ops = self.n_resps, self.n_reqs, self.n_ops
        c.wire_len, c.strings_len = int(arrs["wire"].size), int(arrs["strings"].size)
        for k, a in arrs.items():
            if a.size == 0:  # an empty array still gets a valid address
                a = arrs[k] = np.zeros(1, a.dtype)
            setattr(c, k, _ptr(a))
        return c, arrs


@dataclass
class Write1Decoded:
    """Outputs of write1_reply_decode (mochi_write1_decoded): the caller's buffers, whole
    (n_grants / n_certs say how much of the per-grant / per-certificate ones is meant)."""

    rc: int
    n_grants: int
    n_certs: int
    arrays: dict  # name -> array, names as in mochi_write1_decoded; "sig" [cap, 256] or absent

    def __getattr__(self, k):
        try:
            return self.__dict__["arrays"][k]
        except KeyError:
            raise AttributeError(k)

    def trimmed(self) -> dict:
        """Every array cut to its meaning (per-grant / per-certificate ones to 0 unless rc is OK)."""
        P = self.arrays["resp_status"].shape[0]
        n = dict(P=P, P1=P + 1, N=self.n_grants if self.rc == OK else 0, C=self.n_certs if self.rc == OK else 0)
        out = {k: self.arrays[k][:n[w]] for k, (dt, w) in _W1D_OUT.items()}
        if "sig" in self.arrays:
            out["sig"] = self.arrays["sig"][:n["N"]]
        return out


def write1_reply_decode_bound(wire_len: int, n_resps: int):
    """mochi_write1_reply_decode_bound: safe (grant, certificate) capacities."""
    g, c = ctypes.c_uint64(0), ctypes.c_uint64(0)
    load_library().mochi_write1_reply_decode_bound(int(wire_len), int(n_resps), ctypes.addressof(g), ctypes.addressof(c))
    return int(g.value), int(c.value)


def write1_reply_decode_into(replies: "Write1Replies", server_ids, grant_cap: int, cert_cap: int, want_sig: bool = True,
                             fill: int = 0) -> "Write1Decoded":
    """mochi_write1_reply_decode into buffers of the given capacities, prefilled with
    `fill`.  rc is EINVAL with n_grants / n_certs = the counts needed when one is too
    small (no per-grant or per-certificate array touched); any other failure raises."""
    lib = load_library()
    r, keep = replies.to_c()
    ids, id_off, n_ids = _id_table(server_ids)
    P = replies.n_resps
    n = dict(P=P, P1=P + 1, N=int(grant_cap), C=int(cert_cap))
    arr = {k: np.full(n[w] * np.dtype(dt).itemsize, fill, np.uint8).view(dt) for k, (dt, w) in _W1D_OUT.items()}
    if want_sig:
        arr["sig"] = np.full((int(grant_cap), RSA_BYTES), fill, np.uint8)
    o = Write1Decoded_C()
    for k, a in arr.items():
        setattr(o, k, _ptr(a) if a.size else None)
    o.grant_cap, o.cert_cap = int(grant_cap), int(cert_cap)
    rc = lib.mochi_write1_reply_decode(ctypes.addressof(r), _ptr(ids), _ptr(id_off), n_ids, ctypes.addressof(o))
    if rc != OK and not (rc == EINVAL and (o.n_grants > grant_cap or o.n_certs > cert_cap)):
        raise MochiError(f"mochi_write1_reply_decode rc={rc}: {_err(lib)}")
    return Write1Decoded(rc=rc, n_grants=int(o.n_grants), n_certs=int(o.n_certs), arrays=arr)


def write1_reply_decode(replies: "Write1Replies", server_ids, want_sig: bool = True) -> "Write1Decoded":
    """Host form of the Write1 reply decoder: counts first, then into buffers of exactly
    the sizes needed."""
    first = write1_reply_decode_into(replies, server_ids, 0, 0, want_sig)
    if first.rc == OK:
        return first
    return write1_reply_decode_into(replies, server_ids, first.n_grants, first.n_certs, want_sig)


class DeviceWrite1Replies:
    """A Write1Replies copied into device memory with torch (plumbing only)."""

    def __init__(self, replies: "Write1Replies", device: int = 0):
        import torch

        dev = torch.device("cuda", device)
        sv = {np.uint8: np.uint8, np.uint32: np.int32, np.uint64: np.int64}
        t = {k: torch.from_numpy((a if a.size else np.zeros(1, a.dtype)).view(sv[Write1Replies.DTYPES[k]])).to(dev)
             for k, a in replies.arrays().items()}
        self._set(replies.n_resps, replies.n_reqs, replies.n_ops, int(np.asarray(replies.wire).size),
                  int(np.asarray(replies.strings).size), t)

    def _set(self, P, Q, O, wire_len, strings_len, tensors):
        self.n_resps, self.n_reqs, self.n_ops, self.wire_len, self.strings_len = int(P), int(Q), int(O), int(wire_len), \
            int(strings_len)
        for k in Write1Replies.DTYPES:
            setattr(self, k, tensors[k])

    @classmethod
    def from_tensors(cls, n_resps: int, n_reqs: int, n_ops: int, **tensors) -> "DeviceWrite1Replies":
        """Arrays already on the device (uint64 as int64, uint32 as int32), used as they are."""
        self = cls.__new__(cls)
        self._set(n_resps, n_reqs, n_ops, tensors["wire"].numel(), tensors["strings"].numel(), tensors)
        return self

    def to_c(self) -> Write1Replies_C:
        c = Write1Replies_C()
        c.n_resps, c.n_reqs, c.n_ops = self.n_resps, self.n_reqs, self.n_ops
        c.wire_len, c.strings_len = self.wire_len, self.strings_len
        for k in Write1Replies.DTYPES:
            setattr(c, k, getattr(self, k).data_ptr())
        return c


class DeviceWrite1Decoded:
    """Device buffers for the outputs of Verifier.write1_reply_decode_device, prefilled with
    `fill`; n_grants / n_certs are set by the call.  Tensors carry the ABI widths (uint16 as
    int16, uint32 as int32, uint64 as int64)."""

    def __init__(self, n_resps: int, grant_cap: int, cert_cap: int, want_sig: bool = True, device: int = 0,
                 fill: int = 0):
        import torch

        dev = torch.device("cuda", device)
        sv = {np.uint8: torch.uint8, np.uint16: torch.int16, np.uint32: torch.int32, np.uint64: torch.int64,
              np.int64: torch.int64}
        self.n_resps, self.grant_cap, self.cert_cap = int(n_resps), int(grant_cap), int(cert_cap)
        n = dict(P=self.n_resps, P1=self.n_resps + 1, N=self.grant_cap, C=self.cert_cap)
        pat = lambda dt: int.from_bytes(bytes([fill & 0xFF]) * np.dtype(dt).itemsize, "little", signed=dt != np.uint8)
        for k, (dt, w) in _W1D_OUT.items():
            setattr(self, k, torch.full((max(n[w], 1),), pat(dt), dtype=sv[dt], device=dev))
        self.sig = torch.full((max(self.grant_cap, 1), RSA_BYTES), fill & 0xFF, dtype=torch.uint8, device=dev) \
            if want_sig else None
        self.n_grants = self.n_certs = 0

    def to_c(self) -> Write1Decoded_C:
        o = Write1Decoded_C()
        for k in _W1D_OUT:
            setattr(o, k, getattr(self, k).data_ptr())
        o.sig = None if self.sig is None else self.sig.data_ptr()
        o.grant_cap, o.cert_cap = self.grant_cap, self.cert_cap
        return o

    def to_host(self, rc: int = OK) -> "Write1Decoded":
        """The buffers on the host, whole (as write1_reply_decode_into returns them)."""
        n = dict(P=self.n_resps, P1=self.n_resps + 1, N=self.grant_cap, C=self.cert_cap)
        arr = {k: getattr(self, k).cpu().numpy().view(dt)[:n[w]] for k, (dt, w) in _W1D_OUT.items()}
        if self.sig is not None:
            arr["sig"] = self.sig.cpu().numpy()[:self.grant_cap]
        return Write1Decoded(rc=rc, n_grants=self.n_grants, n_certs=self.n_certs, arrays=arr)


# ---------------------------------------------------------------------------
# Write1 request decode (the server's side of the round): Write1ToServer bodies ->
# the wire half of a Write1Batch with its batch-wide key numbering; the key-state join
# ---------------------------------------------------------------------------
W1Q_OK, W1Q_MALFORMED, W1Q_FALLBACK = range(3)
W1_REQUEST_STAGES = ("k_w1q_req", "entry_scan", "k_w1q_ops", "final_scan_offsets", "k_w1q_emit", "k_w1q_claim",
                     "k_w1q_rank", "key_scan", "k_w1q_number")


class Write1Requests_C(ctypes.Structure):
    _fields_ = [("n_reqs", ctypes.c_uint32), ("_pad0", ctypes.c_uint32), ("wire", ctypes.c_void_p),
                ("wire_len", ctypes.c_uint64), ("msg_off", ctypes.c_void_p), ("msg_len", ctypes.c_void_p)]


class Write1RequestsDecoded_C(ctypes.Structure):
    _fields_ = [("req_status", ctypes.c_void_p), ("req_seed", ctypes.c_void_p), ("req_hash_off", ctypes.c_void_p),
                ("req_hash_len", ctypes.c_void_p), ("req_client_off", ctypes.c_void_p),
                ("req_client_len", ctypes.c_void_p), ("req_op_off", ctypes.c_void_p),
                ("n_ops", ctypes.c_uint32), ("n_keys", ctypes.c_uint32), ("op_cap", ctypes.c_uint32),
                ("_pad0", ctypes.c_uint32), ("op_key_off", ctypes.c_void_p), ("op_key_len", ctypes.c_void_p),
                ("op_flags", ctypes.c_void_p), ("op_obj", ctypes.c_void_p), ("key_op", ctypes.c_void_p)]


class Write1KeyState_C(ctypes.Structure):
    _fields_ = [("n_keys", ctypes.c_uint32), ("n_given", ctypes.c_uint32), ("key_flags", ctypes.c_void_p),
                ("key_epoch", ctypes.c_void_p), ("key_given_off", ctypes.c_void_p), ("given_ts", ctypes.c_void_p),
                ("given_stored", ctypes.c_void_p)]


# output arrays by what they are indexed with: "Q" requests, "Q1" the CSR, "O" ops, "K" key_op (op_cap entries)
_W1Q_OUT = dict(req_status=(np.uint8, "Q"), req_seed=(np.uint32, "Q"), req_hash_off=(np.uint64, "Q"),
                req_hash_len=(np.uint32, "Q"), req_client_off=(np.uint64, "Q"), req_client_len=(np.uint32, "Q"),
                req_op_off=(np.uint32, "Q1"), op_key_off=(np.uint64, "O"), op_key_len=(np.uint32, "O"),
                op_flags=(np.uint8, "O"), op_obj=(np.uint32, "O"), key_op=(np.uint32, "K"))


@dataclass
class Write1Requests:
    """The Write1ToServer bodies a server received (mochi_write1_requests, host arrays)."""

    wire: np.ndarray  # uint8
    msg_off: np.ndarray  # uint64 [Q]
    msg_len: np.ndarray  # uint32 [Q]

    DTYPES = dict(wire=np.uint8, msg_off=np.uint64, msg_len=np.uint32)

    @property
    def n_reqs(self) -> int:
        return int(np.asarray(self.msg_off).shape[0])

    def arrays(self) -> dict:
        return {k: np.ascontiguousarray(getattr(self, k), dt).reshape(-1) for k, dt in self.DTYPES.items()}

    def to_c(self):
        arrs = self.arrays()
        c = Write1Requests_C()
        c.n_reqs, c.wire_len = self.n_reqs, int(arrs["wire"].size)
        for k, a in arrs.items():
            if a.size == 0:  # an empty array still gets a valid address
                a = arrs[k] = np.zeros(1, a.dtype)
            setattr(c, k, _ptr(a))
        return c, arrs


@dataclass
class Write1RequestsDecoded:
    """Outputs of write1_request_decode (mochi_write1_requests_decoded): the caller's buffers,
    whole (n_ops / n_keys say how much of the per-op ones / of key_op is meant)."""

    rc: int
    n_ops: int
    n_keys: int
    arrays: dict  # name -> array, names as in mochi_write1_requests_decoded

    def __getattr__(self, k):
        try:
            return self.__dict__["arrays"][k]
        except KeyError:
            raise AttributeError(k)

    def trimmed(self) -> dict:
        """Every array cut to its meaning (per-op ones and key_op to 0 unless rc is OK)."""
        Q = self.arrays["req_status"].shape[0]
        ok = self.rc == OK
        n = dict(Q=Q, Q1=Q + 1, O=self.n_ops if ok else 0, K=self.n_keys if ok else 0)
        return {k: self.arrays[k][:n[w]] for k, (dt, w) in _W1Q_OUT.items()}


def write1_request_decode_bound(wire_len: int, n_reqs: int) -> int:
    """mochi_write1_request_decode_bound: a safe op_cap."""
    return int(load_library().mochi_write1_request_decode_bound(int(wire_len), int(n_reqs)))


def write1_request_decode_into(reqs: "Write1Requests", op_cap: int, fill: int = 0) -> "Write1RequestsDecoded":
    """mochi_write1_request_decode into buffers of the given capacity, prefilled with `fill`.
    rc is EINVAL with n_ops = the count needed when it is too small (no per-op array
    touched); any other failure raises."""
    lib = load_library()
    r, keep = reqs.to_c()
    Q = reqs.n_reqs
    n = dict(Q=Q, Q1=Q + 1, O=int(op_cap), K=int(op_cap))
    arr = {k: np.full(n[w] * np.dtype(dt).itemsize, fill, np.uint8).view(dt) for k, (dt, w) in _W1Q_OUT.items()}
    o = Write1RequestsDecoded_C()
    for k, a in arr.items():
        setattr(o, k, _ptr(a) if a.size else None)
    o.op_cap = int(op_cap)
    rc = lib.mochi_write1_request_decode(ctypes.addressof(r), ctypes.addressof(o))
    if rc != OK and not (rc == EINVAL and o.n_ops > op_cap):
        raise MochiError(f"mochi_write1_request_decode rc={rc}: {_err(lib)}")
    return Write1RequestsDecoded(rc=rc, n_ops=int(o.n_ops), n_keys=int(o.n_keys), arrays=arr)


def write1_request_decode(reqs: "Write1Requests") -> "Write1RequestsDecoded":
    """Host form of the Write1 request decoder: the count first, then into buffers of
    exactly the size needed."""
    first = write1_request_decode_into(reqs, 0)
    if first.rc == OK:
        return first
    return write1_request_decode_into(reqs, first.n_ops)


@dataclass
class Write1KeyState:
    """The store's state per distinct key of a decoded batch (mochi_write1_key_state, host arrays)."""

    key_flags: np.ndarray  # uint8 [U] W1OP_LOCAL | W1OP_HAS_SVOC
    key_epoch: np.ndarray  # int64 [U]
    key_given_off: np.ndarray  # uint32 [U+1]
    given_ts: np.ndarray  # int64 [G]
    given_stored: np.ndarray  # uint32 [G]

    DTYPES = dict(key_flags=np.uint8, key_epoch=np.int64, key_given_off=np.uint32, given_ts=np.int64,
                  given_stored=np.uint32)

    def arrays(self) -> dict:
        return {k: np.ascontiguousarray(getattr(self, k), dt).reshape(-1) for k, dt in self.DTYPES.items()}

    def to_c(self):
        arrs = self.arrays()
        c = Write1KeyState_C()
        c.n_keys, c.n_given = int(arrs["key_flags"].size), int(arrs["given_ts"].size)
        for k, a in arrs.items():
            if a.size == 0:
                a = arrs[k] = np.zeros(1, a.dtype)
            setattr(c, k, _ptr(a))
        return c, arrs


def write1_state_join(req_op_off, req_seed, op_flags_wire, op_obj, keys: "Write1KeyState"):
    """mochi_write1_state_join: (op_flags, op_epoch, op_stored) of a decoded batch."""
    lib = load_library()
    off = np.ascontiguousarray(req_op_off, np.uint32)
    seed = np.ascontiguousarray(req_seed, np.uint32)
    fw = np.ascontiguousarray(op_flags_wire, np.uint8)
    obj = np.ascontiguousarray(op_obj, np.uint32)
    Q, O = int(off.size) - 1, int(obj.size)
    k, keep = keys.to_c()
    fl, ep, st = np.zeros(max(O, 1), np.uint8), np.zeros(max(O, 1), np.int64), np.zeros(max(O, 1), np.uint32)
    pad = lambda a: a if a.size else np.zeros(1, a.dtype)
    rc = lib.mochi_write1_state_join(Q, O, _ptr(off), _ptr(pad(seed)), _ptr(pad(fw)), _ptr(pad(obj)), ctypes.addressof(k),
                                     _ptr(fl), _ptr(ep), _ptr(st))
    if rc != OK:
        raise MochiError(f"mochi_write1_state_join rc={rc}: {_err(lib)}")
    return fl[:O], ep[:O], st[:O]


def _to_dev(a: np.ndarray, device: int):
    import torch

    sv = {np.dtype(np.uint8): np.uint8, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64,
          np.dtype(np.int64): np.int64}
    a = a if a.size else np.zeros(1, a.dtype)
    a = a if a.flags.writeable else a.copy()  # torch refuses a read-only view (np.frombuffer)
    return torch.from_numpy(a.view(sv[a.dtype])).to(torch.device("cuda", device))


class DeviceWrite1Requests:
    """A Write1Requests copied into device memory with torch (plumbing only)."""

    def __init__(self, reqs: "Write1Requests", device: int = 0):
        a = reqs.arrays()
        self._set(reqs.n_reqs, int(a["wire"].size), {k: _to_dev(v, device) for k, v in a.items()})

    def _set(self, Q, wire_len, tensors):
        self.n_reqs, self.wire_len = int(Q), int(wire_len)
        for k in Write1Requests.DTYPES:
            setattr(self, k, tensors[k])

    @classmethod
    def from_tensors(cls, n_reqs: int, **tensors) -> "DeviceWrite1Requests":
        """Arrays already on the device (uint64 as int64, uint32 as int32), used as they are."""
        self = cls.__new__(cls)
        self._set(n_reqs, tensors["wire"].numel(), tensors)
        return self

    def to_c(self) -> Write1Requests_C:
        c = Write1Requests_C()
        c.n_reqs, c.wire_len = self.n_reqs, self.wire_len
        for k in Write1Requests.DTYPES:
            setattr(c, k, getattr(self, k).data_ptr())
        return c


class DeviceWrite1RequestsDecoded:
    """Device buffers for the outputs of DeviceSigner.request_decode_device, prefilled with
    `fill`; n_ops is set by the call, the key count lands in the device word n_keys_dev.
    Tensors carry the ABI widths (uint32 as int32, uint64 as int64)."""

    def __init__(self, n_reqs: int, op_cap: int, device: int = 0, fill: int = 0):
        import torch

        dev = torch.device("cuda", device)
        sv = {np.uint8: torch.uint8, np.uint32: torch.int32, np.uint64: torch.int64}
        self.n_reqs, self.op_cap = int(n_reqs), int(op_cap)
        n = dict(Q=self.n_reqs, Q1=self.n_reqs + 1, O=self.op_cap, K=self.op_cap)
        pat = lambda dt: int.from_bytes(bytes([fill & 0xFF]) * np.dtype(dt).itemsize, "little", signed=dt != np.uint8)
        for k, (dt, w) in _W1Q_OUT.items():
            setattr(self, k, torch.full((max(n[w], 1),), pat(dt), dtype=sv[dt], device=dev))
        self.n_keys_dev = torch.full((1,), pat(np.uint32), dtype=torch.int32, device=dev)
        self.n_ops = 0

    def to_c(self) -> Write1RequestsDecoded_C:
        o = Write1RequestsDecoded_C()
        for k in _W1Q_OUT:
            setattr(o, k, getattr(self, k).data_ptr())
        o.op_cap = self.op_cap
        return o

    def n_keys(self) -> int:
        """The key count (a device read: synchronises)."""
        return int(self.n_keys_dev.cpu().numpy().view(np.uint32)[0])

    def to_host(self, rc: int = OK) -> "Write1RequestsDecoded":
        """The buffers on the host, whole (as write1_request_decode_into returns them)."""
        n = dict(Q=self.n_reqs, Q1=self.n_reqs + 1, O=self.op_cap, K=self.op_cap)
        arr = {k: getattr(self, k).cpu().numpy().view(dt)[:n[w]] for k, (dt, w) in _W1Q_OUT.items()}
        return Write1RequestsDecoded(rc=rc, n_ops=self.n_ops, n_keys=self.n_keys(), arrays=arr)


class DeviceWrite1KeyState:
    """A Write1KeyState copied into device memory with torch (plumbing only)."""

    def __init__(self, keys: "Write1KeyState", device: int = 0):
        a = keys.arrays()
        self.n_keys, self.n_given = int(a["key_flags"].size), int(a["given_ts"].size)
        for k, v in a.items():
            setattr(self, k, _to_dev(v, device))

    def to_c(self) -> Write1KeyState_C:
        c = Write1KeyState_C()
        c.n_keys, c.n_given = self.n_keys, self.n_given
        for k in Write1KeyState.DTYPES:
            setattr(c, k, getattr(self, k).data_ptr())
        return c


# ---------------------------------------------------------------------------
# Result reply decode (the client's closing round): Write2AnsFromServer / ReadFromServer
# bodies -> the arrays tally_responses reads and the per-op values it coalesces
# ---------------------------------------------------------------------------
RR_WRITE2_ANS, RR_READ, RR_OTHER = range(3)
RRS_OK, RRS_MALFORMED, RRS_FALLBACK = range(3)
RRO_HAS_CERT = 0x01
RR_UNDECODED = 0xFFFFFFFF  # resp_n_ops of a MALFORMED / FALLBACK response
RESULT_DECODE_STAGES = ("k_rr_resp", "op_scan", "k_rr_ops", "k_rr_final")


class ResultReplies_C(ctypes.Structure):
    _fields_ = [("n_resps", ctypes.c_uint32), ("n_reqs", ctypes.c_uint32), ("wire", ctypes.c_void_p),
                ("wire_len", ctypes.c_uint64), ("resp_off", ctypes.c_void_p), ("resp_len", ctypes.c_void_p),
                ("resp_kind", ctypes.c_void_p), ("req_resp_off", ctypes.c_void_p), ("n_ops", ctypes.c_void_p),
                ("slot_off", ctypes.c_void_p)]


# output arrays by what they are indexed with: "P" responses, "S" slots
_RR_OUT = dict(resp_status=(np.uint8, "P"), resp_n_ops=(np.uint32, "P"), resp_rid_off=(np.uint64, "P"),
               resp_rid_len=(np.uint32, "P"), resp_nonce_off=(np.uint64, "P"), resp_nonce_len=(np.uint32, "P"),
               op_status=(np.uint8, "S"), op_existed=(np.uint8, "S"), op_flags=(np.uint8, "S"),
               op_result_off=(np.uint64, "S"), op_result_len=(np.uint32, "S"), op_cert_off=(np.uint64, "S"),
               op_cert_len=(np.uint32, "S"))
_RR_SLOT = tuple(k for k, (dt, w) in _RR_OUT.items() if w == "S")
# the coalesced outputs, one entry per (request, op)
_RC_OUT = dict(resp=np.uint32, status=np.uint8, existed=np.uint8, flags=np.uint8, result_off=np.uint64,
               result_len=np.uint32, cert_off=np.uint64, cert_len=np.uint32)


class ResultDecoded_C(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in _RR_OUT]


class ResultTallied_C(ctypes.Structure):
    _fields_ = [("n_reqs", ctypes.c_uint32), ("_pad0", ctypes.c_uint32)] + \
        [(k, ctypes.c_void_p) for k in ("req_resp_off", "n_ops", "chosen", "chosen_off", "accept_bits", "slot_off") +
         _RR_SLOT + ("out_off",)]


class ResultCoalesced_C(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in _RC_OUT]


@dataclass
class ResultReplies:
    """The answers a client received in its closing round (mochi_result_replies, host arrays)."""

    wire: np.ndarray  # uint8
    resp_off: np.ndarray  # uint64 [P]
    resp_len: np.ndarray  # uint32 [P]
    resp_kind: np.ndarray  # uint8 [P] RR_*
    req_resp_off: np.ndarray  # uint32 [Q+1]
    n_ops: np.ndarray  # uint32 [Q]
    slot_off: np.ndarray  # uint64 [P]

    DTYPES = dict(wire=np.uint8, resp_off=np.uint64, resp_len=np.uint32, resp_kind=np.uint8, req_resp_off=np.uint32,
                  n_ops=np.uint32, slot_off=np.uint64)

    @property
    def n_resps(self) -> int:
        return int(np.asarray(self.resp_off).shape[0])

    @property
    def n_reqs(self) -> int:
        return int(np.asarray(self.n_ops).shape[0])

    @property
    def n_slots(self) -> int:
        """Entries the per-slot arrays need: the end of the furthest slot run."""
        if not self.n_resps:
            return 0
        per = np.repeat(np.asarray(self.n_ops, np.uint64), np.diff(np.asarray(self.req_resp_off, np.int64)))
        return int((np.asarray(self.slot_off, np.uint64) + per).max())

    def arrays(self) -> dict:
        return {k: np.ascontiguousarray(getattr(self, k), dt).reshape(-1) for k, dt in self.DTYPES.items()}

    def to_c(self):
        arrs = self.arrays()
        c = ResultReplies_C()
        c.n_resps, c.n_reqs, c.wire_len = self.n_resps, self.n_reqs, int(arrs["wire"].size)
        for k, a in arrs.items():
            if a.size == 0:  # an empty array still gets a valid address
                a = arrs[k] = np.zeros(1, a.dtype)
            setattr(c, k, _ptr(a))
        return c, arrs


def result_reply_decode(replies: "ResultReplies", n_slots: Optional[int] = None, fill: int = 0) -> dict:
    """mochi_result_reply_decode (host form) into buffers prefilled with `fill`: the arrays
    of mochi_result_decoded by name, the per-slot ones n_slots long (default: replies.n_slots)."""
    lib = load_library()
    r, keep = replies.to_c()
    n = dict(P=replies.n_resps, S=replies.n_slots if n_slots is None else int(n_slots))
    arr = {k: np.full(n[w] * np.dtype(dt).itemsize, fill, np.uint8).view(dt) for k, (dt, w) in _RR_OUT.items()}
    o = ResultDecoded_C()
    for k, a in arr.items():
        setattr(o, k, _ptr(a if a.size else np.zeros(1, a.dtype)))
    rc = lib.mochi_result_reply_decode(ctypes.addressof(r), ctypes.addressof(o))
    if rc != OK:
        raise MochiError(f"mochi_result_reply_decode rc={rc}: {_err(lib)}")
    return arr


def _tallied_c(replies_c, slots: dict, chosen, chosen_off, accept_bits, out_off) -> ResultTallied_C:
    """Pointers (ints) in, the C struct out."""
    t = ResultTallied_C()
    t.n_reqs = replies_c.n_reqs
    t.req_resp_off, t.n_ops, t.slot_off = replies_c.req_resp_off, replies_c.n_ops, replies_c.slot_off
    t.chosen, t.chosen_off, t.accept_bits, t.out_off = chosen, chosen_off, accept_bits, out_off
    for k in _RR_SLOT:
        setattr(t, k, slots[k])
    return t


def result_coalesce(replies: "ResultReplies", decoded: dict, chosen: np.ndarray, chosen_off: np.ndarray,
                    accept_bits: np.ndarray, out_off: np.ndarray, n_out: int, fill: int = 0) -> dict:
    """mochi_result_coalesce (host form): the tally's chosen / chosen_off / accept_bits and the
    decoder's per-slot arrays -> the arrays of mochi_result_coalesced, n_out long, prefilled."""
    lib = load_library()
    r, keep = replies.to_c()
    some = lambda a, dt: np.ascontiguousarray(a if np.asarray(a).size else np.zeros(1, dt), dt)
    ins = [some(chosen, np.int32), some(chosen_off, np.uint64), some(accept_bits, np.uint32), some(out_off, np.uint64)]
    slots = {k: some(decoded[k], _RR_OUT[k][0]) for k in _RR_SLOT}
    t = _tallied_c(r, {k: _ptr(a) for k, a in slots.items()}, *[_ptr(a) for a in ins])
    arr = {k: np.full(int(n_out) * np.dtype(dt).itemsize, fill, np.uint8).view(dt) for k, dt in _RC_OUT.items()}
    o = ResultCoalesced_C()
    for k, a in arr.items():
        setattr(o, k, _ptr(a if a.size else np.zeros(1, a.dtype)))
    rc = lib.mochi_result_coalesce(ctypes.addressof(t), ctypes.addressof(o))
    if rc != OK:
        raise MochiError(f"mochi_result_coalesce rc={rc}: {_err(lib)}")
    return arr


class DeviceResultReplies:
    """A ResultReplies copied into device memory with torch (plumbing only)."""

    def __init__(self, replies: "ResultReplies", device: int = 0):
        self.n_resps, self.n_reqs = replies.n_resps, replies.n_reqs
        self.wire_len = int(np.asarray(replies.wire).size)
        for k, a in replies.arrays().items():
            setattr(self, k, _to_dev(a, device))

    def to_c(self) -> ResultReplies_C:
        c = ResultReplies_C()
        c.n_resps, c.n_reqs, c.wire_len = self.n_resps, self.n_reqs, self.wire_len
        for k in ResultReplies.DTYPES:
            setattr(c, k, getattr(self, k).data_ptr())
        return c


def _dev_full(n: int, dt, fill: int, device: int):
    import torch

    sv = {np.uint8: torch.uint8, np.uint32: torch.int32, np.int32: torch.int32, np.uint64: torch.int64}
    pat = int.from_bytes(bytes([fill & 0xFF]) * np.dtype(dt).itemsize, "little", signed=dt != np.uint8)
    return torch.full((max(int(n), 1),), pat, dtype=sv[dt], device=torch.device("cuda", device))


class DeviceResultDecoded:
    """Device buffers for the outputs of Verifier.result_reply_decode_device, prefilled with
    `fill`.  Tensors carry the ABI widths (uint32 as int32, uint64 as int64)."""

    def __init__(self, n_resps: int, n_slots: int, device: int = 0, fill: int = 0):
        self.n = dict(P=int(n_resps), S=int(n_slots))
        for k, (dt, w) in _RR_OUT.items():
            setattr(self, k, _dev_full(self.n[w], dt, fill, device))

    def to_c(self) -> ResultDecoded_C:
        o = ResultDecoded_C()
        for k in _RR_OUT:
            setattr(o, k, getattr(self, k).data_ptr())
        return o

    def to_host(self) -> dict:
        """The buffers on the host, whole (as result_reply_decode returns them)."""
        return {k: getattr(self, k).cpu().numpy().view(dt)[:self.n[w]] for k, (dt, w) in _RR_OUT.items()}


class DeviceResultCoalesced:
    """Device buffers for the outputs of result_coalesce_device, prefilled with `fill`."""

    def __init__(self, n_out: int, device: int = 0, fill: int = 0):
        self.n_out = int(n_out)
        for k, dt in _RC_OUT.items():
            setattr(self, k, _dev_full(self.n_out, dt, fill, device))

    def to_c(self) -> ResultCoalesced_C:
        o = ResultCoalesced_C()
        for k in _RC_OUT:
            setattr(o, k, getattr(self, k).data_ptr())
        return o

    def to_host(self) -> dict:
        return {k: getattr(self, k).cpu().numpy().view(dt)[:self.n_out] for k, dt in _RC_OUT.items()}


def result_coalesce_device(dreplies: "DeviceResultReplies", decoded: "DeviceResultDecoded", chosen, chosen_off,
                           accept_bits, out_off, out: "DeviceResultCoalesced", stream: int = 0) -> None:
    """mochi_result_coalesce_device: one kernel on `stream`, no wait.  chosen / chosen_off /
    accept_bits are the tally's device tensors, out_off an int64 tensor [Q]."""
    lib = load_library()
    t = _tallied_c(dreplies.to_c(), {k: getattr(decoded, k).data_ptr() for k in _RR_SLOT}, chosen.data_ptr(),
                   chosen_off.data_ptr(), accept_bits.data_ptr(), out_off.data_ptr())
    o = out.to_c()
    rc = lib.mochi_result_coalesce_device(ctypes.addressof(t), ctypes.addressof(o), stream or None)
    if rc != OK:
        raise MochiError(f"mochi_result_coalesce_device rc={rc}: {_err(lib)}")


# ---------------------------------------------------------------------------
# Answer encode (the server's closing round): caller arrays -> Write2AnsFromServer /
# ReadFromServer bodies, the inverse of result_reply_decode; and the plan that fills those
# arrays from the Write2 verifier's outputs
# ---------------------------------------------------------------------------
ENC_BAD_OP = 4
RAO_HAS_CERT, RAO_RESULT_STORE, RAO_CERT_STORE = 0x01, 0x02, 0x04
W2A_REPLY, W2A_NO_REPLY, W2A_HOST = range(3)
W2A_HAS_STORED_CERT, W2A_VALUE_NULL = 0x01, 0x02
RESULT_ENCODE_STAGES = ("k_rae_size", "scan", "k_rae_hdr", "k_rae_copy")

# the arrays of mochi_result_answers: "P" per response, "S" per slot, "B" a blob; "?" may be None
_RA_IN = dict(wire=(np.uint8, "B"), store=(np.uint8, "B"), ids=(np.uint8, "B"), resp_kind=(np.uint8, "P"),
              resp_n_ops=(np.uint32, "P"), slot_off=(np.uint64, "P"), rid_off=(np.uint64, "P?"),
              rid_len=(np.uint32, "P?"), nonce_off=(np.uint64, "P?"), nonce_len=(np.uint32, "P?"),
              op_status=(np.uint8, "S"), op_existed=(np.uint8, "S"), op_flags=(np.uint8, "S"),
              op_result_off=(np.uint64, "S"), op_result_len=(np.uint32, "S"), op_cert_off=(np.uint64, "S"),
              op_cert_len=(np.uint32, "S"))
_RA_SLOT = tuple(k for k, (dt, w) in _RA_IN.items() if w == "S")
# the outputs of the Write2 answer plan: "M" per message, "S" per slot
_W2A_OUT = dict(plan_status=(np.uint8, "M"), resp_kind=(np.uint8, "M"), resp_n_ops=(np.uint32, "M"),
                **{k: _RA_IN[k] for k in _RA_SLOT})
# the per-op arrays of mochi_write2_answer_source the store supplies
_W2A_STORE = dict(op_value_off=np.uint64, op_value_len=np.uint32, op_stored_cert_off=np.uint64,
                  op_stored_cert_len=np.uint32, op_store_flags=np.uint8)


class ResultAnswers_C(ctypes.Structure):
    _fields_ = [("n_resps", ctypes.c_uint32), ("n_slots", ctypes.c_uint32), ("wire", ctypes.c_void_p),
                ("wire_len", ctypes.c_uint64), ("store", ctypes.c_void_p), ("store_len", ctypes.c_uint64),
                ("ids", ctypes.c_void_p), ("ids_len", ctypes.c_uint64)] + \
        [(k, ctypes.c_void_p) for k, (dt, w) in _RA_IN.items() if w != "B"]


class Write2AnswerSource_C(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("msg_status", "cert_accept_bits", "op_decision") + tuple(_W2A_STORE)] + \
        [("store_len", ctypes.c_uint64), ("slot_off", ctypes.c_void_p), ("n_slots", ctypes.c_uint32),
         ("_pad0", ctypes.c_uint32)]


class Write2AnswerPlanned_C(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in _W2A_OUT]


@dataclass
class ResultAnswers:
    """What a server answers in the closing round (mochi_result_answers, host arrays).  The
    per-slot arrays all have one length, n_slots."""

    wire: np.ndarray  # uint8: the received request bytes
    store: np.ndarray  # uint8: stored values and certificates
    ids: np.ndarray  # uint8: rid and nonce strings
    resp_kind: np.ndarray  # uint8 [P] RR_*
    resp_n_ops: np.ndarray  # uint32 [P]
    slot_off: np.ndarray  # uint64 [P]
    rid_off: Optional[np.ndarray]  # uint64 [P] or None = every rid empty
    rid_len: Optional[np.ndarray]  # uint32 [P]
    nonce_off: Optional[np.ndarray]  # uint64 [P] or None = every nonce empty
    nonce_len: Optional[np.ndarray]  # uint32 [P]
    op_status: np.ndarray  # uint8 [S]
    op_existed: np.ndarray  # uint8 [S]
    op_flags: np.ndarray  # uint8 [S] RAO_*
    op_result_off: np.ndarray  # uint64 [S]
    op_result_len: np.ndarray  # uint32 [S]
    op_cert_off: np.ndarray  # uint64 [S]
    op_cert_len: np.ndarray  # uint32 [S]

    @property
    def n_resps(self) -> int:
        return int(np.asarray(self.resp_kind).shape[0])

    @property
    def n_slots(self) -> int:
        return int(np.asarray(self.op_status).shape[0])

    @property
    def n_ops(self) -> int:
        return int(np.asarray(self.resp_n_ops, np.uint64).sum())

    def arrays(self) -> dict:
        """Every given array C-contiguous in its ABI dtype (None stays None)."""
        return {k: None if getattr(self, k) is None else np.ascontiguousarray(getattr(self, k), dt).reshape(-1)
                for k, (dt, w) in _RA_IN.items()}

    def to_c(self):
        arrs = self.arrays()
        c = ResultAnswers_C()
        c.n_resps, c.n_slots = self.n_resps, self.n_slots
        c.wire_len, c.store_len, c.ids_len = (int(arrs[k].size) for k in ("wire", "store", "ids"))
        for k, a in arrs.items():
            if a is not None and a.size == 0:  # an empty array still gets a valid address
                a = arrs[k] = np.zeros(1, a.dtype)
            setattr(c, k, _ptr(a))
        return c, arrs


def result_reply_encode_bound(answers) -> int:
    """mochi_result_reply_encode_bound for a ResultAnswers or a DeviceResultAnswers."""
    size = lambda k: int(getattr(answers, k + "_len")) if hasattr(answers, k + "_len") else int(np.asarray(getattr(answers, k)).size)
    return int(load_library().mochi_result_reply_encode_bound(answers.n_resps, answers.n_ops, size("wire"), size("store"),
                                                              size("ids")))


def result_reply_encode_into(answers: "ResultAnswers", wire: Optional[np.ndarray]):
    """mochi_result_reply_encode into the caller's buffer (uint8; None = capacity 0).
    Returns (rc, wire_len, msg_off, msg_len, status); rc is EINVAL with wire_len = the size
    needed when the buffer is too small (no byte of it written); any other failure raises."""
    lib = load_library()
    a, keep = answers.to_c()
    P = answers.n_resps
    off, ln, st = np.zeros(max(P, 1), np.uint64), np.zeros(max(P, 1), np.uint32), np.zeros(max(P, 1), np.uint8)
    cap = 0 if wire is None else int(wire.nbytes)
    need = ctypes.c_uint64(0)
    rc = lib.mochi_result_reply_encode(ctypes.addressof(a), _ptr(wire) if cap else None, cap, _ptr(off), _ptr(ln),
                                       _ptr(st), ctypes.addressof(need))
    if rc != OK and not (rc == EINVAL and int(need.value) > cap):
        raise MochiError(f"mochi_result_reply_encode rc={rc}: {_err(lib)}")
    return rc, int(need.value), off[:P], ln[:P], st[:P]


def result_reply_encode(answers: "ResultAnswers"):
    """Host form of the answer encoder: sizes first, then the bodies into a buffer of exactly
    the size needed.  Returns (wire, msg_off, msg_len, status)."""
    rc, need, off, ln, st = result_reply_encode_into(answers, None)
    wire = np.zeros(need, np.uint8)
    if need:
        rc, need, off, ln, st = result_reply_encode_into(answers, wire)
    assert rc == OK
    return wire, off, ln, st


class DeviceResultAnswers:
    """A ResultAnswers in device memory (plumbing only): copied with torch, or built from
    tensors that are already there (uint32 as int32, uint64 as int64)."""

    def __init__(self, answers: "ResultAnswers", device: int = 0):
        self.n_resps, self.n_slots, self.n_ops = answers.n_resps, answers.n_slots, answers.n_ops
        for k, a in answers.arrays().items():
            if _RA_IN[k][1] == "B":
                setattr(self, k + "_len", int(a.size))
            setattr(self, k, None if a is None else _to_dev(a, device))

    @classmethod
    def from_tensors(cls, n_resps: int, n_slots: int, n_ops: int, **tensors) -> "DeviceResultAnswers":
        """n_ops: the sum of resp_n_ops or a bound on it (read by result_reply_encode_bound alone)."""
        self = cls.__new__(cls)
        self.n_resps, self.n_slots, self.n_ops = int(n_resps), int(n_slots), int(n_ops)
        for k, (dt, w) in _RA_IN.items():
            t = tensors.get(k)
            setattr(self, k, t)
            if w == "B":
                setattr(self, k + "_len", 0 if t is None else int(t.numel()))
        return self

    def to_c(self) -> ResultAnswers_C:
        c = ResultAnswers_C()
        c.n_resps, c.n_slots = self.n_resps, self.n_slots
        c.wire_len, c.store_len, c.ids_len = self.wire_len, self.store_len, self.ids_len
        for k in _RA_IN:
            t = getattr(self, k)
            setattr(c, k, None if t is None else t.data_ptr())
        return c


@dataclass
class Write2AnswerStore:
    """The store's side of a Write2 batch's ops (host arrays, aligned with op_flags_off), the
    blob they point into, and where each message's slots start."""

    store: np.ndarray  # uint8
    op_value_off: np.ndarray  # uint64 [O]
    op_value_len: np.ndarray  # uint32 [O]
    op_stored_cert_off: np.ndarray  # uint64 [O]
    op_stored_cert_len: np.ndarray  # uint32 [O]
    op_store_flags: np.ndarray  # uint8 [O] W2A_*
    slot_off: np.ndarray  # uint64 [M]
    n_slots: int

    def arrays(self) -> dict:
        d = {k: np.ascontiguousarray(getattr(self, k), dt).reshape(-1) for k, dt in _W2A_STORE.items()}
        d["slot_off"] = np.ascontiguousarray(self.slot_off, np.uint64).reshape(-1)
        d["store"] = np.ascontiguousarray(self.store, np.uint8).reshape(-1)
        return d


def write2_answer_plan(wb, msg_status, cert_accept_bits, op_decision, st: "Write2AnswerStore", fill: int = 0) -> dict:
    """mochi_write2_answer_plan (host form) for a workload.WireBatch and the verify call's
    outputs: the arrays of mochi_write2_answer_planned by name, over buffers prefilled with `fill`."""
    lib = load_library()
    b, keep = write2_batch_c(wb)
    some = lambda a, dt: np.ascontiguousarray(a if np.asarray(a).size else np.zeros(1, dt), dt).reshape(-1)
    ins = dict(msg_status=some(msg_status, np.uint8), cert_accept_bits=some(cert_accept_bits, np.uint32),
               op_decision=some(op_decision, np.uint8))
    arrs = st.arrays()
    s = Write2AnswerSource_C()
    for k, a in ins.items():
        setattr(s, k, _ptr(a))
    for k in tuple(_W2A_STORE) + ("slot_off",):
        arrs[k] = arrs[k] if arrs[k].size else np.zeros(1, arrs[k].dtype)
        setattr(s, k, _ptr(arrs[k]))
    s.store_len, s.n_slots = int(arrs["store"].size), int(st.n_slots)
    n = dict(M=int(b.n_msgs), S=int(st.n_slots))
    out = {k: np.full(n[w] * np.dtype(dt).itemsize, fill, np.uint8).view(dt) for k, (dt, w) in _W2A_OUT.items()}
    o = Write2AnswerPlanned_C()
    for k, a in out.items():
        setattr(o, k, _ptr(a if a.size else np.zeros(1, a.dtype)))
    rc = lib.mochi_write2_answer_plan(ctypes.addressof(b), ctypes.addressof(s), ctypes.addressof(o))
    if rc != OK:
        raise MochiError(f"mochi_write2_answer_plan rc={rc}: {_err(lib)}")
    return out


def planned_answers(wire, store, ids, planned: dict, slot_off, rid_off=None, rid_len=None) -> "ResultAnswers":
    """The plan's outputs as the encoder's input (host arrays)."""
    return ResultAnswers(wire=wire, store=store, ids=ids, resp_kind=planned["resp_kind"],
                         resp_n_ops=planned["resp_n_ops"], slot_off=slot_off, rid_off=rid_off, rid_len=rid_len,
                         nonce_off=None, nonce_len=None, **{k: planned[k] for k in _RA_SLOT})


class DeviceWrite2AnswerStore:
    """A Write2AnswerStore copied into device memory with torch (plumbing only)."""

    def __init__(self, st: "Write2AnswerStore", device: int = 0):
        self.n_slots = int(st.n_slots)
        for k, a in st.arrays().items():
            if k == "store":
                self.store_len = int(a.size)
            setattr(self, k, _to_dev(a, device))


class DeviceWrite2AnswerPlanned:
    """Device buffers for the outputs of write2_answer_plan_device, prefilled with `fill`."""

    def __init__(self, n_msgs: int, n_slots: int, device: int = 0, fill: int = 0):
        self.n = dict(M=int(n_msgs), S=int(n_slots))
        for k, (dt, w) in _W2A_OUT.items():
            setattr(self, k, _dev_full(self.n[w], dt, fill, device))

    def to_c(self) -> Write2AnswerPlanned_C:
        o = Write2AnswerPlanned_C()
        for k in _W2A_OUT:
            setattr(o, k, getattr(self, k).data_ptr())
        return o

    def to_host(self) -> dict:
        return {k: getattr(self, k).cpu().numpy().view(dt)[:self.n[w]] for k, (dt, w) in _W2A_OUT.items()}

    def answers(self, dwb: "DeviceWireBatch", dst: "DeviceWrite2AnswerStore", ids=None, rid_off=None,
                rid_len=None) -> "DeviceResultAnswers":
        """The encoder's input over these buffers: no copy, no host round trip."""
        return DeviceResultAnswers.from_tensors(
            self.n["M"], self.n["S"], self.n["S"], wire=dwb.wire, store=dst.store, ids=ids, resp_kind=self.resp_kind,
            resp_n_ops=self.resp_n_ops, slot_off=dst.slot_off, rid_off=rid_off, rid_len=rid_len,
            **{k: getattr(self, k) for k in _RA_SLOT})


def write2_answer_plan_device(dwb: "DeviceWireBatch", verdicts: "DeviceVerdicts", dst: "DeviceWrite2AnswerStore",
                              out: "DeviceWrite2AnswerPlanned", stream: int = 0) -> None:
    """mochi_write2_answer_plan_device: one kernel on `stream`, no wait.  Reads dwb.status,
    verdicts.cert_accept_bits and verdicts.op_decision in stream order: it may be enqueued
    right behind Verifier.verify_write2_device."""
    lib = load_library()
    b = dwb.to_c()
    s = Write2AnswerSource_C()
    s.msg_status, s.cert_accept_bits = dwb.status.data_ptr(), verdicts.cert_accept_bits.data_ptr()
    s.op_decision = verdicts.op_decision.data_ptr()
    for k in tuple(_W2A_STORE) + ("slot_off",):
        setattr(s, k, getattr(dst, k).data_ptr())
    s.store_len, s.n_slots = dst.store_len, dst.n_slots
    o = out.to_c()
    rc = lib.mochi_write2_answer_plan_device(ctypes.addressof(b), ctypes.addressof(s), ctypes.addressof(o), stream or None)
    if rc != OK:
        raise MochiError(f"mochi_write2_answer_plan_device rc={rc}: {_err(lib)}")


# ---------------------------------------------------------------------------
# Read request decode and read answer plan (the server's side of a read): ReadToServer
# bodies -> SoA arrays with their batch-wide key numbering; those and the store's state
# per distinct key -> the answer encoder's input
# ---------------------------------------------------------------------------
RDQ_OK, RDQ_MALFORMED, RDQ_FALLBACK = range(3)
RDOP_READ = 0x01
RDA_REPLY, RDA_NO_REPLY, RDA_HOST = range(3)
RDK_LOCAL, RDK_PRESENT, RDK_AVAILABLE, RDK_HAS_CERT = 0x01, 0x02, 0x04, 0x08
READ_REQUEST_STAGES = ("k_rdq_req", "entry_scan", "k_w1q_ops", "final_scan_offsets", "k_rdq_emit", "k_w1q_claim",
                       "k_w1q_rank", "key_scan", "k_w1q_number")

ReadRequests = Write1Requests  # mochi_read_requests is mochi_write1_requests
DeviceReadRequests = DeviceWrite1Requests

# output arrays by what they are indexed with, as _W1Q_OUT
_RDQ_OUT = dict(req_status=(np.uint8, "Q"), req_client_off=(np.uint64, "Q"), req_client_len=(np.uint32, "Q"),
                req_nonce_off=(np.uint64, "Q"), req_nonce_len=(np.uint32, "Q"), req_op_off=(np.uint32, "Q1"),
                op_key_off=(np.uint64, "O"), op_key_len=(np.uint32, "O"), op_flags=(np.uint8, "O"),
                op_obj=(np.uint32, "O"), key_op=(np.uint32, "K"))
_RDK_IN = dict(key_flags=np.uint8, key_value_off=np.uint64, key_value_len=np.uint32, key_cert_off=np.uint64,
               key_cert_len=np.uint32)
# the outputs of the read answer plan: "Q" per request, "S" per slot (= per op)
_RDA_OUT = dict(plan_status=(np.uint8, "Q"), resp_kind=(np.uint8, "Q"), resp_n_ops=(np.uint32, "Q"),
                slot_off=(np.uint64, "Q"), **{k: _RA_IN[k] for k in _RA_SLOT})


class ReadRequestsDecoded_C(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("req_status", "req_client_off", "req_client_len", "req_nonce_off",
                                               "req_nonce_len", "req_op_off")] + \
        [("n_ops", ctypes.c_uint32), ("n_keys", ctypes.c_uint32), ("op_cap", ctypes.c_uint32), ("_pad0", ctypes.c_uint32)] + \
        [(k, ctypes.c_void_p) for k in ("op_key_off", "op_key_len", "op_flags", "op_obj", "key_op")]


class ReadKeyState_C(ctypes.Structure):
    _fields_ = [("n_keys", ctypes.c_uint32), ("_pad0", ctypes.c_uint32)] + [(k, ctypes.c_void_p) for k in _RDK_IN] + \
        [("store_len", ctypes.c_uint64)]


class ReadAnswerPlanned_C(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in _RDA_OUT]


@dataclass
class ReadRequestsDecoded:
    """Outputs of read_request_decode (mochi_read_requests_decoded): the caller's buffers,
    whole (n_ops / n_keys say how much of the per-op ones / of key_op is meant)."""

    rc: int
    n_ops: int
    n_keys: int
    arrays: dict  # name -> array, names as in mochi_read_requests_decoded

    def __getattr__(self, k):
        try:
            return self.__dict__["arrays"][k]
        except KeyError:
            raise AttributeError(k)

    def trimmed(self) -> dict:
        """Every array cut to its meaning (per-op ones and key_op to 0 unless rc is OK)."""
        Q = self.arrays["req_status"].shape[0]
        ok = self.rc == OK
        n = dict(Q=Q, Q1=Q + 1, O=self.n_ops if ok else 0, K=self.n_keys if ok else 0)
        return {k: self.arrays[k][:n[w]] for k, (dt, w) in _RDQ_OUT.items()}


def read_request_decode_bound(wire_len: int, n_reqs: int) -> int:
    """mochi_read_request_decode_bound: a safe op_cap."""
    return int(load_library().mochi_read_request_decode_bound(int(wire_len), int(n_reqs)))


def read_request_decode_into(reqs: "ReadRequests", op_cap: int, fill: int = 0) -> "ReadRequestsDecoded":
    """mochi_read_request_decode into buffers of the given capacity, prefilled with `fill`.
    rc is EINVAL with n_ops = the count needed when it is too small (no per-op array
    touched); any other failure raises."""
    lib = load_library()
    r, keep = reqs.to_c()
    Q = reqs.n_reqs
    n = dict(Q=Q, Q1=Q + 1, O=int(op_cap), K=int(op_cap))
    arr = {k: np.full(n[w] * np.dtype(dt).itemsize, fill, np.uint8).view(dt) for k, (dt, w) in _RDQ_OUT.items()}
    o = ReadRequestsDecoded_C()
    for k, a in arr.items():
        setattr(o, k, _ptr(a) if a.size else None)
    o.op_cap = int(op_cap)
    rc = lib.mochi_read_request_decode(ctypes.addressof(r), ctypes.addressof(o))
    if rc != OK and not (rc == EINVAL and o.n_ops > op_cap):
        raise MochiError(f"mochi_read_request_decode rc={rc}: {_err(lib)}")
    return ReadRequestsDecoded(rc=rc, n_ops=int(o.n_ops), n_keys=int(o.n_keys), arrays=arr)


def read_request_decode(reqs: "ReadRequests") -> "ReadRequestsDecoded":
    """Host form of the read request decoder: the count first, then into buffers of exactly
    the size needed."""
    first = read_request_decode_into(reqs, 0)
    if first.rc == OK:
        return first
    return read_request_decode_into(reqs, first.n_ops)


@dataclass
class ReadKeyState:
    """The store's state per distinct key of a decoded read batch (mochi_read_key_state, host
    arrays) and the blob its slices point into."""

    store: np.ndarray  # uint8
    key_flags: np.ndarray  # uint8 [U] RDK_*
    key_value_off: np.ndarray  # uint64 [U]
    key_value_len: np.ndarray  # uint32 [U]
    key_cert_off: np.ndarray  # uint64 [U]
    key_cert_len: np.ndarray  # uint32 [U]

    def arrays(self) -> dict:
        d = {k: np.ascontiguousarray(getattr(self, k), dt).reshape(-1) for k, dt in _RDK_IN.items()}
        d["store"] = np.ascontiguousarray(self.store, np.uint8).reshape(-1)
        return d


def read_answer_plan(dec: "ReadRequestsDecoded", keys: "ReadKeyState", fill: int = 0) -> dict:
    """mochi_read_answer_plan (host form) over a decoded batch (its arrays trimmed or whole):
    the arrays of mochi_read_answer_planned by name, over buffers prefilled with `fill`."""
    lib = load_library()
    some = lambda a, dt: np.ascontiguousarray(a if np.asarray(a).size else np.zeros(1, dt), dt).reshape(-1)
    Q = int(np.asarray(dec.arrays["req_status"]).shape[0])
    d = ReadRequestsDecoded_C()
    ins = {k: some(dec.arrays[k], _RDQ_OUT[k][0]) for k in ("req_status", "req_op_off", "op_key_len", "op_flags", "op_obj")}
    for k, a in ins.items():
        setattr(d, k, _ptr(a))
    d.n_ops = int(dec.n_ops)
    karr = keys.arrays()
    ks = ReadKeyState_C()
    ks.n_keys, ks.store_len = int(karr["key_flags"].size), int(karr["store"].size)
    for k in _RDK_IN:
        karr[k] = some(karr[k], _RDK_IN[k])
        setattr(ks, k, _ptr(karr[k]))
    n = dict(Q=Q, S=int(dec.n_ops))
    out = {k: np.full(n[w] * np.dtype(dt).itemsize, fill, np.uint8).view(dt) for k, (dt, w) in _RDA_OUT.items()}
    o = ReadAnswerPlanned_C()
    for k, a in out.items():
        setattr(o, k, _ptr(a if a.size else np.zeros(1, a.dtype)))
    rc = lib.mochi_read_answer_plan(Q, ctypes.addressof(d), ctypes.addressof(ks), ctypes.addressof(o))
    if rc != OK:
        raise MochiError(f"mochi_read_answer_plan rc={rc}: {_err(lib)}")
    return out


def read_planned_answers(wire, store, planned: dict, nonce_off, nonce_len, ids=None, rid_off=None,
                         rid_len=None) -> "ResultAnswers":
    """The read plan's outputs as the encoder's input (host arrays): ids = wire unless given,
    the nonces the decoder's req_nonce_off / req_nonce_len."""
    return ResultAnswers(wire=wire, store=store, ids=wire if ids is None else ids, resp_kind=planned["resp_kind"],
                         resp_n_ops=planned["resp_n_ops"], slot_off=planned["slot_off"], rid_off=rid_off, rid_len=rid_len,
                         nonce_off=nonce_off, nonce_len=nonce_len, **{k: planned[k] for k in _RA_SLOT})


class DeviceReadRequestsDecoded:
    """Device buffers for the outputs of Verifier.read_request_decode_device, prefilled with
    `fill`; n_ops is set by the call, the key count lands in the device word n_keys_dev.
    Tensors carry the ABI widths (uint32 as int32, uint64 as int64)."""

    def __init__(self, n_reqs: int, op_cap: int, device: int = 0, fill: int = 0):
        self.n_reqs, self.op_cap = int(n_reqs), int(op_cap)
        n = dict(Q=self.n_reqs, Q1=self.n_reqs + 1, O=self.op_cap, K=self.op_cap)
        for k, (dt, w) in _RDQ_OUT.items():
            setattr(self, k, _dev_full(n[w], dt, fill, device))
        self.n_keys_dev = _dev_full(1, np.uint32, fill, device)
        self.n_ops = 0

    def to_c(self) -> ReadRequestsDecoded_C:
        o = ReadRequestsDecoded_C()
        for k in _RDQ_OUT:
            setattr(o, k, getattr(self, k).data_ptr())
        o.op_cap, o.n_ops = self.op_cap, self.n_ops
        return o

    def n_keys(self) -> int:
        """The key count (a device read: synchronises)."""
        return int(self.n_keys_dev.cpu().numpy().view(np.uint32)[0])

    def to_host(self, rc: int = OK) -> "ReadRequestsDecoded":
        """The buffers on the host, whole (as read_request_decode_into returns them)."""
        n = dict(Q=self.n_reqs, Q1=self.n_reqs + 1, O=self.op_cap, K=self.op_cap)
        arr = {k: getattr(self, k).cpu().numpy().view(dt)[:n[w]] for k, (dt, w) in _RDQ_OUT.items()}
        return ReadRequestsDecoded(rc=rc, n_ops=self.n_ops, n_keys=self.n_keys(), arrays=arr)


class DeviceReadKeyState:
    """A ReadKeyState copied into device memory with torch (plumbing only)."""

    def __init__(self, keys: "ReadKeyState", device: int = 0):
        a = keys.arrays()
        self.n_keys, self.store_len = int(a["key_flags"].size), int(a["store"].size)
        for k, v in a.items():
            setattr(self, k, _to_dev(v, device))

    def to_c(self) -> ReadKeyState_C:
        c = ReadKeyState_C()
        c.n_keys, c.store_len = self.n_keys, self.store_len
        for k in _RDK_IN:
            setattr(c, k, getattr(self, k).data_ptr())
        return c


class DeviceReadAnswerPlanned:
    """Device buffers for the outputs of read_answer_plan_device, prefilled with `fill`
    (n_slots: the decoder's n_ops or more)."""

    def __init__(self, n_reqs: int, n_slots: int, device: int = 0, fill: int = 0):
        self.n = dict(Q=int(n_reqs), S=int(n_slots))
        for k, (dt, w) in _RDA_OUT.items():
            setattr(self, k, _dev_full(self.n[w], dt, fill, device))

    def to_c(self) -> ReadAnswerPlanned_C:
        o = ReadAnswerPlanned_C()
        for k in _RDA_OUT:
            setattr(o, k, getattr(self, k).data_ptr())
        return o

    def to_host(self) -> dict:
        return {k: getattr(self, k).cpu().numpy().view(dt)[:self.n[w]] for k, (dt, w) in _RDA_OUT.items()}

    def answers(self, dreqs: "DeviceReadRequests", dec: "DeviceReadRequestsDecoded", dkeys: "DeviceReadKeyState",
                rid_off=None, rid_len=None) -> "DeviceResultAnswers":
        """The encoder's input over these buffers, ids = wire and the nonces the decoder's: no
        copy, no host round trip."""
        return DeviceResultAnswers.from_tensors(
            self.n["Q"], dec.n_ops, dec.n_ops, wire=dreqs.wire, store=dkeys.store, ids=dreqs.wire,
            resp_kind=self.resp_kind, resp_n_ops=self.resp_n_ops, slot_off=self.slot_off, rid_off=rid_off, rid_len=rid_len,
            nonce_off=dec.req_nonce_off, nonce_len=dec.req_nonce_len, **{k: getattr(self, k) for k in _RA_SLOT})


def read_answer_plan_device(dec: "DeviceReadRequestsDecoded", dkeys: "DeviceReadKeyState",
                            out: "DeviceReadAnswerPlanned", stream: int = 0) -> None:
    """mochi_read_answer_plan_device: one kernel on `stream`, no wait; reads the decoder's
    arrays in stream order (dec.n_ops is the host field the decode call set)."""
    lib = load_library()
    d, k, o = dec.to_c(), dkeys.to_c(), out.to_c()
    rc = lib.mochi_read_answer_plan_device(dec.n_reqs, ctypes.addressof(d), ctypes.addressof(k), ctypes.addressof(o),
                                           stream or None)
    if rc != OK:
        raise MochiError(f"mochi_read_answer_plan_device rc={rc}: {_err(lib)}")


# ---------------------------------------------------------------------------
# The ProtocolMessage envelope: frames -> status / payload case / body slice / scalars
# (decode), the server's partition by case (route), the client's match of replies to
# requests (join), and bodies -> frames (encode)
# ---------------------------------------------------------------------------
ENV_OK, ENV_MALFORMED, ENV_FALLBACK = range(3)
ENV_KINDS = 13
ENV_LENGTH_PREFIX = 0x1
ENC_BAD_KIND, ENC_BAD_ID = 5, 6
ENVELOPE_STAGES = dict(decode=("k_env_decode",), route=("k_env_hist", "scan", "k_env_scatter"),
                       join=("k_env_claim", "k_env_lookup", "sort", "k_env_group"),
                       encode=("k_env_size", "scan", "k_env_hdr", "k_env_copy"))

_ENV_DEC = dict(status=np.uint8, kind=np.uint8, body_off=np.uint64, body_len=np.uint32, msg_timestamp=np.int64,
                server_id_off=np.uint64, server_id_len=np.uint32, msg_id_off=np.uint64, msg_id_len=np.uint32,
                reply_to_off=np.uint64, reply_to_len=np.uint32)
# the routed / joined outputs: "n" per frame, "K" the 14 kind offsets, "Q1" per request + 1
_ENV_ROUTED = dict(kind_off=(np.uint32, "K"), order=(np.uint32, "n"), body_off=(np.uint64, "n"), body_len=(np.uint32, "n"))
_ENV_JOINED = dict(frame_req=(np.uint32, "n"), req_resp_off=(np.uint32, "Q1"), resp_frame=(np.uint32, "n"),
                   resp_off=(np.uint64, "n"), resp_len=(np.uint32, "n"), resp_w1_kind=(np.uint8, "n"),
                   resp_rr_kind=(np.uint8, "n"))
# the per-message arrays of mochi_envelope_source; "?" may be None
_ENV_SRC = dict(kind=(np.uint8, ""), body_off=(np.uint64, ""), body_len=(np.uint32, ""), msg_timestamp=(np.int64, ""),
                msg_id_off=(np.uint64, "?"), msg_id_len=(np.uint32, "?"), reply_to_off=(np.uint64, "?"),
                reply_to_len=(np.uint32, "?"), server_id_off=(np.uint64, "?"), server_id_len=(np.uint32, "?"))


class EnvelopeFrames_C(ctypes.Structure):
    _fields_ = [("n_frames", ctypes.c_uint32), ("_pad0", ctypes.c_uint32), ("wire", ctypes.c_void_p),
                ("wire_len", ctypes.c_uint64), ("frame_off", ctypes.c_void_p), ("frame_len", ctypes.c_void_p)]


class EnvelopeDecoded_C(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in _ENV_DEC]


class EnvelopeRouted_C(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in _ENV_ROUTED]


class EnvelopeRequests_C(ctypes.Structure):
    _fields_ = [("n_reqs", ctypes.c_uint32), ("_pad0", ctypes.c_uint32), ("ids", ctypes.c_void_p),
                ("ids_len", ctypes.c_uint64), ("id_off", ctypes.c_void_p), ("id_len", ctypes.c_void_p)]


class EnvelopeJoined_C(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in _ENV_JOINED]


class EnvelopeSource_C(ctypes.Structure):
    _fields_ = [("n_msgs", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("bodies", ctypes.c_void_p),
                ("bodies_len", ctypes.c_uint64), ("ids", ctypes.c_void_p), ("ids_len", ctypes.c_uint64)] + \
        [(k, ctypes.c_void_p) for k in _ENV_SRC]


def _some(a, dt) -> np.ndarray:
    """C-contiguous in the ABI dtype; an empty array still gets a valid address."""
    a = np.ascontiguousarray(a, dt).reshape(-1)
    return a if a.size else np.zeros(1, dt)


def _filled(n: int, dt, fill: int) -> np.ndarray:
    return np.full(max(int(n), 1) * np.dtype(dt).itemsize, fill & 0xFF, np.uint8).view(dt)


@dataclass
class EnvelopeFrames:
    """Received frames (mochi_envelope_frames, host arrays): frame f is wire[frame_off[f], +frame_len[f])."""

    wire: np.ndarray  # uint8
    frame_off: np.ndarray  # uint64 [n]
    frame_len: np.ndarray  # uint32 [n]

    @classmethod
    def pack(cls, frames: Sequence[bytes], pad: int = 0) -> "EnvelopeFrames":
        """Frames back to back, frame i behind (i * pad) % 4 filler bytes (misaligned slices)."""
        parts, off, pos = [], [], 0
        for i, f in enumerate(frames):
            p = (i * pad) % 4
            parts.append(b"\xEE" * p)
            off.append(pos + p)
            parts.append(bytes(f))
            pos += p + len(f)
        return cls(np.frombuffer(b"".join(parts), np.uint8).copy(), np.array(off, np.uint64),
                   np.array([len(f) for f in frames], np.uint32))

    @property
    def n_frames(self) -> int:
        return int(np.asarray(self.frame_off).shape[0])

    def to_c(self):
        arrs = dict(wire=_some(self.wire, np.uint8), frame_off=_some(self.frame_off, np.uint64),
                    frame_len=_some(self.frame_len, np.uint32))
        c = EnvelopeFrames_C()
        c.n_frames, c.wire_len = self.n_frames, int(np.asarray(self.wire).size)
        for k, a in arrs.items():
            setattr(c, k, _ptr(a))
        return c, arrs


def _env_out(cls_c, spec: dict, sizes: dict, fill: int):
    arr = {k: _filled(sizes[w], dt, fill) for k, (dt, w) in spec.items()}
    o = cls_c()
    for k, a in arr.items():
        setattr(o, k, _ptr(a))
    return o, arr, {k: a[:sizes[spec[k][1]]] for k, a in arr.items()}


def envelope_decode(frames: "EnvelopeFrames", fill: int = 0) -> dict:
    """mochi_envelope_decode (host form) into buffers prefilled with `fill`: the arrays of
    mochi_envelope_decoded by name."""
    lib = load_library()
    f, keep = frames.to_c()
    o, arr, out = _env_out(EnvelopeDecoded_C, {k: (dt, "n") for k, dt in _ENV_DEC.items()}, dict(n=frames.n_frames), fill)
    rc = lib.mochi_envelope_decode(ctypes.addressof(f), ctypes.addressof(o))
    if rc != OK:
        raise MochiError(f"mochi_envelope_decode rc={rc}: {_err(lib)}")
    return out


def envelope_route(decoded: dict, fill: int = 0) -> dict:
    """mochi_envelope_route (host form) over a decode's outputs: the arrays of
    mochi_envelope_routed by name, order / body_off / body_len whole (n long)."""
    lib = load_library()
    n = int(np.asarray(decoded["status"]).shape[0])
    ins = [_some(decoded[k], _ENV_DEC[k]) for k in ("status", "kind", "body_off", "body_len")]
    o, arr, out = _env_out(EnvelopeRouted_C, _ENV_ROUTED, dict(n=n, K=ENV_KINDS + 1), fill)
    rc = lib.mochi_envelope_route(n, *[_ptr(a) for a in ins], ctypes.addressof(o))
    if rc != OK:
        raise MochiError(f"mochi_envelope_route rc={rc}: {_err(lib)}")
    return out


def _env_requests_c(ids: Sequence[bytes]):
    blob = _some(np.frombuffer(b"".join(ids), np.uint8), np.uint8)
    ln = np.array([len(i) for i in ids], np.uint32)
    off = np.concatenate([[0], np.cumsum(ln, dtype=np.uint64)[:-1]]).astype(np.uint64) if len(ids) else np.zeros(0, np.uint64)
    arrs = dict(ids=blob, id_off=_some(off, np.uint64), id_len=_some(ln, np.uint32))
    c = EnvelopeRequests_C()
    c.n_reqs, c.ids_len = len(ids), sum(len(i) for i in ids)
    for k, a in arrs.items():
        setattr(c, k, _ptr(a))
    return c, arrs


def envelope_join(request_ids: Sequence[bytes], frames: "EnvelopeFrames", decoded: dict, fill: int = 0):
    """mochi_envelope_join (host form): the outstanding requests' msgIds, the frames and
    their decode -> (the arrays of mochi_envelope_joined by name, whole; P)."""
    lib = load_library()
    r, keep_r = _env_requests_c(request_ids)
    f, keep_f = frames.to_c()
    d = EnvelopeDecoded_C()
    ins = {k: _some(decoded[k], dt) for k, dt in _ENV_DEC.items()}
    for k, a in ins.items():
        setattr(d, k, _ptr(a))
    o, arr, out = _env_out(EnvelopeJoined_C, _ENV_JOINED, dict(n=frames.n_frames, Q1=len(request_ids) + 1), fill)
    P = ctypes.c_uint32(0)
    rc = lib.mochi_envelope_join(ctypes.addressof(r), ctypes.addressof(f), ctypes.addressof(d), ctypes.addressof(o),
                                 ctypes.addressof(P))
    if rc != OK:
        raise MochiError(f"mochi_envelope_join rc={rc}: {_err(lib)}")
    return out, int(P.value)


@dataclass
class EnvelopeSource:
    """What to wrap (mochi_envelope_source, host arrays).  Any id pair may be None."""

    bodies: np.ndarray  # uint8
    ids: np.ndarray  # uint8
    kind: np.ndarray  # uint8 [M]
    body_off: np.ndarray  # uint64 [M]
    body_len: np.ndarray  # uint32 [M]
    msg_timestamp: np.ndarray  # int64 [M]
    msg_id_off: Optional[np.ndarray] = None
    msg_id_len: Optional[np.ndarray] = None
    reply_to_off: Optional[np.ndarray] = None
    reply_to_len: Optional[np.ndarray] = None
    server_id_off: Optional[np.ndarray] = None
    server_id_len: Optional[np.ndarray] = None
    flags: int = 0

    @property
    def n_msgs(self) -> int:
        return int(np.asarray(self.kind).shape[0])

    def arrays(self) -> dict:
        d = {k: None if getattr(self, k) is None else np.ascontiguousarray(getattr(self, k), dt).reshape(-1)
             for k, (dt, w) in _ENV_SRC.items()}
        d["bodies"] = np.ascontiguousarray(self.bodies, np.uint8).reshape(-1)
        d["ids"] = np.ascontiguousarray(self.ids, np.uint8).reshape(-1)
        return d

    def to_c(self):
        arrs = self.arrays()
        c = EnvelopeSource_C()
        c.n_msgs, c.flags = self.n_msgs, int(self.flags)
        c.bodies_len, c.ids_len = int(arrs["bodies"].size), int(arrs["ids"].size)
        for k, a in arrs.items():
            if a is not None and a.size == 0:
                a = arrs[k] = np.zeros(1, a.dtype)
            setattr(c, k, _ptr(a))
        return c, arrs


def envelope_encode_bound(n_msgs: int, bodies_len: int, ids_len: int) -> int:
    return int(load_library().mochi_envelope_encode_bound(n_msgs, bodies_len, ids_len))


def envelope_encode_into(src: "EnvelopeSource", wire: Optional[np.ndarray]):
    """mochi_envelope_encode into the caller's buffer (uint8; None = capacity 0).  Returns
    (rc, wire_len, msg_off, msg_len, status) as result_reply_encode_into."""
    lib = load_library()
    s, keep = src.to_c()
    M = src.n_msgs
    off, ln, st = np.zeros(max(M, 1), np.uint64), np.zeros(max(M, 1), np.uint32), np.zeros(max(M, 1), np.uint8)
    cap = 0 if wire is None else int(wire.nbytes)
    need = ctypes.c_uint64(0)
    rc = lib.mochi_envelope_encode(ctypes.addressof(s), _ptr(wire) if cap else None, cap, _ptr(off), _ptr(ln), _ptr(st),
                                   ctypes.addressof(need))
    if rc != OK and not (rc == EINVAL and int(need.value) > cap):
        raise MochiError(f"mochi_envelope_encode rc={rc}: {_err(lib)}")
    return rc, int(need.value), off[:M], ln[:M], st[:M]


def envelope_encode(src: "EnvelopeSource"):
    """Host form of the wrap: sizes first, then the frames into a buffer of exactly the size
    needed.  Returns (wire, msg_off, msg_len, status)."""
    rc, need, off, ln, st = envelope_encode_into(src, None)
    wire = np.zeros(need, np.uint8)
    if need:
        rc, need, off, ln, st = envelope_encode_into(src, wire)
    assert rc == OK
    return wire, off, ln, st


class DeviceEnvelopeFrames:
    """An EnvelopeFrames in device memory (plumbing only): copied with torch, or built from
    tensors that are already there (uint8 wire, int64 frame_off, int32 frame_len)."""

    def __init__(self, frames: "EnvelopeFrames", device: int = 0):
        self.n_frames, self.wire_len = frames.n_frames, int(np.asarray(frames.wire).size)
        c, arrs = frames.to_c()
        for k, a in arrs.items():
            setattr(self, k, _to_dev(a, device))

    @classmethod
    def from_tensors(cls, n_frames: int, wire, frame_off, frame_len, wire_len: Optional[int] = None):
        self = cls.__new__(cls)
        self.n_frames, self.wire, self.frame_off, self.frame_len = int(n_frames), wire, frame_off, frame_len
        self.wire_len = int(wire.numel()) if wire_len is None else int(wire_len)
        return self

    def to_c(self) -> EnvelopeFrames_C:
        c = EnvelopeFrames_C()
        c.n_frames, c.wire_len = self.n_frames, self.wire_len
        c.wire, c.frame_off, c.frame_len = self.wire.data_ptr(), self.frame_off.data_ptr(), self.frame_len.data_ptr()
        return c


def _dev_i64_full(n: int, fill: int, device: int):
    import torch

    pat = int.from_bytes(bytes([fill & 0xFF]) * 8, "little", signed=True)
    return torch.full((max(int(n), 1),), pat, dtype=torch.int64, device=torch.device("cuda", device))


class _DevOut:
    """Device buffers prefilled with `fill`, by a spec of (dtype, size key); uint32 as int32,
    uint64 / int64 as int64."""

    SPEC: dict = {}
    C = None

    def _alloc(self, sizes: dict, device: int, fill: int):
        self.sizes = sizes
        for k, (dt, w) in self.SPEC.items():
            t = _dev_i64_full(sizes[w], fill, device) if dt == np.int64 else _dev_full(sizes[w], dt, fill, device)
            setattr(self, k, t)

    def to_c(self):
        o = self.C()
        for k in self.SPEC:
            setattr(o, k, getattr(self, k).data_ptr())
        return o

    def to_host(self) -> dict:
        """The buffers on the host, whole."""
        return {k: getattr(self, k).cpu().numpy().view(dt)[:self.sizes[w]] for k, (dt, w) in self.SPEC.items()}


class DeviceEnvelopeDecoded(_DevOut):
    SPEC = {k: (dt, "n") for k, dt in _ENV_DEC.items()}
    C = EnvelopeDecoded_C

    def __init__(self, n_frames: int, device: int = 0, fill: int = 0):
        self.n = int(n_frames)
        self._alloc(dict(n=self.n), device, fill)


class DeviceEnvelopeRouted(_DevOut):
    SPEC = _ENV_ROUTED
    C = EnvelopeRouted_C

    def __init__(self, n_frames: int, device: int = 0, fill: int = 0):
        self._alloc(dict(n=int(n_frames), K=ENV_KINDS + 1), device, fill)


class DeviceEnvelopeJoined(_DevOut):
    SPEC = _ENV_JOINED
    C = EnvelopeJoined_C

    def __init__(self, n_frames: int, n_reqs: int, device: int = 0, fill: int = 0):
        self._alloc(dict(n=int(n_frames), Q1=int(n_reqs) + 1), device, fill)
        self.n_resps = _dev_full(1, np.uint32, fill, device)


class DeviceEnvelopeRequests:
    """The outstanding requests' msgIds in device memory (plumbing only)."""

    def __init__(self, request_ids: Sequence[bytes], device: int = 0):
        c, arrs = _env_requests_c(request_ids)
        self.n_reqs, self.ids_len = int(c.n_reqs), int(c.ids_len)
        for k, a in arrs.items():
            setattr(self, k, _to_dev(a, device))

    def to_c(self) -> EnvelopeRequests_C:
        c = EnvelopeRequests_C()
        c.n_reqs, c.ids_len = self.n_reqs, self.ids_len
        c.ids, c.id_off, c.id_len = self.ids.data_ptr(), self.id_off.data_ptr(), self.id_len.data_ptr()
        return c


class DeviceEnvelopeSource:
    """An EnvelopeSource in device memory (plumbing only): copied with torch, or built from
    tensors that are already there."""

    def __init__(self, src: "EnvelopeSource", device: int = 0):
        self.n_msgs, self.flags = src.n_msgs, int(src.flags)
        for k, a in src.arrays().items():
            if k in ("bodies", "ids"):
                setattr(self, k + "_len", int(a.size))
            setattr(self, k, None if a is None else _to_dev(a, device))

    @classmethod
    def from_tensors(cls, n_msgs: int, flags: int = 0, **tensors) -> "DeviceEnvelopeSource":
        self = cls.__new__(cls)
        self.n_msgs, self.flags = int(n_msgs), int(flags)
        for k in ("bodies", "ids") + tuple(_ENV_SRC):
            t = tensors.get(k)
            setattr(self, k, t)
            if k in ("bodies", "ids"):
                setattr(self, k + "_len", 0 if t is None else int(t.numel()))
        return self

    def to_c(self) -> EnvelopeSource_C:
        c = EnvelopeSource_C()
        c.n_msgs, c.flags, c.bodies_len, c.ids_len = self.n_msgs, self.flags, self.bodies_len, self.ids_len
        for k in ("bodies", "ids") + tuple(_ENV_SRC):
            t = getattr(self, k)
            setattr(c, k, None if t is None else t.data_ptr())
        return c


# ---------------------------------------------------------------------------
# Multi-GPU (include/mochi_hip.h)
# ---------------------------------------------------------------------------
def shard_plan(n_certs: int, n_shards: int, cert_grant_off: Optional[np.ndarray] = None) -> np.ndarray:
    """Contiguous 32-aligned certificate shards (mochi_shard_plan): cert_lo[n_shards+1]."""
    lib = load_library()
    out = np.zeros(n_shards + 1, np.uint32)
    cgo = None if cert_grant_off is None else np.ascontiguousarray(cert_grant_off, np.uint32)
    if lib.mochi_shard_plan(n_certs, _ptr(cgo), n_shards, _ptr(out)) != OK:
        raise MochiError("mochi_shard_plan failed")
    return out


def shard_words(cert_lo: np.ndarray) -> int:
    lo = np.ascontiguousarray(cert_lo, np.uint32)
    return int(load_library().mochi_shard_words(lo.shape[0] - 1, _ptr(lo)))


def bits_assemble(cert_lo: np.ndarray, gathered: np.ndarray) -> np.ndarray:
    """The batch's accept bitmap from the all-gathered per-shard slots (mochi_bits_assemble)."""
    lo = np.ascontiguousarray(cert_lo, np.uint32)
    g = np.ascontiguousarray(gathered, np.uint32)
    n = lo.shape[0] - 1
    out = np.zeros(max(1, (int(lo[-1]) + 31) // 32), np.uint32)
    if load_library().mochi_bits_assemble(n, _ptr(lo), g.shape[0] // n, _ptr(g), _ptr(out)) != OK:
        raise MochiError("mochi_bits_assemble failed")
    return out[:(int(lo[-1]) + 31) // 32]


class MultiVerifier:
    """mochi_mctx: one process, the GPUs of device_mask, one context + host thread
    each, RCCL all-gather of the verdict bitmaps."""

    def __init__(self, moduli_be, device_mask: int):
        self.lib = load_library()
        mod = np.ascontiguousarray(np.frombuffer(b"".join(bytes(m) for m in moduli_be), np.uint8))
        self._mod = mod
        self.h = self.lib.mochi_mctx_create(device_mask, mod.ctypes.data, mod.size // RSA_BYTES, RSA_BYTES, RSA_E)
        if not self.h:
            raise MochiError(f"mochi_mctx_create: {_err(self.lib)}")
        devs = (ctypes.c_int * 64)()
        self.devices = list(devs)[:self.lib.mochi_mctx_devices(self.h, devs, 64)]

    def set_server_ids(self, server_ids) -> None:
        enc = [x.encode() if isinstance(x, str) else bytes(x) for x in server_ids]
        blob = np.frombuffer(b"".join(enc) or b"\x00", np.uint8).copy()
        off = np.zeros(len(enc) + 1, np.uint32)
        np.cumsum([len(x) for x in enc], out=off[1:])
        if self.lib.mochi_mctx_set_server_ids(self.h, _ptr(blob), _ptr(off), len(enc)) != OK:
            raise MochiError(_err(self.lib))

    def verify(self, batch: Batch, replication_factor: int, strict_gt: bool = True, quorum_mode: int = 0) -> Verdicts:
        b = batch.normalized()
        out = Verdicts.alloc(b.n_grants, b.n_certs, b.n_ops)
        bc, vc = b.to_c(), out.to_c()
        vc.grant_valid_bits = None
        p = params(replication_factor, strict_gt, quorum_mode)
        rc = self.lib.mochi_mverify_batch(self.h, ctypes.byref(bc), ctypes.byref(p), ctypes.byref(vc))
        if rc != OK:
            raise MochiError(f"mochi_mverify_batch rc={rc}: {_err(self.lib)}")
        out.grant_valid_bits = np.zeros_like(out.grant_valid_bits)
        return out

    def verify_write2(self, wb, replication_factor: int, strict_gt: bool = True, quorum_mode: int = 0):
        wc, keep = write2_batch_c(wb)
        M = wb.n_msgs
        O = int(wb.op_flags_off[-1]) if wb.op_flags_off is not None else 0
        out = Verdicts.alloc(0, M, O)
        vc = out.to_c()
        vc.grant_valid_bits = vc.grant_flags = vc.grant_ts = None
        if wb.op_flags_off is None:
            vc.op_decision = vc.op_g0 = vc.op_ts = None
        p = params(replication_factor, strict_gt, quorum_mode)
        st = np.zeros(max(M, 1), np.uint8)
        rc = self.lib.mochi_mverify_write2(self.h, ctypes.addressof(wc), ctypes.addressof(p), ctypes.addressof(vc),
                                           _ptr(st))
        if rc != OK:
            raise MochiError(f"mochi_mverify_write2 rc={rc}: {_err(self.lib)}")
        return out, st[:M].copy()

    def gathered_bits(self, i: int):
        """(device pointer, words per device slot) of device i's all-gathered buffer."""
        p, w = ctypes.c_void_p(), ctypes.c_uint32()
        if self.lib.mochi_mctx_gathered_bits(self.h, i, ctypes.byref(p), ctypes.byref(w)) != OK:
            raise MochiError(_err(self.lib))
        return p.value, w.value

    def close(self):
        if self.h:
            self.lib.mochi_mctx_destroy(self.h)
            self.h = None


class Comm:
    """mochi_comm: one process per GPU; the verdict-bitmap all-gather through librccl."""

    def __init__(self, unique_id: bytes, n_ranks: int, rank: int, device: int):
        self.lib = load_library()
        idb = ctypes.create_string_buffer(bytes(unique_id), 128)
        self.h = self.lib.mochi_comm_init(idb, n_ranks, rank, device)
        if not self.h:
            raise MochiError(f"mochi_comm_init: {_err(self.lib)}")
        self.n_ranks = n_ranks

    @staticmethod
    def unique_id() -> bytes:
        lib = load_library()
        b = ctypes.create_string_buffer(128)
        if lib.mochi_comm_unique_id(b) != OK:
            raise MochiError(f"mochi_comm_unique_id: {_err(lib)}")
        return b.raw

    def allgather_bits(self, local_t, out_t, stream: int = 0) -> None:
        """int32 torch tensors: local [W] -> out [n_ranks * W] (async on `stream`)."""
        rc = self.lib.mochi_comm_allgather_bits(self.h, local_t.data_ptr(), local_t.numel(), out_t.data_ptr(), stream)
        if rc != OK:
            raise MochiError(f"mochi_comm_allgather_bits: {_err(self.lib)}")

    def close(self):
        if self.h:
            self.lib.mochi_comm_destroy(self.h)
            self.h = None


def properties_bytes(text: str) -> bytes:
    """A str as the bytes of a properties file Properties.load(InputStream) reads
    back as that str: ISO-8859-1 for U+0000..U+00FF, a \\uXXXX escape per UTF-16
    code unit above (a supplementary character becomes its surrogate pair)."""
    out = bytearray()
    for ch in text:
        cp = ord(ch)
        if cp <= 0xFF:
            out.append(cp)
        else:
            u = ch.encode("utf-16-be", "surrogatepass")
            for i in range(0, len(u), 2):
                out += b"\\u%04X" % int.from_bytes(u[i:i + 2], "big")
    return bytes(out)


class ClusterConfig:
    """The reference's cluster properties file (mochi_config_*;
    ClusterConfiguration.loadInitialConfigurationFromProperties,
    ClusterConfiguration.java:138-187)."""

    def __init__(self, path: Optional[str] = None, text=None):
        # text: the file's bytes (read as ISO-8859-1, like Properties.load(InputStream)),
        # or a str, written the way Properties.store would: ISO-8859-1, every
        # character above U+00FF as a \\uXXXX escape (UTF-16 units), so an id given
        # as a str reads back as that same str (not its UTF-8 bytes re-read as Latin-1)
        self.lib = load_library()
        if path is not None:
            self.h = self.lib.mochi_config_load(path.encode())
        else:
            raw = text if isinstance(text, (bytes, bytearray)) else properties_bytes(text or "")
            self.h = self.lib.mochi_config_parse(raw, len(raw))
        if not self.h:
            raise MochiError(f"mochi_config: {_err(self.lib)}")

    @property
    def replication_factor(self) -> int:
        return int(self.lib.mochi_config_replication(self.h))

    @property
    def majority(self) -> int:
        return int(self.lib.mochi_config_majority(self.h))

    def servers(self):
        n = self.lib.mochi_config_n_servers(self.h)
        return [(self.lib.mochi_config_server_id(self.h, i).decode(), self.lib.mochi_config_server_url(self.h, i).decode())
                for i in range(n)]

    def servers_for_key(self, key: str):
        """getServersForObject(key): indices into servers(), replica order."""
        kb = key.encode()
        out = np.zeros(self.replication_factor, np.uint32)
        rc = self.lib.mochi_config_servers_for_key(self.h, kb, len(kb), _ptr(out))
        if rc != OK:
            raise MochiError(f"mochi_config_servers_for_key: {_err(self.lib)}")
        return [int(i) for i in out]

    def replica_ids(self, key: Optional[str] = None):
        """(ids blob, id_off[R+1]) for mochi_ctx_set_server_ids."""
        kb = key.encode() if key is not None else None
        off = np.zeros(self.replication_factor + 1, np.uint32)
        need = self.lib.mochi_config_replica_ids(self.h, kb, len(kb) if kb else 0, None, 0, _ptr(off))
        if need < 0:
            raise MochiError(f"mochi_config_replica_ids: {_err(self.lib)}")
        blob = np.zeros(max(int(need), 1), np.uint8)
        self.lib.mochi_config_replica_ids(self.h, kb, len(kb) if kb else 0, _ptr(blob), int(need), _ptr(off))
        return blob[:int(need)], off

    def replica_id_list(self, key: Optional[str] = None):
        blob, off = self.replica_ids(key)
        b = blob.tobytes()
        return [b[off[i]:off[i + 1]].decode() for i in range(len(off) - 1)]

    def close(self):
        if getattr(self, "h", None):
            self.lib.mochi_config_free(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass
