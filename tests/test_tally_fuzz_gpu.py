"""Certificate tally on the device == oracle_tally on the fuzz batches of tally_fuzz.py
(needs an MI355X): up to MOCHI_MAX_OPS_PER_CERT ops per certificate, repeated and shuffled
key slots, certificates of unequal size, every launch sequence and both grant layouts.

Every comparison is exact, array for array.  The oracle's grant flags come from OpenSSL
once per batch (oracle verify_grants); each parameter set then costs one oracle_tally.
test_tally_fuzz_cpu.py shows what the batches cover.
"""
import ctypes
import functools

import numpy as np
import pytest

import mochi_hip as mh
import oracle_ffi as O
import tally_fuzz as TF
import workload as W

pytestmark = pytest.mark.gpu

SEED = 20260  # the batches test_tally_fuzz_cpu.py asserts coverage for
GUARD = 0x5A5AA5A5
CERT_OP_ARRAYS = ("cert_accept_bits", "cert_reason", "cert_fail_op", "op_decision", "op_g0", "op_ts")
DECODE_KEYS = ("grant_off", "grant_len", "sig", "signer", "grant_key", "cert_grant_off", "cert_op_off", "op_key",
               "op_flags", "msg_status", "cert_mg_off", "mg_grant_off", "op_key_off", "op_key_len")


@functools.lru_cache(maxsize=None)
def fuzz(R):
    """The batch, and the oracle's (OpenSSL's) grant flags and timestamps for it, once."""
    fz = TF.make(R, SEED)
    flags, ts = O.verify_grants(fz.moduli, fz.batch, 0, fz.batch.n_grants, 8)
    return fz, flags, ts


@functools.lru_cache(maxsize=None)
def oracle(R, n_certs, strict, qm, csr):
    """oracle_tally over the first n_certs certificates (the grant layout does not matter to it)."""
    fz, flags, ts = fuzz(R)
    b = TF.head(fz.batch, n_certs)
    return O.tally(b if csr else TF.without_csr(b), flags[:b.n_grants], ts[:b.n_grants], R, strict, qm)


def check(g, R, n_certs, strict, qm, csr, what):
    """Device verdicts g of the first n_certs certificates == the oracle, every array."""
    _, flags, ts = fuzz(R)
    what = f"{what} R={R} C={n_certs} strict={strict} qm={qm} csr={csr}"
    n = g.grant_flags.shape[0]
    np.testing.assert_array_equal(g.grant_flags, flags[:n], err_msg=f"grant_flags {what}")
    np.testing.assert_array_equal(g.grant_ts, ts[:n], err_msg=f"grant_ts {what}")
    bits = np.packbits((flags[:n] & mh.GRANT_SIG_OK).astype(bool), bitorder="little")
    bits = np.concatenate([bits, np.zeros(-bits.size % 4, np.uint8)]).view("<u4")
    np.testing.assert_array_equal(g.grant_valid_bits, bits, err_msg=f"grant_valid_bits {what}")
    o = oracle(R, n_certs, strict, qm, csr)
    for k in CERT_OP_ARRAYS:
        np.testing.assert_array_equal(getattr(g, k), getattr(o, k), err_msg=f"{k} {what}")


def layouts(b):
    return (("separate", b), ("shared", TF.shared_copies(b)))


# One lane of k_tally walks a whole certificate, and with MOCHI_Q_DISTINCT_SIGNERS / MOCHI_Q_BIND
# it re-derives which grants count per (op, grant): the 64-op certificates take it 0.1-0.4 s per
# call over the whole batch (measured, MI355X), against 10-20 ms in mode 0.  So the leading
# certificates (every deep shape class, 1/5 of the grants) see the full cross product, and the
# whole batch sees mode 0 under every (strict, CSR, layout) and the other modes under four sets
# that rotate strict, CSR and layout: (strict, quorum_mode, csr).
WHOLE_BATCH_MODES = {"separate": {(True, 1, True), (False, 3, False)},
                     "shared": {(False, 2, True), (True, 1, False)}}


@pytest.fixture(scope="module")
def vers():
    made = {}

    def get(R):
        if R not in made:
            made[R] = mh.Verifier(fuzz(R)[0].moduli, 0)
            made[R].set_server_ids(W.SERVER_IDS[:R])
        v = made[R]
        v.set_small_batch(4096)
        v.set_chunk_grants(0)
        return v

    yield get
    for v in made.values():
        v.close()


@pytest.mark.parametrize("seq", ["large", "default"])
@pytest.mark.parametrize("R", [4, 7])
def test_fuzz_tally_matches_oracle(vers, R, seq):
    """The whole batch and its leading certificates of at most 4096 grants, which take the
    small-batch sequence under `default` (per-grant prep, k_tally<false>) and the large one
    under `large` (staged / lane-by-lane k_grant_prep_cert, k_grant_match on separate copies,
    equal offsets on shared ones, k_tally<true> outside MOCHI_Q_BIND)."""
    fz, _, _ = fuzz(R)
    ver = vers(R)
    if seq == "large":
        ver.set_small_batch(0)
    n_head = TF.certs_within(fz.batch, 4096)
    assert sum(k.startswith("deep") for k in fz.kind[:n_head]) >= 8
    for n_certs in (fz.batch.n_certs, n_head):
        part = TF.head(fz.batch, n_certs)
        for csr in (True, False):
            for name, b in layouts(part if csr else TF.without_csr(part)):
                for strict in (True, False):
                    for qm in (0, 1, 2, 3):
                        if n_certs != n_head and qm and (strict, qm, csr) not in WHOLE_BATCH_MODES[name]:
                            continue
                        g = ver.verify(b, R, strict, quorum_mode=qm)
                        check(g, R, n_certs, strict, qm, csr, f"{seq} {name}")


def test_fuzz_tally_chunked_and_device_resident(vers):
    """The chunked host pipeline on certificates of unequal size (rebased CSR arrays, a launch
    sequence picked per chunk) and the device-resident entry point: each == the unchunked host
    result == the oracle."""
    import torch

    R = 4
    fz, _, _ = fuzz(R)
    ver = vers(R)
    C = fz.batch.n_certs
    cgo = np.asarray(fz.batch.cert_grant_off, np.int64)
    chunk32 = np.diff(cgo[np.r_[np.arange(0, C, 32), C]])
    assert chunk32.max() > 4096 > chunk32.min()  # 32-certificate chunks on both sides of the small-batch threshold
    # mode 0 on every (CSR, layout); the slow modes (see WHOLE_BATCH_MODES) once each
    extra = {(True, "separate"): (False, 3), (False, "shared"): (True, 1)}
    for csr in (True, False):
        for name, b in layouts(fz.batch if csr else TF.without_csr(fz.batch)):
            for strict, qm in [(True, 0)] + ([extra[csr, name]] if (csr, name) in extra else []):
                ver.set_chunk_grants(0)
                whole = ver.verify(b, R, strict, quorum_mode=qm)
                check(whole, R, C, strict, qm, csr, f"unchunked {name}")
                results = {}
                for chunk in (1, 1000):
                    ver.set_chunk_grants(chunk)
                    results[f"chunk {chunk}"] = ver.verify(b, R, strict, quorum_mode=qm)
                dev = mh.DeviceBatch(b, 0)
                out = mh.DeviceVerdicts(dev.n_grants, dev.n_certs, 0, full=True, n_ops=dev.n_ops)
                ver.verify_device(dev, out, R, strict, stream=torch.cuda.current_stream().cuda_stream, quorum_mode=qm)
                torch.cuda.synchronize()
                results["device-resident"] = out.to_host()
                for how, g in results.items():
                    check(g, R, C, strict, qm, csr, f"{how} {name}")
                    for k in ("grant_flags", "grant_ts", "grant_valid_bits") + CERT_OP_ARRAYS:
                        np.testing.assert_array_equal(getattr(g, k), getattr(whole, k), err_msg=f"{k} {how} {name}")


def verify_host_guarded(ver, b, R, strict, qm):
    """ver.verify with cert_accept_bits one word longer than needed, every word preset."""
    b = b.normalized()
    out = mh.Verdicts.alloc(b.n_grants, b.n_certs, b.n_ops)
    words = (b.n_certs + 31) // 32
    out.cert_accept_bits = np.full(words + 1, GUARD, np.uint32)
    bc, vc, p = b.to_c(), out.to_c(), mh.params(R, strict, qm)
    rc = ver.lib.mochi_verify_batch(ver.ctx, ctypes.byref(bc), ctypes.byref(p), ctypes.byref(vc))
    assert rc == mh.OK, rc
    guard = int(out.cert_accept_bits[words])
    out.cert_accept_bits = out.cert_accept_bits[:words].copy()
    return out, guard


@pytest.mark.parametrize("n_certs", [1, 31, 32, 33, 63, 64, 65, 255, 256, 257])
def test_fuzz_tally_bitmap_edges(vers, n_certs):
    """k_tally's ballot writes two words per wave: certificate counts around the word, wave
    and block sizes write every word of the bitmap and none after it."""
    import torch

    R = 4
    fz, _, _ = fuzz(R)
    ver = vers(R)
    b = TF.head(fz.batch, n_certs)
    words = (n_certs + 31) // 32
    for small in (4096, 0):
        ver.set_small_batch(small)
        g, guard = verify_host_guarded(ver, b, R, True, 0)
        assert guard == GUARD, f"host path wrote past the bitmap (small_batch={small})"
        check(g, R, n_certs, True, 0, True, f"host small_batch={small}")
        dev = mh.DeviceBatch(b, 0)
        out = mh.DeviceVerdicts(dev.n_grants, dev.n_certs, 0, full=True, n_ops=dev.n_ops)
        out.cert_accept_bits = torch.from_numpy(np.full(words + 1, GUARD, np.uint32).view(np.int32)).to("cuda:0")
        ver.verify_device(dev, out, R, True, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        h = out.to_host()
        assert int(h.cert_accept_bits[words]) == GUARD, f"k_tally wrote past the bitmap (small_batch={small})"
        h.cert_accept_bits = h.cert_accept_bits[:words].copy()
        if dev.n_ops == 0:  # no per-op arrays were passed
            h.op_decision, h.op_g0, h.op_ts = (np.zeros(0, dt) for dt in (np.uint8, np.uint32, np.int64))
        check(h, R, n_certs, True, 0, True, f"device-resident small_batch={small}")


def einval(ver, b, R):
    with pytest.raises(mh.MochiError) as e:
        ver.verify(b, R, True)
    assert f"rc={mh.EINVAL}" in str(e.value), e.value
    return str(e.value)


def test_ops_limit(vers):
    """MOCHI_MAX_OPS_PER_CERT on both entry points: 64 ops verify, 65 are refused (SoA:
    MOCHI_EINVAL, as an op key slot of 64 is) or left undecided (wire: MSG_FALLBACK)."""
    R = 4
    ver = vers(R)
    mods = fuzz(R)[0].moduli
    rng = np.random.default_rng(SEED)
    shapes = [(1, 0, 1), (4, 3, 2), (5, 4, 4), (32, 31, 16), (63, 32, 62), (64, 63, 64), (64, 32, 32), (65, 64, 32)]
    certs = [TF.deep_cert(rng, R, k, J, d, "none") for k, J, d in shapes]
    certs += [TF.deep_cert(rng, R, 64, 63, 63, f) for f in ("drop_all", "bad_then_evil", "flag19")]
    # --- SoA ---
    for cert in certs:
        b, _, _ = TF.assemble([cert], R, rng)
        if len(cert.ops) > mh.MAX_OPS_PER_CERT:
            assert "more than 64 ops" in einval(ver, b, R)
            continue
        for strict in (True, False):
            for qm in (0, 3):
                g = ver.verify(b, R, strict, quorum_mode=qm)
                o = O.verify_batch(mods, b, R, strict, 4, quorum_mode=qm)
                for k in ("grant_flags", "grant_ts", "grant_valid_bits") + CERT_OP_ARRAYS:
                    np.testing.assert_array_equal(getattr(g, k), getattr(o, k), err_msg=f"{k} {cert.kind}")
                if cert.fault_op < 0:
                    assert g.cert_accept.all() and g.cert_fail_op[0] == 0xFF
                else:
                    assert g.cert_fail_op[0] == cert.fault_op == 63
    b, _, _ = TF.assemble([certs[1]], R, rng)
    b.op_key[-1] = 64
    assert "op_key[3] >= 64" in einval(ver, b, R)
    # --- wire: the same certificates as Write2ToServer messages, ops of a slot repeating operand1 ---
    wb = TF.wire_batch(certs, R)
    ids, off = W.server_id_table(R)
    d, od = ver.decode_write2(wb), O.w2_decode(wb, ids, off)
    for k in DECODE_KEYS:
        np.testing.assert_array_equal(d[k], od[k], err_msg=k)
    n_ops = np.array([len(c.ops) for c in certs])
    want_status = np.where(n_ops > mh.MAX_OPS_PER_CERT, mh.MSG_FALLBACK, mh.MSG_OK)
    np.testing.assert_array_equal(d["msg_status"], want_status)
    for strict in (True, False):
        for qm in (0, 3):
            g, st = ver.verify_write2(wb, R, strict, quorum_mode=qm)
            o, ost = O.verify_write2(mods, ids, off, wb, R, strict, quorum_mode=qm)
            np.testing.assert_array_equal(st, ost)
            np.testing.assert_array_equal(st, want_status)
            for k in CERT_OP_ARRAYS:
                np.testing.assert_array_equal(getattr(g, k), getattr(o, k), err_msg=f"wire {k} strict={strict} qm={qm}")
            for c, cert in enumerate(certs):
                if len(cert.ops) > mh.MAX_OPS_PER_CERT:
                    assert g.cert_reason[c] == mh.UNDECIDED and not g.cert_accept[c]
                    assert (g.op_decision[wb.op_flags_off[c]:wb.op_flags_off[c + 1]] == mh.OPD_SKIPPED).all()
                elif cert.fault_op < 0:
                    assert g.cert_reason[c] == mh.ACCEPT and g.cert_accept[c], cert.kind
                else:
                    assert g.cert_fail_op[c] == 63, cert.kind
