"""Every Write2 wire form of w2_wire_corpus.py through every launch path of the wire
decoder (needs an MI355X): the single-block and the multi-kernel decode sequences on
either side of their 1024-message switch, the small- and large-batch verify sequences,
the chunked host pipeline and the device-resident entry point.

Every comparison is exact, array for array, against the oracle (O.w2_decode /
O.verify_write2 over the same WireBatch), per-op outputs included: every message, clean
or not, has caller op arrays here.  test_w2_wire_corpus_cpu.py shows what the corpus covers.
"""
import ctypes
import dataclasses

import numpy as np
import pytest

import mochi_hip as mh
import oracle_ffi as O
import w2_wire_corpus as WC
import workload as W
from test_write2_wire_cpu import _golden

pytestmark = pytest.mark.gpu

GUARD = 0x5A5AA5A5
KEYS = ("grant_off", "grant_len", "sig", "signer", "grant_key", "cert_grant_off", "cert_op_off", "op_key",
        "op_flags", "msg_status", "cert_mg_off", "mg_grant_off", "op_key_off", "op_key_len")
VERDICT_ARRAYS = ("cert_accept_bits", "cert_reason", "cert_fail_op", "op_decision", "op_g0", "op_ts")
BIG = max(WC.SIZES)


@pytest.fixture(scope="module")
def shared_ver():
    v = mh.Verifier(WC.pool().moduli, 0)
    v.set_server_ids(W.SERVER_IDS[:WC.R])
    yield v
    v.close()


@pytest.fixture
def ver(shared_ver):
    shared_ver.set_small_batch(4096)
    shared_ver.set_chunk_grants(0)
    yield shared_ver
    shared_ver.set_small_batch(4096)
    shared_ver.set_chunk_grants(0)


def assert_verdicts_equal(g, st, want, want_st, what):
    np.testing.assert_array_equal(st, want_st, err_msg=f"msg_status {what}")
    for k in VERDICT_ARRAYS:
        np.testing.assert_array_equal(getattr(g, k), getattr(want, k), err_msg=f"{k} {what}")


@pytest.mark.parametrize("M,how", [(M, "packed") for M in WC.SIZES] + [(min(WC.SIZES), "permuted"),
                                                                       (min(WC.SIZES), "shared"), (BIG, "shared")])
def test_decode_arrays(ver, M, how):
    """decode_write2 == O.w2_decode on both sides of the decoder's 1024-message switch (at 2100
    messages the shared layout has hundreds of offsets that up to eight messages point at)."""
    d, o = ver.decode_write2(WC.batch(M, how)[0]), WC.oracle_decode(M, how)
    for k in KEYS:
        np.testing.assert_array_equal(d[k], o[k], err_msg=f"{k} M={M} {how}")


def test_golden_vectors_on_the_large_path():
    """The golden protobuf vectors, cycled past 1024 messages: they had only met the
    single-block decode kernels."""
    vecs, ids, blob, off = _golden()
    v = mh.Verifier(WC.pool().moduli[:1] * len(ids), 0)
    v.set_server_ids(ids)
    msgs = WC.tile([bytes.fromhex(x["hex"]) for x in vecs], 1030)
    for pad in (1, 3):
        wb = WC._pack(msgs, pad=pad)
        d, o = v.decode_write2(wb), O.w2_decode(wb, blob, off)
        assert len(set(o["msg_status"].tolist())) == 3
        for k in KEYS:
            np.testing.assert_array_equal(d[k], o[k], err_msg=f"{k} golden x 1030 pad={pad}")
    v.close()


# the full cross product on one size of either decode sequence; the corner parameter sets elsewhere
FULL_CROSS = (600, 1024)


@pytest.mark.parametrize("small_batch", [4096, 0])
@pytest.mark.parametrize("M", WC.SIZES)
def test_verdicts_and_per_op_outputs(ver, M, small_batch):
    """verify_write2 == O.verify_write2: status, certificate verdicts and the per-op outputs
    of every message, under the small- and the large-batch verify sequence."""
    ver.set_small_batch(small_batch)
    wb = WC.batch(M)[0]
    for strict, qm in WC.PARAMS if M in FULL_CROSS else ((True, 0), (False, 3)):
        g, st = ver.verify_write2(wb, WC.R, strict, quorum_mode=qm)
        want, want_st = WC.oracle_verify(M, strict, qm)
        assert_verdicts_equal(g, st, want, want_st, f"M={M} strict={strict} qm={qm} small_batch={small_batch}")


def verify_write2_guarded(ver, wb, strict, qm):
    """ver.verify_write2 with cert_accept_bits one word longer than needed, every word preset."""
    wc, keep = mh.write2_batch_c(wb)
    M, n_ops = wb.n_msgs, int(wb.op_flags_off[-1])
    out = mh.Verdicts.alloc(0, M, n_ops)
    words = (M + 31) // 32
    out.cert_accept_bits = np.full(words + 1, GUARD, np.uint32)
    vc = out.to_c()
    vc.grant_valid_bits = vc.grant_flags = vc.grant_ts = None
    p = mh.params(WC.R, strict, qm)
    st = np.zeros(M, np.uint8)
    rc = ver.lib.mochi_verify_write2(ver.ctx, ctypes.addressof(wc), ctypes.addressof(p), ctypes.addressof(vc),
                                     st.ctypes.data)
    assert rc == mh.OK, rc
    guard = int(out.cert_accept_bits[words])
    out.cert_accept_bits = out.cert_accept_bits[:words].copy()
    return out, st, guard


@pytest.mark.parametrize("how", WC.LAYOUTS)
def test_chunked_pipeline(ver, how):
    """The chunked host pipeline on messages that are not clean: 32-message chunks (one in
    which nothing decodes, one of fallback messages only, one without a caller op, a partial
    last one) and a chunk of at least 1024 messages, bodies in order, permuted and shared.  Each
    == the unchunked result == the oracle, and no word past the accept bitmap is written."""
    wb = WC.batch(BIG, how)[0]
    large = WC.large_chunk_grants(wb.msg_len)
    for strict, qm in ((True, 0), (False, 3)):
        want, want_st = WC.oracle_verify(BIG, strict, qm, how)
        whole, whole_st = ver.verify_write2(wb, WC.R, strict, quorum_mode=qm)
        assert_verdicts_equal(whole, whole_st, want, want_st, f"unchunked {how} strict={strict} qm={qm}")
        for chunk in (1, large):
            ver.set_chunk_grants(chunk)
            g, st, guard = verify_write2_guarded(ver, wb, strict, qm)
            ver.set_chunk_grants(0)
            what = f"chunk_grants={chunk} {how} strict={strict} qm={qm}"
            assert guard == GUARD, f"wrote past the accept bitmap ({what})"
            assert_verdicts_equal(g, st, want, want_st, what)
            assert_verdicts_equal(g, st, whole, whole_st, what + " vs unchunked")


def device_expectation(M, strict, qm):
    """The oracle's result for mochi_verify_write2_device.  That entry only enqueues device work:
    no host decoder runs on it (wire forms x launch paths; the header is silent
    about it), so the rows the oracle reports MOCHI_MSG_FALLBACK stay undecided -- those rows
    alone are overwritten."""
    o, st = WC.oracle_verify(M, strict, qm)
    wb = WC.batch(M)[0]
    want = dataclasses.replace(o, **{k: getattr(o, k).copy() for k in VERDICT_ARRAYS})
    fb = np.nonzero(st == mh.MSG_FALLBACK)[0]
    assert fb.size >= M // 20
    for m in fb:
        want.cert_accept_bits[m >> 5] &= ~np.uint32(1 << (m & 31))
        lo, hi = int(wb.op_flags_off[m]), int(wb.op_flags_off[m + 1])
        want.op_decision[lo:hi], want.op_g0[lo:hi], want.op_ts[lo:hi] = mh.OPD_SKIPPED, 0xFFFFFFFF, 0
    want.cert_reason[fb], want.cert_fail_op[fb] = mh.UNDECIDED, 0xFF
    return want, st


@pytest.mark.parametrize("M", [600, 1024, BIG])
def test_device_resident(ver, M):
    """mochi_verify_write2_device on malformed, fallback and ops-mismatch rows."""
    import torch

    src = WC.batch(M)[0]
    wb = dataclasses.replace(src, **{f.name: getattr(src, f.name).copy() for f in dataclasses.fields(src)})
    dwb = mh.DeviceWireBatch(wb, 0)
    n_ops = int(wb.op_flags_off[-1])
    for small_batch, strict, qm in ((4096, True, 0), (4096, False, 3), (0, True, 0)):
        ver.set_small_batch(small_batch)
        out = mh.DeviceVerdicts(0, M, 0, full=True, n_ops=n_ops)
        for name in VERDICT_ARRAYS + ("status",):  # whatever is left unwritten shows
            getattr(dwb if name == "status" else out, name).fill_(0x6E)
        ver.verify_write2_device(dwb, out, WC.R, strict, stream=torch.cuda.current_stream().cuda_stream,
                                 quorum_mode=qm)
        torch.cuda.synchronize()
        want, want_st = device_expectation(M, strict, qm)
        assert_verdicts_equal(out.to_host(), dwb.status.cpu().numpy()[:M], want, want_st,
                              f"device-resident M={M} strict={strict} qm={qm} small_batch={small_batch}")
