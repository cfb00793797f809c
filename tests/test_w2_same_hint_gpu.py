"""The Write2 wire decoder's first-grant hint on the GPU (needs an MI355X): decode_write2's
"grant_same" is sound on every message (w2_same_hint.check_hint: it names only the message's
first grant, and only for byte-equal grants) and complete on the messages the model covers,
on the one-byte sweep around mg_match's window seams and length edges, on the wire corpus and
on the reference-grant adversaries -- and the consumer, k_grant_prep_cert, which trusts the
hint without a byte compare, reaches the oracle's verdicts on really signed grants, where a
false hint would show as an invalid signature.

Every comparison is exact.  test_w2_same_hint_cpu.py shows what the builders cover.
"""
import functools

import numpy as np
import pytest

import mochi_hip as mh
import oracle_ffi as O
import w2_same_hint as SH
import w2_wire_corpus as WC
import workload as W
from test_write2_wire_gpu import assert_decode_equal

pytestmark = pytest.mark.gpu

VERDICT_ARRAYS = ("cert_accept_bits", "cert_reason", "cert_fail_op", "op_decision", "op_g0", "op_ts")


@functools.lru_cache(maxsize=None)
def keys():
    pems = W.load_keys(SH.R)
    return pems, [W.pem_modulus(p) for p in pems]


@functools.lru_cache(maxsize=None)
def signature(r: int, gb: bytes) -> bytes:
    """Replica r's SHA256withRSA signature of gb, by the project's signer."""
    return mh.sign_grants(keys()[0][r], np.frombuffer(gb, np.uint8), np.zeros(1, np.uint64),
                          np.array([len(gb)], np.uint32), 1)[0].tobytes()


@pytest.fixture(scope="module")
def shared_ver():
    v = mh.Verifier(keys()[1], 0)
    v.set_server_ids(SH.IDS4)
    yield v
    v.close()


@pytest.fixture
def ver(shared_ver):
    shared_ver.set_small_batch(4096)
    shared_ver.set_chunk_grants(0)
    yield shared_ver
    shared_ver.set_small_batch(4096)
    shared_ver.set_chunk_grants(0)


def hinted_per_msg(dec, same):
    cgo = dec["cert_grant_off"].astype(np.int64)
    h = np.concatenate([[0], np.cumsum(same != np.arange(same.shape[0]))])
    return h[cgo[1:]] - h[cgo[:-1]]


def decode_checks(ver, wb, what):
    """decode_write2 == the oracle's decode, its hint sound everywhere and complete where the
    model applies; returns (device decode, oracle decode, qualifying messages, hinted grants per message)."""
    d, o = ver.decode_write2(wb), SH.fast_decode(wb)
    np.testing.assert_array_equal(d["msg_status"], o["msg_status"], err_msg=f"msg_status {what}")
    assert_decode_equal(d, o, what)
    same = d["grant_same"]
    assert same.dtype == np.uint32 and same.shape == d["grant_len"].shape
    unsound = SH.check_hint(wb.wire, d, same)
    assert unsound == [], f"{what}: unsound hints (message, grant, rule) {unsound[:8]}"
    bad, qual = SH.model_violations(wb, o["msg_status"], o, same)
    assert bad == [], f"{what}: (message, grant, hint, expected) {bad[:8]} of {len(bad)}"
    return d, o, qual, hinted_per_msg(d, same)


@pytest.mark.parametrize("M", [1023, 1025])
def test_sweep_hint(ver, M, capsys):
    """The whole sweep in batches of M messages, below and above the decoder's switch from its
    single-block kernels (kW2SmallM = 1024).  Prints, per grant length, the messages decoded
    and the grants hinted (two per one-byte message, three per message of equal grants)."""
    msgs = SH.sweep()
    ok, hinted = {gl: 0 for gl in SH.GLS}, {gl: 0 for gl in SH.GLS}
    seen = 0
    for t, tile in enumerate(SH.tiles(msgs, M)):
        wb = SH.pack(tile)
        d, o, qual, h = decode_checks(ver, wb, f"sweep M={M} tile {t}")
        qual = set(qual)
        for i, m in enumerate(tile):
            if seen + i >= len(msgs):  # the fill of the last batch: counted once
                break
            if o["msg_status"][i] == SH.MSG_OK:
                assert i in qual, (m.kind, m.gl, m.kl, m.p)
                ok[m.gl] += 1
                hinted[m.gl] += int(h[i])
        seen += len(tile)
    with capsys.disabled():
        print(f"\nsweep M={M}: gl: messages OK / built, grants hinted")
        for gl in SH.GLS:
            n = sum(1 for m in msgs if m.gl == gl)
            print(f"  gl={gl}: {ok[gl]} / {n}, {hinted[gl]}")
    for gl in SH.GLS:  # each of the 2 key lengths: gl positions less the structural ones, the status variant, the equal grants
        assert ok[gl] >= 2 * (gl - SH.MAX_STRUCTURAL + 2) and hinted[gl] >= 2 * (2 * (gl - SH.MAX_STRUCTURAL + 1) + 3)


def test_sweep_chunked_pipeline(ver):
    """The sweep as one batch with the host pipeline cut into 32-message chunks: the verify call
    decodes chunk by chunk (hints relative to each launch, consumed by that chunk's prep) and
    reports the oracle's statuses and verdicts; the decode-only call stays one launch whatever
    the chunk target, so its hint indices are batch-global as they come."""
    msgs = SH.sweep()
    wb = SH.pack(msgs)
    assert len(WC.chunk_plan(wb.msg_len, 1)) > 32
    ver.set_chunk_grants(1)
    d, o, qual, h = decode_checks(ver, wb, "sweep, one batch, chunk_grants=1")
    assert d["grant_same"].max() > SH.R * 1025  # indices past any the batches of test_sweep_hint reach
    ids, ido = W.server_id_table(SH.R)
    for strict in (True, False):
        g, st = ver.verify_write2(wb, SH.R, strict)
        want, want_st = O.verify_write2(keys()[1], ids, ido, wb, SH.R, strict)
        np.testing.assert_array_equal(st, want_st)
        np.testing.assert_array_equal(st, o["msg_status"])
        for k in VERDICT_ARRAYS[:3]:
            np.testing.assert_array_equal(getattr(g, k), getattr(want, k), err_msg=f"{k} strict={strict}")


@pytest.mark.parametrize("M", [600, 1025])
def test_corpus_hint(ver, M):
    """Every wire form of the corpus (matcher forms, fallback forms, fuzz kinds): sound, and
    complete on the messages that qualify; the plain matcher form qualifies and is hinted."""
    wb, kinds, _, _ = WC.batch(M)
    d, o, qual, h = decode_checks(ver, wb, f"corpus M={M}")
    qual = np.array(sorted(qual))
    plain = np.nonzero((kinds == "matcher:plain") & (o["msg_status"] == mh.MSG_OK))[0]
    assert plain.size >= 2 and np.isin(plain, qual).all()
    assert (h[plain] == WC.R - 1).all()
    assert qual.size > M // 3 and h[qual].sum() > qual.size  # much of the corpus takes part


def test_adversaries(ver):
    """First MultiGrants whose first grants entry is not the message's first decoded grant, or
    that the reference parse declines: no unsound hint, and with real signatures the verdicts
    are the oracle's (a follower given the wrong grant's digest would fail its signature)."""
    adv = SH.adversaries(signature)
    wb = SH.pack(adv, with_ops=True)
    decode_checks(ver, wb, "adversaries")
    ids, ido = W.server_id_table(SH.R)
    for small_batch in (4096, 0):
        ver.set_small_batch(small_batch)
        for strict in (True, False):
            g, st = ver.verify_write2(wb, SH.R, strict)
            want, want_st = O.verify_write2(keys()[1], ids, ido, wb, SH.R, strict)
            np.testing.assert_array_equal(st, want_st)
            for k in VERDICT_ARRAYS:
                np.testing.assert_array_equal(getattr(g, k), getattr(want, k),
                                              err_msg=f"{k} strict={strict} small_batch={small_batch}")
            acc = {m.kind for m, a in zip(adv, want.cert_accept) if a}
            assert {"adv:server_id_first:first", "adv:grant_key_128:first", "adv:first_grant_193:first",
                    "adv:first_grant_reordered:first", "adv:repeated_grant_key:last"} <= acc, acc


@functools.lru_cache(maxsize=None)
def signed_sweep():
    msgs = SH.sweep(signature, SH.verdict_positions)
    return msgs, SH.pack(msgs, with_ops=True)


def oracle_batch(wb, o):
    """The oracle's decode as the SoA batch the verify path is given."""
    return mh.Batch(grant_bytes=wb.wire, expected_hash=wb.expected_hash,
                    **{k: o[k] for k in ("grant_off", "grant_len", "sig", "signer", "grant_key", "cert_grant_off",
                                         "cert_op_off", "op_key", "op_flags", "cert_mg_off", "mg_grant_off",
                                         "op_object_ts", "op_key_off", "op_key_len")})


@functools.lru_cache(maxsize=None)
def signed_sweep_oracle(strict: bool):
    """(the oracle's wire verdicts and statuses, its decode, O.verify_batch over that decode)."""
    msgs, wb = signed_sweep()
    ids, ido = W.server_id_table(SH.R)
    want, want_st = O.verify_write2(keys()[1], ids, ido, wb, SH.R, strict)
    o = O.w2_decode(wb, ids, ido)
    return want, want_st, o, O.verify_batch(keys()[1], oracle_batch(wb, o), SH.R, strict)


@pytest.mark.parametrize("small_batch,chunk", [(0, 0), (0, 1), (4096, 0)])
def test_verdicts_on_signed_sweep(ver, small_batch, chunk):
    """The consumer: every replica signs its own bytes, so each grant verifies under its OWN
    digest only.  verify_write2 == O.verify_batch over the oracle's decode == O.verify_write2:
    verdicts, reasons, failing op and per-op outputs; by the oracle every signature is valid,
    and the one-byte variants reject with TS_MISMATCH / HASH_MISMATCH exactly where it says.
    small_batch = 0 is the large-batch verify sequence, the one whose prep dedups grants and so
    reads the hint -- in one launch, and chunk by chunk (32 messages each, the hint relative to
    the chunk); the small-batch sequence preps every grant on its own and must agree."""
    msgs, wb = signed_sweep()
    ver.set_small_batch(small_batch)
    ver.set_chunk_grants(chunk)
    ofo = wb.op_flags_off
    for strict in (True, False):
        want, want_st, o, vb = signed_sweep_oracle(strict)
        g, st = ver.verify_write2(wb, SH.R, strict)
        what = f"strict={strict} small_batch={small_batch} chunk_grants={chunk}"
        np.testing.assert_array_equal(st, want_st, err_msg=what)
        for k in VERDICT_ARRAYS:
            np.testing.assert_array_equal(getattr(g, k), getattr(want, k), err_msg=f"{k} {what}")
        # ... and the SoA oracle over the oracle's decode, on the decoded messages
        ok = np.nonzero(want_st == mh.MSG_OK)[0]
        assert ok.size > len(msgs) * 3 // 4
        n_g = np.diff(o["cert_grant_off"].astype(np.int64))
        assert (n_g[ok] == SH.R).all()
        assert (vb.grant_flags & mh.GRANT_SIG_OK).all() and (vb.grant_flags & mh.GRANT_PARSED).all()
        np.testing.assert_array_equal(g.cert_accept[ok], vb.cert_accept[ok], err_msg=what)
        np.testing.assert_array_equal(g.cert_reason[ok], vb.cert_reason[ok], err_msg=what)
        np.testing.assert_array_equal(g.cert_fail_op[ok], vb.cert_fail_op[ok], err_msg=what)
        coo = o["cert_op_off"]
        assert (np.diff(coo.astype(np.int64))[ok] == 1).all()
        for k in ("op_decision", "op_g0", "op_ts"):
            np.testing.assert_array_equal(getattr(g, k)[ofo[ok]], getattr(vb, k)[coo[ok]], err_msg=f"{k} {what}")
        reasons = set(g.cert_reason[ok].tolist())
        assert {mh.REJECT_TS_MISMATCH, mh.REJECT_HASH_MISMATCH} <= reasons, reasons
        real = np.array([m.gl == SH.REAL_GL for m in msgs])
        equal = np.array([m.kind == "equal" for m in msgs])
        assert g.cert_accept[real & equal].all() and (real & equal).sum() == len(SH.KLS)  # four valid equal grants
