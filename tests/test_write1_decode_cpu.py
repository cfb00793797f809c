"""Write1 reply decoder, host form (mochi_write1_reply_decode): array for array equal to
the plain-Python model (write1_decode_model, itself cross-checked against
google.protobuf) on every body the reply encoder produces and on a mutation corpus; the
round trip of the reply encoder's inputs; what the corpus covers; the capacity rule;
argument errors."""
import numpy as np
import pytest

import mochi_hip as mh
import write1_decode_model as DM
import write1_issue_model as M
import write1_reply_model as RM

replies_of, SERVER_IDS = DM.replies_of, DM.REPLY_SERVER_IDS


def check(replies, ids=DM.IDS, what=""):
    want = DM.decode(replies, ids)
    got = mh.write1_reply_decode(replies, ids)
    assert got.rc == mh.OK and got.n_grants == len(want["grant_off"]) and got.n_certs == len(want["cert_key_off"])
    DM.assert_equal(got.trimmed(), want, what)
    bg, bc = mh.write1_reply_decode_bound(np.asarray(replies.wire).size, replies.n_resps)
    assert bg >= got.n_grants and bc >= got.n_certs
    return got, want


@pytest.fixture(scope="module")
def corpus_batch():
    return DM.batch(DM.corpus())


# 1. the model against google.protobuf ------------------------------------------------
def test_model_agrees_with_google_protobuf():
    pytest.importorskip("google.protobuf")
    seen = set()
    for c in DM.corpus():
        if c.kind in (mh.W1_OK, mh.W1_REFUSED) and c.body not in seen:
            seen.add(c.body)
            DM.crosscheck(c.body, DM.decode_body(c.body))
    for case in RM.hand_cases().values():
        r = replies_of(case)
        wire = r.wire.tobytes()
        for p in range(r.n_resps):
            body = wire[int(r.resp_off[p]):int(r.resp_off[p]) + int(r.resp_len[p])]
            DM.crosscheck(body, DM.decode_body(body))


# 2. every body the reply encoder produces ---------------------------------------------
@pytest.mark.parametrize("name", sorted(RM.reply_cases()))
def test_reply_encoder_bodies_equal_the_model(name):
    check(replies_of(RM.reply_cases()[name]), SERVER_IDS, name)


def test_issue_case_bodies_equal_the_model():
    for name, case in RM.issue_cases().items():
        check(replies_of(case), SERVER_IDS, name)


def test_round_trip_of_the_reply_encoder():
    """Real WriteCertificates: the listed grants, signatures, keys and certificates come back."""
    cert_of = lambda k: DM.writecert([k, b"other"]) if k != b"q" else b""
    cases = {"refused_mixed": RM.from_requests(M._store({b"a": 1000, b"b": 2000}, [(b"a", 5, M.H(9))]),
                                               [M.Request(5, M.H(1), [(M.WRITE, b"b")]),
                                                M.Request(5, M.H(2), [(M.WRITE, b"a"), (M.WRITE, b"b")])], cert_of=cert_of),
             "two_keys": RM.from_requests(M._store({}), [M.Request(i, M.H(i), [(M.WRITE, b"p"), (M.WRITE, b"q")])
                                                         for i in range(5)], cert_of=cert_of),
             "ok_64_ops": RM.from_requests(M._store({}), [M.Request(3, M.H(1), [(M.WRITE, b"key-%02d" % i)
                                                                              for i in range(64)])], cert_of=cert_of)}
    for name, case in cases.items():
        batch, issued, src = case
        r = replies_of(case)
        got, _ = check(r, SERVER_IDS, name)
        d = got.trimmed()
        wire = r.wire.tobytes()
        strings = np.asarray(batch.strings, np.uint8).tobytes()
        assert (d["resp_status"] == mh.W1R_OK).all() and (d["mg_signer"][issued.req_kind != mh.W1K_THROWS] == 1).all()
        np.testing.assert_array_equal(np.diff(d["resp_grant_off"].astype(np.int64)), np.diff(issued.req_grant_off.astype(np.int64)))
        assert d["grant_flags"].tolist() == [mh.W1G_HAS_SIG] * got.n_grants
        n_certs = 0
        for q in range(batch.n_reqs):
            o0 = int(batch.req_op_off[q])
            for i, e in enumerate(range(int(issued.req_grant_off[q]), int(issued.req_grant_off[q + 1]))):
                g = int(d["resp_grant_off"][q]) + i
                ref = int(issued.req_grant[e])
                if ref & mh.W1_STORED:
                    j = ref & ~mh.W1_STORED
                    want = src.stored_bytes[int(src.stored_off[j]):int(src.stored_off[j]) + int(src.stored_len[j])].tobytes()
                    sig = np.asarray(src.stored_sig).reshape(-1, 256)[j]
                else:
                    want, sig = issued.grant(ref), np.asarray(issued.sig).reshape(-1, 256)[ref]
                assert wire[int(d["grant_off"][g]):int(d["grant_off"][g]) + int(d["grant_len"][g])] == want
                np.testing.assert_array_equal(d["sig"][g], sig)
                o = o0 + int(d["grant_key"][g])
                key = strings[int(batch.op_key_off[o]):int(batch.op_key_off[o]) + int(batch.op_key_len[o])]
                assert key == DM.parse_grant(want, 0, len(want)).object_id
                n_certs += bool(cert_of(key))
        keys = [wire[int(a):int(a) + int(b)] for a, b in zip(d["cert_key_off"], d["cert_key_len"])]
        vals = [wire[int(a):int(a) + int(b)] for a, b in zip(d["cert_val_off"], d["cert_val_len"])]
        assert n_certs == got.n_certs and all(v == cert_of(k) for k, v in zip(keys, vals))


# 3. the mutation corpus ------------------------------------------------------------------
def test_corpus_equals_the_model(corpus_batch):
    check(corpus_batch, DM.IDS, "corpus")


def test_corpus_in_aliased_slices_equals_the_model():
    cases = DM.corpus()
    r = DM.batch(cases + cases[::-1], layout="shared", per_req=3)
    assert len(set(r.resp_off.tolist())) < r.n_resps
    check(r, DM.IDS, "shared")


def test_corpus_reaches_every_status_and_flag(corpus_batch):
    want = DM.decode(corpus_batch, DM.IDS)
    assert set(want["resp_status"].tolist()) == {mh.W1R_OK, mh.W1R_MALFORMED, mh.W1R_FALLBACK, mh.W1R_UNKNOWN_SERVER}
    fl = want["grant_flags"]
    assert {int(f) & 1 for f in fl} == {0, 1} and {int(f) & 2 for f in fl} == {0, 2}
    assert 0xFF in want["grant_key"] and 0 in want["grant_key"] and 0xFF in want["grant_status"]
    assert (np.diff(want["resp_cert_off"].astype(np.int64)) > 1).any()
    st = {c.name: int(s) for c, s in zip(DM.corpus(), want["resp_status"])}
    for name, s in st.items():  # every form named for a status has it
        if name.startswith("fb:"):
            assert s == mh.W1R_FALLBACK, name
        if name.startswith("mal:") or name.startswith("utf8:") and "ok" not in name:
            assert s == mh.W1R_MALFORMED, name
        if name.startswith("ok:") or name.startswith("rep:"):
            assert s == mh.W1R_OK, name
    assert st["sid:unknown"] == st["sid:empty"] == st["degenerate:empty"] == mh.W1R_UNKNOWN_SERVER
    assert st["degenerate:one_byte"] == st["degenerate:ff_8"] == mh.W1R_MALFORMED
    assert st["sid:repeated"] == mh.W1R_OK and st["sid:repeated_to_unknown"] == mh.W1R_UNKNOWN_SERVER
    # a reply nobody decoded never counts as an empty OK
    bad = np.isin(want["resp_status"], [mh.W1R_MALFORMED, mh.W1R_FALLBACK])
    assert (want["resp_kind_out"][bad] == mh.W1_OTHER).all()
    assert (want["resp_kind_out"][~bad] == corpus_batch.resp_kind[~bad]).all()


# 4. the capacity rule ---------------------------------------------------------------------
@pytest.mark.parametrize("short", ["grants", "certs"])
def test_capacity_one_short_touches_nothing(corpus_batch, short):
    full = mh.write1_reply_decode(corpus_batch, DM.IDS)
    N, C = full.n_grants, full.n_certs
    assert N > 1 and C > 1
    got = mh.write1_reply_decode_into(corpus_batch, DM.IDS, N - (short == "grants"), C - (short == "certs"), fill=0xA5)
    assert got.rc == mh.EINVAL and (got.n_grants, got.n_certs) == (N, C)
    for k, (dt, w) in mh._W1D_OUT.items():
        if w in ("N", "C"):
            assert (got.arrays[k].view(np.uint8) == 0xA5).all(), k
        else:
            np.testing.assert_array_equal(got.arrays[k], full.arrays[k])
    assert (got.arrays["sig"] == 0xA5).all()
    exact = mh.write1_reply_decode_into(corpus_batch, DM.IDS, N, C, want_sig=False, fill=0xA5)
    assert exact.rc == mh.OK and "sig" not in exact.arrays
    np.testing.assert_array_equal(exact.arrays["grant_ts"], full.arrays["grant_ts"])


# 5. argument errors --------------------------------------------------------------------------
def test_argument_errors(corpus_batch):
    import dataclasses
    r = DM.batch(DM.corpus()[:8])
    bad = [dataclasses.replace(r, resp_len=np.where(np.arange(8) == 3, r.wire.size, r.resp_len).astype(np.uint32)),
           dataclasses.replace(r, resp_kind=np.full(8, 4, np.uint8)),
           dataclasses.replace(r, req_resp_off=np.array([0, 4, 7], np.uint32)),
           dataclasses.replace(r, op_key_len=(r.op_key_len + r.strings.size).astype(np.uint32))]
    for b in bad:
        with pytest.raises(mh.MochiError, match="mochi_write1_reply_decode"):
            mh.write1_reply_decode(b, DM.IDS)
