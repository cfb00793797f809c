"""Write1 reply decoder, host form (mochi_write1_reply_decode): array for array equal to
the plain-Python model (write1_decode_model, itself cross-checked against
google.protobuf) on every body the reply encoder produces and on a mutation corpus; the
round trip of the reply encoder's inputs; what the corpus covers; the bodies and batches
the GPU tests use at the device form's launch edges (heavy bodies, the level-2 pattern,
requests without responses or ops, a signature ending the wire); the capacity rule;
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


def test_corpus_signature_sources_cover_every_residue(corpus_batch):
    """The signature gather reads whole 16-byte chunks: every position of a source in its chunk occurs."""
    src = DM.sig_sources(corpus_batch, DM.decode(corpus_batch, DM.IDS))
    assert {s % 16 for s in src} == set(range(16))


# 3b. the bodies and batches of the device form's launch edges -------------------------------
def test_heavy_bodies_have_the_status_their_name_says():
    ec = DM.edge_cases()
    st = {n: DM.decode_body(c.body).status for n, c in ec.items()}
    assert st["ok:heavy"] == st["ok:heavy_light"] == st["ok:heavy_no_sig"] == mh.W1R_OK
    assert st["mal:heavy_bad_63"] == st["mal:heavy_bad_0_and_63"] == st["mal:heavy_bad_31_and_32"] == mh.W1R_MALFORMED
    assert st["fb:heavy"] == mh.W1R_FALLBACK
    assert st["mal:heavy_fb_and_bad_0"] == mh.W1R_MALFORMED  # MALFORMED wins over FALLBACK
    assert st["mal:level1_one_byte"] == mh.W1R_MALFORMED and st["fb:level1_two_multigrants"] == mh.W1R_FALLBACK
    assert DM.decode_body(DM.SMALL_BAD).status == mh.W1R_MALFORMED
    d = DM.decode_body(ec["ok:heavy"].body)
    assert len(d.grants) == 1 and d.grants[0].flags == mh.W1G_HAS_SIG and len(d.certs) == DM.MAX_ENTRIES
    # what the level-2 grid sees of them: the heavy bodies whatever their status, nothing of the rest
    ne = {n: DM.level2_entries(c.body, c.kind) for n, c in ec.items()}
    assert all(ne[n] == (0 if n.startswith("kind:") or "level1" in n else 6 if n == "ok:heavy_no_sig" else 65) for n in ne)


def test_heavy_bodies_agree_with_google_protobuf():
    pytest.importorskip("google.protobuf")
    last = DM.Case("sig_last", DM.reply(DM.multigrant([(DM.K1, DM.grant(DM.K1, 11))])), (DM.K1,))
    bodies = {c.body for c in tuple(DM.edge_cases().values()) + DM.far_cases() + (last,)}
    for r in (DM.grouping_batch(), DM.cap_batch(4, DM.SMALL_BAD)):
        wire = r.wire.tobytes()
        bodies |= {wire[int(o):int(o) + int(n)] for o, n in zip(r.resp_off, r.resp_len)}
    assert len(bodies) > 40
    for b in sorted(bodies):
        DM.crosscheck(b, DM.decode_body(b))


@pytest.mark.parametrize("layout", ["packed", "shared"])
@pytest.mark.parametrize("P", [4, 12, 300])
def test_level2_pattern_equals_the_model(P, layout):
    cases = (DM.edge_cases()["ok:heavy"],) * 3 + (DM.edge_cases()["mal:heavy_bad_63"],) if P == 4 else DM.pattern_cases(P)
    r = DM.batch(cases, layout=layout, per_req=3)
    got, want = check(r, DM.IDS, f"pattern {P} {layout}")
    st = want["resp_status"].tolist()
    if P == 4:
        assert st == [mh.W1R_OK] * 3 + [mh.W1R_MALFORMED]
    else:
        M, F, K = mh.W1R_MALFORMED, mh.W1R_FALLBACK, mh.W1R_OK
        assert st[:12] == [K, M, K, K, K, K, M, F, M, F, M, K]  # an unparsed kind is OK and keeps its kind
        assert want["resp_kind_out"][:6].tolist() == [mh.W1_REQUEST_FAILED, mh.W1_OTHER, mh.W1_OK, mh.W1_OTHER,
                                                      mh.W1_REQUEST_FAILED, mh.W1_OTHER]
    heavy = sum(c.name.split(":")[1].startswith("heavy") for c in cases)
    assert DM.n_level2_entries(r) == 65 * heavy


def test_cap_batch_equals_the_model_at_a_small_size():
    """The block-cap batch's builder, at a size the model decodes in no time."""
    for last in (DM.SMALL_BAD, DM.heavy(bad=63)):
        r = DM.cap_batch(40, last)
        got, want = check(r, DM.IDS, "cap")
        assert want["resp_status"].tolist() == [mh.W1R_OK] * 39 + [mh.W1R_MALFORMED]
        assert DM.n_level2_entries(r) == 2 * 39 + DM.level2_entries(last)
        assert len(set(r.resp_off.tolist())) == 2 and np.diff(r.req_resp_off.astype(np.int64)).tolist() == [1, 12, 7, 18, 2]


def test_request_grouping_equals_the_model():
    r = DM.grouping_batch()
    got, want = check(r, DM.IDS, "grouping")
    n_resp = np.diff(r.req_resp_off.astype(np.int64)).tolist()
    n_ops = np.diff(r.req_op_off.astype(np.int64)).tolist()
    assert n_resp == [0, 2, 0, 0, 3, 3, 1, 0] and n_ops == [1, 2, 0, 1, 0, 64, 2, 1]
    assert (want["resp_status"] == mh.W1R_OK).all()
    keys = lambda q: [int(k) for p in range(int(r.req_resp_off[q]), int(r.req_resp_off[q + 1]))
                      for k in want["grant_key"][int(want["resp_grant_off"][p]):int(want["resp_grant_off"][p + 1])]]
    assert keys(1) == [0, 0xFF, 0xFF]  # alpha; key-A and key-B are not this request's
    assert keys(4) == [0xFF] * 5  # a request without ops
    assert keys(5) == [0, 63, 0xFF, 63, 0, 63]  # key-A at slots 0 and 7: the first; key-B at the last slot alone
    assert keys(6) == [1]


@pytest.mark.parametrize("lead", [0, 5])
def test_signature_ends_the_wire(lead):
    """No filler after the last body, whose last field is its signature: the last 256 bytes of the wire."""
    by = {c.name: c for c in DM.corpus()}
    last = DM.Case("sig_last", DM.reply(DM.multigrant([(DM.K1, DM.grant(DM.K1, 11))])), (DM.K1,))
    r = DM.batch((by["rep:sigs"], by["mutate:2"], last), per_req=2, lead=lead, tail=0)
    assert int(r.resp_off[-1]) + int(r.resp_len[-1]) == r.wire.size
    got, want = check(r, DM.IDS, "wire end")
    assert want["grant_flags"][-1] == mh.W1G_HAS_SIG
    np.testing.assert_array_equal(want["sig"][-1], r.wire[-256:])
    assert DM.sig_sources(r, want)[-1] == r.wire.size - 256


def test_far_cases_cover_what_the_offset_test_needs():
    cases = DM.far_cases()
    r = DM.batch(cases, per_req=3, mod=16)
    got, want = check(r, DM.IDS, "far")
    assert r.wire.size <= 64 << 10 and {int(o) % 16 for o in r.resp_off} == set(range(16))
    assert {s % 16 for s in DM.sig_sources(r, want)} == set(range(16))
    assert len(cases) == 32 and set(want["resp_status"].tolist()) == {0, 1, 2, 3}
    assert {mh.W1_REQUEST_FAILED, mh.W1_OTHER, mh.W1_REFUSED} <= {c.kind for c in cases}
    assert {int(f) & mh.W1G_HAS_SIG for f in want["grant_flags"]} == {0, mh.W1G_HAS_SIG}
    assert (want["resp_client_len"] > 0).any() and len(want["cert_key_off"]) > 64


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
