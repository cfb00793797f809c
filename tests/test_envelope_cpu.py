"""The envelope codec's host forms against the independent model (envelope_model.py), and
the model against google.protobuf.  No GPU."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import envelope_cases as X
import envelope_model as E
import mochi_hip as mh


def _decode_both(frames, pad=1, fill=0xA5):
    fr = mh.EnvelopeFrames.pack(frames, pad=pad)
    got = mh.envelope_decode(fr, fill=fill)
    want = E.decode(frames, [int(o) for o in fr.frame_off])
    return fr, got, want


def _assert_decoded(got, want, names=None):
    for k in E.DEC_KEYS:
        bad = np.flatnonzero(got[k] != want[k])
        assert bad.size == 0, (k, int(bad[0]), None if names is None else names[int(bad[0])], got[k][bad[0]], want[k][bad[0]])


# ---- conditions on the corpus (model alone) ----------------------------------------------
def test_corpus_is_not_vacuous():
    parsed = [E.parse(c.frame) for c in E.corpus()]
    assert {p.status for p in parsed} == {E.OK, E.MALFORMED, E.FALLBACK}
    assert {p.kind for p in parsed if p.status == E.OK} == set(range(E.KINDS))
    names = [c.name for c in E.corpus()]
    assert len(set(names)) == len(names)
    by = dict(zip(names, parsed))
    # the cases whose verdict the issue spells out
    assert by["group_depth_100"].status == E.OK and by["group_depth_101"].status == E.MALFORMED
    assert by["tag_overlong_field7"].status == E.OK and by["tag_overlong_field7"].msg_id[1] == 2
    assert by["ts_negative_1"].ts == -1 and by["ts_11_bytes"].status == E.MALFORMED
    assert by["payload_overrun_1"].status == E.MALFORMED and by["payload_exact"].status == E.OK
    for n in ("two_payloads_same", "two_payloads_differ", "two_payloads_differ_reversed", "two_payloads_first_malformed",
              "two_payloads_same_first_malformed", "three_payloads"):
        assert by[n].status == E.FALLBACK, n
    for n in ("utf8_overlong_nul", "utf8_surrogate", "utf8_above_max", "utf8_cut_by_slice_end", "field_0_varint", "field_0_ld"):
        assert by[n].status == E.MALFORMED, n
    assert by["empty_payload_kind_7"].kind == 7 and by["empty_payload_kind_7"].body[1] == 0
    assert by["payload_and_varint_payload"].status == E.OK and by["payload_and_varint_payload"].kind == 7
    assert len(E.truncations()) > 100


# ---- model against google.protobuf -----------------------------------------------------------
def test_model_matches_google_protobuf():
    pytest.importorskip("google.protobuf")
    from google.protobuf.message import DecodeError

    PM = E.protocol_message_class()
    compared = 0
    for c in E.corpus():
        if c.java_only:
            continue
        p = E.parse(c.frame)
        m = PM()
        try:
            m.ParseFromString(c.frame)
            threw = False
        except DecodeError:
            threw = True
        if p.status == E.FALLBACK:
            assert not threw, c.name  # the envelope level of a FALLBACK frame parses
            continue
        assert threw == (p.status == E.MALFORMED), c.name
        compared += 1
        if threw:
            continue
        which = m.WhichOneof("payload")
        assert (0 if which is None else 1 + E.PAYLOAD_NAMES.index(which)) == p.kind, c.name
        sl = lambda s: c.frame[s[0]:s[0] + s[1]]
        if which is not None:
            assert getattr(m, which) == sl(p.body), c.name
        assert m.msgTimestamp == p.ts, c.name
        assert (m.serverId.encode(), m.msgId.encode(), m.replyToMsgId.encode()) == (sl(p.server_id), sl(p.msg_id), sl(p.reply_to)), c.name
    assert compared > 1000


# ---- host form against the model ----------------------------------------------------------------
def test_decode_corpus():
    frames = [c.frame for c in E.corpus()]
    fr, got, want = _decode_both(frames)
    _assert_decoded(got, want, [c.name for c in E.corpus()])


SHAPES = [("one_kind", lambda n: E.batch_one_kind(n)), ("mix", lambda n: E.batch_mix(n, seed=n))]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 513])
@pytest.mark.parametrize("shape", [s[0] for s in SHAPES])
def test_decode_and_route_shapes(shape, n):
    frames = dict(SHAPES)[shape](n)
    fr, got, want = _decode_both(frames, pad=3)
    _assert_decoded(got, want)
    _check_route(got, want)


def _check_route(got_dec, want_dec):
    r = mh.envelope_route(got_dec, fill=0xA5)
    kind_off, order, boff, blen = E.route(want_dec)
    assert np.array_equal(r["kind_off"], kind_off)
    P = int(kind_off[-1])
    assert np.array_equal(r["order"][:P], order) and np.array_equal(r["body_off"][:P], boff)
    assert np.array_equal(r["body_len"][:P], blen)
    for k in ("order", "body_off", "body_len"):  # nothing past the routed frames is written
        assert np.all(r[k][P:].view(np.uint8) == 0xA5), k


def test_route_per_kind_and_corpus():
    for frames in (E.batch_per_kind(), [c.frame for c in E.corpus()]):
        fr, got, want = _decode_both(frames)
        _check_route(got, want)
    fr, got, want = _decode_both(E.batch_per_kind())
    assert list(mh.envelope_route(got)["kind_off"]) == list(range(14))


def test_route_ignores_kind_above_12():
    dec = dict(status=np.array([0, 0], np.uint8), kind=np.array([13, 3], np.uint8), body_off=np.array([1, 2], np.uint64),
               body_len=np.array([3, 4], np.uint32))
    r = mh.envelope_route(dec)
    assert int(r["kind_off"][13]) == 1 and int(r["order"][0]) == 1


@pytest.mark.parametrize("name", sorted(X.join_cases()))
def test_join(name):
    ids, frames = X.join_cases()[name]
    fr, got, want = _decode_both(frames, pad=1)
    _assert_decoded(got, want)
    j, P = mh.envelope_join(ids, fr, got, fill=0xA5)
    w = E.join(ids, frames, want)
    assert P == len(w["resp_frame"]) == int(w["req_resp_off"][-1])
    assert np.array_equal(j["frame_req"], w["frame_req"]) and np.array_equal(j["req_resp_off"], w["req_resp_off"])
    for k in ("resp_frame", "resp_off", "resp_len", "resp_w1_kind", "resp_rr_kind"):
        assert np.array_equal(j[k][:P], w[k]), k
        assert np.all(j[k][P:].view(np.uint8) == 0xA5), k


def test_join_kind_maps():
    frames = [E.frame(k, b"", reply_to=b"q") for k in range(1, 13)]
    fr, got, want = _decode_both(frames)
    j, P = mh.envelope_join([b"q"], fr, got)
    assert P == 12
    assert list(j["resp_w1_kind"]) == [mh.W1_OTHER] * 7 + [mh.W1_OK, mh.W1_REFUSED, mh.W1_OTHER, mh.W1_OTHER, mh.W1_REQUEST_FAILED]
    assert list(j["resp_rr_kind"]) == [mh.RR_OTHER] * 5 + [mh.RR_READ] + [mh.RR_OTHER] * 4 + [mh.RR_WRITE2_ANS, mh.RR_OTHER]


# ---- encode ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, mh.ENV_LENGTH_PREFIX])
def test_encode_matches_model_and_round_trips(flags):
    src, msgs = X.encode_source(flags, n_extra=40)
    wire, off, ln, st = mh.envelope_encode(src)
    want, woff, frames = X.expected_wire(msgs, flags)
    assert wire.tobytes() == want
    assert list(off) == woff and list(ln) == [len(f) for f in frames] and not st.any()
    assert E.frame(7) == b"\xDA\x06\x00"
    # decode returns the inputs
    fr = mh.EnvelopeFrames(wire, off, ln)
    d = mh.envelope_decode(fr)
    sl = lambda o, n: wire[int(o):int(o) + int(n)].tobytes()
    for i, m in enumerate(msgs):
        assert d["status"][i] == mh.ENV_OK and d["kind"][i] == m["kind"] and d["msg_timestamp"][i] == m["ts"]
        assert sl(d["body_off"][i], d["body_len"][i]) == (m["body"] if m["kind"] else b"")
        assert sl(d["msg_id_off"][i], d["msg_id_len"][i]) == m["msg_id"]
        assert sl(d["reply_to_off"][i], d["reply_to_len"][i]) == m["reply_to"]
        assert sl(d["server_id_off"][i], d["server_id_len"][i]) == m["server_id"]


def test_encoded_frames_parse_with_google_protobuf():
    pytest.importorskip("google.protobuf")
    PM = E.protocol_message_class()
    src, msgs = X.encode_source(0, n_extra=10)
    wire, off, ln, st = mh.envelope_encode(src)
    for i, m in enumerate(msgs):
        b = wire[int(off[i]):int(off[i]) + int(ln[i])].tobytes()
        pm = PM()
        pm.ParseFromString(b)
        assert pm.SerializeToString() == b  # the canonical form
        which = pm.WhichOneof("payload")
        assert (0 if which is None else 1 + E.PAYLOAD_NAMES.index(which)) == m["kind"]
        if which:
            assert getattr(pm, which) == m["body"]
        assert (pm.msgTimestamp, pm.serverId.encode(), pm.msgId.encode(), pm.replyToMsgId.encode()) == \
            (m["ts"], m["server_id"], m["msg_id"], m["reply_to"])


def test_encode_capacity_rule():
    src, msgs = X.encode_source(mh.ENV_LENGTH_PREFIX)
    rc, need, off, ln, st = mh.envelope_encode_into(src, None)
    assert rc == mh.EINVAL and need == len(X.expected_wire(msgs, mh.ENV_LENGTH_PREFIX)[0])
    buf = np.full(need - 1, 0xA5, np.uint8)
    rc, need2, off, ln, st = mh.envelope_encode_into(src, buf)
    assert rc == mh.EINVAL and need2 == need and np.all(buf == 0xA5)
    assert "wire_cap is smaller" in mh._err(mh.load_library())
    assert mh.envelope_encode_bound(src.n_msgs, src.bodies.size, src.ids.size) >= need


# ---- argument errors ------------------------------------------------------------------------------
def _expect(rc, text):
    assert rc == mh.EINVAL
    assert text in mh._err(mh.load_library()), mh._err(mh.load_library())


def test_decode_argument_errors():
    lib = mh.load_library()
    fr = mh.EnvelopeFrames.pack([b"\x28\x01", b"\x28\x02"])
    f, keep = fr.to_c()
    o = mh.EnvelopeDecoded_C()
    _expect(lib.mochi_envelope_decode(None, ctypes.addressof(o)), "null argument")
    _expect(lib.mochi_envelope_decode(ctypes.addressof(f), None), "null argument")
    _expect(lib.mochi_envelope_decode(ctypes.addressof(f), ctypes.addressof(o)), "every output array is required")
    big = mh.EnvelopeFrames_C()
    big.n_frames = (1 << 24) + 1
    _expect(lib.mochi_envelope_decode(ctypes.addressof(big), ctypes.addressof(o)), "more than 2^24 frames")
    f.frame_off = None
    _expect(lib.mochi_envelope_decode(ctypes.addressof(f), ctypes.addressof(o)), "wire / frame_off / frame_len required")
    for off, ln in ((5, 0), (3, 2), (1 << 40, 0)):
        bad = mh.EnvelopeFrames(fr.wire, np.array([0, off], np.uint64), np.array([2, ln], np.uint32))
        with pytest.raises(mh.MochiError, match="a frame slice lies outside wire"):
            mh.envelope_decode(bad)
    assert mh.envelope_decode(mh.EnvelopeFrames(fr.wire, np.array([4], np.uint64), np.array([0], np.uint32)))["status"][0] == mh.ENV_OK
    empty = mh.EnvelopeFrames_C()
    assert lib.mochi_envelope_decode(ctypes.addressof(empty), ctypes.addressof(o)) == mh.OK


def test_route_argument_errors():
    lib = mh.load_library()
    a = np.zeros(4, np.uint64)
    o = mh.EnvelopeRouted_C()
    _expect(lib.mochi_envelope_route(0, None, None, None, None, None), "kind_off required")
    _expect(lib.mochi_envelope_route(0, None, None, None, None, ctypes.addressof(o)), "kind_off required")
    o.kind_off = a.ctypes.data
    _expect(lib.mochi_envelope_route((1 << 24) + 1, None, None, None, None, ctypes.addressof(o)), "more than 2^24 frames")
    _expect(lib.mochi_envelope_route(1, None, None, None, None, ctypes.addressof(o)), "status / kind / body_off / body_len required")
    p = a.ctypes.data
    _expect(lib.mochi_envelope_route(1, p, p, p, p, ctypes.addressof(o)), "every output array is required")
    ko = np.full(14, 7, np.uint32)
    o.kind_off = ko.ctypes.data
    assert lib.mochi_envelope_route(0, None, None, None, None, ctypes.addressof(o)) == mh.OK and not ko.any()


def test_join_argument_errors():
    lib = mh.load_library()
    fr = mh.EnvelopeFrames.pack([E.frame(8, b"b", reply_to=b"id")])
    dec = mh.envelope_decode(fr)
    P = ctypes.c_uint32(9)
    r, keep_r = mh._env_requests_c([b"id"])
    f, keep_f = fr.to_c()
    d, o = mh.EnvelopeDecoded_C(), mh.EnvelopeJoined_C()
    pa = lambda *x: [None if v is None else ctypes.addressof(v) for v in x]
    _expect(lib.mochi_envelope_join(*pa(r, f, d, o), None), "n_resps required")
    _expect(lib.mochi_envelope_join(*pa(None, f, d, o), ctypes.addressof(P)), "null argument")
    assert P.value == 0
    _expect(lib.mochi_envelope_join(*pa(r, None, d, o), ctypes.addressof(P)), "null argument")
    _expect(lib.mochi_envelope_join(*pa(r, f, d, o), ctypes.addressof(P)), "req_resp_off required")
    rro = np.zeros(2, np.uint32)
    o.req_resp_off = rro.ctypes.data
    _expect(lib.mochi_envelope_join(*pa(r, f, d, o), ctypes.addressof(P)), "reply_to_off / reply_to_len required")
    ins = {k: np.ascontiguousarray(dec[k]) for k in dec}
    for k, a in ins.items():
        setattr(d, k, a.ctypes.data)
    _expect(lib.mochi_envelope_join(*pa(r, f, d, o), ctypes.addressof(P)), "every output array is required")
    r2, keep2 = mh._env_requests_c([b"id"])
    r2.n_reqs = (1 << 24) + 1
    _expect(lib.mochi_envelope_join(*pa(r2, f, d, o), ctypes.addressof(P)), "more than 2^24 requests")
    r2.n_reqs, r2.id_off = 1, None
    _expect(lib.mochi_envelope_join(*pa(r2, f, d, o), ctypes.addressof(P)), "ids / id_off / id_len required")
    # slices outside their blobs
    bad = dict(dec, reply_to_off=np.array([fr.wire.size], np.uint64))
    with pytest.raises(mh.MochiError, match="a replyToMsgId lies outside wire"):
        mh.envelope_join([b"id"], fr, bad)
    r3, keep3 = mh._env_requests_c([b"id"])
    r3.ids_len = 1
    out = {k: np.zeros(4, dt) for k, (dt, w) in mh._ENV_JOINED.items()}
    for k, a in out.items():
        setattr(o, k, a.ctypes.data)
    _expect(lib.mochi_envelope_join(*pa(r3, f, d, o), ctypes.addressof(P)), "a request id lies outside ids")


def test_encode_argument_errors():
    lib = mh.load_library()
    src, msgs = X.encode_source()
    need = ctypes.c_uint64(5)
    s, keep = src.to_c()
    M = src.n_msgs
    off, ln, st = np.zeros(M, np.uint64), np.zeros(M, np.uint32), np.zeros(M, np.uint8)
    call = lambda s_, wire=None, cap=0, o=off, wl=need: lib.mochi_envelope_encode(
        None if s_ is None else ctypes.addressof(s_), wire, cap, None if o is None else o.ctypes.data, ln.ctypes.data, st.ctypes.data,
        None if wl is None else ctypes.addressof(wl))
    _expect(call(s, wl=None), "wire_len required")
    _expect(call(None), "null argument")
    assert need.value == 0
    _expect(call(s, o=None), "msg_off / msg_len / status required")
    _expect(call(s, cap=10), "wire_out required")
    s.flags = 2
    _expect(call(s), "unknown flags")
    s.flags = 0
    for a, b, text in (("msg_id_off", "msg_id_len", "msg_id_off and msg_id_len go together"),
                       ("reply_to_len", "reply_to_off", "reply_to_off and reply_to_len go together"),
                       ("server_id_off", "server_id_len", "server_id_off and server_id_len go together")):
        keep_ptr = getattr(s, a)
        setattr(s, a, None)
        _expect(call(s), text)
        setattr(s, a, keep_ptr)
    keep_ptr, s.ids = s.ids, None
    _expect(call(s), "ids required")
    s.ids = keep_ptr
    keep_ptr, s.bodies = s.bodies, None
    _expect(call(s), "bodies required")
    s.bodies = keep_ptr
    s.n_msgs = 0xFFFFFFFF
    _expect(call(s), "batch too large")

    def broken(**kw):
        b, _ = X.encode_source()
        for k, v in kw.items():
            a = np.array(getattr(b, k)).copy()
            a[v[0]] = v[1]
            setattr(b, k, a)
        return b

    for kw, text in ((dict(kind=(0, 13)), "a kind is above 12"), (dict(body_off=(1, 1 << 40)), "a body slice lies outside bodies"),
                     (dict(msg_id_len=(0, 1 << 30)), "a msgId lies outside ids"),
                     (dict(reply_to_off=(1, 1 << 40)), "a replyToMsgId lies outside ids"),
                     (dict(server_id_len=(2, 1 << 30)), "a serverId lies outside ids")):
        with pytest.raises(mh.MochiError, match=text):
            mh.envelope_encode_into(broken(**kw), None)
    for badid in (b"\xC0\x80", b"\xED\xA0\x80", b"\xF4\x90\x80\x80", b"ab\xC3"):
        b = mh.EnvelopeSource(bodies=np.zeros(1, np.uint8), ids=np.frombuffer(badid + b"\xA9", np.uint8), kind=np.array([0], np.uint8),
                              body_off=np.zeros(1, np.uint64), body_len=np.zeros(1, np.uint32), msg_timestamp=np.zeros(1, np.int64),
                              reply_to_off=np.zeros(1, np.uint64), reply_to_len=np.array([len(badid)], np.uint32))
        with pytest.raises(mh.MochiError, match="an id is not UTF-8"):
            mh.envelope_encode_into(b, None)
    # kind 0 does not look at its body slice; no message needs no pointer
    ok = broken(body_off=(len(X.BODY_LENS), 1 << 40))
    assert mh.envelope_encode_into(ok, None)[0] == mh.EINVAL  # the capacity alone
    e = mh.EnvelopeSource_C()
    assert lib.mochi_envelope_encode(ctypes.addressof(e), None, 0, None, None, None, ctypes.addressof(need)) == mh.OK
