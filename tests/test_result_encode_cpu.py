"""Answer encoder, host form (mochi_result_reply_encode): the plain-Python model
(result_encode_model) agrees with google.protobuf's serializer and with the decoder's model
on every case; the host form equals the model byte for byte, with offsets, lengths and
statuses, on the named cases in dense, aliased and guarded layouts; every body is read back
by mochi_result_reply_decode with equal values; the decoder's corpus re-encodes to the
canonical form; argument errors, the capacity rule and TOO_LONG."""
import ctypes

import numpy as np
import pytest

import mochi_hip as mh
import result_encode_model as E
import result_reply_model as RRM

NAMES = sorted(E.cases())


def encode_checked(ra, answers, what=""):
    """The host form over `ra` into an exactly sized buffer: equal to the model's arrays."""
    wire, off, ln, st = mh.result_reply_encode(ra)
    w_wire, w_off, w_ln, w_st = E.expected_arrays(answers)
    np.testing.assert_array_equal(st, w_st, err_msg=what + " status")
    np.testing.assert_array_equal(ln, w_ln, err_msg=what + " msg_len")
    np.testing.assert_array_equal(off, w_off, err_msg=what + " msg_off")
    assert wire.tobytes() == w_wire.tobytes(), what
    return wire, off, ln, st


# 1. the model ----------------------------------------------------------------------------
def test_model_agrees_with_google_protobuf():
    pytest.importorskip("google.protobuf")
    n = 0
    for a in E.all_answers():
        if a.kind == E.OTHER or any(o.status == 0xFF for o in a.ops):
            continue
        if any(o.cert is not None and len(o.cert) == 1 for o in a.ops):
            continue  # a lone tag is no WriteCertificate: the classes cannot hold it
        want = E.protobuf_bytes(a)
        # the runtime re-serializes the certificate it parsed: equal for the canonical ones used here
        assert E.message(a) == want, a
        n += 1
    assert n >= 50


def test_model_agrees_with_the_decoder_model():
    """Every body the model writes reads back through result_reply_model.decode_body, value for value."""
    for a in E.all_answers():
        bodies, st = E.expected([a])
        if a.kind == E.OTHER or st[0] != mh.ENC_OK:
            continue
        b = bodies[0]
        d = RRM.decode_body(b, a.kind, len(a.ops))
        if any(o.cert is not None and len(o.cert) == 1 for o in a.ops):
            assert d.status == mh.RRS_MALFORMED
            continue
        assert d.status == mh.RRS_OK and d.n_ops == len(a.ops)
        sl = lambda s: b[s[0]:s[0] + s[1]] if s else b""
        assert sl(d.rid) == a.rid and sl(d.nonce) == (a.nonce if a.kind == E.RD else b"")
        for o, v in zip(a.ops, d.ops):
            assert (v.status, v.existed, v.n_cert, sl(v.result)) == (o.status, o.existed, int(o.cert is not None), o.result)
            assert sl(v.cert) == (o.cert or b"")


def test_sizes_without_building_equal_the_built_ones():
    for a in E.all_answers():
        if a.kind != E.OTHER:
            assert E._size(a) == len(E.message(a))


# 2. host form == model ----------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_named_case(name):
    answers = E.cases()[name]
    encode_checked(E.layout(answers), answers, name)


@pytest.mark.parametrize("alias,slots", [(True, "dense"), (False, "guarded"), (True, "guarded")])
def test_all_cases_in_one_batch(alias, slots):
    answers = E.all_answers()
    ra = E.layout(answers, alias=alias, slots=slots)
    if slots == "guarded":
        assert (np.diff(ra.slot_off.astype(np.int64)) < 0).all() and ra.n_slots > ra.n_ops
    if alias:
        assert len(set(ra.op_cert_off[ra.op_cert_len > 0].tolist())) < int((ra.op_cert_len > 0).sum())
    encode_checked(ra, answers)


def test_wire_bytes_of_the_small_shapes():
    """The framing spelled out: 0A 00 for no operations, an empty operation, 12 00 for the default
    certificate, a two-byte status."""
    body = lambda a: mh.result_reply_encode(E.layout([a]))[0].tobytes()
    assert body(E.Ans(E.W2)) == b"\x0a\x00"
    assert body(E.Ans(E.RD, (), b"r", b"n")) == b"\x0a\x00\x12\x01n\x1a\x01r"
    assert body(E.Ans(E.W2, (E.OpR(),), b"r")) == b"\x0a\x02\x0a\x00\x12\x01r"
    assert body(E.Ans(E.W2, (E.OpR(0, b"", True, b""),))) == b"\x0a\x06\x0a\x04\x12\x00\x18\x01"
    assert body(E.Ans(E.W2, (E.OpR(1),))) == b"\x0a\x04\x0a\x02\x20\x01"
    assert body(E.Ans(E.W2, (E.OpR(254),))) == b"\x0a\x05\x0a\x03\x20\xfe\x01"
    assert body(E.Ans(E.W2, (E.OpR(), ), b"", b"ignored")) == b"\x0a\x02\x0a\x00"


def test_no_ids_arrays():
    answers = (E.Ans(E.W2, (E.OpR(0, b"v", True, E.CERT),)), E.Ans(E.RD, (E.OpR(1),)))
    ra = E.layout(answers, ids=False)
    assert ra.rid_off is None and ra.nonce_off is None
    encode_checked(ra, answers)


def test_empty_batch_needs_no_pointer():
    lib = mh.load_library()
    a = mh.ResultAnswers_C()
    need = ctypes.c_uint64(7)
    assert lib.mochi_result_reply_encode(ctypes.addressof(a), None, 0, None, None, None, ctypes.addressof(need)) == mh.OK
    assert need.value == 0
    wire, off, ln, st = mh.result_reply_encode(E.layout([]))
    assert wire.size == off.size == ln.size == st.size == 0


# 3. round trip ------------------------------------------------------------------------------
def _decode(wire, off, ln, kinds, n_ops):
    P = len(kinds)
    k = np.asarray(n_ops, np.int64)
    r = mh.ResultReplies(wire=wire, resp_off=off, resp_len=ln, resp_kind=np.asarray(kinds, np.uint8),
                         req_resp_off=np.arange(P + 1, dtype=np.uint32), n_ops=k.astype(np.uint32),
                         slot_off=np.concatenate([[0], np.cumsum(k)[:-1]]).astype(np.uint64))
    return r, mh.result_reply_decode(r)


def test_every_body_reads_back():
    answers = [a for a in E.all_answers() if a.kind != E.OTHER and all(o.status != 0xFF for o in a.ops)]
    wire, off, ln, st = encode_checked(E.layout(answers, alias=True), answers)
    r, d = _decode(wire, off, ln, [a.kind for a in answers], [len(a.ops) for a in answers])
    RRM.assert_equal(d, RRM.decode(r, fill=0))
    w = wire.tobytes()
    sl = lambda o, n: w[int(o):int(o) + int(n)]
    for p, a in enumerate(answers):
        lone_tag = any(o.cert is not None and len(o.cert) == 1 for o in a.ops)
        assert d["resp_status"][p] == (mh.RRS_MALFORMED if lone_tag else mh.RRS_OK)
        if lone_tag:
            continue
        assert d["resp_n_ops"][p] == len(a.ops)
        assert sl(d["resp_rid_off"][p], d["resp_rid_len"][p]) == a.rid
        assert sl(d["resp_nonce_off"][p], d["resp_nonce_len"][p]) == (a.nonce if a.kind == E.RD else b"")
        for j, o in enumerate(a.ops):
            s = int(r.slot_off[p]) + j
            assert (d["op_status"][s], d["op_existed"][s], d["op_flags"][s]) == (o.status, int(o.existed), int(o.cert is not None))
            assert sl(d["op_result_off"][s], d["op_result_len"][s]) == o.result
            assert sl(d["op_cert_off"][s], d["op_cert_len"][s]) == (o.cert or b"")


def test_decoded_corpus_re_encodes_to_the_canonical_form():
    """decode -> encode over every OK body of the decoder's corpus whose count is its request's:
    the decoder's outputs are the encoder's inputs as they are (offsets into the received
    bytes), and the bytes are the model's for the decoded values."""
    cases = [c for c in RRM.own_cases() + RRM.corpus() if c.kind != RRM.OTHER]
    r = RRM.batch(cases)
    d = mh.result_reply_decode(r)
    keep = [p for p, c in enumerate(cases)
            if d["resp_status"][p] == mh.RRS_OK and d["resp_n_ops"][p] == c.n_ops and
            all(d["op_status"][int(r.slot_off[p]) + j] != 0xFF for j in range(c.n_ops))]
    assert len(keep) > 300
    take = lambda k: np.ascontiguousarray(d[k][keep])
    ra = mh.ResultAnswers(wire=r.wire, store=np.zeros(0, np.uint8), ids=r.wire, resp_kind=r.resp_kind[keep],
                          resp_n_ops=take("resp_n_ops"), slot_off=r.slot_off[keep], rid_off=take("resp_rid_off"),
                          rid_len=take("resp_rid_len"), nonce_off=take("resp_nonce_off"), nonce_len=take("resp_nonce_len"),
                          **{k: d[k] for k in mh._RA_SLOT})
    w = r.wire.tobytes()
    sl = lambda o, n: w[int(o):int(o) + int(n)]
    answers = []
    for p in keep:
        s0 = int(r.slot_off[p])
        ops = tuple(E.OpR(int(d["op_status"][s]), sl(d["op_result_off"][s], d["op_result_len"][s]), bool(d["op_existed"][s]),
                          sl(d["op_cert_off"][s], d["op_cert_len"][s]) if d["op_flags"][s] & mh.RRO_HAS_CERT else None)
                    for s in range(s0, s0 + cases[p].n_ops))
        answers.append(E.Ans(cases[p].kind, ops, sl(d["resp_rid_off"][p], d["resp_rid_len"][p]),
                             sl(d["resp_nonce_off"][p], d["resp_nonce_len"][p])))
    wire, off, ln, st = encode_checked(ra, answers)
    assert (st == mh.ENC_OK).all()
    # and the canonical bytes decode to the same values again
    r2, d2 = _decode(wire, off, ln, [a.kind for a in answers], [len(a.ops) for a in answers])
    assert (d2["resp_status"] == mh.RRS_OK).all()
    np.testing.assert_array_equal(d2["resp_n_ops"], take("resp_n_ops"))


# 4. errors, capacity, TOO_LONG -----------------------------------------------------------------
def _rc(ra, cap=None):
    lib = mh.load_library()
    a, keep = ra.to_c()
    P = ra.n_resps
    off, ln, st = np.zeros(max(P, 1), np.uint64), np.zeros(max(P, 1), np.uint32), np.zeros(max(P, 1), np.uint8)
    wire = np.zeros(1 << 16 if cap is None else max(cap, 1), np.uint8)
    need = ctypes.c_uint64(0)
    rc = lib.mochi_result_reply_encode(ctypes.addressof(a), mh._ptr(wire), wire.size if cap is None else cap, mh._ptr(off),
                                       mh._ptr(ln), mh._ptr(st), ctypes.addressof(need))
    return rc, mh._err(lib), a, keep


def _base():
    return E.layout(E.cases()["other_between"])


@pytest.mark.parametrize("field,value,text", [
    ("op_result_off", 1 << 40, "result slice"),
    ("op_result_len", 1 << 30, "result slice"),
    ("op_cert_off", 1 << 40, "certificate slice"),
    ("op_cert_len", 1 << 30, "certificate slice"),
    ("rid_len", 1 << 20, "rid"),
    ("rid_off", 1 << 40, "rid"),
    ("resp_n_ops", 65, "MOCHI_MAX_OPS_PER_CERT"),
    ("resp_kind", 3, "MOCHI_RR_"),
    ("slot_off", 1 << 33, "slot run"),
])
def test_einval_for_an_inconsistent_input(field, value, text):
    ra = _base()
    a = np.array(getattr(ra, field)).copy()
    a[0] = value
    setattr(ra, field, a)
    rc, err, _, _ = _rc(ra)
    assert rc == mh.EINVAL and text in err, err


def test_einval_for_a_nonce_outside_ids_and_store_slices():
    ra = _base()
    ra.nonce_len = ra.nonce_len.copy()
    ra.nonce_len[2] = 1 << 20  # the READ answer's; a Write2 answer's nonce is never read
    rc, err, _, _ = _rc(ra)
    assert rc == mh.EINVAL and "nonce" in err
    ra = _base()
    ra.nonce_len = ra.nonce_len.copy()
    ra.nonce_len[0] = 1 << 20
    assert _rc(ra)[0] == mh.OK
    # the same offset is inside `wire` and outside the (shorter) `store`
    ra = _base()
    ra.store = ra.store[:2]
    ra.op_flags = ra.op_flags.copy()
    ra.op_flags[0] |= mh.RAO_CERT_STORE
    rc, err, _, _ = _rc(ra)
    assert rc == mh.EINVAL and "certificate slice" in err


@pytest.mark.parametrize("field", ["resp_kind", "resp_n_ops", "slot_off", "op_status", "op_flags", "op_cert_len", "rid_len",
                                   "nonce_off", "wire"])
def test_einval_for_a_null_array(field):
    lib = mh.load_library()
    ra = _base()
    a, keep = ra.to_c()
    setattr(a, field, None)
    off, ln, st = np.zeros(4, np.uint64), np.zeros(4, np.uint32), np.zeros(4, np.uint8)
    wire = np.zeros(1 << 16, np.uint8)
    need = ctypes.c_uint64(0)
    rc = lib.mochi_result_reply_encode(ctypes.addressof(a), mh._ptr(wire), wire.size, mh._ptr(off), mh._ptr(ln), mh._ptr(st),
                                       ctypes.addressof(need))
    assert rc == mh.EINVAL
    for i in range(3):  # the outputs and wire_len
        args = [mh._ptr(off), mh._ptr(ln), mh._ptr(st)]
        args[i] = None
        b, keep = ra.to_c()
        assert lib.mochi_result_reply_encode(ctypes.addressof(b), mh._ptr(wire), wire.size, *args, ctypes.addressof(need)) == mh.EINVAL
    b, keep = ra.to_c()
    assert lib.mochi_result_reply_encode(ctypes.addressof(b), mh._ptr(wire), wire.size, mh._ptr(off), mh._ptr(ln), mh._ptr(st),
                                         None) == mh.EINVAL


def test_capacity_rule_writes_no_byte():
    answers = E.all_answers()
    ra = E.layout(answers)
    w_wire, w_off, w_ln, w_st = E.expected_arrays(answers)
    for cap in (0, 1, w_wire.size - 1):
        buf = np.full(w_wire.size + 8, E.FILL, np.uint8)
        rc, need, off, ln, st = mh.result_reply_encode_into(ra, buf[:cap] if cap else None)
        assert rc == mh.EINVAL and need == w_wire.size
        assert (buf == E.FILL).all()
        np.testing.assert_array_equal(ln, w_ln)
    buf = np.full(w_wire.size + 8, E.FILL, np.uint8)
    rc, need, off, ln, st = mh.result_reply_encode_into(ra, buf[:w_wire.size])
    assert rc == mh.OK and buf[:need].tobytes() == w_wire.tobytes() and (buf[need:] == E.FILL).all()
    assert mh.result_reply_encode_bound(ra) >= need


def test_too_long_by_aliasing_one_large_slice():
    """64 operations that all point at one certificate of 2^25 bytes: 2^31 and a few bytes."""
    big = bytes(1 << 25)
    long_ = E.Ans(E.RD, tuple(E.OpR(0, b"", True, big) for _ in range(64)), b"r", b"n")
    short = E.Ans(E.RD, long_.ops[:63], b"r", b"n")
    small = E.Ans(E.W2, (E.OpR(1),), b"rid")
    answers = (small, long_, small)
    ra = E.layout(answers, alias=True)
    assert ra.wire.size < (1 << 25) + 64
    rc, need, off, ln, st = mh.result_reply_encode_into(ra, None)
    assert st.tolist() == [mh.ENC_OK, mh.ENC_TOO_LONG, mh.ENC_OK] and ln[1] == 0 and off[2] == off[1] == ln[0]
    np.testing.assert_array_equal(st, E.expected(answers)[1])
    # one operation fewer fits: the size alone, from both sides
    rc, need, off, ln, st = mh.result_reply_encode_into(E.layout((short,), alias=True), None)
    assert st.tolist() == [mh.ENC_OK] and int(ln[0]) == need == E._size(short) < 2 ** 31
