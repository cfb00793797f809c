"""Read request decoder and read answer plan, host forms (mochi_read_request_decode,
mochi_read_answer_plan): the plain-Python model (read_request_model) agrees with
google.protobuf on every case and every mutation (named departures of the Python runtime
apart); the host decoder equals the model array for array in dense and in aliased
layouts; the capacity rule; argument errors; the key numbering at its edges; the host plan
equals the model on every rule; plan -> result_reply_encode gives the bytes of
result_encode_model.message, which google.protobuf parses as a ReadFromServer with the
request's nonce and result_reply_decode turns back into the slots; and a round of 300
random requests against a dict store equals cluster_harness.Server.read."""
import ctypes

import numpy as np
import pytest

import cluster_harness as H
import mochi_hip as mh
import read_request_model as RQ
import result_encode_model as E

FILL = 0xA5


def check(reqs):
    want = RQ.decode(reqs)
    got = mh.read_request_decode(reqs)
    assert got.rc == mh.OK and got.n_ops == len(want["op_obj"]) and got.n_keys == len(want["key_op"])
    RQ.assert_equal(got.trimmed(), want)
    assert mh.read_request_decode_bound(np.asarray(reqs.wire).size, reqs.n_reqs) >= got.n_ops
    return got


def one(body):
    return {k: v.tolist() for k, v in check(RQ.batch([body])).trimmed().items()}


# 1. the model against google.protobuf ------------------------------------------------
def test_model_agrees_with_google_protobuf():
    pytest.importorskip("google.protobuf")
    cases = RQ.own_cases() + RQ.mutations()
    assert set(RQ.PYTHON_DEPARTS) <= {c.name for c in cases}
    for c in cases:
        RQ.crosscheck(c.body, RQ.decode_body(c.body), RQ.PYTHON_DEPARTS.get(c.name, (None,))[0])


def test_what_the_cases_cover():
    st = {c.name: RQ.decode_body(c.body) for c in RQ.own_cases()}
    ok, mal, fb = mh.RDQ_OK, mh.RDQ_MALFORMED, mh.RDQ_FALLBACK
    assert st["empty"] == RQ.Body(ok) and st["only:nonce"].nonce[1] == len(RQ.NONCE) and not st["only:nonce"].ops
    acts = ("absent", "explicit_0", "10_bytes_low_0", "1", "2", "7")
    assert [st["action:" + n].ops[0][0] for n in acts] == [0, 0, 0, 1, 2, 7]
    assert [a for a, *_ in st["action:last_wins"].ops] == [0, 1]
    body = {c.name: c.body for c in RQ.own_cases()}
    sl = lambda n, s: body[n][s[0]:s[0] + s[1]]
    assert sl("nonce:twice", st["nonce:twice"].nonce) == b"second" and sl("client:twice", st["client:twice"].client) == b"second"
    assert st["field3:varint"].status == ok and st["field3:varint"].nonce == (0, 0)
    assert sl("field3:varint_then_nonce", st["field3:varint_then_nonce"].nonce) == RQ.NONCE
    assert st["field4:string"].status == st["field4:varint"].status == st["foreign:top"].status == ok  # bad UTF-8 there: unknown
    assert [st["tx:" + n].status for n in ("twice", "twice_second_bad")] == [fb, mal]
    assert [st["ops:" + n].status for n in ("64", "65", "65_one_bad")] == [ok, fb, mal]
    assert len(st["ops:64"].ops) == 64
    for where in ("top", "op"):
        assert [st["group:%s_%d" % (where, d)].status for d in (100, 101)] == [ok, mal]
    utf8 = [n for n in st if n.startswith("utf8:")]
    assert len(utf8) == 6 and all(st[n].status == mal for n in utf8)
    assert [st[n].status for n in ("field:0", "varint:11_bytes", "len:past_end", "len:past_end_in_tx")] == [mal] * 4
    assert all(RQ.decode_body(b).status == ok for b in RQ.mutation_bodies())
    stm = [RQ.decode_body(c.body).status for c in RQ.mutations()]
    assert stm.count(ok) > 200 and stm.count(mal) > 200


# 2. the host form against the model ---------------------------------------------------
@pytest.mark.parametrize("layout", ["dense", "aliased"])
@pytest.mark.parametrize("which", ["own", "mutations"])
def test_host_form_equals_the_model(which, layout):
    cases = RQ.own_cases() if which == "own" else RQ.mutations()
    got = check(RQ.batch([c.body for c in cases], layout))
    assert set(got.arrays["req_status"].tolist()) >= {0, 1} and (which != "own" or 2 in got.arrays["req_status"])


def test_each_own_case_alone():
    for c in RQ.own_cases():
        check(RQ.batch([c.body], lead=len(c.name) % 5))


def test_values():
    r = one(RQ.read(b"client-1", RQ.transaction([RQ.operation(RQ.READ, b"k1"), RQ.operation(RQ.WRITE, b"k1", b"v"),
                                                 RQ.operation(RQ.READ, b"k2"), RQ.operation(7, b"k2")]), b"nn"))
    assert r["req_status"] == [0] and r["req_nonce_len"] == [2] and r["req_client_len"] == [8]
    assert r["op_flags"] == [mh.RDOP_READ, 0, mh.RDOP_READ, 0] and r["op_obj"] == [0, mh.W1_NONE, 1, mh.W1_NONE]
    assert r["key_op"] == [0, 2] and r["op_key_len"] == [2, 2, 2, 2] and r["req_op_off"] == [0, 4]
    # absent fields: the request's own offset, length 0
    r = one(RQ.read(tx=RQ.transaction([b"\x08\x00"])))
    assert r["req_nonce_off"] == r["req_client_off"] == r["op_key_off"] == [3] and r["op_key_len"] == [0]
    assert r["op_flags"] == [mh.RDOP_READ] and r["op_obj"] == [mh.W1_NONE] and r["key_op"] == []
    # not decoded: nothing but the status
    r = one(b"\x0a\x05abc")
    assert r["req_status"] == [mh.RDQ_MALFORMED] and r["req_op_off"] == [0, 0]
    assert r["req_nonce_off"] == r["req_nonce_len"] == r["req_client_off"] == r["req_client_len"] == [0]


def test_empty_batch():
    got = check(mh.ReadRequests(wire=np.zeros(0, np.uint8), msg_off=np.zeros(0, np.uint64), msg_len=np.zeros(0, np.uint32)))
    assert got.n_ops == 0 and got.arrays["req_op_off"].tolist() == [0]


# 3. capacity, argument errors ------------------------------------------------------------
def test_capacity_one_short_touches_nothing():
    r = RQ.batch([c.body for c in RQ.own_cases()])
    full = mh.read_request_decode(r)
    got = mh.read_request_decode_into(r, full.n_ops - 1, fill=FILL)
    assert got.rc == mh.EINVAL and got.n_ops == full.n_ops
    for k, (dt, w) in mh._RDQ_OUT.items():
        if w in ("O", "K"):
            assert (got.arrays[k].view(np.uint8) == FILL).all(), k
        else:
            np.testing.assert_array_equal(got.arrays[k], full.arrays[k])
    exact = mh.read_request_decode_into(r, full.n_ops, fill=FILL)
    assert exact.rc == mh.OK and (exact.arrays["key_op"][exact.n_keys:].view(np.uint8) == FILL).all()
    RQ.assert_equal(exact.trimmed(), full.trimmed())


def test_decode_argument_errors():
    body = {c.name: c.body for c in RQ.own_cases()}["full"]
    r = RQ.batch([body, body], lead=0)
    end = r.wire.size
    for off, ln in (([0, end - len(body) + 1], [len(body)] * 2), ([0, end + 1], [len(body), 0]), ([0, 0], [len(body), end + 1])):
        bad = mh.ReadRequests(wire=r.wire, msg_off=np.array(off, np.uint64), msg_len=np.array(ln, np.uint32))
        with pytest.raises(mh.MochiError, match="outside wire"):
            mh.read_request_decode(bad)
    lib = mh.load_library()
    c, keep = r.to_c()
    out = mh.read_request_decode_into(r, 8)
    o = mh.ReadRequestsDecoded_C()
    for k, a in out.arrays.items():
        setattr(o, k, a.ctypes.data)
    o.op_cap = 8
    for n, rc in (((1 << 24) + 1, mh.EINVAL), (2, mh.OK)):
        c.n_reqs = n
        assert lib.mochi_read_request_decode(ctypes.addressof(c), ctypes.addressof(o)) == rc
    o.op_key_len = None  # a NULL per-op array with op_cap > 0
    assert lib.mochi_read_request_decode(ctypes.addressof(c), ctypes.addressof(o)) == mh.EINVAL
    o.op_key_len, o.req_nonce_off = out.arrays["op_key_len"].ctypes.data, None
    assert lib.mochi_read_request_decode(ctypes.addressof(c), ctypes.addressof(o)) == mh.EINVAL


# 4. the key numbering -------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RQ.dedup_batches()))
def test_key_numbering(name):
    got = check(RQ.batch(RQ.dedup_batches()[name])).trimmed()
    obj, key_op, NONE = got["op_obj"].tolist(), got["key_op"].tolist(), mh.W1_NONE
    if name == "one_key":
        assert obj == [0] * 80 and key_op == [0]
    elif name == "last_byte":
        assert len(key_op) == 26 and obj[:4] == [0, 1, 2, 1]
    elif name == "read_and_non_read":  # the WRITE and the unknown action on "k" do not number it
        assert obj == [NONE, NONE, 0, 1, NONE] and key_op == [2, 3]
    elif name == "empty_key":
        assert obj == [NONE, 0, NONE, 0] and key_op == [1]
    else:  # the malformed request's ops are gone: `shared` is numbered from the second request
        assert got["req_status"].tolist() == [1, 0] and obj == [0, 1] and key_op == [0, 1]


# 5. the plan --------------------------------------------------------------------------------
def _plan(reqs, lookup=RQ.store_lookup, fill=FILL):
    dec = mh.read_request_decode(reqs)
    t = dec.trimmed()
    ks = RQ.key_state(reqs, t, lookup)
    planned = mh.read_answer_plan(dec, ks, fill=fill)
    want = RQ.assert_planned(planned, reqs, t, ks, lookup)
    return dec, ks, planned, want


def _encode(reqs, dec, ks, planned):
    t = dec.trimmed()
    ra = mh.read_planned_answers(reqs.wire, ks.store, planned, t["req_nonce_off"], t["req_nonce_len"])
    wire, off, ln, status = mh.result_reply_encode(ra)
    assert (status == mh.ENC_OK).all()
    return [wire[int(o):int(o) + int(n)].tobytes() for o, n in zip(off, ln)]


@pytest.mark.parametrize("layout", ["dense", "aliased"])
def test_plan_equals_the_model(layout):
    cases = RQ.plan_cases()
    reqs = RQ.batch([c.body for c in cases], layout)
    dec, ks, planned, want = _plan(reqs)
    by = {c.name: w[0] for c, w in zip(cases, want)}
    assert all(by[n] == mh.RDA_REPLY for n in by if n.startswith("reply:"))
    assert all(by[n] == mh.RDA_NO_REPLY for n in by if n.startswith("no_reply:")) and by["malformed"] == mh.RDA_NO_REPLY
    assert by["host:65_ops"] == by["host:tx_twice"] == mh.RDA_HOST
    assert len([n for n in by if n.startswith("no_reply:last:")]) == len(RQ.NO_REPLY_CAUSES) == 5
    kinds = {(r.status, bool(r.result), r.existed, bool(r.cert)) for w in want if w[1] for r in w[1]}
    assert {(1, False, False, False), (0, True, True, True), (0, True, True, False), (0, False, False, True),
            (0, False, True, True)} <= kinds


def test_plan_each_case_alone():
    for c in RQ.plan_cases():
        _plan(RQ.batch([c.body], lead=len(c.name) % 4))


@pytest.mark.parametrize("cause", [None] + sorted(RQ.NO_REPLY_CAUSES))
def test_plan_64_ops_cause_in_the_last_op(cause):
    dec, ks, planned, want = _plan(RQ.batch([RQ.full_request(None), RQ.full_request(cause), RQ.full_request(None)]))
    assert [w[0] for w in want] == [mh.RDA_REPLY, mh.RDA_NO_REPLY if cause else mh.RDA_REPLY, mh.RDA_REPLY]
    assert dec.n_ops == 192


def test_plan_empty_batch_and_errors():
    lib = mh.load_library()
    assert lib.mochi_read_answer_plan(0, None, None, None) == mh.OK  # no pointer is needed
    reqs = RQ.batch([RQ.req([(RQ.READ, b"val"), (RQ.READ, b"far")]), RQ.req([(RQ.READ, b"val2")])])
    dec, ks, planned, _ = _plan(reqs)
    t = dec.trimmed()

    def with_(**kw):
        arrays = dict(t)
        arrays.update({k: np.asarray(v, t[k].dtype) for k, v in kw.items()})
        return mh.ReadRequestsDecoded(rc=mh.OK, n_ops=dec.n_ops, n_keys=dec.n_keys, arrays=arrays)

    for off in ([1, 2, 3], [0, 2, 4], [0, 3, 2], [0, 2, 2]):
        with pytest.raises(mh.MochiError, match="req_op_off"):
            mh.read_answer_plan(with_(req_op_off=off), ks)
    with pytest.raises(mh.MochiError, match="op_obj"):
        mh.read_answer_plan(with_(op_obj=[0, 1, 3]), ks)
    mh.read_answer_plan(with_(op_obj=[0, mh.W1_NONE, 2]), ks)  # NONE is no index
    S = ks.store.size
    for name, val in (("key_value_off", S + 1), ("key_value_len", S + 1), ("key_cert_off", S + 1), ("key_cert_len", S + 1)):
        bad = mh.ReadKeyState(**{**{k: getattr(ks, k) for k in ("store",) + tuple(mh._RDK_IN)},
                                 name: np.array([val, 0, 0], getattr(ks, name).dtype)})
        with pytest.raises(mh.MochiError, match="store"):
            mh.read_answer_plan(dec, bad)
    # a NULL array
    d, k, o = mh.ReadRequestsDecoded_C(), mh.ReadKeyState_C(), mh.ReadAnswerPlanned_C()
    assert lib.mochi_read_answer_plan(2, ctypes.addressof(d), ctypes.addressof(k), ctypes.addressof(o)) == mh.EINVAL
    assert lib.mochi_read_answer_plan(2, None, ctypes.addressof(k), ctypes.addressof(o)) == mh.EINVAL


# 6. plan -> encode -> decode ---------------------------------------------------------------------
def test_plan_then_encode_gives_the_models_bytes():
    pytest.importorskip("google.protobuf")
    cases = RQ.plan_cases()
    reqs = RQ.batch([c.body for c in cases])
    dec, ks, planned, want = _plan(reqs)
    bodies = _encode(reqs, dec, ks, planned)
    assert bodies == RQ.expected_bodies(want)
    n = 0
    for c, body, (st, res, nonce) in zip(cases, bodies, want):
        if st != mh.RDA_REPLY:
            continue
        m = RQ.reply_protobuf(body)
        assert m.nonce.encode() == nonce == (b"" if c.name == "reply:no_nonce" else RQ.NONCE), c.name
        assert len(m.result.operations) == len(res) and m.rid == ""
        assert body == E.protobuf_bytes(E.Ans(E.RD, res, nonce=nonce))
        for r, w in zip(m.result.operations, res):
            assert (r.status, r.result.encode(), r.existed, r.HasField("currentCertificate")) == \
                (w.status, w.result, w.existed, w.cert is not None)
            n += 1
    assert n >= 16


def test_encoded_bodies_decode_back_to_the_slots():
    cases = [c for c in RQ.plan_cases() if c.name.startswith("reply:")]
    reqs = RQ.batch([c.body for c in cases])
    dec, ks, planned, want = _plan(reqs)
    bodies = _encode(reqs, dec, ks, planned)
    k = np.array([len(w[1]) for w in want], np.uint32)
    ln = np.array([len(b) for b in bodies], np.uint32)
    off = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.uint64)
    Q = len(bodies)
    r = mh.ResultReplies(wire=np.frombuffer(b"".join(bodies), np.uint8), resp_off=off, resp_len=ln,
                         resp_kind=np.full(Q, mh.RR_READ, np.uint8), req_resp_off=np.arange(Q + 1, dtype=np.uint32), n_ops=k,
                         slot_off=planned["slot_off"])
    back = mh.result_reply_decode(r)
    assert (back["resp_status"] == mh.RRS_OK).all()
    np.testing.assert_array_equal(back["resp_n_ops"], k)
    wire, store = r.wire.tobytes(), ks.store.tobytes()
    for q, (st, res, nonce) in enumerate(want):
        assert wire[int(back["resp_nonce_off"][q]):][:int(back["resp_nonce_len"][q])] == nonce
        for j in range(len(res)):
            s = int(planned["slot_off"][q]) + j
            for name in ("op_status", "op_existed"):
                assert back[name][s] == planned[name][s], (q, j, name)
            assert bool(back["op_flags"][s] & mh.RRO_HAS_CERT) == bool(planned["op_flags"][s] & mh.RAO_HAS_CERT)
            for what in ("result", "cert"):
                a = wire[int(back[f"op_{what}_off"][s]):][:int(back[f"op_{what}_len"][s])]
                b = store[int(planned[f"op_{what}_off"][s]):][:int(planned[f"op_{what}_len"][s])]
                assert a == b, (q, j, what)


# 7. a random round against cluster_harness.Server.read -----------------------------------------------
class _Server(H.Server):
    def local(self, key):  # by key here: a request may mix shards
        return not key.startswith("far/")


def test_random_round_equals_the_harness_server():
    rng = np.random.default_rng(20251)
    srv = _Server(0, "server-0", "localhost:8001", ["server-0"])
    certs = [H.Cert([]) for _ in range(4)]
    cert_bytes = {id(c): E.padded_cert(40 + 17 * i) for i, c in enumerate(certs)}
    hot = ["W1_KEY_%d" % i for i in range(12) if i % 7 != 3]  # shared between requests
    for i in range(400):
        key = "W1_KEY_%d" % i
        if i % 7 == 3:
            continue  # never written: no container
        deleted = i % 5 == 1
        srv.store[key] = H.SVOC(key, None if deleted else "value-%d-é" % i, not deleted, certs[i % 4])
    srv.store["far/held"] = H.SVOC("far/held", "x", True, certs[0])
    reqs, ops_of = [], []
    for q in range(300):
        ops = []
        for j in range(int(rng.integers(1, 6))):
            i = 4 * int(rng.integers(100)) + (q + j) % 3
            key = hot[int(rng.integers(len(hot)))] if rng.random() < 0.3 else "W1_KEY_%d" % (i + (i % 7 == 3))  # a present key
            if rng.random() < 0.08:
                key = ("far/k%d" % q) if rng.random() < 0.7 else "far/held"
            ops.append(H.Op(H.READ, key))
        cause = q % 25
        if cause == 5:
            ops.append(H.Op(H.WRITE, "W1_KEY_0", "v"))
        elif cause == 11:
            ops.insert(0, H.Op(H.READ, ""))
        elif cause == 17:
            ops.append(H.Op(H.READ, "W1_KEY_3"))  # no container
        elif cause == 21:
            ops = []
        ops_of.append(ops)
        reqs.append(RQ.read(b"client-%d" % (q % 9), RQ.transaction([RQ.operation(o.action, o.key.encode(), o.value.encode()) for o in ops]),
                            b"nonce-%d" % q))
    batch = RQ.batch(reqs)
    lookups = []

    def lookup(key: bytes) -> RQ.KeyRec:
        lookups.append(key)
        k = key.decode()
        sv = srv.store.get(k)
        if sv is None:
            return RQ.KeyRec(srv.local(k))
        return RQ.KeyRec(srv.local(k), True, sv.available, None if sv.value is None else sv.value.encode(),
                         None if sv.current_c is None else cert_bytes[id(sv.current_c)])

    dec = mh.read_request_decode(batch)
    t = dec.trimmed()
    ks = RQ.key_state(batch, t, lookup)
    assert len(lookups) == len(set(lookups)) == dec.n_keys < 0.8 * dec.n_ops  # one lookup per distinct key
    planned = mh.read_answer_plan(dec, ks, fill=FILL)
    bodies = _encode(batch, dec, ks, planned)
    counts = {mh.RDA_REPLY: 0, mh.RDA_NO_REPLY: 0}
    for q, ops in enumerate(ops_of):
        res = srv.read(ops)
        st = int(planned["plan_status"][q])
        counts[st] += 1
        assert (st == mh.RDA_NO_REPLY) == (res is None), q
        if res is None:
            assert bodies[q] == b""
            continue
        want = E.Ans(E.RD, tuple(E.OpR(1) if r.status == H.ST_WRONG_SHARD else
                                 E.OpR(0, r.result.encode(), r.existed, cert_bytes[id(r.cert)]) for r in res), nonce=b"nonce-%d" % q)
        assert bodies[q] == E.message(want), q
    assert counts[mh.RDA_NO_REPLY] == 36 and counts[mh.RDA_REPLY] == 264  # twelve of each cause
