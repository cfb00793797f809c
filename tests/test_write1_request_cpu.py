"""Write1 request decoder and key-state join, host forms (mochi_write1_request_decode,
mochi_write1_state_join): the plain-Python model (write1_request_model) agrees with
google.protobuf on every case and every mutation, value for value and error for error
(three named places where the Python runtime departs); the host form equals the model
array for array in dense and in aliased layouts; the capacity rule; argument errors; the
batch-wide key numbering at its edges; the join at its edges; and the server's round on
the host: bodies -> decode -> join -> mochi_write1_issue equals mochi_write1_issue on the
SoA batch the bodies were encoded from."""
import numpy as np
import pytest

import mochi_hip as mh
import workload as W
import write1_request_model as QM

FILL = 0xA5
WD = mh.W1OP_WRITE | mh.W1OP_DELETE


def check(reqs):
    want = QM.decode(reqs)
    got = mh.write1_request_decode(reqs)
    assert got.rc == mh.OK and got.n_ops == len(want["op_obj"]) and got.n_keys == len(want["key_op"])
    QM.assert_equal(got.trimmed(), want)
    assert mh.write1_request_decode_bound(np.asarray(reqs.wire).size, reqs.n_reqs) >= got.n_ops
    return got


def one(body):
    return {k: v.tolist() for k, v in check(QM.batch([body])).trimmed().items()}


# 1. the model against google.protobuf ------------------------------------------------
def test_model_agrees_with_google_protobuf():
    pytest.importorskip("google.protobuf")
    cases = QM.own_cases() + QM.mutations()
    assert set(QM.PYTHON_DEPARTS) <= {c.name for c in cases}
    for c in cases:
        QM.crosscheck(c.body, QM.decode_body(c.body), QM.PYTHON_DEPARTS.get(c.name, (None,))[0])


def test_what_the_cases_cover():
    st = {c.name: QM.decode_body(c.body) for c in QM.own_cases()}
    ok, mal, fb = mh.W1Q_OK, mh.W1Q_MALFORMED, mh.W1Q_FALLBACK
    assert st["empty"] == QM.Body(ok)
    assert st["repeat:scalars"].seed == 2 and st["seed:0"].seed == 0 and st["seed:max"].seed == 2 ** 32 - 1
    assert st["seed:10_bytes"].seed == 0x12345678
    assert [st["ops:%s" % n].status for n in ("0", "1", "64", "65", "65_one_bad")] == [ok, ok, ok, fb, mal]
    assert [st["tx:" + n].status for n in ("twice", "twice_second_bad", "twice_first_bad")] == [fb, mal, mal]
    assert [st["action:" + n].ops[0][0] for n in ("0", "1", "2", "3", "2_31", "10_bytes_low_2")] == [0, 1, 2, 3, 2 ** 31, 2]
    for where in ("top", "op"):
        assert [st["group:%s_%d" % (where, d)].status for d in (1, 100, 101)] == [ok, ok, mal]
    assert all(d.status == mal for n, d in st.items() if n.startswith("utf8:"))
    assert all(d.status == ok for n, d in st.items() if n.startswith(("foreign:", "unknown:", "key:", "only:")))
    bodies = QM.mutation_bodies()
    assert all(QM.decode_body(b).status == ok for b in bodies)
    tags = set()  # every field of the three messages is in one of the three bodies
    for b in bodies:
        for f, wt, _, po, pl in QM.DM._msg(b, 0, len(b)):
            tags.add(("w", f, wt))
            if (f, wt) == (2, 2):
                for ef, ewt, _, eo, el in QM.DM._msg(b, po, pl):
                    tags.add(("t", ef, ewt))
                    if (ef, ewt) == (1, 2):
                        tags |= {("o", of, owt) for of, owt, *_ in QM.DM._msg(b, eo, el)}
    assert tags >= {("w", 1, 2), ("w", 2, 2), ("w", 3, 0), ("w", 4, 2), ("t", 1, 2), ("o", 1, 0), ("o", 2, 2), ("o", 3, 2),
                    ("o", 4, 2)}
    stm = [QM.decode_body(c.body).status for c in QM.mutations()]
    assert stm.count(ok) > 300 and stm.count(mal) > 300


# 2. the host form against the model ---------------------------------------------------
@pytest.mark.parametrize("layout", ["dense", "aliased"])
@pytest.mark.parametrize("which", ["own", "mutations"])
def test_host_form_equals_the_model(which, layout):
    cases = QM.own_cases() if which == "own" else QM.mutations()
    got = check(QM.batch([c.body for c in cases], layout))
    assert set(got.arrays["req_status"].tolist()) == ({0, 1, 2} if which == "own" else {0, 1})


def test_each_own_case_alone():
    for c in QM.own_cases():
        check(QM.batch([c.body], lead=len(c.name) % 5))


def test_values():
    r = one(QM.write1(b"client-1", QM.transaction([QM.operation(QM.WRITE, b"k1", b"v"), QM.operation(QM.READ, b"k1"),
                                                    QM.operation(QM.DELETE, b"k2"), QM.operation(7, b"k2")]), 9, b"hh"))
    assert r["req_status"] == [0] and r["req_seed"] == [9] and r["req_hash_len"] == [2] and r["req_client_len"] == [8]
    assert r["op_flags"] == [mh.W1OP_WRITE, 0, mh.W1OP_DELETE, 0] and r["op_obj"] == [0, mh.W1_NONE, 1, mh.W1_NONE]
    assert r["key_op"] == [0, 2] and r["op_key_len"] == [2, 2, 2, 2] and r["req_op_off"] == [0, 4]
    # absent fields: the request's own offset, length 0
    r = one(QM.write1(tx=QM.transaction([b"\x08\x02"])))
    assert r["req_hash_off"] == r["req_client_off"] == r["op_key_off"] == [3] and r["op_key_len"] == [0]
    assert r["op_obj"] == [mh.W1_NONE] and r["key_op"] == []
    # not decoded: nothing but the status
    r = one(b"\x0a\x05abc")
    assert r["req_status"] == [mh.W1Q_MALFORMED] and r["req_op_off"] == [0, 0]
    assert r["req_seed"] == r["req_hash_off"] == r["req_hash_len"] == r["req_client_off"] == r["req_client_len"] == [0]


def test_empty_batch():
    got = check(mh.Write1Requests(wire=np.zeros(0, np.uint8), msg_off=np.zeros(0, np.uint64), msg_len=np.zeros(0, np.uint32)))
    assert got.n_ops == 0 and got.arrays["req_op_off"].tolist() == [0]


# 3. capacity, argument errors ------------------------------------------------------------
def test_capacity_one_short_touches_nothing():
    r = QM.batch([c.body for c in QM.own_cases()])
    full = mh.write1_request_decode(r)
    got = mh.write1_request_decode_into(r, full.n_ops - 1, fill=FILL)
    assert got.rc == mh.EINVAL and got.n_ops == full.n_ops
    for k, (dt, w) in mh._W1Q_OUT.items():
        if w in ("O", "K"):
            assert (got.arrays[k].view(np.uint8) == FILL).all(), k
        else:
            np.testing.assert_array_equal(got.arrays[k], full.arrays[k])
    exact = mh.write1_request_decode_into(r, full.n_ops, fill=FILL)
    assert exact.rc == mh.OK and (exact.arrays["key_op"][exact.n_keys:].view(np.uint8) == FILL).all()
    QM.assert_equal(exact.trimmed(), full.trimmed())


def test_argument_errors():
    body = QM.own_cases()[6].body
    r = QM.batch([body, body], lead=0)
    end = r.wire.size
    for off, ln in (([0, end - len(body) + 1], [len(body)] * 2), ([0, end + 1], [len(body), 0]), ([0, 0], [len(body), end + 1])):
        bad = mh.Write1Requests(wire=r.wire, msg_off=np.array(off, np.uint64), msg_len=np.array(ln, np.uint32))
        with pytest.raises(mh.MochiError, match="outside wire"):
            mh.write1_request_decode(bad)
    check(mh.Write1Requests(wire=r.wire, msg_off=np.array([end, 0], np.uint64), msg_len=np.array([0, end], np.uint32)))
    # more than 2^24 requests: refused before any array is read (the arrays here hold two)
    import ctypes

    lib = mh.load_library()
    c, keep = r.to_c()
    out = mh.write1_request_decode_into(r, 8)
    o = mh.Write1RequestsDecoded_C()
    for k, a in out.arrays.items():
        setattr(o, k, a.ctypes.data)
    o.op_cap = 8
    for n, rc in (((1 << 24) + 1, mh.EINVAL), (2, mh.OK)):
        c.n_reqs = n
        assert lib.mochi_write1_request_decode(ctypes.addressof(c), ctypes.addressof(o)) == rc
    c.n_reqs = (1 << 24) + 1
    lib.mochi_write1_request_decode(ctypes.addressof(c), ctypes.addressof(o))
    assert "2^24" in mh._err(lib)


# 4. the key numbering -------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(QM.dedup_batches()))
def test_key_numbering(name):
    got = check(QM.batch(QM.dedup_batches()[name])).trimmed()
    obj, key_op = got["op_obj"].tolist(), got["key_op"].tolist()
    if name == "one_key":
        assert obj == [0] * 80 and key_op == [0]
    elif name == "all_distinct":
        assert obj == list(range(80)) == key_op
    elif name == "last_byte":
        assert len(key_op) == 26 and obj[:4] == [0, 1, 2, 1]
    elif name == "prefix":
        assert obj == [0, 1, 2, 0, 3] and key_op == [0, 1, 2, 4]
    elif name == "ok_and_malformed":  # the malformed request's ops are gone: `shared` is numbered from the second request
        assert got["req_status"].tolist() == [1, 0, 0] and obj == [0, 1, 2] and key_op == [0, 1, 2]
    else:
        assert obj == [mh.W1_NONE, 0, mh.W1_NONE, mh.W1_NONE, mh.W1_NONE] and key_op == [1]


# 5. the join -----------------------------------------------------------------------------------
def test_join():
    off, seed, flags, obj, ks, want_stored = QM.join_case()
    fl, ep, st = mh.write1_state_join(off, seed, flags, obj, ks)
    mfl, mep, mst = QM.join(off, seed, flags, obj, ks)
    np.testing.assert_array_equal(fl, mfl)
    np.testing.assert_array_equal(ep, mep)
    np.testing.assert_array_equal(st, mst)
    assert st.tolist() == want_stored
    assert fl.tolist() == [4 | 3, 8 | 1, 0, 4 | 3, 4 | 3, 4, 8 | 2, 4 | 3, 4 | 1]
    assert ep.tolist() == [1000, 2000, 0, 100, 2 ** 63 - 4, -7, 50, 0, 2000]


def test_join_empty_and_errors():
    ks0 = mh.Write1KeyState(*(np.zeros(n, dt) for n, dt in ((0, np.uint8), (0, np.int64), (1, np.uint32), (0, np.int64),
                                                             (0, np.uint32))))
    fl, ep, st = mh.write1_state_join([0], [], [], [], ks0)
    assert fl.size == ep.size == st.size == 0
    fl, ep, st = mh.write1_state_join([0, 1], [3], [4], [mh.W1_NONE], ks0)
    assert (fl.tolist(), ep.tolist(), st.tolist()) == ([4], [0], [mh.W1_NONE])
    off, seed, flags, obj, ks, _ = QM.join_case()
    with pytest.raises(mh.MochiError, match="op_obj"):
        mh.write1_state_join(off, seed, flags, [7] + obj[1:], ks)
    for bad in ([1, 0, 3, 6, 8, 9, 11, 11], [0, 0, 3, 2, 8, 9, 11, 11], [0, 0, 3, 6, 8, 9, 11, 12], [0, 0, 3, 6, 8, 9, 11, 10]):
        kb = mh.Write1KeyState(ks.key_flags, ks.key_epoch, np.array(bad, np.uint32), ks.given_ts, ks.given_stored)
        with pytest.raises(mh.MochiError, match="key_given_off"):
            mh.write1_state_join(off, seed, flags, obj, kb)
    with pytest.raises(mh.MochiError, match="req_op_off"):
        mh.write1_state_join([0, 3, 5, 5, 8], seed, flags, obj, ks)


# 6. the server's round on the host ---------------------------------------------------------------
def decoded_batch(b, dec, fl, ep, st, wire, sh_off, sh_len):
    t = dec.trimmed()
    return mh.Write1Batch(strings=wire, req_op_off=t["req_op_off"], req_seed=t["req_seed"], req_hash_off=t["req_hash_off"],
                          req_hash_len=t["req_hash_len"], op_key_off=t["op_key_off"], op_key_len=t["op_key_len"], op_flags=fl,
                          op_obj=t["op_obj"], op_epoch=ep, op_stored=st, stored_hash_off=sh_off, stored_hash_len=sh_len)


@pytest.mark.parametrize("n_reqs, k, contention", [(300, 2, 0.1), (64, 5, 0.6)])
def test_round_on_the_host_equals_the_soa_batch(n_reqs, k, contention):
    b = W.make_write1_batch(n_reqs, k=k, contention=contention, stored=0.2)
    assert (np.asarray(b.op_stored) != mh.W1_NONE).sum() > 5
    reqs, sh_off, sh_len = QM.wire_of_batch(b)
    dec = check(reqs)
    t = dec.trimmed()
    assert (t["req_status"] == 0).all() and dec.n_ops == b.n_ops and dec.n_keys == np.unique(b.op_obj).size < b.n_ops
    assert QM.same_partition(t["op_obj"], b.op_obj)
    ks = QM.key_state_of(b, t["key_op"], t["op_obj"])
    fl, ep, st = mh.write1_state_join(t["req_op_off"], t["req_seed"], t["op_flags"], t["op_obj"], ks)
    np.testing.assert_array_equal(fl, b.op_flags)
    np.testing.assert_array_equal(ep, b.op_epoch)
    np.testing.assert_array_equal(st, b.op_stored)
    got = mh.write1_issue(decoded_batch(b, dec, fl, ep, st, reqs.wire, sh_off, sh_len))
    want = mh.write1_issue(b)
    assert got.rc == want.rc == mh.OK and got.n_new == want.n_new > 0
    for name in ("op_decision", "op_grant", "req_kind", "req_grant_off", "req_grant", "grant_len", "grant_op", "grant_ts"):
        np.testing.assert_array_equal(getattr(got, name), getattr(want, name), err_msg=name)
    assert [got.grant(g) for g in range(got.n_new)] == [want.grant(g) for g in range(want.n_new)]
    assert len(set(got.op_decision.tolist())) >= 3
