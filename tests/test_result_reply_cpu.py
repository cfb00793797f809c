"""Result reply decoder and coalescing step, host forms (mochi_result_reply_decode,
mochi_result_coalesce): the plain-Python model (result_reply_model) agrees with
google.protobuf on every named case and the whole mutation corpus, value for value and
error for error (with the named places where the Python runtime departs, one test each);
the host form equals the model array for array in dense, aliased and guarded layouts;
decode -> mochi_tally_responses -> coalesce equals the plain-Python client; argument
errors with their texts."""
import ctypes

import numpy as np
import pytest

import mochi_hip as mh
import result_reply_model as M

OK, MAL, FB = mh.RRS_OK, mh.RRS_MALFORMED, mh.RRS_FALLBACK


def check(r, what=""):
    n = M.n_slots(r)
    got = mh.result_reply_decode(r, n, fill=M.FILL)
    M.assert_equal(got, M.decode(r, n), what)
    return got


def one(case, **kw):
    return {k: v.tolist() for k, v in check(M.batch([case], **kw), case.name).items()}


# 1. the model against google.protobuf ------------------------------------------------
def test_model_agrees_with_google_protobuf():
    pytest.importorskip("google.protobuf")
    cases = M.own_cases() + M.corpus()
    assert set(M.PYTHON_DEPARTS) <= {c.name for c in cases}
    for c in cases:
        if c.kind != M.OTHER:
            M.crosscheck(c.body, c.kind, M.decode_body(c.body, c.kind, M.MAX_OPS), M.PYTHON_DEPARTS.get(c.name, (None,))[0])


def _case(name):
    return next(c for c in M.own_cases() + M.corpus() if c.name == name)


@pytest.mark.parametrize("name", sorted(M.PYTHON_DEPARTS))
def test_where_python_departs(name):
    """Each named departure, alone: the runtime's verdict, the model's, and the host form's
    (which is the model's: the rule of protobuf-java as csrc/wire_walk.h states it)."""
    pytest.importorskip("google.protobuf")
    c = _case(name)
    rule = M.PYTHON_DEPARTS[name][0]
    d = M.decode_body(c.body, c.kind, c.n_ops)
    m = M.parse_protobuf(c.body, c.kind)
    assert (m is None, d.status == MAL) == ((True, False) if rule == "python_rejects" else (False, True))
    assert one(c)["resp_status"] == [d.status]


def test_enum_values_outside_the_range_are_kept_as_int32():
    """readEnum keeps the low 32 bits, signed; Python holds the same int32 (no departure), and
    the library's byte is that value inside 0..254, else 0xFF."""
    pytest.importorskip("google.protobuf")
    for nm, want, byte in (("2_31", -2 ** 31, 0xFF), ("neg", -1, 0xFF), ("255", 255, 0xFF), ("254", 254, 254), ("2", 2, 2)):
        c = _case("status:" + nm)
        assert M.parse_protobuf(c.body, c.kind).result.operations[0].status == want
        assert M.decode_body(c.body, c.kind, 2).ops[0].status == want
        assert one(c)["op_status"][:2] == [byte, 1]
    c = _case("status:10_bytes_low_1")
    assert [o.status for o in M.parse_protobuf(c.body, c.kind).result.operations] == [1, -1]
    assert one(c)["op_status"][:2] == [1, 0xFF]


def test_what_the_cases_cover():
    st = {c.name: M.decode_body(c.body, c.kind, c.n_ops) for c in M.own_cases()}
    assert st["empty"] == M.Body(OK, 0) and st["kind:other_garbage"] == M.Body(OK, 0)
    assert (st["utf8:field3_write2"].status, st["utf8:field3_read"].status) == (OK, MAL)
    assert all(d.status == MAL for n, d in st.items() if n.startswith("utf8:") and n not in
               ("utf8:field3_write2", "utf8:result_multibyte"))
    assert [st["count:" + n].status for n in ("n_minus_1", "n_plus_1", "n_plus_1_bad_cert", "n_plus_1_cert_twice")] == [OK, OK, MAL, OK]
    assert [st["count:" + n].n_ops for n in ("n_minus_1", "n_plus_1", "64", "63_of_64", "65_of_64", "65_trivial")] == [1, 3, 64, 63, 65, 65]
    assert [st["count:" + n].status for n in ("65_one_bad", "65_cert_twice", "65_result_twice", "64_last_bad")] == [MAL, OK, FB, MAL]
    assert [st["result:" + n].status for n in ("twice", "twice_empty", "twice_second_bad", "twice_first_bad")] == [FB, FB, MAL, MAL]
    assert [st["cert:" + n].status for n in ("twice", "twice_second_empty", "twice_second_bad", "twice_and_utf8")] == [FB, FB, MAL, MAL]
    assert [st["cert:" + n].status for n in ("empty", "bad", "bad_grant", "foreign_wire_type")] == [OK, MAL, MAL, OK]
    assert st["repeat:top_strings"].rid[1] == 2 and st["repeat:op_scalars"].ops[0][:2] == (0, True)
    assert [o.existed for o in st["existed:2"].ops] == [True, True] and st["existed:10_bytes_high"].ops[0].existed
    assert [st["group:op_%d" % d].status for d in (1, 98, 99, 100, 101)] == [OK, OK, OK, OK, MAL]
    assert [st["group:top_%d" % d].status for d in (1, 100, 101)] == [OK, OK, MAL]
    assert all(d.status == OK for n, d in st.items() if n.startswith(("foreign:", "unknown:", "only:", "full:", "status:")))
    # every field of the four messages is in one of the mutation bodies
    tags = set()
    for kind, b, k in M.mutation_bodies():
        for f, wt, _, po, pl in M.DM._msg(b, 0, len(b)):
            tags.add((kind, f, wt))
            if (f, wt) == (1, 2):
                for ef, ewt, _, eo, el in M.DM._msg(b, po, pl):
                    tags.add(("t", ef, ewt))
                    tags |= {("o", of, owt) for of, owt, *_ in M.DM._msg(b, eo, el)}
    assert tags >= {(M.W2, 1, 2), (M.W2, 2, 2), (M.RD, 1, 2), (M.RD, 2, 2), (M.RD, 3, 2), ("t", 1, 2), ("o", 1, 2), ("o", 2, 2),
                    ("o", 3, 0), ("o", 4, 0)}


def test_corpus_holds_every_status():
    """A corpus that drifts to all-malformed checks little: 50 bodies or more of each status."""
    st = [M.decode_body(c.body, c.kind, c.n_ops).status for c in M.corpus()]
    assert min(st.count(OK), st.count(MAL), st.count(FB)) >= 50, [st.count(s) for s in (OK, MAL, FB)]
    names = {c.name.split(":")[0] for c in M.corpus()}
    assert names == {"cut", "flip", "shuffle"}


# 2. the host form against the model ---------------------------------------------------
@pytest.mark.parametrize("slots", ["dense", "guarded"])
@pytest.mark.parametrize("layout", ["dense", "aliased"])
@pytest.mark.parametrize("which", ["own", "corpus"])
def test_host_form_equals_the_model(which, layout, slots):
    cases = M.own_cases() if which == "own" else M.corpus()
    got = check(M.batch(cases, layout, slots=slots))
    assert set(got["resp_status"].tolist()) == {OK, MAL, FB}


def test_each_own_case_alone():
    for c in M.own_cases():
        check(M.batch([c], lead=len(c.name) % 5), c.name)


@pytest.mark.parametrize("k", [0, 1, 2, 64])
def test_one_request_owns_every_response(k):
    cases = M.own_cases()
    check(M.batch(cases, grouping="one", slots="guarded", n_ops=k))


def test_values():
    c = M.cert()
    body = M.answer(M.RD, [M.op_result(0, b"val", True, c), M.WS], b"rid-9", b"nonce")
    r = one(M.Case("v", M.RD, body, 3), lead=4)
    assert r["resp_status"] == [OK] and r["resp_n_ops"] == [2]
    assert body[r["resp_rid_off"][0] - 4:][:r["resp_rid_len"][0]] == b"rid-9"
    assert body[r["resp_nonce_off"][0] - 4:][:r["resp_nonce_len"][0]] == b"nonce"
    assert r["op_status"][:3] == [0, 1, 0xFF] and r["op_existed"][:3] == [1, 0, 0]
    assert r["op_flags"][:3] == [mh.RRO_HAS_CERT, 0, 0]
    assert body[r["op_result_off"][0] - 4:][:r["op_result_len"][0]] == b"val"
    assert body[r["op_cert_off"][0] - 4:][:r["op_cert_len"][0]] == c
    # absent fields: the operation's own offset, length 0 (WRONG_SHARD carries `status` alone)
    ws = body.index(M.WS, len(c)) + 4
    assert (r["op_result_off"][1], r["op_result_len"][1], r["op_cert_off"][1], r["op_cert_len"][1]) == (ws, 0, ws, 0)
    assert r["op_result_off"][2] == r["op_cert_off"][2] == 0
    # a Write2 answer has no nonce; an answer without strings: the response's own offset
    r = one(M.Case("v", M.W2, M.answer(M.W2, [M.WS]), 1), lead=7)
    assert (r["resp_rid_off"], r["resp_rid_len"], r["resp_nonce_off"], r["resp_nonce_len"]) == ([7], [0], [7], [0])
    # not decoded: a count no n_ops equals, every slot absent
    for name in ("len:past_end", "result:twice_empty"):
        r = one(_case(name), lead=5)
        assert r["resp_n_ops"] == [mh.RR_UNDECODED] and r["resp_rid_off"] == r["resp_nonce_off"] == [0]
    r = one(_case("count:64_last_bad"))
    assert r["resp_status"] == [MAL] and r["op_status"][:64] == [0xFF] * 64 and r["op_flags"][:64] == [0] * 64
    r = one(_case("kind:other"), lead=5)
    assert r["resp_status"] == [OK] and r["resp_n_ops"] == [0] and r["resp_rid_off"] == [0] and r["op_status"][:2] == [0xFF] * 2


def test_empty_batch_needs_no_pointer():
    lib = mh.load_library()
    r, o = mh.ResultReplies_C(), mh.ResultDecoded_C()
    assert lib.mochi_result_reply_decode(ctypes.addressof(r), ctypes.addressof(o)) == mh.OK
    r.n_reqs = 3
    assert lib.mochi_result_reply_decode(ctypes.addressof(r), ctypes.addressof(o)) == mh.OK
    t, c = mh.ResultTallied_C(), mh.ResultCoalesced_C()
    assert lib.mochi_result_coalesce(ctypes.addressof(t), ctypes.addressof(c)) == mh.OK
    got = check(M.batch([]))
    assert all((v.view(np.uint8) == M.FILL).all() for v in got.values())


# 3. decode -> tally -> coalesce against the plain-Python client -------------------------
def run_client(r, R, fill=M.FILL):
    Q = r.n_reqs
    k = np.asarray(r.n_ops, np.int64)
    # the coalesced entries of request q: descending, two guards between the runs
    out_off = (np.cumsum((k + 2)[::-1])[::-1] - k).astype(np.uint64) if Q else np.zeros(0, np.uint64)
    n_out = int(k.sum() + 2 * Q + 2)
    chosen_off = np.concatenate([[0], np.cumsum(k)])[:-1].astype(np.uint64)
    dec = mh.result_reply_decode(r, M.n_slots(r), fill=fill)
    chosen, reason, bits = M.tally_host(r, dec, R, chosen_off, int(k.sum()))
    got = mh.result_coalesce(r, dec, chosen, chosen_off, bits, out_off, n_out, fill=fill)
    accept, why, want = M.client(r, R, out_off, n_out, fill)
    np.testing.assert_array_equal(mh.unpack_bits(bits, Q), accept)
    np.testing.assert_array_equal(reason, why)
    M.assert_equal(got, want)
    return accept, got


@pytest.mark.parametrize("slots", ["dense", "guarded"])
def test_decode_tally_coalesce_equals_the_client(slots):
    groups, ks = M.cluster_batch()
    accept, got = run_client(M.batch_grouped(groups, ks, slots), 4)
    assert accept.any() and not accept.all()
    assert (got["flags"] == mh.RRO_HAS_CERT).any() and (got["existed"] == 1).any()


def test_client_on_the_named_cases():
    """Every named case as the only answer (R = 1: a majority of one), and all of them to one request."""
    cases = M.own_cases()
    accept, _ = run_client(M.batch(cases), 1)
    assert accept.any() and not accept.all()
    run_client(M.batch(cases, grouping="one", n_ops=2), 4)
    run_client(M.batch([]), 4)


# 4. argument errors ---------------------------------------------------------------------
def _decode_rc(r, edit=None, out_edit=None):
    lib = mh.load_library()
    r = mh.ResultReplies(**{k: np.array(getattr(r, k), dt) for k, dt in r.DTYPES.items()})  # edits stay in this call
    c, keep = r.to_c()
    n = dict(P=r.n_resps, S=M.n_slots(r))
    arr = {k: np.zeros(max(n[w], 1), dt) for k, (dt, w) in mh._RR_OUT.items()}
    o = mh.ResultDecoded_C()
    for k, a in arr.items():
        setattr(o, k, mh._ptr(a))
    if edit:
        edit(c, keep)
    if out_edit:
        out_edit(o)
    rc = lib.mochi_result_reply_decode(ctypes.addressof(c), ctypes.addressof(o))
    return rc, mh._err(lib)


def test_argument_errors():
    lib = mh.load_library()
    r = M.batch(M.own_cases()[:6])
    assert _decode_rc(r)[0] == mh.OK

    def bad(text, edit=None, out_edit=None):
        rc, err = _decode_rc(r, edit, out_edit)
        assert rc == mh.EINVAL and text in err, (rc, err)

    def poke(name, i, v):
        def f(c, keep):
            keep[name][i] = v
        return f

    bad("a response slice lies outside wire", poke("resp_off", 2, r.wire.size + 1))
    bad("a response slice lies outside wire", poke("resp_len", 5, r.wire.size))
    bad("req_resp_off is not a CSR over n_resps", poke("req_resp_off", 0, 1))
    bad("req_resp_off is not a CSR over n_resps", poke("req_resp_off", 6, 5))
    bad("req_resp_off is not a CSR over n_resps", poke("req_resp_off", 3, 5))
    bad("more than MOCHI_MAX_OPS_PER_CERT ops", poke("n_ops", 1, 65))
    bad("resp_kind is no MOCHI_RR_*", poke("resp_kind", 0, 3))
    bad("more than 2^24 responses", lambda c, keep: setattr(c, "n_resps", 2 ** 24 + 1))
    bad("responses without a request", lambda c, keep: setattr(c, "n_reqs", 0))
    for name in ("wire", "resp_off", "resp_len", "resp_kind"):
        bad("wire / resp_off / resp_len / resp_kind required", lambda c, keep, name=name: setattr(c, name, None))
    for name in ("req_resp_off", "n_ops", "slot_off"):
        bad("req_resp_off / n_ops / slot_off required", lambda c, keep, name=name: setattr(c, name, None))
    for name, (dt, w) in mh._RR_OUT.items():
        bad("the per-response outputs are required" if w == "P" else "the per-slot outputs are required",
            out_edit=lambda o, name=name: setattr(o, name, None))
    assert lib.mochi_result_reply_decode(None, None) == mh.EINVAL and "null argument" in mh._err(lib)


def test_coalesce_argument_errors():
    lib = mh.load_library()
    groups, ks = M.cluster_batch(4)
    r = M.batch_grouped(groups, ks)
    dec = mh.result_reply_decode(r)
    k = np.asarray(ks, np.int64)
    off = np.concatenate([[0], np.cumsum(k)])[:-1].astype(np.uint64)
    chosen, reason, bits = M.tally_host(r, dec, 4, off, int(k.sum()))
    assert bits[0] & 1  # request 0 is accepted: its chosen entries are read
    mh.result_coalesce(r, dec, chosen, off, bits, off, int(k.sum()))
    bad_chosen = chosen.copy()
    bad_chosen[0] = 4
    with pytest.raises(mh.MochiError, match="a chosen index lies past the request's responses"):
        mh.result_coalesce(r, dec, bad_chosen, off, bits, off, int(k.sum()))
    r2 = M.batch_grouped(groups, ks)
    r2.req_resp_off = r2.req_resp_off.copy()
    r2.req_resp_off[1] = 9
    with pytest.raises(mh.MochiError, match="req_resp_off descends"):
        mh.result_coalesce(r2, dec, chosen, off, bits, off, int(k.sum()))
    r3 = M.batch_grouped(groups, ks)
    r3.n_ops = r3.n_ops.copy()
    r3.n_ops[2] = 65
    with pytest.raises(mh.MochiError, match="more than MOCHI_MAX_OPS_PER_CERT ops"):
        mh.result_coalesce(r3, dec, chosen, off, bits, off, int(k.sum()))
    t, c = mh.ResultTallied_C(), mh.ResultCoalesced_C()
    t.n_reqs = 1
    assert lib.mochi_result_coalesce(ctypes.addressof(t), ctypes.addressof(c)) == mh.EINVAL
    assert "chosen / chosen_off / accept_bits" in mh._err(lib)
    dummy = np.zeros(8, np.uint64)
    for name in ("req_resp_off", "n_ops", "chosen", "chosen_off", "accept_bits", "slot_off", "out_off"):
        setattr(t, name, mh._ptr(dummy))
    assert lib.mochi_result_coalesce(ctypes.addressof(t), ctypes.addressof(c)) == mh.EINVAL
    assert "the per-slot inputs are required" in mh._err(lib)
    for name in mh._RR_SLOT:
        setattr(t, name, mh._ptr(dummy))
    assert lib.mochi_result_coalesce(ctypes.addressof(t), ctypes.addressof(c)) == mh.EINVAL
    assert "the coalesced outputs are required" in mh._err(lib)
    assert lib.mochi_result_coalesce(None, None) == mh.EINVAL and "null argument" in mh._err(lib)
