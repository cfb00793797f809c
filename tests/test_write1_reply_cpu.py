"""Write1 reply encoder, host form (mochi_write1_reply_encode): byte-exact with
the plain-Python model on every issue case set and on the encoder's own hand,
varint-step, certificate-length and alignment sets; the bodies read back with
google.protobuf; the capacity rule; every argument error with its text."""
import ctypes

import numpy as np
import pytest

import mochi_hip as mh
import write1_issue_model as M
import write1_reply_model as RM


@pytest.fixture(scope="module")
def own_cases():
    return RM.reply_cases()


@pytest.fixture(scope="module")
def models(own_cases):
    return {k: RM.encode(*v) for k, v in own_cases.items()}


def _check(case, want=None):
    """Host form == model, byte for byte, with offsets, lengths and statuses."""
    batch, issued, src = case
    want = want or RM.encode(batch, issued, src)
    wire, off, ln, st = mh.write1_reply_encode(batch, issued, src)
    lens = np.array([len(b) for b in want.bodies], np.int64)
    np.testing.assert_array_equal(ln, lens)
    np.testing.assert_array_equal(off, np.concatenate([[0], np.cumsum(lens)[:-1]]) if len(lens) else lens)
    assert (st == mh.ENC_OK).all()
    assert wire.tobytes() == want.wire
    bound = mh.write1_reply_bound(batch, src, issued.grant_bytes_len, issued.sig is not None)
    assert bound >= wire.size
    return wire, off, ln


ISSUE_NAMES = sorted(M.hand_cases()) + sorted(M.edge_cases()) + [f"random{i}" for i in range(6)] + ["alignment"]


# 1. byte-exact with the model ------------------------------------------------------
@pytest.mark.parametrize("sigs", [True, False], ids=["sig", "nosig"])
@pytest.mark.parametrize("certs", [True, False], ids=["certs", "nocerts"])
def test_issue_cases_equal_the_model(certs, sigs):
    cases = RM.issue_cases(certs, sigs)
    assert sorted(cases) == sorted(ISSUE_NAMES)
    kinds = set()
    for name, case in cases.items():
        _check(case)
        kinds |= set(case[1].req_kind.tolist())
    assert kinds == {mh.W1K_OK, mh.W1K_REFUSED, mh.W1K_THROWS}


@pytest.mark.parametrize("name", ["ok_empty_no_ids", "ok_empty_ids", "throws", "refused_mixed", "ok_64_ops", "one_key_twice",
                                  "stored_shared", "cert_alias", "steps", "cert_lens", "alignment"])
def test_own_cases_equal_the_model(own_cases, models, name):
    _check(own_cases[name], models[name])


# 2. hand cases: what each one is about ------------------------------------------------
def test_ok_without_grants_is_an_empty_multigrant(own_cases, models):
    assert models["ok_empty_no_ids"].bodies == [b"\x0a\x00", b"\x0a\x00"]
    wire, off, ln, st = mh.write1_reply_encode(*own_cases["ok_empty_no_ids"])
    assert wire.tobytes() == b"\x0a\x00\x0a\x00" and ln.tolist() == [2, 2]
    ids = models["ok_empty_ids"].bodies
    assert ids[0] == b"\x0a\x14" + b"\x12\x08client-0" + b"\x22\x08server-0"
    wire, off, ln, st = mh.write1_reply_encode(*own_cases["ok_empty_ids"])
    assert wire.tobytes() == b"".join(ids)


def test_throws_gets_an_empty_body(own_cases):
    batch, issued, src = own_cases["throws"]
    assert issued.req_kind.tolist() == [mh.W1K_THROWS, mh.W1K_THROWS, mh.W1K_OK]
    wire, off, ln, st = mh.write1_reply_encode(batch, issued, src)
    assert ln[0] == 0 and ln[1] == 0 and ln[2] > 2 and st.tolist() == [0, 0, 0] and off.tolist() == [0, 0, 0]


def test_refused_mixes_a_stored_and_a_new_grant(own_cases, models):
    batch, issued, src = own_cases["refused_mixed"]
    assert issued.req_kind.tolist() == [mh.W1K_OK, mh.W1K_REFUSED]
    refs = issued.req_grant[int(issued.req_grant_off[1]):int(issued.req_grant_off[2])].tolist()
    assert refs == [mh.W1_STORED | 0, 0]
    body = models["refused_mixed"].bodies[1]
    assert RM.fake_sig(1, 0) in body and RM.fake_sig(0, 0) in body  # the stored grant's and the new grant's signature
    assert issued.grant(0) in body and src.stored_bytes[:int(src.stored_len[0])].tobytes() in body


def test_64_ops_and_one_key_twice(own_cases, models):
    batch, issued, src = own_cases["ok_64_ops"]
    assert batch.n_ops == 64 and int(issued.req_grant_off[1]) == 64
    assert len(models["ok_64_ops"].lengths["grants_entry"]) == 64
    batch, issued, src = own_cases["one_key_twice"]
    assert np.diff(issued.req_grant_off.astype(np.int64)).tolist() == [1, 1]
    assert len(models["one_key_twice"].lengths["grants_entry"]) == 2


def test_stored_grant_shared_and_aliased_certificates(own_cases, models):
    batch, issued, src = own_cases["stored_shared"]
    assert (issued.req_grant == (mh.W1_STORED | 0)).sum() >= 3
    batch, issued, src = own_cases["cert_alias"]
    assert len(set(src.op_cert_off.tolist())) == 2 and batch.n_ops == 12
    assert sum(b"C" * 300 in b for b in models["cert_alias"].bodies) == 6


# 3. varint steps, certificate lengths, alignment: the coverage is asserted ---------------
def test_varint_steps_are_covered(models):
    got = models["steps"].lengths
    for what in ("grants_entry", "multigrant", "cert_value", "cert_entry", "message"):
        assert set(RM.STEPS) <= set(got[what]), (what, sorted(set(got[what])))


def test_certificate_lengths_are_covered(models):
    assert sorted(models["cert_lens"].lengths["cert_value"]) == sorted(RM.CERT_LENS)


def test_alignment_set_covers_every_residue_pair(models):
    runs = models["alignment"].runs
    assert {r.kind for r in runs} == {"grant", "sig", "cert"}
    assert len(RM.residues(runs)) == 256
    assert len(RM.residues(runs, ("cert",))) == 256  # the certificate path on its own
    assert len(RM.residues(runs, ("grant",))) == 256  # and the 16-lane path


# 4. read back with google.protobuf ----------------------------------------------------
@pytest.mark.parametrize("name", ["refused_mixed", "stored_shared", "ok_64_ops", "cert_alias", "ok_empty_ids", "cert_lens"])
def test_bodies_read_back_with_protobuf(own_cases, name):
    pytest.importorskip("google.protobuf")
    Reply, Grant = RM.classes()
    batch, issued, src = own_cases[name]
    wire, off, ln, st = mh.write1_reply_encode(batch, issued, src)
    strings = np.asarray(batch.strings, np.uint8)
    for q in range(batch.n_reqs):
        body = wire[int(off[q]):int(off[q]) + int(ln[q])].tobytes()
        if issued.req_kind[q] == mh.W1K_THROWS:
            assert body == b""
            continue
        m = Reply()
        m.ParseFromString(body)
        assert m.HasField("multiGrant") and m.clientId == "" and m.hash == ""
        mg = m.multiGrant
        assert mg.serverId.encode() == RM.SERVER_ID and mg.hash == ""
        assert mg.clientId.encode() == src.ids[int(src.req_client_off[q]):][:int(src.req_client_len[q])].tobytes()
        refs = issued.req_grant[int(issued.req_grant_off[q]):int(issued.req_grant_off[q + 1])].tolist()
        assert len(mg.grants) == len(refs) == len(mg.grantSignatures)
        want_certs = {}
        for r in refs:
            if r & mh.W1_STORED:
                i = r & ~mh.W1_STORED
                gb = src.stored_bytes[int(src.stored_off[i]):][:int(src.stored_len[i])].tobytes()
                sig = src.stored_sig.reshape(-1, 256)[i].tobytes()
            else:
                gb, sig = issued.grant(r), issued.sig[r].tobytes()
            g = Grant()
            g.ParseFromString(gb)
            assert mg.grants[g.objectId].SerializeToString() == gb  # canonical bytes: equal means byte-equal
            assert mg.grantSignatures[g.objectId] == sig
            op = next(o for o in range(int(batch.req_op_off[q]), int(batch.req_op_off[q + 1]))
                      if issued.op_grant[o] == r)
            assert strings[int(batch.op_key_off[op]):][:int(batch.op_key_len[op])].tobytes() == g.objectId.encode()
            cert = src.certs[int(src.op_cert_off[op]):][:int(src.op_cert_len[op])].tobytes()
            if cert:
                want_certs[g.objectId] = cert
        assert dict(m.currentCertificates) == want_certs


def test_empty_certificate_value_and_empty_multigrant_as_protobuf_writes_them():
    """The two layout facts the encoder relies on, from google.protobuf itself."""
    pytest.importorskip("google.protobuf")
    Reply, _ = RM.classes()
    m = Reply()
    m.multiGrant.SetInParent()
    assert m.SerializeToString() == b"\x0a\x00"
    m.currentCertificates["k"] = b""
    assert m.SerializeToString() == b"\x0a\x00" + bytes.fromhex("12050a016b1200")


# 5. capacity ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["refused_mixed", "cert_lens", "steps"])
def test_one_byte_short_is_refused_and_nothing_is_written(own_cases, name):
    batch, issued, src = own_cases[name]
    full, off, ln, st = mh.write1_reply_encode(batch, issued, src)
    wire = np.full(full.size - 1, 0xEE, np.uint8)
    rc, need, off2, ln2, st2 = mh.write1_reply_encode_into(batch, issued, src, wire)
    assert rc == mh.EINVAL and need == full.size and (wire == 0xEE).all()
    assert "wire_cap" in mh._err(mh.load_library())
    np.testing.assert_array_equal(off2, off)
    np.testing.assert_array_equal(ln2, ln)
    wire = np.full(full.size + 5, 0xEE, np.uint8)
    rc, need, *_ = mh.write1_reply_encode_into(batch, issued, src, wire)
    assert rc == mh.OK and wire[:need].tobytes() == full.tobytes() and (wire[need:] == 0xEE).all()


def test_too_long_body_gets_status_and_length_zero():
    """Six ops alias one 400 MiB certificate: the body would pass 2^31 bytes."""
    R, W = M.Request, M.WRITE
    big = 400 << 20
    reqs = [R(1, M.H(1), [(W, b"big%d" % i) for i in range(6)]), R(1, M.H(2), [(W, b"small")])]
    batch, issued, src = RM.from_requests(M._store({}), reqs, sigs=False, cert_of=lambda k: b"c")
    src.certs = np.zeros(big, np.uint8)
    src.op_cert_off = np.zeros(batch.n_ops, np.uint64)
    src.op_cert_len = np.array([big] * 6 + [3], np.uint32)
    rc, need, off, ln, st = mh.write1_reply_encode_into(batch, issued, src, None)
    assert st.tolist() == [mh.ENC_TOO_LONG, mh.ENC_OK] and ln[0] == 0 and 0 < ln[1] == need < 400
    assert mh.write1_reply_bound(batch, src, issued.grant_bytes_len, False) >= need


# 6. argument errors ------------------------------------------------------------------------
def _rc(batch, issued, src, mutate):
    """rc and error text of the host form after `mutate(b, o, s)` edited the C structs."""
    lib = mh.load_library()
    b, kb = batch.to_c()
    o, ko = mh._issued_c(issued)
    s, ks = src.to_c()
    Q = batch.n_reqs
    off, ln, st = np.zeros(Q + 1, np.uint64), np.zeros(Q + 1, np.uint32), np.zeros(Q + 1, np.uint8)
    wire = np.zeros(1 << 16, np.uint8)
    args = dict(wire=mh._ptr(wire), cap=wire.size, off=mh._ptr(off), ln=mh._ptr(ln), st=mh._ptr(st))
    keep = mutate(b, o, s, args)
    need = ctypes.c_uint64(0)
    rc = lib.mochi_write1_reply_encode(ctypes.addressof(b), ctypes.addressof(o), ctypes.addressof(s), args["wire"],
                                       args["cap"], args["off"], args["ln"], args["st"], ctypes.addressof(need))
    return rc, mh._err(lib)


def _arr(values, dt):
    return np.ascontiguousarray(np.array(values, dt))


ERRORS = {
    "req_op_off": (lambda b, o, s, a: [x := _arr([0, 1, 1], np.uint32), setattr(b, "req_op_off", mh._ptr(x))],
                   "req_op_off is not a CSR"),
    "req_grant_off": (lambda b, o, s, a: [x := _arr([0, 3, 2], np.uint32), setattr(o, "req_grant_off", mh._ptr(x))],
                      "req_grant_off is not a CSR"),
    "req_grant_off_long": (lambda b, o, s, a: [x := _arr([0, 1, 9], np.uint32), setattr(o, "req_grant_off", mh._ptr(x))],
                           "req_grant_off is not a CSR"),
    "req_kind": (lambda b, o, s, a: [x := _arr([0, 7], np.uint8), setattr(o, "req_kind", mh._ptr(x))],
                 "req_kind"),
    "ref_new": (lambda b, o, s, a: [x := _arr([0, 5, 0], np.uint32), setattr(o, "req_grant", mh._ptr(x))],
                "outside n_new"),
    "ref_stored": (lambda b, o, s, a: [x := _arr([0, mh.W1_STORED | 4, 0], np.uint32), setattr(o, "req_grant", mh._ptr(x))],
                   "outside n_stored"),
    "ref_unlisted": (lambda b, o, s, a: [x := _arr([mh.W1_STORED | 0, mh.W1_STORED | 0, 0], np.uint32),
                                         setattr(o, "req_grant", mh._ptr(x))],
                     "no listed op"),
    "server_id": (lambda b, o, s, a: setattr(s, "server_id_off", 1 << 40), "server id lies outside ids"),
    "client_id": (lambda b, o, s, a: [x := _arr([0, 1 << 40], np.uint64), setattr(s, "req_client_off", mh._ptr(x))],
                  "client id lies outside ids"),
    "key": (lambda b, o, s, a: [x := _arr([0, 1 << 40, 0], np.uint64), setattr(b, "op_key_off", mh._ptr(x))],
            "key lies outside strings"),
    "stored": (lambda b, o, s, a: [x := _arr([1 << 40], np.uint64), setattr(s, "stored_off", mh._ptr(x))],
               "stored grant lies outside stored_bytes"),
    "new_grant": (lambda b, o, s, a: [x := _arr([1 << 40, 0, 0], np.uint64), setattr(o, "grant_off", mh._ptr(x))],
                  "new grant lies outside grant_bytes"),
    "cert": (lambda b, o, s, a: [x := _arr([7, 7, 7], np.uint32), setattr(s, "certs_len", 3),
                                  setattr(s, "op_cert_len", mh._ptr(x))], "certificate lies outside certs"),
    "stored_sig": (lambda b, o, s, a: setattr(s, "stored_sig", None), "stored_sig is required"),
    "cert_pair": (lambda b, o, s, a: setattr(s, "op_cert_len", None), "op_cert_off and op_cert_len go together"),
    "client_pair": (lambda b, o, s, a: setattr(s, "req_client_len", None), "req_client_off and req_client_len go together"),
    "wire": (lambda b, o, s, a: a.update(wire=None), "wire required"),
    "outputs": (lambda b, o, s, a: a.update(ln=None), "msg_off / msg_len / status required"),
    "n_new": (lambda b, o, s, a: setattr(o, "n_new", 99), "n_new exceeds n_ops"),
}


@pytest.mark.parametrize("name", sorted(ERRORS))
def test_argument_errors_come_with_text(own_cases, name):
    batch, issued, src = own_cases["refused_mixed"]  # Q = 2, O = 3, S = 1, n_new = 1; entries [new 0 | stored 0, new 0]
    assert (batch.n_reqs, batch.n_ops, batch.n_stored, issued.n_new) == (2, 3, 1, 1)
    rc, text = _rc(batch, issued, src, lambda b, o, s, a: None)
    assert rc == mh.OK
    mutate, want = ERRORS[name]
    rc, text = _rc(batch, issued, src, mutate)
    assert rc == mh.EINVAL and want in text, text


def test_null_arguments():
    lib = mh.load_library()
    need = ctypes.c_uint64(0)
    assert lib.mochi_write1_reply_encode(None, None, None, None, 0, None, None, None, ctypes.addressof(need)) == mh.EINVAL
    assert "null argument" in mh._err(lib)
    assert lib.mochi_write1_reply_encode(None, None, None, None, 0, None, None, None, None) == mh.EINVAL
    assert "wire_len required" in mh._err(lib)
