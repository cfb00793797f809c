"""Write2ToServer encoder, host form (mochi_write2_encode): byte-exact with
workload.py's Python encoders, readable by an independent protobuf
implementation and by the oracle decoder, with per-message statuses, the
capacity rule, and the alignment set the device copy kernel is checked on."""
import ctypes
import os
import sys

import numpy as np
import pytest

import mochi_hip as mh
import oracle_ffi as O
import w2_encode_cases as C
import workload as W


@pytest.fixture(scope="module")
def sources():
    return C.byte_exact_sources()


def _pack(msgs):
    ln = np.array([len(m) for m in msgs], np.uint32)
    off = np.zeros(len(msgs), np.uint64)
    if len(msgs) > 1:
        np.cumsum(ln[:-1], out=off[1:])
    return np.frombuffer(b"".join(msgs), np.uint8), off, ln


def _wire_batch(wire, off, ln, n_ops=None):
    return W.WireBatch(wire=wire if wire.size else np.zeros(1, np.uint8), msg_off=off, msg_len=ln, op_flags_off=None,
                       op_flags=np.zeros(1, np.uint8), expected_hash=np.zeros((len(off), 128), np.uint8))


# 1. byte-exact --------------------------------------------------------------
@pytest.mark.parametrize("name", ["r4", "r7k2", "client", "nosig", "hand", "hand_nosig", "steps", "steps_nosig",
                                  "wc16383", "wc16384", "msg16383", "msg16384"])
def test_host_form_is_byte_exact_with_the_python_encoders(sources, name):
    src = sources[name]
    wire, off, ln, st = mh.encode_write2(src, C.IDS)
    ref = C.py_encode(src)
    ewire, eoff, eln = _pack([m for m, _, _, _ in ref])
    assert (st == 0).all()
    np.testing.assert_array_equal(ln, eln)
    np.testing.assert_array_equal(off, eoff)
    assert wire.tobytes() == ewire.tobytes()
    assert mh.write2_encode_bound(src, max(len(x) for x in C.IDS)) >= wire.size


@pytest.mark.parametrize("name,R,k,cid", [("r4", 4, 1, ""), ("r7k2", 7, 2, ""), ("client", 4, 1, "client-7f3a")])
def test_workload_source_gives_encode_wire_batch(sources, name, R, k, cid):
    """write2_source(s) is the source of exactly encode_wire_batch(s)'s messages."""
    wb = W.encode_wire_batch(C.synth(R, k), client_id=cid)
    wire, off, ln, st = mh.encode_write2(sources[name], C.IDS)
    np.testing.assert_array_equal(ln, wb.msg_len)
    np.testing.assert_array_equal(off, wb.msg_off)
    assert wire.tobytes() == wb.wire[:wire.size].tobytes() and wire.size == int(wb.msg_len.sum())


def test_varint_steps_are_covered(sources):
    """The sources above put lengths on both sides of every varint step."""
    e1, mgl = set(), set()
    for name in ("steps", "steps_nosig"):
        for _, _, mg_lens, e1_lens in C.py_encode(sources[name]):
            e1.update(e1_lens)
            mgl.update(mg_lens)
    assert {127, 128} <= e1 and {127, 128} <= mgl
    for t in (16383, 16384):
        m, wc, mg_lens, _ = C.py_encode(sources[f"wc{t}"])[0]
        assert wc == t and len(mg_lens) == 7
        assert len(C.py_encode(sources[f"msg{t}"])[0][0]) == t
    hand = C.py_encode(sources["hand"])
    assert len(hand[4][0]) == 0 and b"\x0a\x00" in hand[3][0]  # the empty message; the key of an empty objectId


# 2. an independent protobuf implementation -----------------------------------
@pytest.mark.parametrize("name", ["r4", "r7k2", "client", "hand"])
def test_google_protobuf_reads_the_source_back(sources, name):
    pytest.importorskip("google.protobuf")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_write2_golden as G

    Write2, Grant = G.classes()
    src = sources[name]
    wire, off, ln, st = mh.encode_write2(src, C.IDS)
    blob, strs = src.grant_bytes.tobytes(), src.strings.tobytes()
    for m in range(src.n_msgs):
        msg = Write2()
        msg.ParseFromString(wire[int(off[m]):int(off[m]) + int(ln[m])].tobytes())
        cid = "" if src.client_off is None else strs[int(src.client_off[m]):int(src.client_off[m]) + int(src.client_len[m])].decode()
        i0, i1 = int(src.cert_mg_off[m]), int(src.cert_mg_off[m + 1])
        assert sorted(msg.writeCertificate.grants) == sorted({C.IDS[int(src.mg_signer[i])] for i in range(i0, i1)})
        for i in range(i0, i1):
            sid = C.IDS[int(src.mg_signer[i])]
            mg = msg.writeCertificate.grants[sid]
            assert mg.serverId == sid and mg.clientId == cid and mg.hash == ""
            want_g, want_s = {}, {}
            for g in range(int(src.mg_grant_off[i]), int(src.mg_grant_off[i + 1])):
                gb = blob[int(src.grant_off[g]):int(src.grant_off[g]) + int(src.grant_len[g])]
                want_g[W.grant_object_id(gb)] = gb
                want_s[W.grant_object_id(gb)] = src.sig[g].tobytes()
            assert {k: v.SerializeToString() for k, v in mg.grants.items()} == want_g
            assert dict(mg.grantSignatures) == want_s
        o0, o1 = int(src.cert_op_off[m]), int(src.cert_op_off[m + 1])
        assert len(msg.transaction.operations) == o1 - o0
        for o, op in zip(range(o0, o1), msg.transaction.operations):
            assert op.action == int(src.op_action[o])
            assert op.operand1.encode() == strs[int(src.op1_off[o]):int(src.op1_off[o]) + int(src.op1_len[o])]
            assert op.operand2.encode() == strs[int(src.op2_off[o]):int(src.op2_off[o]) + int(src.op2_len[o])]


# 3. round trip through the oracle decoder --------------------------------------
@pytest.mark.parametrize("name,R", [("r4", 4), ("r7k2", 7), ("client", 4)])
def test_oracle_decoder_round_trip(sources, name, R):
    src = sources[name]
    wire, off, ln, st = mh.encode_write2(src, C.IDS)
    ids, id_off = W.server_id_table(R)
    d = O.w2_decode(_wire_batch(wire, off, ln), ids, id_off)
    assert (d["msg_status"] == 0).all()
    np.testing.assert_array_equal(d["sig"], src.sig)
    np.testing.assert_array_equal(d["grant_len"], src.grant_len)
    np.testing.assert_array_equal(d["mg_grant_off"], src.mg_grant_off)
    np.testing.assert_array_equal(d["cert_mg_off"], src.cert_mg_off)
    np.testing.assert_array_equal(d["cert_op_off"], src.cert_op_off)
    np.testing.assert_array_equal(d["cert_grant_off"], src.mg_grant_off[src.cert_mg_off])
    np.testing.assert_array_equal(d["signer"], np.repeat(src.mg_signer, np.diff(src.mg_grant_off.astype(np.int64))))
    for g in range(src.n_grants):
        a = wire[int(d["grant_off"][g]):int(d["grant_off"][g]) + int(d["grant_len"][g])]
        e = src.grant_bytes[int(src.grant_off[g]):int(src.grant_off[g]) + int(src.grant_len[g])]
        assert a.tobytes() == e.tobytes()
    np.testing.assert_array_equal(d["op_key_len"], src.op1_len)
    for o in range(src.n_ops):
        a = wire[int(d["op_key_off"][o]):int(d["op_key_off"][o]) + int(d["op_key_len"][o])]
        e = src.strings[int(src.op1_off[o]):int(src.op1_off[o]) + int(src.op1_len[o])]
        assert a.tobytes() == e.tobytes()


# 4. statuses ----------------------------------------------------------------
def test_bad_messages_are_emitted_empty_and_neighbours_unchanged():
    src, want = C.bad_source()
    wire, off, ln, st = mh.encode_write2(src, C.IDS)
    np.testing.assert_array_equal(st, want)
    ref = dict(zip((0, 2, 4, 6), C.py_encode(src, only=(0, 2, 4, 6))))  # the sound messages, each on its own
    pos = 0
    for m in range(7):
        assert int(off[m]) == pos
        if want[m]:
            assert ln[m] == 0
            continue
        assert wire[pos:pos + int(ln[m])].tobytes() == ref[m][0]
        pos += int(ln[m])
    assert pos == wire.size
    assert mh.write2_encode_bound(src, max(len(x) for x in C.IDS)) >= wire.size


def test_grant_mutants_against_the_oracle():
    """One message per mutant of the grant corpus: BAD_GRANT exactly where the oracle's Grant
    parser refuses the bytes, and otherwise the Python encoder's message keyed by the
    objectId the oracle read."""
    grants = C.grant_mutants()
    src = C.mutant_source()
    assert src.n_msgs == len(grants) > 3000
    wire, off, ln, st = mh.encode_write2(src, C.IDS)
    parsed = [O.grant_parse(gb) for gb in grants]
    np.testing.assert_array_equal(st, [mh.ENC_BAD_GRANT if p is None else mh.ENC_OK for p in parsed])
    assert 1000 < sum(p is not None for p in parsed) < len(grants) - 1000
    op = W.encode_operation(2, "k", "v")
    pos = 0
    for m, (gb, p) in enumerate(zip(grants, parsed)):
        assert int(off[m]) == pos
        if p is None:
            assert ln[m] == 0
            continue
        oid = p["object_id"].decode()
        mg = W.encode_multigrant([(oid, gb)], C.IDS[0], "", "", [(oid, src.sig[m].tobytes())])
        want = W.encode_write2([(C.IDS[0], mg)], [op])
        assert wire[pos:pos + int(ln[m])].tobytes() == want, m
        pos += int(ln[m])
    assert pos == wire.size


def test_inconsistent_source_is_refused():
    src = C.hand_source()
    src.cert_mg_off = src.cert_mg_off.copy()
    src.cert_mg_off[-1] -= 1
    rc, need, *_ = mh.encode_write2_into(src, C.IDS, None)
    assert rc == mh.EINVAL and need == 0
    src = C.hand_source()
    src.op1_off = src.op1_off.copy()
    src.op1_off[0] = src.strings.size
    rc, need, *_ = mh.encode_write2_into(src, C.IDS, None)
    assert rc == mh.EINVAL and need == 0


# 5. capacity ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["r4", "hand"])
def test_capacity_rule(sources, name):
    src = sources[name]
    wire, off, ln, st = mh.encode_write2(src, C.IDS)
    need = wire.size
    buf = np.full(need - 1, 0xEE, np.uint8)
    rc, n, off2, ln2, st2 = mh.encode_write2_into(src, C.IDS, buf)
    assert rc == mh.EINVAL and n == need and (buf == 0xEE).all()
    np.testing.assert_array_equal(off2, off)
    np.testing.assert_array_equal(ln2, ln)
    buf = np.full(need + 64, 0xEE, np.uint8)
    rc, n, *_ = mh.encode_write2_into(src, C.IDS, buf)
    assert rc == mh.OK and n == need
    assert buf[:need].tobytes() == wire.tobytes() and (buf[need:] == 0xEE).all()


def test_no_messages():
    src = C.head(C.hand_source(), 0)
    rc, n, off, ln, st = mh.encode_write2_into(src, C.IDS, None)
    assert rc == mh.OK and n == 0 and off.size == 0
    assert mh.write2_encode_bound(src, 24) == 0


def test_bound_reads_counts_only():
    c = mh.Write2Source_C()
    c.n_msgs, c.n_mgs, c.n_grants, c.n_ops, c.grant_bytes_len, c.strings_len = 3, 12, 12, 3, 2000, 100
    lib = mh.load_library()
    b = lib.mochi_write2_encode_bound(ctypes.addressof(c), 24)  # every pointer NULL
    assert 12 * (3 * 2000 + 256) < b <= 3 * (2 ** 31 - 1)
    c.grant_bytes_len = 2 ** 40
    assert lib.mochi_write2_encode_bound(ctypes.addressof(c), 24) == 3 * (2 ** 31 - 1)


# 6. the alignment set of the device copy kernel --------------------------------
def test_alignment_set_covers_every_case():
    src = C.align_source()
    wire, off, ln, st = mh.encode_write2(src, C.IDS)
    assert (st == 0).all() and src.n_msgs == 1024
    assert wire.tobytes() == _pack([m for m, _, _, _ in C.py_encode(src)])[0].tobytes()
    grants, sigs = C.payload_offsets(wire, off, ln)
    assert len(grants) == len(sigs) == src.n_grants == 4096
    assert [n for _, n in grants] == src.grant_len.tolist()
    # device buffers are aligned to 16 bytes and more, so offsets decide the alignment there
    pairs = {(int(src.grant_off[g]) % 16, grants[g][0] % 16) for g in range(4096) if src.grant_len[g]}
    assert len(pairs) == 256
    assert {o % 16 for o in sigs} == set(range(16))
    assert {int(n) % 16 for n in src.grant_len} == set(range(16))
    assert (src.grant_len < 16).sum() >= 8 and (src.grant_len > 128).any()
