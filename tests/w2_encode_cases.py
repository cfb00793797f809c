"""Inputs of the Write2ToServer encoder tests (test_write2_encode_cpu.py and
test_write2_encode_gpu.py): the sources, a Python restatement of the encoder on
top of workload.py's byte yardsticks, and a walker that finds where the grant
bytes and signatures of an encoded message lie."""
from __future__ import annotations

import functools

import numpy as np

import mochi_hip as mh
import workload as W

IDS = W.SERVER_IDS  # 7 ids; a context over R keys takes IDS[:R]
TH = "ab" * 64


def source(msgs, blob_pad=None, sigs=True, client_ids=None, seed=5):
    """Hand-built source.  msgs = [(multigrants, operations)], multigrants =
    [(signer, [grant bytes, ...])], operations = [(action, operand1, operand2)]
    (operands bytes).  blob_pad(g) = filler bytes in front of grant g in the blob."""
    rng = np.random.default_rng(seed)
    blob, goff, glen, cmo, mgo, sgn, coo = [], [], [], [0], [0], [], [0]
    strs, act, o1, l1, o2, l2, co, cl = [], [], [], [], [], [], [], []
    pos = spos = 0

    def put(b):
        nonlocal spos
        strs.append(b)
        spos += len(b)
        return spos - len(b)

    for m, (mgs, ops) in enumerate(msgs):
        for signer, grants in mgs:
            sgn.append(signer)
            for gb in grants:
                pad = blob_pad(len(goff)) if blob_pad else 0
                blob.append(b"\xee" * pad + gb)
                goff.append(pos + pad)
                glen.append(len(gb))
                pos += pad + len(gb)
            mgo.append(len(goff))
        cmo.append(len(sgn))
        for a, x, y in ops:
            act.append(a)
            l1.append(len(x)); o1.append(put(x))
            l2.append(len(y)); o2.append(put(y))
        coo.append(len(act))
        if client_ids is not None:
            cl.append(len(client_ids[m])); co.append(put(client_ids[m]))
    n = len(goff)
    return mh.Write2Source(
        grant_bytes=np.frombuffer(b"".join(blob) or b"\x00", np.uint8).copy(), grant_off=np.array(goff, np.uint64),
        grant_len=np.array(glen, np.uint32),
        sig=rng.integers(0, 256, (n, 256), dtype=np.uint8) if sigs else None,
        cert_mg_off=np.array(cmo, np.uint32), mg_grant_off=np.array(mgo, np.uint32), mg_signer=np.array(sgn, np.uint16),
        strings=np.frombuffer(b"".join(strs) or b"\x00", np.uint8).copy(), cert_op_off=np.array(coo, np.uint32),
        op_action=np.array(act, np.uint8), op1_off=np.array(o1, np.uint64), op1_len=np.array(l1, np.uint32),
        op2_off=np.array(o2, np.uint64), op2_len=np.array(l2, np.uint32),
        client_off=None if client_ids is None else np.array(co, np.uint64),
        client_len=None if client_ids is None else np.array(cl, np.uint32))


def head(src, m):
    """The first m messages of a source (blobs shared)."""
    nm, no = int(src.cert_mg_off[m]), int(src.cert_op_off[m])
    n = int(src.mg_grant_off[nm])
    cut = lambda a, k: None if a is None else a[:k]
    return mh.Write2Source(
        grant_bytes=src.grant_bytes, grant_off=src.grant_off[:n], grant_len=src.grant_len[:n], sig=cut(src.sig, n),
        cert_mg_off=src.cert_mg_off[:m + 1], mg_grant_off=src.mg_grant_off[:nm + 1], mg_signer=src.mg_signer[:nm],
        strings=src.strings, cert_op_off=src.cert_op_off[:m + 1], op_action=src.op_action[:no],
        op1_off=src.op1_off[:no], op1_len=src.op1_len[:no], op2_off=cut(src.op2_off, no), op2_len=cut(src.op2_len, no),
        client_off=cut(src.client_off, m), client_len=cut(src.client_len, m))


def py_encode(src, ids=IDS, only=None):
    """The messages of a source (or those listed in `only`) through workload.py's encoders, one by one:
    [(bytes, WriteCertificate length, [MultiGrant lengths], [grants-entry body lengths])]."""
    blob, strs = src.grant_bytes.tobytes(), src.strings.tobytes()
    sl = lambda off, ln, i: strs[int(off[i]):int(off[i]) + int(ln[i])].decode()
    out = []
    for m in (range(src.n_msgs) if only is None else only):
        cid = "" if src.client_off is None else sl(src.client_off, src.client_len, m)
        enc, mg_lens, e1 = [], [], []
        for i in range(int(src.cert_mg_off[m]), int(src.cert_mg_off[m + 1])):
            items = []
            for g in range(int(src.mg_grant_off[i]), int(src.mg_grant_off[i + 1])):
                gb = blob[int(src.grant_off[g]):int(src.grant_off[g]) + int(src.grant_len[g])]
                oid = W.grant_object_id(gb)
                items.append((oid, gb, None if src.sig is None else src.sig[g].tobytes()))
                e1.append(len(W._ld(1, oid.encode()) + W._ld(2, gb)))
            sid = ids[int(src.mg_signer[i])]
            mg = W.encode_multigrant([(o, gb) for o, gb, _ in items], sid, cid, "",
                                     None if src.sig is None else [(o, sg) for o, _, sg in items])
            mg_lens.append(len(mg))
            enc.append((sid, mg))
        ops = [W.encode_operation(int(src.op_action[o]), sl(src.op1_off, src.op1_len, o),
                                  "" if src.op2_off is None else sl(src.op2_off, src.op2_len, o))
               for o in range(int(src.cert_op_off[m]), int(src.cert_op_off[m + 1]))]
        wc = sum(len(W.encode_map_entry(1, sid.encode(), mg)) for sid, mg in enc)
        out.append((W.encode_write2(enc, ops), wc, mg_lens, e1))
    return out


def _varint(b, i):
    v = s = 0
    while True:
        c = b[i]
        i += 1
        v |= (c & 0x7F) << s
        s += 7
        if not c & 0x80:
            return v, i


def _fields(b, lo, hi):
    """(field, value offset, value length) of the length-delimited fields of b[lo:hi]; varints skipped."""
    i = lo
    while i < hi:
        tag, i = _varint(b, i)
        if tag & 7 == 0:
            _, i = _varint(b, i)
            continue
        assert tag & 7 == 2
        n, i = _varint(b, i)
        yield tag >> 3, i, n
        i += n


def payload_offsets(wire, msg_off, msg_len):
    """Wire offsets of every grant value [(offset, length)] and every signature
    value [offset], in wire order (a protobuf walk of each message)."""
    b = wire.tobytes()
    grants, sigs = [], []
    for m in range(len(msg_off)):
        lo = int(msg_off[m])
        for f, o, n in _fields(b, lo, lo + int(msg_len[m])):
            if f != 1:
                continue
            for _, eo, en in _fields(b, o, o + n):  # certificate entries
                for f2, vo, vn in _fields(b, eo, eo + en):
                    if f2 != 2:
                        continue
                    for f3, xo, xn in _fields(b, vo, vo + vn):  # MultiGrant fields
                        if f3 not in (1, 5):
                            continue
                        for f4, yo, yn in _fields(b, xo, xo + xn):
                            if f4 == 2:
                                (grants if f3 == 1 else sigs).append((yo, yn))
    return grants, [o for o, _ in sigs]


@functools.lru_cache(maxsize=None)
def pool(R, k):
    return W.build_pool(R=R, k=k, P=64 if k == 1 else 32, P_f=32 if k == 1 else 16)


@functools.lru_cache(maxsize=None)
def synth(R, k):
    """96 certificates of the seeded stream, faults included (a dropped replica among them)."""
    s = W.make_batch(pool(R, k), 96, first_cert=9000)
    assert (s.fault != W.FAULT_NONE).any()
    return s


def g(oid, ts=1234, th=TH):
    return W.encode_grant(oid, ts, th)


def hand_source(sigs=True):
    A, B = "DEMO_KEY_A", "DEMO_KEY_B"
    op = lambda k, v=b"val": (2, k.encode(), v)
    msgs = [
        ([], [op(A)]),                                            # no MultiGrant
        ([(0, [g(A)]), (1, [g(A, 1235)])], []),                   # no operation
        ([(2, []), (0, [g(A), g(B)])], [(0, b"", b""), op(B)]),   # an empty MultiGrant; action 0, empty operands
        ([(3, [g(""), g(A)])], [(1, A.encode(), b""), (200, b"", b"x")]),  # empty objectId; two-byte action
        ([], []),                                                 # an empty message
        ([(1, [b""]), (6, [g(B)])], [op(B, b"")]),                # an empty grant; the last id of the table
    ]
    return source(msgs, sigs=sigs, client_ids=[b"", b"c", b"", b"client-7f3a", b"", b""])


def step_source(sigs):
    """One single-grant MultiGrant per message, objectId and transactionHash
    lengths swept so that the grants-entry and MultiGrant lengths pass 127 / 128."""
    msgs = []
    for ol in (1, 9, 30):
        for hl in range(0, 129):
            msgs.append(([(hl % 4, [g("K" * ol, 77, "h" * hl)])], [(2, b"K" * ol, b"v")]))
    return source(msgs, sigs=sigs)


def big_source(target, what):
    """R = 7 with six grants per MultiGrant, tuned so that the WriteCertificate
    (what = "wc") or the whole message (what = "msg") is `target` bytes long."""
    R, K = 7, 6

    def build(l0, tune, v2):
        mgs, t = [], list(tune)
        for r in range(R):
            gs = []
            for j in range(K):
                hl = t.pop() if (r == 0 and t) else l0
                gs.append(g(f"OBJ_{j:06d}", 1000 + r, "h" * hl))
            mgs.append((r, gs))
        return source([(mgs, [(2, b"OBJ_000000", b"v" * v2)])])

    def lens(src):
        m, wc, _, _ = py_encode(src)[0]
        return len(m), wc

    for l0 in range(20, 129):
        _, w0 = lens(build(l0, [112, 112, 112], 300))
        d = target - w0 - (0 if what == "wc" else 340)
        if not 0 <= d <= 45:
            continue
        tune = [112 + min(15, max(0, d - 15 * i)) for i in range(3)]
        src = build(l0, tune, 300)
        n, wc = lens(src)
        if what == "wc":
            assert wc == target
            return src
        src = build(l0, tune, 300 + target - n)
        assert lens(src)[0] == target
        return src
    raise AssertionError("no tuning reaches the target")


@functools.lru_cache(maxsize=None)
def align_source():
    """4096 single-grant MultiGrants, four per message (1024 messages), for the
    payload copy: random objectId lengths 1-40, transactionHash lengths 0-128,
    0-15 filler bytes in front of each grant in the blob."""
    rng = np.random.default_rng(20260)
    n = 4096
    ol, hl, pad = rng.integers(1, 41, n), rng.integers(0, 129, n), rng.integers(0, 16, n)
    hl[rng.random(n) < 0.1] = 0
    ts = np.where(rng.random(n) < 0.3, 0, rng.integers(1, 1 << 20, n))  # timestamp 0: grants under 16 bytes
    grants = [W.encode_grant("k" * int(ol[i]), int(ts[i]), "f" * int(hl[i])) for i in range(n)]
    msgs = [([(int(rng.integers(0, 4)), [grants[4 * m + j]]) for j in range(4)], [(2, b"k", b"v")])
            for m in range(n // 4)]
    return source(msgs, blob_pad=lambda i: int(pad[i]))


def bad_source():
    """Message 1 holds an unparseable grant, message 3 a signer outside the
    table, message 5 both; the even messages are sound."""
    ok = lambda r: (r, [g("DEMO_KEY_A", 1000 + r)])
    trunc = g("DEMO_KEY_A")[:-3]  # transactionHash runs past the end
    utf8 = W.encode_grant("A", 5, "x") [:-1] + b"\xff"  # not UTF-8
    msgs = [([ok(0), ok(1)], [(2, b"DEMO_KEY_A", b"v0")]),
            ([ok(0), (1, [g("DEMO_KEY_A"), trunc])], [(2, b"DEMO_KEY_A", b"v1")]),
            ([ok(2), ok(3)], [(2, b"DEMO_KEY_A", b"v2")]),
            ([ok(0), (9, [g("DEMO_KEY_A")])], [(2, b"DEMO_KEY_A", b"v3")]),
            ([ok(1)], [(2, b"DEMO_KEY_A", b"v4")]),
            ([(0xFFFF, [utf8])], []),
            ([ok(3)], [])]
    return source(msgs), [0, mh.ENC_BAD_GRANT, 0, mh.ENC_BAD_SIGNER, 0, mh.ENC_BAD_GRANT, 0]


def _groups(depth):
    """An unknown group (field 9) nested `depth` deep."""
    return b"\x4b" * depth + b"\x4c" * depth


@functools.lru_cache(maxsize=None)
def grant_mutants():
    """The grant mutation corpus: every truncation and every single-bit flip of three
    grants -- the demo grant; one with multi-byte UTF-8, all five fields, fixed32 /
    fixed64 unknowns and a second objectId; one with unknown groups nested 1, 15, 16 and
    17 deep (the device parser's register stack holds 16) -- and, unmutated, groups
    nested 99, 100 and 101 deep (the recursion limit is 100)."""
    grants = [
        W.encode_grant("DEMO_KEY_1", 1342, "a" * 128),
        W.encode_grant("kéy-€-\U0001f511", 1700000000000, "häsh" + "b" * 27, configstamp=7, status=1) +
        b"\x4d\x01\x02\x03\x04" + b"\x49\x01\x02\x03\x04\x05\x06\x07\x08" + W._ld(1, b"second"),
        W._ld(1, b"grp") + _groups(1) + _groups(15) + _groups(16) + _groups(17) + b"\x10\x05",
    ]
    out = []
    for b in grants:
        out += [b[:n] for n in range(len(b) + 1)]
        out += [b[:i] + bytes([b[i] ^ (1 << bit)]) + b[i + 1:] for i in range(len(b)) for bit in range(8)]
    out += [W._ld(1, b"deep") + _groups(d) for d in (99, 100, 101)]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def mutant_source():
    """One message per grant mutant: one MultiGrant of that one grant, signer 0, one operation."""
    return source([([(0, [gb])], [(2, b"k", b"v")]) for gb in grant_mutants()])


def byte_exact_sources():
    """name -> source, for the cases the host form must match workload.py byte for byte."""
    s4, s7 = synth(4, 1), synth(7, 2)
    nosig = W.write2_source(s4)
    nosig.sig = None
    return {
        "r4": W.write2_source(s4), "r7k2": W.write2_source(s7), "client": W.write2_source(s4, "client-7f3a"),
        "nosig": nosig, "hand": hand_source(), "hand_nosig": hand_source(False), "steps": step_source(True),
        "steps_nosig": step_source(False), "wc16383": big_source(16383, "wc"), "wc16384": big_source(16384, "wc"),
        "msg16383": big_source(16383, "msg"), "msg16384": big_source(16384, "msg"),
    }


def device_sources():
    """Every source the device form is compared with the host form on."""
    d = dict(byte_exact_sources())
    a = align_source()
    d.update(bad=bad_source()[0], align1024=a, align1023=head(a, 1023), one=head(a, 1), none=head(a, 0),
             mutants=mutant_source(), mutants1023=head(mutant_source(), 1023))
    return d
