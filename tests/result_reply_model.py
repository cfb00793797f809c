"""The yardstick for the result reply decoder (mochi_result_reply_decode[_device]) and the
coalescing step (mochi_result_coalesce[_device]): a plain-Python encoder and decoder of
Write2AnsFromServer / ReadFromServer / TransactionResult / OperationResult with
protobuf-java 3.16.3 parsing semantics, written from the .proto and MochiDBClient.java;
the google.protobuf classes it is cross-checked against; and the case sets the CPU and the
GPU tests share.

TEST INFRASTRUCTURE: the library is never its own reference here.  The decoder parses a
body into a tree of fields first (write1_decode_model.fields) and reads the messages off
that tree; certificates are validated by write1_decode_model.parse_writecert.  It shares
no code and no structure with the library's level-by-level walk.
"""
from __future__ import annotations

import functools
from typing import List, NamedTuple, Optional, Tuple

import numpy as np

import client_model as CM
import mochi_hip as mh
import write1_decode_model as DM
import write1_reply_model as RM

Malformed = DM.Malformed
MAX_OPS = 64
U64 = 2 ** 64 - 1
WRONG_SHARD = 1
W2, RD, OTHER = mh.RR_WRITE2_ANS, mh.RR_READ, mh.RR_OTHER
FILL = 0xA5  # what the tests prefill every output with


# ---------------------------------------------------------------------------
# encoder (proto3: defaults omitted, fields in number order; `raw` is appended as it is)
# ---------------------------------------------------------------------------
def op_result(status: int = 0, result: bytes = b"", existed: bool = False, cert: Optional[bytes] = None,
              raw: bytes = b"") -> bytes:
    out = RM.ld(0x0A, result) if result else b""
    if cert is not None:
        out += RM.ld(0x12, cert)
    if existed:
        out += b"\x18\x01"
    if status:
        out += b"\x20" + RM.varint(status & U64)
    return out + raw


def tx_result(ops, raw: bytes = b"") -> bytes:
    return b"".join(RM.ld(0x0A, o) for o in ops) + raw


def answer(kind: int, ops=None, rid: bytes = b"", nonce: bytes = b"", raw: bytes = b"") -> bytes:
    """ops: encoded OperationResults, or None for an answer without `result`."""
    out = RM.ld(0x0A, tx_result(ops)) if ops is not None else b""
    if kind == RD:
        out += (RM.ld(0x12, nonce) if nonce else b"") + (RM.ld(0x1A, rid) if rid else b"")
    else:
        out += RM.ld(0x12, rid) if rid else b""
    return out + raw


def encode(kind: int, results, rid: bytes = b"rid-1", nonce: bytes = b"") -> bytes:
    """results: [(status, result, existed, certificate bytes or None)] per operation."""
    return answer(kind, [op_result(s, r, e, c) for s, r, e, c in results], rid, nonce)


# ---------------------------------------------------------------------------
# decoder
# ---------------------------------------------------------------------------
class OpV(NamedTuple):
    status: int  # the int32 the enum field holds
    existed: bool
    n_cert: int
    result: Tuple[int, int]  # (offset in the body, length); absent: the operation's own offset, 0
    cert: Tuple[int, int]


class Body(NamedTuple):
    status: int
    n_ops: int = mh.RR_UNDECODED  # the wire count
    rid: Optional[Tuple[int, int]] = None  # None: absent
    nonce: Optional[Tuple[int, int]] = None
    ops: tuple = ()


def _op(b: bytes, off: int, n: int) -> OpV:
    status, existed, n_cert, result, cert = 0, False, 0, (off, 0), (off, 0)
    for f, wt, v, po, pl in DM._msg(b, off, n):
        if f == 1 and wt == 2:
            DM._utf8(b, po, pl)
            result = (po, pl)
        elif f == 2 and wt == 2:
            DM.parse_writecert(b, po, pl)  # every occurrence is parsed (a merge)
            cert = (po, pl)
            n_cert += 1
        elif f == 3 and wt == 0:
            existed = v != 0  # readBool: readRawVarint64() != 0
        elif f == 4 and wt == 0:
            status = DM._s32(v)  # readEnum: readRawVarint32
    return OpV(status, existed, n_cert, result, cert)


def decode_body(b: bytes, kind: int, n_ops: int) -> Body:
    """n_ops: the transaction's count (an operation past it may carry anything that parses)."""
    if kind == OTHER:
        return Body(mh.RRS_OK, 0)  # getWrite2AnsFromServer() of another payload: the default message
    try:
        results, rid, nonce = [], None, None
        for f, wt, v, po, pl in DM._msg(b, 0, len(b)):
            if wt != 2:
                continue
            if f == 1:
                results.append([_op(b, eo, el) for ef, ewt, _, eo, el in DM._msg(b, po, pl) if ef == 1 and ewt == 2])
            elif f == 2:
                DM._utf8(b, po, pl)
                if kind == RD:
                    nonce = (po, pl)
                else:
                    rid = (po, pl)
            elif f == 3 and kind == RD:
                DM._utf8(b, po, pl)
                rid = (po, pl)
    except Malformed:
        return Body(mh.RRS_MALFORMED)
    if len(results) > 1:
        return Body(mh.RRS_FALLBACK)
    ops = results[0] if results else []
    # above MAX_OPS the count alone is reported: it equals no n_ops, so no value is read
    if len(ops) <= MAX_OPS and any(o.n_cert > 1 for o in ops[:n_ops]):
        return Body(mh.RRS_FALLBACK)
    return Body(mh.RRS_OK, len(ops), rid, nonce, tuple(ops))


def status_u8(s: int) -> int:
    return s if 0 <= s < 255 else 0xFF


ABSENT = dict(op_status=0xFF, op_existed=0, op_flags=0, op_result_off=0, op_result_len=0, op_cert_off=0, op_cert_len=0)


def requests_of(r: "mh.ResultReplies"):
    """[(q, n_ops[q], [p, ...])]."""
    off = np.asarray(r.req_resp_off).tolist()
    return [(q, int(r.n_ops[q]), list(range(off[q], off[q + 1]))) for q in range(r.n_reqs)]


def bodies_of(r: "mh.ResultReplies") -> List[Body]:
    wire = np.asarray(r.wire, np.uint8).tobytes()
    out: List[Optional[Body]] = [None] * r.n_resps
    for q, k, ps in requests_of(r):
        for p in ps:
            o, n = int(r.resp_off[p]), int(r.resp_len[p])
            out[p] = decode_body(wire[o:o + n], int(r.resp_kind[p]), k)
    return out


def decode(r: "mh.ResultReplies", n_slots: Optional[int] = None, fill: int = FILL) -> dict:
    """The arrays of mochi_result_decoded for the batch, whole, over buffers prefilled with `fill`."""
    n = dict(P=r.n_resps, S=r.n_slots if n_slots is None else n_slots)
    arr = {k: np.full(n[w] * np.dtype(dt).itemsize, fill, np.uint8).view(dt) for k, (dt, w) in mh._RR_OUT.items()}
    bodies = bodies_of(r)
    for q, k, ps in requests_of(r):
        for p in ps:
            d, base, s0 = bodies[p], int(r.resp_off[p]), int(r.slot_off[p])
            given = d.status == mh.RRS_OK and int(r.resp_kind[p]) != OTHER
            arr["resp_status"][p] = d.status
            arr["resp_n_ops"][p] = d.n_ops
            for nm, sl in (("rid", d.rid), ("nonce", d.nonce)):
                arr["resp_%s_off" % nm][p] = (base + (sl[0] if sl else 0)) if given else 0
                arr["resp_%s_len" % nm][p] = sl[1] if given and sl else 0
            ops = d.ops if len(d.ops) <= MAX_OPS else ()
            for j in range(k):
                if j < len(ops):
                    o = ops[j]
                    vals = dict(op_status=status_u8(o.status), op_existed=int(o.existed),
                                op_flags=mh.RRO_HAS_CERT if o.n_cert else 0, op_result_off=base + o.result[0],
                                op_result_len=o.result[1], op_cert_off=base + o.cert[0], op_cert_len=o.cert[1])
                else:
                    vals = ABSENT
                for nm, v in vals.items():
                    arr[nm][s0 + j] = v
    return arr


def client(r: "mh.ResultReplies", R: int, out_off, n_out: int, fill: int = FILL):
    """What MochiDBClient does with the batch (client_model.tally over the model's decoded
    values, then the coalesced result): (accept[Q], reason[Q], the arrays of mochi_result_coalesced)."""
    bodies = bodies_of(r)
    arr = {k: np.full(n_out * np.dtype(dt).itemsize, fill, np.uint8).view(dt) for k, dt in mh._RC_OUT.items()}
    accept, reason = [], []
    for q, k, ps in requests_of(r):
        # a body the parser throws on, or one the decoder declines, is never an answer of k operations
        sts = [[status_u8(o.status) for o in bodies[p].ops] if bodies[p].status == mh.RRS_OK else [0] * (k + 1) for p in ps]
        why, chosen = CM.tally(sts, k, R)
        accept.append(why == 0)
        reason.append(why)
        for j in range(k):
            d = int(out_off[q]) + j
            if why or chosen[j] < 0:
                vals = dict(resp=0xFFFFFFFF, status=0xFF, existed=0, flags=0, result_off=0, result_len=0, cert_off=0, cert_len=0)
            else:
                p = ps[chosen[j]]
                o, base = bodies[p].ops[j], int(r.resp_off[p])
                vals = dict(resp=p, status=status_u8(o.status), existed=int(o.existed),
                            flags=mh.RRO_HAS_CERT if o.n_cert else 0, result_off=base + o.result[0],
                            result_len=o.result[1], cert_off=base + o.cert[0], cert_len=o.cert[1])
            for nm, v in vals.items():
                arr[nm][d] = v
    return np.array(accept, bool), np.array(reason, np.uint8), arr


def tally_host(r: "mh.ResultReplies", dec: dict, R: int, chosen_off, n_chosen: int):
    """mochi_tally_responses on the decoder's arrays: (chosen, reason, accept_bits)."""
    lib = mh.load_library()
    a, keep = r.to_c()
    Q = r.n_reqs
    chosen = np.full(max(n_chosen, 1), -1, np.int32)
    reason = np.zeros(max(Q, 1), np.uint8)
    bits = np.zeros(max((Q + 31) // 32, 1), np.uint32)
    co = np.ascontiguousarray(chosen_off, np.uint64)
    some = lambda x: x if x.size else np.zeros(1, x.dtype)
    rc = lib.mochi_tally_responses(Q, a.req_resp_off, a.n_ops, mh._ptr(some(dec["resp_n_ops"])), a.slot_off,
                                   mh._ptr(some(dec["op_status"])), mh._ptr(some(co)), R, mh._ptr(chosen), mh._ptr(reason),
                                   mh._ptr(bits))
    assert rc == mh.OK
    return chosen, reason[:Q], bits


def assert_equal(got: dict, want: dict, what: str = "") -> None:
    assert set(got) == set(want)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s %s" % (what, k))


# ---------------------------------------------------------------------------
# google.protobuf (tests that use it start with pytest.importorskip("google.protobuf"))
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def classes():
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory

    T = descriptor_pb2.FieldDescriptorProto
    fdp = descriptor_pb2.FileDescriptorProto()
    fdp.name = "mochi_result_reply_model.proto"
    fdp.package = RM.PKG + ".rr"
    fdp.syntax = "proto3"
    en = fdp.enum_type.add()
    en.name = "OperationResultStatus"
    for nm, num in (("OK", 0), ("WRONG_SHARD", 1)):
        v = en.value.add()
        v.name, v.number = nm, num
    p = "." + fdp.package + "."
    O, R = T.LABEL_OPTIONAL, T.LABEL_REPEATED

    def msg(name, flds, maps=()):
        m = fdp.message_type.add()
        m.name = name
        for ename, vty, vtn in maps:
            d = m.nested_type.add()
            d.name = ename
            d.options.map_entry = True
            k = d.field.add()
            k.name, k.number, k.type, k.label = "key", 1, T.TYPE_STRING, O
            v = d.field.add()
            v.name, v.number, v.type, v.label = "value", 2, vty, O
            if vtn:
                v.type_name = vtn
        for nm, num, ty, tn, label in flds:
            f = m.field.add()
            f.name, f.number, f.type, f.label = nm, num, ty, label
            if tn:
                f.type_name = tn

    msg("Grant", [("objectId", 1, T.TYPE_STRING, "", O), ("timestamp", 2, T.TYPE_INT64, "", O),
                  ("configstamp", 3, T.TYPE_INT64, "", O), ("transactionHash", 4, T.TYPE_STRING, "", O),
                  ("status", 5, T.TYPE_ENUM, p + "OperationResultStatus", O)])
    msg("MultiGrant", [("grants", 1, T.TYPE_MESSAGE, p + "MultiGrant.GrantsEntry", R),
                       ("clientId", 2, T.TYPE_STRING, "", O), ("hash", 3, T.TYPE_STRING, "", O),
                       ("serverId", 4, T.TYPE_STRING, "", O),
                       ("grantSignatures", 5, T.TYPE_MESSAGE, p + "MultiGrant.GrantSignaturesEntry", R)],
        maps=[("GrantsEntry", T.TYPE_MESSAGE, p + "Grant"), ("GrantSignaturesEntry", T.TYPE_BYTES, "")])
    msg("WriteCertificate", [("grants", 1, T.TYPE_MESSAGE, p + "WriteCertificate.GrantsEntry", R)],
        maps=[("GrantsEntry", T.TYPE_MESSAGE, p + "MultiGrant")])
    msg("OperationResult", [("result", 1, T.TYPE_STRING, "", O),
                            ("currentCertificate", 2, T.TYPE_MESSAGE, p + "WriteCertificate", O),
                            ("existed", 3, T.TYPE_BOOL, "", O),
                            ("status", 4, T.TYPE_ENUM, p + "OperationResultStatus", O)])
    msg("TransactionResult", [("operations", 1, T.TYPE_MESSAGE, p + "OperationResult", R)])
    msg("Write2AnsFromServer", [("result", 1, T.TYPE_MESSAGE, p + "TransactionResult", O), ("rid", 2, T.TYPE_STRING, "", O)])
    msg("ReadFromServer", [("result", 1, T.TYPE_MESSAGE, p + "TransactionResult", O), ("nonce", 2, T.TYPE_STRING, "", O),
                           ("rid", 3, T.TYPE_STRING, "", O)])
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fdp)
    get = lambda n: message_factory.GetMessageClass(pool.FindMessageTypeByName(fdp.package + "." + n))
    return {n: get(n) for n in ("WriteCertificate", "OperationResult", "Write2AnsFromServer", "ReadFromServer")}


def parse_protobuf(body: bytes, kind: int):
    """The google.protobuf message of the body, or None where it raises DecodeError."""
    from google.protobuf.message import DecodeError

    m = classes()["ReadFromServer" if kind == RD else "Write2AnsFromServer"]()
    try:
        m.ParseFromString(body)
    except DecodeError:
        return None
    return m


# Where the Python runtime (upb) and the decoder's rules part, by case name: what Python does
# there, and why the decoder's verdict stands.  crosscheck() requires exactly this difference;
# tests/test_result_reply_cpu.py has one test per entry.
PYTHON_DEPARTS = {
    # the decoder's rule is the one of csrc/wire_walk.h: groups to depth 100, counted alone, wherever
    # the message sits.  upb (as protobuf-java's recursion limit) also counts the messages around the
    # group: the two around an OperationResult's fields, so it refuses 99 and 100 groups there (at the top
    # level, with no message around them, it draws the line where the decoder does)
    "group:op_99": ("python_rejects", "group depth is counted without the enclosing messages"),
    "group:op_100": ("python_rejects", "group depth is counted without the enclosing messages"),
    # readTag throws invalidTag() for field number 0 wherever it reads a tag, inside an unknown group
    # too (UnknownFieldSet.Builder.mergeFrom); upb lets it pass there
    "group:field_0_inside": ("python_accepts", "field number 0 inside an unknown group: protobuf-java throws"),
    "flip:1:261:3": ("python_accepts", "field number 0 inside an unknown group: protobuf-java throws"),
    # CodedInputStream.readTag is readRawVarint32: a five-byte tag keeps its low 32 bits; upb refuses
    # a tag above 2^32 - 1
    "tag:over_32_bits": ("python_rejects", "tag varint over 32 bits: protobuf-java truncates it"),
}


def crosscheck(body: bytes, kind: int, d: Body, java_rule: Optional[str] = None) -> None:
    """decode_body(body, kind, MAX_OPS) == d against google.protobuf: MALFORMED <=> DecodeError,
    and the values of an OK body equal the parsed message's.  java_rule ("python_rejects" /
    "python_accepts") names a case of PYTHON_DEPARTS: the two verdicts must then DIFFER in the
    stated way."""
    m = parse_protobuf(body, kind)
    if java_rule == "python_rejects":
        assert m is None and d.status != mh.RRS_MALFORMED, body.hex()
        return
    if java_rule == "python_accepts":
        assert m is not None and d.status == mh.RRS_MALFORMED, body.hex()
        return
    assert (m is not None) == (d.status != mh.RRS_MALFORMED), (d.status, body.hex())
    if m is None:
        return
    tops = [(f, po, pl) for f, wt, _, po, pl in DM._msg(body, 0, len(body)) if wt == 2]
    if d.status == mh.RRS_FALLBACK:  # a merge of several results, or of two certificates in one operation
        assert sum(1 for f, _, _ in tops if f == 1) > 1 or any(o.n_cert > 1 for o in _ops_of(body, tops))
        return
    sl = lambda s: body[s[0]:s[0] + s[1]] if s else b""
    assert m.rid.encode() == sl(d.rid)
    if kind == RD:
        assert m.nonce.encode() == sl(d.nonce)
    ops = m.result.operations
    assert len(ops) == d.n_ops == len(d.ops)
    for po, o in zip(ops, d.ops):
        assert po.status == o.status  # an int32 in Python: unknown values kept
        assert po.existed == o.existed and po.result.encode() == sl(o.result)
        assert po.HasField("currentCertificate") == (o.n_cert > 0)
        if o.n_cert == 1:
            wc = classes()["WriteCertificate"]()
            wc.ParseFromString(sl(o.cert))
            assert po.currentCertificate == wc


def _ops_of(body: bytes, tops):
    return [_op(body, eo, el) for f, po, pl in tops if f == 1 for ef, ewt, _, eo, el in DM._msg(body, po, pl)
            if ef == 1 and ewt == 2]


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------
K1, K2 = b"alpha", "kéy-€-\U0001F511".encode()
BAD_UTF8 = b"a\xc3(z"
BAD_CERT = DM.BAD_CERT_VALUE
TEN = b"\xff" * 9 + b"\x01"


@functools.lru_cache(maxsize=None)
def cert(n_keys: int = 1, n_servers: int = 3, sigs: bool = False) -> bytes:
    keys = [b"key-%d" % i for i in range(n_keys)]
    if not sigs:
        return DM.writecert(keys, n_servers)
    out = b""
    for s in range(n_servers):
        out += DM.entry(0x0A, DM.IDS[s], DM.multigrant([(k, DM.grant(k, 100 + s)) for k in keys], DM.IDS[s]))
    return out


def groups(depth: int, field: int = 9, inner: bytes = b"\x08\x01") -> bytes:
    start, end = RM.varint(field << 3 | 3), RM.varint(field << 3 | 4)
    return start * depth + inner + end * depth


def _varint10(low: int) -> bytes:
    """A 10-byte varint whose low 32 bits are `low` and whose higher bits are set."""
    return RM.varint((low & 0xFFFFFFFF) | (U64 ^ 0xFFFFFFFF))


class Case(NamedTuple):
    name: str
    kind: int
    body: bytes
    n_ops: int = 2  # the count of the transaction it answers


def _ok(result=b"value", c=True, existed=True):
    return op_result(0, result, existed, cert() if c else None)


WS = op_result(WRONG_SHARD)  # InMemoryDataStore.java:581-587: only status = 1


@functools.lru_cache(maxsize=None)
def own_cases() -> Tuple[Case, ...]:
    full_w = answer(W2, [_ok(), WS], b"rid-7")
    full_r = answer(RD, [_ok(b"read-value"), _ok(b"", True, False)], b"rid-8", b"nonce-8")
    c: List[Case] = [
        Case("empty", W2, b""),
        Case("empty:read", RD, b""),
        Case("empty:n_ops_0", W2, b"", 0),
        Case("full:write2", W2, full_w),
        Case("full:read", RD, full_r),
        Case("full:read_sigs", RD, answer(RD, [op_result(0, b"v", True, cert(2, 4, True))], b"r", b"n"), 1),
        Case("only:rid", W2, answer(W2, None, b"r")),
        Case("only:result_empty", W2, answer(W2, [])),
        Case("only:nonce", RD, answer(RD, None, b"", b"n")),
        Case("kind:other", OTHER, full_w),
        Case("kind:other_garbage", OTHER, b"\xff\xff\xff"),
        Case("kind:read_as_write2", W2, full_r),  # field 3 is unknown there
        Case("kind:write2_as_read", RD, full_w),  # field 2 is the nonce there
        # field 3: a string in a ReadFromServer alone
        Case("utf8:field3_write2", W2, answer(W2, [WS, WS], b"r", raw=RM.ld(0x1A, BAD_UTF8))),
        Case("utf8:field3_read", RD, answer(RD, [WS, WS], b"", b"n", raw=RM.ld(0x1A, BAD_UTF8))),
        Case("utf8:rid_write2", W2, answer(W2, [WS, WS], BAD_UTF8)),
        Case("utf8:nonce", RD, answer(RD, [WS, WS], b"r", BAD_UTF8)),
        Case("utf8:result", W2, answer(W2, [op_result(0, BAD_UTF8), WS], b"r")),
        Case("utf8:result_replaced_later", W2, answer(W2, [RM.ld(0x0A, BAD_UTF8) + RM.ld(0x0A, b"fine"), WS], b"r")),
        Case("utf8:result_multibyte", W2, answer(W2, [op_result(0, K2, True), op_result(0, K2[:-1] + b"\x90")], b"r")),
        Case("utf8:past_n_ops", W2, answer(W2, [WS, WS, op_result(0, BAD_UTF8)], b"r")),
        # last-wins
        Case("repeat:top_strings", RD, RM.ld(0x12, b"n1") + RM.ld(0x1A, b"r1") + RM.ld(0x0A, tx_result([WS, WS])) +
             RM.ld(0x12, b"n2") + RM.ld(0x1A, b"r2")),
        Case("repeat:op_scalars", W2, answer(W2, [b"\x20\x01\x18\x00\x0a\x01a\x20\x00\x18\x05\x0a\x02bc", WS], b"r")),
        # counts against n_ops
        Case("count:n_minus_1", W2, answer(W2, [_ok()], b"r")),
        Case("count:n_plus_1", W2, answer(W2, [_ok(), WS, _ok(b"third")], b"r")),
        Case("count:n_plus_1_bad_cert", W2, answer(W2, [_ok(), WS, op_result(0, b"x", False, BAD_CERT)], b"r")),
        Case("count:n_plus_1_cert_twice", W2, answer(W2, [_ok(), WS, _ok() + RM.ld(0x12, cert())], b"r")),
        Case("count:0_of_0", W2, answer(W2, [], b"r"), 0),
        Case("count:1_of_0", W2, answer(W2, [_ok()], b"r"), 0),
        Case("count:1_of_0_bad", W2, answer(W2, [op_result(0, BAD_UTF8)], b"r"), 0),
        Case("count:64", W2, answer(W2, [op_result(i & 1, b"r%d" % i, i % 3 == 0) for i in range(64)], b"r"), 64),
        Case("count:64_certs", RD, answer(RD, [_ok(b"r%d" % i) for i in range(64)], b"r", b"n"), 64),
        Case("count:63_of_64", W2, answer(W2, [WS] * 63, b"r"), 64),
        Case("count:65_of_64", W2, answer(W2, [op_result(0, b"r%d" % i) for i in range(65)], b"r"), 64),
        Case("count:65_trivial", W2, answer(W2, [b""] * 65, b"r"), 64),
        Case("count:65_one_bad", W2, answer(W2, [WS] * 64 + [op_result(0, BAD_UTF8)], b"r"), 64),
        Case("count:65_cert_twice", W2, answer(W2, [_ok() + RM.ld(0x12, cert())] + [WS] * 64, b"r"), 64),
        Case("count:65_result_twice", W2, answer(W2, [WS] * 65, b"r", raw=RM.ld(0x0A, tx_result([WS]))), 64),
        Case("count:64_last_bad", W2, answer(W2, [_ok(b"r%d" % i, i < 2) for i in range(63)] +
                                             [op_result(0, b"x", False, BAD_CERT)], b"r"), 64),
        # FALLBACK
        Case("result:twice", W2, RM.ld(0x0A, tx_result([_ok()])) + RM.ld(0x0A, tx_result([WS])) + RM.ld(0x12, b"r")),
        Case("result:twice_empty", W2, RM.ld(0x0A, b"") + RM.ld(0x0A, b""), 0),
        Case("result:twice_second_bad", W2, RM.ld(0x0A, tx_result([_ok()])) + RM.ld(0x0A, tx_result([op_result(0, BAD_UTF8)]))),
        Case("result:twice_first_bad", W2, RM.ld(0x0A, tx_result([op_result(0, b"", False, BAD_CERT)])) + RM.ld(0x0A, tx_result([WS]))),
        Case("cert:twice", W2, answer(W2, [_ok() + RM.ld(0x12, cert(2)), WS], b"r")),
        Case("cert:twice_second_empty", W2, answer(W2, [WS, _ok() + RM.ld(0x12, b"")], b"r")),
        Case("cert:twice_second_bad", W2, answer(W2, [_ok() + RM.ld(0x12, BAD_CERT), WS], b"r")),
        Case("cert:twice_and_utf8", RD, answer(RD, [_ok() + RM.ld(0x12, cert()), WS], b"r", BAD_UTF8)),
        # the certificate
        Case("cert:empty", W2, answer(W2, [op_result(0, b"v", True, b""), WS], b"r")),
        Case("cert:bad", W2, answer(W2, [WS, op_result(0, b"v", True, BAD_CERT)], b"r")),
        Case("cert:bad_grant", W2, answer(W2, [op_result(0, b"v", True, DM.writecert([K1], 3, bad_grant=True)), WS], b"r")),
        Case("cert:foreign_wire_type", W2, answer(W2, [op_result(0, b"v", True, raw=b"\x10\x07"), WS], b"r")),
        # scalars
        Case("existed:2", W2, answer(W2, [b"\x18\x02", b"\x18\x80\x01"], b"r")),
        Case("existed:10_bytes_high", W2, answer(W2, [b"\x18" + b"\x80" * 9 + b"\x01", b"\x18\x00"], b"r")),
        Case("status:10_bytes_low_1", W2, answer(W2, [b"\x20" + _varint10(1), b"\x20" + TEN], b"r")),
        # foreign wire types on every known field: skipped
        Case("foreign:top", RD, b"\x08\x01" + b"\x15" + bytes(4) + b"\x11" + bytes(8) + b"\x1d" + bytes(4) + b"\x18\x03" + full_r),
        Case("foreign:tx", W2, RM.ld(0x0A, b"\x08\x07" + b"\x0d" + bytes(4) + tx_result([_ok(), WS]) + b"\x09" + bytes(8))),
        Case("foreign:op", W2, answer(W2, [b"\x08\x01" + b"\x0d" + bytes(4) + b"\x15" + bytes(4) + b"\x11" + bytes(8) +
                                           RM.ld(0x1A, b"\xff") + RM.ld(0x22, b"\xff") + b"\x1d" + bytes(4) + b"\x25" + bytes(4) +
                                           _ok(), WS], b"r")),
        Case("unknown:fields", W2, full_w + b"\x28\x01" + RM.ld(0x32, b"\xff\xfe") + b"\x3d" + bytes(4) + b"\xf8\x07\x01"),
        Case("unknown:in_tx_and_op", W2, RM.ld(0x0A, RM.ld(0x12, b"\xff") + RM.ld(0x0A, WS + RM.ld(0x2A, b"\xff") + b"\x30\x01") +
                                               RM.ld(0x0A, _ok()))),
        Case("field:0", W2, full_w + b"\x00\x01"),
        Case("field:0_in_op", W2, answer(W2, [WS + b"\x02\x00", WS], b"r")),
        Case("varint:11_bytes", W2, answer(W2, [b"\x20" + b"\xff" * 10 + b"\x01", WS])),
        Case("tag:end_group", W2, full_w + b"\x4c"),
        Case("tag:over_32_bits", W2, full_w + b"\xa8\x80\x80\x80\x10\x01"),
        Case("wire_type:6", W2, full_w + b"\x4e"),
        Case("len:past_end", W2, b"\x0a\x05abc"),
        Case("len:negative", W2, b"\x12\xff\xff\xff\xff\x0f"),
        Case("len:op_past_tx", W2, RM.ld(0x0A, b"\x0a\x05\x20\x01")),
        Case("group:unterminated", W2, full_w + b"\x4b\x08\x01"),
        Case("group:wrong_end", W2, full_w + b"\x4b\x54"),
        Case("group:field_0_inside", W2, full_w + b"\x4b\x00\x01\x4c"),
    ]
    for depth in (1, 98, 99, 100, 101):
        c.append(Case("group:op_%d" % depth, W2, answer(W2, [WS + groups(depth), WS], b"r")))
    for depth in (1, 100, 101):
        c.append(Case("group:top_%d" % depth, RD, full_r + groups(depth)))
    for s, nm in ((0, "0"), (1, "1"), (2, "2"), (254, "254"), (255, "255"), (2 ** 31, "2_31"), (-1, "neg")):
        c.append(Case("status:" + nm, W2, answer(W2, [op_result(s, b"v", True), WS], b"r")))
    return tuple(c)


@functools.lru_cache(maxsize=None)
def mutation_bodies():
    """(kind, body, n_ops): three bodies that together hold every field of the four messages, and
    a fourth that is a FALLBACK (so that the corpus keeps bodies of all three statuses)."""
    small = DM.writecert([b"k"], 1)
    return (
        (W2, answer(W2, [op_result(0, b"value", True, small), WS], b"rid-1"), 2),
        (RD, answer(RD, [op_result(0, b"read", True, small), op_result(0, b"", False, small)], b"rid-2", b"nonce-2") + groups(2), 2),
        (W2, answer(W2, [WS, op_result(0, b"extra", False, small)], b"r"), 1),
        (W2, RM.ld(0x0A, tx_result([op_result(0, b"first")])) + RM.ld(0x12, b"rid") + RM.ld(0x0A, tx_result([WS])), 1),
    )


@functools.lru_cache(maxsize=None)
def corpus() -> Tuple[Case, ...]:
    """The named cases' neighbours: every truncation and single-bit flip of the four bodies,
    and duplicated / reordered / re-typed fields and unknown groups at every level."""
    out: List[Case] = []
    for i, (kind, b, k) in enumerate(mutation_bodies()):
        out += [Case("cut:%d:%d" % (i, n), kind, b[:n], k) for n in range(len(b) + 1)]
        out += [Case("flip:%d:%d:%d" % (i, p, bit), kind, b[:p] + bytes([b[p] ^ 1 << bit]) + b[p + 1:], k)
                for p in range(len(b)) for bit in range(8)]
    small = DM.writecert([b"k"], 1)
    op_fields = [RM.ld(0x0A, b"res"), RM.ld(0x12, small), b"\x18\x01", b"\x20\x01"]
    rng = np.random.RandomState(20)
    for t in range(120):
        # an operation from a shuffled multiset of its fields: duplicates (the certificate too), any order
        pick = [op_fields[j] for j in rng.randint(0, 4, rng.randint(1, 7))]
        extra = [b"", groups(int(rng.randint(1, 4))), b"\x0d" + bytes(4), b"\x10\x01", RM.ld(0x1A, b"\xfe")][rng.randint(0, 5)]
        op = b"".join(pick) + extra
        kind = RD if t & 1 else W2
        where = t % 3  # the shuffled operation first, second, or past n_ops
        ops = [WS, WS]
        ops.insert(where, op)
        top = [RM.ld(0x0A, tx_result(ops[:2 + (where == 2)])), RM.ld(0x12, b"two"), RM.ld(0x1A, b"three")]
        if t % 5 == 0:
            top.append(RM.ld(0x0A, tx_result([WS])))  # a second result
        if t % 7 == 0:
            top.append(RM.ld(0x12, b"again"))
        order = rng.permutation(len(top))
        out.append(Case("shuffle:%d" % t, kind, b"".join(top[j] for j in order), 2))
    return tuple(out)


def batch(cases, layout: str = "dense", grouping: str = "each", slots: str = "dense", lead: int = 3, tail: int = 1,
          n_ops: Optional[int] = None):
    """The cases as one mochi_result_replies.
    layout   dense: the bodies back to back behind `lead` bytes and before `tail` bytes, every alignment as it comes;
             aliased: each distinct body stored once, in reverse order, at odd offsets, responses pointing at it.
    grouping each: Q = P, every response its own request with the case's n_ops; one: Q = 1 owning all responses,
             with `n_ops` (default: the first case's).
    slots    dense: slot runs back to back in response order; guarded: in descending order with three guard slots
             between the runs and before the first."""
    cases = list(cases)
    bodies = [c.body for c in cases]
    if layout == "dense":
        off = np.cumsum([lead] + [len(b) for b in bodies])[:-1] if bodies else np.zeros(0)
        blob = b"\x5a" * lead + b"".join(bodies) + b"\x5a" * tail
    else:
        where, blob = {}, b"\xa5"
        for b in sorted(set(bodies), reverse=True):
            where[b] = len(blob)
            blob += b
        off = [where[b] for b in bodies]
    P = len(cases)
    if grouping == "each":
        req_off, k_of_q = np.arange(P + 1), [c.n_ops for c in cases]
    else:
        req_off, k_of_q = np.array([0, P]), [cases[0].n_ops if n_ops is None and cases else (n_ops or 0)]
    k_of_p = np.repeat(np.asarray(k_of_q, np.int64), np.diff(req_off)) if P else np.zeros(0, np.int64)
    if slots == "dense":
        slot_off = np.cumsum(np.concatenate([[0], k_of_p]))[:-1]
    else:
        ends = np.cumsum((k_of_p + 3)[::-1])[::-1]  # response 0 last
        slot_off = ends - k_of_p
    return mh.ResultReplies(wire=np.frombuffer(blob, np.uint8), resp_off=np.asarray(off, np.uint64),
                            resp_len=np.array([len(b) for b in bodies], np.uint32),
                            resp_kind=np.array([c.kind for c in cases], np.uint8),
                            req_resp_off=np.asarray(req_off, np.uint32), n_ops=np.asarray(k_of_q, np.uint32),
                            slot_off=np.asarray(slot_off, np.uint64))


def n_slots(r: "mh.ResultReplies") -> int:
    """Slots to allocate for a batch: to the end of the furthest run, plus three guards."""
    return r.n_slots + 3


# ---------------------------------------------------------------------------
# four servers' answers to a batch of transactions (the chain tests)
# ---------------------------------------------------------------------------
def cluster_batch(n_tx: int = 12, seed: int = 7):
    """Q transactions of 1..4 ops answered by R = 4 servers, a mix of Write2 answers and reads:
    WRONG_SHARD ops (a server that does not hold the key), a read-instead-of-apply result (the
    stored value and certificate, `existed`), a server short of one operation, a MALFORMED and a
    FALLBACK answer, one payload of another kind.  Returns (cases grouped per request, k per request)."""
    rng = np.random.RandomState(seed)
    groups_, ks = [], []
    for q in range(n_tx):
        k = 1 + q % 4
        kind = RD if q % 3 == 2 else W2
        resp = []
        for s in range(4):
            ops = []
            for j in range(k):
                if (q + s + j) % 5 == 0 or (q % 8 == 4 and s < 2 and j == 0):  # the second: two of four, below the majority
                    ops.append(WS)
                elif (q + j) % 4 == 1:  # applied earlier: the server reads instead (InMemoryDataStore.java:521-574)
                    ops.append(op_result(0, b"stored-%d-%d" % (q, j), True, cert(1, 3)))
                else:
                    ops.append(op_result(0, b"v%d" % int(rng.randint(100)) if kind == RD else b"", kind == RD, cert(1, 3)))
            body = answer(kind, ops, b"rid-%d" % q, b"nonce-%d" % q if kind == RD else b"")
            c_kind = kind
            if q == 3 and s == 1:
                body = answer(kind, ops[:-1], b"rid")  # one operation short
            elif q == 5 and s == 2:
                body = body[:-2]  # MALFORMED
            elif q == 6 and s == 0:
                body = body + RM.ld(0x0A, b"")  # FALLBACK
            elif q == 7 and s == 3:
                c_kind = OTHER
            resp.append(Case("tx%d:s%d" % (q, s), c_kind, body, k))
        groups_.append(resp)
        ks.append(k)
    return groups_, ks


def batch_grouped(groups_, ks, slots: str = "dense"):
    flat = [c for g in groups_ for c in g]
    r = batch(flat, slots=slots)
    req_off = np.cumsum([0] + [len(g) for g in groups_]).astype(np.uint32)
    k_of_p = np.repeat(np.asarray(ks, np.int64), np.diff(req_off.astype(np.int64)))
    if slots == "dense":
        slot_off = np.cumsum(np.concatenate([[0], k_of_p]))[:-1]
    else:
        ends = np.cumsum((k_of_p + 3)[::-1])[::-1]
        slot_off = ends - k_of_p
    r.req_resp_off, r.n_ops, r.slot_off = req_off, np.asarray(ks, np.uint32), np.asarray(slot_off, np.uint64)
    return r
