"""The yardstick for the read request decoder (mochi_read_request_decode[_device]) and the
read answer plan (mochi_read_answer_plan[_device]): a plain-Python encoder and decoder of
ReadToServer with protobuf-java 3.16.3 parsing semantics, written from the .proto; the
google.protobuf classes it is cross-checked against; the plan, written from
InMemoryDataStore.processReadRequest (:201-231) and processRead (:75-103); and the case
sets the CPU and the GPU tests share.

TEST INFRASTRUCTURE: the library is never its own reference here.  The decoder parses a
body into a tree of fields first (write1_decode_model.fields) and reads the messages off
that tree; keys are numbered with a dict, in op order; the plan works on bytes and on a
dict store, not on arrays.  Operation / Transaction encoding and the Operation reader are
write1_request_model's: the messages are the same.
"""
from __future__ import annotations

import functools
from typing import Callable, Dict, List, NamedTuple, Optional, Tuple

import numpy as np

import mochi_hip as mh
import result_encode_model as E
import result_reply_model as RRM
import write1_decode_model as DM
import write1_reply_model as RM
import write1_request_model as QM
from write1_request_model import BAD_UTF8, DELETE, READ, WRITE, Case, groups, operation, transaction

Malformed = DM.Malformed
MAX_OPS = 64
K1, K2 = QM.K1, QM.K2


# ---------------------------------------------------------------------------
# encoder (proto3: defaults omitted, fields in number order)
# ---------------------------------------------------------------------------
def read(client: bytes = b"", tx: Optional[bytes] = None, nonce: bytes = b"") -> bytes:
    out = RM.ld(0x0A, client) if client else b""
    if tx is not None:
        out += RM.ld(0x12, tx)
    if nonce:
        out += RM.ld(0x1A, nonce)
    return out


# ---------------------------------------------------------------------------
# decoder
# ---------------------------------------------------------------------------
class Body(NamedTuple):
    status: int
    client: Tuple[int, int] = (0, 0)  # (offset in the body, length)
    nonce: Tuple[int, int] = (0, 0)
    ops: tuple = ()  # ((action as uint32, (operand1 offset, length), operand2 bytes, operand3 bytes), ...)


def decode_body(b: bytes) -> Body:
    try:
        client, nonce, txs = (0, 0), (0, 0), []
        for f, wt, v, po, pl in DM._msg(b, 0, len(b)):
            if wt != 2:
                continue  # no varint field here: field 3 as a varint is unknown
            if f in (1, 3):
                DM._utf8(b, po, pl)
                if f == 1:
                    client = (po, pl)
                else:
                    nonce = (po, pl)
            elif f == 2:
                txs.append([QM._operation(b, eo, el) for ef, ewt, _, eo, el in DM._msg(b, po, pl) if ef == 1 and ewt == 2])
    except Malformed:
        return Body(mh.RDQ_MALFORMED)
    if len(txs) > 1 or (txs and len(txs[0]) > MAX_OPS):
        return Body(mh.RDQ_FALLBACK)
    return Body(mh.RDQ_OK, client, nonce, tuple(txs[0]) if txs else ())


def _bodies(reqs: "mh.ReadRequests") -> List[Tuple[int, bytes]]:
    wire = np.asarray(reqs.wire, np.uint8).tobytes()
    return [(off, wire[off:off + ln]) for off, ln in zip(np.asarray(reqs.msg_off).tolist(), np.asarray(reqs.msg_len).tolist())]


def decode(reqs: "mh.ReadRequests") -> dict:
    """The trimmed arrays of mochi_read_requests_decoded for the batch."""
    cols = {k: [] for k in mh._RDQ_OUT}
    cols["req_op_off"].append(0)
    keys = {}
    for off, body in _bodies(reqs):
        d = decode_body(body)
        base = off if d.status == mh.RDQ_OK else 0
        cols["req_status"].append(d.status)
        cols["req_client_off"].append(base + d.client[0])
        cols["req_client_len"].append(d.client[1])
        cols["req_nonce_off"].append(base + d.nonce[0])
        cols["req_nonce_len"].append(d.nonce[1])
        for action, (ko, kl), _, _ in d.ops:
            o = len(cols["op_obj"])
            u = mh.W1_NONE
            if action == READ and kl:
                key = body[ko:ko + kl]
                if key not in keys:
                    keys[key] = len(keys)
                    cols["key_op"].append(o)
                u = keys[key]
            cols["op_key_off"].append(off + ko)
            cols["op_key_len"].append(kl)
            cols["op_flags"].append(mh.RDOP_READ if action == READ else 0)
            cols["op_obj"].append(u)
        cols["req_op_off"].append(len(cols["op_obj"]))
    return {k: np.array(cols[k], dt) for k, (dt, w) in mh._RDQ_OUT.items()}


assert_equal = QM.assert_equal
batch = QM.batch  # the layouts of the Write1 request tests: dense / aliased


# ---------------------------------------------------------------------------
# the plan (InMemoryDataStore.java:201-231, :75-103)
# ---------------------------------------------------------------------------
class KeyRec(NamedTuple):
    """What the store holds for a key, as the reference sees it."""
    local: bool = True  # objectBelongsToCurrentShardServer
    present: bool = False  # getDataMap(key).get(key) != null
    available: bool = False  # isValueAvailble()
    value: Optional[bytes] = None  # getValue()
    cert: Optional[bytes] = None  # getCurrentC(), serialized


ABSENT = KeyRec()


def plan_body(body: bytes, lookup: Callable[[bytes], KeyRec]):
    """(plan status, the OperationResults or None, the nonce) of one ReadToServer body."""
    d = decode_body(body)
    if d.status == mh.RDQ_MALFORMED:
        return mh.RDA_NO_REPLY, None, b""  # parseFrom threw
    if d.status == mh.RDQ_FALLBACK:
        return mh.RDA_HOST, None, b""
    out = []
    for action, (ko, kl), _, _ in d.ops:  # :213
        if action != READ:
            return mh.RDA_NO_REPLY, None, b""  # :217 checkAndFailOnReadOnly(true)
        key = body[ko:ko + kl]
        if not key:
            return mh.RDA_NO_REPLY, None, b""  # :77 checkOp1IsNonEmptyKeyError
        rec = lookup(key)  # :79
        if not rec.local:  # :82, before any null check
            out.append(E.OpR(1))
            continue
        if not rec.present:
            return mh.RDA_NO_REPLY, None, b""  # :99 keyStoreValue.isValueAvailble() on null
        if rec.cert is None:
            return mh.RDA_NO_REPLY, None, b""  # :100 setCurrentCertificate(null) throws
        # :96-101: setResult only for a non-null value; an empty string is not written either
        out.append(E.OpR(0, rec.value or b"", rec.available, rec.cert, "s", "s"))
    return mh.RDA_REPLY, tuple(out), body[d.nonce[0]:d.nonce[0] + d.nonce[1]]


def key_state(reqs: "mh.ReadRequests", dec: dict, lookup: Callable[[bytes], KeyRec]) -> "mh.ReadKeyState":
    """The host's one store lookup per distinct key of a decoded batch (`dec`: its trimmed
    arrays): flags and the value and certificate slices in a blob built here."""
    wire = np.asarray(reqs.wire, np.uint8).tobytes()
    blob = bytearray(b"\x5a\xa5")
    fl, vo, vl, co, cl = [], [], [], [], []
    for o in dec["key_op"].tolist():
        ko, kl = int(dec["op_key_off"][o]), int(dec["op_key_len"][o])
        rec = lookup(wire[ko:ko + kl])
        fl.append((mh.RDK_LOCAL if rec.local else 0) | (mh.RDK_PRESENT if rec.present else 0) |
                  (mh.RDK_AVAILABLE if rec.available else 0) | (mh.RDK_HAS_CERT if rec.cert is not None else 0))
        for s, offs, lens in ((rec.value, vo, vl), (rec.cert, co, cl)):
            offs.append(len(blob))
            lens.append(len(s or b""))
            blob += (s or b"") + b"\x5a"
    return mh.ReadKeyState(store=np.frombuffer(bytes(blob), np.uint8), key_flags=np.array(fl, np.uint8),
                           key_value_off=np.array(vo, np.uint64), key_value_len=np.array(vl, np.uint32),
                           key_cert_off=np.array(co, np.uint64), key_cert_len=np.array(cl, np.uint32))


def assert_planned(planned: dict, reqs: "mh.ReadRequests", dec: dict, ks: "mh.ReadKeyState",
                   lookup: Callable[[bytes], KeyRec]) -> list:
    """The library's plan over `dec` holds what plan_body says of every body.  Returns the
    model's (status, results, nonce) per request."""
    store = np.asarray(ks.store, np.uint8).tobytes()
    want = [plan_body(b, lookup) for _, b in _bodies(reqs)]
    np.testing.assert_array_equal(planned["plan_status"], [w[0] for w in want])
    np.testing.assert_array_equal(planned["slot_off"], dec["req_op_off"][:-1])
    for q, (st, res, _) in enumerate(want):
        o0, o1 = int(dec["req_op_off"][q]), int(dec["req_op_off"][q + 1])
        assert int(planned["resp_kind"][q]) == (mh.RR_READ if st == mh.RDA_REPLY else mh.RR_OTHER), q
        assert int(planned["resp_n_ops"][q]) == (o1 - o0 if st == mh.RDA_REPLY else 0), q
        for j, s in enumerate(range(o0, o1)):
            got = tuple(int(planned[k][s]) for k in mh._RA_SLOT)
            if st != mh.RDA_REPLY:
                assert got == (0xFF, 0, 0, 0, 0, 0, 0), (q, j, got)  # absent, as the Write2 plan writes it
                continue
            r = res[j]
            if r.status == 1:
                assert got == (1, 0, 0, 0, 0, 0, 0), (q, j, got)
                continue
            status, existed, flags, ro, rl, co, cl = got
            assert (status, existed, flags) == (0, int(r.existed), mh.RAO_RESULT_STORE | mh.RAO_HAS_CERT | mh.RAO_CERT_STORE)
            assert store[ro:ro + rl] == r.result and store[co:co + cl] == r.cert, (q, j)
    return want


def expected_bodies(want) -> List[bytes]:
    """The ReadFromServer body of every request of assert_planned's list (b"" where none is sent)."""
    return [E.message(E.Ans(E.RD, res, nonce=nonce)) if st == mh.RDA_REPLY else b"" for st, res, nonce in want]


# ---------------------------------------------------------------------------
# google.protobuf (tests that use it start with pytest.importorskip("google.protobuf"))
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def classes():
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory

    T = descriptor_pb2.FieldDescriptorProto
    fdp = descriptor_pb2.FileDescriptorProto()
    fdp.name = "mochi_read_request_model.proto"
    fdp.package = RM.PKG + ".rdq"
    fdp.syntax = "proto3"
    en = fdp.enum_type.add()
    en.name = "OperationAction"
    for nm, num in (("READ", 0), ("DELETE", 1), ("WRITE", 2)):
        v = en.value.add()
        v.name, v.number = nm, num
    p = "." + fdp.package + "."
    O, R = T.LABEL_OPTIONAL, T.LABEL_REPEATED

    def msg(name, flds):
        m = fdp.message_type.add()
        m.name = name
        for nm, num, ty, tn, label in flds:
            f = m.field.add()
            f.name, f.number, f.type, f.label = nm, num, ty, label
            if tn:
                f.type_name = tn

    msg("Operation", [("action", 1, T.TYPE_ENUM, p + "OperationAction", O), ("operand1", 2, T.TYPE_STRING, "", O),
                      ("operand2", 3, T.TYPE_STRING, "", O), ("operand3", 4, T.TYPE_STRING, "", O)])
    msg("Transaction", [("operations", 1, T.TYPE_MESSAGE, p + "Operation", R)])
    msg("ReadToServer", [("clientId", 1, T.TYPE_STRING, "", O), ("transaction", 2, T.TYPE_MESSAGE, p + "Transaction", O),
                         ("nonce", 3, T.TYPE_STRING, "", O)])
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fdp)
    get = lambda n: message_factory.GetMessageClass(pool.FindMessageTypeByName(fdp.package + "." + n))
    return {n: get(n) for n in ("Operation", "Transaction", "ReadToServer")}


def parse_protobuf(body: bytes):
    """The google.protobuf message of the body, or None where it raises DecodeError."""
    from google.protobuf.message import DecodeError

    m = classes()["ReadToServer"]()
    try:
        m.ParseFromString(body)
    except DecodeError:
        return None
    return m


# Where the Python runtime (upb) and the decoder's rules part, by case name: what Python does
# there, and why the decoder's verdict stands (the reasons of write1_request_model.PYTHON_DEPARTS).
# crosscheck() requires exactly this difference.
PYTHON_DEPARTS = {
    # the flip turns the action's tag 08 into 0A: its ten-byte varint is now a length.  A length is read
    # with readRawVarint32, which keeps the low 32 bits of a longer varint (0 here: an empty field 1 of
    # a foreign wire type, skipped); upb refuses a length above 2^32 - 1
    "flip:1:9:1": ("python_rejects", "length varint over 32 bits: protobuf-java truncates it"),
    # readTag throws invalidTag() for field number 0 wherever it reads a tag, inside an unknown group
    # too (UnknownFieldSet.Builder.mergeFrom); upb lets it pass there
    "flip:1:29:3": ("python_accepts", "field number 0 inside an unknown group: protobuf-java throws"),
    # the decoder's rule is wire_walk.h's: groups to depth 100, counted alone; upb also counts the two
    # messages around an Operation's fields and refuses 99 and 100 groups there
    "group:op_100": ("python_rejects", "group depth is counted without the enclosing messages"),
}


def crosscheck(body: bytes, d: Body, java_rule: Optional[str] = None) -> None:
    """decode_body(body) == d against google.protobuf: MALFORMED <=> DecodeError, and the
    values of an OK body equal the parsed message's.  java_rule names a case of
    PYTHON_DEPARTS: the two verdicts must then DIFFER in the stated way."""
    m = parse_protobuf(body)
    if java_rule == "python_rejects":
        assert m is None and d.status != mh.RDQ_MALFORMED, body.hex()
        return
    if java_rule == "python_accepts":
        assert m is not None and d.status == mh.RDQ_MALFORMED, body.hex()
        return
    assert (m is not None) == (d.status != mh.RDQ_MALFORMED), (d.status, body.hex())
    if m is None:
        return
    ops = m.transaction.operations
    if d.status == mh.RDQ_FALLBACK:
        assert len(ops) > MAX_OPS or sum(1 for f, wt, *_ in DM._msg(body, 0, len(body)) if f == 2 and wt == 2) > 1
        return
    sl = lambda s: body[s[0]:s[0] + s[1]]
    assert m.clientId.encode() == sl(d.client) and m.nonce.encode() == sl(d.nonce)
    assert len(ops) == len(d.ops)
    for po, (action, k, o2, o3) in zip(ops, d.ops):
        assert po.action & 0xFFFFFFFF == action
        assert po.operand1.encode() == sl(k) and po.operand2.encode() == o2 and po.operand3.encode() == o3


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------
NONCE = b"nonce-0123456789"
_r = lambda k, o2=b"", o3=b"": operation(READ, k, o2, o3)


@functools.lru_cache(maxsize=None)
def own_cases() -> Tuple[Case, ...]:
    full = read(b"client-1", transaction([_r(K1), _r(K2), _r(K1)]), NONCE)
    act = lambda a: read(b"c", transaction([b"\x08" + a + RM.ld(0x12, K1), _r(K2)]), NONCE)
    c: List[Case] = [
        Case("empty", b""),
        Case("only:nonce", read(nonce=NONCE)),
        Case("only:client", read(client=b"c")),
        Case("only:tx_empty", read(tx=b"")),
        Case("full", full),
        Case("key:multibyte", read(b"c", transaction([_r(K2), _r(K2[:-1] + b"\x90"), _r(K2)]), NONCE)),
        Case("key:empty", read(b"c", transaction([_r(b""), _r(K1)]), NONCE)),
        Case("action:absent", read(b"c", transaction([RM.ld(0x12, K1)]), NONCE)),
        Case("action:explicit_0", act(b"\x00")),
        Case("action:10_bytes_low_0", act(QM._varint10(0))),
        Case("action:1", act(RM.varint(1))),
        Case("action:2", act(RM.varint(2))),
        Case("action:7", act(RM.varint(7))),
        Case("action:last_wins", read(b"c", transaction([b"\x08\x02\x08\x00" + RM.ld(0x12, K1), b"\x08\x00\x08\x01" + RM.ld(0x12, K2)]))),
        Case("nonce:twice", read(b"c", transaction([_r(K1)]), b"first") + RM.ld(0x1A, b"second")),
        Case("client:twice", RM.ld(0x0A, b"first") + read(b"second", transaction([_r(K1)]), NONCE)),
        Case("field3:varint", read(b"c", transaction([_r(K1)])) + b"\x18\x07"),
        Case("field3:varint_then_nonce", b"\x18\x07" + read(b"c", transaction([_r(K1)]), NONCE)),
        Case("field4:string", read(b"c", transaction([_r(K1)]), NONCE) + RM.ld(0x22, b"\xff\xfe")),
        Case("field4:varint", read(b"c", transaction([_r(K1)]), NONCE) + b"\x20\x05"),
        Case("foreign:top", b"\x08\x01" + b"\x15" + bytes(4) + b"\x11" + bytes(8) + b"\x1d" + bytes(4) + full),
        Case("tx:twice", RM.ld(0x12, transaction([_r(K1)])) + RM.ld(0x12, transaction([_r(K2)])) + RM.ld(0x1A, NONCE)),
        Case("tx:twice_second_bad", RM.ld(0x12, transaction([_r(K1)])) + RM.ld(0x12, transaction([_r(BAD_UTF8)]))),
        Case("ops:64", read(b"c", transaction([_r(b"k%d" % i) for i in range(64)]), NONCE)),
        Case("ops:65", read(b"c", transaction([_r(b"k%d" % i) for i in range(65)]), NONCE)),
        Case("ops:65_one_bad", read(b"c", transaction([_r(b"k%d" % i) for i in range(64)] + [_r(BAD_UTF8)]), NONCE)),
        Case("utf8:client", read(BAD_UTF8, transaction([_r(K1)]), NONCE)),
        Case("utf8:nonce", read(b"c", transaction([_r(K1)]), BAD_UTF8)),
        Case("utf8:operand1", read(b"c", transaction([_r(K1), _r(BAD_UTF8)]), NONCE)),
        Case("utf8:operand2", read(b"c", transaction([operation(WRITE, K1, BAD_UTF8)]), NONCE)),
        Case("utf8:operand3", read(b"c", transaction([operation(DELETE, K1, b"v", BAD_UTF8)]), NONCE)),
        Case("utf8:read_operand2", read(b"c", transaction([_r(K1), _r(K2, BAD_UTF8)]), NONCE)),
        Case("field:0", full + b"\x00\x01"),
        Case("varint:11_bytes", full + b"\x28" + b"\xff" * 10 + b"\x01"),
        Case("len:past_end", b"\x1a\x05abc"),
        Case("len:past_end_in_tx", read(tx=b"\x0a\x09" + _r(K1))),
    ]
    for depth in (100, 101):
        c.append(Case("group:top_%d" % depth, full + groups(depth)))
        c.append(Case("group:op_%d" % depth, read(b"c", transaction([_r(K1) + groups(depth)]), NONCE)))
    return tuple(c)


@functools.lru_cache(maxsize=None)
def mutation_bodies() -> Tuple[bytes, ...]:
    """Two bodies that together hold every field of the three messages, unknown fields and a group."""
    return (
        read(b"client-1", transaction([operation(READ, K1, b"o2", b"o3"), operation(DELETE, K2)]), NONCE),
        RM.ld(0x12, transaction([_r(b"r"), b"\x08" + QM._varint10(0) + RM.ld(0x12, b"k")]) + b"\x10\x01") + b"\x18\x07" +
        groups(2) + RM.ld(0x1A, b"n2") + RM.ld(0x0A, b"c2") + RM.ld(0x22, b"h"),
    )


@functools.lru_cache(maxsize=None)
def mutations() -> Tuple[Case, ...]:
    """Every truncation and every single-bit flip of the two bodies."""
    out = []
    for i, b in enumerate(mutation_bodies()):
        out += [Case("cut:%d:%d" % (i, n), b[:n]) for n in range(len(b) + 1)]
        out += [Case("flip:%d:%d:%d" % (i, p, bit), b[:p] + bytes([b[p] ^ 1 << bit]) + b[p + 1:])
                for p in range(len(b)) for bit in range(8)]
    return tuple(out)


def req(ops, nonce: bytes = NONCE) -> bytes:
    """A ReadToServer of (action, key) ops."""
    return read(b"c", transaction([operation(a, k) for a, k in ops]), nonce)


def dedup_batches() -> Dict[str, List[bytes]]:
    long = b"k" * 40
    return {
        "one_key": [req([(READ, b"same"), (READ, b"same")]) for _ in range(40)],
        "last_byte": [req([(READ, long + bytes([65 + (q + j) % 26])) for j in range(3)]) for q in range(30)],
        # the WRITE and the unknown action come first: were they numbered, "k" would be key 0 at op 0
        "read_and_non_read": [req([(WRITE, b"k"), (9, b"k"), (READ, b"other"), (READ, b"k"), (DELETE, b"only-delete")])],
        "empty_key": [req([(READ, b""), (READ, b"a"), (READ, b""), (READ, b"a")])],
        "ok_and_malformed": [req([(READ, b"shared"), (READ, b"mine")])[:-1], req([(READ, b"other"), (READ, b"shared")])],
    }


# ---------------------------------------------------------------------------
# the plan's cases: one store, requests that meet every rule
# ---------------------------------------------------------------------------
CERT = E.CERT
STORE: Dict[bytes, KeyRec] = {
    b"val": KeyRec(True, True, True, b"v-val", CERT),
    b"val2": KeyRec(True, True, True, "wért-€".encode(), E.CERT4),
    b"empty-cert": KeyRec(True, True, True, b"x", b""),  # written as 12 00
    b"deleted": KeyRec(True, True, False, None, CERT),  # a null value: no result field
    b"empty-value": KeyRec(True, True, True, b"", CERT),  # an empty value: no result field either
    b"nocert": KeyRec(True, True, False, None, None),  # a Write1 grant made the container, no Write2 yet
    b"far-held": KeyRec(False, True, True, b"elsewhere", CERT),
    b"far": KeyRec(False, False),
    # b"absent": local, no container (the default)
}
NO_REPLY_CAUSES = {"non_read": (WRITE, b"val"), "unknown_action": (7, b"val"), "empty_key": (READ, b""),
                   "absent": (READ, b"absent"), "nocert": (READ, b"nocert")}


def store_lookup(key: bytes) -> KeyRec:
    return STORE.get(key, ABSENT)


@functools.lru_cache(maxsize=None)
def plan_cases() -> Tuple[Case, ...]:
    fine = [(READ, b"val"), (READ, b"far"), (READ, b"val2")]
    c = [
        Case("reply:one", req([(READ, b"val")])),
        Case("reply:every_kind", req([(READ, b"val"), (READ, b"empty-cert"), (READ, b"deleted"), (READ, b"empty-value"),
                                      (READ, b"far"), (READ, b"far-held"), (READ, b"val"), (READ, b"val2")])),
        Case("reply:zero_ops", read(b"c", b"", NONCE)),
        Case("reply:no_transaction", read(b"c", None, NONCE)),
        Case("reply:no_nonce", req([(READ, b"val")], b"")),
        Case("reply:wrong_shard_alone", req([(READ, b"far")])),
        Case("reply:wrong_shard_before_null_checks", req([(READ, b"far"), (READ, b"far-held")])),
        Case("malformed", req(fine)[:-1]),
        Case("host:65_ops", read(b"c", transaction([_r(b"val")] * 65), NONCE)),
        Case("host:tx_twice", RM.ld(0x12, transaction([_r(b"val")])) + RM.ld(0x12, transaction([_r(b"val")]))),
    ]
    for nm, op in NO_REPLY_CAUSES.items():
        c.append(Case("no_reply:first:" + nm, req([op] + fine)))
        c.append(Case("no_reply:last:" + nm, req(fine + [op])))
        c.append(Case("no_reply:only:" + nm, req([op])))
    c.append(Case("reply:after_the_causes", req(fine)))
    return tuple(c)


def full_request(cause: Optional[str]) -> bytes:
    """64 ops, fine but for the last, which carries the cause (None: none)."""
    ops = [(READ, (b"val", b"far", b"deleted", b"val2")[j % 4]) for j in range(64)]
    if cause:
        ops[-1] = NO_REPLY_CAUSES[cause]
    return req(ops)


def reply_protobuf(body: bytes):
    """A ReadFromServer body parsed by google.protobuf."""
    m = RRM.classes()["ReadFromServer"]()
    m.ParseFromString(body)
    return m
