"""The yardstick for the Write1 request decoder (mochi_write1_request_decode[_device]) and
the key-state join: a plain-Python encoder and decoder of Write1ToServer / Transaction /
Operation with protobuf-java 3.16.3 parsing semantics, written from the .proto; the
google.protobuf classes it is cross-checked against; the join; and the case sets the CPU
and the GPU tests share.

TEST INFRASTRUCTURE: the library is never its own reference here.  The decoder parses a
body into a tree of fields first (write1_decode_model.fields) and reads the messages off
that tree; it shares no code and no structure with the library's level-by-level walk.
Keys are numbered with a dict, in op order.
"""
from __future__ import annotations

import functools
from typing import List, NamedTuple, Optional, Tuple

import numpy as np

import mochi_hip as mh
import write1_decode_model as DM
import write1_reply_model as RM

Malformed = DM.Malformed
MAX_OPS = 64
READ, DELETE, WRITE = 0, 1, 2
U64 = 2 ** 64 - 1


# ---------------------------------------------------------------------------
# encoder (proto3: defaults omitted, fields in number order)
# ---------------------------------------------------------------------------
def operation(action: int = 0, o1: bytes = b"", o2: bytes = b"", o3: bytes = b"") -> bytes:
    out = b"\x08" + RM.varint(action & U64) if action else b""
    for tag, v in ((0x12, o1), (0x1A, o2), (0x22, o3)):
        if v:
            out += RM.ld(tag, v)
    return out


def transaction(ops) -> bytes:
    return b"".join(RM.ld(0x0A, o) for o in ops)


def write1(client: bytes = b"", tx: Optional[bytes] = None, seed: int = 0, tx_hash: bytes = b"") -> bytes:
    out = RM.ld(0x0A, client) if client else b""
    if tx is not None:
        out += RM.ld(0x12, tx)
    if seed:
        out += b"\x18" + RM.varint(seed)
    if tx_hash:
        out += RM.ld(0x22, tx_hash)
    return out


# ---------------------------------------------------------------------------
# decoder
# ---------------------------------------------------------------------------
class Body(NamedTuple):
    status: int
    seed: int = 0
    client: Tuple[int, int] = (0, 0)  # (offset in the body, length)
    tx_hash: Tuple[int, int] = (0, 0)
    ops: tuple = ()  # ((action as uint32, (operand1 offset, length), operand2 bytes, operand3 bytes), ...)


def _operation(b: bytes, off: int, n: int):
    action, o = 0, [(0, 0), (0, 0), (0, 0)]
    for f, wt, v, po, pl in DM._msg(b, off, n):
        if f == 1 and wt == 0:
            action = v & 0xFFFFFFFF
        elif wt == 2 and f in (2, 3, 4):
            DM._utf8(b, po, pl)
            o[f - 2] = (po, pl)
    return action, o[0], b[o[1][0]:o[1][0] + o[1][1]], b[o[2][0]:o[2][0] + o[2][1]]


def decode_body(b: bytes) -> Body:
    try:
        seed, client, tx_hash, txs = 0, (0, 0), (0, 0), []
        for f, wt, v, po, pl in DM._msg(b, 0, len(b)):
            if f == 3 and wt == 0:
                seed = v & 0xFFFFFFFF
            elif wt == 2 and f in (1, 4):
                DM._utf8(b, po, pl)
                if f == 1:
                    client = (po, pl)
                else:
                    tx_hash = (po, pl)
            elif wt == 2 and f == 2:
                txs.append([_operation(b, eo, el) for ef, ewt, _, eo, el in DM._msg(b, po, pl) if ef == 1 and ewt == 2])
    except Malformed:
        return Body(mh.W1Q_MALFORMED)
    if len(txs) > 1 or (txs and len(txs[0]) > MAX_OPS):
        return Body(mh.W1Q_FALLBACK)
    return Body(mh.W1Q_OK, seed, client, tx_hash, tuple(txs[0]) if txs else ())


def op_flags(action: int) -> int:
    return mh.W1OP_WRITE if action == WRITE else mh.W1OP_DELETE if action == DELETE else 0


def decode(reqs: "mh.Write1Requests") -> dict:
    """The trimmed arrays of mochi_write1_requests_decoded for the batch."""
    wire = np.asarray(reqs.wire, np.uint8).tobytes()
    cols = {k: [] for k in mh._W1Q_OUT}
    cols["req_op_off"].append(0)
    keys = {}
    for off, ln in zip(np.asarray(reqs.msg_off).tolist(), np.asarray(reqs.msg_len).tolist()):
        d = decode_body(wire[off:off + ln])
        base = off if d.status == mh.W1Q_OK else 0
        cols["req_status"].append(d.status)
        cols["req_seed"].append(d.seed)
        cols["req_hash_off"].append(base + d.tx_hash[0])
        cols["req_hash_len"].append(d.tx_hash[1])
        cols["req_client_off"].append(base + d.client[0])
        cols["req_client_len"].append(d.client[1])
        for action, (ko, kl), _, _ in d.ops:
            o = len(cols["op_obj"])
            fl = op_flags(action)
            u = mh.W1_NONE
            if fl and kl:
                key = wire[off + ko:off + ko + kl]
                if key not in keys:
                    keys[key] = len(keys)
                    cols["key_op"].append(o)
                u = keys[key]
            cols["op_key_off"].append(off + ko)
            cols["op_key_len"].append(kl)
            cols["op_flags"].append(fl)
            cols["op_obj"].append(u)
        cols["req_op_off"].append(len(cols["op_obj"]))
    return {k: np.array(cols[k], dt) for k, (dt, w) in mh._W1Q_OUT.items()}


def assert_equal(got: dict, want: dict) -> None:
    assert set(got) == set(want)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def join(req_op_off, req_seed, flags_wire, op_obj, ks: "mh.Write1KeyState"):
    """mochi_write1_state_join in plain Python."""
    off = np.asarray(req_op_off).tolist()
    fl, ep, st = [], [], []
    for q in range(len(off) - 1):
        for o in range(off[q], off[q + 1]):
            u, f, e, s = int(op_obj[o]), int(flags_wire[o]), 0, mh.W1_NONE
            if u != mh.W1_NONE:
                f |= int(ks.key_flags[u]) & (mh.W1OP_LOCAL | mh.W1OP_HAS_SVOC)
                e = int(ks.key_epoch[u])
                ts = DM._s64((e + int(req_seed[q])) & U64)
                for g in range(int(ks.key_given_off[u]), int(ks.key_given_off[u + 1])):
                    if int(ks.given_ts[g]) == ts:
                        s = int(ks.given_stored[g])
                        break
            fl.append(f)
            ep.append(e)
            st.append(s)
    return np.array(fl, np.uint8), np.array(ep, np.int64), np.array(st, np.uint32)


# ---------------------------------------------------------------------------
# google.protobuf (tests that use it start with pytest.importorskip("google.protobuf"))
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def classes():
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory

    T = descriptor_pb2.FieldDescriptorProto
    fdp = descriptor_pb2.FileDescriptorProto()
    fdp.name = "mochi_write1_request_model.proto"
    fdp.package = RM.PKG + ".w1q"
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
    msg("Write1ToServer", [("clientId", 1, T.TYPE_STRING, "", O), ("transaction", 2, T.TYPE_MESSAGE, p + "Transaction", O),
                           ("seed", 3, T.TYPE_UINT32, "", O), ("transactionHash", 4, T.TYPE_STRING, "", O)])
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fdp)
    get = lambda n: message_factory.GetMessageClass(pool.FindMessageTypeByName(fdp.package + "." + n))
    return {n: get(n) for n in ("Operation", "Transaction", "Write1ToServer")}


def parse_protobuf(body: bytes):
    """The google.protobuf message of the body, or None where it raises DecodeError."""
    from google.protobuf.message import DecodeError

    m = classes()["Write1ToServer"]()
    try:
        m.ParseFromString(body)
    except DecodeError:
        return None
    return m


# Where the Python runtime (upb) and the decoder's rules part, by case name: what Python does
# there, and why the decoder's verdict stands.  crosscheck() requires exactly this difference.
PYTHON_DEPARTS = {
    # CodedInputStream.readTag is readRawVarint32: a five-byte tag keeps its low 32 bits (here field 5
    # of wire type 0 behind a truncated tag); upb refuses a tag above 2^32 - 1
    "flip:0:1:5": ("python_rejects", "tag varint over 32 bits: protobuf-java truncates it"),
    # readTag throws invalidTag() for field number 0 wherever it reads a tag, inside an unknown group
    # too (UnknownFieldSet.Builder.mergeFrom); upb lets it pass there
    "flip:1:20:3": ("python_accepts", "field number 0 inside an unknown group: protobuf-java throws"),
    # the decoder's rule is the one of csrc/wire_walk.h: groups to depth 100, counted alone.  upb (as
    # protobuf-java's recursion limit) also counts the two messages around an Operation's fields, so it
    # refuses 99 and 100 groups there; the decoder skips them (they carry no value it reads)
    "group:op_100": ("python_rejects", "group depth is counted without the enclosing messages"),
}


def crosscheck(body: bytes, d: Body, java_rule: Optional[str] = None) -> None:
    """decode_body(body) == d against google.protobuf: MALFORMED <=> DecodeError, and the
    values of an OK body equal the parsed message's.  java_rule ("python_rejects" /
    "python_accepts") names a case of PYTHON_DEPARTS: the two verdicts must then DIFFER
    in the stated way."""
    m = parse_protobuf(body)
    if java_rule == "python_rejects":
        assert m is None and d.status != mh.W1Q_MALFORMED, body.hex()
        return
    if java_rule == "python_accepts":
        assert m is not None and d.status == mh.W1Q_MALFORMED, body.hex()
        return
    assert (m is not None) == (d.status != mh.W1Q_MALFORMED), (d.status, body.hex())
    if m is None:
        return
    ops = m.transaction.operations
    if d.status == mh.W1Q_FALLBACK:  # a merge of several transactions, or more ops than the decoder takes
        assert len(ops) > MAX_OPS or sum(1 for f, wt, *_ in DM._msg(body, 0, len(body)) if f == 2 and wt == 2) > 1
        return
    sl = lambda s: body[s[0]:s[0] + s[1]]
    assert m.seed == d.seed and m.clientId.encode() == sl(d.client) and m.transactionHash.encode() == sl(d.tx_hash)
    assert len(ops) == len(d.ops)
    for po, (action, k, o2, o3) in zip(ops, d.ops):
        assert po.action & 0xFFFFFFFF == action  # an int32 in Python: unknown values kept, sign-extended
        assert po.operand1.encode() == sl(k) and po.operand2.encode() == o2 and po.operand3.encode() == o3


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------
K1, K2 = b"alpha", "kéy-€-\U0001F511".encode()  # a multi-byte UTF-8 key: 2, 3 and 4 byte forms
HASH = b"ab" * 64
BAD_UTF8 = b"a\xc3(z"
TEN = b"\xff" * 9 + b"\x01"  # the 10-byte varint of 2^64 - 1: low word 2^32 - 1


def groups(depth: int, field: int = 9) -> bytes:
    """`depth` nested unknown groups around one varint field."""
    start, end = RM.varint(field << 3 | 3), RM.varint(field << 3 | 4)
    return start * depth + b"\x08\x01" + end * depth


class Case(NamedTuple):
    name: str
    body: bytes


def _varint10(low: int) -> bytes:
    """A 10-byte varint whose low 32 bits are `low` and whose higher bits are set."""
    return RM.varint((low & 0xFFFFFFFF) | (U64 ^ 0xFFFFFFFF))


@functools.lru_cache(maxsize=None)
def own_cases() -> Tuple[Case, ...]:
    w, d, r = (lambda k, o2=b"v": operation(WRITE, k, o2)), (lambda k: operation(DELETE, k)), (lambda k: operation(READ, k))
    full = write1(b"client-1", transaction([w(K1), d(K2), r(K1)]), 77, HASH)
    c: List[Case] = [
        Case("empty", b""),
        Case("only:client", write1(client=b"c")),
        Case("only:tx_empty", write1(tx=b"")),
        Case("only:tx", write1(tx=transaction([w(K1)]))),
        Case("only:seed", write1(seed=5)),
        Case("only:hash", write1(tx_hash=HASH)),
        Case("full", full),
        # last-wins on every singular field, top level and Operation
        Case("repeat:scalars", RM.ld(0x0A, b"first") + b"\x18\x01" + RM.ld(0x22, b"h1") + RM.ld(0x12, transaction([w(K1)])) +
             RM.ld(0x0A, b"second") + b"\x18\x02" + RM.ld(0x22, b"h2")),
        Case("repeat:op_fields", write1(tx=transaction([b"\x08\x01\x12\x01a\x08\x02\x12\x02bc\x1a\x01x\x1a\x01y\x22\x01p\x22\x01q"]))),
        Case("seed:0", write1(b"c", transaction([w(K1)]), 0, HASH) + b"\x18\x00"),
        Case("seed:max", write1(b"c", transaction([w(K1)]), 2 ** 32 - 1, HASH)),
        Case("seed:10_bytes", b"\x18" + _varint10(0x12345678) + RM.ld(0x12, transaction([w(K1)]))),
        Case("ops:0", write1(b"c", b"", 1, HASH)),
        Case("ops:1", write1(b"c", transaction([w(K1)]), 1, HASH)),
        Case("ops:64", write1(b"c", transaction([w(b"k%d" % i) for i in range(64)]), 1, HASH)),
        Case("ops:65", write1(b"c", transaction([w(b"k%d" % i) for i in range(65)]), 1, HASH)),
        Case("ops:65_one_bad", write1(b"c", transaction([w(b"k%d" % i) for i in range(64)] + [w(BAD_UTF8)]), 1, HASH)),
        Case("tx:twice", RM.ld(0x12, transaction([w(K1)])) + RM.ld(0x12, transaction([d(K2)]))),
        Case("tx:twice_second_bad", RM.ld(0x12, transaction([w(K1)])) + RM.ld(0x12, transaction([r(BAD_UTF8)]))),
        Case("tx:twice_first_bad", RM.ld(0x12, transaction([r(BAD_UTF8)])) + RM.ld(0x12, transaction([w(K1)]))),
        Case("key:empty", write1(b"c", transaction([w(b""), w(K1), d(b"")]), 1, HASH)),
        Case("key:multibyte", write1(b"c", transaction([w(K2), d(K2), w(K2[:-1] + b"\x90")]), 1, HASH)),
        Case("key:absent_with_value", write1(tx=transaction([b"\x08\x02\x1a\x01v"]))),
        # foreign wire types on every known field: skipped
        Case("foreign:top", b"\x08\x01" + b"\x15" + bytes(4) + b"\x11" + bytes(8) + b"\x1a\x01x" + b"\x1d" + bytes(4) +
             b"\x20\x05" + b"\x21" + bytes(8) + full),
        Case("foreign:tx", write1(tx=b"\x08\x07" + b"\x0d" + bytes(4) + RM.ld(0x0A, w(K1)) + b"\x09" + bytes(8))),
        Case("foreign:op", write1(tx=transaction([b"\x0a\x01\xff" + b"\x0d" + bytes(4) + b"\x10\x01" + b"\x15" + bytes(4) +
                                                  b"\x18\x02" + b"\x19" + bytes(8) + b"\x20\x03" + b"\x25" + bytes(4) +
                                                  w(K1)]))),
        Case("unknown:fields", full + b"\x28\x01" + RM.ld(0x32, b"\xff\xfe") + b"\x3d" + bytes(4) + b"\xf8\x07\x01"),
        Case("unknown:in_tx_and_op", write1(tx=RM.ld(0x12, b"\xff") + RM.ld(0x0A, w(K1) + RM.ld(0x2A, b"\xff") + b"\x30\x01"))),
        Case("field:0", full + b"\x00\x01"),
        Case("field:0_in_op", write1(tx=transaction([w(K1) + b"\x02\x00"]))),
        Case("varint:11_bytes", b"\x18" + b"\xff" * 10 + b"\x01"),
        Case("tag:end_group", full + b"\x4c"),
        Case("wire_type:6", full + b"\x4e"),
        Case("len:past_end", b"\x0a\x05abc"),
        Case("len:negative", b"\x0a\xff\xff\xff\xff\x0f"),
    ]
    for a, nm in ((0, "0"), (1, "1"), (2, "2"), (3, "3"), (2 ** 31, "2_31")):
        c.append(Case("action:" + nm, write1(b"c", transaction([b"\x08" + RM.varint(a) + RM.ld(0x12, K1), w(K1)]), 1, HASH)))
    c.append(Case("action:10_bytes_low_2", write1(b"c", transaction([b"\x08" + _varint10(2) + RM.ld(0x12, K1)]), 1, HASH)))
    # groups: Java counts the recursion of messages and groups together (limit 100), as the library's
    # rule "groups to depth 100" does inside any message; see tests/test_write1_request_cpu.py for the runtime
    for depth in (1, 100, 101):
        c.append(Case("group:top_%d" % depth, full + groups(depth)))
        c.append(Case("group:op_%d" % depth, write1(b"c", transaction([w(K1) + groups(depth)]), 1, HASH)))
    c.append(Case("group:unterminated", full + b"\x4b\x08\x01"))
    c.append(Case("group:wrong_end", full + b"\x4b\x54"))
    for i, nm in enumerate(("client", "hash")):
        c.append(Case("utf8:" + nm, write1(BAD_UTF8 if i == 0 else b"c", transaction([w(K1)]), 1, BAD_UTF8 if i else HASH)))
    c.append(Case("utf8:operand1", write1(b"c", transaction([w(K1), w(BAD_UTF8)]), 1, HASH)))
    c.append(Case("utf8:operand2", write1(b"c", transaction([w(K1, BAD_UTF8)]), 1, HASH)))
    c.append(Case("utf8:operand3", write1(b"c", transaction([operation(WRITE, K1, b"v", BAD_UTF8)]), 1, HASH)))
    c.append(Case("utf8:read_operand1", write1(b"c", transaction([w(K1), r(BAD_UTF8)]), 1, HASH)))
    c.append(Case("utf8:surrogate", write1(b"c", transaction([w(b"\xed\xa0\x80")]), 1, HASH)))
    c.append(Case("utf8:overlong", write1(b"\xc0\x80", transaction([w(K1)]), 1, HASH)))
    c.append(Case("utf8:replaced_later", write1(tx=transaction([b"\x12\x02\xc3\x28\x12\x01a"]))))  # every occurrence is checked
    return tuple(c)


@functools.lru_cache(maxsize=None)
def mutation_bodies() -> Tuple[bytes, ...]:
    """Three bodies that together hold every field of the three messages, unknown fields and a group."""
    return (
        write1(b"client-1", transaction([operation(WRITE, K1, b"value", b"third"), operation(DELETE, K2)]), 300, b"ab" * 8),
        RM.ld(0x12, transaction([operation(READ, b"r"), operation(WRITE, b"k")]) + b"\x10\x01") + b"\x18\x07" +
        groups(2) + RM.ld(0x0A, b"c2") + RM.ld(0x22, b"h"),
        b"\x18" + _varint10(9) + RM.ld(0x12, transaction([b"\x08" + _varint10(2) + RM.ld(0x12, K2) + RM.ld(0x1A, K2)])),
    )


@functools.lru_cache(maxsize=None)
def mutations() -> Tuple[Case, ...]:
    """Every truncation and every single-bit flip of the three bodies."""
    out = []
    for i, b in enumerate(mutation_bodies()):
        out += [Case("cut:%d:%d" % (i, n), b[:n]) for n in range(len(b) + 1)]
        out += [Case("flip:%d:%d:%d" % (i, p, bit), b[:p] + bytes([b[p] ^ 1 << bit]) + b[p + 1:])
                for p in range(len(b)) for bit in range(8)]
    return tuple(out)


def batch(bodies, layout: str = "dense", lead: int = 3, tail: int = 1) -> "mh.Write1Requests":
    """dense: the bodies back to back behind `lead` bytes and before `tail` bytes, every alignment as it comes.
    aliased: each distinct body stored once, in reverse order, requests pointing at it."""
    bodies = list(bodies)
    if layout == "dense":
        off = np.cumsum([lead] + [len(b) for b in bodies])[:-1] if bodies else np.zeros(0)
        blob = b"\x5a" * lead + b"".join(bodies) + b"\x5a" * tail
    else:
        where, blob = {}, b"\xa5"
        for b in sorted(set(bodies), reverse=True):
            where[b] = len(blob)
            blob += b
        off = [where[b] for b in bodies]
    return mh.Write1Requests(wire=np.frombuffer(blob, np.uint8), msg_off=np.asarray(off, np.uint64),
                             msg_len=np.array([len(b) for b in bodies], np.uint32))


def encode_batch(b: "mh.Write1Batch", client_of=lambda q: b"client-%d" % q) -> List[bytes]:
    """The Write1ToServer bodies of a SoA batch (WRITE / DELETE / READ from op_flags; operand2 a value for WRITE)."""
    s = np.asarray(b.strings, np.uint8).tobytes()
    sl = lambda o, n: s[int(o):int(o) + int(n)]
    out = []
    for q in range(b.n_reqs):
        ops = []
        for o in range(int(b.req_op_off[q]), int(b.req_op_off[q + 1])):
            f = int(b.op_flags[o])
            a = WRITE if f & mh.W1OP_WRITE else DELETE if f & mh.W1OP_DELETE else READ
            ops.append(operation(a, sl(b.op_key_off[o], b.op_key_len[o]), b"v" if a == WRITE else b""))
        out.append(write1(client_of(q), transaction(ops), int(b.req_seed[q]), sl(b.req_hash_off[q], b.req_hash_len[q])))
    return out


# ---------------------------------------------------------------------------
# a SoA batch as the server would receive it: bodies, and the store's state per distinct key
# ---------------------------------------------------------------------------
def wire_of_batch(b: "mh.Write1Batch"):
    """(requests, stored_hash_off, stored_hash_len): the batch's requests as bodies in one
    blob, with the stored grants' hashes behind them (so that the blob can be `strings`)."""
    r = batch(encode_batch(b), lead=0)
    s = np.asarray(b.strings, np.uint8).tobytes()
    hashes = [s[int(o):int(o) + int(n)] for o, n in zip(b.stored_hash_off, b.stored_hash_len)]
    off = np.cumsum([r.wire.size] + [len(h) for h in hashes])[:-1] if hashes else np.zeros(0)
    wire = np.concatenate([r.wire, np.frombuffer(b"".join(hashes), np.uint8)])
    return (mh.Write1Requests(wire=wire, msg_off=r.msg_off, msg_len=r.msg_len), np.asarray(off, np.uint64),
            np.asarray(b.stored_hash_len, np.uint32))


def key_state_of(b: "mh.Write1Batch", key_op, op_obj) -> "mh.Write1KeyState":
    """What a store that holds the batch's state answers for each distinct key of the decoded
    batch (its ops are the batch's, in order): flags and epoch of the key's container, and
    the grants it has given: one entry per stored grant an op of the batch meets, at that
    op's timestamp."""
    q_of = np.repeat(np.arange(b.n_reqs), np.diff(np.asarray(b.req_op_off, np.int64)))
    given = [dict() for _ in key_op]
    for o in np.nonzero(np.asarray(b.op_stored) != mh.W1_NONE)[0].tolist():
        ts = DM._s64((int(b.op_epoch[o]) + int(b.req_seed[q_of[o]])) & U64)
        given[int(op_obj[o])].setdefault(ts, int(b.op_stored[o]))
    off = np.cumsum([0] + [len(g) for g in given])
    return mh.Write1KeyState(
        key_flags=np.array([int(b.op_flags[o]) & (mh.W1OP_LOCAL | mh.W1OP_HAS_SVOC) for o in key_op], np.uint8),
        key_epoch=np.array([int(b.op_epoch[o]) for o in key_op], np.int64), key_given_off=off.astype(np.uint32),
        given_ts=np.array([t for g in given for t in g], np.int64),
        given_stored=np.array([s for g in given for s in g.values()], np.uint32))


def same_partition(a, b) -> bool:
    """Do two labelings split the ops into the same groups?"""
    pairs = set(zip(np.asarray(a).tolist(), np.asarray(b).tolist()))
    return len(pairs) == len({x for x, _ in pairs}) == len({y for _, y in pairs})


# ---------------------------------------------------------------------------
# key numbering and join cases the CPU and the GPU tests share
# ---------------------------------------------------------------------------
def req(ops, seed=1):
    return write1(b"c", transaction([operation(a, k, b"v" if a == WRITE else b"") for a, k in ops]), seed, b"h")


def dedup_batches():
    W_, D_, R_ = WRITE, DELETE, READ
    long = b"k" * 40
    return {
        "one_key": [req([(W_, b"same"), (D_, b"same")]) for _ in range(40)],
        "all_distinct": [req([(W_, b"key-%d" % (2 * q)), (W_, b"key-%d" % (2 * q + 1))]) for q in range(40)],
        "last_byte": [req([(W_, long + bytes([65 + (q + j) % 26])) for j in range(3)]) for q in range(30)],
        "prefix": [req([(W_, b"abc"), (W_, b"abcd"), (D_, b"ab"), (W_, b"abc"), (W_, b"abcd\x00")])],
        "ok_and_malformed": [req([(W_, b"shared"), (W_, b"mine")])[:-1], req([(W_, b"other"), (W_, b"shared")]),
                             req([(W_, b"mine")])],
        "read_equals_write": [req([(R_, b"k"), (W_, b"k"), (R_, b"k"), (9, b"k"), (R_, b"only-read")])],
    }


def join_case():
    """Seven keys over four requests; (req_op_off, req_seed, flags, op_obj, key state)."""
    NONE = mh.W1_NONE
    off, seed = [0, 3, 5, 5, 9], [5, 2 ** 32 - 1, 0, 7]
    obj = [0, 1, NONE, 2, 3, 4, 5, 6, 1]
    flags = [mh.W1OP_WRITE, mh.W1OP_DELETE, 0, mh.W1OP_WRITE, mh.W1OP_WRITE, mh.W1OP_WRITE, mh.W1OP_DELETE, mh.W1OP_WRITE,
             mh.W1OP_WRITE]
    big = 2 ** 63 - 4
    ks = mh.Write1KeyState(
        key_flags=np.array([3, 1, 3, 3, 0, 2, 0xFF], np.uint8),
        key_epoch=np.array([1000, 2000, 100, big, -7, 50, 0], np.int64),
        #  key 0: empty list | key 1: hit at the first entry (request 0) and at the last (request 3)
        #  key 2: duplicate timestamps, the first wins | key 3: epoch + seed wraps past 2^63
        #  key 4: a negative epoch | key 5: no entry matches | key 6: flags outside LOCAL | HAS_SVOC are not copied
        key_given_off=np.array([0, 0, 3, 6, 8, 9, 11, 11], np.uint32),
        given_ts=np.array([2005, 1, 2007, 99, 100 + 2 ** 32 - 1, 100 + 2 ** 32 - 1, 0, big + 2 ** 32 - 1 - 2 ** 64, 0, 56, 58],
                          np.int64),
        given_stored=np.array([10, 11, 12, 20, 21, 22, 30, 31, 40, 50, 51], np.uint32))
    want_stored = [NONE, 10, NONE, 21, 31, 40, NONE, NONE, 12]
    return off, seed, flags, obj, ks, want_stored
