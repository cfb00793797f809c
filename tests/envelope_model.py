"""The yardstick for the ProtocolMessage envelope codec (mochi_envelope_decode / _route /
_join / _encode): a plain-Python parser with the oneof rule, the partition, the join and
the writer, a google.protobuf class to check the parser against, and the named cases and
the mutation corpus the CPU and the GPU tests share.

TEST INFRASTRUCTURE: the library is never its own reference here.  Everything below works
from bytes and Python lists and shares no code with the library.

Envelope (MochiProtocol.proto:194-213), parsed as protobuf-java 3.16.3 parses it:
  ProtocolMessage = [28 msgTimestamp] [32 serverId] [3A msgId] [42 replyToMsgId]
                    [payload: one of the fields 101..112, length-delimited]
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

PKG = "edu.stanford.cs244b.mochi.server.messages"
OK, MALFORMED, FALLBACK = 0, 1, 2
KINDS = 13
NONE = 0xFFFFFFFF
GROUP_DEPTH = 100  # CodedInputStream's default recursion limit
PAYLOAD_NAMES = ("helloToServer", "helloFromServer", "helloToServer2", "helloFromServer2", "readToServer",
                 "readFromServer", "write1ToServer", "write1OkFromServer", "write1RefusedFromServer", "write2ToServer",
                 "write2AnsFromServer", "requestFailedFromServer")  # fields 101..112
W1_KIND = {8: 0, 9: 1, 12: 2}  # -> MOCHI_W1_OK / REFUSED / REQUEST_FAILED, else OTHER (3)
RR_KIND = {11: 0, 6: 1}  # -> MOCHI_RR_WRITE2_ANS / READ, else OTHER (2)


class Malformed(Exception):
    pass


# ---------------------------------------------------------------------------
# the parser
# ---------------------------------------------------------------------------
def _varint(b: bytes, pos: int, end: int) -> Tuple[int, int]:
    v = 0
    for i in range(10):
        if pos >= end:
            raise Malformed("truncated varint")
        c = b[pos]
        pos += 1
        v |= (c & 0x7F) << (7 * i)
        if not c & 0x80:
            return v & 0xFFFFFFFFFFFFFFFF, pos
    raise Malformed("varint longer than ten bytes")


def _length(b: bytes, pos: int, end: int) -> Tuple[int, int]:
    v, pos = _varint(b, pos, end)
    v &= 0xFFFFFFFF  # readRawVarint32
    if v >= 0x80000000 or v > end - pos:
        raise Malformed("bad length")
    return v, pos


def _skip(b: bytes, pos: int, end: int, field: int, wt: int, depth: int) -> int:
    """Position after the value of an unknown field whose tag was just read."""
    if wt == 0:
        return _varint(b, pos, end)[1]
    if wt == 1 or wt == 5:
        n = 8 if wt == 1 else 4
        if end - pos < n:
            raise Malformed("truncated fixed")
        return pos + n
    if wt == 2:
        n, pos = _length(b, pos, end)
        return pos + n
    if wt == 3:
        if depth >= GROUP_DEPTH:
            raise Malformed("groups nested too deep")
        while True:
            tag, pos = _varint(b, pos, end)
            tag &= 0xFFFFFFFF
            f, w = tag >> 3, tag & 7
            if f == 0:
                raise Malformed("field number 0")
            if w == 4:
                if f != field:
                    raise Malformed("end group of another field")
                return pos
            pos = _skip(b, pos, end, f, w, depth + 1)
    raise Malformed("wire type %d" % wt)  # a lone END_GROUP, wire types 6 and 7


@dataclass
class Parsed:
    status: int
    kind: int = 0
    body: Tuple[int, int] = (0, 0)  # offset inside the frame, length
    ts: int = 0  # as int64
    server_id: Tuple[int, int] = (0, 0)
    msg_id: Tuple[int, int] = (0, 0)
    reply_to: Tuple[int, int] = (0, 0)


def parse(frame: bytes) -> Parsed:
    """One frame.  Unless the status is OK every other member is at its default."""
    b, end, pos = bytes(frame), len(frame), 0
    p = Parsed(OK)
    n_payload = 0
    try:
        while pos < end:
            tag, pos = _varint(b, pos, end)
            tag &= 0xFFFFFFFF
            field, wt = tag >> 3, tag & 7
            if field == 0:
                raise Malformed("field number 0")
            if field == 5 and wt == 0:
                v, pos = _varint(b, pos, end)
                p.ts = v - (1 << 64) if v >> 63 else v
            elif wt == 2 and (6 <= field <= 8 or 101 <= field <= 112):
                n, pos = _length(b, pos, end)
                if field <= 8:
                    try:
                        b[pos:pos + n].decode("utf-8", "strict")
                    except UnicodeDecodeError:
                        raise Malformed("string is not UTF-8")
                    setattr(p, ("server_id", "msg_id", "reply_to")[field - 6], (pos, n))
                else:
                    n_payload += 1
                    p.kind, p.body = field - 100, (pos, n)
                pos += n
            else:
                pos = _skip(b, pos, end, field, wt, 0)
    except Malformed:
        return Parsed(MALFORMED)
    return p if n_payload <= 1 else Parsed(FALLBACK)


# ---------------------------------------------------------------------------
# decode / route / join over a batch, in the shape of the library's outputs
# ---------------------------------------------------------------------------
DEC_KEYS = ("status", "kind", "body_off", "body_len", "msg_timestamp", "server_id_off", "server_id_len", "msg_id_off",
            "msg_id_len", "reply_to_off", "reply_to_len")


def decode(frames: Sequence[bytes], offsets: Sequence[int]) -> Dict[str, np.ndarray]:
    rows = []
    for f, base in zip(frames, offsets):
        p = parse(f)
        rows.append((p.status, p.kind, base + p.body[0], p.body[1], p.ts, base + p.server_id[0], p.server_id[1],
                     base + p.msg_id[0], p.msg_id[1], base + p.reply_to[0], p.reply_to[1]))
    dts = (np.uint8, np.uint8, np.uint64, np.uint32, np.int64, np.uint64, np.uint32, np.uint64, np.uint32, np.uint64, np.uint32)
    return {k: np.array([r[i] for r in rows], dt) for i, (k, dt) in enumerate(zip(DEC_KEYS, dts))}


def route(dec: Dict[str, np.ndarray]):
    """(kind_off[14], order, body_off, body_len), the last three kind_off[13] long."""
    runs: List[List[int]] = [[] for _ in range(KINDS)]
    for f, (st, k) in enumerate(zip(dec["status"], dec["kind"])):
        if st == OK and k < KINDS:
            runs[int(k)].append(f)
    order = [f for r in runs for f in r]
    kind_off = np.cumsum([0] + [len(r) for r in runs]).astype(np.uint32)
    return kind_off, np.array(order, np.uint32), dec["body_off"][order], dec["body_len"][order]


def join(request_ids: Sequence[bytes], frames: Sequence[bytes], dec: Dict[str, np.ndarray]):
    """dict(frame_req [n], req_resp_off [Q+1], resp_frame / resp_off / resp_len / resp_w1_kind /
    resp_rr_kind [P]).  The replyToMsgId is read from the frames, not through offsets."""
    first: Dict[bytes, int] = {}
    for q, i in enumerate(request_ids):
        if i:
            first.setdefault(bytes(i), q)
    frame_req, groups = [], [[] for _ in request_ids]
    for f, fr in enumerate(frames):
        p = parse(fr)
        q = NONE
        if p.status == OK and p.reply_to[1]:
            q = first.get(bytes(fr[p.reply_to[0]:p.reply_to[0] + p.reply_to[1]]), NONE)
        frame_req.append(q)
        if q != NONE:
            groups[q].append(f)
    resp = [f for g in groups for f in g]
    kinds = [int(dec["kind"][f]) for f in resp]
    return dict(frame_req=np.array(frame_req, np.uint32),
                req_resp_off=np.cumsum([0] + [len(g) for g in groups]).astype(np.uint32),
                resp_frame=np.array(resp, np.uint32), resp_off=dec["body_off"][resp], resp_len=dec["body_len"][resp],
                resp_w1_kind=np.array([W1_KIND.get(k, 3) for k in kinds], np.uint8),
                resp_rr_kind=np.array([RR_KIND.get(k, 2) for k in kinds], np.uint8))


# ---------------------------------------------------------------------------
# the writer
# ---------------------------------------------------------------------------
def varint(v: int) -> bytes:
    v &= 0xFFFFFFFFFFFFFFFF
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def tag(field: int, wt: int) -> bytes:
    return varint(field << 3 | wt)


def ld(field: int, payload: bytes) -> bytes:
    return tag(field, 2) + varint(len(payload)) + payload


def frame(kind: int = 0, body: bytes = b"", ts: int = 0, server_id: bytes = b"", msg_id: bytes = b"",
          reply_to: bytes = b"") -> bytes:
    """ProtocolMessage.toByteArray(): fields in number order, defaults omitted, a set payload
    written even when empty."""
    out = b""
    if ts:
        out += b"\x28" + varint(ts)
    for f, s in ((6, server_id), (7, msg_id), (8, reply_to)):
        if s:
            out += ld(f, s)
    if kind:
        out += ld(100 + kind, body)
    return out


def prefixed(msg: bytes) -> bytes:
    """ProtobufVarint32LengthFieldPrepender."""
    return varint(len(msg)) + msg


# ---------------------------------------------------------------------------
# google.protobuf class (dynamic descriptor; tests that use it start with
# pytest.importorskip("google.protobuf")).  The payloads are declared `bytes`: the same
# wire type as the messages, read back without a parse, so that the library throws on
# the envelope level alone.
# ---------------------------------------------------------------------------
def protocol_message_class():
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory

    T = descriptor_pb2.FieldDescriptorProto
    fdp = descriptor_pb2.FileDescriptorProto()
    fdp.name = "mochi_envelope_model.proto"
    fdp.package = PKG
    fdp.syntax = "proto3"
    m = fdp.message_type.add()
    m.name = "ProtocolMessage"
    m.oneof_decl.add().name = "payload"
    for i, nm in enumerate(PAYLOAD_NAMES):
        f = m.field.add()
        f.name, f.number, f.type, f.label, f.oneof_index = nm, 101 + i, T.TYPE_BYTES, T.LABEL_OPTIONAL, 0
    for nm, num, ty in (("msgTimestamp", 5, T.TYPE_INT64), ("serverId", 6, T.TYPE_STRING), ("msgId", 7, T.TYPE_STRING),
                        ("replyToMsgId", 8, T.TYPE_STRING)):
        f = m.field.add()
        f.name, f.number, f.type, f.label = nm, num, ty, T.LABEL_OPTIONAL
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fdp)
    return message_factory.GetMessageClass(pool.FindMessageTypeByName(PKG + ".ProtocolMessage"))


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
UUID = b"123e4567-e89b-12d3-a456-4266141740%02d"  # 36 bytes, as UUID.randomUUID().toString()


def body_of(kind: int, i: int = 0) -> bytes:
    """A stand-in body: the envelope codec does not look inside."""
    return b"" if kind == 0 else ld(1, b"body-%d-%d" % (kind, i)) + b"\x18" + varint(i)


def canonical(kind: int, i: int = 0) -> bytes:
    return frame(kind, body_of(kind, i), ts=1_700_000_000_000 + i, server_id=b"server-%d" % (i % 4), msg_id=UUID % (i % 100),
                 reply_to=UUID % ((i + 1) % 100) if kind in (2, 4, 6, 8, 9, 11, 12) else b"")


def _group(field: int, depth: int) -> bytes:
    return tag(field, 3) * depth + tag(field, 4) * depth


def _value(wt: int) -> Optional[bytes]:
    """A well-formed value of the wire type (field 9's group for 3), None where none exists."""
    return {0: b"\x07", 1: b"\x01" * 8, 2: b"\x02hi", 5: b"\x01" * 4}.get(wt)


@dataclass
class Case:
    name: str
    frame: bytes
    java_only: bool = False  # a form on which protobuf-java and upb are known to differ: not compared with the library


def named_cases() -> List[Case]:
    c: List[Case] = [Case("empty", b"")]
    for k in range(KINDS):
        c.append(Case("canonical_kind_%d" % k, canonical(k, k)))
        if k:
            c.append(Case("empty_payload_kind_%d" % k, frame(k, b"", msg_id=b"m")))
    base = frame(7, body_of(7), ts=5, server_id=b"s", msg_id=b"m", reply_to=b"r")
    # wire-type swaps on the known fields
    for field in list(range(5, 9)) + list(range(101, 113)):
        for wt in range(8):
            if wt == 3:
                v = tag(field, 3) + tag(field, 4)
            elif wt == 4:
                v = tag(field, 4)
            else:
                val = _value(wt)
                v = tag(field, wt) + (val if val is not None else b"\x00")
            c.append(Case("swap_f%d_wt%d" % (field, wt), frame(ts=9, msg_id=b"before") + v + frame(8, b"after", reply_to=b"r")))
    c += [
        Case("field_0_varint", b"\x00\x00" + base),
        Case("field_0_ld", base + b"\x02\x00"),
        Case("ts_negative_1", frame(7, b"x", ts=-1)),
        Case("ts_min", frame(7, b"x", ts=-(1 << 63))),
        Case("ts_10_bytes_noncanonical", b"\x28" + b"\xFF" * 9 + b"\x7F" + ld(107, b"x"), java_only=True),
        Case("ts_11_bytes", b"\x28" + b"\xFF" * 10 + b"\x01" + ld(107, b"x")),
        Case("ts_twice", b"\x28\x05\x28\x06"),
        Case("tag_overlong_field7", b"\xBA\x00\x02id" + ld(107, b"x")),
        Case("tag_overlong_payload", b"\xDA\x86\x80\x00\x01x"),
        Case("tag_5_bytes_high_bits", b"\xBA\x80\x80\x80\x70\x02id", java_only=True),
        Case("len_overlong", b"\x3A\x82\x00id"),
        Case("len_negative", b"\x3A\xFF\xFF\xFF\xFF\x0F"),
        Case("len_10_bytes", b"\x3A\x82\x80\x80\x80\x80\x80\x80\x80\x80\x00id", java_only=True),
        Case("group_depth_100", _group(20, 100) + base),
        Case("group_depth_101", _group(20, 101) + base),
        Case("group_wrong_end", tag(20, 3) + tag(21, 4)),
        Case("group_unclosed", tag(20, 3) + b"\x08\x01"),
        Case("group_holding_fields", tag(20, 3) + ld(7, b"\xC0\x80") + b"\x28\x01" + tag(20, 4) + base),
        Case("unknown_between", b"\x28\x05" + b"\x08\x01" + ld(6, b"s") + ld(9, b"unknown") + ld(7, b"m") + b"\x65" + b"\x00" * 4 +
             ld(107, b"body") + tag(200, 1) + b"\x00" * 8),
        Case("unknown_after_payload", ld(107, b"body") + ld(4, b"zz")),
        Case("payload_overrun_1", b"\x28\x05" + tag(107, 2) + b"\x05body"),
        Case("payload_exact", b"\x28\x05" + tag(107, 2) + b"\x04body"),
        Case("string_overrun_1", b"\x3A\x03id"),
        Case("two_payloads_same", ld(107, b"\x0A\x01a") + ld(107, b"\x18\x05")),
        Case("two_payloads_differ", ld(107, b"\x0A\x01a") + ld(110, b"\x0A\x01b")),
        Case("two_payloads_differ_reversed", ld(110, b"\x0A\x01b") + ld(107, b"\x0A\x01a")),
        Case("two_payloads_first_malformed", ld(107, b"\x0A\x7Fa") + ld(108, b"")),
        Case("two_payloads_same_first_malformed", ld(108, b"\x0A\x7Fa") + ld(108, b"")),
        Case("two_payloads_then_truncated", ld(107, b"a") + ld(108, b"b") + b"\x3A\x05id"),
        Case("two_payloads_bad_string", ld(107, b"a") + ld(108, b"b") + ld(7, b"\xC0\x80")),
        Case("payload_and_varint_payload", ld(107, b"a") + tag(108, 0) + b"\x01"),
        Case("three_payloads", ld(101, b"") + ld(102, b"") + ld(103, b"")),
        Case("utf8_2_byte", ld(7, "é".encode())),
        Case("utf8_4_byte", ld(6, "\U0001F600".encode()) + ld(8, "\U0010FFFF".encode())),
        Case("utf8_overlong_nul", ld(7, b"a\xC0\x80")),
        Case("utf8_surrogate", ld(8, b"\xED\xA0\x80")),
        Case("utf8_above_max", ld(6, b"\xF4\x90\x80\x80")),
        Case("utf8_cut_by_slice_end", b"\x3A\x03ab\xC3" + ld(101, b"")),  # ld(101, ..) begins with AA: C3 AA would be valid
        Case("utf8_cut_3_byte", ld(7, b"\xE2\x82") + ld(107, b"")),
        Case("utf8_bad_then_good", ld(7, b"\xFF") + ld(7, b"good")),
        Case("utf8_lone_continuation", ld(8, b"\x80")),
        Case("utf8_in_varint_typed_string", tag(7, 0) + b"\xC0\x00"),
        Case("strings_twice", ld(7, b"first") + ld(7, b"second") + ld(6, b"a") + ld(6, b"")),
        Case("long_ids", frame(8, b"b", msg_id=b"m" * 300, reply_to=b"r" * 200, server_id=b"s" * 130)),
        Case("end_group_top_level", tag(7, 4)),
    ]
    return c


MUTATED_BASES = (("req7", lambda: canonical(7, 3)), ("reply8", lambda: canonical(8, 4)),
                 ("bare0", lambda: frame(0, ts=-2, msg_id=b"\xC3\xA9-id", server_id=b"s")))


@functools.lru_cache(maxsize=None)
def corpus() -> Tuple[Case, ...]:
    """The named cases, then every truncation and every single-bit flip of three base frames."""
    out = named_cases()
    for nm, make in MUTATED_BASES:
        b = make()
        out += [Case("%s_trunc_%d" % (nm, i), b[:i]) for i in range(len(b))]
        out += [Case("%s_flip_%d_%d" % (nm, i, bit), b[:i] + bytes([b[i] ^ (1 << bit)]) + b[i + 1:])
                for i in range(len(b)) for bit in range(8)]
    return tuple(out)


def truncations() -> List[bytes]:
    return [c.frame for c in corpus() if "_trunc_" in c.name]


def batch_one_kind(n: int, kind: int = 7) -> List[bytes]:
    return [canonical(kind, i) for i in range(n)]


def batch_per_kind() -> List[bytes]:
    return [canonical(k, k) for k in range(KINDS)]


def batch_mix(n: int, seed: int = 0) -> List[bytes]:
    """Seeded: every third frame is not OK (malformed and fallback in turn), the rest canonical
    frames of drawn kinds."""
    rng = np.random.default_rng(seed)
    bad = [c.frame for c in named_cases() if parse(c.frame).status != OK]
    out = []
    for i in range(n):
        if i % 3 == 2:
            out.append(bad[(i // 3) % len(bad)])
        else:
            out.append(canonical(int(rng.integers(0, KINDS)), i))
    return out
