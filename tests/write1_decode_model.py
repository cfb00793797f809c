"""The yardstick for the Write1 reply decoder (mochi_write1_reply_decode[_device]): a
plain-Python decoder of Write1OkFromServer / Write1RefusedFromServer bodies with
protobuf-java 3.16.3 parsing semantics, the google.protobuf classes it is cross-checked
against, and the corpus the CPU and the GPU tests share.

TEST INFRASTRUCTURE: the library is never its own reference here.  The decoder below
parses a body into a tree of fields first and reads the messages off that tree; it
shares no code and no structure with the library's level-by-level walk.  Map order comes
from its own field walk (a dict keeps first-insertion order, as a LinkedHashMap does),
not from google.protobuf's map iteration; crosscheck() compares the VALUES with
google.protobuf and requires MALFORMED <=> DecodeError.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

import mochi_hip as mh
import write1_reply_model as RM

MAX_ENTRIES = 64
GROUP_DEPTH = 100


class Malformed(Exception):
    pass


# ---------------------------------------------------------------------------
# the field tree
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
            return v & (2 ** 64 - 1), pos
    raise Malformed("varint longer than 10 bytes")


def _length(b: bytes, pos: int, end: int) -> Tuple[int, int]:
    v, pos = _varint(b, pos, end)
    v &= 0xFFFFFFFF  # readRawVarint32
    if v >= 2 ** 31 or v > end - pos:
        raise Malformed("length")
    return v, pos


def fields(b: bytes, pos: int, end: int, group: Optional[int] = None, depth: int = 0):
    """[(field, wire type, value, payload offset, payload length)] of b[pos:end] (the
    payload span for wire type 2; a group is one item of wire type 3).  Inside a group:
    up to its END_GROUP; returns (items, position after)."""
    out = []
    while pos < end:
        tag, pos = _varint(b, pos, end)
        tag &= 0xFFFFFFFF
        f, wt = tag >> 3, tag & 7
        if f == 0:
            raise Malformed("field 0")
        if wt == 0:
            v, pos = _varint(b, pos, end)
            out.append((f, 0, v, 0, 0))
        elif wt == 1 or wt == 5:
            n = 8 if wt == 1 else 4
            if end - pos < n:
                raise Malformed("truncated fixed")
            pos += n
            out.append((f, wt, None, 0, 0))
        elif wt == 2:
            n, pos = _length(b, pos, end)
            out.append((f, 2, None, pos, n))
            pos += n
        elif wt == 3:
            if depth >= GROUP_DEPTH:
                raise Malformed("groups nested too deep")
            _, pos = fields(b, pos, end, group=f, depth=depth + 1)
            out.append((f, 3, None, 0, 0))
        elif wt == 4:
            if group is None or f != group:
                raise Malformed("stray END_GROUP")
            return out, pos
        else:
            raise Malformed("wire type 6 / 7")
    if group is not None:
        raise Malformed("unterminated group")
    return out, pos


def _msg(b: bytes, off: int, n: int):
    return fields(b, off, off + n)[0]


def _utf8(b: bytes, off: int, n: int) -> None:
    try:
        b[off:off + n].decode("utf-8")
    except UnicodeDecodeError:
        raise Malformed("invalid UTF-8")


# ---------------------------------------------------------------------------
# the messages
# ---------------------------------------------------------------------------
@dataclass
class GrantV:
    object_id: bytes = b""
    ts: int = 0  # int64
    configstamp: int = 0
    tx_hash: bytes = b""
    status: int = 0  # int32

    def encode(self) -> bytes:
        """Grant.toByteArray()."""
        u64 = lambda v: v & (2 ** 64 - 1)
        out = b""
        if self.object_id:
            out += RM.ld(0x0A, self.object_id)
        if self.ts:
            out += b"\x10" + RM.varint(u64(self.ts))
        if self.configstamp:
            out += b"\x18" + RM.varint(u64(self.configstamp))
        if self.tx_hash:
            out += RM.ld(0x22, self.tx_hash)
        if self.status:
            out += b"\x28" + RM.varint(u64(self.status))  # writeEnum: the int32 sign-extended
        return out


def _s64(v: int) -> int:
    return v - 2 ** 64 if v >= 2 ** 63 else v


def _s32(v: int) -> int:
    v &= 0xFFFFFFFF
    return v - 2 ** 32 if v >= 2 ** 31 else v


def parse_grant(b: bytes, off: int, n: int) -> GrantV:
    g = GrantV()
    for f, wt, v, o, l in _msg(b, off, n):
        if f in (1, 4) and wt == 2:
            _utf8(b, o, l)
            if f == 1:
                g.object_id = b[o:o + l]
            else:
                g.tx_hash = b[o:o + l]
        elif f == 2 and wt == 0:
            g.ts = _s64(v)
        elif f == 3 and wt == 0:
            g.configstamp = _s64(v)
        elif f == 5 and wt == 0:
            g.status = _s32(v)
    return g


@dataclass
class EntryV:
    key: Tuple[int, int] = (0, 0)  # slice (offset, length), last occurrence
    val: Tuple[int, int] = (0, 0)
    n_val: int = 0


def parse_entry(b: bytes, off: int, n: int, value=None) -> EntryV:
    """A map entry; `value(b, off, n)` validates every value given."""
    e = EntryV()
    for f, wt, v, o, l in _msg(b, off, n):
        if wt != 2:
            continue
        if f == 1:
            _utf8(b, o, l)
            e.key = (o, l)
        elif f == 2:
            if value:
                value(b, o, l)
            e.val = (o, l)
            e.n_val += 1
    return e


@dataclass
class MultiGrantV:
    grants: List[EntryV] = field(default_factory=list)  # wire order
    sigs: List[EntryV] = field(default_factory=list)
    client: Tuple[int, int] = (0, 0)
    server: Tuple[int, int] = (0, 0)


def parse_multigrant(b: bytes, off: int, n: int) -> MultiGrantV:
    m = MultiGrantV()
    for f, wt, v, o, l in _msg(b, off, n):
        if wt != 2:
            continue
        if f == 1:
            m.grants.append(parse_entry(b, o, l, parse_grant))
        elif f in (2, 3, 4):
            _utf8(b, o, l)
            if f == 2:
                m.client = (o, l)
            elif f == 4:
                m.server = (o, l)
        elif f == 5:
            m.sigs.append(parse_entry(b, o, l))
    return m


def parse_writecert(b: bytes, off: int, n: int) -> None:
    for f, wt, v, o, l in _msg(b, off, n):
        if f == 1 and wt == 2:
            parse_entry(b, o, l, parse_multigrant)


def linked_map(b: bytes, entries: List[EntryV]) -> Dict[bytes, Tuple[EntryV, EntryV]]:
    """key bytes -> (the key's first entry, the entry holding its final value), in
    first-insertion order."""
    out: Dict[bytes, Tuple[EntryV, EntryV]] = {}
    for e in entries:
        k = b[e.key[0]:e.key[0] + e.key[1]]
        out[k] = (out[k][0], e) if k in out else (e, e)
    return out


@dataclass
class GrantOut:
    key: Tuple[int, int]  # the map key's slice (the first entry's)
    val: Tuple[int, int]
    ts: int
    status: int  # as grant_status: 0..254, else 0xFF
    flags: int
    sig: bytes  # 256 bytes (zeros without W1G_HAS_SIG)


@dataclass
class Decoded:
    status: int
    grants: List[GrantOut] = field(default_factory=list)
    certs: List[Tuple[Tuple[int, int], Tuple[int, int]]] = field(default_factory=list)  # (key slice, value slice)
    client: Tuple[int, int] = (0, 0)
    server: bytes = b""


def decode_body(b: bytes) -> Decoded:
    """One body, offsets relative to it.  status is OK / MALFORMED / FALLBACK here; the
    server lookup (UNKNOWN_SERVER) is decode()'s."""
    try:
        top = _msg(b, 0, len(b))
        mgs, ces = [], []
        for f, wt, v, o, l in top:
            if wt != 2:
                continue
            if f == 1:
                mgs.append(parse_multigrant(b, o, l))
            elif f == 2:
                ces.append(parse_entry(b, o, l, parse_writecert))
            elif f in (3, 4):
                _utf8(b, o, l)
    except Malformed:
        return Decoded(mh.W1R_MALFORMED)
    mg = mgs[-1] if mgs else MultiGrantV()
    if (len(mgs) > 1 or len(ces) > MAX_ENTRIES or any(e.n_val > 1 for e in ces) or len(mg.grants) > MAX_ENTRIES or
            len(mg.sigs) > MAX_ENTRIES or any(e.n_val > 1 for e in mg.grants)):
        return Decoded(mh.W1R_FALLBACK)
    out = Decoded(mh.W1R_OK, client=mg.client, server=b[mg.server[0]:mg.server[0] + mg.server[1]])
    sigs = linked_map(b, mg.sigs)
    for k, (first, last) in linked_map(b, mg.grants).items():
        raw = b[last.val[0]:last.val[0] + last.val[1]]
        g = parse_grant(b, *last.val)
        if g.encode() != raw:
            return Decoded(mh.W1R_FALLBACK)
        sv = sigs[k][1].val if k in sigs else (0, 0)
        has = k in sigs and sv[1] == 256
        flags = (mh.W1G_HAS_SIG if has else 0) | (mh.W1G_KEY_DIFFERS if k != g.object_id else 0)
        out.grants.append(GrantOut(first.key, last.val, g.ts, g.status if 0 <= g.status < 255 else 0xFF, flags,
                                   b[sv[0]:sv[0] + 256] if has else bytes(256)))
    for k, (first, last) in linked_map(b, ces).items():
        out.certs.append((first.key, last.val))
    return out


def decode(r: mh.Write1Replies, server_ids) -> dict:
    """The arrays of mochi_write1_decoded for a batch, trimmed as Write1Decoded.trimmed()."""
    ids = [x.encode() if isinstance(x, str) else bytes(x) for x in server_ids]
    wire = np.asarray(r.wire, np.uint8).tobytes()
    strings = np.asarray(r.strings, np.uint8).tobytes()
    P = r.n_resps
    req_of = np.repeat(np.arange(r.n_reqs), np.diff(np.asarray(r.req_resp_off, np.int64)))
    cols = {k: [] for k in mh._W1D_OUT}
    sig = []
    cols["resp_grant_off"].append(0)
    cols["resp_cert_off"].append(0)
    for p in range(P):
        base, kind = int(r.resp_off[p]), int(r.resp_kind[p])
        d = Decoded(mh.W1R_OK)
        parsed = kind in (mh.W1_OK, mh.W1_REFUSED)
        if parsed:
            d = decode_body(wire[base:base + int(r.resp_len[p])])
        decoded = parsed and d.status == mh.W1R_OK
        idx = ids.index(d.server) if decoded and d.server in ids else None
        if decoded and idx is None:
            d.status = mh.W1R_UNKNOWN_SERVER
        cols["resp_status"].append(d.status)
        cols["resp_kind_out"].append(mh.W1_OTHER if d.status in (mh.W1R_MALFORMED, mh.W1R_FALLBACK) else kind)
        cols["resp_server"].append(idx if idx is not None else 0x80000000 | p)
        cols["mg_signer"].append(idx if idx is not None else 0xFFFF)
        cols["resp_client_off"].append(base + d.client[0] if decoded else 0)
        cols["resp_client_len"].append(d.client[1] if decoded else 0)
        q = int(req_of[p])
        ops = [strings[int(r.op_key_off[o]):int(r.op_key_off[o]) + int(r.op_key_len[o])]
               for o in range(int(r.req_op_off[q]), int(r.req_op_off[q + 1]))]
        body = wire[base:base + int(r.resp_len[p])]
        for g in d.grants:
            key = body[g.key[0]:g.key[0] + g.key[1]]
            cols["grant_off"].append(base + g.val[0])
            cols["grant_len"].append(g.val[1])
            cols["grant_key"].append(ops.index(key) if key in ops else 0xFF)
            cols["grant_ts"].append(g.ts)
            cols["grant_status"].append(g.status)
            cols["grant_flags"].append(g.flags)
            sig.append(g.sig)
        for k, v in d.certs:
            cols["cert_key_off"].append(base + k[0])
            cols["cert_key_len"].append(k[1])
            cols["cert_val_off"].append(base + v[0])
            cols["cert_val_len"].append(v[1])
        cols["resp_grant_off"].append(len(cols["grant_off"]))
        cols["resp_cert_off"].append(len(cols["cert_key_off"]))
    out = {k: np.array(cols[k], dt) for k, (dt, w) in mh._W1D_OUT.items()}
    out["sig"] = np.frombuffer(b"".join(sig), np.uint8).reshape(-1, 256)
    return out


# ---------------------------------------------------------------------------
# google.protobuf (tests that use it start with pytest.importorskip("google.protobuf"))
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def classes():
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory

    T = descriptor_pb2.FieldDescriptorProto
    fdp = descriptor_pb2.FileDescriptorProto()
    fdp.name = "mochi_write1_decode_model.proto"
    fdp.package = RM.PKG + ".w1d"
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
    msg("Write1OkFromServer", [("multiGrant", 1, T.TYPE_MESSAGE, p + "MultiGrant", O),
                               ("currentCertificates", 2, T.TYPE_MESSAGE,
                                p + "Write1OkFromServer.CurrentCertificatesEntry", R),
                               ("clientId", 3, T.TYPE_STRING, "", O), ("hash", 4, T.TYPE_STRING, "", O)],
        maps=[("CurrentCertificatesEntry", T.TYPE_MESSAGE, p + "WriteCertificate")])
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fdp)
    get = lambda n: message_factory.GetMessageClass(pool.FindMessageTypeByName(fdp.package + "." + n))
    return {n: get(n) for n in ("Grant", "MultiGrant", "WriteCertificate", "Write1OkFromServer")}


def crosscheck(body: bytes, d: Decoded) -> None:
    """decode_body(body) == d against google.protobuf: MALFORMED <=> DecodeError, and a
    decoded body's values equal the parsed message's (maps compared as dicts)."""
    from google.protobuf.message import DecodeError

    C = classes()
    m = C["Write1OkFromServer"]()
    try:
        m.ParseFromString(body)
        ok = True
    except DecodeError:
        ok = False
    assert ok == (d.status != mh.W1R_MALFORMED), (ok, d.status, body.hex())
    if d.status != mh.W1R_OK:
        return
    mg = m.multiGrant
    sl = lambda s: body[s[0]:s[0] + s[1]]
    assert mg.serverId.encode() == d.server and mg.clientId.encode() == sl(d.client)
    assert len(d.grants) == len(mg.grants) and {sl(g.key).decode() for g in d.grants} == set(mg.grants)
    for g in d.grants:
        k = sl(g.key).decode()
        pg = mg.grants[k]
        assert pg.SerializeToString() == sl(g.val)
        assert pg.timestamp == g.ts and (pg.status if 0 <= pg.status < 255 else 0xFF) == g.status
        assert bool(g.flags & mh.W1G_KEY_DIFFERS) == (pg.objectId != k)
        has = k in mg.grantSignatures and len(mg.grantSignatures[k]) == 256
        assert bool(g.flags & mh.W1G_HAS_SIG) == has
        assert g.sig == (mg.grantSignatures[k] if has else bytes(256))
    assert len(d.certs) == len(m.currentCertificates)
    for k, v in d.certs:
        wc = C["WriteCertificate"]()
        wc.ParseFromString(sl(v))
        assert m.currentCertificates[sl(k).decode()] == wc


# ---------------------------------------------------------------------------
# The corpus: bodies with the request (operand keys) each answers
# ---------------------------------------------------------------------------
SEED = 4126
IDS = [b"server-%d" % i for i in range(4)]
N_MUTATE_KINDS = 10


def grant(oid: bytes, ts: int = 7, h: bytes = b"ab" * 32, status: int = 0, configstamp: int = 0) -> bytes:
    return GrantV(oid, ts, configstamp, h, status).encode()


def entry(tag: int, key: bytes, val: Optional[bytes]) -> bytes:
    return RM.ld(tag, RM.ld(0x0A, key) + (RM.ld(0x12, val) if val is not None else b""))


def multigrant(grants, server=IDS[0], client=b"client-1", sigs=None, extra=b"") -> bytes:
    """grants: [(key, grant bytes)]; sigs: [(key, bytes)] (default: one of 256 bytes per grant)."""
    if sigs is None:
        sigs = [(k, RM.fake_sig(3, i)) for i, (k, _) in enumerate(grants)]
    return (b"".join(entry(0x0A, k, g) for k, g in grants) + (RM.ld(0x12, client) if client else b"") +
            (RM.ld(0x22, server) if server else b"") + b"".join(entry(0x2A, k, s) for k, s in sigs) + extra)


def writecert(keys, n_servers=3, bad_grant=False) -> bytes:
    """A real WriteCertificate: n_servers MultiGrants over `keys`."""
    out = b""
    for s in range(n_servers):
        gs = [(k, grant(k, 100 + s)) for k in keys]
        if bad_grant and s == n_servers - 1:
            gs[-1] = (gs[-1][0], b"\x0a\x05ab")  # objectId runs past the Grant's end
        out += entry(0x0A, IDS[s], multigrant(gs, IDS[s], sigs=[]))
    return out


def reply(mg: Optional[bytes], certs=(), extra=b"") -> bytes:
    return (RM.ld(0x0A, mg) if mg is not None else b"") + b"".join(entry(0x12, k, v) for k, v in certs) + extra


@dataclass(frozen=True)
class Case:
    name: str
    body: bytes
    keys: Tuple[bytes, ...]  # operand1 of the request's ops
    kind: int = mh.W1_OK


def _mutate(rng, kind: int, i: int) -> Case:
    """The ten mutation kinds (w2_wire_corpus._mutate's, on a reply)."""
    keys = [b"k%d-%d" % (i, j) for j in range(1 + i % 3)]
    gs = [(k, grant(k, 50 + i)) for k in keys]
    sigs = [(k, RM.fake_sig(4, 8 * i + j)) for j, k in enumerate(keys)]
    certs = [(k, writecert([k])) for k in keys]
    ops = list(keys)
    extra = mg_extra = b""
    if kind == 1:
        gs = gs[::-1]  # map order is wire order
    elif kind == 2:
        sigs = sigs[1:]  # a grant without signature
    elif kind == 3:
        mg_extra = b"\x48\x07" + RM.ld(0x6A, b"unknown")  # unknown fields
        extra = b"\x5b\x08\x01\x5b\x5c\x5c"  # nested unknown groups (field 11) with a varint inside
    elif kind == 4:
        certs = certs + [(keys[0], writecert(keys, 2))]  # repeated certificate key: first place, last value
    elif kind == 5:
        gs = [gs[0]] + gs  # duplicate of the first entry
    elif kind == 6:
        ops = ops + ops  # ops repeating a key: the first slot
    elif kind == 9:
        ops = [b"other"] + ops[1:] + [b""]  # a grant no op names
    body = reply(multigrant(gs, IDS[i % 4], b"client-%d" % i, sigs, mg_extra), certs,
                 extra + (RM.ld(0x1A, b"cid") + RM.ld(0x22, b"hash") if kind == 3 else b""))
    if kind == 7:
        at = int(rng.integers(0, len(body)))
        body = body[:at] + bytes([body[at] ^ (1 << int(rng.integers(0, 8)))]) + body[at + 1:]
    elif kind == 8:
        body = body[:int(rng.integers(0, len(body) + 1))]
    return Case(f"mutate:{kind}", body, tuple(ops), mh.W1_REFUSED if i % 5 == 0 else mh.W1_OK)


@functools.lru_cache(maxsize=None)
def corpus() -> Tuple[Case, ...]:
    rng = np.random.default_rng(SEED)
    out: List[Case] = []
    k1, k2 = b"alpha", b"beta"
    g1, g2 = grant(k1, 11), grant(k2, 12)
    base = [
        reply(multigrant([(k1, g1)]), [(k1, writecert([k1]))]),
        reply(multigrant([(k1, g1), (k2, g2)], IDS[2]), [(k1, writecert([k1, k2])), (k2, writecert([k2], 2))]),
        reply(multigrant([(k2, g2)], IDS[1], b""), []),
    ]
    for n, b in enumerate(base):  # every truncation of three bodies
        out += [Case(f"cut:{n}", b[:i], (k1, k2)) for i in range(len(b) + 1)]
    for kind in range(N_MUTATE_KINDS):
        for i in range(12 if kind in (7, 8) else 4):
            out.append(_mutate(rng, kind, 16 * kind + i))

    def add(name, body, keys=(k1, k2), kind=mh.W1_OK):
        out.append(Case(name, body, tuple(keys), kind))

    # FALLBACK forms, each on both sides of its limit
    add("fb:two_multigrants", reply(multigrant([(k1, g1)])) + RM.ld(0x0A, multigrant([(k2, g2)], sigs=[])))
    add("fb:grant_value_twice", reply(multigrant([], sigs=[]) + RM.ld(0x0A, RM.ld(0x0A, k1) + RM.ld(0x12, g1) * 2)))
    add("ok:sig_value_twice", reply(multigrant([(k1, g1)], sigs=[]) +
                                    RM.ld(0x2A, RM.ld(0x0A, k1) + RM.ld(0x12, b"x" * 256) + RM.ld(0x12, b"y" * 256))))
    add("fb:cert_value_twice", reply(multigrant([(k1, g1)])) +
        RM.ld(0x12, RM.ld(0x0A, k1) + RM.ld(0x12, writecert([k1], 1)) * 2))
    add("fb:grant_reordered", reply(multigrant([(k1, RM.ld(0x22, b"hh") + RM.ld(0x0A, k1))])))
    add("fb:grant_unknown_field", reply(multigrant([(k1, g1 + b"\x48\x01")])))
    add("ok:replaced_grant_noncanonical", reply(multigrant([(k1, g1 + b"\x48\x01"), (k1, g1)])))
    for n in (MAX_ENTRIES, MAX_ENTRIES + 1):
        st = "ok" if n == MAX_ENTRIES else "fb"
        many = [(b"m%02d" % j, grant(b"m%02d" % j, 5)) for j in range(n)]
        add(f"{st}:{n}_grants", reply(multigrant(many, sigs=[])), [b"m63", b"m64", b"m00"])
        add(f"{st}:{n}_grant_entries_one_key", reply(multigrant([(k1, g1)] * n, sigs=[])))
        add(f"{st}:{n}_sigs", reply(multigrant([(k1, g1)], sigs=[(b"s%d" % j, b"z") for j in range(n - 1)] +
                                               [(k1, RM.fake_sig(5, 0))])))
        add(f"{st}:{n}_certs", reply(multigrant([(k1, g1)]), [(b"c%d" % (j % 40), b"") for j in range(n)]))
    # repeated keys: first position, last value
    add("rep:grants", reply(multigrant([(k1, g1), (k2, g2), (k1, grant(k1, 99))])))
    add("rep:sigs", reply(multigrant([(k1, g1)], sigs=[(k1, b"q" * 256), (k2, b"r" * 256), (k1, b"s" * 256)])))
    add("rep:sig_last_short", reply(multigrant([(k1, g1)], sigs=[(k1, b"q" * 256), (k1, b"s" * 255)])))
    add("rep:certs", reply(multigrant([(k1, g1)]), [(k1, writecert([k1])), (k2, b""), (k1, writecert([k2], 1))]))
    add("rep:scalars", reply(multigrant([(k1, g1)], extra=RM.ld(0x22, IDS[3]) + RM.ld(0x12, b"late-client"))))
    for n in (255, 256, 257):
        add(f"sig:{n}", reply(multigrant([(k1, g1)], sigs=[(k1, b"\x77" * n)])))
    add("sig:under_other_key", reply(multigrant([(k1, g1)], sigs=[(k2, b"\x77" * 256)])))
    add("key:differs", reply(multigrant([(k1, grant(k2, 3))])))
    add("key:empty_and_no_oid", reply(multigrant([(b"", GrantV(b"", 4, 0, b"h", 0).encode())])), [b"x", b""])
    add("entry:no_value", reply(multigrant([], sigs=[]) + RM.ld(0x0A, RM.ld(0x0A, k1))))
    add("entry:no_key", reply(multigrant([], sigs=[]) + RM.ld(0x0A, RM.ld(0x12, g1))))
    add("entry:cert_no_value", reply(multigrant([(k1, g1)])) + RM.ld(0x12, RM.ld(0x0A, k1)))
    add("grant:status_1", reply(multigrant([(k1, grant(k1, 0, status=1))])))
    add("grant:status_300", reply(multigrant([(k1, grant(k1, 9, status=300))])))
    add("grant:status_negative", reply(multigrant([(k1, grant(k1, 9, status=-1))])))
    add("grant:ts_negative", reply(multigrant([(k1, grant(k1, -5))])))
    add("grant:ts_min", reply(multigrant([(k1, grant(k1, -2 ** 63, configstamp=2 ** 62))])))
    add("grant:ts_overlong_varint", reply(multigrant([(k1, RM.ld(0x0A, k1) + b"\x10\x85\x00")])))
    add("utf8:key", reply(multigrant([(b"\xc3\x28", g1)])))
    add("utf8:key_multibyte_ok", reply(multigrant([("ké€\U0001F600".encode(), g1)]), [("cé".encode(), b"")]))
    add("utf8:surrogate", reply(multigrant([(k1, g1)], server=b"\xed\xa0\x80")))
    add("utf8:overlong", reply(multigrant([(k1, g1)], client=b"\xc0\xaf")))
    add("utf8:field3", reply(multigrant([(k1, g1)]), extra=RM.ld(0x1A, b"\xff")))
    add("utf8:field4", reply(multigrant([(k1, g1)]), extra=RM.ld(0x22, b"\xf5\x80\x80\x80")))
    add("utf8:cert_key", reply(multigrant([(k1, g1)]), [(b"\x80", b"")]))
    # serverId: unknown, empty, repeated
    add("sid:unknown", reply(multigrant([(k1, g1)], server=b"server-9")))
    add("sid:prefix_of_known", reply(multigrant([(k1, g1)], server=b"server-")))
    add("sid:empty", reply(multigrant([(k1, g1)], server=b"")))
    add("sid:repeated", reply(multigrant([(k1, g1)], server=b"nobody", extra=RM.ld(0x22, IDS[1]))))
    add("sid:repeated_to_unknown", reply(multigrant([(k1, g1)], server=IDS[1], extra=RM.ld(0x22, b"nobody"))))
    add("mg:absent", reply(None, [(k1, writecert([k1]))]))
    add("mg:empty", reply(b""))
    # malformed inside a nested current certificate
    add("mal:nested_cert_grant", reply(multigrant([(k1, g1)]), [(k1, writecert([k1, k2], bad_grant=True))]))
    add("mal:replaced_cert_value", reply(multigrant([(k1, g1)]), [(k1, writecert([k1], bad_grant=True)),
                                                                 (k1, writecert([k1]))]))
    add("mal:replaced_grant_value", reply(multigrant([(k1, b"\x0a\x09x"), (k1, g1)])))
    add("mal:end_group", reply(multigrant([(k1, g1)]), extra=b"\x5c"))
    add("mal:group_mismatch", reply(multigrant([(k1, g1)]), extra=b"\x5b\x64"))
    add("mal:field_0", reply(multigrant([(k1, g1)]), extra=b"\x00\x00"))
    add("mal:wire_type_7", reply(multigrant([(k1, g1)]), extra=b"\x0f"))
    add("ok:foreign_wire_types", reply(multigrant([(k1, g1)]), extra=b"\x08\x01\x15abcd\x11abcdefgh"))
    for name, b in (("empty", b""), ("one_byte", b"\x0a"), ("ff_8", b"\xff" * 8)):
        add(f"degenerate:{name}", b)
    add("kind:request_failed", b"\xff\xff", kind=mh.W1_REQUEST_FAILED)
    add("kind:other", base[0], kind=mh.W1_OTHER)
    add("kind:refused", base[1], kind=mh.W1_REFUSED)
    return tuple(out)


def batch(cases, layout: str = "packed", per_req: int = 4, lead: int = 5, tail: int = 3, mod: int = 0) -> mh.Write1Replies:
    """The cases as one batch: `per_req` consecutive responses share a request, whose ops
    are the FIRST case's keys.  Layouts: packed (pad residues 0..3, any alignment),
    shared (equal bodies point at one copy: aliased slices).  `lead` / `tail` filler
    bytes before the first and after the last body (tail=0: the last body ends the wire);
    mod > 0: body i begins at an offset congruent to i modulo `mod` instead."""
    P = len(cases)
    parts, pos, off, at = [b"\xee" * lead], lead, [], {}
    for i, c in enumerate(cases):
        if layout == "shared" and c.body in at:
            off.append(at[c.body])
            continue
        pad = (i - pos) % mod if mod else i % 4
        parts += [b"\xee" * pad, c.body]
        at[c.body] = pos + pad
        off.append(pos + pad)
        pos += pad + len(c.body)
    parts.append(b"\xee" * tail)
    heads = list(range(0, P, per_req))
    keys = [cases[h].keys for h in heads]
    flat = [k for ks in keys for k in ks]
    strings, k_off, k_len = RM.pack(list(flat), lambda i: i % 3)
    return mh.Write1Replies(
        wire=np.frombuffer(b"".join(parts), np.uint8).copy(), resp_off=np.array(off, np.uint64),
        resp_len=np.array([len(c.body) for c in cases], np.uint32), resp_kind=np.array([c.kind for c in cases], np.uint8),
        req_resp_off=np.array(heads + [P], np.uint32), strings=strings,
        req_op_off=np.concatenate([[0], np.cumsum([len(k) for k in keys])]).astype(np.uint32),
        op_key_off=k_off if flat else np.zeros(0, np.uint64), op_key_len=k_len if flat else np.zeros(0, np.uint32))


KIND_OF = {mh.W1K_OK: mh.W1_OK, mh.W1K_REFUSED: mh.W1_REFUSED, mh.W1K_THROWS: mh.W1_REQUEST_FAILED}
REPLY_SERVER_IDS = [b"server-1", RM.SERVER_ID, b"", b"server-0"]  # the encoder's id at index 1; the duplicate never wins


def replies_of(case) -> mh.Write1Replies:
    """The reply encoder's output for a case as the decoder's input: one response per request."""
    batch, issued, src = case
    wire, off, ln, st = mh.write1_reply_encode(batch, issued, src)
    assert (st == mh.ENC_OK).all()
    Q = batch.n_reqs
    return mh.Write1Replies(wire=wire, resp_off=off, resp_len=ln,
                            resp_kind=np.array([KIND_OF[int(k)] for k in issued.req_kind], np.uint8),
                            req_resp_off=np.arange(Q + 1, dtype=np.uint32), strings=batch.strings,
                            req_op_off=batch.req_op_off, op_key_off=batch.op_key_off, op_key_len=batch.op_key_len)


# ---------------------------------------------------------------------------
# Bodies and batches for the launch edges of the device form
# ---------------------------------------------------------------------------
K1, K2 = b"alpha", b"beta"
BAD_CERT_VALUE = b"\x0a\x05ab"  # a WriteCertificate whose one entry runs past its end


def heavy(n: int = MAX_ENTRIES, bad=None, fb: bool = False, light: bool = False, sig: bool = True) -> bytes:
    """A body of 1 + n level-2 entries: one MultiGrant (one grant, its signature unless
    `sig` is off) and n currentCertificates entries with distinct keys, each value
    writecert([K1], 1).  The entries listed in `bad` (an index or several) hold a Grant
    that runs past its end: MALFORMED, which only that entry's level-2 lane finds.  `fb`
    appends an unknown field to the grant: FALLBACK, which only the MultiGrant lane finds.
    `light`: empty certificate values (a large batch stays small in bytes)."""
    bad = () if bad is None else (bad,) if isinstance(bad, int) else tuple(bad)
    assert all(0 <= j < n for j in bad) and not (light and bad)
    g = grant(K1, 11) + (b"\x48\x01" if fb else b"")
    certs = [(b"h%02d" % j, b"" if light else writecert([K1], 1, bad_grant=j in bad)) for j in range(n)]
    return reply(multigrant([(K1, g)], sigs=None if sig else []), certs)


def level2_entries(body: bytes, kind: int = mh.W1_OK) -> int:
    """How many level-2 entries a response has: 1 + its currentCertificates entries on the
    wire when its kind is parsed and its top level is accepted (it parses, map keys and
    strings included, and holds at most one multiGrant, at most MAX_ENTRIES certificate
    entries and no entry with two values); 0 otherwise.  Read off the field tree."""
    if kind not in (mh.W1_OK, mh.W1_REFUSED):
        return 0
    try:
        n_mg, ces = 0, []
        for f, wt, v, o, l in _msg(body, 0, len(body)):
            if wt != 2:
                continue
            if f == 1:
                n_mg += 1
            elif f == 2:
                ces.append(parse_entry(body, o, l))
            elif f in (3, 4):
                _utf8(body, o, l)
    except Malformed:
        return 0
    if n_mg > 1 or len(ces) > MAX_ENTRIES or any(e.n_val > 1 for e in ces):
        return 0
    return 1 + len(ces)


def n_level2_entries(r: mh.Write1Replies) -> int:
    """level2_entries summed over a batch (each distinct slice and kind parsed once)."""
    wire = np.asarray(r.wire, np.uint8).tobytes()
    trip, counts = np.unique(np.stack([np.asarray(r.resp_off, np.uint64), np.asarray(r.resp_len, np.uint64),
                                       np.asarray(r.resp_kind, np.uint64)], 1), axis=0, return_counts=True)
    return sum(int(n) * level2_entries(wire[int(o):int(o) + int(l)], int(k)) for (o, l, k), n in zip(trip, counts))


@functools.lru_cache(maxsize=None)
def edge_cases() -> Dict[str, Case]:
    """The heavy bodies by name, with the unparsed kinds and the level-1 rejects the
    level-2 pattern mixes them with."""
    two_mg = heavy(8) + RM.ld(0x0A, multigrant([(K2, grant(K2, 12))], sigs=[]))  # merged by the parser: the whole body at level 1
    cs = [Case("ok:heavy", heavy(), (K1, K2)),
          Case("ok:heavy_light", heavy(light=True), (K2, K1)),
          Case("ok:heavy_no_sig", heavy(5, sig=False), (K1,)),
          Case("mal:heavy_bad_63", heavy(bad=63), (K1, K2)),
          Case("mal:heavy_bad_0_and_63", heavy(bad=(0, 63)), (K1, K2)),
          Case("mal:heavy_bad_31_and_32", heavy(bad=(31, 32)), (K1, K2)),
          Case("fb:heavy", heavy(fb=True), (K1, K2)),
          Case("mal:heavy_fb_and_bad_0", heavy(fb=True, bad=0), (K1, K2)),
          Case("mal:level1_one_byte", b"\x0a", (K1, K2)),
          Case("fb:level1_two_multigrants", two_mg, (K1, K2)),
          Case("kind:failed", b"\xff\xff", (K1, K2), mh.W1_REQUEST_FAILED),
          Case("kind:other_heavy_bad", heavy(bad=63), (K1, K2), mh.W1_OTHER)]
    return {c.name: c for c in cs}


# twelve responses: level-2 entries exist only at 2, 6, 7, 8 and 10, so the entry offsets
# repeat (a run of responses without entries) at the start, in the middle and at the end
PATTERN = ("kind:failed", "mal:level1_one_byte", "ok:heavy", "kind:other_heavy_bad", "kind:failed", "kind:other_heavy_bad",
           "mal:heavy_bad_63", "fb:heavy", "mal:heavy_fb_and_bad_0", "fb:level1_two_multigrants", "mal:heavy_bad_0_and_63",
           "kind:failed")


def pattern_cases(P: int) -> Tuple[Case, ...]:
    """The first P responses of PATTERN repeated."""
    ec = edge_cases()
    return tuple(ec[PATTERN[i % len(PATTERN)]] for i in range(P))


def batch_explicit(bodies, which, kinds, req_resp_off, req_keys, lead: int = 5, tail: int = 3) -> mh.Write1Replies:
    """A batch from its parts: response p is bodies[which[p]] (each body once in the wire,
    pad residues 0..3: responses alias), of kind kinds[p]; the requests are the CSR
    req_resp_off, request q's ops the keys req_keys[q]."""
    parts, pos, at = [b"\xee" * lead], lead, []
    for i, b in enumerate(bodies):
        parts += [b"\xee" * (i % 4), b]
        at.append(pos + i % 4)
        pos += i % 4 + len(b)
    parts.append(b"\xee" * tail)
    which = np.asarray(which, np.int64)
    flat = [k for ks in req_keys for k in ks]
    strings, k_off, k_len = RM.pack(list(flat), lambda i: i % 3)
    assert len(req_keys) == len(req_resp_off) - 1 and int(req_resp_off[-1]) == which.size
    return mh.Write1Replies(
        wire=np.frombuffer(b"".join(parts), np.uint8).copy(), resp_off=np.array(at, np.uint64)[which],
        resp_len=np.array([len(b) for b in bodies], np.uint32)[which], resp_kind=np.asarray(kinds, np.uint8),
        req_resp_off=np.asarray(req_resp_off, np.uint32), strings=strings,
        req_op_off=np.concatenate([[0], np.cumsum([len(k) for k in req_keys])]).astype(np.uint32),
        op_key_off=k_off if flat else np.zeros(0, np.uint64), op_key_len=k_len if flat else np.zeros(0, np.uint32))


def cap_batch(P: int, last: bytes) -> mh.Write1Replies:
    """P responses of two level-2 entries each (one grant without signature, one
    certificate entry with an empty value), all slices of one copy; the last response
    alone is `last`.  Five requests of unequal size."""
    small = reply(multigrant([(K1, grant(K1, 11))], sigs=[]), [(K1, b"")])
    which = np.zeros(P, np.int64)
    which[-1] = 1
    cuts = [0, 1, P // 3, P // 3 + 7, P - 2, P]
    return batch_explicit([small, last], which, np.full(P, mh.W1_OK, np.uint8), cuts, [(K1,), (K2, K1), (), (K2,), (K1, K2)])


SMALL_BAD = reply(multigrant([(K1, grant(K1, 11))], sigs=[]), [(K1, BAD_CERT_VALUE)])  # two entries, the second MALFORMED


def grouping_batch() -> mh.Write1Replies:
    """Requests without responses first, twice in a row in the middle and last; a request
    without ops; a request of MOCHI_MAX_OPS_PER_CERT ops that name the replies' grants at
    slots 0 and 63 alone, slot 0's key again at slot 7 (the first slot wins)."""
    A, B = b"key-A", b"key-B"
    bodies = [reply(multigrant([(K1, grant(K1, 11))]), [(K1, writecert([K1]))]),
              reply(multigrant([(A, grant(A, 21)), (B, grant(B, 22))], IDS[1])),
              reply(multigrant([(b"nobody", grant(b"nobody", 23)), (B, grant(B, 24))], IDS[2]), [(A, writecert([A], 1))])]
    ops64 = [b"f%02d" % j for j in range(mh.MAX_OPS_PER_CERT)]
    ops64[0], ops64[7], ops64[63] = A, A, B
    reqs = [((), (K1,)),  # (responses, ops)
            ((0, 1), (K1, K2)),
            ((), ()),
            ((), (b"x",)),
            ((1, 0, 2), ()),
            ((1, 2, 1), tuple(ops64)),
            ((0,), (K2, K1)),
            ((), (K1,))]
    which = [w for ws, _ in reqs for w in ws]
    return batch_explicit(bodies, which, np.full(len(which), mh.W1_OK, np.uint8),
                          np.concatenate([[0], np.cumsum([len(ws) for ws, _ in reqs])]), [ks for _, ks in reqs])


def far_cases() -> Tuple[Case, ...]:
    """Thirty-two responses for the offsets past 4 GiB: with and without signature, with a
    client id, with certificates, MALFORMED, FALLBACK, an unknown server, unparsed kinds."""
    by = {c.name: c for c in corpus()}
    ec = edge_cases()
    names = ["mutate:0", "mutate:2", "mutate:4", "rep:certs", "rep:sigs", "rep:scalars", "sig:255", "ok:sig_value_twice",
             "sig:256", "sid:unknown", "mal:nested_cert_grant", "fb:grant_unknown_field", "kind:request_failed",
             "kind:other", "kind:refused", "key:differs", "utf8:key_multibyte_ok", "ok:64_certs", "mg:absent"]
    cs = [by[n] for n in names] + [ec[n] for n in ("ok:heavy_light", "mal:heavy_bad_63", "ok:heavy_no_sig", "fb:heavy")]
    cs += [c for c in corpus() if c.name in ("mutate:1", "mutate:3", "mutate:5", "mutate:6", "mutate:9")][:9]
    return tuple(cs[:32])


def sig_sources(r: mh.Write1Replies, d: dict) -> List[int]:
    """Wire offset of every decoded signature (grants with W1G_HAS_SIG), found inside its
    response's slice; a signature whose bytes occur there more than once is left out."""
    wire = np.asarray(r.wire, np.uint8).tobytes()
    out = []
    for p in range(r.n_resps):
        body = wire[int(r.resp_off[p]):int(r.resp_off[p]) + int(r.resp_len[p])]
        for g in range(int(d["resp_grant_off"][p]), int(d["resp_grant_off"][p + 1])):
            if int(d["grant_flags"][g]) & mh.W1G_HAS_SIG:
                s = d["sig"][g].tobytes()
                assert s in body
                if body.count(s) == 1:
                    out.append(int(r.resp_off[p]) + body.find(s))
    return out


def assert_equal(got: dict, want: dict, what: str = "") -> None:
    for k in want:
        assert k in got, k
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), \
            (what, k, np.nonzero(np.asarray(got[k]).reshape(len(got[k]), -1) != np.asarray(want[k]).reshape(len(want[k]), -1))[0][:8]
             if got[k].shape == want[k].shape else (got[k].shape, want[k].shape))
