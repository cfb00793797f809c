"""The yardstick for the Write1 reply encoder (mochi_write1_reply_encode[_device]):
a plain-Python encoder of Write1OkFromServer / Write1RefusedFromServer bodies
(MochiProtocol.proto:117-161 with INTEGRATION.md's grantSignatures = 5, as
InMemoryDataStore.java:283-308 fills them), a google.protobuf class to read
them back with, and the case sets the CPU and the GPU tests share.

TEST INFRASTRUCTURE: the library is never its own reference here.  The encoder
below works from the arrays alone (Write1Batch, Write1Issued, Write1ReplySource)
and shares no code with the library.
"""
from __future__ import annotations

import hashlib
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np

import mochi_hip as mh
import write1_issue_model as M

PKG = "edu.stanford.cs244b.mochi.server.messages"
SERVER_ID = b"server-0"


# ---------------------------------------------------------------------------
# the encoder
# ---------------------------------------------------------------------------
def varint(v: int) -> bytes:
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def ld(tag: int, payload: bytes) -> bytes:
    return bytes([tag]) + varint(len(payload)) + payload


@dataclass
class Run:
    """One payload run of the wire: where its bytes come from and where they go."""

    kind: str  # "grant", "sig" or "cert"
    src: int  # offset in its source blob
    dst: int  # offset in the wire
    length: int


@dataclass
class Encoded:
    bodies: List[bytes]
    # lengths met while encoding, for the varint-step coverage test
    lengths: Dict[str, List[int]] = field(default_factory=lambda: dict(grants_entry=[], multigrant=[], cert_value=[],
                                                                        cert_entry=[], message=[]))
    runs: List[Run] = field(default_factory=list)

    @property
    def wire(self) -> bytes:
        return b"".join(self.bodies)


def _listed(kind: int, d: int) -> bool:
    if kind == mh.W1K_OK:
        return d in (mh.W1D_NEW, mh.W1D_RETRY, mh.W1D_WRONG_SHARD)
    return kind == mh.W1K_REFUSED and d == mh.W1D_REFUSED


def encode(batch: mh.Write1Batch, issued: mh.Write1Issued, src: mh.Write1ReplySource) -> Encoded:
    out = Encoded([])
    strings = np.asarray(batch.strings, np.uint8)
    ids = np.asarray(src.ids, np.uint8)
    sl = lambda blob, off, ln: blob[int(off):int(off) + int(ln)].tobytes()
    server = sl(ids, src.server_id_off, src.server_id_len)
    pos = 0
    for q in range(batch.n_reqs):
        kind = int(issued.req_kind[q])
        if kind == mh.W1K_THROWS:
            out.bodies.append(b"")
            continue
        o0, o1 = int(batch.req_op_off[q]), int(batch.req_op_off[q + 1])
        entries = []  # (key, grant bytes, grant src, sig, sig src, cert, cert src)
        for e in range(int(issued.req_grant_off[q]), int(issued.req_grant_off[q + 1])):
            r = int(issued.req_grant[e])
            op = next(o for o in range(o0, o1)
                      if int(issued.op_grant[o]) == r and _listed(kind, int(issued.op_decision[o])))
            key = sl(strings, batch.op_key_off[op], batch.op_key_len[op])
            if r & mh.W1_STORED:
                i = r & ~mh.W1_STORED
                g_src = int(src.stored_off[i])
                grant = sl(np.asarray(src.stored_bytes, np.uint8), g_src, src.stored_len[i])
                sig = None if issued.sig is None else np.asarray(src.stored_sig, np.uint8).reshape(-1, 256)[i].tobytes()
            else:
                g_src = int(issued.grant_off[r])
                grant = issued.grant(r)
                sig = None if issued.sig is None else np.asarray(issued.sig, np.uint8).reshape(-1, 256)[r].tobytes()
            cert, c_src = b"", 0
            if src.op_cert_off is not None:
                c_src = int(src.op_cert_off[op])
                cert = sl(np.asarray(src.certs, np.uint8), c_src, src.op_cert_len[op])
            entries.append((key, grant, g_src, sig, 256 * (r & ~mh.W1_STORED), cert, c_src))
        client = b"" if src.req_client_off is None else sl(ids, src.req_client_off[q], src.req_client_len[q])
        # MultiGrant
        mg = bytearray()
        marks = []  # (kind, src, offset inside mg / tail, length)
        for key, grant, g_src, sig, s_src, cert, c_src in entries:
            ent = ld(0x0A, key) + ld(0x12, grant)
            out.lengths["grants_entry"].append(len(ent))
            mg += ld(0x0A, ent)
            marks.append(("grant", g_src, len(mg) - len(grant), len(grant)))
        if client:
            mg += ld(0x12, client)
        if server:
            mg += ld(0x22, server)
        for key, grant, g_src, sig, s_src, cert, c_src in entries:
            if sig is not None:
                mg += ld(0x2A, ld(0x0A, key) + ld(0x12, sig))
                marks.append(("sig", s_src, len(mg) - 256, 256))
        out.lengths["multigrant"].append(len(mg))
        head = bytes([0x0A]) + varint(len(mg))
        body = bytearray(head + mg)
        for kind_, s, at, n in marks:
            out.runs.append(Run(kind_, s, pos + len(head) + at, n))
        for key, grant, g_src, sig, s_src, cert, c_src in entries:
            if not cert:
                continue
            ent = ld(0x0A, key) + ld(0x12, cert)
            out.lengths["cert_value"].append(len(cert))
            out.lengths["cert_entry"].append(len(ent))
            body += ld(0x12, ent)
            out.runs.append(Run("cert", c_src, pos + len(body) - len(cert), len(cert)))
        out.lengths["message"].append(len(body))
        out.bodies.append(bytes(body))
        pos += len(body)
    return out


def residues(runs: List[Run], kinds=("grant", "sig", "cert")) -> set:
    """(source mod 16, destination mod 16) of the payload runs of the given kinds."""
    return {(r.src % 16, r.dst % 16) for r in runs if r.kind in kinds and r.length}


# ---------------------------------------------------------------------------
# google.protobuf classes (dynamic descriptors; tests that use them start with
# pytest.importorskip("google.protobuf")).  A certificate is opaque to the
# encoder, so the currentCertificates value is declared `bytes` here: the same
# wire type as the WriteCertificate message, read back without a parse.
# ---------------------------------------------------------------------------
def classes():
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory

    T = descriptor_pb2.FieldDescriptorProto
    fdp = descriptor_pb2.FileDescriptorProto()
    fdp.name = "mochi_write1_reply_model.proto"
    fdp.package = PKG
    fdp.syntax = "proto3"
    e = fdp.enum_type.add()
    e.name = "OperationResultStatus"
    for nm, num in (("OK", 0), ("WRONG_SHARD", 1)):
        v = e.value.add()
        v.name, v.number = nm, num

    def msg(name, fields, nested=()):
        m = fdp.message_type.add()
        m.name = name
        for nd in nested:
            m.nested_type.add().CopyFrom(nd)
        for nm, num, ty, tn, label in fields:
            f = m.field.add()
            f.name, f.number, f.type, f.label = nm, num, ty, label
            if tn:
                f.type_name = tn
        return m

    def entry(name, vty, vtn):
        d = descriptor_pb2.DescriptorProto()
        d.name = name
        d.options.map_entry = True
        k = d.field.add()
        k.name, k.number, k.type, k.label = "key", 1, T.TYPE_STRING, T.LABEL_OPTIONAL
        v = d.field.add()
        v.name, v.number, v.type, v.label = "value", 2, vty, T.LABEL_OPTIONAL
        if vtn:
            v.type_name = vtn
        return d

    O, R = T.LABEL_OPTIONAL, T.LABEL_REPEATED
    p = "." + PKG + "."
    msg("Grant", [("objectId", 1, T.TYPE_STRING, "", O), ("timestamp", 2, T.TYPE_INT64, "", O),
                  ("configstamp", 3, T.TYPE_INT64, "", O), ("transactionHash", 4, T.TYPE_STRING, "", O),
                  ("status", 5, T.TYPE_ENUM, p + "OperationResultStatus", O)])
    msg("MultiGrant", [("grants", 1, T.TYPE_MESSAGE, p + "MultiGrant.GrantsEntry", R),
                       ("clientId", 2, T.TYPE_STRING, "", O), ("hash", 3, T.TYPE_STRING, "", O),
                       ("serverId", 4, T.TYPE_STRING, "", O),
                       ("grantSignatures", 5, T.TYPE_MESSAGE, p + "MultiGrant.GrantSignaturesEntry", R)],
        nested=[entry("GrantsEntry", T.TYPE_MESSAGE, p + "Grant"), entry("GrantSignaturesEntry", T.TYPE_BYTES, "")])
    msg("Write1OkFromServer", [("multiGrant", 1, T.TYPE_MESSAGE, p + "MultiGrant", O),
                               ("currentCertificates", 2, T.TYPE_MESSAGE,
                                p + "Write1OkFromServer.CurrentCertificatesEntry", R),
                               ("clientId", 3, T.TYPE_STRING, "", O), ("hash", 4, T.TYPE_STRING, "", O)],
        nested=[entry("CurrentCertificatesEntry", T.TYPE_BYTES, "")])
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fdp)
    get = lambda n: message_factory.GetMessageClass(pool.FindMessageTypeByName(PKG + "." + n))
    return get("Write1OkFromServer"), get("Grant")


# ---------------------------------------------------------------------------
# Inputs: a case = (batch, issued, source).  Signatures of the host form are
# stand-ins (no key on the host): 256 bytes derived from the grant's number.
# ---------------------------------------------------------------------------
def fake_sig(tag: int, i: int) -> bytes:
    return (hashlib.sha512(b"sig-%d-%d" % (tag, i)).digest() * 4)[:256]


def key_cert(key: bytes) -> bytes:
    """The container's current certificate: about three in four keys have one, 1..600 bytes."""
    h = hashlib.sha256(b"cert-of-" + key).digest()
    if h[0] % 4 == 0:
        return b""
    n = 1 + int.from_bytes(h[1:3], "little") % 600
    return (hashlib.sha512(h).digest() * (n // 64 + 1))[:n]


def stored_grants(store: M.Store, batch: mh.Write1Batch) -> List[bytes]:
    """Bytes of the batch's stored grants by stored index (after M.build_batch named them)."""
    out: List[Optional[bytes]] = [None] * batch.n_stored
    for c in store.data.values():
        for g in c.grants.values():
            if g.ref >= 0 and g.ref & mh.W1_STORED and (g.ref & ~mh.W1_STORED) < batch.n_stored:
                out[g.ref & ~mh.W1_STORED] = g.data
    assert all(x is not None for x in out)
    return out


def pack(items: List[bytes], pad=None):
    """items back to back (pad(i) filler bytes before the i-th): blob, offsets, lengths."""
    blob, off = bytearray(), []
    for i, x in enumerate(items):
        blob.extend(b"\xee" * (pad(i) if pad else 0))
        off.append(len(blob))
        blob.extend(x)
    return (np.frombuffer(bytes(blob) or b"\x00", np.uint8).copy(), np.array(off, np.uint64),
            np.array([len(x) for x in items], np.uint32))


def make_source(batch: mh.Write1Batch, stored: List[bytes], certs: bool = True, sigs: bool = True,
                cert_of=key_cert, client_of=None, server: bytes = SERVER_ID, pad=None) -> mh.Write1ReplySource:
    """Certificates by key (ops on one key share one slice: the slices alias), client ids by request."""
    Q, O = batch.n_reqs, batch.n_ops
    strings = np.asarray(batch.strings, np.uint8)
    client_of = client_of or (lambda q: b"" if q % 5 == 4 else b"client-%d" % (q * 7919 % 1000))
    ids, id_off, id_len = pack([server] + [client_of(q) for q in range(Q)], pad)
    s_blob, s_off, s_len = pack(stored, pad)
    op_cert_off = op_cert_len = None
    c_blob = np.zeros(1, np.uint8)
    if certs:
        keys = [strings[int(batch.op_key_off[o]):int(batch.op_key_off[o]) + int(batch.op_key_len[o])].tobytes()
                for o in range(O)]
        distinct = sorted(set(keys))
        c_blob, c_off, c_len = pack([cert_of(k) for k in distinct], pad)
        at = {k: i for i, k in enumerate(distinct)}
        op_cert_off = np.array([c_off[at[k]] for k in keys], np.uint64)
        op_cert_len = np.array([c_len[at[k]] for k in keys], np.uint32)
    return mh.Write1ReplySource(
        ids=ids, server_id_off=int(id_off[0]), server_id_len=int(id_len[0]), req_client_off=id_off[1:],
        req_client_len=id_len[1:], stored_bytes=s_blob, stored_off=s_off, stored_len=s_len,
        stored_sig=(np.frombuffer(b"".join(fake_sig(1, i) for i in range(len(stored))) or b"\x00" * 256,
                                  np.uint8).reshape(-1, 256).copy() if sigs else None),
        certs=c_blob, op_cert_off=op_cert_off, op_cert_len=op_cert_len)


def issue(batch: mh.Write1Batch, sigs: bool = True) -> mh.Write1Issued:
    issued = mh.write1_issue(batch)
    if sigs:
        issued.sig = np.frombuffer(b"".join(fake_sig(0, g) for g in range(issued.n_new)) or b"\x00" * 256,
                                   np.uint8).reshape(-1, 256).copy()
    return issued


def from_requests(store: M.Store, reqs, pad=None, certs: bool = True, sigs: bool = True, **kw):
    M.prepare(store, reqs)
    batch = M.build_batch(store, reqs, pad)
    return batch, issue(batch, sigs), make_source(batch, stored_grants(store, batch), certs, sigs, pad=pad, **kw)


def issue_cases(certs: bool = True, sigs: bool = True) -> dict:
    """Every case of write1_issue_model.all_cases() as reply inputs."""
    return {name: from_requests(store, reqs, pad, certs, sigs) for name, (store, reqs, pad) in M.all_cases().items()}


# ---- hand cases -----------------------------------------------------------------
def hand_cases() -> dict:
    R, W, D, RD = M.Request, M.WRITE, M.DELETE, M.READ
    H = M.H
    none = lambda q: b""
    c = {}
    c["ok_empty_no_ids"] = from_requests(M._store({}), [R(1, H(1), [(RD, b"x")]), R(2, H(2), [])], client_of=none,
                                         server=b"")
    c["ok_empty_ids"] = from_requests(M._store({}), [R(1, H(1), [(RD, b"x")]), R(2, H(2), [])],
                                      client_of=lambda q: b"client-%d" % q)
    c["throws"] = from_requests(M._store({}), [R(1, H(1), [(W, b"a"), (W, b"")]), R(1, H(2), [(D, b"gone")]),
                                               R(1, H(3), [(W, b"b")])])
    # refused by a stored grant AND by a grant request 0 of the same batch won
    c["refused_mixed"] = from_requests(M._store({b"a": 1000, b"b": 2000}, [(b"a", 5, H(9))]),
                                       [R(5, H(1), [(W, b"b")]), R(5, H(2), [(W, b"a"), (W, b"b")])])
    c["ok_64_ops"] = from_requests(M._store({}), [R(3, H(1), [(W, b"key-%02d" % i) for i in range(64)])])
    c["one_key_twice"] = from_requests(M._store({}), [R(2, H(1), [(W, b"g"), (W, b"g")]),
                                                      R(2, H(1), [(W, b"far1"), (D, b"far1")])])
    c["stored_shared"] = from_requests(M._store({b"s": 3000}, [(b"s", 1, H(1))]),
                                       [R(1, H(1), [(W, b"s")]), R(1, H(2), [(W, b"s")]), R(1, H(1), [(D, b"s"), (W, b"t")]),
                                        R(1, H(3), [(W, b"s"), (W, b"u")])])
    # every op of every request on one of two keys: the certificate slices alias across requests
    c["cert_alias"] = from_requests(M._store({}), [R(i, H(i), [(W, b"p"), (W, b"q")]) for i in range(6)],
                                    cert_of=lambda k: b"C" * 300 if k == b"p" else b"D" * 40)
    return c


# ---- varint steps -----------------------------------------------------------------
STEPS = (127, 128, 16383, 16384)


def _vs(v: int) -> int:
    return len(varint(v))


def _lds(n: int) -> int:
    return 1 + _vs(n) + n


def _grant_len(kl: int, hl: int, ts: int) -> int:
    return _lds(kl) + (1 + _vs(ts) if ts else 0) + (_lds(hl) if hl else 0)


def _solve(fn, target: int):
    """(key length, free length) with fn(kl, x) == target."""
    for kl in range(6, 40):
        for x in range(max(0, target - 200), target + 1):
            if fn(kl, x) == target:
                return kl, x
    raise AssertionError(f"no parameters reach {target}")


def step_cases() -> dict:
    """One-op requests (seed 1 on epoch 0: timestamp 1; no ids, no signatures) whose
    lengths fall on both sides of the one- / two- / three-byte varint steps."""
    R, W = M.Request, M.WRITE
    hash_of = lambda n: (b"0123456789abcdef" * (n // 16 + 1))[:n]
    reqs, cert_len = [], {}

    def add(kl, hl, cl):
        key = (b"s%03d" % len(reqs)).ljust(kl, b"x")
        assert len(key) == kl
        reqs.append(R(1, hash_of(hl), [(W, key)]))
        cert_len[key] = cl

    e1 = lambda kl, hl: _lds(kl) + _lds(_grant_len(kl, hl, 1))  # a grants entry
    for t in STEPS:
        add(*_solve(e1, t), 0)
        add(*_solve(lambda kl, hl: _lds(e1(kl, hl)), t), 0)  # the MultiGrant body
        add(8, 10, t)  # a certificate value
        kl, cl = _solve(lambda kl, cl: _lds(kl) + _lds(cl), t)  # a currentCertificates entry
        add(kl, 10, cl)
        msg = lambda kl, cl: _lds(_lds(e1(kl, 10))) + (_lds(_lds(kl) + _lds(cl)) if cl else 0)  # the message
        kl, cl = _solve(msg, t)
        add(kl, 10, cl)
    return {"steps": from_requests(M._store({}), reqs, sigs=False, client_of=lambda q: b"", server=b"",
                                   cert_of=lambda k: (b"\x5a" * cert_len[k]))}


CERT_LENS = (1, 15, 16, 17, 1023, 1024, 1025, 65537)


def cert_len_case():
    """Certificates on both sides of a 16-byte chunk, of a wave's 1 KiB stride and of 64 KiB."""
    R, W = M.Request, M.WRITE
    keys = [b"cl-%d" % n for n in CERT_LENS]
    want = dict(zip(keys, CERT_LENS))
    body = lambda k: (hashlib.sha512(k).digest() * (want[k] // 64 + 1))[:want[k]]
    return from_requests(M._store({}), [R(4, M.H(i), [(W, k)]) for i, k in enumerate(keys)], cert_of=body)


def alignment_case(n: int = 1400):
    """Requests of one to three ops with random key, hash, id and certificate lengths
    and random padding before every source slice: the payload runs land on every
    (source, destination) residue pair mod 16 (asserted by the tests)."""
    rng = np.random.default_rng(2718)
    R, W = M.Request, M.WRITE
    reqs = [R(int(rng.integers(0, 1 << 20)), M.H(i, int(rng.integers(1, 140))),
              [(W, (b"far" if (i + j) % 7 == 0 else b"al") + b"%d-%d" % (i, j) + b"y" * int(rng.integers(0, 30)))
               for j in range(int(rng.integers(1, 4)))]) for i in range(n)]
    pads = rng.integers(0, 16, 8 * n + 64)
    lens = {}

    def cert_of(k):
        if k not in lens:
            lens[k] = int(rng.integers(0, 400))
        return (hashlib.sha512(k).digest() * 7)[:lens[k]]

    return from_requests(M._store({}), reqs, pad=lambda i: int(pads[i % pads.size]), cert_of=cert_of,
                         client_of=lambda q: b"c" * (q % 23))


def reply_cases() -> dict:
    """The reply encoder's own case sets (beside issue_cases())."""
    c = dict(hand_cases())
    c.update(step_cases())
    c["cert_lens"] = cert_len_case()
    c["alignment"] = alignment_case()
    return c
