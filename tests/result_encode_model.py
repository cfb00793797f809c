"""The yardstick for the answer encoder (mochi_result_reply_encode[_device]): a plain-Python
writer of Write2AnsFromServer / ReadFromServer / TransactionResult / OperationResult from
Python values, written from MochiProtocol.proto:45-60, 82-87, 102-105 and the lines of
InMemoryDataStore.java that fill them (:521-574, :582-587, :641-666, :75-103, :201-231);
the google.protobuf classes it is cross-checked against (result_reply_model.classes); the
function that lays a list of answers out as the library's input arrays; and the case sets
the CPU and the GPU tests share.

TEST INFRASTRUCTURE: the library is never its own reference here.  The model goes from
values to bytes (one bytes object per message, joined); the library goes from slices and
flags to sizes, offsets and bytes in separate phases.  They share no code and no structure.
"""
from __future__ import annotations

import functools
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

import mochi_hip as mh
import result_reply_model as RRM

W2, RD, OTHER = mh.RR_WRITE2_ANS, mh.RR_READ, mh.RR_OTHER
FILL = 0xA5  # what the tests prefill every output with
MAX_MSG = 2 ** 31 - 1


class OpR(NamedTuple):
    """One OperationResult.  cert None: no currentCertificate; b"": the default instance."""
    status: int = 0
    result: bytes = b""
    existed: bool = False
    cert: Optional[bytes] = None
    # where the library is told to find the two slices: "w" wire, "s" store
    result_in: str = "w"
    cert_in: str = "w"


class Ans(NamedTuple):
    kind: int
    ops: Tuple[OpR, ...] = ()
    rid: bytes = b""
    nonce: bytes = b""  # a Write2AnsFromServer has no such field: ignored there


# ---------------------------------------------------------------------------
# the writer (proto3 as protobuf-java serializes: fields in number order, defaults omitted,
# a message field written whenever it was set)
# ---------------------------------------------------------------------------
def varint(v: int) -> bytes:
    out = bytearray()
    while v > 0x7F:
        out.append(0x80 | (v & 0x7F))
        v >>= 7
    out.append(v)
    return bytes(out)


def delimited(field: int, payload: bytes) -> bytes:
    return varint(field << 3 | 2) + varint(len(payload)) + payload


def operation_result(o: OpR) -> bytes:
    out = b""
    if o.result:  # string result = 1
        out += delimited(1, o.result)
    if o.cert is not None:  # WriteCertificate currentCertificate = 2: set, so written, also when empty
        out += delimited(2, o.cert)
    if o.existed:  # bool existed = 3
        out += varint(3 << 3) + b"\x01"
    if o.status:  # OperationResultStatus status = 4
        out += varint(4 << 3) + varint(o.status)
    return out


def _size(a: Ans) -> int:
    """len(message(a)) without building it (a test aliases one large certificate 64 times)."""
    tx = 0
    for o in a.ops:
        n = len(operation_result(o._replace(cert=None)))
        if o.cert is not None:
            n += 1 + len(varint(len(o.cert))) + len(o.cert)
        tx += 1 + len(varint(n)) + n
    tail = [a.nonce, a.rid] if a.kind == RD else [a.rid]
    return 1 + len(varint(tx)) + tx + sum(1 + len(varint(len(t))) + len(t) for t in tail if t)


def message(a: Ans) -> bytes:
    tx = b"".join(delimited(1, operation_result(o)) for o in a.ops)  # repeated OperationResult operations = 1
    out = delimited(1, tx)  # TransactionResult result = 1: setResult is always called
    if a.kind == RD:
        if a.nonce:
            out += delimited(2, a.nonce)
        if a.rid:
            out += delimited(3, a.rid)
    elif a.rid:
        out += delimited(2, a.rid)
    return out


def expected(answers: Sequence[Ans]):
    """(bodies, status): what the encoder must give per response."""
    bodies, status = [], []
    for a in answers:
        if a.kind == OTHER:
            bodies.append(b"")
            status.append(mh.ENC_OK)
        elif any(o.status == 0xFF for o in a.ops):
            bodies.append(b"")
            status.append(mh.ENC_BAD_OP)
        elif _size(a) > MAX_MSG:
            bodies.append(b"")
            status.append(mh.ENC_TOO_LONG)
        else:
            bodies.append(message(a))
            status.append(mh.ENC_OK)
    return bodies, np.array(status, np.uint8)


def expected_arrays(answers: Sequence[Ans]):
    """(wire, msg_off, msg_len, status): the bodies back to back in response order."""
    bodies, status = expected(answers)
    ln = np.array([len(b) for b in bodies], np.uint32)
    off = np.concatenate([[0], np.cumsum(ln.astype(np.uint64))[:-1]]).astype(np.uint64) if bodies else np.zeros(0, np.uint64)
    return np.frombuffer(b"".join(bodies), np.uint8), off, ln, status


# ---------------------------------------------------------------------------
# the values as the library's input
# ---------------------------------------------------------------------------
class _Blob:
    """Bytes at odd offsets; with `alias`, equal strings are stored once."""

    def __init__(self, alias: bool, lead: bytes):
        self.b, self.alias, self.where = bytearray(lead), alias, {}

    def put(self, s: bytes) -> int:
        if self.alias and s in self.where:
            return self.where[s]
        at = len(self.b)
        self.b += s
        if self.alias:
            self.where[s] = at
        else:
            self.b += b"\x5a"  # so that consecutive slices do not all share an alignment
        return at


def layout(answers: Sequence[Ans], alias: bool = False, slots: str = "dense", ids: bool = True) -> "mh.ResultAnswers":
    """alias  equal strings stored once (slices alias);
    slots  dense: slot runs back to back in response order; guarded: in descending order with
           three guard slots between the runs and before the first;
    ids    False: rid / nonce arrays NULL (every answer must then have none)."""
    answers = list(answers)
    P = len(answers)
    k = np.array([len(a.ops) for a in answers], np.int64)
    if slots == "dense":
        slot_off = np.concatenate([[0], np.cumsum(k)[:-1]]) if P else np.zeros(0, np.int64)
        S = int(k.sum())
    else:
        ends = np.cumsum((k + 3)[::-1])[::-1]  # response 0 last
        slot_off = ends - k
        S = int(ends[0]) if P else 0
    blobs = dict(w=_Blob(alias, b"\xa5"), s=_Blob(alias, b"\x5a\xa5\x5a"))
    idb = _Blob(alias, b"\xa5\xa5")
    arr = {nm: np.zeros(S, dt) for nm, (dt, w) in mh._RA_IN.items() if w == "S"}
    arr["op_status"][:] = 0xFF  # guards read absent: nobody may look at them
    rid = np.zeros((P, 2), np.uint64)
    nonce = np.zeros((P, 2), np.uint64)
    for p, a in enumerate(answers):
        if not ids:
            assert not a.rid and not a.nonce
        rid[p] = (idb.put(a.rid), len(a.rid))
        nonce[p] = (idb.put(a.nonce), len(a.nonce))
        for j, o in enumerate(a.ops):
            s = int(slot_off[p]) + j
            fl = 0
            arr["op_status"][s], arr["op_existed"][s] = o.status, int(o.existed)
            arr["op_result_off"][s], arr["op_result_len"][s] = blobs[o.result_in].put(o.result), len(o.result)
            fl |= mh.RAO_RESULT_STORE if o.result_in == "s" else 0
            if o.cert is not None:
                arr["op_cert_off"][s], arr["op_cert_len"][s] = blobs[o.cert_in].put(o.cert), len(o.cert)
                fl |= mh.RAO_HAS_CERT | (mh.RAO_CERT_STORE if o.cert_in == "s" else 0)
            arr["op_flags"][s] = fl
    u8 = lambda b: np.frombuffer(bytes(b.b), np.uint8)
    return mh.ResultAnswers(
        wire=u8(blobs["w"]), store=u8(blobs["s"]), ids=u8(idb), resp_kind=np.array([a.kind for a in answers], np.uint8),
        resp_n_ops=k.astype(np.uint32), slot_off=slot_off.astype(np.uint64),
        rid_off=rid[:, 0].copy() if ids else None, rid_len=rid[:, 1].astype(np.uint32) if ids else None,
        nonce_off=nonce[:, 0].copy() if ids else None, nonce_len=nonce[:, 1].astype(np.uint32) if ids else None, **arr)


# ---------------------------------------------------------------------------
# google.protobuf (tests that use it start with pytest.importorskip("google.protobuf"))
# ---------------------------------------------------------------------------
def protobuf_bytes(a: Ans) -> bytes:
    """The answer built with the google.protobuf classes and serialized by them."""
    C = RRM.classes()
    m = C["ReadFromServer" if a.kind == RD else "Write2AnsFromServer"]()
    m.result.SetInParent()
    for o in a.ops:
        r = m.result.operations.add()
        r.result = o.result.decode()
        if o.cert is not None:
            r.currentCertificate.SetInParent()
            r.currentCertificate.MergeFromString(o.cert)
        r.existed = bool(o.existed)
        r.status = o.status
    m.rid = a.rid.decode()
    if a.kind == RD:
        m.nonce = a.nonce.decode()
    return m.SerializeToString(deterministic=True)


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------
CERT = RRM.cert(1, 3)  # ~340 bytes
CERT4 = RRM.cert(2, 4, True)  # with signatures


def padded_cert(n: int) -> bytes:
    """n bytes that parse as a WriteCertificate (one unknown length-delimited field 15) for
    n != 1; n == 1 is a lone tag: opaque to the encoder, MALFORMED to the decoder."""
    if n == 0:
        return b""
    if n == 1:
        return b"\x7a"
    m = n - 2
    while 1 + len(varint(m)) + m > n:
        m -= 1
    out = b"\x7a" + varint(m) + b"c" * m
    return out + b"\x78\x00" * ((n - len(out)) // 2) if len(out) < n else out


def text(n: int, seed: int = 0) -> bytes:
    return bytes(0x61 + (i * 7 + seed) % 26 for i in range(n))


def _subsets() -> Tuple[OpR, ...]:
    return tuple(OpR(status=1 if m & 8 else 0, result=b"value-%d" % m if m & 1 else b"", existed=bool(m & 4),
                     cert=CERT if m & 2 else None) for m in range(16))


def _result_len_for_body(n: int) -> int:
    """The `result` length that makes an OperationResult with that field alone n bytes long."""
    r = n - 2
    while 1 + len(varint(r)) + r > n:
        r -= 1
    assert 1 + len(varint(r)) + r == n
    return r


def _result_len_for_tx(n: int) -> int:
    """... that makes a TransactionResult of that one operation n bytes long."""
    b = n - 2
    while 1 + len(varint(b)) + b > n:
        b -= 1
    assert 1 + len(varint(b)) + b == n
    return _result_len_for_body(b)


EDGES = (0, 1, 127, 128, 16383, 16384)


@functools.lru_cache(maxsize=None)
def cases() -> Dict[str, Tuple[Ans, ...]]:
    c: Dict[str, Tuple[Ans, ...]] = {}
    two = (OpR(0, b"written", True, CERT), OpR(1))
    c["one"] = (Ans(W2, two, b"rid-1"),)
    c["other_between"] = (Ans(W2, two, b"rid-1"), Ans(OTHER, two, b"rid-x", b"n"), Ans(RD, two[:1], b"rid-2", b"nonce-2"))
    c["ops_0"] = (Ans(W2, (), b"r"), Ans(RD, (), b"r", b"n"), Ans(W2), Ans(RD))
    c["ops_64"] = (Ans(W2, tuple(OpR(i & 1, b"r%d" % i, i % 3 == 0, CERT if i % 5 == 0 else None) for i in range(64)), b"r"),
                   Ans(RD, tuple(OpR(0, b"v", True, CERT) for _ in range(64)), b"r", b"n"))
    c["field_subsets"] = (Ans(W2, _subsets(), b"rid"),) + tuple(Ans(RD, (o,), b"r", b"n") for o in _subsets())
    c["cert_empty"] = (Ans(RD, (OpR(0, b"v", True, b""), OpR(0, b"", False, b"")), b"r", b"n"),)
    c["status"] = (Ans(W2, tuple(OpR(s, b"x") for s in (1, 2, 127, 128, 254)), b"r"),)
    c["bad_op"] = (Ans(W2, two, b"r1"), Ans(W2, (OpR(0, b"a"), OpR(0xFF, b"b"), OpR(1)), b"r2"), Ans(RD, two, b"r3", b"n3"),
                   Ans(RD, (OpR(0xFF),), b"r4"))
    c["ids"] = tuple(Ans(kind, two, rid, nonce) for kind in (W2, RD) for rid in (b"", b"rid-7") for nonce in (b"", b"nonce-7"))
    c["len_result"] = tuple(Ans(W2, (OpR(0, text(n), True),), b"r") for n in EDGES)
    c["len_cert"] = tuple(Ans(RD, (OpR(0, b"v", True, padded_cert(n)),), b"r", b"n") for n in EDGES)
    c["len_op"] = tuple(Ans(W2, (OpR(0, text(_result_len_for_body(n))), OpR(1)), b"r") for n in EDGES[2:])
    c["len_tx"] = tuple(Ans(W2, (OpR(0, text(_result_len_for_tx(n))),), b"r") for n in EDGES[2:]) + (Ans(W2, (OpR(),)),)
    c["sources"] = (Ans(W2, (OpR(0, b"from-wire", True, CERT, "w", "w"), OpR(0, b"from-store", True, CERT4, "s", "s"),
                             OpR(0, b"mixed-1", False, CERT, "s", "w"), OpR(0, b"mixed-2", True, CERT4, "w", "s")), b"r"),)
    c["unicode"] = (Ans(RD, (OpR(0, RRM.K2, True, CERT),), "rïd".encode(), "nonce-€".encode()),)
    return c


def all_answers() -> Tuple[Ans, ...]:
    return tuple(a for v in cases().values() for a in v)


COPY_EDGE_LENS = (0, 1, 15, 16, 17, 1023, 1024, 1025, 3071, 3072, 3073)


def copy_edge():
    """(answers, their layout): certificates at the chunk and wave-round edges of the copy
    kernel, each at every source misalignment 0..15 (its offset in `wire` or `store` is
    congruent to it mod 16; the two blobs alternate).  The destination misalignments are the
    caller's: it shifts the output buffer."""
    answers = []
    for n in COPY_EDGE_LENS:
        cert = bytes((i * 131 + n) & 0xFF for i in range(n))
        for shift in range(16):
            answers.append(Ans(RD, (OpR(0, text(shift % 5, n), True, cert, "w", "ws"[shift & 1]),), b"r", b"n"))
    ra = layout(answers)
    blobs = dict(w=bytearray(ra.wire.tobytes()), s=bytearray(ra.store.tobytes()))
    for i, a in enumerate(answers):
        b = blobs[a.ops[0].cert_in]
        b += b"\x5a" * ((i % 16 - len(b)) % 16)
        ra.op_cert_off[i] = len(b)
        b += a.ops[0].cert
    ra.wire, ra.store = (np.frombuffer(bytes(blobs[k]), np.uint8) for k in "ws")
    return tuple(answers), ra
