"""The yardstick for the Write2 answer plan (mochi_write2_answer_plan[_device]): what the
reference's server does with an accepted Write2ToServer, as a per-message walk over Python
dictionaries, written from InMemoryDataStore.java (processWrite2ToServer :641-666,
applyOperation / readOperation :521-574, the WRONG_SHARD branch :582-587) and
StoreValueObjectContainer.java:91-94; the Write2AnsFromServer the server then builds, at
the level of values (result_encode_model writes its bytes); and the case set the CPU and the
GPU tests share.

TEST INFRASTRUCTURE: the library is never its own reference here.  The model parses a body
into a tree first (write1_decode_model.fields) and reads the message off that tree; it
shares no code and no structure with the library's walk.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

import mochi_hip as mh
import result_encode_model as E
import result_reply_model as RRM
import write1_decode_model as DM

READ, DELETE, WRITE = 0, 1, 2  # OperationAction, MochiProtocol.proto:20-24
APPLY, RD, WS, FAILED, SKIPPED = mh.OPD_APPLY, mh.OPD_READ, mh.OPD_WRONG_SHARD, mh.OPD_FAILED, mh.OPD_SKIPPED
FILL = 0xA5
ABSENT = dict(op_status=0xFF, op_existed=0, op_flags=0, op_result_off=0, op_result_len=0, op_cert_off=0, op_cert_len=0)


class Stored(NamedTuple):
    """The key's container as the op flags' snapshot saw it."""
    value: Optional[bytes] = b""  # None: getValue() is null
    cert: Optional[bytes] = None  # None: no stored certificate


class Tx(NamedTuple):
    name: str
    body: bytes
    decisions: Tuple[int, ...]  # per op of op_flags_off
    store: Tuple[Stored, ...]
    msg_status: int = mh.MSG_OK
    accepted: bool = True


# ---------------------------------------------------------------------------
# the message as a dictionary
# ---------------------------------------------------------------------------
def parse(body: bytes) -> Optional[dict]:
    """{"cert": (off, len) or None, "ops": [{"action", "operand2": (off, len) or None, "at": off}]},
    every singular field at its last occurrence; None where the parser throws."""
    try:
        msg = dict(cert=None, ops=[])
        tx = None
        for f, wt, v, po, pl in DM._msg(body, 0, len(body)):
            if wt == 2 and f == 1:
                msg["cert"] = (po, pl)
            elif wt == 2 and f == 2:
                tx = (po, pl)
        if tx:
            for f, wt, v, po, pl in DM._msg(body, *tx):
                if f != 1 or wt != 2:
                    continue
                op = dict(action=0, operand2=None, at=po)
                for g, gwt, gv, go, gl in DM._msg(body, po, pl):
                    if g == 1 and gwt == 0:
                        op["action"] = gv & 0xFFFFFFFF
                    elif g == 3 and gwt == 2:
                        op["operand2"] = (go, gl)
                msg["ops"].append(op)
        return msg
    except DM.Malformed:
        return None


def plan(t: Tx):
    """(plan status, per op a dict of values or None): what the server answers.
    An op's dict: status, existed, and `result` / `cert` as ("w" | "s", bytes or None)."""
    k = len(t.decisions)
    if t.msg_status == mh.MSG_FALLBACK:
        return (mh.W2A_HOST if t.accepted else mh.W2A_NO_REPLY), None
    if t.msg_status != mh.MSG_OK or not t.accepted:
        return mh.W2A_NO_REPLY, None  # never reached the store, or processWrite2ToServer threw
    msg = parse(t.body)
    if msg is None or len(msg["ops"]) != k:
        return mh.W2A_NO_REPLY, None
    out = []
    for op, d, sv in zip(msg["ops"], t.decisions, t.store):
        if d == WS:  # :582-587: status alone
            out.append(dict(status=1, existed=False, result=("w", None), cert=("w", None), has_cert=False))
        elif d == APPLY:  # :521-552: the incoming certificate, operand2, setValueAvailble's argument
            o2 = op["operand2"]
            out.append(dict(status=0, existed=op["action"] == WRITE, has_cert=True,
                            result=("w", o2 if o2 else (op["at"], 0)), cert=("w", msg["cert"] or (0, 0))))
        elif d == RD:  # :556-574: the stored value and certificate
            if sv.value is None:
                return mh.W2A_NO_REPLY, None  # setResult(null) throws
            out.append(dict(status=0, existed=True, has_cert=sv.cert is not None, result=("s", sv.value), cert=("s", sv.cert)))
        else:
            return mh.W2A_NO_REPLY, None  # FAILED / SKIPPED: the reference threw here
    return mh.W2A_REPLY, out


def server_answer(t: Tx) -> Optional[E.Ans]:
    """The Write2AnsFromServer of the transaction as values, or None where no reply is sent
    (the HOST case included: the caller builds that one)."""
    st, ops = plan(t)
    if st != mh.W2A_REPLY:
        return None
    sl = lambda s: t.body[s[0]:s[0] + s[1]]
    res = []
    for o in ops:
        if o["status"]:
            res.append(E.OpR(1))
        elif o["result"][0] == "w":
            res.append(E.OpR(0, sl(o["result"][1]), o["existed"], sl(o["cert"][1])))
        else:
            res.append(E.OpR(0, o["result"][1], True, o["cert"][1], "s", "s"))
    return E.Ans(E.W2, tuple(res))


# ---------------------------------------------------------------------------
# a list of transactions as the library's input, and the arrays it must give
# ---------------------------------------------------------------------------
def batch(txs, slots: str = "dense"):
    """(WireBatch-like namespace, msg_status, accept_bits, op_decision, mh.Write2AnswerStore)."""
    txs = list(txs)
    M = len(txs)
    k = np.array([len(t.decisions) for t in txs], np.int64)
    blob, off = b"\xa5", []
    for t in txs:
        off.append(len(blob))
        blob += t.body + b"\x5a"
    fo = np.concatenate([[0], np.cumsum(k)]).astype(np.uint32)
    O = int(fo[-1])
    wb = SimpleNamespace(wire=np.frombuffer(blob, np.uint8).copy(), msg_off=np.array(off, np.uint64),
                         msg_len=np.array([len(t.body) for t in txs], np.uint32), op_flags_off=fo,
                         op_flags=np.full(max(O, 1), mh.OP_LOCAL | mh.OP_HAS_SVOC, np.uint8),
                         expected_hash=np.zeros((M, 128), np.uint8), op_object_ts=None, n_msgs=M)
    bits = np.zeros(max((M + 31) // 32, 1), np.uint32)
    for m, t in enumerate(txs):
        if t.accepted:
            bits[m >> 5] |= np.uint32(1 << (m & 31))
    store, val, cert, fl = b"\x5a\x5a\x5a", np.zeros((O, 2), np.uint64), np.zeros((O, 2), np.uint64), np.zeros(O, np.uint8)
    i = 0
    for t in txs:
        assert len(t.store) == len(t.decisions)
        for sv in t.store:
            if sv.value is None:
                fl[i] |= mh.W2A_VALUE_NULL
            else:
                val[i] = (len(store), len(sv.value))
                store += sv.value + b"\xa5"
            if sv.cert is not None:
                fl[i] |= mh.W2A_HAS_STORED_CERT
                cert[i] = (len(store), len(sv.cert))
                store += sv.cert
            i += 1
    if slots == "dense":
        slot_off, S = fo[:-1].astype(np.uint64), O
    else:
        ends = np.cumsum((k + 3)[::-1])[::-1]
        slot_off, S = (ends - k).astype(np.uint64), int(ends[0]) if M else 0
    st = mh.Write2AnswerStore(store=np.frombuffer(store, np.uint8), op_value_off=val[:, 0].copy(),
                              op_value_len=val[:, 1].astype(np.uint32), op_stored_cert_off=cert[:, 0].copy(),
                              op_stored_cert_len=cert[:, 1].astype(np.uint32), op_store_flags=fl, slot_off=slot_off, n_slots=S)
    return (wb, np.array([t.msg_status for t in txs], np.uint8), bits,
            np.array([d for t in txs for d in t.decisions], np.uint8), st)


def expected(txs, wb, st: "mh.Write2AnswerStore", fill: int = FILL) -> dict:
    """The arrays of mochi_write2_answer_planned over buffers prefilled with `fill`."""
    txs = list(txs)
    n = dict(M=len(txs), S=int(st.n_slots))
    arr = {k: np.full(n[w] * np.dtype(dt).itemsize, fill, np.uint8).view(dt) for k, (dt, w) in mh._W2A_OUT.items()}
    i = 0
    for m, t in enumerate(txs):
        status, ops = plan(t)
        k, s0, base = len(t.decisions), int(st.slot_off[m]), int(wb.msg_off[m])
        arr["plan_status"][m] = status
        arr["resp_kind"][m] = E.W2 if status == mh.W2A_REPLY else E.OTHER
        arr["resp_n_ops"][m] = k if status == mh.W2A_REPLY else 0
        for j in range(k):
            if ops is None:
                vals = ABSENT
            else:
                o = ops[j]
                vals = dict(op_status=o["status"], op_existed=int(o["existed"]), op_flags=0, op_result_off=0, op_result_len=0,
                            op_cert_off=0, op_cert_len=0)
                if o["status"] == 0 and o["result"][0] == "w":
                    vals.update(op_flags=mh.RAO_HAS_CERT, op_result_off=base + o["result"][1][0], op_result_len=o["result"][1][1],
                                op_cert_off=base + o["cert"][1][0], op_cert_len=o["cert"][1][1])
                elif o["status"] == 0:
                    vals.update(op_flags=mh.RAO_RESULT_STORE | mh.RAO_CERT_STORE | (mh.RAO_HAS_CERT if o["has_cert"] else 0),
                                op_result_off=int(st.op_value_off[i + j]), op_result_len=int(st.op_value_len[i + j]),
                                op_cert_off=int(st.op_stored_cert_off[i + j]) if o["has_cert"] else 0,
                                op_cert_len=int(st.op_stored_cert_len[i + j]) if o["has_cert"] else 0)
            for nm, v in vals.items():
                arr[nm][s0 + j] = v
        i += k
    return arr


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------
ld = lambda tag, b: bytes([tag]) + E.varint(len(b)) + b
CERT = RRM.cert(2, 4, True)
STORED = RRM.cert(1, 3)


def operation(action: int, key: bytes, value: bytes = b"", raw: bytes = b"") -> bytes:
    return (b"\x08" + E.varint(action) if action else b"") + (ld(0x12, key) if key else b"") + (ld(0x1A, value) if value else b"") + raw


def write2(cert: Optional[bytes], ops, raw: bytes = b"") -> bytes:
    return (ld(0x0A, cert) if cert is not None else b"") + ld(0x12, b"".join(ld(0x0A, o) for o in ops)) + raw


def _tx(name, ops, decisions, store=None, cert=CERT, **kw) -> Tx:
    store = tuple(store) if store is not None else tuple(Stored(b"old-%d" % j, STORED) for j in range(len(decisions)))
    return Tx(name, write2(cert, ops), tuple(decisions), store, **kw)


@functools.lru_cache(maxsize=None)
def cases() -> Tuple[Tx, ...]:
    w = lambda j, v=None: operation(WRITE, b"key-%d" % j, b"value-%d" % j if v is None else v)
    three = [w(0), w(1), w(2)]
    c: List[Tx] = [
        _tx("apply:all", three, [APPLY] * 3),
        _tx("apply:one", [w(0)], [APPLY]),
        _tx("apply:64", [w(j) for j in range(64)], [APPLY] * 64),
        _tx("ws:all_no_cert", three, [WS] * 3, cert=None),
        _tx("mixed", three + [w(3)], [APPLY, RD, WS, APPLY]),
        _tx("delete", [operation(DELETE, b"key-0"), w(1)], [APPLY, APPLY]),
        _tx("read:stored_cert", [w(0)], [RD], [Stored(b"stored-value", STORED)]),
        _tx("read:no_stored_cert", [w(0), w(1)], [RD, RD], [Stored(b"v", None), Stored(b"", None)]),
        _tx("read:value_null", [w(0), w(1)], [APPLY, RD], [Stored(), Stored(None, STORED)]),
        _tx("apply:value_null_is_fine", [w(0)], [APPLY], [Stored(None, None)]),
        _tx("not_accepted", three, [APPLY] * 3, accepted=False),
        _tx("failed:middle", three, [APPLY, FAILED, SKIPPED]),
        _tx("skipped:first", three, [SKIPPED] * 3),
        _tx("status:malformed", three, [SKIPPED] * 3, msg_status=mh.MSG_MALFORMED, accepted=False),
        _tx("status:malformed_accepted", three, [APPLY] * 3, msg_status=mh.MSG_MALFORMED),
        _tx("status:ops_mismatch", three, [APPLY] * 3, msg_status=mh.MSG_OPS_MISMATCH),
        _tx("status:fallback_accepted", three, [APPLY] * 3, msg_status=mh.MSG_FALLBACK),
        _tx("status:fallback_rejected", three, [SKIPPED] * 3, msg_status=mh.MSG_FALLBACK, accepted=False),
        _tx("operand2:absent", [operation(WRITE, b"key-0"), w(1)], [APPLY, APPLY]),
        _tx("operand2:twice", [operation(WRITE, b"k", b"first", ld(0x1A, b"the-last-one")), w(1)], [APPLY, APPLY]),
        _tx("operand2:foreign_wire_type", [operation(WRITE, b"k", b"", b"\x18\x07"), operation(WRITE, b"k", b"kept", b"\x1d" + bytes(4))],
            [APPLY, APPLY]),
        _tx("action:twice", [operation(WRITE, b"k", b"v", b"\x08\x01"), operation(DELETE, b"k", b"v", b"\x08\x02")], [APPLY, APPLY]),
        _tx("action:foreign_wire_type", [operation(0, b"k", b"v", ld(0x0A, b"\x02")), w(1)], [APPLY, APPLY]),
        _tx("action:10_byte_varint", [operation(0, b"k", b"v", b"\x08\x82" + b"\x80" * 3 + b"\xf0" + b"\xff" * 4 + b"\x01")], [APPLY]),
        Tx("cert:after_transaction", ld(0x12, ld(0x0A, w(0))) + ld(0x0A, CERT), (APPLY,), (Stored(),)),
        Tx("cert:twice_last_wins", ld(0x0A, STORED) + ld(0x12, ld(0x0A, w(0))) + ld(0x0A, CERT), (APPLY,), (Stored(),)),
        _tx("cert:empty", [w(0)], [APPLY], cert=b""),
        Tx("unknown:top", b"\x28\x01" + RRM.groups(2) + write2(CERT, three, ld(0x32, b"\xff") + b"\x3d" + bytes(4)), (APPLY,) * 3,
           (Stored(),) * 3),
        Tx("unknown:in_tx_and_op", ld(0x0A, CERT) + ld(0x12, ld(0x12, b"\xff") + ld(0x0A, w(0) + RRM.groups(3) + b"\x30\x01") +
                                                     b"\x08\x05" + ld(0x0A, w(1) + ld(0x22, b"\xfe"))), (APPLY, RD), (Stored(), Stored(b"s", STORED))),
        _tx("count:one_more_on_the_wire", three, [APPLY, APPLY]),
        _tx("count:one_fewer_on_the_wire", three[:2], [APPLY] * 3),
        _tx("count:none_of_none", [], []),
        Tx("count:no_transaction", ld(0x0A, CERT), (), ()),
        Tx("walk:truncated", write2(CERT, three)[:-3], (APPLY,) * 3, (Stored(),) * 3),
        Tx("walk:bad_op_inside", ld(0x12, ld(0x0A, b"\x1a\x7fxx")), (APPLY,), (Stored(),)),
        Tx("walk:empty_body", b"", (), ()),
    ]
    return tuple(c)
