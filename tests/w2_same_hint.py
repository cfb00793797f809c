"""The Write2 wire decoder's first-grant hint (`grant_same`) pinned to the
grant bytes: message builders, a model-free checker and a completeness model.  No GPU.

k_w2_mg compares each MultiGrant's grant with the first grant of its message (mg_match from
64-byte windows, the walk with bytes_equal), k_w2_emit_mg hands the result to grant prep as
grant_same[g] -- g itself, or the index of the message's first grant -- and k_grant_prep_cert
then gives g the first grant's digest, timestamp and flags WITHOUT comparing a byte.

  check_hint()        soundness: a hint names the message's first grant, which lies before g
                      and holds g's bytes.  Needs no model of the decoder.
  model_violations()  completeness, on the messages qualifies() accepts: hinted if and only if
                      the bytes are equal (a lost hint costs prep its dedup, nothing else shows it).
  sweep()             R = 4, one op: at every grant length around the compare's edges, one
                      message per byte position p, one replica's grant differing from the
                      first grant's in byte p alone; plus variants in the first grant itself,
                      longer variants and four equal grants.
  adversaries()       first MultiGrants whose first grants entry is NOT the message's first
                      decoded grant, or that the hint's reference parse declines.

test_w2_same_hint_cpu.py asserts what the builders cover (oracle only);
test_w2_same_hint_gpu.py runs the decoder and the verify path on them.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Iterable, List, Optional, Tuple

import numpy as np

import oracle_ffi as O
import workload as W

R = 4
IDS4 = W.SERVER_IDS[:R]
TS = 1000  # a two-byte varint (0xE8 0x07): either byte XOR 1 is still a minimal varint
MSG_OK, MSG_FALLBACK = 0, 2  # enum mochi_msg_status

# Grant length -> (objectId length, transactionHash length) of encode_grant("K" * L, TS, "h" * hl):
# gl = 2 + L + 3 + (2 or 3) + hl.  63/64/65, 127/128/129 and 191/192 lie on either side of
# mg_match's 64-byte windows; 127 -> 128 grows the grant-length varint to two bytes (ref_head's
# mask); 192 -> 193 leaves the matcher for the walk.  The three longest carry a two-byte hash length.
SHAPES = {20: (7, 6), 63: (30, 26), 64: (30, 27), 65: (30, 28), 127: (60, 60), 128: (60, 61), 129: (60, 62),
          191: (53, 130), 192: (54, 130), 193: (55, 130)}
REAL_OID, REAL_TXN = "DEMO_KEY_TEST_7", 7  # the real shape: a 128-hex transaction hash
REAL_GL = 2 + len(REAL_OID) + 3 + 3 + 128
GLS = tuple(sorted(list(SHAPES) + [REAL_GL]))
KLS = (4, 60)  # grants-entry key lengths: the entry length L1 turns two bytes at other grant lengths
# Of a grant's gl positions, those whose XOR 1 is not a canonical grant of the same shape: the three
# tags, the objectId length and the one or two hash-length bytes.  Every other position holds
# ASCII (stays ASCII) or the timestamp varint (stays minimal).
MAX_STRUCTURAL = 6


def base_grant(gl: int) -> bytes:
    if gl == REAL_GL:
        return W.encode_grant(REAL_OID, TS, W.txn_hash_hex(REAL_TXN))
    L, hl = SHAPES[gl]
    return W.encode_grant("K" * L, TS, "h" * hl)


def expected_hash(gl: int) -> bytes:
    """The real shape's own hash; the synthetic shapes' hashes are not 128 bytes, so no value matches."""
    return (W.txn_hash_hex(REAL_TXN) if gl == REAL_GL else "0" * 128).encode()


def flip(gb: bytes, p: int) -> bytes:
    return gb[:p] + bytes([gb[p] ^ 0x01]) + gb[p + 1:]


def unsigned(r: int, gb: bytes) -> bytes:
    """Decode never reads a signature's bytes: any 256 will do."""
    return bytes([0x41 + r]) * 256


@dataclass(frozen=True)
class Msg:
    kind: str            # "flip", "flip_first", "longer_unknown", "longer_status", "equal", "adv:<name>:<first|last>"
    gl: int              # the base grant's length
    kl: int              # the grants-entry key's length
    p: int               # the differing byte position, -1 = none
    grants: Tuple[bytes, ...]  # sweep: replica r's grant bytes
    data: bytes
    hash: bytes          # the certificate's expected transaction hash
    n_ops: int = 1


def one_grant_mg(r: int, key: str, gb: bytes, sign: Callable[[int, bytes], bytes]) -> bytes:
    """The reference encoder's MultiGrant of replica r: one grant, its signature under the grant's key."""
    return W.encode_multigrant([(key, gb)], IDS4[r], "", "", [(key, sign(r, gb))])


def message(key: str, grants, sign: Callable[[int, bytes], bytes]) -> bytes:
    ent = [(IDS4[r], one_grant_mg(r, key, gb, sign)) for r, gb in enumerate(grants)]
    return W.encode_write2(ent, [W.encode_operation(2, key)])


def sweep(sign: Callable[[int, bytes], bytes] = unsigned,
          positions: Optional[Callable[[int], Iterable[int]]] = None) -> List[Msg]:
    """The sweep in a fixed order; positions(gl): the flip positions to build (None: every one)."""
    out = []
    for kl in KLS:
        key = "q" * kl
        for gl in GLS:
            base, h = base_grant(gl), expected_hash(gl)
            assert len(base) == gl

            def add(kind, p, grants):
                out.append(Msg(kind, gl, kl, p, tuple(grants), message(key, grants, sign), h))

            for p in (range(gl) if positions is None else sorted(set(q for q in positions(gl) if 0 <= q < gl))):
                grants = [base] * R
                grants[1 + p % 3] = flip(base, p)
                add("flip", p, grants)
            for p in (0, gl // 2, gl - 1):  # nobody equals the first grant
                add("flip_first", p, [flip(base, p)] + [base] * (R - 1))
            add("longer_unknown", -1, [base, base + b"\x30\x01", base, base])  # field 6: parses, not canonical
            add("longer_status", -1, [base, base, base + b"\x28\x01", base])   # Grant.status = 1: canonical
            add("equal", -1, [base] * R)
    return out


VERDICT_POSITIONS = (0, 1, 2, 3, 62, 63, 64, 65, 126, 127, 128, 129)


def verdict_positions(gl: int) -> Iterable[int]:
    """The flip positions of the verdict leg: every one of the real shape, the edges of the others."""
    return range(gl) if gl == REAL_GL else VERDICT_POSITIONS + (gl - 2, gl - 1)


# ---------------------------------------------------------------------------
# Reference-grant adversaries
# ---------------------------------------------------------------------------
def _rd_varint(b: bytes, i: int) -> Tuple[int, int]:
    v, sh = 0, 0
    while True:
        if i >= len(b) or sh > 63:
            raise ValueError("varint")
        c = b[i]
        v |= (c & 0x7F) << sh
        sh += 7
        i += 1
        if not c & 0x80:
            return v, i


def walk(b: bytes):
    """(field, wire type, value or payload, raw field bytes) of protobuf bytes; ValueError on a
    group, an unknown wire type or a truncated field."""
    i, n = 0, len(b)
    while i < n:
        i0 = i
        t, i = _rd_varint(b, i)
        f, wt = t >> 3, t & 7
        if wt == 0:
            v, i = _rd_varint(b, i)
        elif wt == 1:
            v, i = b[i:i + 8], i + 8
        elif wt == 5:
            v, i = b[i:i + 4], i + 4
        elif wt == 2:
            ln, i = _rd_varint(b, i)
            v, i = b[i:i + ln], i + ln
        else:
            raise ValueError("wire type")
        if i > n or f == 0:
            raise ValueError("truncated")
        yield f, wt, v, b[i0:i]


def reorder(gb: bytes) -> bytes:
    """A canonical Grant with its fields written in reverse order (the same parsed Grant)."""
    return b"".join(raw for _, _, _, raw in reversed(list(walk(gb))))


def adversaries(sign: Callable[[int, bytes], bytes] = unsigned) -> List[Msg]:
    """Two messages per form: the three followers carry the bytes of the first MultiGrant's
    first value (A) in the first message and of its last value (B) in the second.  Where the
    first MultiGrant holds one value only, B is that value with its timestamp one higher."""
    key, h = "q" * 4, W.txn_hash_hex(REAL_TXN)
    A = W.encode_grant(REAL_OID, TS, h)
    B = W.encode_grant(REAL_OID, TS + 1, h)
    A193 = W.encode_grant("K" * 57, TS, h)
    B193 = W.encode_grant("K" * 57, TS + 1, h)
    assert len(A193) == 193
    sid0 = IDS4[0]

    def sig_entry(k, gb, r=0):
        return W.encode_map_entry(5, k.encode(), sign(r, gb))

    def mg0_two_values_one_entry():
        ent = W._ld(1, W._ld(1, key.encode()) + W._ld(2, A) + W._ld(2, B))
        return ent + W._ld(4, sid0.encode()) + sig_entry(key, B)

    key128 = "q" * 128
    forms = {
        # name: (first MultiGrant, extra certificate entries, op keys, grants key of the followers, (A, B))
        "repeated_grant_key": (W.encode_multigrant([(key, A), (key, B)], sid0, "", "", [(key, sign(0, B))]), [], [key], key, (A, B)),
        "value_twice_in_entry": (mg0_two_values_one_entry(), [], [key], key, (A, B)),
        "two_grant_keys": (W.encode_multigrant([(key, A), (key + "2", B)], sid0, "", "",
                                               [(key, sign(0, A)), (key + "2", sign(0, B))]), [], [key, key + "2"], key, (A, B)),
        "cert_key_repeated": (one_grant_mg(0, key, A, sign), [(sid0, one_grant_mg(0, key, B, sign))], [key], key, (A, B)),
        "server_id_first": (W._ld(4, sid0.encode()) + W.encode_map_entry(1, key.encode(), A) + sig_entry(key, A),
                            [], [key], key, (A, B)),
        "grant_key_128": (one_grant_mg(0, key128, A, sign), [], [key128], key128, (A, B)),
        # the signature covers Grant.toByteArray(), the canonical bytes
        "first_grant_reordered": (W.encode_multigrant([(key, reorder(A))], sid0, "", "", [(key, sign(0, A))]), [], [key], key,
                                  (reorder(A), A)),
        "first_grant_193": (one_grant_mg(0, key, A193, sign), [], [key], key, (A193, B193)),
    }
    out = []
    for name, (mg0, extra, op_keys, fkey, values) in forms.items():
        for which, gb in zip(("first", "last"), values):
            signed = A if name == "first_grant_reordered" else gb
            ent = [(sid0, mg0)]
            for r in range(1, R):
                ent.append((IDS4[r], W.encode_multigrant([(fkey, gb)], IDS4[r], "", "", [(fkey, sign(r, signed))])))
            data = W.encode_write2(ent + extra, [W.encode_operation(2, k) for k in op_keys])
            out.append(Msg(f"adv:{name}:{which}", len(values[0]), len(fkey), -1, (), data, h.encode(), len(op_keys)))
    return out


# ---------------------------------------------------------------------------
# Layout
# ---------------------------------------------------------------------------
def pack(msgs: List[Msg], with_ops: bool = False) -> W.WireBatch:
    """Message i after a pad of i % 16 bytes: the offsets take every residue mod 16.  with_ops:
    caller op arrays, one operation per message, LOCAL | HAS_SVOC, no stored certificate."""
    off, parts, pos = [], [], 0
    for i, m in enumerate(msgs):
        parts.append(b"\xee" * (i % 16))
        pos += i % 16
        off.append(pos)
        parts.append(m.data)
        pos += len(m.data)
    M = len(msgs)
    ofo = np.zeros(M + 1, np.uint32)
    np.cumsum([m.n_ops for m in msgs], out=ofo[1:])
    return W.WireBatch(wire=np.frombuffer(b"".join(parts) or b"\x00", np.uint8).copy(), msg_off=np.array(off, np.uint64),
                       msg_len=np.array([len(m.data) for m in msgs], np.uint32), op_flags_off=ofo if with_ops else None,
                       op_flags=np.full(int(ofo[-1]) if with_ops else 1, 3, np.uint8),
                       expected_hash=np.stack([np.frombuffer(m.hash, np.uint8) for m in msgs]).copy(),
                       op_object_ts=np.zeros(int(ofo[-1]), np.int64) if with_ops else None)


def tiles(msgs: List[Msg], M: int) -> List[List[Msg]]:
    """msgs cut into batches of exactly M messages (the last one filled up from the start)."""
    n = len(msgs)
    return [[msgs[(s + i) % n] for i in range(M)] for s in range(0, n, M)]


# ---------------------------------------------------------------------------
# Checker (soundness) and model (completeness)
# ---------------------------------------------------------------------------
def _grant(wire: np.ndarray, dec: dict, g: int) -> bytes:
    o, n = int(dec["grant_off"][g]), int(dec["grant_len"][g])
    return wire[o:o + n].tobytes()


def check_hint(wire: np.ndarray, dec: dict, same: np.ndarray) -> List[Tuple[int, int, str]]:
    """The (message, grant, rule) of every hint that is not sound.  same[g] == g always passes;
    any other value must be the index of the message's first grant ("first"), which lies before
    g ("order"), has g's length ("len") and g's bytes ("bytes")."""
    cgo = dec["cert_grant_off"]
    assert same.shape == dec["grant_len"].shape
    bad = []
    for m in range(cgo.shape[0] - 1):
        first = int(cgo[m])
        for g in range(first, int(cgo[m + 1])):
            s = int(same[g])
            if s == g:
                continue
            if s != first:
                bad.append((m, g, "first"))
            elif not g > first:
                bad.append((m, g, "order"))
            elif dec["grant_len"][g] != dec["grant_len"][first]:
                bad.append((m, g, "len"))
            elif _grant(wire, dec, g) != _grant(wire, dec, first):
                bad.append((m, g, "bytes"))
    return bad


def _ld_fields(b: bytes, field: int) -> List[bytes]:
    return [v for f, wt, v, _ in walk(b) if f == field and wt == 2]


def qualifies(data: bytes) -> bool:
    """A message whose hint the decoder documents as complete (given the oracle's fast-path
    status is OK): no certificate key repeated; every MultiGrant holds exactly one grants entry
    with one value and at most one grantSignatures entry (the shape decoded without a map
    walk); and the first MultiGrant begins with that grants entry in the reference encoder's
    layout -- key, then value, minimal lengths, the key under 128 bytes -- which is where the
    reference grant is read from (ref_head)."""
    try:
        wcs = _ld_fields(data, 1)
        if len(wcs) != 1:
            return False
        keys, mgs = [], []
        for e in _ld_fields(wcs[0], 1):
            k, v = _ld_fields(e, 1), _ld_fields(e, 2)
            if len(v) != 1:
                return False
            keys.append(k[-1] if k else b"")
            mgs.append(v[0])
        if not mgs or len(set(keys)) != len(keys):
            return False
        for mg in mgs:
            ge = _ld_fields(mg, 1)
            if len(ge) != 1 or len(_ld_fields(mg, 5)) > 1 or len(_ld_fields(ge[0], 2)) != 1:
                return False
        ge = _ld_fields(mgs[0], 1)[0]
        k, v = _ld_fields(ge, 1), _ld_fields(ge, 2)
        return len(k) == 1 and len(k[0]) < 128 and mgs[0].startswith(W.encode_map_entry(1, k[0], v[0]))
    except ValueError:
        return False


def model_violations(wb: W.WireBatch, status: np.ndarray, dec: dict, same: np.ndarray):
    """([(message, grant, hint, expected)], the qualifying messages): on an OK message that
    qualifies(), same[g] is the first grant's index iff g is not the first and holds its bytes."""
    cgo = dec["cert_grant_off"]
    bad, qual = [], []
    for m in range(wb.n_msgs):
        if status[m] != MSG_OK:
            continue
        o, n = int(wb.msg_off[m]), int(wb.msg_len[m])
        if not qualifies(wb.wire[o:o + n].tobytes()):
            continue
        qual.append(m)
        first = int(cgo[m])
        ref = _grant(wb.wire, dec, first) if cgo[m + 1] > first else b""
        for g in range(first, int(cgo[m + 1])):
            want = first if g != first and _grant(wb.wire, dec, g) == ref else g
            if int(same[g]) != want:
                bad.append((m, g, int(same[g]), want))
    return bad, qual


def fast_decode(wb: W.WireBatch) -> dict:
    ids, off = W.server_id_table(R)
    return O.w2_decode(wb, ids, off)
