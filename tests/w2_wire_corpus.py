"""Write2ToServer wire forms for the decoder tests: the hand-built message builders
(shared with test_write2_wire_gpu.py) and a seeded corpus that crosses every form
with every launch path of the wire decoder.

The corpus (corpus()) holds every structural mutation of _mutate, every form around the
layout matcher's edges, every fallback form, degenerate messages, a 65-operation message
and certificates without operations, each with its kind and its certificate's real
expected hash.  batch(M, layout) cycles it to M messages, lays the bodies out in the
blob (packed / permuted / shared) and adds the caller's per-op arrays for EVERY message,
clean or not: op_flags_off with the message's true operation count (on purpose off by
one on every 16th message), drawn op_flags and stored timestamps around the oracle's
own op_ts.  The oracle reads the same WireBatch, so it follows any layout.

Order: the corpus begins with three groups of 32 messages -- malformed only, fallback
only, certificates without operations -- so that under 32-message chunks a batch holds a
chunk in which nothing decodes, one that is left to the host decoder entirely and one
without a single caller op.  The rest is shuffled; the corpus length is no multiple of
32, so every repeat of a message lands at another alignment, next to other neighbours.

test_w2_wire_corpus_cpu.py asserts what the corpus covers (oracle only);
test_w2_wire_corpus_gpu.py compares the device with the oracle on it.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import List, Tuple

import numpy as np

import mochi_hip as mh
import oracle_ffi as O
import workload as W


def _pack(msgs, pad=1):
    off, parts, pos = [], [], 0
    for i, m in enumerate(msgs):
        p = (i * pad) % 4
        parts.append(b"\x00" * p)
        pos += p
        off.append(pos)
        parts.append(m)
        pos += len(m)
    M = len(msgs)
    return W.WireBatch(wire=np.frombuffer(b"".join(parts) or b"\x00", np.uint8).copy(),
                       msg_off=np.array(off, np.uint64), msg_len=np.array([len(m) for m in msgs], np.uint32),
                       op_flags_off=None, op_flags=np.zeros(1, np.uint8),
                       expected_hash=np.zeros((M, 128), np.uint8))


N_MUTATE_KINDS = 10


def _mutate(rng, s, c, ids, kind=None):
    """One certificate's message with a structural mutation (decode-semantics fuzz);
    kind: one of range(N_MUTATE_KINDS), drawn when None."""
    b = s.batch
    g0, g1 = int(b.cert_grant_off[c]), int(b.cert_grant_off[c + 1])
    mgs = {}
    for g in range(g0, g1):
        gb = b.grant_bytes[int(b.grant_off[g]):int(b.grant_off[g]) + int(b.grant_len[g])].tobytes()
        mgs.setdefault(int(b.signer[g]), []).append((W.grant_object_id(gb), gb, b.sig[g].tobytes()))
    order = list(mgs)
    if kind is None:
        kind = int(rng.integers(0, N_MUTATE_KINDS))
    if kind == 1:
        rng.shuffle(order)  # MultiGrant wire order decides g0
    enc = []
    for r in order:
        items = mgs[r]
        sigs = [(o, sg) for o, _, sg in items]
        if kind == 2:
            sigs = sigs[1:]  # a grant without signature
        extra = b""
        if kind == 3:
            extra = b"\x48\x07" + W._ld(13, b"unknown")  # unknown fields
        enc.append((ids[r], W.encode_multigrant([(o, gb) for o, gb, _ in items], ids[r], "cl", "", sigs) + extra))
    if kind == 4 and len(enc) > 1:
        enc.append((enc[0][0], enc[-1][1]))  # repeated certificate key: first place, last value
    if kind == 5:
        enc.insert(0, (ids[order[0]], enc[0][1]))  # duplicate of the first entry
    ops = [W.encode_operation(2, o) for o, _, _ in mgs[order[0]]]
    if kind == 6:
        ops = ops + ops  # ops repeating a key (multiplicity)
    if kind == 9:  # READ / DELETE / unknown actions, an empty operand1 -> MOCHI_OP_NOT_WRITE or not
        ops = [W.encode_operation(int(rng.choice([0, 1, 2, 5])), o) for o, _, _ in mgs[order[0]]]
        ops.append(W.encode_operation(2, ""))
    m = W.encode_write2(enc, ops)
    if kind == 7 and len(m) > 8:
        i = int(rng.integers(0, len(m)))
        m = m[:i] + bytes([m[i] ^ (1 << int(rng.integers(0, 8)))]) + m[i + 1:]  # random bit flip
    if kind == 8:
        m = m[:int(rng.integers(0, len(m) + 1))]  # truncation
    return m


def _fields(b):
    """(tag, raw field bytes) of a protobuf message with varint / length-delimited fields."""
    out, i = [], 0
    while i < len(b):
        j = i
        while b[j] & 0x80:
            j += 1
        tag = b[i]
        j += 1
        if tag & 7 == 0:
            while b[j] & 0x80:
                j += 1
            j += 1
        else:
            n, sh, k = 0, 0, j
            while True:
                n |= (b[k] & 0x7F) << sh
                sh += 7
                k += 1
                if not b[k - 1] & 0x80:
                    break
            j = k + n
        out.append((tag, b[i:j]))
        i = j
    return out


def _reorder(gb):
    """A canonical Grant with its fields written in reverse order (same parsed Grant)."""
    return b"".join(raw for _, raw in reversed(_fields(gb)))


def _fallback_forms(s, c, ids):
    """Certificate c of a synthetic batch re-encoded in legal forms the device fast path
    declines (MOCHI_MSG_FALLBACK); the library's host decoder must decide them."""
    b = s.batch
    g0, g1 = int(b.cert_grant_off[c]), int(b.cert_grant_off[c + 1])
    mgs = {}
    for g in range(g0, g1):
        gb = b.grant_bytes[int(b.grant_off[g]):int(b.grant_off[g]) + int(b.grant_len[g])].tobytes()
        mgs.setdefault(int(b.signer[g]), []).append((W.grant_object_id(gb), gb, b.sig[g].tobytes()))
    ent = [(ids[r], W.encode_multigrant([(o, gb) for o, gb, _ in it], ids[r], "cl", "", [(o, sg) for o, _, sg in it]))
           for r, it in mgs.items()]
    ops = [W.encode_operation(2, o) for o, _, _ in next(iter(mgs.values()))]
    canon = W.encode_write2(ent, ops)
    wc = b"".join(W.encode_map_entry(1, k.encode(), v) for k, v in ent)
    tx = b"".join(W._ld(1, o) for o in ops)
    oid, gb, _ = next(iter(mgs.values()))[0]
    forms = {
        "canonical": canon,
        "wc_split": W._ld(1, wc[:len(W.encode_map_entry(1, ent[0][0].encode(), ent[0][1]))]) + W._ld(2, tx) +
                    W._ld(1, wc[len(W.encode_map_entry(1, ent[0][0].encode(), ent[0][1])):]),
        "tx_twice": W._ld(1, wc) + W._ld(2, tx) + W._ld(2, b""),
        # 29 extra MultiGrants from unknown servers, unsigned, same grant: 33 MultiGrants in all
        "33_multigrants": W.encode_write2(ent + [(f"extra-{i}", W.encode_multigrant([(oid, gb)], f"extra-{i}"))
                                                 for i in range(29)], ops),
        # 33 certificate entries on the wire, 32 distinct keys (the first entry repeated
        # last): the fast path counts wire entries, so this leaves it too
        "33_entries_32_keys": W.encode_write2(ent + [(f"extra-{i}", W.encode_multigrant([(oid, gb)], f"extra-{i}"))
                                                     for i in range(28)] + [ent[0]], ops),
        # one MultiGrant repeating its grants / grantSignatures entries 65 times each
        "65_grant_entries": W.encode_write2(
            [(ids[r], W.encode_multigrant([(o, gb) for o, gb, _ in it] * 65, ids[r], "cl", "",
                                          [(o, sg) for o, _, sg in it] * 65)) for r, it in mgs.items()], ops),
        # every grant's fields out of canonical order: the signature covers the canonical
        # re-encoding (Grant.toByteArray()), so it still verifies
        "noncanonical_grants": W.encode_write2(
            [(ids[r], W.encode_multigrant([(o, _reorder(gb)) for o, gb, _ in it], ids[r], "cl", "",
                                          [(o, sg) for o, _, sg in it])) for r, it in mgs.items()], ops),
    }
    return forms


def _bad_key_byte(m, oid):
    """m with the last byte of its first grants entry's key made 0xFF (invalid UTF-8)."""
    kb = oid.encode()
    pat = b"\x0a" + bytes([len(kb)]) + kb + b"\x12"
    assert pat in m
    return m.replace(pat, pat[:-2] + b"\xff\x12", 1)


def _matcher_forms(s, c, ids):
    """Certificate c re-encoded at and around the edges of k_w2_mg's layout matcher
    (mg_match: the reference encoder's one-grant MultiGrant, ASCII key and serverId
    <= 60 bytes, signature entry under the grant's key, Grant in its common canonical
    shape <= 192 bytes).  Each form is legal protobuf; the matcher either decodes it
    exactly as the walk does or leaves it to the walk."""
    b = s.batch
    g0, g1 = int(b.cert_grant_off[c]), int(b.cert_grant_off[c + 1])
    items = []
    for g in range(g0, g1):
        gb = b.grant_bytes[int(b.grant_off[g]):int(b.grant_off[g]) + int(b.grant_len[g])].tobytes()
        items.append((int(b.signer[g]), W.grant_object_id(gb), gb, b.sig[g].tobytes()))
    r0, oid, gb, _ = items[0]
    p = O.grant_parse(gb)
    ts, th = int(p["timestamp"]), p["transaction_hash"].decode()
    th_alt = th[:-1] + ("0" if th[-1] != "0" else "1")

    def msg(grant_of=lambda r, g: g, key_of=lambda r, o: o, sig_key_of=None, sid_of=lambda r: ids[r],
            sig_of=lambda r, sg: sg, extra_of=None, ops_of=None, cert_key_of=lambda r: ids[r], dup_entry=False):
        ent = []
        for r, o, g, sg in items:
            k = key_of(r, o)
            sk = sig_key_of(r, k) if sig_key_of else k
            gl = grant_of(r, g)
            grants = gl if isinstance(gl, list) else [(k, gl)]
            mg = W.encode_multigrant(grants, sid_of(r), "", "", [(sk, sig_of(r, sg))])
            ent.append((cert_key_of(r), mg + (extra_of(r) if extra_of else b"")))
        if dup_entry:
            ent.append(ent[0])  # a repeated certificate key: first position, last value
        key = key_of(r0, oid)
        return W.encode_write2(ent, ops_of(key) if ops_of else [W.encode_operation(2, key)])

    return {
        "plain": msg(),
        "sig_under_other_key": msg(sig_key_of=lambda r, k: k + "x"),
        "key_60": msg(key_of=lambda r, o: (o + "-" + "k" * 60)[:60]),
        "key_61": msg(key_of=lambda r, o: (o + "-" + "k" * 61)[:61]),
        "key_non_ascii": msg(key_of=lambda r, o: o + "é"),
        "sid_non_ascii": msg(sid_of=lambda r: ids[r] + "é"),
        "sid_61": msg(sid_of=lambda r: (ids[r] + "-" + "s" * 61)[:61]),
        "sig_255": msg(sig_of=lambda r, sg: sg[:255]),
        "trailing_unknown": msg(extra_of=lambda r: b"\x48\x07"),
        "short_grant": msg(grant_of=lambda r, g: W.encode_grant(oid, ts, "ab")),
        "grant_hash_127": msg(grant_of=lambda r, g: W.encode_grant(oid, ts, "c" * 127)),
        "grant_hash_128": msg(grant_of=lambda r, g: W.encode_grant(oid, ts, "c" * 128)),
        "grant_ts_1": msg(grant_of=lambda r, g: W.encode_grant(oid, 1, th)),
        "grant_ts_9_bytes": msg(grant_of=lambda r, g: W.encode_grant(oid, 1 << 62, th)),
        "grant_ts_negative": msg(grant_of=lambda r, g: W.encode_grant(oid, -7, th)),
        "grant_configstamp": msg(grant_of=lambda r, g: W.encode_grant(oid, ts, th, configstamp=3)),
        "grant_oid_non_ascii": msg(grant_of=lambda r, g: W.encode_grant(oid + "é", ts, th)),
        "grant_hash_non_ascii": msg(grant_of=lambda r, g: W.encode_grant(oid, ts, th[:-1] + "é")),
        "grant_reordered": msg(grant_of=lambda r, g: _reorder(g)),
        "grant_200_bytes": msg(grant_of=lambda r, g: W.encode_grant(oid + "o" * 40, ts, th)),
        "key_bad_utf8": _bad_key_byte(msg(), oid),
        # level-1 shapes: operations, certificate keys
        "op_no_action": msg(ops_of=lambda k: [W.encode_operation(0, k)]),
        "op_operand2": msg(ops_of=lambda k: [W.encode_operation(2, k, "v")]),
        "ops_4": msg(ops_of=lambda k: [W.encode_operation(2, k + str(i) if i else k) for i in range(4)]),
        "ops_5": msg(ops_of=lambda k: [W.encode_operation(2, k + str(i) if i else k) for i in range(5)]),
        "op_second_names_key": msg(ops_of=lambda k: [W.encode_operation(2, k + "z"), W.encode_operation(2, k)]),
        "op_key_57": msg(key_of=lambda r, o: (o + "-" + "q" * 57)[:57]),
        "cert_key_non_ascii": msg(cert_key_of=lambda r: ids[r] + "é"),
        "cert_key_57": msg(cert_key_of=lambda r: (ids[r] + "-" + "c" * 57)[:57]),
        "cert_key_repeated": msg(dup_entry=True),
        "cert_keys_equal_pairs": msg(cert_key_of=lambda r: ids[r % 2]),
        # the first MultiGrant names the grant key twice: LinkedHashMap keeps the first
        # position and the LAST value (a variant: another transaction hash), while every
        # other MultiGrant carries the first value's bytes -- they must not take the
        # variant's prep results
        "repeated_key_first_mg": msg(grant_of=lambda r, g: [(oid, g), (oid, W.encode_grant(oid, ts, th_alt))]
                                     if r == r0 else g),
    }


# ---------------------------------------------------------------------------
# The corpus
# ---------------------------------------------------------------------------
SEED = 31337
R = 4
SIZES = (600, 1023, 1024, 1025, 2100)
LAYOUTS = ("packed", "permuted", "shared")
GROUP = 32            # messages per accept-bitmap word: the host pipeline's chunk granule
# Messages per _mutate kind: five certificates with a planted fault each, the rest clean.
# Kind 0 (no mutation at all) is the clean traffic around the broken forms; the bit flips (7)
# and truncations (8) are what most of the malformed messages come from.
MUTATE_COUNTS = (110, 30, 30, 30, 30, 30, 30, 25, 25, 30)
MATCHER_CERTS = 4
FALLBACK_CERTS = 8
MISMATCH_EVERY = 16   # every 16th message of a batch: the caller's op count off by one
ZERO_OPS_GROUP = (2 * GROUP, 3 * GROUP)  # batch positions of the chunk without caller ops
# The op flags test_wire_stored_state_and_per_op_outputs draws.  LOCAL|HAS_SVOC (3) and
# ...|HAS_CURRENT_C (7) let a sound certificate through; each of the others rejects it or
# skips the op (WRONG_SHARD).  About one draw in four is one of those six, so that every
# decision occurs hundreds of times while most sound certificates are still accepted.
OP_FLAGS = np.array([3, 7, 15, 1, 2, 23, 19, 11], np.uint8)
OP_FLAGS_P = (0.34, 0.42) + (0.04,) * 6
N_OPS_65 = 65         # MOCHI_MAX_OPS_PER_CERT + 1
DEGENERATE = {"empty": b"", "one_byte": b"\x0a", "ff_8": b"\xff" * 8}


@dataclass(frozen=True)
class Msg:
    kind: str     # "mutate:<k>", "matcher:<form>", "fallback:<form>", "degenerate:<name>", "cut_to_1", "ops_65", "no_ops"
    data: bytes
    hash: bytes   # the certificate's expected transaction hash, 128 hex characters


@functools.lru_cache(maxsize=None)
def pool():
    return W.build_pool(R=R, k=1, P=512, P_f=64)


@functools.lru_cache(maxsize=None)
def id_table():
    return W.server_id_table(R)


def _cert_entries(s, c, ids):
    """Certificate c as canonical (certificate key, MultiGrant) entries, and its op key."""
    b = s.batch
    ent, oid = [], None
    for g in range(int(b.cert_grant_off[c]), int(b.cert_grant_off[c + 1])):
        gb = b.grant_bytes[int(b.grant_off[g]):int(b.grant_off[g]) + int(b.grant_len[g])].tobytes()
        o, r = W.grant_object_id(gb), int(b.signer[g])
        oid = oid or o
        ent.append((ids[r], W.encode_multigrant([(o, gb)], ids[r], "cl", "", [(o, b.sig[g].tobytes())])))
    return ent, oid


def fast_status(msgs) -> np.ndarray:
    """The oracle's fast-path status of each message (no caller arrays)."""
    ids, off = id_table()
    return O.w2_decode(_pack([m.data for m in msgs]), ids, off)["msg_status"]


@functools.lru_cache(maxsize=None)
def corpus() -> Tuple[Msg, ...]:
    p = pool()
    ids4 = W.SERVER_IDS[:R]
    rng = np.random.default_rng(SEED)
    msgs: List[Msg] = []
    # every mutation kind on one certificate of each planted fault of the synthetic stream (bad
    # signature, timestamp, either hash, a dropped grant: 1 in 36 certificates has one) and on
    # clean ones
    s = W.make_batch(p, 8192, first_cert=999)
    by_fault = [np.nonzero(s.fault == f)[0] for f in range(6)]
    first_clean = 0
    for k, n in enumerate(MUTATE_COUNTS):
        clean = by_fault[W.FAULT_NONE][first_clean:first_clean + n - 5]
        first_clean += n - 5
        for c in [int(by_fault[f][k]) for f in range(1, 6)] + clean.tolist():
            msgs.append(Msg(f"mutate:{k}", _mutate(rng, s, c, W.SERVER_IDS, kind=k), s.batch.expected_hash[c].tobytes()))
    s = W.make_batch(p, 4 * MATCHER_CERTS, first_cert=5150, faults=False)
    for c in range(0, 4 * MATCHER_CERTS, 4):
        for form, m in _matcher_forms(s, c, ids4).items():
            msgs.append(Msg(f"matcher:{form}", m, s.batch.expected_hash[c].tobytes()))
    s = W.make_batch(p, 8 * FALLBACK_CERTS, first_cert=4242, faults=False)
    for c in range(0, 8 * FALLBACK_CERTS, 8):
        for form, m in _fallback_forms(s, c, ids4).items():
            msgs.append(Msg(f"fallback:{form}", m, s.batch.expected_hash[c].tobytes()))
    s = W.make_batch(p, GROUP + 2, first_cert=7100, faults=False)
    for name, m in DEGENERATE.items():
        msgs.append(Msg(f"degenerate:{name}", m, s.batch.expected_hash[0].tobytes()))
    ent, oid = _cert_entries(s, 0, ids4)
    msgs.append(Msg("cut_to_1", W.encode_write2(ent, [W.encode_operation(2, oid)])[:1], s.batch.expected_hash[0].tobytes()))
    # 65 operations: past MOCHI_MAX_OPS_PER_CERT, FALLBACK that the host decoder cannot express either
    ent, oid = _cert_entries(s, 1, ids4)
    ops = [W.encode_operation(2, oid + str(i) if i else oid) for i in range(N_OPS_65)]
    msgs.append(Msg("ops_65", W.encode_write2(ent, ops), s.batch.expected_hash[1].tobytes()))
    # a certificate without a transaction: decodes, no operation
    for c in range(2, GROUP + 2):
        msgs.append(Msg("no_ops", W.encode_write2(_cert_entries(s, c, ids4)[0], []), s.batch.expected_hash[c].tobytes()))
    # order: 32 malformed, 32 fallback, the 32 without operations, the rest shuffled
    st = fast_status(msgs)
    kinds = np.array([m.kind for m in msgs])
    idx = np.arange(len(msgs))
    head = [idx[st == mh.MSG_MALFORMED][:GROUP], idx[(st == mh.MSG_FALLBACK) & (kinds != "ops_65")][:GROUP],
            idx[kinds == "no_ops"]]
    assert all(h.size == GROUP for h in head)
    rest = np.setdiff1d(idx, np.concatenate(head))
    rng.shuffle(rest)
    return tuple(msgs[i] for i in np.concatenate(head + [rest]))


def tile(msgs, M: int):
    """msgs cycled to M messages."""
    return [msgs[i % len(msgs)] for i in range(M)]


def layout(msgs, how: str, seed: int = SEED):
    """(wire, msg_off) of the message bodies under one of LAYOUTS."""
    rng = np.random.default_rng(seed)
    M = len(msgs)
    off = np.zeros(M, np.uint64)
    if how == "packed":  # in order, pad residues 0..3 (as _pack does)
        wb = _pack([m.data for m in msgs], pad=1)
        return wb.wire, wb.msg_off
    parts, pos = [b"\xee" * 37], 37  # slack before the first body ...
    if how == "permuted":  # message order stays, the bodies lie in a random permutation
        for i in rng.permutation(M):
            pad = int(rng.integers(0, 4))
            parts += [b"\xee" * pad, msgs[i].data]
            off[i] = pos + pad
            pos += pad + len(msgs[i].data)
    elif how == "shared":  # equal messages point at one copy of their bytes
        at = {}
        for i, m in enumerate(msgs):
            if m.data not in at:
                pad = int(rng.integers(0, 4))
                parts += [b"\xee" * pad, m.data]
                at[m.data] = pos + pad
                pos += pad + len(m.data)
            off[i] = at[m.data]
    else:
        raise ValueError(how)
    parts.append(b"\xee" * 91)  # ... and after the last
    return np.frombuffer(b"".join(parts), np.uint8).copy(), off


def true_op_counts(wire, off, ln, hashes) -> Tuple[np.ndarray, np.ndarray]:
    """Per message: the oracle's fast-path status and its operation count by the FULL
    decode (a fallback message's true count; 0 for a malformed one)."""
    ids, ido = id_table()
    wb = W.WireBatch(wire=wire, msg_off=off, msg_len=ln, op_flags_off=None, op_flags=np.zeros(1, np.uint8),
                     expected_hash=hashes)
    fast = O.w2_decode(wb, ids, ido)
    full = O.w2_decode_full(wb, ids, ido)
    n_fast, n_full = np.diff(fast["cert_op_off"].astype(np.int64)), np.diff(full["cert_op_off"].astype(np.int64))
    ok = fast["msg_status"] == mh.MSG_OK
    assert (n_fast[ok] == n_full[ok]).all() and (n_fast[~ok] == 0).all()
    return fast["msg_status"], n_full


@functools.lru_cache(maxsize=None)
def batch(M: int, how: str = "packed"):
    """(WireBatch, kinds [M], fast-path status before any caller array [M], mismatch [M]) of
    the corpus cycled to M messages under layout `how`, with caller arrays for every
    message.  The caller arrays depend on M alone, so the layouts of one M must agree."""
    msgs = tile(corpus(), M)
    wire, off = layout(msgs, how)
    ln = np.array([len(m.data) for m in msgs], np.uint32)
    hashes = np.stack([np.frombuffer(m.hash, np.uint8) for m in msgs])
    status, n_ops = true_op_counts(wire, off, ln, hashes)
    rng = np.random.default_rng([SEED, M])
    drawn = rng.integers(0, 4, M)
    n_ops = np.where(status == mh.MSG_MALFORMED, drawn, n_ops)
    # the 65-op message is beyond the oracle's full decode too (it reports no op): its caller
    # still names all 65, and every one of them has to read MOCHI_OPD_SKIPPED
    kinds = np.array([m.kind for m in msgs])
    n_ops[kinds == "ops_65"] = N_OPS_65
    pos = np.arange(M)
    n_ops[(pos >= ZERO_OPS_GROUP[0]) & (pos < ZERO_OPS_GROUP[1])] = 0
    # every 16th message: one op more or fewer than the message holds
    mismatch = (pos % MISMATCH_EVERY == 0) & ~((pos >= ZERO_OPS_GROUP[0]) & (pos < ZERO_OPS_GROUP[1]))
    delta = np.where(rng.integers(0, 2, M) == 1, 1, -1)
    delta[n_ops == 0] = 1
    n_ops = n_ops + np.where(mismatch, delta, 0)
    ofo = np.zeros(M + 1, np.uint32)
    np.cumsum(n_ops, out=ofo[1:])
    n = int(ofo[-1])
    wb = W.WireBatch(wire=wire, msg_off=off, msg_len=ln, op_flags_off=ofo, op_flags=rng.choice(OP_FLAGS, n, p=OP_FLAGS_P),
                     expected_hash=hashes, op_object_ts=np.zeros(n, np.int64))
    # stored timestamps around the oracle's own op_ts (first pass: no stored state), so that
    # both the read and the apply branch occur
    ids, ido = id_table()
    first, _ = O.verify_write2(pool().moduli, ids, ido, wb, R, True)
    wb.op_object_ts = first.op_ts + rng.integers(-2, 3, n)
    for a in (wb.wire, wb.msg_off, wb.msg_len, wb.op_flags_off, wb.op_flags, wb.expected_hash, wb.op_object_ts):
        a.setflags(write=False)
    return wb, kinds, status, mismatch


PARAMS = [(strict, qm) for strict in (True, False) for qm in (0, 3)]


@functools.lru_cache(maxsize=None)
def oracle_decode(M: int, how: str = "packed"):
    ids, ido = id_table()
    return O.w2_decode(batch(M, how)[0], ids, ido)


@functools.lru_cache(maxsize=None)
def oracle_verify(M: int, strict: bool, quorum_mode: int, how: str = "packed"):
    """(Verdicts, msg_status) of the oracle; computed once, shared, not to be changed."""
    ids, ido = id_table()
    return O.verify_write2(pool().moduli, ids, ido, batch(M, how)[0], R, strict, quorum_mode=quorum_mode)


def chunk_plan(msg_len, chunk_grants: int) -> List[Tuple[int, int]]:
    """The host pipeline's chunks [(m0, m1)] of a wire batch (mochi_verify_write2): whole
    groups of 32 messages until the chunk's bytes reach chunk_grants * 256."""
    ln = np.asarray(msg_len, np.int64)
    M, target = ln.shape[0], chunk_grants * 256
    out, m0 = [], 0
    while m0 < M:
        m1, size = m0, 0
        while True:
            nxt = min(m1 + GROUP, M)
            size += int(ln[m1:nxt].sum())
            m1 = nxt
            if not (m1 < M and size < target):
                break
        out.append((m0, m1))
        m0 = m1
    return out


def large_chunk_grants(msg_len, first: int = 1024) -> int:
    """The smallest chunk target under which the first chunk holds at least `first`
    messages (it takes the decoder's large launch sequence inside the pipeline)."""
    ln = np.asarray(msg_len, np.int64)
    last_group = (first - 1) // GROUP * GROUP  # the chunk must still be open after this many messages
    return int(ln[:last_group].sum()) // 256 + 1
