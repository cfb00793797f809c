"""What w2_same_hint.py's builders cover and what its checker catches, by the oracle alone (no
GPU): test_w2_same_hint_gpu.py then runs the device decoder and the verify path on them."""
import functools

import numpy as np

import oracle_ffi as O
import w2_same_hint as SH
import workload as W


@functools.lru_cache(maxsize=None)
def sweep_decoded():
    msgs = SH.sweep()
    wb = SH.pack(msgs)
    return msgs, wb, SH.fast_decode(wb)


def honest(dec, wire):
    """The hint the contract allows at most: every later grant with the first grant's bytes."""
    cgo = dec["cert_grant_off"]
    same = np.arange(dec["grant_len"].shape[0], dtype=np.uint32)
    for m in range(cgo.shape[0] - 1):
        first = int(cgo[m])
        for g in range(first + 1, int(cgo[m + 1])):
            if SH._grant(wire, dec, g) == SH._grant(wire, dec, first):
                same[g] = first
    return same


def test_checker_flags_falsified_hints():
    """Hand-made arrays: three messages of four, four and two grants.  The honest hint passes;
    each of four falsifications is reported under its rule."""
    A, B, C = b"grant-bytes-A", b"grant-bytes-B", b"grant-bytes-A"  # C: another message's first grant, A's bytes
    parts = [A, A, B, A, B, B, B, A, C, C]
    wire = np.frombuffer(b"".join(parts), np.uint8)
    off = np.cumsum([0] + [len(p) for p in parts[:-1]]).astype(np.uint64)
    dec = dict(grant_off=off, grant_len=np.array([len(p) for p in parts], np.uint32),
               cert_grant_off=np.array([0, 4, 8, 10], np.uint32))
    good = np.array([0, 0, 2, 0, 4, 4, 4, 7, 8, 8], np.uint32)
    np.testing.assert_array_equal(good, honest(dec, wire))
    assert SH.check_hint(wire, dec, good) == []
    assert SH.check_hint(wire, dec, np.arange(10, dtype=np.uint32)) == []  # no hint at all is sound

    def falsified(g, v):
        s = good.copy()
        s[g] = v
        return SH.check_hint(wire, dec, s)

    assert falsified(2, 0) == [(0, 2, "bytes")]   # a hint at unequal bytes (equal lengths)
    assert falsified(0, 1) == [(0, 0, "first")]   # a hint at a later grant
    assert falsified(9, 0) == [(2, 9, "first")]   # a hint at another message's first grant (equal bytes)
    assert falsified(6, 5) == [(1, 6, "first")]   # a hint at an equal grant that is not the first
    assert falsified(7, 4) == [(1, 7, "bytes")]
    longer = dict(dec, grant_len=dec["grant_len"].copy())
    longer["grant_len"][1] -= 1
    assert SH.check_hint(wire, longer, good) == [(0, 1, "len")]


def test_sweep_shapes_and_layout():
    msgs, wb, dec = sweep_decoded()
    assert set(SH.GLS) == {20, 63, 64, 65, 127, 128, 129, 151, 191, 192, 193}
    for gl in SH.GLS:
        assert len(SH.base_grant(gl)) == gl
    per = sum(gl + 6 for gl in SH.GLS)
    assert len(msgs) == len(SH.KLS) * per
    assert set((wb.msg_off % 16).tolist()) == set(range(16))
    for gl in SH.GLS[1:]:  # ... and within one grant length (the shortest has 20 positions only)
        res = {int(o) % 16 for o, m in zip(wb.msg_off, msgs) if m.gl == gl and m.kl == 4 and m.kind == "flip"}
        assert res == set(range(16)), gl
    # every flip is one byte, in a replica that is not the first
    for m in msgs:
        if m.kind == "flip":
            r = 1 + m.p % 3
            assert [g == m.grants[0] for g in m.grants] == [k != r for k in range(SH.R)]
            diff = [i for i in range(m.gl) if m.grants[r][i] != m.grants[0][i]]
            assert diff == [m.p] and len(m.grants[r]) == m.gl
    assert max(len(m.data) for m in msgs) < 3072


def test_sweep_grants_round_trip_through_the_oracle():
    """Every base grant parses to the fields it was built from; a one-byte variant that still
    parses to a canonical grant re-encodes to its own bytes, and at most MAX_STRUCTURAL
    positions of a grant do not."""
    for gl in SH.GLS:
        base = SH.base_grant(gl)
        p = O.grant_parse(base)
        assert p is not None and p["timestamp"] == SH.TS and p["configstamp"] == 0 and p["status"] == 0
        assert O.grant_encode(p["object_id"], p["timestamp"], p["transaction_hash"]) == base
        assert W.encode_grant(p["object_id"].decode(), SH.TS, p["transaction_hash"].decode()) == base
        structural = []
        for pos in range(gl):
            v = SH.flip(base, pos)
            q = O.grant_parse(v)
            if q is None or O.grant_encode(q["object_id"], q["timestamp"], q["transaction_hash"], q["configstamp"],
                                           q["status"]) != v:
                structural.append(pos)
            else:
                assert (q["object_id"], q["timestamp"], q["transaction_hash"]) != \
                    (p["object_id"], p["timestamp"], p["transaction_hash"])
        assert len(structural) <= SH.MAX_STRUCTURAL, (gl, structural)


def test_sweep_is_not_vacuous():
    """By the oracle's fast-path status: of the gl one-byte positions of each (gl, kl) at most
    MAX_STRUCTURAL leave the message undecoded; every other message decodes four grants, of
    which the model expects exactly two hinted (three for four equal grants, none when the
    first grant is the variant)."""
    msgs, wb, dec = sweep_decoded()
    st, n = dec["msg_status"], np.diff(dec["cert_grant_off"].astype(np.int64))
    same = honest(dec, wb.wire)
    assert SH.check_hint(wb.wire, dec, same) == []
    bad, qual = SH.model_violations(wb, st, dec, same)
    assert bad == []
    qual = set(qual)
    cgo = dec["cert_grant_off"]
    hinted = [sum(int(same[g]) != g for g in range(int(cgo[i]), int(cgo[i + 1]))) for i in range(len(msgs))]
    for kl in SH.KLS:
        for gl in SH.GLS:
            idx = [i for i, m in enumerate(msgs) if m.gl == gl and m.kl == kl]
            flips = [i for i in idx if msgs[i].kind == "flip"]
            assert len(flips) == gl
            lost = [msgs[i].p for i in flips if st[i] != SH.MSG_OK or n[i] < SH.R]
            assert len(lost) <= SH.MAX_STRUCTURAL, (gl, kl, lost)
            for i in idx:
                k = msgs[i].kind
                if st[i] != SH.MSG_OK:
                    continue
                assert n[i] == SH.R and i in qual, (gl, kl, k, msgs[i].p)
                assert hinted[i] == {"flip": 2, "flip_first": 0, "longer_status": 2, "equal": 3}[k], (gl, kl, k, msgs[i].p)
            kinds = {msgs[i].kind: st[i] for i in idx if msgs[i].kind != "flip"}
            assert kinds["equal"] == SH.MSG_OK and kinds["longer_status"] == SH.MSG_OK
            assert kinds["longer_unknown"] != SH.MSG_OK  # not canonical: left to the host decoder


def test_verdict_positions_exist():
    for gl in SH.GLS:
        ps = sorted(set(q for q in SH.verdict_positions(gl) if 0 <= q < gl))
        assert {0, 1, 2, 3, gl - 2, gl - 1} <= set(ps)
        if gl == SH.REAL_GL:
            assert ps == list(range(gl))
    msgs = SH.sweep(positions=SH.verdict_positions)
    assert len(msgs) < 800


def test_qualifies():
    msgs, wb, dec = sweep_decoded()
    assert all(SH.qualifies(m.data) for m in msgs if m.kind == "equal")
    adv = {m.kind: m for m in SH.adversaries()}
    assert len(adv) == 16
    # these leave the model (soundness only): a repeated key or value, two grants entries, a
    # reference grant that is not where the hint's parse looks for it
    for name in ("repeated_grant_key", "value_twice_in_entry", "two_grant_keys", "cert_key_repeated", "server_id_first",
                 "grant_key_128"):
        assert not SH.qualifies(adv[f"adv:{name}:first"].data), name
    for name in ("first_grant_reordered", "first_grant_193"):
        assert SH.qualifies(adv[f"adv:{name}:first"].data), name


def test_adversaries_by_the_oracle():
    """What each adversary decodes to: which of the first MultiGrant's values is the first grant,
    and that the followers' bytes are the ones announced."""
    adv = SH.adversaries()
    wb = SH.pack(adv)
    dec = SH.fast_decode(wb)
    st, cgo = dec["msg_status"], dec["cert_grant_off"]
    first_is = {"repeated_grant_key": "last", "two_grant_keys": "first", "cert_key_repeated": "last",
                "server_id_first": "first", "grant_key_128": "first", "first_grant_193": "first"}
    for i, m in enumerate(adv):
        _, name, which = m.kind.split(":")
        if name in ("value_twice_in_entry", "first_grant_reordered"):
            assert st[i] == SH.MSG_FALLBACK, m.kind  # the host decoder's
            continue
        assert st[i] == SH.MSG_OK, m.kind
        g0, g1 = int(cgo[i]), int(cgo[i + 1])
        assert g1 - g0 == (5 if name == "two_grant_keys" else 4), m.kind
        followers = {SH._grant(wb.wire, dec, g) for g in range(g1 - 3, g1)}
        assert len(followers) == 1
        assert (SH._grant(wb.wire, dec, g0) in followers) == (first_is[name] == which), m.kind
    same = honest(dec, wb.wire)
    assert SH.check_hint(wb.wire, dec, same) == []
