"""What the Write2 wire corpus (w2_wire_corpus.py) covers -- oracle only, no GPU.

test_w2_wire_corpus_gpu.py compares the device with the oracle on this corpus; the
assertions here keep it from passing on an empty case: every form is present, every
status, reason and op decision occurs, the shares of clean and broken messages stay in
a band, the layouts are what they claim to be and the chunks the host pipeline cuts hold
the hard cases.
"""
import numpy as np
import pytest

import mochi_hip as mh
import oracle_ffi as O
import w2_wire_corpus as WC
import workload as W

BIG = max(WC.SIZES)
VERDICT_ARRAYS = ("cert_accept_bits", "cert_reason", "cert_fail_op", "op_decision", "op_g0", "op_ts")
OFFSET_KEYS = ("grant_off", "op_key_off")  # positions in the blob: they follow the layout


def kinds_of(prefix):
    return [m.kind for m in WC.corpus() if m.kind.startswith(prefix)]


def test_every_form_is_present():
    corpus = WC.corpus()
    assert len(corpus) % WC.GROUP, "repeats of a message must land at another alignment"
    assert len(corpus) < min(WC.SIZES), "every size must hold the whole corpus"
    assert len(WC.MUTATE_COUNTS) == WC.N_MUTATE_KINDS
    for k, n in enumerate(WC.MUTATE_COUNTS):
        assert len(kinds_of(f"mutate:{k}")) == n >= 20, k
    s = W.make_batch(WC.pool(), 1, faults=False)
    matcher, fallback = (f(s, 0, W.SERVER_IDS[:WC.R]) for f in (WC._matcher_forms, WC._fallback_forms))
    for form in matcher:
        assert len(kinds_of(f"matcher:{form}")) == WC.MATCHER_CERTS, form
    for form in fallback:
        assert len(kinds_of(f"fallback:{form}")) == WC.FALLBACK_CERTS, form
    # the figures DESIGN.md gives: 370 mutated + 32 forms x 4 + 7 forms x 8 + 3 + 1 + 1 + 32 messages
    assert (sum(WC.MUTATE_COUNTS), len(matcher), len(fallback), len(WC.DEGENERATE)) == (370, 32, 7, 3)
    assert len(kinds_of("matcher:")) == 128 and len(kinds_of("fallback:")) == 56 and len(kinds_of("degenerate:")) == 3
    assert len(corpus) == 591
    by_kind = {m.kind: m for m in corpus}
    assert by_kind["degenerate:empty"].data == b""
    assert len(by_kind["degenerate:one_byte"].data) == 1
    assert by_kind["degenerate:ff_8"].data == b"\xff" * 8
    assert len(by_kind["cut_to_1"].data) == 1
    assert len(kinds_of("no_ops")) == WC.GROUP
    # the 65-op message: one operation past the limit, FALLBACK to the fast and to the full
    # decode; with 64 operations the same certificate decodes
    assert WC.N_OPS_65 == mh.MAX_OPS_PER_CERT + 1
    ids, off = WC.id_table()
    m65 = by_kind["ops_65"].data
    fields = WC._fields(m65)
    assert [t for t, _ in fields] == [0x0A, 0x12]
    ops = WC._fields(fields[1][1][3:])  # the transaction: a 2-byte length, then 65 operations
    assert len(ops) == WC.N_OPS_65 and b"".join(r for _, r in ops) == fields[1][1][3:]
    m64 = fields[0][1] + W._ld(2, b"".join(r for _, r in ops[:-1]))
    both = WC._pack([m65, m64])
    np.testing.assert_array_equal(O.w2_decode(both, ids, off)["msg_status"], [mh.MSG_FALLBACK, mh.MSG_OK])
    np.testing.assert_array_equal(O.w2_decode_full(both, ids, off)["msg_status"], [mh.MSG_FALLBACK, mh.MSG_OK])
    np.testing.assert_array_equal(O.w2_decode(both, ids, off)["cert_op_off"], [0, 0, mh.MAX_OPS_PER_CERT])
    # no message carries a made-up hash: each is its certificate's, 128 hex characters
    assert all(len(m.hash) == 128 and set(m.hash) <= set(b"0123456789abcdef") for m in corpus)


def test_same_corpus_every_time():
    WC.corpus.cache_clear()
    a = WC.corpus()
    WC.corpus.cache_clear()
    assert a == WC.corpus()


def test_statuses_reasons_and_decisions_occur():
    for M in WC.SIZES:
        assert set(np.unique(WC.oracle_decode(M)["msg_status"]).tolist()) == {0, 1, 2, 3}, M
    for M in (min(WC.SIZES), BIG):
        reasons, decisions = set(), set()
        for strict, qm in WC.PARAMS:
            v, st = WC.oracle_verify(M, strict, qm)
            np.testing.assert_array_equal(st, WC.oracle_decode(M)["msg_status"])
            reasons |= set(np.unique(v.cert_reason).tolist())
            decisions |= set(np.unique(v.op_decision).tolist())
            # both branches of the stored-timestamp comparison
            assert {mh.OPD_APPLY, mh.OPD_READ} <= set(np.unique(v.op_decision).tolist())
        assert reasons >= {0, 1, 2, 3, 4, 5, 6, 7, 9, 10}, (M, reasons)
        assert decisions == {0, 1, 2, 3, 4}, (M, decisions)
        for strict in (True, False):
            a, b = WC.oracle_verify(M, strict, 0)[0], WC.oracle_verify(M, strict, 3)[0]
            assert (a.cert_accept != b.cert_accept).any(), "quorum_mode changes no verdict"


def test_caller_arrays_for_messages_that_are_not_clean():
    """Caller op counts: the true count of every OK and every fallback message, off by one on
    every 16th message; what the oracle answers there."""
    wb, kinds, status, mismatch = WC.batch(BIG)
    n_ops = np.diff(wb.op_flags_off.astype(np.int64))
    v, st = WC.oracle_verify(BIG, True, 0)
    assert mismatch.sum() >= BIG // WC.MISMATCH_EVERY - 2
    ok, fb, bad = (status == s for s in (mh.MSG_OK, mh.MSG_FALLBACK, mh.MSG_MALFORMED))
    # off by one: an OK message becomes OPS_MISMATCH, a fallback one stays FALLBACK; both UNDECIDED
    assert (ok & mismatch).sum() >= 50 and (fb & mismatch).sum() >= 5 and (bad & mismatch).sum() >= 5
    np.testing.assert_array_equal(st[ok & mismatch], mh.MSG_OPS_MISMATCH)
    np.testing.assert_array_equal(st[~(ok & mismatch)], status[~(ok & mismatch)])
    np.testing.assert_array_equal(v.cert_reason[(ok | fb) & mismatch], mh.UNDECIDED)
    np.testing.assert_array_equal(v.cert_reason[bad], mh.REJECT_MALFORMED)
    # fallback messages whose count is right are decided: the caller's count is their true one
    decided = fb & ~mismatch & (kinds != "ops_65")
    assert decided.sum() >= 100 and (v.cert_reason[decided] != mh.UNDECIDED).all()
    assert (n_ops[decided] >= 1).all() and v.cert_accept[decided].sum() >= 30
    i65 = np.nonzero(kinds == "ops_65")[0]
    assert i65.size >= 3 and not mismatch[i65].any()
    assert (n_ops[i65] == mh.MAX_OPS_PER_CERT + 1).all() and (v.cert_reason[i65] == mh.UNDECIDED).all()
    # ops of every undecided or malformed message: skipped, no grant, no timestamp -- and there are many
    skipped = np.repeat(np.isin(v.cert_reason, (mh.UNDECIDED, mh.REJECT_MALFORMED)), n_ops)
    assert skipped.sum() >= 300
    assert (v.op_decision[skipped] == mh.OPD_SKIPPED).all()
    assert (v.op_g0[skipped] == 0xFFFFFFFF).all() and (v.op_ts[skipped] == 0).all()
    assert (n_ops[bad] > 0).sum() >= 50, "malformed messages with caller ops"
    # messages that repeat an op key, and NOT_WRITE derived by the decoder, with per-op outputs
    for kind in ("mutate:6", "mutate:9"):
        sel = np.repeat((kinds == kind) & (st == mh.MSG_OK), n_ops)
        assert sel.sum() >= 100 and len(set(v.op_decision[sel].tolist())) >= 3, kind
    assert set(np.unique(wb.op_flags).tolist()) == set(WC.OP_FLAGS.tolist())


def test_shares():
    """Conditions on the largest batch: mostly clean traffic, enough of every broken kind."""
    v, st = WC.oracle_verify(BIG, True, 0)
    _, _, status, _ = WC.batch(BIG)
    for s in (st, status):  # with and without the caller's op counts
        share = np.bincount(s, minlength=4) / BIG
        assert share[mh.MSG_OK] >= 0.75, share
        assert 0.03 <= share[mh.MSG_MALFORMED] <= 0.15, share
        assert 0.03 <= share[mh.MSG_FALLBACK] <= 0.15, share
    assert v.cert_accept.mean() >= 0.40, v.cert_accept.mean()


def decreasing_inside_a_group(off):
    off = np.asarray(off, np.int64)
    d = np.diff(off) < 0
    d[WC.GROUP - 1::WC.GROUP] = False  # a step from one group to the next does not count
    return bool(d.any())


@pytest.mark.parametrize("M", [min(WC.SIZES), BIG])
def test_layouts(M):
    wb, kinds, status, mismatch = WC.batch(M)
    assert not decreasing_inside_a_group(wb.msg_off)
    assert set((wb.msg_off % 4).tolist()) == {0, 1, 2, 3}
    for how in ("permuted", "shared"):
        other = WC.batch(M, how)[0]
        for k in ("msg_len", "op_flags_off", "op_flags", "op_object_ts", "expected_hash"):
            np.testing.assert_array_equal(getattr(other, k), getattr(wb, k), err_msg=f"{k} {how}")
        end = other.msg_off.astype(np.int64) + other.msg_len
        assert other.msg_off.min() > 0 and end.max() < other.wire.size, "slack on both sides"
        for i in range(0, M, 97):
            a = wb.wire[int(wb.msg_off[i]):int(wb.msg_off[i]) + int(wb.msg_len[i])]
            b = other.wire[int(other.msg_off[i]):int(other.msg_off[i]) + int(other.msg_len[i])]
            np.testing.assert_array_equal(a, b)
        d, od = WC.oracle_decode(M), WC.oracle_decode(M, how)
        for k in d:
            if k not in OFFSET_KEYS:
                np.testing.assert_array_equal(od[k], d[k], err_msg=f"{k} {how}")
        for strict, qm in ((True, 0), (False, 3)):
            (v, st), (ov, ost) = WC.oracle_verify(M, strict, qm), WC.oracle_verify(M, strict, qm, how)
            np.testing.assert_array_equal(ost, st)
            for k in VERDICT_ARRAYS:
                np.testing.assert_array_equal(getattr(ov, k), getattr(v, k), err_msg=f"{k} {how}")
    assert decreasing_inside_a_group(WC.batch(M, "permuted")[0].msg_off)
    shared = WC.batch(M, "shared")[0]
    off, n = np.unique(shared.msg_off, return_counts=True)
    assert (n > 1).any(), "no two messages share their bytes"
    full = shared.msg_len > 0  # (the empty message shares its offset with whatever comes next)
    off, n = np.unique(shared.msg_off[full], return_counts=True)
    assert (n > 1).any()
    if M == BIG:  # every message of the corpus shares its bytes with its repeats
        assert (n > 1).sum() >= 500 and n.max() >= 4
    for o in off[n > 1][:20]:
        assert len(set(shared.msg_len[full & (shared.msg_off == o)].tolist())) == 1


def test_chunk_plan_restates_the_pipeline_rule():
    assert WC.chunk_plan([10] * 70, 1) == [(0, 32), (32, 64), (64, 70)]  # 320 >= 256 bytes after one group
    assert WC.chunk_plan([4] * 70, 1) == [(0, 64), (64, 70)]             # 128 bytes after one group, 256 after two
    assert WC.chunk_plan([0] * 70, 1) == [(0, 70)]
    assert WC.chunk_plan([300] * 33, 1 << 20) == [(0, 33)]
    assert WC.chunk_plan([], 1) == []


def test_chunks_hold_the_hard_cases():
    wb, kinds, status, mismatch = WC.batch(BIG)
    n_ops = np.diff(wb.op_flags_off.astype(np.int64))
    st = WC.oracle_decode(BIG)["msg_status"]
    plan = WC.chunk_plan(wb.msg_len, 1)
    assert BIG % WC.GROUP and len(plan) == -(-BIG // WC.GROUP)
    assert all(m1 - m0 == WC.GROUP for m0, m1 in plan[:-1]) and plan[-1][1] - plan[-1][0] == BIG % WC.GROUP
    assert sum((st[a:b] == mh.MSG_MALFORMED).all() and n_ops[a:b].sum() > 0 for a, b in plan) >= 1
    assert sum((st[a:b] == mh.MSG_FALLBACK).all() for a, b in plan) >= 1
    assert sum(n_ops[a:b].sum() == 0 for a, b in plan) >= 1
    zero = [(a, b) for a, b in plan if n_ops[a:b].sum() == 0][0]
    assert zero == WC.ZERO_OPS_GROUP and wb.op_flags_off[zero[0]] > 0  # not at the front of the op arrays
    # zero-length messages inside chunks, not only at their edges
    empty = np.nonzero(wb.msg_len == 0)[0]
    assert empty.size >= 3 and (empty % WC.GROUP != 0).any()
    # the large chunk target: the first chunk alone takes the decoder's large launch sequence
    cg = WC.large_chunk_grants(wb.msg_len)
    big_plan = WC.chunk_plan(wb.msg_len, cg)
    assert len(big_plan) >= 2 and big_plan[0][1] - big_plan[0][0] >= 1024, big_plan
    assert WC.chunk_plan(wb.msg_len, cg - 1)[0][1] < 1024, "not the smallest such target"
    # permuted bodies: a chunk's byte range then spans most of the blob
    perm = WC.batch(BIG, "permuted")[0]
    a, b = plan[5]
    span = int((perm.msg_off[a:b].astype(np.int64) + perm.msg_len[a:b]).max() - perm.msg_off[a:b].min())
    assert span > 10 * int(perm.msg_len[a:b].sum())
