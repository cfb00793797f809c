"""Client aggregation: the plain-Python model of MochiDBClient.java (client_model.py), the
oracle restatement and the host C++ agree on every case set of client_model.py (no GPU).

Acceptance, reason and every chosen entry are compared for the tally, the decision for the
Write1 round.  Each test also asserts what its set is there to cover, so that a set cannot
quietly degenerate.  test_client_gpu.py runs the same sets on the device.
"""
from collections import Counter

import numpy as np
import pytest

import client_model as M
import mochi_hip as mh
import oracle_ffi as O


def assert_tally_equals_model(got, b, who):
    """got = (accept, reason, chosen) of one batch b, in the wrappers' format."""
    acc, reason, chosen = got
    want_acc = [r == 0 for r in b.reason]
    bad = [i for i in range(len(b.names))
           if bool(acc[i]) != want_acc[i] or int(reason[i]) != b.reason[i] or chosen[i].tolist() != b.chosen[i]]
    first = bad[:5]
    assert not bad, (f"{who} != model on {len(bad)} of {len(b.names)} requests of {b.label} (R={b.R}): " + "; ".join(
        f"{b.names[i]}: got accept={bool(acc[i])} reason={int(reason[i])} chosen={chosen[i].tolist()}, "
        f"want reason={b.reason[i]} chosen={b.chosen[i]}" for i in first))


def assert_decisions_equal(got, want, b, who):
    bad = [i for i in range(len(b.names)) if int(got[i]) != int(want[i])]
    assert not bad, (f"{who} differs on {len(bad)} of {len(b.names)} requests of {b.label}: " + "; ".join(
        f"{b.names[i]}: got {int(got[i])}, want {int(want[i])}" for i in bad[:5]))


def test_model_constants_are_the_headers():
    assert (M.OK, M.REFUSED, M.REQUEST_FAILED, M.OTHER) == (mh.W1_OK, mh.W1_REFUSED, mh.W1_REQUEST_FAILED, mh.W1_OTHER)
    assert (M.PROCEED, M.RETRY, M.THROW_REFUSED, M.THROW_FAILED, M.THROW_UNSUPPORTED) == (
        mh.W1_PROCEED, mh.W1_RETRY, mh.W1_THROW_REFUSED, mh.W1_THROW_FAILED, mh.W1_THROW_UNSUPPORTED)
    assert M.MAX_OPS == mh.MAX_OPS_PER_CERT
    assert [M.majority(R) for R in range(11)] == [O.lib().oracle_server_majority(R) for R in range(11)]
    assert list(M.tally_batches()) == M.TALLY_LABELS and list(M.classify_batches()) == M.CLASSIFY_LABELS


@pytest.mark.parametrize("label", M.TALLY_LABELS)
def test_tally_sets_oracle_and_host_equal_model(label):
    b = M.tally_batches()[label]
    assert_tally_equals_model(O.tally_responses(b.responses, b.n_ops, b.R), b, "oracle")
    assert_tally_equals_model(mh.tally_responses(b.responses, b.n_ops, b.R), b, "host")


@pytest.mark.parametrize("label", M.CLASSIFY_LABELS)
def test_classify_sets_oracle_and_host_equal_model(label):
    b = M.classify_batches()[label]
    oracle = O.write1_classify(b.responses)
    if b.decision is None:  # outside the model's contract: the oracle is the expectation
        with pytest.raises(AssertionError):
            M.classify(b.responses[0])
    else:
        assert_decisions_equal(oracle, b.decision, b, "oracle vs model")
        named = [(i, e) for i, e in enumerate(b.expect) if e is not None]
        assert all(b.decision[i] == e for i, e in named), [b.names[i] for i, e in named if b.decision[i] != e]
    assert_decisions_equal(mh.write1_classify(b.responses), oracle if b.decision is None else b.decision, b, "host")


def test_tally_sets_cover_what_they_are_for():
    tb = M.tally_batches()
    ex = tb["exhaustive_R4"]
    assert len(ex.names) == 16917 and set(ex.reason) == {0, 1, 2}
    for R in M.EXHAUSTIVE_R:
        assert {0, 1, 2} == set(tb[f"exhaustive_R{R}"].reason)
    # R < 3 (M = 1) and a multiple of 3 move the line: the same requests, other verdicts
    assert len({tuple(tb[f"exhaustive_R{R}"].reason) for R in (2, 3, 6)}) == 3
    assert tb["exhaustive_R0"].reason == tb["exhaustive_R2"].reason
    assert any(k == 0 for k in ex.n_ops)  # zero-op transactions
    for R in M.MAJORITY_LINE_R:
        b = tb[f"majority_line_R{R}"]
        assert set(b.reason) == {0, 2}, R
        m = M.majority(R)
        counts = {min(sum(st[j] != 1 for st in resps) for j in (0, 1)) for resps in b.responses}
        assert counts == {m - 1, m}, (R, counts)  # every request sits on the line or one below it
        assert len({tuple(c) for c in b.chosen}) >= 4  # the WRONG_SHARD placement moves `chosen`
    sv = [tb[f"status_values_R{R}"] for R in (4, 7, 10)]
    assert {s for b in sv for resps in b.responses for st in resps for s in st} == set(M.STATUS_VALUES)
    assert {r for b in sv for r in b.reason} == {0, 2}
    wide = tb["wide"]
    assert set(wide.n_ops) == {M.MAX_OPS} and set(wide.reason) == {0, 1, 2}
    assert sum(r == 2 for r in wide.reason) == M.MAX_OPS and sum(r == 1 for r in wide.reason) == 6
    # an op-count mismatch keeps the chosen results of the responses before it
    assert {max(c) for c, r in zip(wide.chosen, wide.reason) if r == 1} == {-1, 4, 8}
    for n in M.TALLY_GEOMETRY_N:
        g = tb[f"geometry_{n}"]
        assert len(g.names) == n
        assert [r == 0 for r in g.reason] == [M.tally_geometry_accepts(i) for i in range(n)]
        if n >= 31:
            assert set(g.reason) == {0, 1, 2}
    words = np.packbits([M.tally_geometry_accepts(i) for i in range(128)], bitorder="little").view("<u4")
    assert words[0] != words[1] and words[0] == words[2] and words[1] == words[3]
    assert all(words[w] >> 31 and words[w] & 1 for w in range(4))


def test_classify_sets_cover_what_they_are_for():
    cb = M.classify_batches()
    ex = cb["exhaustive"]
    assert len(ex.names) == 33825
    assert Counter(ex.decision) == {M.PROCEED: 219, M.RETRY: 208, M.THROW_REFUSED: 7994, M.THROW_FAILED: 19400,
                                    M.THROW_UNSUPPORTED: 6004}
    assert set(cb["timestamps"].decision) == {M.PROCEED, M.RETRY}
    assert len(cb["timestamps"].names) == 2 * len(M.TS_PAIRS)
    keys = cb["keys"]
    assert set(keys.decision) == {M.PROCEED, M.RETRY}
    differing = Counter()
    for resps, d in zip(keys.responses, keys.decision):
        if len(resps) == 2 and d == M.RETRY:
            a, b = (dict((s, ts) for s, ts, _ in g) for _, _, g in resps)
            differing.update(s for s in a if s in b and a[s] != b[s])
    assert set(differing) == set(range(0xFF))  # every slot 0..0xFE decides a RETRY of its own
    assert max(len(g) for resps in keys.responses for _, _, g in resps) == 8
    servers = cb["servers"]
    assert {sid for resps in servers.responses for _, sid, _ in resps} >= set(M.SERVER_IDS)
    assert set(servers.decision) == {M.PROCEED, M.RETRY, M.THROW_REFUSED, M.THROW_FAILED}
    assert max(Counter(sid for k, sid, _ in resps if k == M.OK).most_common(1)[0][1]
               for resps in servers.responses) == 4
    assert set(cb["kinds"].decision) == {0, 1, 2, 3, 4}
    assert [] in cb["kinds"].responses
    assert max(len(resps) for resps in cb["kinds"].responses) == 64
    for n in M.CLASSIFY_GEOMETRY_N:
        assert cb[f"geometry_{n}"].decision == [i % 5 for i in range(n)]
    dup = O.write1_classify(cb["dup_in_response"].responses)
    assert set(dup.tolist()) == {M.PROCEED, M.RETRY, M.THROW_REFUSED}, dup


def test_model_restates_the_hand_cases():
    """The hand cases of test_capi_cpu.py, whose expectations were read off the Java."""
    assert M.tally([[0], [0], [0], [0]], 1, 4) == (0, [3])
    assert M.tally([[0], [1], [0], [1]], 1, 4) == (2, [2])
    assert M.tally([[0, 0], [0]], 2, 4) == (1, [0, 0])
    ok = lambda sid, g: (M.OK, sid, g)
    assert M.classify([ok(0, [(0, 5, 0)]), ok(1, [(0, 5, 0)])]) == M.PROCEED
    assert M.classify([ok(0, [(0, 5, 0)]), ok(1, [(0, 6, 0)]), (M.REFUSED, 2, [(0, 9, 0)])]) == M.RETRY
    assert M.classify([ok(0, [(0, 5, 0)]), (M.REFUSED, 1, [(0, 9, 0)])]) == M.THROW_REFUSED
    assert M.classify([ok(0, [(0, 5, 0)]), ok(1, [(0, 6, 0)]), (M.REQUEST_FAILED, 2, [])]) == M.THROW_FAILED
    assert M.classify([ok(0, [(0, 5, 1)])]) == M.THROW_UNSUPPORTED
    assert M.classify([ok(0, [(0, 5, 0)]), ok(1, [(0, 6, 0)]), ok(0, [(0, 6, 0)])]) == M.PROCEED
    assert M.classify([ok(0, [(0, 5, 0), (0xFF, 1, 0)]), ok(1, [(0, 5, 0), (0xFF, 2, 0)])]) == M.PROCEED
    assert M.classify([ok(0, [(0, 5, 0)]), (M.OTHER, 1, [])]) == M.THROW_REFUSED


def test_host_argument_rules():
    """The host functions follow the device forms' rule (include/mochi_hip.h): an argument
    nobody reads is not required."""
    lib = mh.load_library()
    p = lambda a: a.ctypes.data
    resp_off = np.array([0, 3], np.uint32)
    n_ops = np.array([2], np.uint32)
    rn = np.array([2, 2, 2], np.uint32)
    so = np.array([0, 2, 4], np.uint64)
    st = np.array([0, 0, 0, 1, 0, 0], np.uint8)
    co = np.array([1], np.uint64)

    def run(chosen_off, chosen, reason, n=1):
        bits = np.full(2, 0xFFFFFFFF, np.uint32)
        rc = lib.mochi_tally_responses(n, p(resp_off), p(n_ops), p(rn), p(so), p(st), chosen_off, 4,
                                       None if chosen is None else p(chosen), None if reason is None else p(reason),
                                       p(bits))
        return rc, bits.tolist()

    chosen, reason = np.full(4, -7, np.int32), np.full(2, 0xEE, np.uint8)
    assert run(p(co), chosen, reason) == (mh.OK, [0, 0xFFFFFFFF])  # op 1: 2 < 3
    assert chosen.tolist() == [-7, 2, 2, -7] and reason.tolist() == [2, 0xEE]
    st[3] = 0
    full = run(p(co), chosen, reason)
    assert full == (mh.OK, [1, 0xFFFFFFFF]) and chosen.tolist() == [-7, 2, 2, -7] and reason.tolist() == [0, 0xEE]
    # optional outputs; chosen_off is read only with chosen
    assert run(None, None, reason) == full
    assert run(p(co), None, reason) == full
    assert run(p(co), chosen, None) == full
    assert run(None, None, None) == full
    assert run(None, chosen, reason)[0] == mh.EINVAL
    # every other pointer is required
    args = [p(resp_off), p(n_ops), p(rn), p(so), p(st), p(co), 4, p(chosen), p(reason), p(np.zeros(1, np.uint32))]
    for i in (0, 1, 2, 3, 4, 9):
        a = list(args)
        a[i] = None
        assert lib.mochi_tally_responses(1, *a) == mh.EINVAL, i
    # n_requests = 0: nothing is read or written
    assert lib.mochi_tally_responses(0, None, None, None, None, None, None, 4, None, None, None) == mh.OK
    chosen[:], reason[:] = -7, 0xEE
    assert run(p(co), chosen, reason, n=0) == (mh.OK, [0xFFFFFFFF, 0xFFFFFFFF])
    assert (chosen == -7).all() and (reason == 0xEE).all()

    assert lib.mochi_write1_classify(0, None, None, None, None, None, None, None, None) == mh.OK
    decision = np.full(4, 0xEE, np.uint8)
    a = mh.pack_write1([[(mh.W1_OK, 0, []), (mh.W1_REFUSED, 1, [])], [(mh.W1_OK, 0, [])]])
    assert not a[3].any()  # no response has a grant: the grant arrays are never read
    ptrs = [p(x) for x in a]
    assert lib.mochi_write1_classify(0, *ptrs, p(decision)) == mh.OK and (decision == 0xEE).all()
    assert lib.mochi_write1_classify(2, *ptrs[:4], None, None, None, p(decision)) == mh.OK
    assert decision.tolist() == [mh.W1_THROW_REFUSED, mh.W1_PROCEED, 0xEE, 0xEE]
    for i in range(4):
        b = list(ptrs)
        b[i] = None
        assert lib.mochi_write1_classify(2, *b, p(decision)) == mh.EINVAL, i
    assert lib.mochi_write1_classify(2, *ptrs, None) == mh.EINVAL
    # NULL grant arrays where grants exist: the host can tell, and refuses
    g = mh.pack_write1([[(mh.W1_OK, 0, [(0, 5, 0)])]])
    for i in (4, 5, 6):
        b = [p(x) for x in g]
        b[i] = None
        assert lib.mochi_write1_classify(1, *b, p(decision)) == mh.EINVAL, i
