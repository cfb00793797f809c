"""The tally fuzz generator (tally_fuzz.py) is sound and covers the ground -- oracle only, no GPU.

Soundness: the flags and timestamps it states by construction are what the oracle's
parser and OpenSSL find.  Coverage: under every parameter set the GPU test runs, the
oracle's verdicts over the batch reach the branches the generator exists for (deep op
indices, every reason code, g0 behind a slot's first grant, ...), asserted line by line
so that a later edit of the generator cannot hollow the GPU test out.
"""
import numpy as np
import pytest

import mochi_hip as mh
import oracle_ffi as O
import tally_fuzz as TF

SEED = 20260
PARAMS = [(strict, qm, csr) for strict in (True, False) for qm in (0, 1, 2, 3) for csr in (True, False)]


@pytest.fixture(scope="module", params=[4, 7])
def fz(request):
    return TF.make(request.param, SEED)


@pytest.fixture(scope="module")
def tallies(fz):
    """Oracle verdicts per (strict, quorum_mode, CSR present), from the flags by construction."""
    out = {}
    for strict, qm, csr in PARAMS:
        b = fz.batch if csr else TF.without_csr(fz.batch)
        out[strict, qm, csr] = O.tally(b, fz.grant_flags, fz.grant_ts, fz.R, strict, qm)
    return out


def op_index(b):
    """Per op: its certificate and its index inside it."""
    coo = np.asarray(b.cert_op_off, np.int64)
    cert = np.repeat(np.arange(b.n_certs), np.diff(coo))
    return cert, np.arange(b.n_ops) - coo[cert]


def test_construction_matches_oracle_parse(fz):
    flags, ts = O.parse_grants(fz.batch)
    np.testing.assert_array_equal(flags, fz.grant_flags & mh.GRANT_PARSED)
    np.testing.assert_array_equal(ts, fz.grant_ts)


def test_construction_matches_openssl(fz):
    flags, ts = O.verify_grants(fz.moduli, fz.batch, 0, fz.batch.n_grants, 8)
    np.testing.assert_array_equal(flags, fz.grant_flags)
    np.testing.assert_array_equal(ts, fz.grant_ts)
    # every flag combination occurs, and so does a signer outside the key table
    assert set(np.unique(fz.grant_flags).tolist()) == {0, 1, 2, 3}
    assert (fz.batch.signer == fz.R).any()


def test_same_seed_same_batch(fz):
    again = TF.make(fz.R, SEED)
    for k in mh.Batch.FIELDS + mh.Batch.OPTIONAL:
        np.testing.assert_array_equal(getattr(again.batch, k), getattr(fz.batch, k), err_msg=k)
    np.testing.assert_array_equal(again.grant_flags, fz.grant_flags)
    assert again.kind == fz.kind
    other = TF.make(fz.R, SEED + 1, n_certs=40)
    assert not np.array_equal(other.batch.op_flags, TF.head(fz.batch, 40).op_flags)


def test_batch_shape(fz):
    """The shapes the issue's list of unreached logic names, and a batch that stays small."""
    b = fz.batch
    assert b.n_certs == 400
    n_ops = np.diff(np.asarray(b.cert_op_off, np.int64))
    per = np.diff(np.asarray(b.cert_grant_off, np.int64))
    assert set(TF.DEEP_OPS) <= set(n_ops.tolist()) and set(range(6)) <= set(n_ops.tolist())
    assert 0.7 <= (n_ops <= 5).mean() <= 0.8
    assert b.n_grants < (20000 if fz.R == 4 else 36000)
    assert TF.n_signed() < 2500  # distinct (bytes, signer) pairs signed, both R together
    # key slots above 1 everywhere; grants filed under slots >= 64 (k_grant_prep_cert's scan-back branch)
    assert set(range(64)) <= set(b.op_key.tolist())
    assert {64, 200, 255} <= set(b.grant_key.tolist())
    # multiplicity 3 and more; three or more slots in certificates of unequal size
    cert, _ = op_index(b)
    mult = max(np.bincount(b.op_key[cert == c], minlength=64).max() for c in np.nonzero(n_ops)[0])
    assert mult >= 3
    assert len(set(per.tolist())) > 40
    # the prefix that fits the small-batch launch sequence holds both strata
    n = TF.certs_within(b, 4096)
    assert sum(k.startswith("deep") for k in fz.kind[:n]) >= 8 and fz.kind[:n].count("small") >= 24
    # 32-certificate chunks on both sides of the small-batch threshold (R = 4: the chunked test's batch)
    cgo = np.asarray(b.cert_grant_off, np.int64)
    chunk = np.diff(cgo[np.r_[np.arange(0, b.n_certs, 32), b.n_certs]])
    assert chunk.max() > 4096 and chunk.min() < 4096
    # separate copies: no two grants share an offset; shared copies: most do
    assert len(set(b.grant_off.tolist())) == b.n_grants
    sh = TF.shared_copies(b)
    assert len(set(sh.grant_off.tolist())) < b.n_grants // 2
    def grant_bytes(x):
        return [x.grant_bytes[int(o):int(o) + int(n)].tobytes() for o, n in zip(x.grant_off, x.grant_len)]

    assert grant_bytes(sh) == grant_bytes(b)


@pytest.mark.parametrize("strict,qm,csr", PARAMS)
def test_coverage(fz, tallies, strict, qm, csr):
    b = fz.batch
    v = tallies[strict, qm, csr]
    reason, fail_op = v.cert_reason, v.cert_fail_op
    n_ops = np.diff(np.asarray(b.cert_op_off, np.int64))
    # every reason code.  Under MOCHI_Q_BIND HASH_MISMATCH (4) cannot occur: a grant counts only
    # if its transactionHash equals the expected hash, so a counted g0 always passes :591.
    want = {0, 1, 2, 3, 4, 5, 6, 8, 9, 10} - ({mh.REJECT_HASH_MISMATCH} if qm & mh.Q_BIND else set())
    assert want <= set(np.unique(reason).tolist()), sorted(want - set(np.unique(reason).tolist()))
    assert mh.UNDECIDED not in reason
    # accepted certificates with ops past a 32-bit mask, and at the limit
    acc = v.cert_accept
    assert (acc == (reason == mh.ACCEPT)).all()
    assert (acc & (n_ops >= 33)).any() and (acc & (n_ops == 64)).any()
    # failing ops at index >= 32, per reason
    deep_fail = [mh.REJECT_NO_GRANT, mh.REJECT_BELOW_QUORUM, mh.REJECT_NO_SVOC, mh.REJECT_STORED_CERT,
                 mh.REJECT_NOT_WRITE] + ([mh.REJECT_HASH_MISMATCH] if qm == 0 else [])
    for r in deep_fail:
        assert ((reason == r) & (fail_op >= 32) & (fail_op != 0xFF)).any(), mh.REASON_NAMES[r]
    # every op decision at op indices >= 32
    _, j = op_index(b)
    assert set(np.unique(v.op_decision[j >= 32]).tolist()) == {mh.OPD_SKIPPED, mh.OPD_APPLY, mh.OPD_READ,
                                                              mh.OPD_WRONG_SHARD, mh.OPD_FAILED}
    # some op's g0 is not the first grant filed under its slot
    cert, _ = op_index(b)
    cgo = np.asarray(b.cert_grant_off, np.int64)
    behind = False
    for o in np.nonzero(v.op_g0 != 0xFFFFFFFF)[0]:
        c = cert[o]
        first = cgo[c] + int(np.argmax(b.grant_key[cgo[c]:cgo[c + 1]] == b.op_key[o]))
        if cgo[c] + int(v.op_g0[o]) != first:
            behind = True
            break
    assert behind
    # an earlier apply to the same slot DECIDES a later op (applied_before): the op would read its
    # stored certificate (HAS_CURRENT_C, op_object_ts > g0's timestamp) but that certificate is now
    # the incoming one, so it applies.  `high`: every such earlier apply sits at an op index >= 32.
    decided = high = 0
    for c in np.nonzero(n_ops >= 33)[0]:
        o0 = int(b.cert_op_off[c])
        sl = slice(o0, o0 + n_ops[c])
        d, k, fl = v.op_decision[sl], b.op_key[sl], b.op_flags[sl]
        for q in np.nonzero((d == mh.OPD_APPLY) & (fl == 7) & (b.op_object_ts[sl] > v.op_ts[sl]))[0]:
            earlier = np.nonzero((k[:q] == k[q]) & (d[:q] == mh.OPD_APPLY))[0]
            assert earlier.size  # nothing else makes such an op apply
            decided += 1
            high += int(earlier.min() >= 32)
    assert decided >= 50 and high >= 5, (decided, high)
    # the leading certificates that fit the small-batch launch sequence reach past op 32 as well
    n = TF.certs_within(b, 4096)
    o_n = int(b.cert_op_off[n])
    assert (acc[:n] & (n_ops[:n] >= 33)).any()
    assert ((fail_op[:n] >= 32) & (fail_op[:n] != 0xFF)).any()
    assert set(np.unique(v.op_decision[:o_n][j[:o_n] >= 32]).tolist()) == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("strict", [True, False])
def test_quorum_modes_change_verdicts(fz, tallies, strict):
    base = tallies[strict, 0, True].cert_reason
    for qm in (mh.Q_DISTINCT_SIGNERS, mh.Q_BIND):
        other = tallies[strict, qm, True]
        assert ((base == mh.ACCEPT) != (other.cert_reason == mh.ACCEPT)).any(), qm
    # REJECT_TS_MISMATCH survives the bind modes (skew and hash are drawn independently)
    assert (tallies[strict, mh.Q_BIND, True].cert_reason == mh.REJECT_TS_MISMATCH).any()
    # the MultiGrant CSR matters: some verdict differs when MultiGrants are signer runs
    assert (tallies[strict, 0, False].cert_reason != base).any()


def test_planted_faults_land_where_planted(fz, tallies):
    """Reference parity mode, R as built: each deep certificate's verdict is its planted fault's."""
    v = tallies[True, 0, True]
    by = {"none": mh.ACCEPT, "drop_all": mh.REJECT_NO_GRANT, "evil_first": mh.REJECT_HASH_MISMATCH,
          "bad_then_evil": mh.REJECT_HASH_MISMATCH, "ts_last": mh.REJECT_TS_MISMATCH, "flag1": mh.REJECT_NO_SVOC,
          "flag15": mh.REJECT_STORED_CERT, "flag19": mh.REJECT_NOT_WRITE}
    seen = set()
    for c, cert in enumerate(fz.certs):
        if not cert.kind.startswith("deep"):
            continue
        fault = cert.kind.split(":")[1]
        seen.add(fault)
        if fault == "drop_but_two":
            assert v.cert_reason[c] in (mh.REJECT_BELOW_QUORUM, mh.REJECT_APPLY_STATE), cert.kind
        elif fault == "bad_then_evil":  # R - 1 grants count: the quorum check (:590) comes before the hash (:591)
            mult = sum(s == cert.ops[cert.fault_op][0] for s, _, _ in cert.ops)
            below = (fz.R - 1) * mult <= mh.majority(fz.R)
            assert v.cert_reason[c] == (mh.REJECT_BELOW_QUORUM if below else mh.REJECT_HASH_MISMATCH), cert.kind
        else:
            assert v.cert_reason[c] == by[fault], cert.kind
        want_op = 0xFF if fault in ("none", "ts_last") else cert.fault_op
        assert v.cert_fail_op[c] == want_op, cert.kind
    assert seen == set(TF.DEEP_FAULTS)


def test_wire_form_decodes_to_the_same_certificate():
    """wire_message(): the oracle's decoder reads back the grants, signers and op slots' sharing."""
    R = 4
    cert = TF.deep_cert(np.random.default_rng(5), R, 33, 32, 16, "none")
    wb = TF.wire_batch([cert], R)
    import workload as W

    ids, off = W.server_id_table(R)
    d = O.w2_decode(wb, ids, off)
    assert d["msg_status"].tolist() == [mh.MSG_OK]
    assert d["cert_op_off"].tolist() == [0, 33] and d["cert_grant_off"].tolist() == [0, 16 * R]
    assert d["signer"].tolist() == [m for m in range(R) for _ in range(16)]
    slots = [s for s, _, _ in cert.ops]
    same = [[a == b for b in slots] for a in slots]
    assert [[a == b for b in d["op_key"]] for a in d["op_key"]] == same
