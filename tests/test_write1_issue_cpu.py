"""Write1 grant issuance, host form (mochi_write1_issue) against the sequential
model of the reference's Write1 path (write1_issue_model.py): decisions, request
kinds, reply views, new-grant numbering and Grant bytes, all exact."""
import os
import sys

import numpy as np
import pytest

import mochi_hip as mh
import oracle_ffi as O
import write1_issue_model as M


@pytest.fixture(scope="module")
def cases():
    """name -> (batch, host outputs, model outputs, requests, store before the batch)."""
    out = {}
    for name, (store, reqs, pad) in M.all_cases().items():
        M.prepare(store, reqs)
        batch = M.build_batch(store, reqs, pad)
        want = M.run(M.copy_store(store), reqs)
        out[name] = (batch, mh.write1_issue(batch), want, reqs, store)
    return out


CASE_NAMES = sorted(M.hand_cases()) + sorted(M.edge_cases()) + [f"random{i}" for i in range(6)] + ["alignment"]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_host_form_equals_the_model(cases, name):
    batch, got, want, _, _ = cases[name]
    M.assert_matches(got, want)
    assert mh.write1_issue_bound(batch) >= got.grant_bytes_len


def test_the_case_sets_reach_every_branch(cases):
    """Every decision and kind occurs, and the hand-built cases are the ones the names say."""
    seen_d, seen_k = set(), set()
    for _, got, _, _, _ in cases.values():
        seen_d.update(got.op_decision.tolist())
        seen_k.update(got.req_kind.tolist())
    assert seen_d == set(range(7)) and seen_k == {0, 1, 2}
    D = lambda name: cases[name][1].op_decision.tolist()
    K = lambda name: cases[name][1].req_kind.tolist()
    # the winner's own request is REFUSED / THROWS, its grant stands and later requests meet it
    assert D("winner_refused") == [mh.W1D_NEW, mh.W1D_REFUSED, mh.W1D_REFUSED, mh.W1D_RETRY]
    assert K("winner_refused") == [mh.W1K_REFUSED, mh.W1K_REFUSED, mh.W1K_OK]
    assert cases["winner_refused"][1].op_grant.tolist() == [0, mh.W1_STORED | 0, 0, 0]
    assert D("winner_throws") == [mh.W1D_NEW, mh.W1D_FAILED, mh.W1D_NEW, mh.W1D_REFUSED, mh.W1D_REFUSED]
    assert K("winner_throws") == [mh.W1K_THROWS, mh.W1K_REFUSED, mh.W1K_REFUSED]
    # ops behind the empty key claim nothing: request 1 wins e and f
    assert D("empty_mid") == [mh.W1D_NEW, mh.W1D_FAILED, mh.W1D_SKIPPED, mh.W1D_SKIPPED, mh.W1D_SKIP, mh.W1D_SKIPPED,
                              mh.W1D_NEW, mh.W1D_NEW, mh.W1D_FAILED, mh.W1D_SKIPPED]
    assert D("delete_absent") == [mh.W1D_FAILED, mh.W1D_NEW, mh.W1D_FAILED, mh.W1D_REFUSED]
    g = cases["same_key_twice"][1]
    assert g.op_decision.tolist()[:7] == [mh.W1D_NEW, mh.W1D_RETRY, mh.W1D_RETRY] + [mh.W1D_WRONG_SHARD] * 4
    assert g.op_grant.tolist()[:7] == [0, 0, 0, 1, 1, 2, 1]
    assert g.req_grant.tolist()[:3] == [0, 1, 2]  # each distinct grant once, at its first op
    assert D("read_between")[:4] == [mh.W1D_NEW, mh.W1D_SKIP, mh.W1D_NEW, mh.W1D_SKIP]
    # an empty hash against an empty hash is a RETRY
    assert D("hash_len")[-2:] == [mh.W1D_RETRY, mh.W1D_RETRY]


def test_new_grants_parse_back(cases):
    """Each new grant, parsed by the oracle, gives back objectId, timestamp, hash and status."""
    for name, (batch, got, _, reqs, _) in cases.items():
        keys = [key for r in reqs for _, key in r.ops]
        req_of = np.repeat(np.arange(len(reqs)), [len(r.ops) for r in reqs])
        for g in range(got.n_new):
            o = int(got.grant_op[g])
            v = O.grant_parse(got.grant(g))
            ws = got.op_decision[o] == mh.W1D_WRONG_SHARD
            assert v is not None and v["object_id"] == keys[o], name
            assert v["transaction_hash"] == reqs[int(req_of[o])].txn_hash
            assert v["timestamp"] == int(got.grant_ts[g]) and v["status"] == (1 if ws else 0) and v["configstamp"] == 0
            assert (v["timestamp"] == 0) if ws else (got.op_decision[o] == mh.W1D_NEW)


def test_byte_edges_are_covered(cases):
    """The edge sets put lengths and timestamps on both sides of every varint step."""
    ts = set()
    for name in ("ts_steps", "ts_from_seed", "negative_epoch"):
        ts.update(cases[name][1].grant_ts.tolist())
    assert {0, 127, 128, 16383, 16384, 1 << 31, (1 << 32) - 1, (1 << 63) - 1, -(1 << 63), -4999} <= ts
    assert {len(cases["ts_steps"][1].grant(g)) for g in range(7)} == {136 + n for n in (0, 2, 3, 4, 6, 10)}
    neg = cases["negative_epoch"][1]
    assert len(neg.grant(0)) == 2 + 1 + 11 + 131  # a negative timestamp is a ten-byte varint
    assert sorted(set(cases["key_len"][0].op_key_len.tolist())) == [1, 4, 127, 128, 130, 131]
    assert sorted(set(cases["hash_len"][0].req_hash_len.tolist())) == [0, 1, 127, 128, 129]
    assert int(cases["ts_from_seed"][0].req_seed.max()) == (1 << 32) - 1
    assert len(M.payload_residues(cases["alignment"][0], cases["alignment"][1])) == 256


def test_grant_bytes_are_what_google_protobuf_reads(cases):
    """The model's byte source (the oracle encoder) cross-checked once by an
    independent protobuf implementation, through the host form's output."""
    pytest.importorskip("google.protobuf")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_write2_golden as G

    _, Grant = G.classes()
    for name in ("key_len", "hash_len", "ts_steps", "negative_epoch", "same_key_twice"):
        _, got, want, _, _ = cases[name]
        for g in range(got.n_new):
            m = Grant()
            m.ParseFromString(got.grant(g))
            assert m.SerializeToString() == got.grant(g) == want["grants"][g]
            assert m.objectId.encode() == want["new"][g].object_id and m.timestamp == want["new"][g].ts
            assert m.transactionHash.encode() == want["new"][g].txn_hash


def test_capacity_rule(cases):
    batch, got, _, _, _ = cases["random0"]
    need = got.grant_bytes_len
    assert need > 0
    for cap in (0, 1, need - 1):
        buf = np.full(max(cap, 1), 0xEE, np.uint8)
        r = mh.write1_issue_into(batch, buf if cap else None)
        assert r.rc == mh.EINVAL and r.grant_bytes_len == need and r.n_new == got.n_new
        assert (buf == 0xEE).all()  # no grant byte written
        np.testing.assert_array_equal(r.op_decision, got.op_decision)
        np.testing.assert_array_equal(r.req_kind, got.req_kind)
        np.testing.assert_array_equal(r.req_grant_off, got.req_grant_off)
    buf = np.full(need + 32, 0xEE, np.uint8)
    r = mh.write1_issue_into(batch, buf)
    assert r.rc == mh.OK and (buf[need:] == 0xEE).all() and buf[:need].tobytes() == got.grant_bytes[:need].tobytes()


def _mutated(batch, **kw):
    d = {k: np.array(getattr(batch, k)) for k in mh.Write1Batch.DTYPES}
    d.update(kw)
    return mh.Write1Batch(**d)


def test_inconsistent_inputs_are_rejected(cases):
    batch = cases["stored"][0]
    assert mh.write1_issue(batch).rc == mh.OK
    O_, Q = batch.n_ops, batch.n_reqs
    L = int(batch.strings.size)

    def at(arr, i, v):
        a = np.array(arr)
        a[i] = v
        return a

    bad = dict(
        csr_start=("CSR", _mutated(batch, req_op_off=at(batch.req_op_off, 0, 1))),
        csr_end=("CSR", _mutated(batch, req_op_off=at(batch.req_op_off, Q, O_ - 1))),
        csr_order=("CSR", _mutated(batch, req_op_off=at(at(batch.req_op_off, 1, 3), 2, 1))),
        key_outside=("key lies outside", _mutated(batch, op_key_off=at(batch.op_key_off, 0, L))),
        key_too_long=("key lies outside", _mutated(batch, op_key_len=at(batch.op_key_len, O_ - 1, L + 1))),
        hash_outside=("transactionHash lies outside", _mutated(batch, req_hash_off=at(batch.req_hash_off, 1, L - 5))),
        stored_outside=("stored hash lies outside", _mutated(batch, stored_hash_len=at(batch.stored_hash_len, 0, L + 1))),
        stored_index=("op_stored index", _mutated(batch, op_stored=at(batch.op_stored, 0, batch.n_stored))),
        epochs_differ=("different op_epoch", _mutated(batch, op_epoch=at(batch.op_epoch, 0, int(batch.op_epoch[0]) + 1000))),
    )
    assert int(batch.op_obj[0]) == int(batch.op_obj[1])  # op 0 and op 1 are the same container
    for name, (why, b) in bad.items():
        with pytest.raises(mh.MochiError, match=why):
            mh.write1_issue(b)
    # more than MOCHI_MAX_OPS_PER_CERT ops in one request
    n = 65
    ops = mh.Write1Batch(strings=np.frombuffer(b"kh", np.uint8), req_op_off=np.array([0, n], np.uint32),
                         req_seed=np.zeros(1, np.uint32), req_hash_off=np.ones(1, np.uint64),
                         req_hash_len=np.ones(1, np.uint32), op_key_off=np.zeros(n, np.uint64),
                         op_key_len=np.ones(n, np.uint32), op_flags=np.full(n, 0x07, np.uint8),
                         op_obj=np.zeros(n, np.uint32), op_epoch=np.zeros(n, np.int64),
                         op_stored=np.full(n, mh.W1_NONE, np.uint32), stored_hash_off=np.zeros(0, np.uint64),
                         stored_hash_len=np.zeros(0, np.uint32))
    with pytest.raises(mh.MochiError, match="MOCHI_MAX_OPS_PER_CERT"):
        mh.write1_issue(ops)
    ok = _mutated(ops, req_op_off=np.array([0, 64], np.uint32), **{k: np.array(getattr(ops, k))[:64] for k in
                  ("op_key_off", "op_key_len", "op_flags", "op_obj", "op_epoch", "op_stored")})
    r = mh.write1_issue(ok)
    assert r.rc == mh.OK and r.op_decision.tolist() == [mh.W1D_NEW] + [mh.W1D_RETRY] * 63 and r.req_grant.tolist() == [0]


def test_three_rounds_through_the_store():
    """Apply the library's outputs to a store, bump some epochs, go again: at every
    round the store equals the one the model alone builds."""
    rng = np.random.default_rng(4242)
    lib_store = M.random_store(rng)
    model_store = M.copy_store(lib_store)
    for rnd in range(3):
        reqs = M.random_reqs(rng, 50)
        for s in (lib_store, model_store):
            M.prepare(s, reqs)
        batch = M.build_batch(lib_store, reqs)
        M.build_batch(model_store, reqs)  # names the model's stored grants
        got = mh.write1_issue(batch)
        want = M.run(model_store, reqs)
        M.assert_matches(got, want)
        M.apply_outputs(lib_store, reqs, batch, got)
        assert lib_store.snapshot() == model_store.snapshot()
        assert got.n_new > 0 and (batch.op_stored != mh.W1_NONE).any() == (rnd > 0)
        for key in sorted(lib_store.data)[::3]:  # moveToNextEpochIfNecessary on some containers
            ts = max(lib_store.data[key].grants, default=0) + 1000 * rnd
            for s in (lib_store, model_store):
                s.data[key].move_to_next_epoch_if_necessary(ts)
        assert lib_store.snapshot() == model_store.snapshot()
