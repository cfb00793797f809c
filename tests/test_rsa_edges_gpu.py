"""The RSA kernels against forged near-miss signatures, structured operands and edge
moduli (needs an MI355X).  Every comparison is exact.

tests/rsa_edge_vectors.py makes, from the committed private test keys, signatures
whose s^65537 mod n differs from the expected encoding in one chosen limb, bit or
byte -- for each of the 74 compare positions of k_rsa_final / k_rsa_final_lat one
forgery differs there alone (asserted in tests/test_rsa_edge_vectors_cpu.py) -- and
operands whose limbs are all ones, all zeros, equal halves or single bits, under
moduli with an all-ones top, a long zero run, almost no set bits and n == +-1 (mod
2^28).  Every test runs under both launch sequences: the small-batch one
(k_bucket_small, k_rsa_pow_lat, k_rsa_final_lat) and the large-batch one
(k_bucket_*, k_rsa_pow, k_rsa_final).
"""
import contextlib

import numpy as np
import pytest

import fold_model as FM
import mochi_hip as mh
import oracle_ffi as O
import rsa_edge_vectors as EV

pytestmark = pytest.mark.gpu

SMALL_DEFAULT = 4096


@contextlib.contextmanager
def launch_sequence(ver, seq):
    """`small`: the default (batches of up to 4096 grants take the small-batch
    sequence); `large`: never.  The default is restored afterwards."""
    ver.set_small_batch(SMALL_DEFAULT if seq == "small" else 0)
    try:
        yield ver
    finally:
        ver.set_small_batch(SMALL_DEFAULT)


@pytest.fixture(scope="module")
def server_set():
    kvs = EV.server_vectors()
    ver = mh.Verifier([kv.key.modulus_be for kv in kvs], 0)
    yield kvs, ver
    ver.close()


@pytest.fixture(scope="module")
def edge_set():
    kvs = EV.edge_vectors()
    ver = mh.Verifier([kv.key.modulus_be for kv in kvs], 0)
    yield kvs, ver
    ver.close()


@pytest.fixture(scope="module")
def chain_set():
    """The seven moduli of the residue checks with the model's 16-step chain results."""
    moduli = EV.chain_moduli()
    ver = mh.Verifier([n.to_bytes(256, "big") for _, n in moduli], 0)
    yield [(name, n, EV.model_chain(n)) for name, n in moduli], ver
    ver.close()


def _interleave(kvs):
    """[(signer, msg, vector)]: the keys' vectors round-robin, so valid and forged
    signatures and the signers alternate through the batch."""
    out, depth = [], max(len(kv.vectors) for kv in kvs)
    for i in range(depth):
        for k, kv in enumerate(kvs):
            if i < len(kv.vectors):
                out.append((k, kv.msg, kv.vectors[i]))
    return out


def _batch(items):
    """Every grant its own one-grant certificate with its own copy of the signed bytes."""
    n = len(items)
    msgs = [m for _, m, _ in items]
    blob = np.frombuffer(b"".join(msgs), np.uint8).copy()
    off = np.cumsum([0] + [len(m) for m in msgs[:-1]]).astype(np.uint64)
    return mh.Batch(
        grant_bytes=blob, grant_off=off, grant_len=np.array([len(m) for m in msgs], np.uint32),
        sig=np.frombuffer(b"".join(v.sig for _, _, v in items), np.uint8).reshape(n, 256).copy(),
        signer=np.array([k for k, _, _ in items], np.uint16), grant_key=np.zeros(n, np.uint8),
        cert_grant_off=np.arange(n + 1, dtype=np.uint32), cert_op_off=np.zeros(n + 1, np.uint32),
        op_key=np.zeros(0, np.uint8), op_flags=np.zeros(0, np.uint8), expected_hash=np.zeros((n, 128), np.uint8))


def _check_flags(ver, moduli, items, what):
    b = _batch(items)
    g = ver.verify(b, 4, True)
    o = O.verify_batch(moduli, b, 4, True, 4)
    truth = np.array([v.valid for _, _, v in items])
    names = [(k, v.name) for k, _, v in items]
    got = (g.grant_flags & mh.GRANT_SIG_OK) != 0
    wrong = [names[i] for i in np.nonzero(got != truth)[0]]
    assert not wrong, f"{what}: verdict differs from the constructed truth for {wrong}"
    assert ((o.grant_flags & mh.GRANT_SIG_OK) != 0).tolist() == truth.tolist(), what
    np.testing.assert_array_equal(g.grant_flags, o.grant_flags, err_msg=what)
    np.testing.assert_array_equal(g.grant_ts, o.grant_ts, err_msg=what)
    np.testing.assert_array_equal(g.cert_accept_bits, o.cert_accept_bits, err_msg=what)
    assert (g.grant_flags & mh.GRANT_PARSED).all(), what
    return int(got.sum())


@pytest.mark.parametrize("seq", ["small", "large"])
@pytest.mark.parametrize("keys", ["server", "edge"])
def test_forged_near_miss_rejected(keys, seq, server_set, edge_set):
    """One batch per key set holding every near-miss vector and the valid ones: the
    device rejects exactly the forgeries -- flags == the oracle's (OpenSSL) == the
    truth by construction -- and accepts one signature per key."""
    kvs, ver = server_set if keys == "server" else edge_set
    items = _interleave(kvs)
    assert 700 <= len(items) <= 900
    with launch_sequence(ver, seq):
        n_valid = _check_flags(ver, [kv.key.modulus_be for kv in kvs], items, f"{keys} {seq}")
    assert n_valid == len(kvs)


def _limbs_of(row):
    return [int(v) for v in row]


@pytest.mark.parametrize("seq", ["small", "large"])
def test_chain_matches_model_bit_exact(seq, chain_set):
    """rsa_public_op on the structured operands under the seven edge moduli, several
    signers per call: y == pow(s, 65537, n) for s < n, and the chain intermediate z
    equals the fold model's 16-step result limb for limb under both sequences, so
    k_rsa_pow == k_rsa_pow_lat == tests/fold_model.py, whose assertions then bound
    what the kernels compute."""
    chains, ver = chain_set
    with launch_sequence(ver, seq):
        for lo, hi in ((0, 4), (4, len(chains))):  # two calls, several signers each
            rows = [(k, op, s, z) for k in range(lo, hi) for op, s, z in chains[k][2]]
            assert len(rows) <= 800
            sigs = np.frombuffer(b"".join(s.to_bytes(256, "big") for _, _, s, _ in rows), np.uint8)
            y, z = mh.rsa_public_op(ver, sigs, np.array([k for k, _, _, _ in rows], np.uint16), want_z=True)
            for i, (k, op, s, zm) in enumerate(rows):
                name, n = chains[k][0], chains[k][1]
                zd = _limbs_of(z[i])
                zi = FM.from_limbs(zd)
                assert max(zd) < 1 << 28 and zi < 1 << 2064, (name, op)
                assert zi % n == pow(s, 1 << 16, n), (name, op)
                assert zd == list(zm), (name, op, "device z != fold model z")
                if s < n:
                    assert int.from_bytes(y[i].tobytes(), "big") == pow(s, 65537, n), (name, op)


@pytest.mark.parametrize("count", [1, 31, 32, 33, 63, 64, 65])
def test_signer_chunk_edges(count, server_set):
    """The small sequence's 64-slot chunks: one signer with exactly `count` grants (a
    chunk with slots 32..63 empty folds one N-tile only; 33 and 65 put one grant
    past the boundary) beside a signer with 3, valid and forged signatures
    alternating.  Flags == oracle == truth, and rsa_public_op's residues are the
    vectors' targets.  (Slot order inside a bucket is unspecified: nothing is
    asserted per slot.)"""
    kvs, ver = server_set
    a, b = kvs[0], kvs[1]
    items = [(0, a.msg, a.vectors[0] if i % 2 == 0 else a.vectors[1 + i // 2]) for i in range(count)]
    other = [(1, b.msg, b.vectors[j]) for j in (0, 5, 0)]
    for j, it in enumerate(other):  # the second signer's grants spread through the batch
        items.insert(min(len(items), (j * count) // 2 + j), it)
    assert sum(1 for k, _, _ in items if k == 0) == count and len(items) == count + 3
    moduli = [kv.key.modulus_be for kv in kvs]
    with launch_sequence(ver, "small"):
        n_valid = _check_flags(ver, moduli, items, f"count={count}")
        sigs = np.frombuffer(b"".join(v.sig for _, _, v in items), np.uint8)
        y = mh.rsa_public_op(ver, sigs, np.array([k for k, _, _ in items], np.uint16))
    assert n_valid == (count + 1) // 2 + 2
    for i, (k, _, v) in enumerate(items):
        assert int.from_bytes(y[i].tobytes(), "big") == v.y, (count, i, v.name)
