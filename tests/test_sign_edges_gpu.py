"""The device signer (k_rsa_sign: rsa_sign.hip, mont_crt.h, sha256_dev.h) at its key and
length edges, byte for byte against OpenSSL and the plain Python CRT.

A signer bug does not show as a wrong signature: the public-key check after
k_rsa_sign zeroes the row and counts it.  Every test here compares the bytes AND
reads rejected().

  keys      the constructed moduli of tests/golden/edge_moduli.json in both prime
            orders (low limb +-1, primes just under 2^1024 and just over 2^1023.5) and
            the short-exponent keys of tests/golden/sign_edge_keys.json (exponent
            lengths in every residue mod 4, top windows 1..13), on 257 messages that
            reach each of Garner's paths (tests/test_sign_edge_keys_cpu.py asserts it)
  batches   0, 1, 63..65, 255..257 grants, both entry points
  SHA-256   every length 0..191, 247..257, 4095..4097 at each of the 16 alignments,
            sorted (whole waves of full blocks) and shuffled (mixed block counts)
"""
import hashlib

import numpy as np
import pytest

import mochi_hip as mh
import rsa_edge_vectors as EV
import workload as W

pytestmark = pytest.mark.gpu

KEYS = {k.name: k for k in EV.signer_test_keys()}


@pytest.mark.parametrize("name", list(KEYS))
def test_edge_key_signatures_exact(name):
    key = KEYS[name]
    pem = EV.key_pem(key)
    sm = EV.signer_messages(key)
    blob, off, ln = EV.pack_messages(sm.msgs)
    assert len(off) == 257
    ref = mh.sign_grants(pem, blob, off, ln, 8)
    s = mh.DeviceSigner(pem, 0)
    try:
        got = s.sign(blob, off, ln)  # one launch: a full block and one lane of a second
        rejected = s.rejected()
    finally:
        s.close()
    bad = np.nonzero((got != ref).any(axis=1))[0]
    assert bad.size == 0, (name, "rows differing from OpenSSL", bad[:16].tolist(),
                           [sm.classes[i] for i in bad[:16] if i < len(sm.classes)])
    for i in range(32):
        assert got[i].tobytes() == key.raw_sign(EV.em(sm.msgs[i])).to_bytes(256, "big"), (name, i, sm.classes[i])
    assert rejected == 0


def test_batch_size_edges():
    import torch

    key = KEYS["low_limb_one/swapped"]  # p < q: all four Garner paths
    pem = EV.key_pem(key)
    msgs = EV.signer_messages(key).msgs
    blob, off, ln = EV.pack_messages(msgs)
    ref = mh.sign_grants(pem, blob, off, ln, 8)
    for i in range(32):
        assert ref[i].tobytes() == key.raw_sign(EV.em(msgs[i])).to_bytes(256, "big")
    d = torch.device("cuda", 0)
    bt = torch.from_numpy(blob).to(d)
    ot = torch.from_numpy(off.view(np.int64)).to(d)
    lt = torch.from_numpy(ln.view(np.int32)).to(d)
    fill = np.arange(264 * 256, dtype=np.uint32).astype(np.uint8).reshape(264, 256) | 1  # no zero row
    s = mh.DeviceSigner(pem, 0)
    try:
        for n in (0, 1, 63, 64, 65, 255, 256, 257):
            got = s.sign(blob, off[:n], ln[:n])
            assert got.shape == (n, 256)
            np.testing.assert_array_equal(got, ref[:n], err_msg=f"sign n={n}")
            assert s.rejected() == 0
            st = torch.from_numpy(fill).to(d)
            s.sign_device(bt, ot, lt, n, st, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            out = st.cpu().numpy()
            np.testing.assert_array_equal(out[:n], ref[:n], err_msg=f"sign_device n={n}")
            np.testing.assert_array_equal(out[n:], fill[n:], err_msg=f"sign_device n={n}: rows past n")
            assert s.rejected() == 0
    finally:
        s.close()


SHA_LENGTHS = list(range(0, 192)) + list(range(247, 258)) + [4095, 4096, 4097]


def _sha_sweep():
    """Seeded random bytes (about half with the high bit set) of every SHA_LENGTHS length
    at every offset residue mod 16, sorted by (length, residue): 3,296 messages."""
    blob, off, ln = bytearray(), [], []
    for n in SHA_LENGTHS:
        for r in range(16):
            blob += b"\xa5" * ((r - len(blob)) % 16)
            off.append(len(blob))
            ln.append(n)
            seed = hashlib.sha256(f"sha sweep {n} {r}".encode()).digest()
            blob += hashlib.shake_128(seed).digest(n)
    blob += b"\x5a" * 16
    return np.frombuffer(bytes(blob), np.uint8).copy(), np.array(off, np.uint64), np.array(ln, np.uint32)


def test_sha256_lengths_and_alignments_through_the_signer():
    pem = W.load_keys(1)[0]
    blob, off, ln = _sha_sweep()
    n = len(off)
    assert n == 16 * len(SHA_LENGTHS) and sorted(set((off % 16).tolist())) == list(range(16))
    for length in SHA_LENGTHS:
        assert sorted((off[ln == length] % 16).tolist()) == list(range(16))
    assert {x % 64 for x in SHA_LENGTHS} == set(range(64))
    assert 0.4 < (blob >= 0x80).mean() < 0.6
    # sorted: some wave (64 consecutive lanes from a multiple of 64) holds only messages of
    # >= 128 bytes -- its first two blocks are full in every lane
    assert any((ln[w:w + 64] >= 128).all() for w in range(0, n - 63, 64))
    ref = mh.sign_grants(pem, blob, off, ln, 8)
    perm = np.random.default_rng(20).permutation(n)
    blocks = (ln[perm].astype(np.int64) + 9 + 63) >> 6
    assert all(len(set(blocks[w:w + 64].tolist())) > 1 for w in range(0, n - 63, 64))  # mixed block counts
    s = mh.DeviceSigner(pem, 0)
    try:
        got = s.sign(blob, off, ln)
        rej_sorted = s.rejected()
        got_p = s.sign(blob, off[perm], ln[perm])
        rej_shuffled = s.rejected()
    finally:
        s.close()
    for what, g, r in (("sorted", got, ref), ("shuffled", got_p, ref[perm])):
        bad = np.nonzero((g != r).any(axis=1))[0]
        o, l = (off, ln) if what == "sorted" else (off[perm], ln[perm])
        assert bad.size == 0, (what, "(length, offset mod 16) of the rows differing from OpenSSL",
                               [(int(l[i]), int(o[i] % 16)) for i in bad[:24]])
    assert rej_sorted == 0 and rej_shuffled == 0
