"""The forged near-miss vectors and structured operands of tests/rsa_edge_vectors.py on
the CPU: the references alone (OpenSSL through the oracle, the final-check replay of
test_final_algebra.py, the fold model) handle every vector, and the set is strong
enough for the limb-level mistakes it is meant to catch -- every compare position of
k_rsa_final's D' == n check, the last carry included, is the ONLY differing position
of some forged signature, so a compare that skipped one would accept a forgery.
(The same vectors on the device: tests/test_rsa_edges_gpu.py.)
"""
import json
import os

import numpy as np
import pytest

import fold_model as FM
import mochi_hip as mh
import oracle_ffi as O
import rsa_edge_vectors as EV
from test_final_algebra import CPAD, XMAX, final_check, final_diffs

SETS = {"server": EV.server_vectors, "edge": EV.edge_vectors}


def test_private_key_reader_matches_openssl():
    for i in range(7):
        pem, key = EV.server_pem(i), EV.server_key(i)
        assert key.modulus_be == O.pem_modulus(pem)
        msg = EV.grant_message(f"reader{i}")
        # PKCS#1 v1.5 signing is deterministic: the CRT signature of EM is OpenSSL's
        assert key.raw_sign(EV.em(msg)).to_bytes(256, "big") == O.rsa_sign(pem, msg)
    assert EV.CPAD == CPAD and EV.XMAX == XMAX


def test_edge_moduli_shapes(golden_dir):
    doc = json.load(open(os.path.join(golden_dir, "edge_moduli.json")))
    assert list(doc["keys"]) == ["top_ones", "above_2_2047", "sparse", "low_limb_one", "low_limb_minus_one"]
    keys = {k.name: k for k in EV.edge_keys()}
    for k in keys.values():
        assert k.n % 2 == 1 and k.n.bit_length() == 2048 and k.p * k.q == k.n
        assert (k.p - 1) % EV.E and (k.q - 1) % EV.E
    n0inv = lambda n: (-pow(n, -1, 1 << 28)) % (1 << 28)
    assert keys["top_ones"].n >> 1048 == (1 << 1000) - 1
    assert keys["above_2_2047"].n >> 1040 == 1 << 1007
    assert sum(1 for v in FM.to_limbs(keys["sparse"].n) if v == 0) > 60
    assert keys["low_limb_one"].n % (1 << 28) == 1 and n0inv(keys["low_limb_one"].n) == (1 << 28) - 1
    assert keys["low_limb_minus_one"].n % (1 << 28) == (1 << 28) - 1 and n0inv(keys["low_limb_minus_one"].n) == 1


@pytest.mark.parametrize("name", [k.name for k in EV.edge_keys()])
def test_fold_matrix_accepts_edge_modulus(name):
    n = dict(EV.chain_moduli())[name]
    img, cadd = mh.fold_matrix(n.to_bytes(256, "big"))
    img_m, cadd_m, W = FM.make_weights(n)
    np.testing.assert_array_equal(img, img_m)
    np.testing.assert_array_equal(cadd, cadd_m)
    assert np.abs(W).max() <= 128 and np.abs(W.reshape(74, 4, -1)[:, 3]).max() <= 8


def test_vector_set_sizes():
    sv, ev = EV.server_vectors(), EV.edge_vectors()
    EM0 = EV.em(sv[0].msg)
    # (every bit-28j flip equals EM + 2^(28j) or EM - 2^(28j): duplicates are signed once)
    assert len(EV.limb_set(sv[0].key.n, EM0)) >= 220 and len(EV.encoding_set(sv[0].key.n, EM0)) >= 80
    assert len(sv[0].vectors) >= 300 and all(len(kv.vectors) >= 74 for kv in sv[1:])
    assert all(len(kv.vectors) >= 140 for kv in ev)
    assert len(EV.structured_operands(sv[0].key.n)) >= 160


@pytest.mark.parametrize("which", sorted(SETS))
def test_vectors_against_openssl(which):
    for kv in SETS[which]():
        n_be = kv.key.modulus_be
        assert [v.valid for v in kv.vectors].count(True) == 1 and kv.vectors[0].valid
        for v in kv.vectors:
            s = int.from_bytes(v.sig, "big")
            assert s < kv.key.n and pow(s, EV.E, kv.key.n) == v.y, (kv.key.name, v.name)
            assert v.valid == (v.y == EV.em(kv.msg))
            assert O.rsa_verify(n_be, kv.msg, v.sig) == v.valid, (kv.key.name, v.name)


@pytest.mark.parametrize("which", sorted(SETS))
def test_final_check_isolates_every_compare_position(which):
    """The replayed final check rejects every forgery and accepts the valid signature
    for the smallest and the largest representative x < 2^2064 of s^65537, and for
    each of the 74 compare positions (D' limbs 0..72, the last carry) some forgery
    differs from n at that position ALONE."""
    for kv in SETS[which]():
        n, h = kv.key.n, EV.digest_int(kv.msg)
        isolated = set()
        for v in kv.vectors:
            s = int.from_bytes(v.sig, "big")
            top = (XMAX - 1 - v.y) // n
            for j in (0, top):
                d = final_diffs(n, v.y + j * n, h)
                assert len(d) == 74
                assert final_check(n, s, v.y + j * n, h) == v.valid == (not any(d)), (kv.key.name, v.name, j)
                nz = [k for k, x in enumerate(d) if x]
                if len(nz) == 1:
                    isolated.add(nz[0])
        assert isolated == set(range(74)), (kv.key.name, sorted(set(range(74)) - isolated))


@pytest.mark.parametrize("name", [m[0] for m in EV.chain_moduli()])
def test_fold_model_structured_chain(name):
    """16 fold_square steps from every structured operand under an edge modulus: the
    model's own assertions hold on the way (EV.model_chain), the result is
    s^(2^16) mod n and stays below 2^2064 in 28-bit limbs."""
    n = dict(EV.chain_moduli())[name]
    chain = EV.model_chain(n)
    assert len(chain) >= 160
    for op, s, z in chain:
        zi = FM.from_limbs(z)
        assert len(z) == 74 and max(z) < 1 << 28 and zi < 1 << 2064, op
        assert zi % n == pow(s, 1 << 16, n), op


@pytest.mark.parametrize("which", sorted(SETS))
def test_final_product_inside_model_bounds(which):
    """k_rsa_final's t = z*s and its fold with cnc = cadd + n - Cpad and the digest
    subtracted, in the model (64-bit columns, |t_j| < 2^29, int32 halves), for every
    near-miss signature and the extreme representatives of z; for the valid
    signature and each key's first forgeries z is the model's own 16-step chain.  The
    D it leaves gives the replayed final check's verdict."""
    for kv in SETS[which]():
        n, msg_h = kv.key.n, EV.digest_int(kv.msg)
        W, cadd = EV.model_weights(n)
        cnc = FM.to_limbs(FM.from_limbs(cadd) + n - CPAD)
        hl = FM.to_limbs(msg_h, 10)
        for idx, v in enumerate(kv.vectors):
            s = int.from_bytes(v.sig, "big")
            sl = FM.to_limbs(s)
            z0 = pow(s, 1 << 16, n)
            zs = [z0, z0 + (XMAX - 1 - z0) // n * n]
            if idx < 3:
                x = sl
                for _ in range(16):
                    x = FM.fold_square(x, W, cadd)
                zs.append(FM.from_limbs(x))
            for z in zs:
                D = FM.from_limbs(FM.fold_signed(FM.kara_terms(FM.to_limbs(z), sl), W, cnc, sub_h=hl))
                assert (D - (v.y - EV.em(kv.msg))) % n == 0 and 0 < D < XMAX + n, (kv.key.name, v.name)
                x_rep = D - (n - CPAD) + msg_h
                assert final_check(n, s, x_rep, msg_h) == v.valid, (kv.key.name, v.name)
