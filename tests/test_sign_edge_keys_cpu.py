"""The device signer's test keys and messages (tests/rsa_edge_vectors.py) on the CPU:
private_pem writes keys OpenSSL loads and signs with exactly as the plain Python CRT
does, the short-exponent fixture is what its generator produces, the key set covers
the exponent lengths and top windows k_rsa_sign's mont_pow branches on, every key's
messages reach each Garner path, and the signer refuses the one edge key whose prime
does not fit its 1024-bit fields.  (The same keys on the device:
tests/test_sign_edges_gpu.py.)
"""
import json
import os
import sys
from collections import Counter

import numpy as np
import pytest

import mochi_hip as mh
import oracle_ffi as O
import rsa_edge_vectors as EV

KEYS = {k.name: k for k in EV.signer_test_keys()}


def _sparse():
    return next(k for k in EV.edge_keys() if k.name == "sparse")


def test_private_pem_round_trips():
    keys = list(EV.signer_test_keys()) + [_sparse(), EV.swapped(_sparse())]
    keys += [EV.swapped(k) for k in EV.short_exponent_keys()]
    for k in keys:
        n, e, d, p, q, dp, dq, qinv = EV.rsa_private(EV.private_pem(k.p, k.q))
        assert (n, e, p, q, dp, dq, qinv) == (k.n, EV.E, k.p, k.q, k.dp, k.dq, k.qinv), k.name
        assert d * EV.E % ((p - 1) * (q - 1)) == 1
    # the reader's inverse: a committed key comes back with the same numbers
    s0 = EV.server_key(0)
    assert EV.rsa_private(EV.private_pem(s0.p, s0.q))[3:] == (s0.p, s0.q, s0.dp, s0.dq, s0.qinv)


@pytest.mark.parametrize("name", sorted(KEYS))
def test_openssl_signs_like_the_python_crt(name):
    key = KEYS[name]
    pem = EV.key_pem(key)
    assert O.pem_modulus(pem) == key.modulus_be and mh.pem_modulus(pem) == key.modulus_be
    msgs = EV.signer_messages(key).msgs[:8]
    blob, off, ln = EV.pack_messages(msgs)
    bulk = mh.sign_grants(pem, blob, off, ln, 2)
    for i, msg in enumerate(msgs):
        want = key.raw_sign(EV.em(msg)).to_bytes(256, "big")
        assert O.rsa_sign(pem, msg) == want and bulk[i].tobytes() == want, (name, i)
        assert O.rsa_verify(key.modulus_be, msg, want)


def test_fixture_is_what_the_generator_produces(golden_dir):
    sys.path.insert(0, golden_dir)
    try:
        import make_sign_edge_keys as G
    finally:
        sys.path.remove(golden_dir)
    doc = json.load(open(os.path.join(golden_dir, "sign_edge_keys.json")))
    built = G.build()
    assert doc["e"] == EV.E and list(doc["keys"]) == list(built)
    for name, (p, q) in built.items():
        assert doc["keys"][name] == {"p": f"{p:x}", "q": f"{q:x}"}, name
    assert [k.name for k in EV.short_exponent_keys()] == list(built)


def test_signer_key_set_covers_the_exponent_shapes():
    keys = EV.signer_key_set()
    assert len(EV.short_exponent_keys()) in (4, 5) and len(keys) == 8 + len(EV.short_exponent_keys()) + 7
    shapes = []
    for k in keys:
        assert k.n.bit_length() == 2048 and k.p.bit_length() <= 1024 and k.q.bit_length() <= 1024, k.name
        assert k.dp == pow(EV.E, -1, k.p - 1) and k.dq == pow(EV.E, -1, k.q - 1), k.name
        shapes += [EV.exponent_shape(k.dp), EV.exponent_shape(k.dq)]
    for bits, top in shapes:  # mont_pow's own reading of the exponent
        assert 2 <= bits <= 1024 and 1 <= top <= 15 and top.bit_length() == (bits - 1) % 4 + 1
    bits = [b for b, _ in shapes]
    tops = [t for _, t in shapes]
    assert {b % 4 for b in bits} == {0, 1, 2, 3}
    assert min(bits) <= 1010 and max(bits) == 1024
    assert 1 in tops and max(tops) >= 8
    # the server keys alone leave the gap this set closes
    server = [EV.exponent_shape(e)[0] for i in range(7) for e in (EV.server_key(i).dp, EV.server_key(i).dq)]
    assert 1 not in {b % 4 for b in server} and min(server) >= 1020
    # structured primes: low limb +-1 (p0inv = 2^28 - 1 or 1), just under 2^1024, just over 2^1023.5
    by = {k.name: k for k in keys}
    n0inv = lambda m: (-pow(m, -1, 1 << 28)) % (1 << 28)
    assert n0inv(by["low_limb_one"].p) == (1 << 28) - 1 and n0inv(by["low_limb_one"].q) == (1 << 28) - 1
    assert n0inv(by["low_limb_minus_one"].q) == 1 and n0inv(by["low_limb_minus_one/swapped"].p) == 1
    assert (1 << 1024) - by["top_ones"].p < 1 << 20 and (1 << 1024) - by["top_ones"].q < 1 << 20
    assert by["above_2_2047"].p ** 2 >> 1040 == 1 << 1007  # p^2 = 2^2047 + small
    # one key with p < q and (q - p) / q >= 1/8: m2 >= p is common
    assert any(k.p < k.q and 8 * (k.q - k.p) >= k.q for k in EV.short_exponent_keys())


@pytest.mark.parametrize("name", sorted(KEYS))
def test_signer_messages_reach_every_garner_class(name):
    key = KEYS[name]
    sm = EV.signer_messages(key)
    assert len(sm.msgs) == EV.SIGNER_MESSAGES == 257 and len(set(sm.msgs)) == 257
    assert 32 <= len(sm.classes) <= 257
    reachable = ["m1>=m2", "m1<m2"]
    if key.p < key.q and key.q - key.p > 1 << 1018:
        reachable += ["m2<p", "m2>=p"]
    assert list(EV.garner_reachable(key)) == reachable
    # the classes again, from the definitions
    count = Counter()
    for msg, cls in zip(sm.msgs, sm.classes):
        EM = EV.em(msg)
        m1, m2 = pow(EM, key.dp, key.p), pow(EM, key.dq, key.q)
        mine = ["m1>=m2" if m1 >= m2 % key.p else "m1<m2"]
        if len(reachable) == 4:
            mine.append("m2>=p" if m2 >= key.p else "m2<p")
        assert list(cls) == mine
        count.update(mine)
        # Garner from the two halves is the signature
        h = (key.qinv * (m1 - m2)) % key.p
        assert pow(m2 + h * key.q, EV.E, key.n) == EM
    assert all(count[c] >= 4 for c in reachable), (name, dict(count))


def test_some_keys_reach_the_m2_ge_p_path():
    four = [k.name for k in EV.signer_test_keys() if len(EV.garner_reachable(k)) == 4]
    assert "short_gap" in four and "low_limb_one/swapped" in four and "low_limb_one" not in four


@pytest.mark.parametrize("order", ["p_q", "q_p"])
def test_signer_refuses_a_1025_bit_prime(order):
    """SignKey's primes and exponents are 1024-bit fields: `sparse` = nextprime(2^1023) *
    nextprime(2^1024) is a valid RSA-2048 key (OpenSSL signs with it) that does not fit.
    The key is checked before the device is looked for."""
    k = _sparse() if order == "p_q" else EV.swapped(_sparse())
    assert max(k.p.bit_length(), k.q.bit_length()) == 1025 and k.n.bit_length() == 2048
    pem = EV.key_pem(k)
    msg = EV.grant_message("sparse")
    assert O.rsa_sign(pem, msg) == k.raw_sign(EV.em(msg)).to_bytes(256, "big")
    with pytest.raises(mh.MochiError, match="not an RSA-2048 private key with CRT parameters"):
        mh.DeviceSigner(pem, 0)
