#!/usr/bin/env python3
"""Generate tests/golden/sign_edge_keys.json: RSA-2048 test keys for the device signer
(k_rsa_sign) whose CRT exponents are SHORT, of chosen lengths (tests/rsa_edge_vectors.py).

    python tests/golden/make_sign_edge_keys.py

k_rsa_sign's mont_pow takes its loop count and its start value from the exponent's bit
length: (bits + 3) >> 2 four-bit windows, the top window picks the first table entry.
The server keys' dp / dq have 1020..1024 bits, so lengths == 1 (mod 4) -- top window
1, start value T[1] = base -- and short exponents never occur among them.  Here a
prime p is searched with

    k (p - 1) + 1 == 0  (mod 65537),      so   dp = e^-1 mod (p - 1) = (k (p - 1) + 1) / 65537

exactly (dp e = 1 + k (p - 1), and dp < p - 1): dp has about 1008 + log2(k) bits.
Pure Python, deterministic (the primality test and the seeding of make_edge_moduli.py),
a few seconds.  TEST-ONLY keys: the factors are committed.

  short_2_4      k = 2, 4:    the shortest exponents, 1009 and 1010 bits
  short_6_8      k = 6, 8
  short_16_32    k = 16, 32:  1012 bits (top window >= 8) and 1013 bits (top window 1)
  short_gap      k = 64, 128; p < 13/16 2^1024, q >= 15/16 2^1024: (q - p) / q > 1/8, so
                 Garner's m2 >= p (m2 mod p subtracts p) holds for one message in eight
  short_3_full   k = 3 for p, an ordinary prime q: a short dp beside a full-length dq
"""
from __future__ import annotations

import json
import os

from make_edge_moduli import E, _seeded, is_prime, usable

HERE = os.path.dirname(os.path.abspath(__file__))
TOP = 1 << 1024


def _start(label: str, lo16: int = 12, hi16: int = 16) -> int:
    """A fixed starting point in [lo16, hi16) / 16 * 2^1024 (the default: the two top bits set)."""
    span = (hi16 - lo16) * (TOP >> 4)
    return lo16 * (TOP >> 4) + _seeded(label) % span


def short_exponent_prime(k: int, start: int) -> int:
    """The first prime p >= start with k (p - 1) + 1 == 0 (mod 65537)."""
    r = (1 - pow(k, -1, E)) % E  # p == 1 - 1/k
    p = start - start % E + r
    if p < start:
        p += E
    if p % 2 == 0:
        p += E
    tried = 0
    while not is_prime(p):
        p += 2 * E
        tried += 1
        assert tried < 20000
    assert (k * (p - 1) + 1) % E == 0 and p >> 1022 == 3
    return p


def crt_exponent(p: int) -> int:
    return pow(E, -1, p - 1)


def exponent_shape(e: int):
    """(bit length, top window) as mont_pow reads the exponent."""
    bits = e.bit_length()
    return bits, e >> (4 * (((bits + 3) >> 2) - 1))


def build():
    sp = lambda k, label, lo=12, hi=16: short_exponent_prime(k, _start(f"short exponent {label}", lo, hi))
    keys = {
        "short_2_4": [sp(2, "k2"), sp(4, "k4")],
        "short_6_8": [sp(6, "k6"), sp(8, "k8")],
        "short_16_32": [sp(16, "k16"), sp(32, "k32")],
        "short_gap": [sp(64, "gap k64", 12, 13), sp(128, "gap k128", 15, 16)],
    }
    q = _start("short exponent full q") | 1
    while not usable(q):
        q += 2
    keys["short_3_full"] = [sp(3, "k3"), q]
    ks = {"short_2_4": (2, 4), "short_6_8": (6, 8), "short_16_32": (16, 32), "short_gap": (64, 128),
          "short_3_full": (3, None)}
    shapes = []
    for name, (p, q) in keys.items():
        n = p * q
        assert p != q and n.bit_length() == 2048 and p >> 1022 == 3 and q >> 1022 == 3, name
        assert (p - 1) % E and (q - 1) % E, name
        for prime, k in zip((p, q), ks[name]):
            if k is not None:
                assert crt_exponent(prime) * E == k * (prime - 1) + 1, name
            shapes.append(exponent_shape(crt_exponent(prime)))
    p, q = keys["short_gap"]
    assert p < q and 8 * (q - p) >= q
    bits = [b for b, _ in shapes]
    tops = [t for _, t in shapes]
    # (the whole signer key set -- these, the edge keys, the server keys -- is checked
    # again in tests/test_sign_edge_keys_cpu.py; these keys alone already cover it,
    # but for the 1024-bit exponent, which short_3_full's q supplies or a server key does)
    assert {b % 4 for b in bits} == {0, 1, 2, 3} and min(bits) <= 1010
    assert 1 in tops and max(tops) >= 8
    return keys


def main():
    keys = build()
    doc = {"comment": "TEST-ONLY RSA-2048 keys with short CRT exponents (make_sign_edge_keys.py); e = 65537",
           "e": E, "keys": {k: {"p": f"{p:x}", "q": f"{q:x}"} for k, (p, q) in keys.items()}}
    with open(os.path.join(HERE, "sign_edge_keys.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
