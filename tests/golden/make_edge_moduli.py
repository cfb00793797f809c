#!/usr/bin/env python3
"""Generate tests/golden/edge_moduli.json: five constructed RSA-2048 test keys whose
moduli sit at the edges of the RSA kernels' limb arithmetic (tests/rsa_edge_vectors.py).

    python tests/golden/make_edge_moduli.py

Pure Python, a few seconds.  Primality: Miller-Rabin over the fixed bases below (the
first 40 primes), so the output is the same on every run; every prime p has
gcd(65537, p - 1) = 1, so e = 65537 has an inverse.  TEST-ONLY keys: the factors
are committed.

  top_ones            the two largest primes below 2^1024: the top ~1000 bits of n are ones
  above_2_2047        the two smallest primes >= ceil(sqrt(2^2047)): n = 2^2047 + small,
                      a long run of zeros under the top bit
  sparse              nextprime(2^1023) * nextprime(2^1024): almost every limb of n is zero,
                      the fold digits of 2^k mod n are extreme
  low_limb_one        p == q == 1 (mod 2^28): n == 1, so -n^-1 mod 2^28 = 2^28 - 1
  low_limb_minus_one  p == 1, q == -1 (mod 2^28): n == -1, so -n^-1 mod 2^28 = 1
"""
from __future__ import annotations

import hashlib
import json
import math
import os

HERE = os.path.dirname(os.path.abspath(__file__))
E = 65537
B28 = 1 << 28


def _small_primes(limit):
    sieve = bytearray([1]) * limit
    sieve[0:2] = b"\x00\x00"
    for i in range(2, int(limit ** 0.5) + 1):
        if sieve[i]:
            sieve[i * i::i] = bytearray(len(sieve[i * i::i]))
    return [i for i in range(limit) if sieve[i]]


SMALL = _small_primes(4000)
BASES = SMALL[:40]


def is_prime(n: int) -> bool:
    if n < 2:
        return False
    for p in SMALL:
        if n % p == 0:
            return n == p
    d, r = n - 1, 0
    while d % 2 == 0:
        d //= 2
        r += 1
    for a in BASES:
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(r - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def usable(p: int) -> bool:
    return (p - 1) % E != 0 and is_prime(p)


def search(start: int, step: int, count: int = 1):
    """The first `count` usable primes start, start + step, start + 2 step, ..."""
    out, p = [], start
    while len(out) < count:
        if usable(p):
            out.append(p)
        p += step
    return out


def _seeded(label: str) -> int:
    """A fixed 1024-bit starting point with its two top bits set (so p * q has 2048 bits)."""
    raw = b"".join(hashlib.sha256(f"mochi edge modulus {label} {i}".encode()).digest() for i in range(4))
    return int.from_bytes(raw, "big") | (3 << 1022)


def build():
    keys = {}
    keys["top_ones"] = search((1 << 1024) - 1, -2, 2)
    root = math.isqrt(1 << 2047)
    root += root * root < (1 << 2047)  # ceil(sqrt(2^2047))
    keys["above_2_2047"] = search(root | 1, 2, 2)
    keys["sparse"] = search((1 << 1023) + 1, 2) + search((1 << 1024) + 1, 2)
    one = lambda label: search((_seeded(label) & ~(B28 - 1)) + 1, B28)[0]
    minus_one = lambda label: search((_seeded(label) | (B28 - 1)), B28)[0]
    keys["low_limb_one"] = [one("one p"), one("one q")]
    keys["low_limb_minus_one"] = [one("minus one p"), minus_one("minus one q")]
    for name, (p, q) in keys.items():
        n = p * q
        assert p != q and n % 2 == 1 and n.bit_length() == 2048, name
        assert math.gcd(E, (p - 1) * (q - 1)) == 1, name
    n0inv = lambda n: (-pow(n, -1, B28)) % B28
    assert n0inv(math.prod(keys["low_limb_one"])) == B28 - 1
    assert n0inv(math.prod(keys["low_limb_minus_one"])) == 1
    assert math.prod(keys["above_2_2047"]) >> 1040 == 1 << (2047 - 1040)
    assert (math.prod(keys["top_ones"]) >> 1048) == (1 << 1000) - 1
    return keys


def main():
    keys = build()
    doc = {"comment": "TEST-ONLY RSA-2048 keys with constructed moduli (make_edge_moduli.py); e = 65537",
           "e": E, "keys": {k: {"p": f"{p:x}", "q": f"{q:x}"} for k, (p, q) in keys.items()}}
    with open(os.path.join(HERE, "edge_moduli.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
