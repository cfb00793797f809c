"""Grant prep (prep_dev.h, sha256_dev.h) at every length and alignment, against the oracle.

sha256_block_words takes any alignment through a 4-or-5-load window and a per-lane
dword rotation picked by base & 15, pads per word, and grant_prep_fast decides "both
strings are ASCII" from a popcount over the SHA message words that must equal a
length-dependent count (the header's continuation bytes, the 0x80 pad byte, and bits
7, 15 and 23 of the bit length).  A wrong count in the accepting direction marks a
malformed grant PARSED and changes its certificate's verdict.

  sweep   a common-shape grant of every total length 6..330, 4094..4098, 8190..8194
          at each of the 16 alignments
  ASCII   one stray 0x80 / 0xFF byte (malformed) or one "é" (fine) in the objectId or
          the hash, in both classes of len mod 32 and on both sides of 4096 bytes

Both launch sequences: the small-batch one (k_grant_prep, every grant on its own) and
the large-batch one with three-grant certificates whose grants sit in key slots 0, 1, 2
-- k_grant_prep_cert's LDS store, its direct store and k_grant_prep_rare -- rotated so
that every grant takes every role.  (The sweep's small batches exceed the 1,024 grants
that k_bucket_small preps itself, so k_grant_prep runs; the ASCII set is small enough to
take that fused form.)
"""
import hashlib

import numpy as np
import pytest

import mochi_hip as mh
import oracle_ffi as O
import workload as W

pytestmark = pytest.mark.gpu

SIG_OK = 1
SMALL_MAX = 4096  # the small-batch sequence takes at most this many grants


@pytest.fixture(scope="module")
def pems():
    return W.load_keys(4)


@pytest.fixture(scope="module")
def ver(pems):
    v = mh.Verifier([mh.pem_modulus(p) for p in pems], 0)
    yield v
    v.close()


def _ascii(label: str, n: int) -> bytes:
    """n printable ASCII bytes, fixed by the label."""
    raw = hashlib.shake_128(label.encode()).digest(n)
    return bytes(0x21 + b % 94 for b in raw)


def fast_grant(total: int, oid_len: int = None) -> tuple:
    """(grant bytes, objectId slice, hash slice): 0x0A L objectId 0x10 ts 0x22 H hash of
    exactly `total` >= 6 bytes, L < 128, a timestamp of 1..3 varint bytes, ASCII strings."""
    ts = 5 if total < 12 else (1000, 70000, 5)[total % 3]
    tsb = W._varint(ts)
    rest = total - (2 + 1 + len(tsb) + 1)  # L + the hash length's bytes + the hash
    assert rest >= 1
    L = min((total * 7) % 128 if oid_len is None else oid_len, rest - 1)
    if rest - L == 129:  # no hash fills 129 bytes with its length: 1 + 127, 2 + 128
        L += 1 if L < 127 else -1
    hl = rest - L - 1 if rest - L - 1 < 128 else rest - L - 2
    oid, th = _ascii(f"oid {total}", L), _ascii(f"hash {total}", hl)
    g = b"\x0a" + bytes([L]) + oid + b"\x10" + tsb + b"\x22" + W._varint(hl) + th
    assert len(g) == total and 0 <= L < 128
    o0 = 2
    h0 = total - hl
    assert g[o0:o0 + L] == oid and g[h0:] == th
    return g, (o0, L), (h0, hl)


class Grants:
    """Distinct grant byte strings, each placed in one blob at chosen alignments and signed
    by OpenSSL (signer = entry index mod 4)."""

    def __init__(self, pems, items):
        """items: [(grant bytes, alignment mod 16)]"""
        blob, off = bytearray(b"\x07"), []
        for gb, al in items:
            blob += b"\xee" * ((al - len(blob)) % 16)
            off.append(len(blob))
            blob += gb
        blob += b"\xee" * 16
        self.n = len(items)
        self.blob = np.frombuffer(bytes(blob), np.uint8).copy()
        self.off = np.array(off, np.uint64)
        self.len = np.array([len(gb) for gb, _ in items], np.uint32)
        self.signer = (np.arange(self.n) % 4).astype(np.uint16)
        self.sig = np.zeros((self.n, 256), np.uint8)
        for k in range(4):
            idx = np.nonzero(self.signer == k)[0]
            self.sig[idx] = mh.sign_grants(pems[k], self.blob, self.off[idx], self.len[idx], 8)

    def batch(self, certs, slots):
        """certs: [[entry index, ...]]; the j-th grant of a certificate sits in key slot
        slots[j], and one op names each slot."""
        idx = np.array([i for c in certs for i in c], np.int64)
        C, k = len(certs), len(slots)
        assert all(len(c) == k for c in certs)
        return mh.Batch(grant_bytes=self.blob, grant_off=self.off[idx], grant_len=self.len[idx], sig=self.sig[idx],
                        signer=self.signer[idx], grant_key=np.tile(np.array(slots, np.uint8), C),
                        cert_grant_off=(np.arange(C + 1) * k).astype(np.uint32),
                        cert_op_off=(np.arange(C + 1) * k).astype(np.uint32),
                        op_key=np.tile(np.arange(k, dtype=np.uint8), C), op_flags=np.full(C * k, 3, np.uint8),
                        expected_hash=np.zeros((C, 128), np.uint8)), idx


def assert_same(g, o, what):
    for k in ("grant_flags", "grant_ts", "grant_valid_bits", "cert_accept_bits", "cert_reason", "cert_fail_op"):
        a, b = getattr(g, k), getattr(o, k)
        if k in ("grant_flags", "grant_ts") and not np.array_equal(a, b):
            bad = np.nonzero(a != b)[0]
            raise AssertionError(f"{k} {what}: grants {bad[:16].tolist()} got {a[bad[:16]].tolist()} "
                                 f"want {b[bad[:16]].tolist()}")
        np.testing.assert_array_equal(a, b, err_msg=f"{k} {what}")


def run_both_sequences(ver, moduli, G: Grants, check):
    """Every grant through k_grant_prep (small-batch sequence, one-grant certificates) and
    through each role of the large-batch sequence; check(what, entry indices, gpu
    verdicts, certificates) runs on every result after the comparison with the oracle."""
    try:
        ver.set_small_batch(SMALL_MAX)
        for lo in range(0, G.n, 2680):  # above the fused-prep bound, within the small-batch bound
            certs = [[i] for i in range(lo, min(lo + 2680, G.n))]
            b, idx = G.batch(certs, (0,))
            assert b.grant_off.shape[0] <= SMALL_MAX
            g = ver.verify(b, 4, False)
            assert_same(g, O.verify_batch(moduli, b, 4, False, 8), f"small [{lo}..]")
            check(f"small [{lo}..]", idx, g, certs)
        ver.set_small_batch(0)
        order = list(range(G.n)) + list(range((-G.n) % 3))  # a whole number of certificates
        for rot in range(3):
            certs = [[order[c + (j + rot) % 3] for j in range(3)] for c in range(0, len(order), 3)]
            b, idx = G.batch(certs, (0, 1, 2))
            g = ver.verify(b, 4, False)
            assert_same(g, O.verify_batch(moduli, b, 4, False, 8), f"large, rotation {rot}")
            check(f"large, rotation {rot}", idx, g, certs)
    finally:
        ver.set_small_batch(SMALL_MAX)


SWEEP_LENGTHS = list(range(6, 331)) + list(range(4094, 4099)) + list(range(8190, 8195))


def test_fast_shape_grants_at_every_length_and_alignment(ver, pems):
    items = [(fast_grant(total)[0], al) for total in SWEEP_LENGTHS for al in range(16)]
    G = Grants(pems, items)
    assert G.n == 16 * len(SWEEP_LENGTHS) and {int(x) for x in G.off % 16} == set(range(16))
    assert {t % 64 for t in SWEEP_LENGTHS} == set(range(64))
    assert all(fast_grant(t)[2][1] >= 128 for t in SWEEP_LENGTHS[-10:])  # a two-byte hash length
    moduli = [mh.pem_modulus(p) for p in pems]
    want_ts = np.array([(5 if t < 12 else (1000, 70000, 5)[t % 3]) for t in SWEEP_LENGTHS for _ in range(16)], np.int64)

    def check(what, idx, g, certs):
        assert (g.grant_flags & SIG_OK).all(), what
        long_enough = G.len[idx] >= 8  # grant_prep_fast's own bound; 6 and 7: the oracle's verdict
        assert (g.grant_flags[long_enough] & mh.GRANT_PARSED).all(), what
        np.testing.assert_array_equal(g.grant_ts[long_enough], want_ts[idx][long_enough], err_msg=what)
        assert not (g.cert_reason == mh.REJECT_MALFORMED)[[all(G.len[i] >= 8 for i in c) for c in certs]].any(), what

    run_both_sequences(ver, moduli, G, check)


def _utf8_ok(gb: bytes, oid, th) -> bool:
    try:
        gb[oid[0]:oid[0] + oid[1]].decode("utf-8")
        gb[th[0]:th[0] + th[1]].decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


# len mod 32 in [0, 16) and in [16, 32) (bit 7 of the bit length), below and above 4096 bytes (bit 15)
ASCII_LENGTHS = (168, 184, 4296, 4312)


def test_ascii_count_rejects_one_stray_byte(ver, pems):
    assert [(t % 32 >= 16, t >= 4096) for t in ASCII_LENGTHS] == [(False, False), (True, False), (False, True),
                                                                    (True, True)]
    items, want = [], []
    for total in ASCII_LENGTHS:
        base, oid, th = fast_grant(total, oid_len=21)
        assert oid[1] == 21 and th[1] >= 100 and _utf8_ok(base, oid, th)
        mid = th[0] + th[1] // 2
        # (position, whether a two-byte sequence goes before it instead of after it)
        spots = [(oid[0], False), (oid[0] + oid[1] - 1, True), (th[0], False), (total - 1, True)]
        spots += [(mid + k, False) for k in range(4)]
        variants = [(base, True)]
        for pos, before in spots:
            for stray in (b"\x80", b"\xff"):
                variants.append((base[:pos] + stray + base[pos + 1:], False))
            at = pos - 1 if before else pos
            variants.append((base[:at] + "é".encode() + base[at + 2:], True))
        assert len({v for v, _ in variants}) == 1 + 3 * len(spots)
        for gb, ok in variants:
            assert len(gb) == total and _utf8_ok(gb, oid, th) == ok
            assert (O.grant_parse(gb) is not None) == ok  # the oracle's parse agrees with Python's decoder
            for al in range(4):
                items.append((gb, al))
                want.append(ok)
    want = np.array(want)
    G = Grants(pems, items)
    assert G.n == len(ASCII_LENGTHS) * 25 * 4 and (~want).sum() == len(ASCII_LENGTHS) * 16 * 4
    moduli = [mh.pem_modulus(p) for p in pems]

    def check(what, idx, g, certs):
        assert (g.grant_flags & SIG_OK).all(), what
        parsed = (g.grant_flags & mh.GRANT_PARSED) != 0
        bad = np.nonzero(parsed != want[idx])[0]
        assert bad.size == 0, (what, "entries with the wrong PARSED flag", idx[bad[:16]].tolist())
        malformed = np.array([not all(want[i] for i in c) for c in certs])
        np.testing.assert_array_equal(g.cert_reason == mh.REJECT_MALFORMED, malformed, err_msg=what)

    run_both_sequences(ver, moduli, G, check)
