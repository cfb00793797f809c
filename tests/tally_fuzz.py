"""Seeded, stratified certificate generator for the tally fuzz tests.

The verdict logic (k_tally and the grant dedup kernels around it) restates
InMemoryDataStore.java:576-640; the committed fixtures reach it only with at
most two operations per certificate.  make() builds a batch whose certificates
have up to MOCHI_MAX_OPS_PER_CERT operations, repeated and shuffled key slots,
unequal sizes, repeated / unknown signers and every grant fault the tally
distinguishes, together with the ground truth BY CONSTRUCTION of every grant's
flags and timestamp, so that oracle_tally can judge it without re-verifying a
signature per parameter set.

Conventions: key slot s has objectId FZ_<s> and timestamp 1000 + 7*s in every
certificate, and every certificate expects the same "good" hash, so the set of
distinct (grant bytes, signer) pairs -- each signed once with the committed test
keys, through a cache -- stays in the hundreds.  A "bad" signature is the valid
one with one bit flipped.  Signer R lies outside the key table.

Two strata, independent of each other; every random decision has its own draw:
  small  0..5 ops over slots from a random base, multiplicity up to 3, shuffled;
         a random number of MultiGrants with random faults per (MultiGrant, slot)
  deep   31..64 ops, enumerated shapes (deep_shapes), R honest MultiGrants and
         exactly one planted fault at op index J (the first op naming its slot)
"""
from __future__ import annotations

import hashlib
from dataclasses import dataclass, field, replace
from typing import Dict, List, Optional, Tuple

import numpy as np

import mochi_hip as mh
import oracle_ffi as O
import workload as W

GOOD = hashlib.sha512(b"tally-fuzz").hexdigest()
EVIL = hashlib.sha512(b"tally-fuzz-evil").hexdigest()
HASHES = {"good": GOOD, "evil": EVIL, "short": GOOD[:127]}
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1

SMALL_OP_FLAGS = (3, 7, 0, 2, 1, 15, 11, 19, 23)
_SMALL_OP_P = (0.35, 0.30, 0.10) + (0.25 / 6,) * 6
UNNAMED_SLOTS = (63, 64, 200, 255)

DEEP_OPS = (31, 32, 33, 48, 63, 64)
DEEP_DISTINCT = ("k", "k-1", "k/2")
DEEP_FAULTS = ("none", "drop_all", "drop_but_two", "evil_first", "bad_then_evil", "ts_last", "flag1", "flag15",
               "flag19")
_DEEP_STEP = 5  # every 5th shape of the enumeration (coprime to its length)


def slot_ts(s: int) -> int:
    return 1000 + 7 * s


def slot_key(s: int) -> str:
    return f"FZ_{s}"


@dataclass(frozen=True)
class Grant:
    slot: int
    skew: int = 0           # added to the slot's timestamp
    hash: str = "good"      # good | evil | short (127 characters)
    foreign: bool = False   # objectId FZ_<s>x: another object (MOCHI_Q_BIND)
    malformed: bool = False  # trailing 0x0f (wire type 7)
    badsig: bool = False

    def encode(self) -> bytes:
        return _grant_bytes(self.slot, self.skew, self.hash, self.foreign, self.malformed)

    @property
    def object_id(self) -> str:
        return slot_key(self.slot) + ("x" if self.foreign else "")


@dataclass
class Cert:
    kind: str
    mgs: List[Tuple[int, List[Grant]]]      # (signer, grants) in wire order
    ops: List[Tuple[int, int, int]]         # (key slot, op flags, stored currentC timestamp)
    fault_op: int = -1                      # deep: the op index the fault is planted at

    @property
    def n_grants(self) -> int:
        return sum(len(g) for _, g in self.mgs)


_bytes_cache: Dict[tuple, bytes] = {}
_sig_cache: Dict[Tuple[bytes, int], bytes] = {}


def _grant_bytes(slot, skew, hname, foreign, malformed) -> bytes:
    k = (slot, skew, hname, foreign, malformed)
    b = _bytes_cache.get(k)
    if b is None:
        b = W.encode_grant(slot_key(slot) + ("x" if foreign else ""), slot_ts(slot) + skew, HASHES[hname])
        if malformed:
            b += b"\x0f"
        _bytes_cache[k] = b
    return b


def n_signed() -> int:
    """Distinct (grant bytes, signer) pairs signed so far."""
    return len(_sig_cache)


def signature(pems: List[bytes], gb: bytes, signer: int, bad: bool) -> bytes:
    """The signer's SHA256withRSA signature of gb (signed once per distinct pair).  A signer
    outside the key table gets key 0's: valid bytes under an index that names no key."""
    key = signer if signer < len(pems) else 0
    s = _sig_cache.get((gb, key))
    if s is None:
        s = _sig_cache[(gb, key)] = O.rsa_sign(pems[key], gb)
    if bad:
        s = s[:100] + bytes([s[100] ^ 0x10]) + s[101:]
    return s


# ---------------------------------------------------------------------------
# small certificates
# ---------------------------------------------------------------------------
def small_cert(rng: np.random.Generator, R: int) -> Cert:
    k = int(rng.integers(0, 6))
    base = int(rng.integers(0, 64))
    op_slots: List[int] = []
    i = 0
    while len(op_slots) < k:
        m = min(int(rng.choice((1, 2, 3), p=(0.6, 0.25, 0.15))), k - len(op_slots))
        op_slots += [(base + i) % 64] * m
        i += 1
    rng.shuffle(op_slots)
    slots = sorted(set(op_slots), key=op_slots.index)
    # how faulty the certificate is: every per-grant rate below is scaled by it
    level = float(rng.choice((0.0, 0.3, 1.0), p=(0.3, 0.45, 0.25)))
    n_mg = R if rng.random() < 0.7 else int(rng.integers(0, R + 3))
    extra: Optional[int] = None
    if rng.random() < 0.15:
        x = int(rng.choice(UNNAMED_SLOTS + ((base + 23) % 64,)))
        extra = None if x in slots else x
    mgs = []
    for m in range(n_mg):
        signer = m % R if rng.random() < 0.8 else int(rng.integers(0, R + 1))
        grants: List[Grant] = []
        for s in slots:
            # one draw per decision, drawn whether or not an earlier one already decided
            d = rng.random(8)
            if d[0] < 0.07 * level:
                continue  # missing
            g = Grant(slot=s, skew=int(d[1] < 0.05 * level),
                      hash="evil" if d[2] < 0.05 * level else "short" if d[2] < 0.08 * level else "good",
                      foreign=bool(d[3] < 0.05 * level), malformed=bool(d[4] < 0.015 * level),
                      badsig=bool(d[5] < 0.07 * level))
            grants.append(g)
            if d[6] < 0.05 * level:  # duplicated (its signature quality drawn again)
                grants.append(replace(g, badsig=bool(d[7] < 0.07 * level)))
        if extra is not None and rng.random() < 0.5:
            grants.insert(int(rng.integers(0, len(grants) + 1)), Grant(slot=extra))
        mgs.append((signer, grants))
    ops = []
    for s in op_slots:
        fl = int(rng.choice(SMALL_OP_FLAGS, p=_SMALL_OP_P))
        t = slot_ts(s)
        ots = (t - 1, t, t + 1, 0, I64_MIN, I64_MAX)[int(rng.choice(6, p=(0.25, 0.2, 0.25, 0.1, 0.1, 0.1)))]
        ops.append((s, fl, ots))
    return Cert("small", mgs, ops)


# ---------------------------------------------------------------------------
# deep certificates
# ---------------------------------------------------------------------------
def deep_shapes() -> List[Tuple[int, int, str, str]]:
    """(ops k, fault op J, distinct-slot rule, fault), enumerated: J in {0, 31, 32, k-1}."""
    out = []
    for k in DEEP_OPS:
        for J in sorted({j for j in (0, 31, 32, k - 1) if j < k}):
            for dm in DEEP_DISTINCT:
                for f in DEEP_FAULTS:
                    out.append((k, J, dm, f))
    return out


def n_distinct(k: int, rule: str) -> int:
    return {"k": k, "k-1": k - 1, "k/2": k // 2}[rule]


def deep_cert(rng: np.random.Generator, R: int, k: int, J: int, d: int, fault: str) -> Cert:
    """k ops over d distinct slots, R honest MultiGrants, `fault` planted at op J, which is the
    first op naming its slot.  The other ops apply, read or are WRONG_SHARD; none fails."""
    assert 1 <= d <= min(k, 64) and 0 <= J < k
    if d == 1:
        J = 0
    slot_ids = [int(x) for x in rng.permutation(64)[:d]]
    # the ops that name a new slot: 0, J and d - 2 more
    firsts = {0, J}
    others = [j for j in range(1, k) if j != J]
    if d > len(firsts):
        firsts |= set(int(x) for x in rng.choice(others, d - len(firsts), replace=False))
    op_slots, order = [], []
    for j in range(k):
        if j in firsts:
            order.append(slot_ids[len(order)])
            op_slots.append(order[-1])
        else:
            # a repeat: any earlier slot, or (half of them) one of the last eight, so that the
            # earlier apply that decides it (applied_before) often sits at an op index >= 32 too
            recent = rng.random() < 0.5
            lo = max(0, len(order) - 8) if recent else 0
            op_slots.append(order[int(rng.integers(lo, len(order)))])
    sJ = op_slots[J]
    keep_two = set(int(x) for x in rng.choice(R, 2, replace=False))
    mgs = []
    for m in range(R):
        grants = []
        for s in order:
            g = Grant(slot=s)
            if s == sJ:
                if fault == "drop_all" or (fault == "drop_but_two" and m not in keep_two):
                    continue
                if fault == "evil_first" and m == 0:
                    g = replace(g, hash="evil")
                if fault == "bad_then_evil" and m == 0:
                    g = replace(g, badsig=True)
                if fault == "bad_then_evil" and m == 1:
                    g = replace(g, hash="evil")
                if fault == "ts_last" and m == R - 1:
                    g = replace(g, skew=1)
            grants.append(g)
        mgs.append((m, grants))
    ops = []
    for j, s in enumerate(op_slots):
        t = slot_ts(s)
        # a repeat reads the stored certificate more often: after an apply to its slot that
        # certificate is the incoming one (not op_object_ts), and the op applies instead
        p = (0.4, 0.2, 0.2, 0.2) if j in firsts else (0.25, 0.45, 0.15, 0.15)
        fl, ots = ((3, 0), (7, t + 1), (7, t - 1), (0, 0))[int(rng.choice(4, p=p))]
        if j == J and fault != "none":
            fl, ots = {"flag1": 1, "flag15": 15, "flag19": 19}.get(fault, 3), t
        ops.append((s, fl, ots))
    return Cert(f"deep:{fault}:k{k}:J{J}:d{d}", mgs, ops, fault_op=J if fault != "none" else -1)


# ---------------------------------------------------------------------------
# assembly
# ---------------------------------------------------------------------------
@dataclass
class Fuzz:
    R: int
    seed: int
    batch: mh.Batch
    grant_flags: np.ndarray  # [N] MOCHI_GRANT_* by construction
    grant_ts: np.ndarray     # [N] by construction
    kind: List[str]          # per certificate
    certs: List[Cert] = field(repr=False, default_factory=list)

    @property
    def moduli(self) -> List[bytes]:
        return [O.pem_modulus(p) for p in W.load_keys(self.R)]


def assemble(certs: List[Cert], R: int, rng: np.random.Generator) -> Tuple[mh.Batch, np.ndarray, np.ndarray]:
    """Certificates -> Batch with every optional array set, every grant its own copy of its
    bytes after 0..3 filler bytes, each certificate's op keys after its grants; plus the
    flags and timestamps by construction."""
    pems = W.load_keys(R)
    blob = bytearray()
    goff, glen, sigs, signer, gkey, flags, ts = [], [], [], [], [], [], []
    cgo, coo, cmo, mgo = [0], [0], [0], [0]
    opk, opf, ots, okoff, oklen = [], [], [], [], []
    for c in certs:
        for sg, grants in c.mgs:
            for g in grants:
                gb = g.encode()
                blob += b"\xee" * int(rng.integers(0, 4))
                goff.append(len(blob))
                glen.append(len(gb))
                blob += gb
                sigs.append(signature(pems, gb, sg, g.badsig))
                signer.append(sg)
                gkey.append(g.slot)
                flags.append((0 if g.malformed else mh.GRANT_PARSED) |
                             (0 if g.badsig or sg >= R else mh.GRANT_SIG_OK))
                ts.append(0 if g.malformed else slot_ts(g.slot) + g.skew)
            mgo.append(len(goff))
        cmo.append(len(mgo) - 1)
        cgo.append(len(goff))
        for s, fl, t in c.ops:
            kb = slot_key(s).encode()
            okoff.append(len(blob))
            oklen.append(len(kb))
            blob += kb
            opk.append(s)
            opf.append(fl)
            ots.append(t)
        coo.append(len(opk))
    C = len(certs)
    batch = mh.Batch(
        grant_bytes=np.frombuffer(bytes(blob) or b"\0", np.uint8).copy(),
        grant_off=np.asarray(goff, np.uint64), grant_len=np.asarray(glen, np.uint32),
        sig=np.frombuffer(b"".join(sigs), np.uint8).reshape(-1, 256).copy() if sigs else np.zeros((0, 256), np.uint8),
        signer=np.asarray(signer, np.uint16), grant_key=np.asarray(gkey, np.uint8),
        cert_grant_off=np.asarray(cgo, np.uint32), cert_op_off=np.asarray(coo, np.uint32),
        op_key=np.asarray(opk, np.uint8), op_flags=np.asarray(opf, np.uint8),
        expected_hash=np.tile(np.frombuffer(GOOD.encode(), np.uint8), (C, 1)),
        cert_mg_off=np.asarray(cmo, np.uint32), mg_grant_off=np.asarray(mgo, np.uint32),
        op_object_ts=np.asarray(ots, np.int64), op_key_off=np.asarray(okoff, np.uint64),
        op_key_len=np.asarray(oklen, np.uint32))
    return batch, np.asarray(flags, np.uint8), np.asarray(ts, np.int64)


def _spread(deep: List[Cert]) -> List[Cert]:
    """Deep certificates reordered so that any few leading ones hold every fault and both ends
    of the op range (the enumeration has the shapes below 33 ops first): round robin over the
    faults, each fault's certificates alternating largest / smallest (late fault op first),
    every other fault starting at the small end."""
    rounds = []
    for i, f in enumerate(DEEP_FAULTS):
        g = sorted((c for c in deep if c.kind.split(":")[1] == f), key=lambda c: (-len(c.ops), -c.fault_op))
        zig, big = [], i % 2 == 0
        while g:
            zig.append(g.pop(0 if big else -1))
            big = not big
        rounds.append(zig)
    return [g[r] for r in range(max(map(len, rounds))) for g in rounds if r < len(g)]


def make(R: int, seed: int, n_certs: int = 400) -> Fuzz:
    """n_certs certificates, a quarter of them deep.  Order: a stretch where every fourth
    certificate is deep (so a prefix of a few thousand grants holds both strata), then the
    remaining deep ones, largest first (32-certificate chunks of more than 4096 grants), then
    the remaining small ones (chunks far below)."""
    shapes = deep_shapes()
    n_deep = n_certs // 4
    deep = []
    for i in range(n_deep):
        k, J, dm, f = shapes[(i * _DEEP_STEP) % len(shapes)]
        deep.append(deep_cert(np.random.default_rng([seed, R, 1, i]), R, k, J, n_distinct(k, dm), f))
    small = [small_cert(np.random.default_rng([seed, R, 2, i]), R) for i in range(n_certs - n_deep)]
    n_inter = min(n_deep, 32, len(small) // 3)
    deep = _spread(deep)
    certs: List[Cert] = []
    for i in range(n_inter):
        certs += small[3 * i:3 * i + 3] + [deep[i]]
    certs += sorted(deep[n_inter:], key=lambda c: -c.n_grants)
    certs += small[3 * n_inter:]
    batch, flags, ts = assemble(certs, R, np.random.default_rng([seed, R, 3]))
    return Fuzz(R, seed, batch, flags, ts, [c.kind for c in certs], certs)


# ---------------------------------------------------------------------------
# views of a batch
# ---------------------------------------------------------------------------
def shared_copies(b: mh.Batch) -> mh.Batch:
    """The same batch with the byte-equal grants of a (certificate, slot) pointing at ONE
    copy, the first: the layout in which the dedup kernels match grants by equal offsets,
    where the separate copies of make() are matched by comparing bytes."""
    off = np.array(b.grant_off, np.uint64)
    blob = b.grant_bytes
    for c in range(b.n_certs):
        first: Dict[Tuple[int, bytes], int] = {}
        for g in range(int(b.cert_grant_off[c]), int(b.cert_grant_off[c + 1])):
            gb = blob[int(off[g]):int(off[g]) + int(b.grant_len[g])].tobytes()
            off[g] = first.setdefault((int(b.grant_key[g]), gb), int(off[g]))
    return replace(b, grant_off=off)


def without_csr(b: mh.Batch) -> mh.Batch:
    """cert_mg_off / mg_grant_off NULL: a MultiGrant is a maximal run of one signer."""
    return replace(b, cert_mg_off=None, mg_grant_off=None)


def head(b: mh.Batch, n: int) -> mh.Batch:
    """The first n certificates (blob shared)."""
    g, o = int(b.cert_grant_off[n]), int(b.cert_op_off[n])
    kw = dict(grant_off=b.grant_off[:g], grant_len=b.grant_len[:g], sig=b.sig[:g], signer=b.signer[:g],
              grant_key=b.grant_key[:g], cert_grant_off=b.cert_grant_off[:n + 1], cert_op_off=b.cert_op_off[:n + 1],
              op_key=b.op_key[:o], op_flags=b.op_flags[:o], expected_hash=b.expected_hash[:n],
              op_object_ts=b.op_object_ts[:o], op_key_off=b.op_key_off[:o], op_key_len=b.op_key_len[:o])
    if b.cert_mg_off is not None:
        m = int(b.cert_mg_off[n])
        kw.update(cert_mg_off=b.cert_mg_off[:n + 1], mg_grant_off=b.mg_grant_off[:m + 1])
    return replace(b, **kw)


def certs_within(b: mh.Batch, max_grants: int) -> int:
    """How many leading certificates hold at most max_grants grants together."""
    return int(np.searchsorted(np.asarray(b.cert_grant_off, np.int64), max_grants, side="right")) - 1


# ---------------------------------------------------------------------------
# Write2ToServer form of a certificate
# ---------------------------------------------------------------------------
def wire_message(cert: Cert, R: int) -> bytes:
    """The certificate as a Write2ToServer body: a MultiGrant per signer (map key =
    MultiGrant.serverId), grants and grantSignatures keyed by objectId, a WRITE operation
    per op with operand1 = its slot's key (ops of one slot repeat it)."""
    pems = W.load_keys(R)
    mgs = []
    for sg, grants in cert.mgs:
        sid = W.SERVER_IDS[sg]
        items = [(g.object_id, g.encode(), signature(pems, g.encode(), sg, g.badsig)) for g in grants]
        mgs.append((sid, W.encode_multigrant([(o, gb) for o, gb, _ in items], sid, sigs=[(o, s) for o, _, s in items])))
    ops = [W.encode_operation(2, slot_key(s), f"v{j}") for j, (s, _, _) in enumerate(cert.ops)]
    return W.encode_write2(mgs, ops)


def wire_batch(certs: List[Cert], R: int) -> W.WireBatch:
    msgs = [wire_message(c, R) for c in certs]
    off, parts, pos = [], [], 0
    for i, m in enumerate(msgs):
        parts.append(b"\xee" * (i % 4))
        pos += i % 4
        off.append(pos)
        parts.append(m)
        pos += len(m)
    ofo = np.zeros(len(certs) + 1, np.uint32)
    np.cumsum([len(c.ops) for c in certs], out=ofo[1:])
    return W.WireBatch(
        wire=np.frombuffer(b"".join(parts) or b"\0", np.uint8).copy(), msg_off=np.asarray(off, np.uint64),
        msg_len=np.asarray([len(m) for m in msgs], np.uint32), op_flags_off=ofo,
        op_flags=np.asarray([fl for c in certs for _, fl, _ in c.ops], np.uint8),
        expected_hash=np.tile(np.frombuffer(GOOD.encode(), np.uint8), (len(certs), 1)),
        op_object_ts=np.asarray([t for c in certs for _, _, t in c.ops], np.int64))
