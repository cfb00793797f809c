"""The yardstick for Write1 grant issuance (mochi_write1_issue[_device]): a short
sequential model of the server's Write1 path, one request at a time against a
dict store, restated from InMemoryDataStore.java:105-155 (processWrite) and
:233-310 (tryProcessWriteRegularly) with StoreValueObjectContainer.java:100-133
(the slot lookup).  Grant bytes come from the CPU oracle (oracle_ffi.grant_encode).

TEST INFRASTRUCTURE: the library is never its own reference here.

The contract the batch forms add to the reference (include/mochi_hip.h): the
caller creates the container of every local WRITE key BEFORE the batch
(prepare), where the reference creates it inside processWrite; the seed is
unsigned; an op behind an empty key is reported SKIPPED.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np

import mochi_hip as mh
import oracle_ffi as O

READ, DELETE, WRITE = 0, 1, 2  # OperationAction (MochiProtocol.proto:20-24)
MASK64 = (1 << 64) - 1


def wrap64(v: int) -> int:
    """Java long arithmetic."""
    v &= MASK64
    return v - (1 << 64) if v >> 63 else v


@dataclass
class StoredGrant:
    object_id: bytes
    ts: int
    txn_hash: bytes
    data: bytes  # Grant.toByteArray()
    ref: int = -1  # how this batch names it: a new-grant index or W1_STORED | stored index


@dataclass
class Container:
    epoch: int = 0
    grants: Dict[int, StoredGrant] = field(default_factory=dict)  # givenWrite1Grants, flattened over epochs

    def move_to_next_epoch_if_necessary(self, timestamp: int) -> None:
        q = abs(timestamp) // 1000  # Java long division truncates toward zero
        nxt = wrap64(((q if timestamp >= 0 else -q) + 1) * 1000)
        if self.epoch < nxt:
            self.epoch = nxt


@dataclass
class Store:
    is_local: Callable[[bytes], bool]
    data: Dict[bytes, Container] = field(default_factory=dict)

    def snapshot(self):
        return {k: (c.epoch, {ts: (g.txn_hash, g.data) for ts, g in c.grants.items()}) for k, c in self.data.items()}


@dataclass
class Request:
    seed: int
    txn_hash: bytes
    ops: List[Tuple[int, bytes]]  # (action, operand1)


def prepare(store: Store, reqs: List[Request]) -> None:
    """The caller's duty before a batch: getOrCreateStoreValue for every local WRITE key."""
    for r in reqs:
        for action, key in r.ops:
            if action == WRITE and key and store.is_local(key) and key not in store.data:
                store.data[key] = Container()


def run(store: Store, reqs: List[Request]) -> dict:
    """Process the requests one after another; the store keeps every new grant.
    Returns the arrays the library gives, with grants as a list of bytes."""
    op_decision, op_grant, req_kind, req_grant_off, req_grant = [], [], [], [0], []
    new: List[StoredGrant] = []
    grant_op: List[int] = []
    for g in (g for c in store.data.values() for g in c.grants.values()):
        assert g.ref & mh.W1_STORED, "stored grants are named by build_batch before the model runs"
    for r in reqs:
        granted: Dict[bytes, StoredGrant] = {}
        rejected: Dict[bytes, Optional[StoredGrant]] = {}
        threw = False
        for action, key in r.ops:
            o = len(op_decision)
            if action not in (WRITE, DELETE):
                op_decision.append(mh.W1D_SKIP)
                op_grant.append(mh.W1_NONE)
                continue
            if threw:
                op_decision.append(mh.W1D_SKIPPED)
                op_grant.append(mh.W1_NONE)
                continue
            # processWrite
            if not key:  # checkOp1IsNonEmptyKeyError
                threw = True
                op_decision.append(mh.W1D_FAILED)
                op_grant.append(mh.W1_NONE)
                continue
            if not store.is_local(key):
                g = granted.get(key)  # grants.put would replace it with an equal grant
                if g is None:
                    g = StoredGrant(key, 0, r.txn_hash, O.grant_encode(key, 0, r.txn_hash, 0, 1), ref=len(new))
                    new.append(g)
                    grant_op.append(o)
                granted[key] = g
                op_decision.append(mh.W1D_WRONG_SHARD)
                op_grant.append(g.ref)
                continue
            c = store.data.get(key)
            if c is None:  # the DELETE of an absent key: Triplet(null, null, false)
                rejected[key] = None
                op_decision.append(mh.W1D_FAILED)
                op_grant.append(mh.W1_NONE)
                continue
            ts = wrap64(c.epoch + r.seed)
            g = c.grants.get(ts)
            if g is None:
                g = StoredGrant(key, ts, r.txn_hash, O.grant_encode(key, ts, r.txn_hash), ref=len(new))
                new.append(g)
                grant_op.append(o)
                c.grants[ts] = g
                granted[key] = g
                op_decision.append(mh.W1D_NEW)
            elif g.txn_hash == r.txn_hash:
                granted[key] = g
                op_decision.append(mh.W1D_RETRY)
            else:
                rejected[key] = g
                op_decision.append(mh.W1D_REFUSED)
            op_grant.append(g.ref)
        if threw or any(g is None for g in rejected.values()):
            kind, view = mh.W1K_THROWS, []
        elif rejected:
            kind, view = mh.W1K_REFUSED, list(rejected.values())
        else:
            kind, view = mh.W1K_OK, list(granted.values())
        req_kind.append(kind)
        req_grant += [g.ref for g in view]
        req_grant_off.append(len(req_grant))
    return dict(op_decision=np.array(op_decision, np.uint8), op_grant=np.array(op_grant, np.uint32),
                req_kind=np.array(req_kind, np.uint8), req_grant_off=np.array(req_grant_off, np.uint32),
                req_grant=np.array(req_grant, np.uint32), grants=[g.data for g in new],
                grant_op=np.array(grant_op, np.uint32), grant_ts=np.array([g.ts for g in new], np.int64),
                new=new)


def build_batch(store: Store, reqs: List[Request], pad: Optional[Callable[[int], int]] = None) -> mh.Write1Batch:
    """The mochi_write1_batch a caller builds from its store (after prepare) for
    these requests.  Names every stored grant an op meets (StoredGrant.ref).
    pad(i) filler bytes go before the i-th string (alignment sets)."""
    blob = bytearray()
    n_str = [0]

    def put(s: bytes):
        blob.extend(b"\xee" * (pad(n_str[0]) if pad else 0))
        n_str[0] += 1
        off = len(blob)
        blob.extend(s)
        return off, len(s)

    obj_of: Dict[bytes, int] = {}
    stored: List[StoredGrant] = []
    for c in store.data.values():
        for g in c.grants.values():
            g.ref = -1
    req_op_off, seeds, rh = [0], [], []
    cols = dict(ko=[], kl=[], fl=[], obj=[], ep=[], st=[])
    for r in reqs:
        seeds.append(r.seed)
        rh.append(put(r.txn_hash))
        for action, key in r.ops:
            ko, kl = put(key)
            f = (mh.W1OP_WRITE if action == WRITE else 0) | (mh.W1OP_DELETE if action == DELETE else 0)
            obj, ep, st = 0, 0, mh.W1_NONE
            if key and store.is_local(key):
                f |= mh.W1OP_LOCAL
                c = store.data.get(key)
                if c is not None:
                    f |= mh.W1OP_HAS_SVOC
                    obj = obj_of.setdefault(key, len(obj_of))
                    ep = c.epoch
                    g = c.grants.get(wrap64(c.epoch + r.seed))
                    if g is not None:
                        if g.ref < 0:
                            g.ref = mh.W1_STORED | len(stored)
                            stored.append(g)
                        st = g.ref & ~mh.W1_STORED
            for k, v in zip(("ko", "kl", "fl", "obj", "ep", "st"), (ko, kl, f, obj, ep, st)):
                cols[k].append(v)
        req_op_off.append(len(cols["fl"]))
    sh = [put(g.txn_hash) for g in stored]
    # grants no op met still need a name for the model's bookkeeping
    n = len(stored)
    for c in store.data.values():
        for g in c.grants.values():
            if g.ref < 0:
                g.ref = mh.W1_STORED | n
                n += 1
    return mh.Write1Batch(
        strings=np.frombuffer(bytes(blob) or b"\x00", np.uint8).copy(),
        req_op_off=np.array(req_op_off, np.uint32), req_seed=np.array(seeds, np.uint32),
        req_hash_off=np.array([x[0] for x in rh], np.uint64), req_hash_len=np.array([x[1] for x in rh], np.uint32),
        op_key_off=np.array(cols["ko"], np.uint64), op_key_len=np.array(cols["kl"], np.uint32),
        op_flags=np.array(cols["fl"], np.uint8), op_obj=np.array(cols["obj"], np.uint32),
        op_epoch=np.array(cols["ep"], np.int64), op_stored=np.array(cols["st"], np.uint32),
        stored_hash_off=np.array([x[0] for x in sh], np.uint64), stored_hash_len=np.array([x[1] for x in sh], np.uint32))


def apply_outputs(store: Store, reqs: List[Request], batch: mh.Write1Batch, out: "mh.Write1Issued") -> None:
    """What the host does after a batch: store EVERY new local grant, whatever its request's kind."""
    keys = [key for r in reqs for _, key in r.ops]
    req_of = np.repeat(np.arange(len(reqs)), np.diff(batch.req_op_off.astype(np.int64)))
    for g in range(out.n_new):
        o = int(out.grant_op[g])
        if out.op_decision[o] != mh.W1D_NEW:
            continue  # a WRONG_SHARD grant is not this server's to keep
        r = reqs[int(req_of[o])]
        ts = int(out.grant_ts[g])
        store.data[keys[o]].grants[ts] = StoredGrant(keys[o], ts, r.txn_hash, out.grant(g))


def assert_matches(out: "mh.Write1Issued", want: dict) -> None:
    """Library outputs == the model's, array for array, byte for byte."""
    assert out.rc == mh.OK
    for k in ("op_decision", "op_grant", "req_kind", "req_grant_off", "req_grant", "grant_op", "grant_ts"):
        np.testing.assert_array_equal(getattr(out, k), want[k], err_msg=k)
    assert out.n_new == len(want["grants"])
    got = [out.grant(g) for g in range(out.n_new)]
    assert got == want["grants"]
    # packed back to back in index order
    ln = np.array([len(x) for x in want["grants"]], np.int64)
    np.testing.assert_array_equal(out.grant_len, ln)
    np.testing.assert_array_equal(out.grant_off, np.concatenate([[0], np.cumsum(ln)[:-1]]) if len(ln) else ln)
    assert out.grant_bytes_len == int(ln.sum())


def copy_store(store: Store) -> Store:
    s = Store(store.is_local)
    for k, c in store.data.items():
        s.data[k] = Container(c.epoch, {ts: StoredGrant(g.object_id, g.ts, g.txn_hash, g.data, g.ref)
                                        for ts, g in c.grants.items()})
    return s


# ---------------------------------------------------------------------------
# Case sets shared by the CPU tests (host form vs model) and the GPU tests
# (device form vs host form).  Each case: (store before prepare, requests, pad).
# ---------------------------------------------------------------------------
def is_local(key: bytes) -> bool:
    return not key.startswith(b"far")


def H(i: int, n: int = 128) -> bytes:
    """A transactionHash stand-in of n ASCII bytes."""
    import hashlib

    return (hashlib.sha512(f"w1-txn-{i}".encode()).hexdigest() * 2).encode()[:n]


def _store(epochs: Dict[bytes, int], grants=()) -> Store:
    s = Store(is_local)
    for k, e in epochs.items():
        s.data[k] = Container(e)
    for key, seed, h in grants:  # a grant given in an earlier batch
        ts = wrap64(s.data[key].epoch + seed)
        s.data[key].grants[ts] = StoredGrant(key, ts, h, O.grant_encode(key, ts, h))
    return s


def hand_cases() -> dict:
    R = Request
    c = {}
    # a winner whose own request is REFUSED; later requests meet its new grant
    c["winner_refused"] = (_store({b"a": 1000, b"b": 2000}, [(b"a", 5, H(9))]),
                           [R(5, H(1), [(WRITE, b"b"), (WRITE, b"a")]), R(5, H(2), [(WRITE, b"b")]),
                            R(5, H(1), [(DELETE, b"b")])])
    # a winner whose request THROWS (DELETE of an absent key); its other ops are still processed
    c["winner_throws"] = (_store({}), [R(3, H(1), [(WRITE, b"c"), (DELETE, b"absent"), (WRITE, b"c2")]),
                                       R(3, H(2), [(WRITE, b"c")]), R(3, H(3), [(WRITE, b"c2")])])
    # an empty key mid-request: later ops SKIPPED, a later request wins the slot they would have claimed
    c["empty_mid"] = (_store({b"f": 0}), [R(7, H(1), [(WRITE, b"d"), (WRITE, b""), (WRITE, b"e"), (DELETE, b"f"),
                                                      (READ, b"e"), (WRITE, b"far-x")]),
                                          R(7, H(2), [(WRITE, b"e"), (DELETE, b"f")]),
                                          R(7, H(1), [(DELETE, b""), (WRITE, b"d")])])
    c["delete_absent"] = (_store({b"here": 4000}), [R(1, H(1), [(DELETE, b"gone")]), R(1, H(2), [(DELETE, b"here")]),
                                                   R(1, H(3), [(DELETE, b"gone"), (DELETE, b"here")])])
    c["same_key_twice"] = (_store({}), [R(2, H(1), [(WRITE, b"g"), (WRITE, b"g"), (DELETE, b"g")]),
                                        R(2, H(1), [(WRITE, b"far1"), (DELETE, b"far1"), (WRITE, b"far2"), (WRITE, b"far1")]),
                                        R(2, H(2), [(WRITE, b"far1"), (WRITE, b"g"), (WRITE, b"g")]),
                                        R(9, H(2), [(WRITE, b"far1"), (WRITE, b"far10")])])
    c["read_between"] = (_store({}), [R(4, H(1), [(WRITE, b"h"), (READ, b"h"), (WRITE, b"i"), (READ, b"")]),
                                      R(4, H(1), [(READ, b"h")]), R(4, H(2), []), R(4, H(2), [(WRITE, b"i")])])
    c["stored"] = (_store({b"s": 3000, b"t": 3000}, [(b"s", 1, H(1)), (b"t", 1, H(2)), (b"t", 2, H(3))]),
                   [R(1, H(1), [(WRITE, b"s")]), R(1, H(1), [(WRITE, b"s"), (WRITE, b"t")]), R(2, H(3), [(DELETE, b"t"), (WRITE, b"t")]),
                    R(2, H(4), [(WRITE, b"s"), (WRITE, b"t")]), R(1, H(2), [(WRITE, b"t"), (WRITE, b"s")])])
    c["empty_batch"] = (_store({}), [])
    c["no_ops"] = (_store({}), [R(1, H(1), []), R(2, H(2), [])])
    return c


def edge_cases() -> dict:
    R = Request
    c = {}
    keys = [b"k", b"K" * 127, b"L" * 128]
    c["key_len"] = (_store({}), [R(1, H(i), [(WRITE, k), (WRITE, b"far" + k)]) for i, k in enumerate(keys)])
    c["hash_len"] = (_store({}), [R(i, H(i, n), [(WRITE, b"hl"), (WRITE, b"far-hl")]) for i, n in enumerate((0, 1, 127, 128, 129))] +
                     [R(0, b"", [(WRITE, b"hl")]), R(1, H(1, 1), [(WRITE, b"hl")])])  # empty vs empty is a RETRY
    ts_vals = [0, 127, 128, 16383, 16384, 1 << 31, (1 << 63) - 1]
    c["ts_steps"] = (_store({b"ts%d" % i: t for i, t in enumerate(ts_vals)}),
                     [R(0, H(i), [(WRITE, b"ts%d" % i)]) for i in range(len(ts_vals))])
    c["ts_from_seed"] = (_store({b"z": 0}), [R(s, H(s % 97), [(WRITE, b"z")]) for s in (0, 127, 128, 16383, 16384, 1 << 31, (1 << 32) - 1)])
    c["negative_epoch"] = (_store({b"n": -5000, b"m": -1, b"w": (1 << 63) - 1, b"v": -(1 << 63)}),
                           [R(1, H(1), [(WRITE, b"n"), (WRITE, b"m"), (WRITE, b"w"), (WRITE, b"v")]),
                            R((1 << 32) - 1, H(2), [(WRITE, b"n"), (WRITE, b"m"), (WRITE, b"w"), (WRITE, b"v")])])
    return c


def random_reqs(rng, n_reqs: int, n_keys: int = 40, seeds=(0, 1, 2, 7, 1000), n_hashes: int = 6, max_ops: int = 5):
    keys = [b"DEMO_KEY_STRESS_TEST_%d" % i for i in range(n_keys)] + [b"far-%d" % i for i in range(4)] + [b"missing-%d" % i for i in range(3)]
    reqs = []
    for _ in range(n_reqs):
        ops = []
        for _ in range(int(rng.integers(0, max_ops + 1))):
            u = rng.random()
            action = WRITE if u < 0.6 else DELETE if u < 0.85 else READ
            key = b"" if rng.random() < 0.03 else keys[int(rng.integers(0, len(keys)))]
            if key.startswith(b"missing"):
                action = DELETE if action == WRITE else action  # stays absent
            ops.append((action, key))
        reqs.append(Request(int(seeds[int(rng.integers(0, len(seeds)))]), H(int(rng.integers(0, n_hashes))), ops))
    return reqs


def random_store(rng, n_keys: int = 40) -> Store:
    s = Store(is_local)
    for i in range(n_keys):
        if rng.random() < 0.7:
            s.data[b"DEMO_KEY_STRESS_TEST_%d" % i] = Container(1000 * int(rng.integers(0, 4)))
    return s


def random_cases(n: int = 6, n_reqs: int = 60) -> dict:
    out = {}
    for i in range(n):
        rng = np.random.default_rng(7700 + i)
        store = random_store(rng)
        # a first batch leaves stored grants behind
        warm = random_reqs(rng, 25)
        prepare(store, warm)
        build_batch(store, warm)
        run(store, warm)
        out[f"random{i}"] = (store, random_reqs(rng, n_reqs))
    return out


def alignment_case(n: int = 1500):
    """One-op requests whose key / hash slices and emitted payloads land on every
    (destination, source) residue pair mod 16 (checked by the tests)."""
    rng = np.random.default_rng(1616)
    reqs = [Request(int(rng.integers(0, 1 << 20)), H(i, int(rng.integers(1, 140))),
                    [(WRITE, (b"far" if i % 5 == 0 else b"al") + b"%d" % i + b"x" * int(rng.integers(0, 40)))])
            for i in range(n)]
    pads = rng.integers(0, 16, 4 * n + 8)
    return _store({}), reqs, (lambda i: int(pads[i]))


def all_cases() -> dict:
    c = {}
    for name, (store, reqs) in {**hand_cases(), **edge_cases(), **random_cases()}.items():
        c[name] = (store, reqs, None)
    c["alignment"] = alignment_case()
    return c


def payload_residues(batch: mh.Write1Batch, out: "mh.Write1Issued") -> set:
    """(destination mod 16, source mod 16) of every key and hash payload emitted."""
    vs = lambda v: max(1, (int(v).bit_length() + 6) // 7)
    req_of = np.repeat(np.arange(batch.n_reqs), np.diff(batch.req_op_off.astype(np.int64)))
    seen = set()
    for g in range(out.n_new):
        o = int(out.grant_op[g])
        q = int(req_of[o])
        kl, hl = int(batch.op_key_len[o]), int(batch.req_hash_len[q])
        d = int(out.grant_off[g]) + 1 + vs(kl)
        seen.add((d % 16, int(batch.op_key_off[o]) % 16))
        ts = int(out.grant_ts[g])
        d += kl + (1 + vs(ts & MASK64) if ts else 0) + 1 + vs(hl)
        if hl:
            seen.add((d % 16, int(batch.req_hash_off[q]) % 16))
    return seen
