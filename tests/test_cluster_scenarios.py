"""The reference's own integration scenarios, replayed through libmochi_hip.

Each test restates one of MochiClientServerCommunicationTest.java's tests on a
fresh in-process 4-server-of-5 cluster built from the reference's
config/sample_config (tests/cluster_harness.py) and asserts exactly what that
test asserts.  Every Write1 grant is signed by its server, every Write2
certificate goes through the batcher's request API with the receiving server's
stored state, and the per-op apply/read decisions the library returns drive
the server model — so these outcomes (the only behavioural expectations the
reference holds for this path) pin the tally / apply semantics (SURVEY §8 a3,
a4, a7) end to end.

* CPU (`-m "not gpu"`): backend "host" — the library's host signing, Write1
  classification and response tally, with Write2 verdicts from the oracle.
* GPU (`-m gpu`): backend "device" — k_rsa_sign, the device classify / tally
  kernels and the batched Write2 verify, and the oracle re-checks every Write2
  verdict and per-op output on the same message and state.
* "wire-host" (CPU) and "wire-device" (GPU), tests/wire_cluster.py: every message
  between a client and a server is protobuf bytes the library's codecs produced
  and consume (request decode, key-state join, grant issuance, reply encode and
  decode, Write2 encode, wire-level verify, answer plan, answer encode and decode
  with coalescing), each stage held against the Python model beside it.  A wire
  run's event log must equal that of a "host" cluster run beside it with the same
  seed and script, and every stage must have run (stats["wire"]).

Not on the wire backends, on purpose:
* test_async_handler_race_protocol — the asynchronous handler goes through the
  batcher's per-request API, which produces no verdict arrays for the answer plan;
* test_write_operation_concurrent_stress at 5 clients x 40 keys (569 steps) — the
  wire backends run the same scenario at 5 x 8 (117 steps, every kind of event; 5 x 4 on
  wire-device, for time) in test_write_operation_concurrent_stress_wire.
"""
import pytest

import cluster_harness as H
import mochi_hip as mh
import wire_cluster as WC

MODEL_BACKENDS = [pytest.param("host", id="host"), pytest.param("device", id="device", marks=pytest.mark.gpu)]
WIRE_BACKENDS = [pytest.param("wire-host", id="wire-host"),
                 pytest.param("wire-device", id="wire-device", marks=pytest.mark.gpu)]
BACKENDS = MODEL_BACKENDS + WIRE_BACKENDS
W1_STAGES = ("w1_server", "w1_client")


def _maker(backend):
    made = []

    def mk(seed=1, **kw):
        if backend.startswith("wire"):
            c = WC.WireCluster(backend=backend, check_oracle=backend == "wire-device", seed=seed, **kw)
        else:
            c = H.Cluster(backend=backend, check_oracle=backend == "device", seed=seed, **kw)
        made.append(c)
        return c

    def run(scenario, seed=1, stages=(), **kw):
        """Run scenario(cluster).  A wire backend's run is followed by the same scenario on a
        "host" cluster with the same seed: the event logs are equal, and the named stages ran."""
        c = mk(seed, **kw)
        scenario(c)
        if c.wire:
            m = H.Cluster(backend="host", seed=seed, **kw)
            try:
                scenario(m)
            finally:
                m.close()
            got, want = WC.plain_log(c), WC.plain_log(m)
            assert len(got) == len(want) and got == want, "the wire run's event log differs from the host backend's"
            for st in stages:
                assert c.stats["wire"][st] > 0, (st, c.stats["wire"])
            print("wire stats", backend, {k: v for k, v in c.stats.items() if k != "wire"}, c.stats["wire"])
        return c

    mk.run = run
    mk.backend = backend
    return mk, made


def _closed(made):
    for c in made:
        if c.backend == "device":  # every verdict applied was re-checked (async: every submission)
            assert c.stats["oracle_checked"] == c.stats["write2"] + c.stats["resubmits"], c.stats
        c.close()


@pytest.fixture(params=BACKENDS)
def make_cluster(request):
    mk, made = _maker(request.param)
    yield mk
    _closed(made)


@pytest.fixture(params=MODEL_BACKENDS)
def make_model_cluster(request):
    mk, made = _maker(request.param)
    yield mk
    _closed(made)


@pytest.fixture(params=WIRE_BACKENDS)
def make_wire_cluster(request):
    mk, made = _maker(request.param)
    yield mk
    _closed(made)


def check_in(v, *allowed):
    return v in allowed


def test_read_operation(make_cluster):
    """testReadOperation (MochiClientServerCommunicationTest.java:173-223)."""
    def scenario(c):
        cl = c.new_client()
        ops = H.write_ops(("DEMO_READ_KEY_1", "NEW_VALUE_FOR_KEY_1_TR_1"), ("DEMO_READ_KEY_2", "NEW_VALUE_FOR_KEY_2_TR_1"))
        r1 = c.execute_write(cl, ops)
        assert len(r1) == 2
        assert r1[0].result == "NEW_VALUE_FOR_KEY_1_TR_1"
        assert r1[1].result == "NEW_VALUE_FOR_KEY_2_TR_1"
        assert r1[0].cert is not None and r1[1].cert is not None
        assert r1[0].existed and r1[1].existed
        r2 = c.execute_read(cl, H.read_ops("DEMO_READ_KEY_1", "DEMO_READ_KEY_2"))
        assert len(r2) == 2
        assert r2[0].result == "NEW_VALUE_FOR_KEY_1_TR_1"
        assert r2[1].result == "NEW_VALUE_FOR_KEY_2_TR_1"
        # every replica applied the certificate and moved the epoch past the grant
        for s in c.replica_idx:
            for k in ("DEMO_READ_KEY_1", "DEMO_READ_KEY_2"):
                sv = c.servers[s].store[k]
                assert sv.current_c is r1[0].cert and sv.epoch == 1000 and not sv.given
                if c.wire:  # the same on the wire: the bytes the client got are the bytes the replica stored
                    assert c.cert_bytes[id(sv.current_c)] == r1[0].cert_bytes == r2[0].cert_bytes
                    assert r1[0].cert_bytes == c.cert_wire(r1[0].cert, ops) and len(r1[0].cert_bytes) > 4 * 2 * 256

    make_cluster.run(scenario, 1, WC.WRITE_STAGES + WC.READ_STAGES)


def test_demo(make_cluster):
    """testDemo (:225-255)."""
    def scenario(c):
        cl = c.new_client()
        c.execute_write(cl, H.write_ops(("KEY1", "Hello"), ("KE2", "World")))
        r = c.execute_read(cl, H.read_ops("KEY1", "KE2"))
        assert r[0].result == "Hello" and r[1].result == "World"

    make_cluster.run(scenario, 2, WC.WRITE_STAGES + WC.READ_STAGES)


def test_delete_operation(make_cluster):
    """testDeleteOperation (:257-348).  The client sends every Write1 op as a
    WRITE without value (MochiDBClient.java:256-261), so the Write1 of a delete
    creates the container and the delete applies at Write2."""
    def scenario(c):
        cl = c.new_client()
        r1 = c.execute_write(cl, H.write_ops(("DEMO_READ_KEY_1", "NEW_VALUE_FOR_KEY_1_TR_1"),
                                             ("DEMO_READ_KEY_2", "NEW_VALUE_FOR_KEY_2_TR_1")))
        assert [x.result for x in r1] == ["NEW_VALUE_FOR_KEY_1_TR_1", "NEW_VALUE_FOR_KEY_2_TR_1"]
        assert all(x.cert is not None and x.existed for x in r1)
        r2 = c.execute_read(cl, H.read_ops("DEMO_READ_KEY_1", "DEMO_READ_KEY_2"))
        assert [x.result for x in r2] == ["NEW_VALUE_FOR_KEY_1_TR_1", "NEW_VALUE_FOR_KEY_2_TR_1"]
        r3 = c.execute_write(cl, H.delete_ops("DEMO_READ_KEY_1", "DEMO_READ_KEY_2"))
        assert len(r3) == 2
        assert r3[0].result == "" and r3[1].result == ""
        assert not r3[0].existed and not r3[1].existed
        r4 = c.execute_read(cl, H.read_ops("DEMO_READ_KEY_1", "DEMO_READ_KEY_2"))
        assert len(r4) == 2
        assert r4[0].result == "" and r4[1].result == ""
        assert not r4[0].existed and not r4[1].existed

    make_cluster.run(scenario, 3, WC.WRITE_STAGES + WC.READ_STAGES)


def test_write_operation_overwrite(make_cluster):
    """testWriteOperation (:350-416): the second certificate's g0 timestamp is in
    the next epoch (StoreValueObjectContainer.java:83-88, Write1 issuance at
    InMemoryDataStore.java:127), so it lands on APPLY, not READ (:594-599)."""
    def scenario(c):
        cl = c.new_client()
        r1 = c.execute_write(cl, H.write_ops(("DEMO_KEY_1", "NEW_VALUE_FOR_KEY_1_TR_1"),
                                             ("DEMO_KEY_2", "NEW_VALUE_FOR_KEY_2_TR_1")))
        assert [x.result for x in r1] == ["NEW_VALUE_FOR_KEY_1_TR_1", "NEW_VALUE_FOR_KEY_2_TR_1"]
        assert all(x.cert is not None and x.existed for x in r1)
        ts1 = r1[0].cert.ts_for("DEMO_KEY_1")
        r2 = c.execute_write(cl, H.write_ops(("DEMO_KEY_1", "NEW_VALUE_FOR_KEY_1_TR_2"),
                                             ("DEMO_KEY_2", "NEW_VALUE_FOR_KEY_2_TR_2")))
        assert len(r2) == 2
        assert r2[0].result == "NEW_VALUE_FOR_KEY_1_TR_2" and r2[0].existed
        assert r2[1].result == "NEW_VALUE_FOR_KEY_2_TR_2" and r2[1].existed
        ts2 = r2[0].cert.ts_for("DEMO_KEY_1")
        assert ts1 < 1000 <= ts2 < 2000  # epoch 0 grant, then an epoch-1000 grant
        assert c.stats["read_branch"] == 0
        r3 = c.execute_read(cl, H.read_ops("DEMO_KEY_1", "DEMO_KEY_2"))
        assert [x.result for x in r3] == ["NEW_VALUE_FOR_KEY_1_TR_2", "NEW_VALUE_FOR_KEY_2_TR_2"]

    make_cluster.run(scenario, 4, WC.WRITE_STAGES + WC.READ_STAGES)


def concurrent_runnable(cl):
    """MochiConcurrentTestRunnable.runTest (:499-595)."""
    r1 = yield ("write", H.write_ops(("DEMO_KEY_1", "NEW_VALUE_FOR_KEY_1_TR_1"),
                                     ("DEMO_KEY_2", "NEW_VALUE_FOR_KEY_2_TR_1")))
    assert isinstance(r1, list) and len(r1) == 2, r1
    assert check_in(r1[0].result, "NEW_VALUE_FOR_KEY_1_TR_1", "NEW_VALUE_FOR_KEY_1_TR_2")
    assert check_in(r1[1].result, "NEW_VALUE_FOR_KEY_2_TR_1", "NEW_VALUE_FOR_KEY_2_TR_2")
    assert r1[0].cert is not None and r1[1].cert is not None
    r2 = yield ("write", H.write_ops(("DEMO_KEY_1", "NEW_VALUE_FOR_KEY_1_TR_2"),
                                     ("DEMO_KEY_2", "NEW_VALUE_FOR_KEY_2_TR_2")))
    assert isinstance(r2, list) and len(r2) == 2, r2
    assert r2[0].existed and check_in(r2[0].result, "NEW_VALUE_FOR_KEY_1_TR_1", "NEW_VALUE_FOR_KEY_1_TR_2")
    assert r2[1].existed and check_in(r2[1].result, "NEW_VALUE_FOR_KEY_2_TR_1", "NEW_VALUE_FOR_KEY_2_TR_2")
    r3 = yield ("read", H.read_ops("DEMO_KEY_1", "DEMO_KEY_2"))
    assert isinstance(r3, list) and len(r3) == 2, r3
    assert check_in(r3[0].result, "NEW_VALUE_FOR_KEY_1_TR_1", "NEW_VALUE_FOR_KEY_1_TR_2")
    assert check_in(r3[1].result, "NEW_VALUE_FOR_KEY_2_TR_1", "NEW_VALUE_FOR_KEY_2_TR_2")
    r4 = yield ("write", H.write_ops(("DEMO_KEY_TEST_1", "1")))
    assert isinstance(r4, list), r4
    r5 = yield ("write", H.write_ops(("DEMO_KEY_TEST_2", "2")))
    assert isinstance(r5, list), r5


def test_write_operation_concurrent(make_cluster):
    """testWriteOperationConcurrent (:418-475): five clients run the runnable one
    by one, then all five concurrently (here: interleaved by the scheduler)."""
    def scenario(c):
        for _ in range(5):  # one by one
            cl = H.ScriptedClient(c, concurrent_runnable)
            H.run_clients(c, [cl])
            assert cl.error is None, cl.error
        clients = [H.ScriptedClient(c, concurrent_runnable) for _ in range(5)]  # concurrently
        H.run_clients(c, clients)
        for cl in clients:
            assert cl.error is None, cl.error
        # the interleaving really was concurrent: Write1 rounds saw mixed epochs and retried,
        # and late certificates took the READ branch
        assert c.stats["retries"] > 0 or c.stats["read_branch"] > 0, c.stats

    c = make_cluster.run(scenario, 5, WC.WRITE_STAGES + WC.READ_STAGES)
    if c.wire:  # the batch-wide logic really ran: requests sharing a key in one batch, several Write2s in one
        w = c.stats["wire"]
        assert w["w1_multi_shared_key"] > 0 and w["w2_multi"] > 0 and c.stats["read_branch"] > 0, c.stats
        assert w["read_branch_answers"] == c.stats["read_branch"]


def stress_runnable(start, n, seed):
    """MochiConcurrentStreeTestRunnable.runTest (:721-753)."""
    def script(cl):
        import random

        rng = random.Random(seed)
        nums = list(range(start, start + n))
        rng.shuffle(nums)
        for i in nums:
            key = f"DEMO_KEY_STRESS_TEST_{i}"
            r = yield ("write", H.write_ops((key, f"New Value for key {key}")))
            assert isinstance(r, list), r
        rng.shuffle(nums)
        for i in nums:
            key = f"DEMO_KEY_STRESS_TEST_{i}"
            r = yield ("read", H.read_ops(key))
            assert isinstance(r, list), r
            assert r[0].result == f"New Value for key {key}"
        for i in nums:
            key = f"DEMO_KEY_STRESS_TEST_{i}"
            r = yield ("write", H.delete_ops(key))
            assert isinstance(r, list), r
    return script


def _stress(n_keys):
    def scenario(c):
        clients = [H.ScriptedClient(c, stress_runnable(n_keys * i, n_keys, 100 + i)) for i in range(5)]
        H.run_clients(c, clients)
        for cl in clients:
            assert cl.error is None, cl.error
        assert c.stats["write2"] == 5 * 2 * n_keys * c.R
    return scenario


def test_write_operation_concurrent_stress(make_model_cluster):
    """testWriteOperationConcurrentStressTest (:636-685): 5 clients x 40 keys each
    (disjoint ranges): write all, read all back, delete all — concurrently."""
    make_model_cluster.run(_stress(40), 6)


def test_write_operation_concurrent_stress_wire(make_wire_cluster):
    """The same scenario through the wire codecs at 5 clients x 8 keys each: 117 steps and
    about 460 server batches, writes, reads and deletes of every client interleaved.
    wire-device runs 5 x 4 keys: at 5 x 8 it took 9.6 s on an MI355X (each batch waits for
    its own kernels), and the smaller run holds the same kinds of event."""
    n_keys = 4 if make_wire_cluster.backend == "wire-device" else 8
    c = make_wire_cluster.run(_stress(n_keys), 6, WC.WRITE_STAGES + WC.READ_STAGES)
    w = c.stats["wire"]
    assert w["w1_multi"] > 0 and w["w2_multi"] > 0 and c.stats["reads"] == 5 * n_keys, c.stats


def test_java_collection_orders():
    """The orders the harness reproduces: String.hashCode / Server.hashCode and
    HashMap iteration (bucket = spread(hash) & 15, collisions in insertion order)."""
    assert H.java_string_hash("") == 0
    assert H.java_string_hash("a") == 97
    assert H.java_string_hash("hello") == 99162322
    assert H.java_string_hash("DEMO_KEY_1") == (0x0 + sum(ord(ch) * 31 ** (9 - i) for i, ch in enumerate("DEMO_KEY_1"))) % 2**32
    # two keys in one bucket keep insertion order; a lower bucket comes first
    ids = ["server-55a78d3f-783d-43ae-95c1-6d0f5f02fe0c", "server-6c023c90-87ed-40d9-8f38-48cb03fa2135",
           "server-ed25bc93-1047-4242-b87b-2246355b020b"]
    h = [H.java_string_hash(x) for x in ids]
    assert H.java_hash_order(ids, h) == [ids[2], ids[0], ids[1]]
    assert H.java_hash_order(ids[1::-1], h[1::-1]) == [ids[1], ids[0]]
    # resize past 12 entries keeps every key once
    keys = [f"k{i}" for i in range(40)]
    assert sorted(H.java_hash_order(keys, [H.java_string_hash(k) for k in keys])) == sorted(keys)


def test_rejected_certificate_hangs_the_client(make_cluster):
    """A tampered Write2 (a MultiGrant signature flipped on every replica's
    copy) is rejected by the servers; the reference throws inside
    processWrite2ToServer, sends no Write2Ans, and the client waits forever.
    The wire backends tamper the bytes of the message itself: one signature byte
    of each MultiGrant's first grant."""
    def scenario(c):
        cl = c.new_client()
        p = c.start_write(cl, H.write_ops(("DEMO_KEY_X", "v")))
        while p.kind == "W1":
            for q, out in c.step():
                assert q is not p, out
        if c.wire:
            msg = bytearray(p.msg)
            for _, mg in p.cert.mgs:
                at = bytes(msg).find(mg.grant(p.ops[0].key).sig)
                assert at > 0
                msg[at] ^= 1
            assert len(msg) == len(p.msg) and sum(a != b for a, b in zip(msg, p.msg)) == c.R
            p.msg = bytes(msg)
        else:
            # corrupt one grant signature of every MultiGrant before Write2 is delivered
            for _, mg in p.cert.mgs:
                g = mg.grants[0]
                g.sig = bytes([g.sig[0] ^ 1]) + g.sig[1:]
            import workload as W

            wc = b"".join(W.encode_map_entry(1, sid.encode(), mg.encode()) for sid, mg in p.cert.mgs)
            p.msg = W._ld(1, wc) + W._ld(2, H.encode_txn(p.ops))
        with pytest.raises(H.Hung):
            c.run(p)
        for s in c.replica_idx:  # nothing applied
            assert c.servers[s].store["DEMO_KEY_X"].current_c is None

    make_cluster.run(scenario, 7, ("w1_server", "w1_client", "w2_encode", "w2_server"))


def shared_keys_runnable(cid, keys, rounds, seed):
    """Clients hammering the same few keys: writes of one or two shared keys, read
    backs (the value is some client's write)."""
    def script(cl):
        import random

        rng = random.Random(seed)
        for j in range(rounds):
            ks = sorted(rng.sample(keys, rng.choice((1, 2))))
            r = yield ("write", H.write_ops(*[(k, f"c{cid}-{j}-{k}") for k in ks]))
            if isinstance(r, H.ClientError):
                continue  # a refused Write1 round (RequestRefused) is the reference's outcome too
            assert isinstance(r, list) and len(r) == len(ks), r
            r = yield ("read", H.read_ops(*ks))
            assert isinstance(r, list), r
            for k, x in zip(ks, r):
                assert x.result.startswith("c") and x.result.endswith(k), x
    return script


def test_async_handler_race_protocol(make_model_cluster):
    """INTEGRATION.md §4's asynchronous handler with Write2s on the
    same keys in flight together.  Each server snapshots the verifier's inputs,
    releases the locks and submits (mochi_batcher_submit_request); completions are
    applied at later steps after the sameWrite2State re-check, resubmitting when a
    Write2 on one of the keys landed meanwhile.  The reference's assertions hold,
    resubmissions happen, and every reply and the final per-key state equal a
    serial replay of the same events through the oracle (the reference holds the
    key write locks across validation and apply, InMemoryDataStore.java:641-666).
    Not on the wire backends (see the module docstring)."""
    c = make_model_cluster(seed=8, async_w2=True)
    clients = [H.ScriptedClient(c, concurrent_runnable) for _ in range(5)]
    keys = [f"SHARED_KEY_{i}" for i in range(3)]
    clients += [H.ScriptedClient(c, shared_keys_runnable(i, keys, 6, 300 + i)) for i in range(6)]
    H.run_clients(c, clients)
    for cl in clients:
        assert cl.error is None, cl.error
    assert c.stats["max_same_key_inflight"] >= 2, c.stats
    assert c.stats["resubmits"] > 0, c.stats
    assert not c.async_q
    n = H.replay_serial(c)
    assert n > 0 and c.stats["write2"] == sum(1 for e in c.log if e[1] == "W2")


def test_serial_replay_of_the_blocking_handler(make_cluster):
    """The replay check itself, on the blocking handler's stress run (no Write2 ever
    races there): replies and final state equal the serial oracle replay."""
    def scenario(c):
        keys = [f"SHARED_KEY_{i}" for i in range(3)]
        clients = [H.ScriptedClient(c, shared_keys_runnable(i, keys, 4, 400 + i)) for i in range(4)]
        H.run_clients(c, clients)
        for cl in clients:
            assert cl.error is None, cl.error
        assert c.stats["resubmits"] == 0
        assert H.replay_serial(c) > 0

    make_cluster.run(scenario, 9, WC.WRITE_STAGES + WC.READ_STAGES)


# --- Write1 paths the reference's scenarios never reach: seeds are random in [0, 1000) and never collide there ---
def test_equal_seeds_are_refused(make_cluster):
    """Two clients write the same key with the same seed and different values, so both ask
    every replica for the same timestamp (InMemoryDataStore.java:233-310).  Delivery is
    scripted: replica 0 sees A then B in one step, replica 1 sees A and a step later B,
    replicas 2 and 3 the same with B first.  Each replica refuses the later request, naming
    the holder's grant: twice inside one batch, twice from a stored grant.  Each client's two
    OK grants carry one timestamp, so there is no retry (MochiDBClient.java:310-318), and
    with a refusal among the replies both throw RequestRefusedException (:320-327, the
    oracle's restatement agrees); nothing is applied."""
    import oracle_ffi as O

    key = "EQUAL_SEED_KEY"

    def scenario(c):
        c.seed_hook = lambda p, drawn: 7
        a = c.start_write(c.new_client(), H.write_ops((key, "value-a")))
        b = c.start_write(c.new_client(), H.write_ops((key, "value-b")))
        assert a.seed == b.seed == 7 and a.thash != b.thash
        s = c.send_order
        done = c.step(deliveries=[(a, s[0]), (b, s[0]), (a, s[1]), (b, s[2]), (a, s[2]), (b, s[3])])
        assert not done
        done = c.step(deliveries=[(b, s[1]), (a, s[3])])
        assert sorted(p.client for p, _ in done) == [a.client, b.client]
        for p, out in done:
            assert isinstance(out, H.RequestRefused), out
            round_ = [({"OK": mh.W1_OK, "REFUSED": mh.W1_REFUSED}[kind], c.replica_ids.index(mg.server_id),
                       [(0, g.ts, g.status) for g in mg.grants]) for kind, mg in (p.replies[i] for i in s)]
            assert O.write1_classify([round_]).tolist() == [mh.W1_THROW_REFUSED]
        # per replica: the first request holds the grant, the later one is refused with that very grant
        for i, (first, later) in enumerate(((a, b), (a, b), (b, a), (b, a))):
            k1, mg1 = first.replies[s[i]]
            k2, mg2 = later.replies[s[i]]
            assert (k1, k2) == ("OK", "REFUSED")
            assert len(mg2.grants) == 1 and mg2.grants[0] is mg1.grants[0]
            assert mg2.grants[0].ts == 7 and mg2.grants[0].txn_hash == first.thash != later.thash
        assert (c.stats["w1_refused"], c.stats["w1_refused_in_batch"], c.stats["w1_refused_stored"]) == (4, 2, 2), c.stats
        assert c.stats["write2"] == 0 and not c.inflight
        for i in c.replica_idx:  # nothing applied for a refused client
            sv = c.servers[i].store[key]
            assert sv.current_c is None and sv.value is None and not sv.available and sorted(sv.given) == [7]
        if c.wire:  # the refusals crossed the wire, and the library made them in both ways
            w = c.stats["wire"]
            assert (w["refused_bodies"], w["refused_in_batch"], w["refused_stored"]) == (4, 2, 2), w
            refused = [(step, srv, body) for step, srv, p, kind, body in c.w1_bodies if kind == "REFUSED"]
            assert len(refused) == 4 and all(len(body) > 256 for _, _, body in refused)

    make_cluster.run(scenario, 10, W1_STAGES)


def test_resent_write1_is_answered_from_the_stored_grant(make_cluster):
    """The same Write1 (same hash, same seed) reaches a replica again before its Write2: the
    reply is OK with the grant and the signature issued the first time
    (InMemoryDataStore.java:139-147: the grant given before), no new grant is signed, and on
    the wire the second reply is byte-equal to the first.  The write then completes."""
    def scenario(c):
        cl = c.new_client()
        p = c.start_write(cl, H.write_ops(("RESEND_KEY", "value")))
        s0 = c.send_order[0]
        assert not c.step(deliveries=[(p, s0)])
        kind1, mg1 = p.replies[s0]
        body1 = p.wire.get(s0)
        signed, sig1 = c.stats["signed"], mg1.grants[0].sig
        assert kind1 == "OK" and signed == 1 and len(sig1) == 256
        c.resend_write1(p, s0)
        assert not c.step(deliveries=[(p, s0)])
        kind2, mg2 = p.replies[s0]
        assert kind2 == "OK" and mg2.grants[0] is mg1.grants[0] and mg2.grants[0].sig == sig1
        assert c.stats["signed"] == signed and c.stats["w1_from_stored"] == 1 and c.stats["w1_refused"] == 0
        assert list(c.servers[s0].store["RESEND_KEY"].given) == [p.seed]
        if c.wire:
            assert p.wire[s0] == body1 and body1[0] == mh.W1_OK and sig1 in body1[1]
            assert c.stats["wire"]["retry_from_stored"] == 1, c.stats["wire"]
        r = c.run(p)
        assert r[0].result == "value" and r[0].existed and c.stats["retries"] == 0
        assert c.execute_read(cl, H.read_ops("RESEND_KEY"))[0].result == "value"

    make_cluster.run(scenario, 11, WC.WRITE_STAGES + WC.READ_STAGES)
