"""Every scenario of test_cluster_scenarios.py that issues reads, with the servers' read stage
on the library's read path (wire_read_cluster.WireReadCluster): ReadToServer bodies ->
read_request_decode -> one store lookup per distinct key -> read_answer_plan ->
result_reply_encode, host forms on wire-host and device forms on wire-device.  The event log
equals a "host" run's with the same seed; the stage's own checks (plan status against the
model, bodies against result_encode_model) run inside the cluster.  Each test prints the
number of reads that met a present key without a certificate (read_no_cert)."""
import pytest

import cluster_harness as H
import test_cluster_scenarios as TS
import wire_cluster as WC
from wire_read_cluster import WireReadCluster

BACKENDS = [pytest.param("wire-host", id="wire-host"), pytest.param("wire-device", id="wire-device", marks=pytest.mark.gpu)]


@pytest.fixture(params=BACKENDS)
def run(request):
    made = []

    def go(scenario, seed, **kw):
        c = WireReadCluster(backend=request.param, check_oracle=request.param == "wire-device", seed=seed, **kw)
        made.append(c)
        scenario(c)
        m = H.Cluster(backend="host", seed=seed, **kw)
        try:
            scenario(m)
        finally:
            m.close()
        got, want = WC.plain_log(c), WC.plain_log(m)
        assert len(got) == len(want) and got == want, "the wire run's event log differs from the host backend's"
        assert c.stats["wire"]["read_server"] > 0 and c.read_stats["requests"] >= c.stats["reads"] > 0, c.read_stats
        print("read stage", request.param, c.read_stats, "read_no_cert", c.read_no_cert)
        return c

    go.backend = request.param
    yield go
    for c in made:
        c.close()


def _write_then_read(keys_values, extra=None):
    def scenario(c):
        cl = c.new_client()
        r1 = c.execute_write(cl, H.write_ops(*keys_values))
        assert [x.result for x in r1] == [v for _, v in keys_values]
        r2 = c.execute_read(cl, H.read_ops(*[k for k, _ in keys_values]))
        assert [x.result for x in r2] == [v for _, v in keys_values] and all(x.existed for x in r2)
        if extra:
            extra(c, cl)
    return scenario


def test_read_operation(run):
    run(_write_then_read([("DEMO_READ_KEY_1", "NEW_VALUE_FOR_KEY_1_TR_1"), ("DEMO_READ_KEY_2", "NEW_VALUE_FOR_KEY_2_TR_1")]), 1)


def test_demo(run):
    run(_write_then_read([("KEY1", "Hello"), ("KE2", "World")]), 2)


def test_delete_operation(run):
    def then_delete(c, cl):
        r3 = c.execute_write(cl, H.delete_ops("DEMO_READ_KEY_1", "DEMO_READ_KEY_2"))
        assert [x.result for x in r3] == ["", ""] and not r3[0].existed and not r3[1].existed
        r4 = c.execute_read(cl, H.read_ops("DEMO_READ_KEY_1", "DEMO_READ_KEY_2"))
        assert [x.result for x in r4] == ["", ""] and not r4[0].existed and not r4[1].existed

    run(_write_then_read([("DEMO_READ_KEY_1", "NEW_VALUE_FOR_KEY_1_TR_1"), ("DEMO_READ_KEY_2", "NEW_VALUE_FOR_KEY_2_TR_1")],
                         then_delete), 3)


def test_write_operation_overwrite(run):
    def scenario(c):
        cl = c.new_client()
        c.execute_write(cl, H.write_ops(("DEMO_KEY_1", "NEW_VALUE_FOR_KEY_1_TR_1"), ("DEMO_KEY_2", "NEW_VALUE_FOR_KEY_2_TR_1")))
        c.execute_write(cl, H.write_ops(("DEMO_KEY_1", "NEW_VALUE_FOR_KEY_1_TR_2"), ("DEMO_KEY_2", "NEW_VALUE_FOR_KEY_2_TR_2")))
        r3 = c.execute_read(cl, H.read_ops("DEMO_KEY_1", "DEMO_KEY_2"))
        assert [x.result for x in r3] == ["NEW_VALUE_FOR_KEY_1_TR_2", "NEW_VALUE_FOR_KEY_2_TR_2"]

    run(scenario, 4)


def test_write_operation_concurrent(run):
    def scenario(c):
        for _ in range(5):  # one by one
            cl = H.ScriptedClient(c, TS.concurrent_runnable)
            H.run_clients(c, [cl])
            assert cl.error is None, cl.error
        clients = [H.ScriptedClient(c, TS.concurrent_runnable) for _ in range(5)]  # concurrently
        H.run_clients(c, clients)
        for cl in clients:
            assert cl.error is None, cl.error

    run(scenario, 5)


def test_write_operation_concurrent_stress(run):
    n_keys = 4  # 5 clients x 4 keys, as the wire-device run of the parent's test: the same kinds of event
    c = run(TS._stress(n_keys), 6)
    assert c.stats["reads"] == 5 * n_keys


def test_serial_replay_of_the_blocking_handler(run):
    """Clients hammering three shared keys, with read backs (the scenario of the test of that name)."""
    def scenario(c):
        keys = [f"SHARED_KEY_{i}" for i in range(3)]
        clients = [H.ScriptedClient(c, TS.shared_keys_runnable(i, keys, 4, 400 + i)) for i in range(4)]
        H.run_clients(c, clients)
        for cl in clients:
            assert cl.error is None, cl.error

    c = run(scenario, 9)
    assert c.read_stats["keys"] < c.read_stats["ops"]  # reads of one step shared keys: one lookup each


def test_resent_write1_then_read(run):
    def scenario(c):
        cl = c.new_client()
        p = c.start_write(cl, H.write_ops(("RESEND_KEY", "value")))
        s0 = c.send_order[0]
        assert not c.step(deliveries=[(p, s0)])
        c.resend_write1(p, s0)
        assert not c.step(deliveries=[(p, s0)])
        assert c.run(p)[0].result == "value"
        assert c.execute_read(cl, H.read_ops("RESEND_KEY"))[0].result == "value"

    run(scenario, 11)
