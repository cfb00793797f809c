"""Read request decoder and read answer plan on the GPU (mochi_read_request_decode_device,
mochi_read_answer_plan_device): the device forms equal the host forms array for array over
guard-filled outputs, on a stream of their own: the own cases and the mutation corpus in
dense and aliased layouts; request counts around the block and empty-batch edges; op counts
around a block; 65 requests of 64 ops and later passes of the grid-stride entry kernel; a
message that ends the wire; the claim table at its edges (4,097 ops on one key, 3,000
distinct keys that differ in their last bytes); the capacity rule; two streams agree;
scratch that grows between calls; the profile; and the plan on every rule, at request counts
around a block and with each NO_REPLY cause in the last of 64 ops.  (Offsets past 2^32 and
the entry kernel's block cap are left to the Write1 request decoder's tests: the walk, the
key numbering and the entry kernel with its grid are the same code.)"""
import numpy as np
import pytest

import mochi_hip as mh
import read_request_model as RQ
import workload as W

pytestmark = pytest.mark.gpu

FILL = 0xA5


@pytest.fixture(scope="module")
def ver():
    v = mh.Verifier([mh.pem_modulus(p) for p in W.load_keys(4)], 0)
    yield v
    v.close()


def _decode_device(ver, reqs, op_cap, stream=None, check=True):
    import torch

    s = stream or torch.cuda.Stream()
    dr = mh.DeviceReadRequests(reqs, 0)
    out = mh.DeviceReadRequestsDecoded(dr.n_reqs, op_cap, fill=FILL)
    torch.cuda.synchronize()  # uploads and fills went to the current stream
    rc = ver.read_request_decode_device(dr, out, stream=s.cuda_stream, check=check)
    torch.cuda.synchronize()
    return out.to_host(rc)


def _assert_decoded(got, want, O, U):
    """The guard-filled device outputs `got` hold the trimmed arrays `want` and nothing else."""
    assert got.rc == mh.OK and (got.n_ops, got.n_keys) == (O, U)
    RQ.assert_equal(got.trimmed(), want)
    for k, (dt, w) in mh._RDQ_OUT.items():  # nothing past the counts is written
        if w in ("O", "K"):
            assert (got.arrays[k][O if w == "O" else U:].view(np.uint8) == FILL).all(), k


def _device_equals_host(ver, reqs, slack=3, model=False):
    host = mh.read_request_decode(reqs)
    got = _decode_device(ver, reqs, host.n_ops + slack)
    _assert_decoded(got, host.trimmed(), host.n_ops, host.n_keys)
    if model:
        RQ.assert_equal(got.trimmed(), RQ.decode(reqs))
    return host


# 1. device == host == model -------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["dense", "aliased"])
@pytest.mark.parametrize("which", ["own", "mutations"])
def test_cases_device_equals_host_and_model(ver, which, layout):
    cases = RQ.own_cases() if which == "own" else RQ.mutations()
    host = _device_equals_host(ver, RQ.batch([c.body for c in cases], layout), model=True)
    assert set(host.arrays["req_status"].tolist()) == ({0, 1, 2} if which == "own" else {0, 1})


@pytest.mark.parametrize("name", sorted(RQ.dedup_batches()))
def test_key_numbering_device_equals_host(ver, name):
    _device_equals_host(ver, RQ.batch(RQ.dedup_batches()[name]), model=True)


# 2. the launch sequence's edges ---------------------------------------------------------------
@pytest.mark.parametrize("Q", [0, 1, 255, 256, 257])
def test_request_counts_around_the_launch_edges(ver, Q):
    cases = [c for c in RQ.own_cases() if not c.name.startswith("ops:6")]
    host = _device_equals_host(ver, RQ.batch([cases[i % len(cases)].body for i in range(Q)]), model=True)
    assert host.arrays["req_op_off"].size == Q + 1


def _ops_lanes(Q):
    """Lanes of the entry kernel's grid: w1_request.h's w1q_ops_blocks(Q) blocks of 256."""
    return 256 * min(max(-(-2 * Q // 256), 1), 4096)


def _full_req(q, n=64, bad=None):
    """A request of n READ ops on keys of its own; op `bad` carries invalid UTF-8 in operand2."""
    return RQ.read(b"c%d" % q, RQ.transaction([RQ.operation(RQ.READ, b"q%d-%d" % (q, j), RQ.BAD_UTF8 if j == bad else b"")
                                               for j in range(n)]), b"n%d" % q)


def test_65_requests_of_64_ops(ver):
    reqs = RQ.batch([_full_req(q) for q in range(65)])
    assert 65 * 64 > 16 * _ops_lanes(65)  # seventeen passes of the one block
    host = _device_equals_host(ver, reqs, model=True)
    assert host.n_ops == host.n_keys == 65 * 64 and (host.arrays["req_status"] == 0).all()


@pytest.mark.parametrize("bad", [(4, 63), (4, 0), (3, 63), None])
def test_entry_kernel_later_pass(ver, bad):
    """Five requests of 64 entries on one block of 256 lanes: request 4's entries are the second
    pass.  A malformed Operation there (its last, its first) or at the first pass's last lane
    takes its request out and no other."""
    reqs = RQ.batch([_full_req(q, bad=bad[1] if bad and bad[0] == q else None) for q in range(5)])
    assert _ops_lanes(5) == 256 == 4 * 64
    host = _device_equals_host(ver, reqs, model=True)
    assert host.arrays["req_status"].tolist() == [int(bad is not None and bad[0] == q) for q in range(5)]
    assert host.n_ops == 64 * (5 - (bad is not None))


@pytest.mark.parametrize("last", ["full", "only:nonce", "action:10_bytes_low_0", "len:past_end", "empty"])
def test_message_ends_the_wire(ver, last):
    """The last message ends on the wire's last byte (the device blob is that long exactly)."""
    by = {c.name: c.body for c in RQ.own_cases()}
    reqs = RQ.batch([by["full"], by["key:multibyte"], by[last]], lead=1, tail=0)
    assert int(reqs.msg_off[-1]) + int(reqs.msg_len[-1]) == reqs.wire.size
    _device_equals_host(ver, reqs, model=True)


# 3. the claim table --------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ops", [1, 2, 1023, 1024, 1025])
def test_op_counts_around_the_launch_edges(ver, n_ops):
    """Half as many keys as ops, each key twice, 33 ops a request; every third op is no READ."""
    ops = [(RQ.READ if o % 3 else RQ.WRITE, b"key-%d" % (o * 5 % max(n_ops // 2, 1))) for o in range(n_ops)]
    host = _device_equals_host(ver, RQ.batch([RQ.req(ops[i:i + 33]) for i in range(0, n_ops, 33)]), model=True)
    assert host.n_ops == n_ops and host.n_keys <= max(n_ops // 2, 1)


def _tiled(bodies_and_counts):
    """(body, count) runs back to back, built with numpy."""
    parts, offs, lens, at = [], [], [], 0
    for body, n in bodies_and_counts:
        parts.append(np.tile(np.frombuffer(body, np.uint8), n))
        offs.append(at + len(body) * np.arange(n, dtype=np.uint64))
        lens.append(np.full(n, len(body), np.uint32))
        at += len(body) * n
    return mh.ReadRequests(wire=np.concatenate(parts), msg_off=np.concatenate(offs).astype(np.uint64),
                           msg_len=np.concatenate(lens))


def test_4097_ops_on_one_key(ver):
    """Every lane on one slot's atomicMin."""
    body = RQ.req([(RQ.READ, b"the-one-key")] * 64)
    host = _device_equals_host(ver, _tiled([(body, 64), (RQ.req([(RQ.READ, b"the-one-key")]), 1)]))
    assert host.n_ops == 4097 and host.n_keys == 1 and (host.arrays["op_obj"][:4097] == 0).all()
    assert host.arrays["key_op"][0] == 0


def test_3000_distinct_keys(ver):
    """3,000 ops, 3,000 keys, 8,192 slots: many probes pass occupied slots.  The keys differ in their
    last bytes alone and are numbered in op order whatever their slots."""
    reqs = RQ.batch([RQ.req([(RQ.READ, b"a-rather-long-common-prefix/%05d" % (60 * q + j)) for j in range(60)]) for q in range(50)])
    host = _device_equals_host(ver, reqs)
    assert host.n_ops == host.n_keys == 3000
    assert host.arrays["op_obj"].tolist() == list(range(3000)) == host.arrays["key_op"].tolist()


# 4. the capacity rule, two streams, scratch growth, the profile ---------------------------------------
def test_capacity_one_short_touches_nothing(ver):
    reqs = RQ.batch([c.body for c in RQ.own_cases()])
    host = mh.read_request_decode(reqs)
    got = _decode_device(ver, reqs, host.n_ops - 1, check=False)
    assert got.rc == mh.EINVAL and got.n_ops == host.n_ops
    for k, (dt, w) in mh._RDQ_OUT.items():
        if w in ("O", "K"):
            assert (got.arrays[k].view(np.uint8) == FILL).all(), k
        else:
            np.testing.assert_array_equal(got.arrays[k], host.arrays[k])
    assert got.n_keys == int.from_bytes(bytes([FILL]) * 4, "little")  # the device word is untouched too
    _assert_decoded(_decode_device(ver, reqs, host.n_ops), host.trimmed(), host.n_ops, host.n_keys)


def test_two_streams_give_equal_arrays(ver):
    import torch

    reqs = RQ.batch([c.body for c in RQ.own_cases() + RQ.mutations()[::7]])
    host = mh.read_request_decode(reqs)
    dr = mh.DeviceReadRequests(reqs, 0)
    outs = [mh.DeviceReadRequestsDecoded(reqs.n_reqs, host.n_ops, fill=FILL) for _ in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for o, s in zip(outs, streams):
        assert ver.read_request_decode_device(dr, o, stream=s.cuda_stream) == mh.OK
    torch.cuda.synchronize()
    for k in list(mh._RDQ_OUT) + ["n_keys_dev"]:
        assert torch.equal(getattr(outs[0], k), getattr(outs[1], k)), k
    RQ.assert_equal(outs[1].to_host().trimmed(), host.trimmed())


def test_scratch_growth_across_streams():
    """A fresh context; three calls alternating between two streams with nothing between them but
    what a call itself waits for: small, large, small.  The second call's batch needs other
    scratch sizes (per request and per op) than the first's.  Each call has guard-filled
    outputs of its own."""
    import torch

    small = RQ.batch([c.body for c in RQ.mutations()[:8]] + [RQ.req([(RQ.READ, b"s")])])
    large = RQ.batch([_full_req(q) for q in range(300)])
    seq = [small, large, small]
    hosts = [mh.read_request_decode(r) for r in seq]
    assert hosts[0].n_ops > 0 and hosts[1].n_ops > 0
    drs = [mh.DeviceReadRequests(r, 0) for r in seq]
    outs = [mh.DeviceReadRequestsDecoded(r.n_reqs, h.n_ops + 3, fill=FILL) for r, h in zip(seq, hosts)]
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    v = mh.Verifier([mh.pem_modulus(p) for p in W.load_keys(1)], 0)
    torch.cuda.synchronize()
    rcs = [v.read_request_decode_device(dr, o, stream=st.cuda_stream) for dr, o, st in zip(drs, outs, (a, b, a))]
    torch.cuda.synchronize()
    for rc, o, h in zip(rcs, outs, hosts):
        _assert_decoded(o.to_host(rc), h.trimmed(), h.n_ops, h.n_keys)
    v.close()


def test_profile_reader(ver):
    reqs = RQ.batch([_full_req(q) for q in range(40)])
    host = mh.read_request_decode(reqs)
    ver.set_profiling(True)
    try:
        got = _decode_device(ver, reqs, host.n_ops)
        prof = ver.read_read_decode_profile()
    finally:
        ver.set_profiling(False)
    assert got.rc == mh.OK and tuple(prof) == mh.READ_REQUEST_STAGES
    assert all(v >= 0 for v in prof.values())
    assert all(prof[k] > 0 for k in ("k_rdq_req", "k_w1q_ops", "k_rdq_emit", "k_w1q_claim", "k_w1q_rank", "k_w1q_number"))


# 5. the plan ------------------------------------------------------------------------------------------
def _plan_device_equals_host(ver, reqs, lookup=RQ.store_lookup):
    """decode -> plan on one stream with no wait between them but the decoder's own; every
    planned array equals the host form's over the fill, and the host form the model."""
    import torch

    host = mh.read_request_decode(reqs)
    t = host.trimmed()
    ks = RQ.key_state(reqs, t, lookup)
    want = mh.read_answer_plan(host, ks, fill=FILL)
    RQ.assert_planned(want, reqs, t, ks, lookup)
    s = torch.cuda.Stream()
    dr = mh.DeviceReadRequests(reqs, 0)
    dec = mh.DeviceReadRequestsDecoded(dr.n_reqs, host.n_ops + 2, fill=FILL)
    dks = mh.DeviceReadKeyState(ks, 0)
    out = mh.DeviceReadAnswerPlanned(dr.n_reqs, host.n_ops + 2, fill=FILL)
    torch.cuda.synchronize()
    assert ver.read_request_decode_device(dr, dec, stream=s.cuda_stream) == mh.OK
    mh.read_answer_plan_device(dec, dks, out, stream=s.cuda_stream)
    torch.cuda.synchronize()
    got = out.to_host()
    for k, (dt, w) in mh._RDA_OUT.items():
        n = reqs.n_reqs if w == "Q" else host.n_ops
        np.testing.assert_array_equal(got[k][:n], want[k], err_msg=k)
        assert (got[k][n:].view(np.uint8) == FILL).all(), k  # the two slots of slack
    return want


@pytest.mark.parametrize("layout", ["dense", "aliased"])
def test_plan_cases_device_equals_host(ver, layout):
    want = _plan_device_equals_host(ver, RQ.batch([c.body for c in RQ.plan_cases()], layout))
    assert set(want["plan_status"].tolist()) == {mh.RDA_REPLY, mh.RDA_NO_REPLY, mh.RDA_HOST}


@pytest.mark.parametrize("Q", [0, 1, 255, 256, 257])
def test_plan_request_counts_around_a_block(ver, Q):
    cases = RQ.plan_cases()
    _plan_device_equals_host(ver, RQ.batch([cases[i % len(cases)].body for i in range(Q)]))


@pytest.mark.parametrize("cause", sorted(RQ.NO_REPLY_CAUSES))
def test_plan_64_ops_cause_in_the_last_op(ver, cause):
    want = _plan_device_equals_host(ver, RQ.batch([RQ.full_request(None), RQ.full_request(cause), RQ.full_request(None)]))
    assert want["plan_status"].tolist() == [mh.RDA_REPLY, mh.RDA_NO_REPLY, mh.RDA_REPLY]
    assert (want["op_status"][64:128] == 0xFF).all()
