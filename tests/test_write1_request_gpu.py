"""Write1 request decoder and key-state join on the GPU (mochi_write1_request_decode_device,
mochi_write1_state_join_device): the device form equals the host form and the model array
for array on the case sets and the mutation corpus (guard-filled outputs, a stream of its
own); request counts around the block and empty-batch edges; 65 requests of 64 ops; later
passes of the grid-stride entry kernel and its block cap; wire offsets past 4 GiB; a message
that ends the wire; the claim table at its edges (op counts around a block, 4,097 ops on one
key, 3,000 distinct keys in 8,192 slots); the capacity rule; two streams agree; scratch that
grows between calls; the profile; the join; and the server's round with no Python parsing:
bodies -> decode -> join -> issue (signed) -> reply encode on one stream, byte-equal to the
replies of the SoA batch the bodies were encoded from."""
import numpy as np
import pytest

import mochi_hip as mh
import workload as W
import write1_reply_model as RM
import write1_request_model as QM

pytestmark = pytest.mark.gpu

FILL = 0xA5


@pytest.fixture(scope="module")
def signer():
    s = mh.DeviceSigner(W.load_keys(1)[0], 0)
    yield s
    s.close()


def _decode_device(signer, reqs, op_cap, stream=None, check=True, dr=None):
    """dr: the batch already on the device (`reqs` is not read then)."""
    import torch

    s = stream or torch.cuda.Stream()
    dr = dr or mh.DeviceWrite1Requests(reqs, 0)
    out = mh.DeviceWrite1RequestsDecoded(dr.n_reqs, op_cap, fill=FILL)
    torch.cuda.synchronize()  # uploads and fills went to the current stream
    rc = signer.request_decode_device(dr, out, stream=s.cuda_stream, check=check)
    torch.cuda.synchronize()
    return out.to_host(rc)


def _assert_decoded(got, want, O, U):
    """The guard-filled device outputs `got` hold the trimmed arrays `want` and nothing else."""
    assert got.rc == mh.OK and (got.n_ops, got.n_keys) == (O, U)
    QM.assert_equal(got.trimmed(), want)
    for k, (dt, w) in mh._W1Q_OUT.items():  # nothing past the counts is written
        if w in ("O", "K"):
            assert (got.arrays[k][O if w == "O" else U:].view(np.uint8) == FILL).all(), k


def _device_equals_host(signer, reqs, slack=3, model=False):
    host = mh.write1_request_decode(reqs)
    got = _decode_device(signer, reqs, host.n_ops + slack)
    _assert_decoded(got, host.trimmed(), host.n_ops, host.n_keys)
    if model:
        QM.assert_equal(got.trimmed(), QM.decode(reqs))
    return host


# 1. device == host == model -------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["dense", "aliased"])
@pytest.mark.parametrize("which", ["own", "mutations"])
def test_cases_device_equals_host_and_model(signer, which, layout):
    cases = QM.own_cases() if which == "own" else QM.mutations()
    host = _device_equals_host(signer, QM.batch([c.body for c in cases], layout), model=True)
    assert set(host.arrays["req_status"].tolist()) == ({0, 1, 2} if which == "own" else {0, 1})


@pytest.mark.parametrize("name", sorted(QM.dedup_batches()))
def test_key_numbering_device_equals_host(signer, name):
    _device_equals_host(signer, QM.batch(QM.dedup_batches()[name]), model=True)


# 2. the launch sequence's edges ---------------------------------------------------------------
@pytest.mark.parametrize("Q", [0, 1, 255, 256, 257])
def test_request_counts_around_the_launch_edges(signer, Q):
    cases = [c for c in QM.own_cases() if not c.name.startswith("ops:6")]
    host = _device_equals_host(signer, QM.batch([cases[i % len(cases)].body for i in range(Q)]), model=True)
    assert host.arrays["req_op_off"].size == Q + 1


def _ops_lanes(Q):
    """Lanes of k_w1q_ops's grid: w1_request.h's w1q_ops_blocks(Q) blocks, clamp(ceil(2Q / 256), 1, 4096), of 256."""
    return 256 * min(max(-(-2 * Q // 256), 1), 4096)


def _full_req(q, n=64, bad=None):
    """A request of n WRITE ops on keys of its own; op `bad` carries invalid UTF-8 in operand2."""
    return QM.write1(b"c%d" % q, QM.transaction([QM.operation(QM.WRITE, b"q%d-%d" % (q, j), QM.BAD_UTF8 if j == bad else b"v")
                                                 for j in range(n)]), q + 1, b"h%d" % q)


def test_65_requests_of_64_ops(signer):
    reqs = QM.batch([_full_req(q) for q in range(65)])
    assert 65 * 64 > 16 * _ops_lanes(65)  # seventeen passes of the one block
    host = _device_equals_host(signer, reqs, model=True)
    assert host.n_ops == host.n_keys == 65 * 64 and (host.arrays["req_status"] == 0).all()


@pytest.mark.parametrize("bad", [(4, 63), (4, 0), (3, 63), None])
def test_entry_kernel_later_pass(signer, bad):
    """Five requests of 64 entries on one block of 256 lanes: request 4's entries are the second
    pass.  A malformed Operation there (its last, its first) or at the first pass's last lane
    takes its request out and no other."""
    reqs = QM.batch([_full_req(q, bad=bad[1] if bad and bad[0] == q else None) for q in range(5)])
    assert _ops_lanes(5) == 256 == 4 * 64
    host = _device_equals_host(signer, reqs, model=True)
    assert host.arrays["req_status"].tolist() == [int(bad is not None and bad[0] == q) for q in range(5)]
    assert host.n_ops == 64 * (5 - (bad is not None))


def _tiled(bodies_and_counts):
    """(body, count) runs back to back, built with numpy."""
    parts, offs, lens, at = [], [], [], 0
    for body, n in bodies_and_counts:
        parts.append(np.tile(np.frombuffer(body, np.uint8), n))
        offs.append(at + len(body) * np.arange(n, dtype=np.uint64))
        lens.append(np.full(n, len(body), np.uint32))
        at += len(body) * n
    return mh.Write1Requests(wire=np.concatenate(parts), msg_off=np.concatenate(offs).astype(np.uint64),
                             msg_len=np.concatenate(lens))


@pytest.mark.parametrize("Q, second_pass", [(524288, False), (524289, True)])
def test_entry_kernel_block_cap(signer, Q, second_pass):
    """4096 blocks: Q = 524,288 requests of 2 ops fill them without the cap, one pass; at Q =
    524,289 the cap holds and block 0 takes the last request's entries in a second pass.  The
    last request alone is MALFORMED, in its last Operation."""
    good = QM.req([(QM.WRITE, b"hot"), (QM.DELETE, b"cold")])
    bad = QM.write1(b"c", QM.transaction([QM.operation(QM.WRITE, b"hot"), QM.operation(QM.READ, b"x", QM.BAD_UTF8)]), 1, b"h")
    reqs = _tiled([(good, Q - 1), (bad, 1)])
    lanes = _ops_lanes(Q)
    assert lanes == 4096 * 256 == _ops_lanes(Q + 1000) and (2 * Q > lanes) == second_pass and (second_pass or 2 * Q == lanes)
    host = mh.write1_request_decode(reqs)
    got = _decode_device(signer, reqs, host.n_ops + 3)
    _assert_decoded(got, host.trimmed(), 2 * (Q - 1), 2)
    st = host.arrays["req_status"]
    assert st[-1] == mh.W1Q_MALFORMED and (st[:-1] == 0).all() and host.arrays["key_op"][:2].tolist() == [0, 1]


# 3. wire offsets past 4 GiB, the wire's end --------------------------------------------------------
def test_offsets_past_4_gib(signer):
    """The own cases in the last 64 KiB of a wire of 2^32 + 64 KiB bytes: every offset the decoder
    emits is the low-offset decode's plus the displacement."""
    import torch

    size = (1 << 32) + (64 << 10)
    free, _ = torch.cuda.mem_get_info(torch.device("cuda", 0))
    if free < size + (512 << 20):
        pytest.skip(f"{free >> 20} MiB of device memory free, the test wants {(size >> 20) + 512}")
    low = QM.batch([c.body for c in QM.own_cases()], tail=0)
    n = low.wire.size
    D = size - n
    assert n <= 64 << 10 and D + int(low.msg_off.min()) >= 1 << 32
    host = mh.write1_request_decode(low)
    want = {k: v.copy() for k, v in host.trimmed().items()}
    ok = want["req_status"] == mh.W1Q_OK
    for k in ("req_hash_off", "req_client_off"):
        want[k][ok] += np.uint64(D)  # an undecoded request keeps 0 / 0
    want["op_key_off"] += np.uint64(D)
    assert ok.any() and not ok.all()
    small = mh.DeviceWrite1Requests(low, 0)
    big = torch.empty(size, dtype=torch.uint8, device="cuda:0")
    big[D:] = small.wire
    dr = mh.DeviceWrite1Requests.from_tensors(low.n_reqs, wire=big, msg_off=small.msg_off + D, msg_len=small.msg_len)
    got = _decode_device(signer, None, host.n_ops + 3, dr=dr)
    del big, dr
    _assert_decoded(got, want, host.n_ops, host.n_keys)
    assert (got.trimmed()["op_key_off"] >= 1 << 32).all()


@pytest.mark.parametrize("last", ["full", "seed:10_bytes", "only:client", "len:past_end", "empty"])
def test_message_ends_the_wire(signer, last):
    """The last message ends on the wire's last byte (the device blob is that long exactly)."""
    by = {c.name: c.body for c in QM.own_cases()}
    reqs = QM.batch([by["full"], by["key:multibyte"], by[last]], lead=1, tail=0)
    assert int(reqs.msg_off[-1]) + int(reqs.msg_len[-1]) == reqs.wire.size
    _device_equals_host(signer, reqs, model=True)


# 4. the claim table --------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ops", [1, 2, 1023, 1024, 1025])
def test_op_counts_around_the_launch_edges(signer, n_ops):
    """Half as many keys as ops, each key twice, 33 ops a request."""
    ops = [(QM.WRITE if o % 3 else QM.DELETE, b"key-%d" % (o * 5 % max(n_ops // 2, 1))) for o in range(n_ops)]
    host = _device_equals_host(signer, QM.batch([QM.req(ops[i:i + 33]) for i in range(0, n_ops, 33)]), model=True)
    assert host.n_ops == n_ops and host.n_keys == max(n_ops // 2, 1)


def test_4097_ops_on_one_key(signer):
    """Every lane on one slot's atomicMin."""
    body = QM.req([(QM.WRITE, b"the-one-key")] * 64)
    host = _device_equals_host(signer, _tiled([(body, 64), (QM.req([(QM.DELETE, b"the-one-key")]), 1)]))
    assert host.n_ops == 4097 and host.n_keys == 1 and (host.arrays["op_obj"][:4097] == 0).all()
    assert host.arrays["key_op"][0] == 0


def test_3000_distinct_keys(signer):
    """3,000 ops, 3,000 keys, 8,192 slots: many probes pass occupied slots.  The keys differ in their
    last bytes alone and are numbered in op order whatever their slots."""
    reqs = QM.batch([QM.req([(QM.WRITE, b"a-rather-long-common-prefix/%05d" % (60 * q + j)) for j in range(60)]) for q in range(50)])
    host = _device_equals_host(signer, reqs)
    assert host.n_ops == host.n_keys == 3000
    assert host.arrays["op_obj"].tolist() == list(range(3000)) == host.arrays["key_op"].tolist()


# 5. the capacity rule, two streams, scratch growth, the profile ---------------------------------------
def test_capacity_one_short_touches_nothing(signer):
    reqs = QM.batch([c.body for c in QM.own_cases()])
    host = mh.write1_request_decode(reqs)
    got = _decode_device(signer, reqs, host.n_ops - 1, check=False)
    assert got.rc == mh.EINVAL and got.n_ops == host.n_ops
    for k, (dt, w) in mh._W1Q_OUT.items():
        if w in ("O", "K"):
            assert (got.arrays[k].view(np.uint8) == FILL).all(), k
        else:
            np.testing.assert_array_equal(got.arrays[k], host.arrays[k])
    assert got.n_keys == int.from_bytes(bytes([FILL]) * 4, "little")  # the device word is untouched too
    _assert_decoded(_decode_device(signer, reqs, host.n_ops), host.trimmed(), host.n_ops, host.n_keys)


def test_two_streams_give_equal_arrays(signer):
    import torch

    reqs = QM.batch([c.body for c in QM.own_cases() + QM.mutations()[::7]])
    host = mh.write1_request_decode(reqs)
    dr = mh.DeviceWrite1Requests(reqs, 0)
    outs = [mh.DeviceWrite1RequestsDecoded(reqs.n_reqs, host.n_ops, fill=FILL) for _ in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for o, s in zip(outs, streams):
        assert signer.request_decode_device(dr, o, stream=s.cuda_stream) == mh.OK
    torch.cuda.synchronize()
    for k in list(mh._W1Q_OUT) + ["n_keys_dev"]:
        assert torch.equal(getattr(outs[0], k), getattr(outs[1], k)), k
    QM.assert_equal(outs[1].to_host().trimmed(), host.trimmed())


@pytest.mark.parametrize("order", ["small_large_small", "large_small_large"])
def test_scratch_growth_across_streams(order):
    """A fresh signer; three calls alternating between two streams with nothing between them but
    what a call itself waits for; the second call's batch needs other scratch sizes (per
    request and per op) than the first's.  Each call has guard-filled outputs of its own."""
    import torch

    small = QM.batch([c.body for c in QM.mutations()[:8]] + [QM.req([(QM.WRITE, b"s")])])
    large = QM.batch([_full_req(q) for q in range(300)])
    seq = [small, large, small] if order == "small_large_small" else [large, small, large]
    hosts = [mh.write1_request_decode(r) for r in seq]
    assert hosts[0].n_ops > 0 and hosts[1].n_ops > 0
    drs = [mh.DeviceWrite1Requests(r, 0) for r in seq]
    outs = [mh.DeviceWrite1RequestsDecoded(r.n_reqs, h.n_ops + 3, fill=FILL) for r, h in zip(seq, hosts)]
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    s = mh.DeviceSigner(W.load_keys(1)[0], 0)
    torch.cuda.synchronize()
    rcs = [s.request_decode_device(dr, o, stream=st.cuda_stream) for dr, o, st in zip(drs, outs, (a, b, a))]
    torch.cuda.synchronize()
    for rc, o, h in zip(rcs, outs, hosts):
        _assert_decoded(o.to_host(rc), h.trimmed(), h.n_ops, h.n_keys)
    s.close()


def test_profile_reader(signer):
    reqs = QM.batch([_full_req(q) for q in range(40)])
    host = mh.write1_request_decode(reqs)
    signer.set_profiling(True)
    try:
        got = _decode_device(signer, reqs, host.n_ops)
        prof = signer.read_request_profile()
    finally:
        signer.set_profiling(False)
    assert got.rc == mh.OK and tuple(prof) == mh.W1_REQUEST_STAGES
    assert all(v >= 0 for v in prof.values())
    assert all(prof[k] > 0 for k in ("k_w1q_req", "k_w1q_ops", "k_w1q_emit", "k_w1q_claim", "k_w1q_rank", "k_w1q_number"))


# 6. the join ------------------------------------------------------------------------------------------
def _join_device(signer, off, seed, flags, obj, ks, in_place=False):
    import torch

    dev = lambda a, dt: mh._to_dev(np.ascontiguousarray(a, dt), 0)
    O = len(obj)
    s = torch.cuda.Stream()
    d_flags = dev(flags, np.uint8)
    fl = d_flags if in_place else torch.full((O + 1,), FILL, dtype=torch.uint8, device="cuda:0")
    ep = torch.full((O + 1,), -1, dtype=torch.int64, device="cuda:0")
    st = torch.full((O + 1,), 7, dtype=torch.int32, device="cuda:0")
    dk = mh.DeviceWrite1KeyState(ks, 0)
    torch.cuda.synchronize()
    signer.state_join_device(len(off) - 1, O, dev(off, np.uint32), dev(seed, np.uint32), d_flags, dev(obj, np.uint32), dk, fl,
                             ep, st, stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert in_place or int(fl[O]) == FILL
    assert int(ep[O]) == -1 and int(st[O]) == 7  # nothing past n_ops
    return fl.cpu().numpy()[:O], ep.cpu().numpy()[:O], st.cpu().numpy().view(np.uint32)[:O]


@pytest.mark.parametrize("in_place", [False, True])
def test_join_device_equals_host(signer, in_place):
    off, seed, flags, obj, ks, want_stored = QM.join_case()
    got = _join_device(signer, off, seed, flags, obj, ks, in_place)
    for g, h in zip(got, mh.write1_state_join(off, seed, flags, obj, ks)):
        np.testing.assert_array_equal(g, h)
    assert got[2].tolist() == want_stored


def test_join_device_more_than_a_block(signer):
    b = W.make_write1_batch(300, k=3, contention=0.5, stored=0.3)
    dec = mh.write1_request_decode(QM.wire_of_batch(b)[0]).trimmed()
    ks = QM.key_state_of(b, dec["key_op"], dec["op_obj"])
    got = _join_device(signer, dec["req_op_off"], dec["req_seed"], dec["op_flags"], dec["op_obj"], ks)
    for g, h in zip(got, (b.op_flags, b.op_epoch, b.op_stored)):
        np.testing.assert_array_equal(g, h)
    assert (got[2] != mh.W1_NONE).sum() > 50


# 7. the server's round on the device ------------------------------------------------------------------
def test_round_bodies_to_replies_equals_the_soa_batch():
    """Path A: the SoA batch through issue (signed) and reply encode.  Path B: its requests as
    bodies through decode, the host's one lookup per distinct key, join, and the same two
    calls, every device call on one stream with no Python parsing.  The replies are byte-equal."""
    import torch

    Q, K = 96, 3
    b = W.make_write1_batch(Q, k=K, contention=0.4, stored=0.2)
    stored = [b"\x0a\x03old\x10" + RM.varint(5 + i) for i in range(b.n_stored)]
    client_of = lambda q: b"client-%d" % q
    server = W.SERVER_IDS[0].encode()
    src = RM.make_source(b, stored, certs=True, sigs=True, server=server, client_of=client_of)
    signer = mh.DeviceSigner(W.load_keys(1)[0], 0)
    stream = torch.cuda.Stream()
    st = stream.cuda_stream

    def replies(db, ds):
        out = mh.DeviceWrite1Issued(Q, b.n_ops, mh.write1_issue_bound(b) + 64 * b.n_ops, sign=True)
        cap = mh.write1_reply_bound(db, ds, out.grant_cap, True)
        wire = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
        off = torch.zeros(Q, dtype=torch.int64, device="cuda:0")
        ln = torch.zeros(Q, dtype=torch.int32, device="cuda:0")
        status = torch.zeros(Q, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        assert signer.issue_device(db, out, stream=st) == mh.OK
        rc, total = signer.reply_encode_device(db, out, ds, wire, off, ln, status, stream=st)
        torch.cuda.synchronize()
        assert rc == mh.OK and bool((status == 0).all())
        w = wire.cpu().numpy()
        return [w[int(o):int(o) + int(n)].tobytes() for o, n in zip(off.cpu().numpy(), ln.cpu().numpy())], \
            out.req_kind[:Q].cpu().numpy()

    d_src = mh.DeviceWrite1ReplySource(src, 0)
    want, want_kind = replies(mh.DeviceWrite1Batch(b, 0), d_src)

    reqs, sh_off, sh_len = QM.wire_of_batch(b)
    blob = np.concatenate([reqs.wire, np.frombuffer(server, np.uint8)])  # bodies, stored hashes, the server id
    dr = mh.DeviceWrite1Requests(mh.Write1Requests(wire=blob, msg_off=reqs.msg_off, msg_len=reqs.msg_len), 0)
    dec = mh.DeviceWrite1RequestsDecoded(Q, mh.write1_request_decode_bound(blob.size, Q), fill=FILL)
    torch.cuda.synchronize()
    assert signer.request_decode_device(dr, dec, stream=st) == mh.OK
    assert dec.n_ops == b.n_ops
    with torch.cuda.stream(stream):  # the host's part: one store lookup per distinct key
        U = dec.n_keys()
        key_op = dec.key_op[:U].cpu().numpy().view(np.uint32)
        op_obj = dec.op_obj[:b.n_ops].cpu().numpy().view(np.uint32)
    assert U == np.unique(b.op_obj).size and QM.same_partition(op_obj, b.op_obj)
    dk = mh.DeviceWrite1KeyState(QM.key_state_of(b, key_op, op_obj), 0)
    op_epoch = torch.zeros(b.n_ops, dtype=torch.int64, device="cuda:0")
    op_stored = torch.zeros(b.n_ops, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    signer.state_join_device(Q, b.n_ops, dec.req_op_off, dec.req_seed, dec.op_flags, dec.op_obj, dk, dec.op_flags, op_epoch,
                             op_stored, stream=st)
    db = mh.DeviceWrite1Batch.__new__(mh.DeviceWrite1Batch)
    db.n_reqs, db.n_ops, db.n_stored, db.strings_len = Q, b.n_ops, b.n_stored, int(blob.size)
    for k, t in dict(strings=dr.wire, req_op_off=dec.req_op_off, req_seed=dec.req_seed, req_hash_off=dec.req_hash_off,
                     req_hash_len=dec.req_hash_len, op_key_off=dec.op_key_off, op_key_len=dec.op_key_len,
                     op_flags=dec.op_flags, op_obj=dec.op_obj, op_epoch=op_epoch, op_stored=op_stored,
                     stored_hash_off=mh._to_dev(sh_off, 0), stored_hash_len=mh._to_dev(sh_len, 0)).items():
        setattr(db, k, t)
    ds = mh.DeviceWrite1ReplySource.from_tensors(
        int(reqs.wire.size), len(server), ids=dr.wire, req_client_off=dec.req_client_off, req_client_len=dec.req_client_len,
        stored_bytes=d_src.stored_bytes, stored_off=d_src.stored_off, stored_len=d_src.stored_len,
        stored_sig=d_src.stored_sig, certs=d_src.certs, op_cert_off=d_src.op_cert_off, op_cert_len=d_src.op_cert_len)
    got, got_kind = replies(db, ds)
    signer.close()
    assert got_kind.tolist() == want_kind.tolist() and len(set(want_kind.tolist())) >= 2
    assert got == want and sum(map(len, want)) > 256 * Q
