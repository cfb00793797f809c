"""Write1 reply encoder on the GPU (mochi_write1_reply_encode_device): the device
form equals the host form byte for byte on every CPU case set; both capacity
modes; issue -> sign -> reply on one stream with a single synchronise; four
servers' replies assembled into Write2ToServer bodies the verifier accepts;
64-bit offsets; two calls on two streams agree."""
import numpy as np
import pytest

import mochi_hip as mh
import workload as W
import write1_issue_model as M
import write1_reply_model as RM

pytestmark = pytest.mark.gpu

OWN_NAMES = ["ok_empty_no_ids", "ok_empty_ids", "throws", "refused_mixed", "ok_64_ops", "one_key_twice", "stored_shared",
             "cert_alias", "steps", "cert_lens", "alignment"]


@pytest.fixture(scope="module")
def pems():
    return W.load_keys(4)


@pytest.fixture(scope="module")
def signer(pems):
    s = mh.DeviceSigner(pems[0], 0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def own_cases():
    return RM.reply_cases()


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _dev_issued(batch, issued):
    """The host outputs of write1_issue copied into device buffers (what issue_device would have left)."""
    import torch

    sv = {np.uint8: np.uint8, np.uint32: np.int32, np.uint64: np.int64, np.int64: np.int64}
    out = mh.DeviceWrite1Issued(batch.n_reqs, batch.n_ops, int(issued.grant_bytes.size), sign=issued.sig is not None)
    for k, dt in mh._W1_OUT_DTYPES.items():
        a = np.ascontiguousarray(getattr(issued, k), dt).reshape(-1)
        if a.size:
            getattr(out, k)[:a.size].copy_(torch.from_numpy(a.view(sv[dt])))
    if issued.grant_bytes.size:
        out.grant_bytes[:issued.grant_bytes.size].copy_(torch.from_numpy(issued.grant_bytes))
    if issued.sig is not None and issued.n_new:
        out.sig[:issued.n_new].copy_(torch.from_numpy(np.ascontiguousarray(issued.sig)))
    out.n_new, out.grant_bytes_len = issued.n_new, issued.grant_bytes_len
    return out


def _outputs(Q, cap, fill=0xEE):
    import torch

    dev = torch.device("cuda", 0)
    return (torch.full((max(cap, 1),), fill, dtype=torch.uint8, device=dev),
            torch.full((max(Q, 1),), -1, dtype=torch.int64, device=dev),
            torch.full((max(Q, 1),), -1, dtype=torch.int32, device=dev),
            torch.full((max(Q, 1),), 0xEE, dtype=torch.uint8, device=dev))


def _host(case):
    wire, off, ln, st = mh.write1_reply_encode(*case)
    return wire, off, ln, st


def _assert_same(host, dev_out, Q, extra_untouched=True):
    hwire, hoff, hln, hst = host
    wire, off, ln, st = dev_out
    n = hwire.size
    w = wire.cpu().numpy()
    assert w[:n].tobytes() == hwire.tobytes()
    if extra_untouched:
        assert (w[n:] == 0xEE).all()  # bytes outside the written range are untouched
    np.testing.assert_array_equal(off.cpu().numpy().view(np.uint64)[:Q], hoff)
    np.testing.assert_array_equal(ln.cpu().numpy().view(np.uint32)[:Q], hln)
    np.testing.assert_array_equal(st.cpu().numpy()[:Q], hst)


def _device_equals_host(signer, case):
    import torch

    batch, issued, src = case
    host = _host(case)
    need = host[0].size
    db, do, ds = mh.DeviceWrite1Batch(batch, 0), _dev_issued(batch, issued), mh.DeviceWrite1ReplySource(src, 0)
    outs = _outputs(batch.n_reqs, need + 64)
    rc, n = signer.reply_encode_device(db, do, ds, *outs, stream=_stream())
    torch.cuda.synchronize()
    assert rc == mh.OK and n == need
    _assert_same(host, outs, batch.n_reqs)
    return db, do, ds, host


# 1. device == host on every CPU case set ------------------------------------------------
@pytest.mark.parametrize("name", OWN_NAMES)
def test_device_form_equals_host_form(signer, own_cases, name):
    _device_equals_host(signer, own_cases[name])


@pytest.mark.parametrize("sigs", [True, False], ids=["sig", "nosig"])
@pytest.mark.parametrize("certs", [True, False], ids=["certs", "nocerts"])
def test_device_form_equals_host_form_on_the_issue_cases(signer, certs, sigs):
    for name, case in RM.issue_cases(certs, sigs).items():
        _device_equals_host(signer, case)


def test_alignment_set_covers_every_residue_pair(own_cases):
    runs = RM.encode(*own_cases["alignment"]).runs
    assert len(RM.residues(runs, ("cert",))) == 256 and len(RM.residues(runs, ("grant",))) == 256


# 2. the single-block scan line -----------------------------------------------------------
def _plain_case(n, k=1, sigs=True):
    batch = W.write1_batch(np.arange(n * k), np.arange(n + 1) * k, np.full(n, 3), np.arange(n))
    return batch, RM.issue(batch, sigs), RM.make_source(batch, [], certs=True, sigs=sigs)


@pytest.mark.parametrize("n", [1023, 1024, 1025])
def test_scan_line(signer, n):
    _device_equals_host(signer, _plain_case(n))


# 3. capacity, mode 1: the host waits for the total ------------------------------------------
def test_one_byte_short_with_a_host_wait(signer, own_cases):
    import torch

    case = own_cases["refused_mixed"]
    batch = case[0]
    db, do, ds, host = _device_equals_host(signer, case)
    need = host[0].size
    outs = _outputs(batch.n_reqs, need - 1)
    rc, n = signer.reply_encode_device(db, do, ds, *outs, stream=_stream(), check=False)
    torch.cuda.synchronize()
    assert rc == mh.EINVAL and n == need and bool((outs[0] == 0xEE).all())
    rc, n = signer.reply_encode_device(db, do, ds, None, *outs[1:], stream=_stream(), check=False)  # the size alone
    assert rc == mh.EINVAL and n == need


# 4. capacity, mode 2: no host wait -----------------------------------------------------------
@pytest.mark.parametrize("name", ["refused_mixed", "cert_lens", "alignment"])
def test_device_side_capacity_rule(signer, own_cases, name):
    import torch

    case = own_cases[name]
    batch = case[0]
    db, do, ds, host = _device_equals_host(signer, case)
    need = host[0].size
    total = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
    outs = _outputs(batch.n_reqs, need + 64)
    rc, n = signer.reply_encode_device(db, do, ds, *outs, stream=_stream(), wire_len_dev=total)
    torch.cuda.synchronize()
    assert rc == mh.OK and n is None and int(total.item()) == need
    _assert_same(host, outs, batch.n_reqs)
    total.fill_(-1)
    outs = _outputs(batch.n_reqs, need - 1)
    rc, n = signer.reply_encode_device(db, do, ds, *outs, stream=_stream(), wire_len_dev=total)
    torch.cuda.synchronize()
    assert rc == mh.OK and int(total.item()) == need
    assert bool((outs[0] == 0xEE).all())  # all or nothing
    np.testing.assert_array_equal(outs[2].cpu().numpy().view(np.uint32)[:batch.n_reqs], host[2])
    np.testing.assert_array_equal(outs[1].cpu().numpy().view(np.uint64)[:batch.n_reqs], host[1])
    np.testing.assert_array_equal(outs[3].cpu().numpy()[:batch.n_reqs], host[3])


# 5. issue -> sign -> reply bytes as one enqueue ------------------------------------------------
def _issue_and_reply(signer, batch, src, stream, reply_stream=None):
    """issue_device(sign) on `stream`, then the reply encoder in mode 2 on `reply_stream` (default: the same), nothing
    in between."""
    import torch

    db, ds = mh.DeviceWrite1Batch(batch, 0), mh.DeviceWrite1ReplySource(src, 0)
    out = mh.DeviceWrite1Issued(batch.n_reqs, batch.n_ops, mh.write1_issue_bound(batch), sign=True)
    cap = mh.write1_reply_bound(batch, src, out.grant_cap, True)  # sized before anything is known
    outs = _outputs(batch.n_reqs, cap)
    total = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
    if reply_stream is not None:
        torch.cuda.synchronize()  # the uploads and fills above went to the current stream
    assert signer.issue_device(db, out, stream=stream) == mh.OK
    rc, _ = signer.reply_encode_device(db, out, ds, *outs, wire_len_dev=total,
                                       stream=stream if reply_stream is None else reply_stream)
    assert rc == mh.OK
    return out, outs, total


def _bodies(outs, total, Q):
    wire, off, ln, st = outs
    n = int(total.item())
    w = wire[:n].cpu().numpy()
    off, ln = off.cpu().numpy().view(np.uint64), ln.cpu().numpy().view(np.uint32)
    assert bool((st[:Q] == 0).all()) and n == int(ln[:Q].sum())
    return [w[int(off[q]):int(off[q]) + int(ln[q])].tobytes() for q in range(Q)]


def _chained_case(pems):
    batch = W.make_write1_batch(300, 2, contention=0.3)
    stored = [b"\x0a\x03old\x10%c" % (i % 100 + 1) for i in range(batch.n_stored)]  # grants given before the batch
    src = RM.make_source(batch, stored, certs=True, sigs=False)
    src.stored_sig = mh.sign_grants(pems[0], *RM.pack(stored))
    return batch, src


def test_chained_issue_sign_reply_without_synchronisation(pems, signer):
    pytest.importorskip("google.protobuf")
    import torch

    Reply, Grant = RM.classes()
    batch, src = _chained_case(pems)
    host = mh.write1_issue(batch)
    out, outs, total = _issue_and_reply(signer, batch, src, _stream())
    torch.cuda.synchronize()  # the only one
    got = out.to_host()
    assert got.n_new == host.n_new and signer.rejected() == 0
    bodies = _bodies(outs, total, batch.n_reqs)
    # the same bytes as the host form over the downloaded issue outputs
    want, _, _, _ = mh.write1_reply_encode(batch, got, src)
    assert b"".join(bodies) == want.tobytes()
    pairs = []  # (grant bytes, the signature beside them)
    for q, body in enumerate(bodies):
        m = Reply()
        m.ParseFromString(body)
        assert m.HasField("multiGrant") and m.multiGrant.serverId.encode() == RM.SERVER_ID
        assert set(m.multiGrant.grants) == set(m.multiGrant.grantSignatures)
        pairs += [(g.SerializeToString(), m.multiGrant.grantSignatures[oid]) for oid, g in m.multiGrant.grants.items()]
    assert set(got.req_kind.tolist()) == {mh.W1K_OK, mh.W1K_REFUSED} and len(pairs) >= 500
    cpu = mh.sign_grants(pems[0], *RM.pack([gb for gb, _ in pairs]))  # one call: the CPU signer over every grant
    for i, (gb, sig) in enumerate(pairs):
        assert sig == cpu[i].tobytes(), i


def test_issue_and_reply_on_different_streams(pems, signer):
    """The reply call reads what the issue call's kernels are still writing: only the signer's scratch order (one for
    both calls) makes stream B wait for stream A."""
    import torch

    batch, src = _chained_case(pems)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    out, outs, total = _issue_and_reply(signer, batch, src, a.cuda_stream, b.cuda_stream)
    torch.cuda.synchronize()  # the only one after the two calls
    got = out.to_host()
    want, _, _, _ = mh.write1_reply_encode(batch, got, src)
    assert b"".join(_bodies(outs, total, batch.n_reqs)) == want.tobytes()
    assert signer.rejected() == 0


# 6. four servers' replies become Write2ToServer bodies the verifier accepts -----------------------
def test_four_servers_replies_feed_the_write2_verifier(pems):
    pytest.importorskip("google.protobuf")
    import torch

    Reply, Grant = RM.classes()
    R, Q, K = 4, 8, 2
    n_ops = Q * K
    batch = W.write1_batch(np.arange(n_ops), np.arange(Q + 1) * K, np.full(Q, 6), np.arange(Q))
    mgs = [[] for _ in range(Q)]  # per request: (server id, MultiGrant bytes) of every server
    for s in range(R):
        sid = W.SERVER_IDS[s].encode()
        src = RM.make_source(batch, [], certs=True, sigs=True, server=sid, client_of=lambda q: b"")
        signer = mh.DeviceSigner(pems[s], 0)
        out, outs, total = _issue_and_reply(signer, batch, src, _stream())
        torch.cuda.synchronize()
        signer.close()
        for q, body in enumerate(_bodies(outs, total, Q)):
            m = Reply()
            m.ParseFromString(body)
            assert m.multiGrant.serverId.encode() == sid and len(m.multiGrant.grants) == K
            # the MultiGrant's own bytes: field 1 of the reply (0A, a length below 2^14, the body)
            assert body[0] == 0x0A
            n = body[1] & 0x7F | (body[2] & 0x7F) << 7 if body[1] & 0x80 else body[1]
            at = 3 if body[1] & 0x80 else 2
            raw = body[at:at + n]
            assert raw == m.multiGrant.SerializeToString(deterministic=True) or len(raw) == m.multiGrant.ByteSize()
            mgs[q].append((W.SERVER_IDS[s], raw))
    strings = np.asarray(batch.strings, np.uint8)
    key = lambda o: strings[int(batch.op_key_off[o]):][:int(batch.op_key_len[o])].tobytes().decode()
    msgs = [W.encode_write2(mgs[q], [W.encode_operation(M.WRITE, key(q * K + j), "v") for j in range(K)]) for q in range(Q)]
    ln = np.array([len(x) for x in msgs], np.uint32)
    h0 = int(batch.req_hash_off[0])
    wb = W.WireBatch(wire=np.frombuffer(b"".join(msgs), np.uint8).copy(),
                     msg_off=np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.uint64), msg_len=ln,
                     op_flags_off=batch.req_op_off.astype(np.uint32),
                     op_flags=np.full(n_ops, mh.OP_LOCAL | mh.OP_HAS_SVOC, np.uint8),
                     expected_hash=strings[h0:h0 + Q * mh.TXN_HASH_BYTES].reshape(Q, mh.TXN_HASH_BYTES).copy())
    ver = mh.Verifier([mh.pem_modulus(p) for p in pems], 0)
    ver.set_server_ids(W.SERVER_IDS[:R])
    v, status = ver.verify_write2(wb, R, True)
    ver.close()
    assert (status == mh.MSG_OK).all()
    assert mh.unpack_bits(v.cert_accept_bits, Q).all() and (v.cert_reason == 0).all()


# 7. 64-bit offsets ---------------------------------------------------------------------------
def test_offsets_past_4_gib(signer):
    """Every request's op points at one aliased 16 KiB certificate, so the inputs
    stay small while the wire passes 2^32 bytes.  Only offsets, lengths and the
    first and last few messages come to the host."""
    import torch

    cert_len = 16384
    n = (1 << 32) // (cert_len + 100) + 64
    batch = W.write1_batch(np.arange(n), np.arange(n + 1), np.full(n, 3), np.arange(n) % 7)
    dev = torch.device("cuda", 0)
    cert = np.frombuffer((b"certificate-bytes" * 1000)[:cert_len], np.uint8).copy()
    src = mh.Write1ReplySource(ids=np.frombuffer(RM.SERVER_ID, np.uint8).copy(), server_id_off=0, server_id_len=len(RM.SERVER_ID),
                               req_client_off=None, req_client_len=None, stored_bytes=np.zeros(1, np.uint8),
                               stored_off=np.zeros(0, np.uint64), stored_len=np.zeros(0, np.uint32), stored_sig=None,
                               certs=cert, op_cert_off=np.zeros(n, np.uint64), op_cert_len=np.full(n, cert_len, np.uint32))
    db, ds = mh.DeviceWrite1Batch(batch, 0), mh.DeviceWrite1ReplySource(src, 0)
    out = mh.DeviceWrite1Issued(n, n, 192 * n)  # a grant here is about 150 bytes
    assert signer.issue_device(db, out, stream=_stream()) == mh.OK
    rc, need = signer.reply_encode_device(db, out, ds, None, *_outputs(n, 0)[1:], stream=_stream(), check=False)
    assert rc == mh.EINVAL and need > 1 << 32
    wire, off, ln, st = _outputs(n, need, fill=0)
    rc, got = signer.reply_encode_device(db, out, ds, wire, off, ln, st, stream=_stream())
    torch.cuda.synchronize()
    assert got == need and bool((st == 0).all()) and out.n_new == n
    h_off, h_ln = off.cpu().numpy().view(np.uint64), ln.cpu().numpy().view(np.uint32)
    want_off = np.zeros(n, np.uint64)
    np.cumsum(h_ln[:-1].astype(np.uint64), out=want_off[1:])
    np.testing.assert_array_equal(h_off, want_off)
    assert int(h_off[-1]) > 1 << 32 and int(h_off[-1]) + int(h_ln[-1]) == need
    # the first and last requests alone through the host form give the same bodies
    grants = out.to_host()
    strings = np.asarray(batch.strings, np.uint8)
    for q in list(range(4)) + list(range(n - 4, n)):
        key = strings[int(batch.op_key_off[q]):][:int(batch.op_key_len[q])].tobytes()
        body = (RM.ld(0x0A, RM.ld(0x0A, RM.ld(0x0A, key) + RM.ld(0x12, grants.grant(q))) + RM.ld(0x22, RM.SERVER_ID)) +
                RM.ld(0x12, RM.ld(0x0A, key) + RM.ld(0x12, cert.tobytes())))
        o = int(h_off[q])
        assert int(h_ln[q]) == len(body), q
        assert wire[o:o + len(body)].cpu().numpy().tobytes() == body, q


# 8. repeatability and the profile ---------------------------------------------------------------
def test_two_streams_give_equal_bytes(signer, own_cases):
    import torch

    case = own_cases["alignment"]
    batch, issued, src = case
    host = _host(case)
    db, do, ds = mh.DeviceWrite1Batch(batch, 0), _dev_issued(batch, issued), mh.DeviceWrite1ReplySource(src, 0)
    outs = [_outputs(batch.n_reqs, host[0].size + 64) for _ in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for o, s in zip(outs, streams):
        rc, n = signer.reply_encode_device(db, do, ds, *o, stream=s.cuda_stream)
        assert n == host[0].size
    torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    _assert_same(host, outs[0], batch.n_reqs)


def test_per_kernel_profile(signer, own_cases):
    import torch

    case = own_cases["cert_lens"]
    batch, issued, src = case
    db, do, ds = mh.DeviceWrite1Batch(batch, 0), _dev_issued(batch, issued), mh.DeviceWrite1ReplySource(src, 0)
    outs = _outputs(batch.n_reqs, _host(case)[0].size)
    signer.reply_encode_device(db, do, ds, *outs, stream=_stream())
    with pytest.raises(mh.MochiError):  # that call was not profiled
        signer.read_reply_profile()
    signer.set_profiling(True)
    signer.reply_encode_device(db, do, ds, *outs, stream=_stream())
    signer.set_profiling(False)
    ms = signer.read_reply_profile()
    torch.cuda.synchronize()
    assert list(ms) == list(mh.W1_REPLY_STAGES)
    assert all(0 <= v < 1000 for v in ms.values()) and ms["k_w1r_copy"] > 0
