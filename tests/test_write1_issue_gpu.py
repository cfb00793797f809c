"""Write1 grant issuance on the GPU (mochi_write1_issue_device): the device form
equals the host form array for array on every CPU case set and at the shapes
where its kernels change path; signatures equal the CPU signer's; the new grants
and signatures of four servers go through the Write2 encoder and verifier without
a host round trip; two calls on two streams agree."""
import numpy as np
import pytest

import mochi_hip as mh
import oracle_ffi as O
import workload as W
import write1_issue_model as M

pytestmark = pytest.mark.gpu

ARRAYS = ("op_decision", "op_grant", "req_kind", "req_grant_off", "req_grant", "grant_off", "grant_len", "grant_op",
          "grant_ts")


@pytest.fixture(scope="module")
def pems():
    return W.load_keys(4)


@pytest.fixture(scope="module")
def signer(pems):
    s = mh.DeviceSigner(pems[0], 0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name, (store, reqs, pad) in M.all_cases().items():
        M.prepare(store, reqs)
        out[name] = M.build_batch(store, reqs, pad)
    return out


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _issue(signer, batch, host, extra=64, sign=False, stream=None):
    import torch

    out = mh.DeviceWrite1Issued(batch.n_reqs, batch.n_ops, host.grant_bytes_len + extra, sign=sign, fill=0xEE)
    rc = signer.issue_device(mh.DeviceWrite1Batch(batch, 0), out, stream=_stream() if stream is None else stream)
    torch.cuda.synchronize()
    assert rc == mh.OK
    return out


def _assert_same(host, out):
    got = out.to_host()
    assert got.n_new == host.n_new and got.grant_bytes_len == host.grant_bytes_len
    for k in ARRAYS:
        np.testing.assert_array_equal(getattr(got, k), getattr(host, k), err_msg=k)
    n = host.grant_bytes_len
    assert got.grant_bytes[:n].tobytes() == host.grant_bytes[:n].tobytes()
    assert (got.grant_bytes[n:] == 0xEE).all()  # bytes outside the written range are untouched
    return got


CASE_NAMES = sorted(M.hand_cases()) + sorted(M.edge_cases()) + [f"random{i}" for i in range(6)] + ["alignment"]


# 1. device == host on every CPU case set -------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_device_form_equals_host_form(signer, cases, name):
    import torch

    batch = cases[name]
    host = mh.write1_issue(batch)
    _assert_same(host, _issue(signer, batch, host))
    if host.grant_bytes_len:  # one byte short: refused, the size reported, no grant byte written
        out = mh.DeviceWrite1Issued(batch.n_reqs, batch.n_ops, host.grant_bytes_len - 1, fill=0xEE)
        rc = signer.issue_device(mh.DeviceWrite1Batch(batch, 0), out, stream=_stream())
        torch.cuda.synchronize()
        assert rc == mh.EINVAL and out.grant_bytes_len == host.grant_bytes_len and out.n_new == host.n_new
        assert bool((out.grant_bytes == 0xEE).all())
        got = out.to_host(rc)
        for k in ("op_decision", "req_kind", "req_grant_off"):
            np.testing.assert_array_equal(getattr(got, k), getattr(host, k), err_msg=k)


def test_alignment_set_covers_every_residue_pair(cases):
    host = mh.write1_issue(cases["alignment"])
    assert len(M.payload_residues(cases["alignment"], host)) == 256


# 2. contention on one slot ------------------------------------------------------
def test_one_slot_under_4096_requests(signer):
    """atomicMin contention: op 0 is NEW, same-hash ops RETRY, the others REFUSED."""
    n = 4096
    batch = W.write1_batch(np.full(n, 5), np.arange(n + 1), np.full(n, 9), np.arange(n) % 3)
    host = mh.write1_issue(batch)
    got = _assert_same(host, _issue(signer, batch, host))
    want = np.where(np.arange(n) % 3 == 0, mh.W1D_RETRY, mh.W1D_REFUSED).astype(np.uint8)
    want[0] = mh.W1D_NEW
    np.testing.assert_array_equal(got.op_decision, want)
    assert got.n_new == 1 and (got.op_grant == 0).all() and (got.req_grant == 0).all()
    np.testing.assert_array_equal(got.req_grant_off, np.arange(n + 1))
    assert got.grant_op.tolist() == [0] and got.grant_ts.tolist() == [5000 + 9]


# 3. distinct slots around the table-capacity doubling and the scan's small-batch line ---
@pytest.mark.parametrize("pattern", ["sequential", "strided", "seeds"])
@pytest.mark.parametrize("n", [1023, 1024, 1025])
def test_distinct_slots(signer, n, pattern):
    """Sequential, 2^20-strided and all-equal object indices (distinct seeds):
    whatever the table's hash, long probe runs are met."""
    i = np.arange(n)
    obj = {"sequential": i, "strided": i << 20, "seeds": np.full(n, 77)}[pattern]
    seeds = i * 3 if pattern == "seeds" else np.full(n, 4)
    batch = W.write1_batch(obj, np.arange(n + 1), seeds, i)
    host = mh.write1_issue(batch)
    got = _assert_same(host, _issue(signer, batch, host))
    assert (got.op_decision == mh.W1D_NEW).all() and (got.req_kind == mh.W1K_OK).all()
    np.testing.assert_array_equal(got.op_grant, i)
    np.testing.assert_array_equal(got.grant_ts, 1000 * (obj % 64) + seeds)


def test_contended_workload_batch(signer):
    """The generator's mix (contended slots, retries, stored grants) above the small-batch line."""
    batch = W.make_write1_batch(1500, 2, contention=0.3)
    host = mh.write1_issue(batch)
    got = _assert_same(host, _issue(signer, batch, host))
    assert {mh.W1D_NEW, mh.W1D_RETRY, mh.W1D_REFUSED} <= set(got.op_decision.tolist())
    assert (got.op_grant >= mh.W1_STORED).any() and set(got.req_kind.tolist()) == {mh.W1K_OK, mh.W1K_REFUSED}


# 4. signatures ----------------------------------------------------------------------
def test_signatures_equal_the_cpu_signer(pems):
    n = 512
    batch = W.write1_batch(np.arange(n), np.arange(n + 1), np.full(n, 3), np.arange(n))
    host = mh.write1_issue(batch)
    assert host.n_new == n
    unsigned = None
    for pem in pems[:2]:
        s = mh.DeviceSigner(pem, 0)
        got = _assert_same(host, _issue(s, batch, host, sign=True))
        if unsigned is None:  # with sig NULL nothing is signed and the other outputs are unchanged
            unsigned = _assert_same(host, _issue(s, batch, host, sign=False))
            assert unsigned.sig is None
        assert s.rejected() == 0
        s.close()
        want = mh.sign_grants(pem, host.grant_bytes, host.grant_off, host.grant_len)
        np.testing.assert_array_equal(got.sig, want)
        n_be = mh.pem_modulus(pem)
        for g in range(n):
            assert O.rsa_verify(n_be, host.grant(g), got.sig[g].tobytes()), g


# 5. the chain: issue -> encode -> verify, nothing through the host but sizes ------------
def _chain(pems, conflict):
    import torch

    R, Q, K = 4, 8, 2
    n_ops = Q * K
    dev = torch.device("cuda", 0)
    ver = mh.Verifier([mh.pem_modulus(p) for p in pems], 0)
    ver.set_server_ids(W.SERVER_IDS[:R])
    plain = W.write1_batch(np.arange(n_ops), np.arange(Q + 1) * K, np.full(Q, 6), np.arange(Q))
    # server 3 gave the slot of request 5's first op to another transaction before the batch
    stored = np.full(n_ops, mh.W1_NONE, np.uint32)
    stored[5 * K] = 0
    other = W.write1_batch(np.arange(n_ops), np.arange(Q + 1) * K, np.full(Q, 6), np.arange(Q), op_stored=stored,
                           stored_hash_id=[999])
    outs, dbatches = [], []
    for s in range(R):
        b = other if conflict and s == 3 else plain
        signer = mh.DeviceSigner(pems[s], 0)
        out = mh.DeviceWrite1Issued(Q, n_ops, mh.write1_issue_bound(b), sign=True)
        db = mh.DeviceWrite1Batch(b, 0)
        assert signer.issue_device(db, out, stream=_stream()) == mh.OK
        torch.cuda.synchronize()
        signer.close()
        outs.append(out)
        dbatches.append(db)
    # which new grant of server s is op o's (known from how the batches were built)
    op_to_grant = [np.arange(n_ops) for _ in range(R)]
    members = [[0, 1, 2, 3] for _ in range(Q)]
    if conflict:
        op_to_grant[3] = np.where(np.arange(n_ops) > 5 * K, np.arange(n_ops) - 1, np.arange(n_ops))
        members[5] = [0, 1, 2]  # server 3 answered REFUSED: the client holds three MultiGrants
        assert outs[3].n_new == n_ops - 1
    base = np.concatenate([[0], np.cumsum([o.n_new for o in outs])])[:R]
    pick = torch.tensor([base[s] + op_to_grant[s][m * K + j] for m in range(Q) for s in members[m] for j in range(K)],
                        dtype=torch.int64, device=dev)
    byte_base = np.concatenate([[0], np.cumsum([o.grant_bytes_len for o in outs])])
    grant_off = torch.cat([o.grant_off[:o.n_new] + int(byte_base[s]) for s, o in enumerate(outs)])[pick]
    grant_len = torch.cat([o.grant_len[:o.n_new] for o in outs])[pick]
    sig = torch.cat([o.sig[:o.n_new] for o in outs])[pick].contiguous()
    n_mgs = sum(len(x) for x in members)
    i32 = lambda a: torch.from_numpy(np.asarray(a, np.uint32).view(np.int32)).to(dev)
    d0 = dbatches[0]
    src = mh.DeviceWrite2Source.from_tensors(
        Q, n_mgs, n_mgs * K, n_ops,
        grant_bytes=torch.cat([o.grant_bytes[:o.grant_bytes_len] for o in outs]), grant_off=grant_off.contiguous(),
        grant_len=grant_len.contiguous(), sig=sig,
        cert_mg_off=i32(np.concatenate([[0], np.cumsum([len(x) for x in members])])),
        mg_grant_off=i32(np.arange(n_mgs + 1) * K),
        mg_signer=torch.tensor([s for x in members for s in x], dtype=torch.int16, device=dev),
        strings=d0.strings, cert_op_off=d0.req_op_off,
        op_action=torch.full((n_ops,), M.WRITE, dtype=torch.uint8, device=dev),
        op1_off=d0.op_key_off, op1_len=d0.op_key_len)
    off = torch.zeros(Q, dtype=torch.int64, device=dev)
    ln = torch.zeros(Q, dtype=torch.int32, device=dev)
    st = torch.zeros(Q, dtype=torch.uint8, device=dev)
    rc, cap = ver.encode_write2_device(src, None, off, ln, st, stream=_stream(), check=False)  # the size
    assert rc == mh.EINVAL and cap > 0
    wire = torch.zeros(cap, dtype=torch.uint8, device=dev)
    ver.encode_write2_device(src, wire, off, ln, st, stream=_stream())
    h0 = int(plain.req_hash_off[0])
    expected = d0.strings[h0:h0 + Q * mh.TXN_HASH_BYTES]  # the request hashes, contiguous in the generator's blob
    dwb = mh.DeviceWireBatch.from_encoded(wire, off, ln, Q, expected, d0.req_op_off,
                                          np.full(n_ops, mh.OP_LOCAL | mh.OP_HAS_SVOC, np.uint8))
    verdicts = mh.DeviceVerdicts(0, Q, 0, full=True, n_ops=n_ops)
    ver.verify_write2_device(dwb, verdicts, R, True, stream=_stream())
    torch.cuda.synchronize()
    assert bool((st == 0).all()) and bool((dwb.status[:Q] == 0).all())
    v = verdicts.to_host()
    ver.close()
    return outs, mh.unpack_bits(v.cert_accept_bits, Q), v.cert_reason


def test_chain_every_certificate_is_accepted(pems):
    outs, accept, reason = _chain(pems, conflict=False)
    assert accept.all() and (reason == 0).all()
    for o in outs:
        h = o.to_host()
        assert (h.req_kind == mh.W1K_OK).all() and (h.op_decision == mh.W1D_NEW).all()


def test_chain_a_refusing_server_leaves_the_certificate_below_quorum(pems):
    outs, accept, reason = _chain(pems, conflict=True)
    h = outs[3].to_host()
    assert h.req_kind.tolist() == [mh.W1K_OK] * 5 + [mh.W1K_REFUSED] + [mh.W1K_OK] * 2
    assert h.op_decision[10] == mh.W1D_REFUSED and h.op_grant[10] == mh.W1_STORED | 0
    assert h.req_grant[int(h.req_grant_off[5]):int(h.req_grant_off[6])].tolist() == [mh.W1_STORED | 0]
    assert accept.tolist() == [True] * 5 + [False] + [True] * 2
    assert reason[5] == 3 and (np.delete(reason, 5) == 0).all()  # MOCHI_REJECT_BELOW_QUORUM


# 6. repeatability and the profile ---------------------------------------------------
def test_two_streams_give_equal_outputs(signer):
    import torch

    batch = W.make_write1_batch(1100, 2, contention=0.3)
    host = mh.write1_issue(batch)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    db = mh.DeviceWrite1Batch(batch, 0)
    outs = [mh.DeviceWrite1Issued(batch.n_reqs, batch.n_ops, host.grant_bytes_len + 64, sign=True, fill=0xEE)
            for _ in streams]
    for out, s in zip(outs, streams):
        assert signer.issue_device(db, out, stream=s.cuda_stream) == mh.OK
    torch.cuda.synchronize()
    a, b = (_assert_same(host, o) for o in outs)
    np.testing.assert_array_equal(a.sig, b.sig)
    assert a.sig.any()


def test_per_kernel_profile(signer, cases):
    batch = cases["random0"]
    host = mh.write1_issue(batch)
    _issue(signer, batch, host)
    with pytest.raises(mh.MochiError):  # that call was not profiled
        signer.read_issue_profile()
    signer.set_profiling(True)
    _issue(signer, batch, host, sign=True)
    signer.set_profiling(False)
    ms = signer.read_issue_profile()
    assert list(ms) == list(mh.W1_ISSUE_STAGES)
    assert all(0 <= v < 1000 for v in ms.values()) and ms["k_w1_emit"] > 0 and ms["sign"] > 0
