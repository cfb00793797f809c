"""Result reply decoder and coalescing step on the GPU (mochi_result_reply_decode_device,
mochi_result_coalesce_device): the device form equals the host form array for array on
the named cases, the mutation corpus and the corpus in aliased, unaligned slices, into
guard-filled outputs with descending, non-dense slot runs; response counts around the
block edges with one request owning everything and with one request per response; n_ops
0 / 1 / 64 against wire counts one below, at, one above and 65; operation totals around
the launch edges of the grid-stride level and one entry past its block cap; two streams;
scratch that grows and shrinks; the profile; and the closing round on one stream with no
synchronise between its three calls, against the plain-Python client."""
import numpy as np
import pytest

import mochi_hip as mh
import result_reply_model as M
import workload as W

pytestmark = pytest.mark.gpu

OK, MAL, FB = mh.RRS_OK, mh.RRS_MALFORMED, mh.RRS_FALLBACK
FILL = M.FILL


@pytest.fixture(scope="module")
def ver():
    v = mh.Verifier([mh.pem_modulus(p) for p in W.load_keys(4)], 0)
    yield v
    v.close()


def _decode_device(ver, r, n_slots, stream=None):
    import torch

    s = stream or torch.cuda.Stream()
    dr = mh.DeviceResultReplies(r, 0)
    out = mh.DeviceResultDecoded(r.n_resps, n_slots, fill=FILL)
    torch.cuda.synchronize()  # uploads and fills went to the current stream
    ver.result_reply_decode_device(dr, out, stream=s.cuda_stream)
    torch.cuda.synchronize()
    return out.to_host()


def _device_equals_host(ver, r, model=False, what=""):
    """Outputs prefilled with FILL in both forms: equal arrays also mean equal untouched bytes."""
    n = M.n_slots(r)
    host = mh.result_reply_decode(r, n, fill=FILL)
    got = _decode_device(ver, r, n)
    M.assert_equal(got, host, what)
    if model:
        M.assert_equal(got, M.decode(r, n), what)
    return got


def _case(name):
    return next(c for c in M.own_cases() if c.name == name)


# 1. device == host == model ---------------------------------------------------------------
@pytest.mark.parametrize("slots", ["dense", "guarded"])
def test_named_cases_device_equals_host(ver, slots):
    got = _device_equals_host(ver, M.batch(M.own_cases(), slots=slots), model=True)
    assert set(got["resp_status"].tolist()) == {OK, MAL, FB}


def test_each_named_case_alone(ver):
    """The cases whose verdict comes from a level of its own, each as a batch of one response."""
    for name in ("empty", "count:n_plus_1_bad_cert", "count:64_last_bad", "count:65_one_bad", "cert:twice", "kind:other"):
        c = _case(name)
        _device_equals_host(ver, M.batch([c], lead=len(name) % 5), model=True, what=name)


def test_corpus_device_equals_host(ver):
    got = _device_equals_host(ver, M.batch(M.corpus(), slots="guarded"), model=True)
    st = got["resp_status"].tolist()
    assert min(st.count(OK), st.count(MAL), st.count(FB)) >= 50


def test_corpus_in_aliased_unaligned_slices(ver):
    cases = M.corpus()
    r = M.batch(cases + cases[::-1], layout="aliased", slots="guarded")
    assert len({int(o) & 3 for o in r.resp_off}) == 4 and len(set(r.resp_off.tolist())) < r.n_resps
    _device_equals_host(ver, r)


# 2. the launch edges of the per-response kernels ------------------------------------------
@pytest.mark.parametrize("grouping", ["each", "one"])
@pytest.mark.parametrize("P", [0, 1, 255, 256, 257])
def test_response_counts_around_the_launch_edges(ver, P, grouping):
    pool = [c for c in M.own_cases() + M.corpus() if not c.name.startswith("cut:")]
    cases = [pool[(7 * i) % len(pool)] for i in range(P)]
    _device_equals_host(ver, M.batch(cases, grouping=grouping, slots="guarded", n_ops=2), model=P <= 257)


def test_empty_batch_touches_nothing(ver):
    import torch

    r = M.batch([])
    out = mh.DeviceResultDecoded(0, 4, fill=FILL)
    ver.result_reply_decode_device(mh.DeviceResultReplies(r, 0), out)
    torch.cuda.synchronize()
    assert all((v.view(np.uint8) == FILL).all() for v in out.to_host().values())


# 3. n_ops against the wire count ------------------------------------------------------------
def _counted(k, n, full):
    ops = [M.op_result(j & 1, b"r%d" % j, j % 3 == 0, M.cert() if full and j % 8 == 0 else None) for j in range(n)]
    return M.Case("k%d:n%d" % (k, n), M.RD if n & 1 else M.W2, M.answer(M.RD if n & 1 else M.W2, ops, b"rid", b"nonce"), k)


@pytest.mark.parametrize("k", [0, 1, 64])
def test_n_ops_against_wire_counts(ver, k):
    cases = [_counted(k, n, full) for n in sorted({max(k - 1, 0), k, k + 1, 65}) for full in (False, True)]
    got = _device_equals_host(ver, M.batch(cases, slots="guarded"), model=True)
    assert sorted(set(got["resp_n_ops"].tolist())) == sorted({max(k - 1, 0), k, k + 1, 65})
    _device_equals_host(ver, M.batch(cases, grouping="one", n_ops=k), model=True)


def test_malformed_operations_reset_the_whole_response(ver):
    """A MALFORMED operation past n_ops, and a MALFORMED last operation beside 63 good ones (which
    other lanes have written by then): every slot of the response reads absent."""
    cases = [_case("count:n_plus_1_bad_cert"), _case("full:write2"), _case("count:64_last_bad"), _case("count:64_certs")]
    r = M.batch(cases, slots="guarded")
    got = _device_equals_host(ver, r, model=True)
    assert got["resp_status"].tolist() == [MAL, OK, MAL, OK] and got["resp_n_ops"].tolist() == [mh.RR_UNDECODED, 2, mh.RR_UNDECODED, 64]
    for p, k in ((0, 2), (2, 64)):
        s = int(r.slot_off[p])
        assert got["op_status"][s:s + k].tolist() == [0xFF] * k
        for nm in ("op_existed", "op_flags", "op_result_off", "op_result_len", "op_cert_off", "op_cert_len"):
            assert not got[nm][s:s + k].any(), nm
    s = int(r.slot_off[3])
    assert got["op_flags"][s:s + 64].tolist() == [mh.RRO_HAS_CERT] * 64


def test_a_certificate_that_ends_the_wire(ver):
    c = M.Case("end", M.W2, M.answer(M.W2, [M.WS, M.op_result(0, b"v", False, M.cert(2, 4, True))]), 2)
    r = M.batch([c], lead=1, tail=0)
    got = _device_equals_host(ver, r, model=True)
    assert int(got["op_cert_off"][1]) + int(got["op_cert_len"][1]) == r.wire.size and got["resp_status"].tolist() == [OK]
    cut = M.Case("end:cut", M.W2, c.body[:-1], 2)
    got = _device_equals_host(ver, M.batch([cut], lead=2, tail=0), model=True)
    assert got["resp_status"].tolist() == [MAL]


# 4. the grid-stride level: totals around its launch edges, and past its block cap --------
def _with_ops(n):
    return M.Case("ops%d" % n, M.W2, M.answer(M.W2, [M.op_result(j & 1, b"x" * j) for j in range(n)], b"r"), n)


@pytest.mark.parametrize("total", [0, 1, 255, 256, 257, 511, 512, 513])
def test_operation_totals_around_the_level3_edges(ver, total):
    """128 responses launch one block of 256 lanes: totals below, at and above one and two strides."""
    P = 128
    if total == 0:
        cases = [M.Case("none", M.OTHER, b"\x0a\x00", 2)] * P
    else:
        per = [total // P] * P
        for i in range(total % P):
            per[(5 * i) % P] += 1
        cases = [_with_ops(n) for n in per]
    got = _device_equals_host(ver, M.batch(cases, slots="guarded"), model=True)
    assert int(got["resp_n_ops"].astype(np.int64).sum()) == total


@pytest.mark.parametrize("last", ["trivial", "certificate"])
def test_one_entry_past_the_level3_block_cap(ver, last):
    """The level-3 grid stops at 4096 blocks, reached at 524,288 responses: with two empty
    operations in all but the last response and three in the last, the entry total is one more
    than the grid has lanes, so exactly one lane takes a second stride."""
    lib = mh.load_library()
    P = 524288
    two = M.answer(M.W2, [b"", b""])
    assert two == bytes.fromhex("0a040a000a00")
    third = b"" if last == "trivial" else M.op_result(0, b"last", True, M.cert(2, 4, True))
    three = M.answer(M.W2, [b"", b"", third], b"r")
    blob = b"\x5a" + two + three
    r = mh.ResultReplies(wire=np.frombuffer(blob, np.uint8),
                         resp_off=np.concatenate([np.full(P - 1, 1), [1 + len(two)]]).astype(np.uint64),
                         resp_len=np.concatenate([np.full(P - 1, len(two)), [len(three)]]).astype(np.uint32),
                         resp_kind=np.zeros(P, np.uint8), req_resp_off=np.array([0, P - 1, P], np.uint32),
                         n_ops=np.array([2, 3], np.uint32), slot_off=(2 * np.arange(P)).astype(np.uint64))
    n = r.n_slots + 3
    assert n == 2 * P + 4
    host = mh.result_reply_decode(r, n, fill=FILL)
    assert int(host["resp_n_ops"].astype(np.int64).sum()) == 4096 * 256 + 1 and not host["resp_status"].any()
    got = _decode_device(ver, r, n)
    M.assert_equal(got, host)
    assert got["op_status"][2 * P - 2:2 * P + 1].tolist() == [0, 0, 0]
    assert int(got["op_flags"][2 * P]) == (0 if last == "trivial" else mh.RRO_HAS_CERT)
    assert (got["op_status"][2 * P + 1:] == FILL).all()


# 5. streams, scratch, profile ---------------------------------------------------------------
def test_two_streams_give_equal_bytes(ver):
    import torch

    r = M.batch(M.corpus(), slots="guarded")
    n = M.n_slots(r)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    dr = mh.DeviceResultReplies(r, 0)
    o1, o2 = mh.DeviceResultDecoded(r.n_resps, n, fill=FILL), mh.DeviceResultDecoded(r.n_resps, n, fill=FILL)
    torch.cuda.synchronize()
    ver.result_reply_decode_device(dr, o1, stream=s1.cuda_stream)
    ver.result_reply_decode_device(dr, o2, stream=s2.cuda_stream)  # the same scratch: ordered behind the first
    torch.cuda.synchronize()
    a, b = o1.to_host(), o2.to_host()
    M.assert_equal(a, b)
    M.assert_equal(a, mh.result_reply_decode(r, n, fill=FILL))


def test_scratch_grows_and_is_reused(ver):
    small = M.batch(M.own_cases()[:5])
    large = M.batch(M.corpus() + M.own_cases(), slots="guarded")
    for r in (small, large, small):
        _device_equals_host(ver, r)


def test_profile_reader(ver):
    r = M.batch(M.own_cases())
    ver.set_profiling(True)
    try:
        _device_equals_host(ver, r)
        prof = ver.read_result_decode_profile()
    finally:
        ver.set_profiling(False)
    assert tuple(prof) == mh.RESULT_DECODE_STAGES and all(0 <= v < 1000 for v in prof.values())
    assert prof["k_rr_resp"] > 0 and prof["k_rr_ops"] > 0
    _device_equals_host(ver, r)  # a call without profiling leaves nothing to read
    with pytest.raises(mh.MochiError, match="no result reply decode call was made while profiling was on"):
        ver.read_result_decode_profile()


# 6. the closing round on one stream ----------------------------------------------------------
@pytest.mark.parametrize("slots", ["dense", "guarded"])
def test_decode_tally_coalesce_on_one_stream(ver, slots):
    """Four servers' answers (WRONG_SHARD ops, read-instead-of-apply results, a short, a
    MALFORMED, a FALLBACK and a foreign answer): decode -> mochi_tally_responses_device ->
    mochi_result_coalesce_device enqueued back to back, one synchronise at the end, against the
    plain-Python client."""
    import torch

    lib = mh.load_library()
    groups, ks = M.cluster_batch(40)
    r = M.batch_grouped(groups, ks, slots)
    Q, R = r.n_reqs, 4
    k = np.asarray(ks, np.int64)
    out_off = (np.cumsum((k + 2)[::-1])[::-1] - k).astype(np.uint64)
    n_out = int(k.sum() + 2 * Q + 2)
    chosen_off = np.concatenate([[0], np.cumsum(k)])[:-1].astype(np.uint64)
    dev = torch.device("cuda", 0)
    dr = mh.DeviceResultReplies(r, 0)
    dec = mh.DeviceResultDecoded(r.n_resps, M.n_slots(r), fill=FILL)
    co = mh.DeviceResultCoalesced(n_out, fill=FILL)
    d_out_off, d_chosen_off = mh._to_dev(out_off, 0), mh._to_dev(chosen_off, 0)
    chosen = torch.full((int(k.sum()),), -1, dtype=torch.int32, device=dev)
    reason = torch.full((Q,), FILL, dtype=torch.uint8, device=dev)
    bits = torch.full(((Q + 31) // 32,), -1, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    ver.result_reply_decode_device(dr, dec, stream=s.cuda_stream)
    rc = lib.mochi_tally_responses_device(Q, dr.req_resp_off.data_ptr(), dr.n_ops.data_ptr(), dec.resp_n_ops.data_ptr(),
                                          dr.slot_off.data_ptr(), dec.op_status.data_ptr(), d_chosen_off.data_ptr(), R,
                                          chosen.data_ptr(), reason.data_ptr(), bits.data_ptr(), s.cuda_stream)
    assert rc == mh.OK
    mh.result_coalesce_device(dr, dec, chosen, d_chosen_off, bits, d_out_off, co, stream=s.cuda_stream)
    torch.cuda.synchronize()
    accept, why, want = M.client(r, R, out_off, n_out, FILL)
    np.testing.assert_array_equal(mh.unpack_bits(bits.cpu().numpy().view(np.uint32), Q), accept)
    np.testing.assert_array_equal(reason.cpu().numpy(), why)
    got = co.to_host()
    M.assert_equal(got, want)
    assert accept.any() and not accept.all() and set(why.tolist()) == {0, 1, 2}
    # and the host chain gives the same bytes
    hdec = mh.result_reply_decode(r, M.n_slots(r), fill=FILL)
    hch, hwhy, hbits = M.tally_host(r, hdec, R, chosen_off, int(k.sum()))
    M.assert_equal(got, mh.result_coalesce(r, hdec, hch, chosen_off, hbits, out_off, n_out, fill=FILL))
