"""Answer encoder on the GPU (mochi_result_reply_encode_device): the device form equals the
host form byte for byte (and both the model) on every CPU case set, into guard-filled
outputs, in both capacity modes -- the too-small capacity in the device mode too: nothing
written, offsets, lengths and statuses still there; response counts around the
single-block scan line with mixed kinds; certificates at the chunk and wave-round edges of
the copy kernel at every source and destination misalignment; a non-default stream, two
streams, the profile; and one batch whose offsets pass 2^32 through aliased certificates."""
import numpy as np
import pytest

import mochi_hip as mh
import result_encode_model as E
import result_reply_model as RRM
import workload as W

pytestmark = pytest.mark.gpu

FILL = 0xEE
SCAN_LINE = 1024  # w2_small: below it the 64-bit scan runs inside the size kernel's one block


@pytest.fixture(scope="module")
def ver():
    v = mh.Verifier([mh.pem_modulus(p) for p in W.load_keys(4)], 0)
    yield v
    v.close()


def _stream():
    import torch

    return torch.cuda.Stream().cuda_stream


def _outputs(P, cap, fill=FILL, shift=0):
    """(wire, msg_off, msg_len, status) on the device, prefilled; `wire` starts `shift` bytes
    into its allocation and ends 16 guard bytes before its end."""
    import torch

    dev = torch.device("cuda", 0)
    buf = torch.full((shift + cap + 16,), fill, dtype=torch.uint8, device=dev)
    pat8 = int.from_bytes(bytes([fill]) * 8, "little", signed=True)
    pat4 = int.from_bytes(bytes([fill]) * 4, "little", signed=True)
    outs = (buf[shift:shift + cap] if cap else None, torch.full((P + 2,), pat8, dtype=torch.int64, device=dev),
            torch.full((P + 2,), pat4, dtype=torch.int32, device=dev), torch.full((P + 2,), fill, dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()  # the fills went to the current stream; the encoder runs on another
    return outs, buf


def _assert_same(host, outs, buf, P, shift=0):
    """Equal bytes, offsets, lengths and statuses; everything past them still the fill byte."""
    wire, off, ln, st = host
    d_wire, d_off, d_ln, d_st = outs
    whole = buf.cpu().numpy()
    n = wire.size
    assert whole[shift:shift + n].tobytes() == wire.tobytes()
    assert (whole[:shift] == FILL).all() and (whole[shift + n:] == FILL).all()
    np.testing.assert_array_equal(d_off.cpu().numpy().view(np.uint64)[:P], off)
    np.testing.assert_array_equal(d_ln.cpu().numpy().view(np.uint32)[:P], ln)
    np.testing.assert_array_equal(d_st.cpu().numpy()[:P], st)
    assert (d_off.cpu().numpy().view(np.uint8)[8 * P:] == FILL).all() and (d_st.cpu().numpy()[P:] == FILL).all()
    assert (d_ln.cpu().numpy().view(np.uint8)[4 * P:] == FILL).all()


def _device_equals_host(ver, ra, answers=None, slack=0, shift=0, stream=None):
    """Mode 1 (the host waits for the total) into a buffer `slack` bytes larger than needed."""
    import torch

    host = mh.result_reply_encode(ra)
    if answers is not None:
        want = E.expected_arrays(answers)
        assert host[0].tobytes() == want[0].tobytes()
        np.testing.assert_array_equal(host[3], want[3])
    da = mh.DeviceResultAnswers(ra, 0)
    outs, buf = _outputs(ra.n_resps, host[0].size + slack, shift=shift)
    torch.cuda.synchronize()  # uploads and fills went to the current stream
    rc, n = ver.result_reply_encode_device(da, *outs, stream=stream or _stream())
    torch.cuda.synchronize()
    assert rc == mh.OK and n == host[0].size
    _assert_same(host, outs, buf, ra.n_resps, shift)
    return da, host


# 1. device == host == model on the CPU case sets ----------------------------------------------
@pytest.mark.parametrize("name", sorted(E.cases()))
def test_named_case(ver, name):
    answers = E.cases()[name]
    _device_equals_host(ver, E.layout(answers), answers, slack=len(name) % 3)


@pytest.mark.parametrize("alias,slots", [(False, "dense"), (True, "dense"), (False, "guarded"), (True, "guarded")])
def test_all_cases_in_one_batch(ver, alias, slots):
    answers = E.all_answers()
    _device_equals_host(ver, E.layout(answers, alias=alias, slots=slots), answers, slack=5)


def test_no_ids_arrays_and_the_empty_batch(ver):
    import torch

    answers = (E.Ans(E.W2, (E.OpR(0, b"v", True, E.CERT),)), E.Ans(E.RD, (E.OpR(1),)))
    _device_equals_host(ver, E.layout(answers, ids=False), answers)
    ra = E.layout([])
    total = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
    outs, buf = _outputs(0, 8)
    rc, n = ver.result_reply_encode_device(mh.DeviceResultAnswers(ra, 0), *outs, stream=_stream())
    assert rc == mh.OK and n == 0
    rc, n = ver.result_reply_encode_device(mh.DeviceResultAnswers(ra, 0), *outs, stream=_stream(), wire_len_dev=total)
    torch.cuda.synchronize()
    assert rc == mh.OK and int(total.item()) == 0
    assert bool((buf == FILL).all()) and bool((outs[3] == FILL).all())


def test_decoded_corpus_re_encodes_on_the_device(ver):
    """The decoder's outputs as the encoder's inputs (offsets into the received bytes; rid and
    nonce out of the same blob), as the CPU test does it."""
    cases = [c for c in RRM.own_cases() + RRM.corpus() if c.kind != RRM.OTHER]
    r = RRM.batch(cases)
    d = mh.result_reply_decode(r)
    keep = [p for p, c in enumerate(cases)
            if d["resp_status"][p] == mh.RRS_OK and d["resp_n_ops"][p] == c.n_ops and
            all(d["op_status"][int(r.slot_off[p]) + j] != 0xFF for j in range(c.n_ops))]
    take = lambda k: np.ascontiguousarray(d[k][keep])
    ra = mh.ResultAnswers(wire=r.wire, store=np.zeros(0, np.uint8), ids=r.wire, resp_kind=r.resp_kind[keep],
                          resp_n_ops=take("resp_n_ops"), slot_off=r.slot_off[keep], rid_off=take("resp_rid_off"),
                          rid_len=take("resp_rid_len"), nonce_off=take("resp_nonce_off"), nonce_len=take("resp_nonce_len"),
                          **{k: d[k] for k in mh._RA_SLOT})
    assert ra.n_resps > SCAN_LINE  # the scanned form
    _device_equals_host(ver, ra)


# 2. the capacity rule, both modes -----------------------------------------------------------------
def test_one_byte_short_with_a_host_wait(ver):
    import torch

    answers = E.all_answers()
    ra = E.layout(answers)
    da, host = _device_equals_host(ver, ra, answers)
    need = host[0].size
    outs, buf = _outputs(ra.n_resps, need - 1)
    rc, n = ver.result_reply_encode_device(da, *outs, stream=_stream(), check=False)
    torch.cuda.synchronize()
    assert rc == mh.EINVAL and n == need and bool((buf == FILL).all())
    rc, n = ver.result_reply_encode_device(da, None, *outs[1:], stream=_stream(), check=False)  # the size alone
    assert rc == mh.EINVAL and n == need
    assert mh.result_reply_encode_bound(da) >= need


@pytest.mark.parametrize("slots", ["dense", "guarded"])
def test_device_side_capacity_rule(ver, slots):
    import torch

    answers = E.all_answers()
    ra = E.layout(answers, slots=slots)
    P = ra.n_resps
    da, host = _device_equals_host(ver, ra, answers)
    need = host[0].size
    total = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
    outs, buf = _outputs(P, need + 64)
    rc, n = ver.result_reply_encode_device(da, *outs, stream=_stream(), wire_len_dev=total)
    torch.cuda.synchronize()
    assert rc == mh.OK and n is None and int(total.item()) == need
    _assert_same(host, outs, buf, P)
    total.fill_(-1)
    outs, buf = _outputs(P, need - 1)
    rc, n = ver.result_reply_encode_device(da, *outs, stream=_stream(), wire_len_dev=total)
    torch.cuda.synchronize()
    assert rc == mh.OK and int(total.item()) == need
    assert bool((buf == FILL).all())  # all or nothing
    np.testing.assert_array_equal(outs[1].cpu().numpy().view(np.uint64)[:P], host[1])
    np.testing.assert_array_equal(outs[2].cpu().numpy().view(np.uint32)[:P], host[2])
    np.testing.assert_array_equal(outs[3].cpu().numpy()[:P], host[3])


# 3. the single-block scan line ----------------------------------------------------------------------
@pytest.mark.parametrize("P", [SCAN_LINE - 1, SCAN_LINE, SCAN_LINE + 1])
def test_scan_line_with_mixed_kinds(ver, P):
    pool = [a for a in E.all_answers() if sum(len(o.result) + len(o.cert or b"") for o in a.ops) < 4096]
    answers = [pool[(7 * i) % len(pool)] for i in range(P)]
    assert {a.kind for a in answers} == {E.W2, E.RD, E.OTHER}
    _device_equals_host(ver, E.layout(answers, alias=True, slots="guarded"), answers)


# 4. the copy kernel's edges ---------------------------------------------------------------------------
def test_certificate_lengths_at_every_misalignment(ver):
    """Certificate lengths at the 16-byte chunk and the 1 KiB wave-round edges; per length the
    source at every residue mod 16 (by its place in the blob), and the whole output at every
    residue mod 16 (by shifting the buffer): every (source, destination) pair."""
    import torch

    answers, ra = E.copy_edge()
    src = {(int(ra.op_cert_len[s]), int(ra.op_cert_off[s]) % 16) for s in range(ra.n_slots)}
    assert src == {(n, m) for n in E.COPY_EDGE_LENS for m in range(16)}
    host = mh.result_reply_encode(ra)
    assert host[0].tobytes() == E.expected_arrays(answers)[0].tobytes()
    da = mh.DeviceResultAnswers(ra, 0)
    assert da.wire.data_ptr() % 16 == 0 and da.store.data_ptr() % 16 == 0
    stream = _stream()
    for shift in range(16):
        outs, buf = _outputs(ra.n_resps, host[0].size, shift=shift)
        assert outs[0].data_ptr() % 16 == shift
        torch.cuda.synchronize()
        rc, n = ver.result_reply_encode_device(da, *outs, stream=stream)
        torch.cuda.synchronize()
        assert rc == mh.OK
        _assert_same(host, outs, buf, ra.n_resps, shift)


# 5. streams and the profile -----------------------------------------------------------------------------
def test_two_streams_give_equal_bytes(ver):
    import torch

    answers = E.all_answers()
    ra = E.layout(answers, alias=True)
    host = mh.result_reply_encode(ra)
    da = mh.DeviceResultAnswers(ra, 0)
    outs = [_outputs(ra.n_resps, host[0].size) for _ in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for (o, buf), s in zip(outs, streams):
        rc, n = ver.result_reply_encode_device(da, *o, stream=s.cuda_stream)
        assert n == host[0].size
    torch.cuda.synchronize()
    assert torch.equal(outs[0][1], outs[1][1])
    for o, buf in outs:
        _assert_same(host, o, buf, ra.n_resps)


def test_per_kernel_profile(ver):
    import torch

    answers = E.cases()["ops_64"]
    ra = E.layout(answers)
    da = mh.DeviceResultAnswers(ra, 0)
    outs, buf = _outputs(ra.n_resps, mh.result_reply_encode(ra)[0].size)
    ver.result_reply_encode_device(da, *outs, stream=_stream())
    with pytest.raises(mh.MochiError):  # that call was not profiled
        ver.read_result_encode_profile()
    ver.set_profiling(True)
    ver.result_reply_encode_device(da, *outs, stream=_stream())
    ver.set_profiling(False)
    ms = ver.read_result_encode_profile()
    torch.cuda.synchronize()
    assert list(ms) == list(mh.RESULT_ENCODE_STAGES)
    assert all(0 <= v < 1000 for v in ms.values()) and ms["k_rae_copy"] > 0


# 6. 64-bit offsets -------------------------------------------------------------------------------------------
def test_offsets_past_4_gib(ver):
    """66 answers of 64 operations that all point at one aliased 1 MiB certificate: 64 MiB each,
    4.1 GiB in all from a 1 MiB input.  Only offsets, lengths and the first and the last
    message come to the host."""
    import torch

    cert = np.frombuffer((b"certificate-bytes" * 70000)[:1 << 20], np.uint8)
    n = 66
    one = E.Ans(E.RD, tuple(E.OpR(0, b"", True, cert.tobytes()) for _ in range(64)), b"rid", b"nonce")
    ra = E.layout([one] * n, alias=True)
    assert ra.wire.size < (1 << 20) + 64
    da = mh.DeviceResultAnswers(ra, 0)
    sizes, _ = _outputs(n, 0)
    rc, need = ver.result_reply_encode_device(da, *sizes, stream=_stream(), check=False)
    body = E.message(one)
    assert rc == mh.EINVAL and need == n * len(body) > 1 << 32
    outs, buf = _outputs(n, need, fill=0)
    rc, got = ver.result_reply_encode_device(da, *outs, stream=_stream())
    torch.cuda.synchronize()
    assert got == need and bool((outs[3][:n] == 0).all())
    h_off, h_ln = outs[1].cpu().numpy().view(np.uint64)[:n], outs[2].cpu().numpy().view(np.uint32)[:n]
    np.testing.assert_array_equal(h_ln, np.full(n, len(body), np.uint32))
    np.testing.assert_array_equal(h_off, np.arange(n, dtype=np.uint64) * np.uint64(len(body)))
    assert int(h_off[-1]) > 1 << 32
    for q in (0, n - 1):
        o = int(h_off[q])
        assert outs[0][o:o + len(body)].cpu().numpy().tobytes() == body, q
    assert bool((buf[need:] == 0).all())
