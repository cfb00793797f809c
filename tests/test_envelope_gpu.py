"""The envelope codec on the GPU (mochi_envelope_decode / _route / _join / _encode _device):
every device form equals its host form array for array, into capacity-sized outputs
prefilled with a guard byte, so that a stray write shows.  Frame counts at the wave and
block edges of the partition ranks (513: three blocks, the cross-block scan), the whole
mutation corpus as one batch, every truncation in front of the bytes it was cut from (an
over-read gives the uncut frame's values) with the last frame ending an exact-size buffer,
the join's probe chains and edge ids, and the wrap at the copy's chunk edges, both prefix
modes and both capacity modes."""
import numpy as np
import pytest

import envelope_cases as C
import envelope_model as E
import mochi_hip as mh
import workload as W

pytestmark = pytest.mark.gpu

FILL = 0xA5


@pytest.fixture(scope="module")
def ver():
    v = mh.Verifier([mh.pem_modulus(p) for p in W.load_keys(4)], 0)
    yield v
    v.close()


def _stream():
    import torch

    return torch.cuda.Stream().cuda_stream


def _sync():
    import torch

    torch.cuda.synchronize()


def _same(dev: dict, host: dict):
    for k, h in host.items():
        d = dev[k]
        assert d.shape == h.shape, k
        bad = np.flatnonzero(d != h)
        assert bad.size == 0, (k, int(bad[0]), d[bad[0]], h[bad[0]])


def _decode_route(ver, fr, model_frames=None):
    """decode, then route, on one stream without a wait between them; both against the host
    forms (and the decode against the model when the frames are given).  Returns the device
    objects and the host decode."""
    n = fr.n_frames
    h_dec = mh.envelope_decode(fr, fill=FILL)
    if model_frames is not None:
        want = E.decode(model_frames, [int(o) for o in fr.frame_off])
        for k in E.DEC_KEYS:
            assert np.array_equal(h_dec[k], want[k]), k
    h_rt = mh.envelope_route(h_dec, fill=FILL)
    dfr = mh.DeviceEnvelopeFrames(fr)
    ddec = mh.DeviceEnvelopeDecoded(n, fill=FILL)
    drt = mh.DeviceEnvelopeRouted(n, fill=FILL)
    _sync()  # uploads and fills went to the current stream
    st = _stream()
    ver.envelope_decode_device(dfr, ddec, stream=st)
    ver.envelope_route_device(ddec, drt, stream=st)
    _sync()
    _same(ddec.to_host(), h_dec)
    _same(drt.to_host(), h_rt)
    return dfr, ddec, h_dec


COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 513]


@pytest.mark.parametrize("n", COUNTS)
def test_one_kind(ver, n):
    frames = E.batch_one_kind(n, kind=(7, 10, 5)[n % 3])
    _decode_route(ver, mh.EnvelopeFrames.pack(frames, pad=1), frames)


@pytest.mark.parametrize("n", COUNTS)
def test_seeded_mix(ver, n):
    frames = E.batch_mix(n, seed=n)
    dfr, ddec, h_dec = _decode_route(ver, mh.EnvelopeFrames.pack(frames, pad=3), frames)
    if n >= 63:
        assert len(set(h_dec["status"])) == 3
    if n >= 255:  # enough draws for every kind (a condition on the batch, checked against the model)
        assert len(set(h_dec["kind"])) == E.KINDS


def test_one_frame_per_kind(ver):
    frames = E.batch_per_kind()
    _decode_route(ver, mh.EnvelopeFrames.pack(frames), frames)
    _decode_route(ver, mh.EnvelopeFrames.pack(frames[::-1], pad=1), frames[::-1])


def test_whole_corpus_one_batch(ver):
    frames = [c.frame for c in E.corpus()]
    _decode_route(ver, mh.EnvelopeFrames.pack(frames, pad=1), frames)


def test_aliased_frames(ver):
    """Slices may alias: every frame the same bytes, and a frame inside another's body."""
    inner = E.canonical(8, 1)
    outer = E.frame(7, inner, msg_id=b"outer")
    wire = np.frombuffer(outer, np.uint8).copy()
    at = outer.index(inner)
    fr = mh.EnvelopeFrames(wire, np.array([0, at, 0, at, 0], np.uint64),
                           np.array([len(outer), len(inner), len(outer), len(inner), len(outer) - 1], np.uint32))
    dfr, ddec, h = _decode_route(ver, fr)
    assert list(h["kind"]) == [7, 8, 7, 8, 0] and h["status"][4] == mh.ENV_MALFORMED


def test_truncations_before_their_own_tail_and_exact_size_buffer(ver):
    """Frame b[:i] lies in front of b[i:], which belongs to no frame: a read past the slice
    decodes the uncut frame.  The last frame ends the device allocation's tensor."""
    import torch

    parts, off, ln, frames, pos = [], [], [], [], 0
    for nm, make in E.MUTATED_BASES:
        b = make()
        for i in range(len(b) + 1):
            off.append(pos)
            ln.append(i)
            frames.append(b[:i])
            parts.append(b)
            pos += len(b)
    last = E.MUTATED_BASES[0][1]()[:-1]
    off.append(pos)
    ln.append(len(last))
    frames.append(last)
    parts.append(last)
    wire = np.frombuffer(b"".join(parts), np.uint8).copy()
    assert int(off[-1]) + ln[-1] == wire.size
    fr = mh.EnvelopeFrames(wire, np.array(off, np.uint64), np.array(ln, np.uint32))
    dfr, ddec, h = _decode_route(ver, fr, frames)
    assert dfr.wire.numel() == wire.size and dfr.wire_len == wire.size
    assert (h["status"] == mh.ENV_MALFORMED).sum() > 50 and (h["status"] == mh.ENV_OK).sum() > 10


def test_streams_and_profile(ver):
    frames = E.batch_mix(300, seed=1)
    fr = mh.EnvelopeFrames.pack(frames)
    ver.set_profiling(True)
    try:
        dfr, ddec, h = _decode_route(ver, fr)
        for which in ("decode", "route"):
            p = ver.read_envelope_profile(which)
            assert tuple(p) == mh.ENVELOPE_STAGES[which] and all(v >= 0 for v in p.values())
    finally:
        ver.set_profiling(False)
    # the null stream
    ddec2 = mh.DeviceEnvelopeDecoded(300, fill=FILL)
    ver.envelope_decode_device(dfr, ddec2)
    _sync()
    _same(ddec2.to_host(), h)


def test_device_argument_errors(ver):
    """What the device forms check beyond the host forms' checks (tests/test_envelope_cpu.py)."""
    import ctypes

    lib = ver.lib
    fr = mh.EnvelopeFrames.pack([E.canonical(8, 0)])
    dfr, ddec = mh.DeviceEnvelopeFrames(fr), mh.DeviceEnvelopeDecoded(1)
    drt, dj, dreq = mh.DeviceEnvelopeRouted(1), mh.DeviceEnvelopeJoined(1, 1), mh.DeviceEnvelopeRequests([b"id"])
    f, d, r, j, q = dfr.to_c(), ddec.to_c(), drt.to_c(), dj.to_c(), dreq.to_c()
    A = ctypes.addressof

    def expect(rc, text):
        assert rc == mh.EINVAL and text in mh._err(lib), mh._err(lib)

    expect(lib.mochi_envelope_decode_device(None, A(f), A(d), None), "null context")
    expect(lib.mochi_envelope_decode_device(ver.ctx, None, A(d), None), "null argument")
    expect(lib.mochi_envelope_route_device(None, 1, ddec.status.data_ptr(), ddec.kind.data_ptr(), ddec.body_off.data_ptr(),
                                           ddec.body_len.data_ptr(), A(r), None), "null context")
    expect(lib.mochi_envelope_route_device(ver.ctx, 1, None, None, None, None, A(r), None), "status / kind / body_off / body_len required")
    expect(lib.mochi_envelope_join_device(None, A(q), A(f), A(d), A(j), dj.n_resps.data_ptr(), None), "null context")
    expect(lib.mochi_envelope_join_device(ver.ctx, A(q), A(f), A(d), A(j), None, None), "n_resps_dev required")
    expect(lib.mochi_envelope_join_device(ver.ctx, None, A(f), A(d), A(j), dj.n_resps.data_ptr(), None), "null argument")
    src, msgs = C.encode_source()
    dsrc = mh.DeviceEnvelopeSource(src)
    s = dsrc.to_c()
    outs, buf = _outputs(src.n_msgs, 8)
    need = ctypes.c_uint64(0)
    tail = (outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr())
    expect(lib.mochi_envelope_encode_device(None, A(s), None, 0, *tail, A(need), None, None), "null context")
    expect(lib.mochi_envelope_encode_device(ver.ctx, A(s), None, 0, *tail, None, None, None), "wire_len or wire_len_dev required")
    expect(lib.mochi_envelope_encode_device(ver.ctx, A(s), None, 8, *tail, A(need), None, None), "wire_out required")
    ms = np.zeros(4, np.float32)
    expect(lib.mochi_ctx_read_envelope_profile(ver.ctx, 7, ms.ctypes.data, 4), "which is no MOCHI_ENV_PROF_*")
    expect(lib.mochi_ctx_read_envelope_profile(None, 0, ms.ctypes.data, 4), "null argument")
    _sync()
    assert bool((buf == FILL).all())


def test_profile_without_a_profiled_call():
    v = mh.Verifier([mh.pem_modulus(p) for p in W.load_keys(4)], 0)
    try:
        with pytest.raises(mh.MochiError, match="no envelope encode call was made while profiling was on"):
            v.read_envelope_profile("encode")
    finally:
        v.close()


# ---- join ----------------------------------------------------------------------------------------
def _join_both(ver, ids, frames, pad=1):
    fr = mh.EnvelopeFrames.pack(frames, pad=pad)
    dfr, ddec, h_dec = _decode_route(ver, fr, frames)
    h, P = mh.envelope_join(ids, fr, h_dec, fill=FILL)
    want = E.join(ids, frames, h_dec)
    assert P == len(want["resp_frame"])
    dreq = mh.DeviceEnvelopeRequests(ids)
    dj = mh.DeviceEnvelopeJoined(fr.n_frames, len(ids), fill=FILL)
    _sync()
    ver.envelope_join_device(dreq, dfr, ddec, dj, stream=_stream())
    _sync()
    _same(dj.to_host(), h)
    assert int(dj.n_resps.cpu().numpy().view(np.uint32)[0]) == P
    return h, P


@pytest.mark.parametrize("name", sorted(C.join_cases()))
def test_join(ver, name):
    ids, frames = C.join_cases()[name]
    _join_both(ver, ids, frames)


def test_join_decode_and_join_on_one_stream(ver):
    """decode -> join without a wait, more frames than one block, profile read back."""
    ids, frames = C.join_cases()["prefix_chains_300"]
    frames = frames + E.batch_mix(200, seed=5)
    fr = mh.EnvelopeFrames.pack(frames, pad=2)
    h_dec = mh.envelope_decode(fr, fill=FILL)
    h, P = mh.envelope_join(ids, fr, h_dec, fill=FILL)
    dfr, dreq = mh.DeviceEnvelopeFrames(fr), mh.DeviceEnvelopeRequests(ids)
    ddec, dj = mh.DeviceEnvelopeDecoded(fr.n_frames, fill=FILL), mh.DeviceEnvelopeJoined(fr.n_frames, len(ids), fill=FILL)
    _sync()
    st = _stream()
    ver.set_profiling(True)
    try:
        ver.envelope_decode_device(dfr, ddec, stream=st)
        ver.envelope_join_device(dreq, dfr, ddec, dj, stream=st)
        _sync()
        assert tuple(ver.read_envelope_profile("join")) == mh.ENVELOPE_STAGES["join"]
    finally:
        ver.set_profiling(False)
    _same(dj.to_host(), h)
    assert P >= 450


# ---- encode --------------------------------------------------------------------------------------
def _outputs(M, cap, shift=0):
    import torch

    dev = torch.device("cuda", 0)
    buf = torch.full((shift + cap + 16,), FILL, dtype=torch.uint8, device=dev)
    pat8 = int.from_bytes(bytes([FILL]) * 8, "little", signed=True)
    pat4 = int.from_bytes(bytes([FILL]) * 4, "little", signed=True)
    outs = (buf[shift:shift + cap] if cap else None, torch.full((M + 2,), pat8, dtype=torch.int64, device=dev),
            torch.full((M + 2,), pat4, dtype=torch.int32, device=dev), torch.full((M + 2,), FILL, dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()
    return outs, buf


def _assert_encoded(host, outs, buf, M, shift=0, wire_written=True):
    wire, off, ln, st = host
    whole = buf.cpu().numpy()
    n = wire.size if wire_written else 0
    if wire_written:
        assert whole[shift:shift + n].tobytes() == wire.tobytes()
    assert (whole[:shift] == FILL).all() and (whole[shift + n:] == FILL).all()
    d_off, d_ln, d_st = (t.cpu().numpy() for t in outs[1:])
    np.testing.assert_array_equal(d_off.view(np.uint64)[:M], off)
    np.testing.assert_array_equal(d_ln.view(np.uint32)[:M], ln)
    np.testing.assert_array_equal(d_st[:M], st)
    assert (d_off.view(np.uint8)[8 * M:] == FILL).all() and (d_ln.view(np.uint8)[4 * M:] == FILL).all() and (d_st[M:] == FILL).all()


@pytest.mark.parametrize("flags", [0, mh.ENV_LENGTH_PREFIX])
@pytest.mark.parametrize("n_extra,shift", [(0, 0), (40, 3), (1100, 9)])  # 1100: past the single-block scan line
def test_encode_equals_host(ver, flags, n_extra, shift):
    src, msgs = C.encode_source(flags, n_extra=n_extra)
    host = mh.envelope_encode(src)
    assert host[0].tobytes() == C.expected_wire(msgs, flags)[0]
    dsrc = mh.DeviceEnvelopeSource(src)
    outs, buf = _outputs(src.n_msgs, host[0].size, shift=shift)
    rc, n = ver.envelope_encode_device(dsrc, *outs, stream=_stream())
    _sync()
    assert rc == mh.OK and n == host[0].size
    _assert_encoded(host, outs, buf, src.n_msgs, shift)


@pytest.mark.parametrize("flags", [0, mh.ENV_LENGTH_PREFIX])
def test_encode_one_byte_short(ver, flags):
    import torch

    src, msgs = C.encode_source(flags, n_extra=20)
    host = mh.envelope_encode(src)
    dsrc = mh.DeviceEnvelopeSource(src)
    M, need = src.n_msgs, host[0].size
    # the host waits for the total: the needed size comes back, nothing of wire is written
    outs, buf = _outputs(M, need - 1)
    rc, n = ver.envelope_encode_device(dsrc, *outs, stream=_stream(), check=False)
    _sync()
    assert rc == mh.EINVAL and n == need
    _assert_encoded(host, outs, buf, M, wire_written=False)
    # no host wait: the total goes to the device word, the kernels write nothing of wire
    total = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
    outs, buf = _outputs(M, need - 1)
    rc, n = ver.envelope_encode_device(dsrc, *outs, stream=_stream(), wire_len_dev=total)
    _sync()
    assert rc == mh.OK and n is None and int(total.item()) == need
    _assert_encoded(host, outs, buf, M, wire_written=False)
    # ... and with the exact capacity everything is
    outs, buf = _outputs(M, need)
    ver.envelope_encode_device(dsrc, *outs, stream=_stream(), wire_len_dev=total)
    _sync()
    _assert_encoded(host, outs, buf, M)


@pytest.mark.parametrize("flags", [0, mh.ENV_LENGTH_PREFIX])
def test_encode_per_message_status(ver, flags):
    """The device form: a kind above 12 and an id that is not UTF-8 are that message's status,
    length 0 (with the prefix: the byte 00), and the neighbours are written as ever."""
    good = dict(kind=7, body=b"body", ts=3, msg_id=b"id", reply_to=b"", server_id=b"s")
    msgs = [good, dict(good, kind=13), good, dict(good, msg_id=b"\xC0\x80"), dict(good, reply_to=b"ab\xC3"),
            dict(good, server_id=b"\xED\xA0\x80"), dict(good, kind=255, msg_id=b"\xFF"), good]
    want_st = [0, mh.ENC_BAD_KIND, 0, mh.ENC_BAD_ID, mh.ENC_BAD_ID, mh.ENC_BAD_ID, mh.ENC_BAD_KIND, 0]
    ids, cols = bytearray(), {k: [] for k in ("msg_id_off", "msg_id_len", "reply_to_off", "reply_to_len", "server_id_off", "server_id_len")}
    for m in msgs:
        for nm in ("msg_id", "reply_to", "server_id"):
            cols[nm + "_off"].append(len(ids))
            cols[nm + "_len"].append(len(m[nm]))
            ids += m[nm] + b"\xA9"  # a continuation byte behind every id: reading past the slice would accept ab C3
    src = mh.EnvelopeSource(bodies=np.frombuffer(b"body", np.uint8), ids=np.frombuffer(bytes(ids), np.uint8),
                            kind=np.array([m["kind"] for m in msgs], np.uint8), body_off=np.zeros(len(msgs), np.uint64),
                            body_len=np.full(len(msgs), 4, np.uint32), msg_timestamp=np.full(len(msgs), 3, np.int64), flags=flags, **cols)
    frames = [E.frame(7, b"body", 3, b"s", b"id") if s == 0 else b"" for s in want_st]
    parts, offs, pos = [], [], 0
    for f in frames:
        pre = E.varint(len(f)) if flags else b""
        offs.append(pos + len(pre))
        parts.append(pre + f)
        pos += len(pre) + len(f)
    host = (np.frombuffer(b"".join(parts), np.uint8), np.array(offs, np.uint64), np.array([len(f) for f in frames], np.uint32),
            np.array(want_st, np.uint8))
    outs, buf = _outputs(len(msgs), host[0].size)
    rc, n = ver.envelope_encode_device(mh.DeviceEnvelopeSource(src), *outs, stream=_stream())
    _sync()
    assert rc == mh.OK and n == host[0].size
    _assert_encoded(host, outs, buf, len(msgs))


def test_encode_then_decode_on_the_device(ver):
    """The wrap's output is the decoder's input in place: frames in HBM to frames in HBM."""
    import torch

    src, msgs = C.encode_source(mh.ENV_LENGTH_PREFIX, n_extra=100)
    host = mh.envelope_encode(src)
    M = src.n_msgs
    outs, buf = _outputs(M, host[0].size)
    total = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    ddec = mh.DeviceEnvelopeDecoded(M, fill=FILL)
    _sync()
    st = _stream()
    dsrc = mh.DeviceEnvelopeSource(src)
    _sync()
    ver.set_profiling(True)
    try:
        ver.envelope_encode_device(dsrc, *outs, stream=st, wire_len_dev=total)
        ver.envelope_decode_device(mh.DeviceEnvelopeFrames.from_tensors(M, outs[0], outs[1], outs[2]), ddec, stream=st)
        _sync()
        p = ver.read_envelope_profile("encode")
        assert tuple(p) == mh.ENVELOPE_STAGES["encode"] and all(v >= 0 for v in p.values())
    finally:
        ver.set_profiling(False)
    d = ddec.to_host()
    assert not d["status"].any()
    assert list(d["kind"]) == [m["kind"] for m in msgs] and list(d["msg_timestamp"]) == [m["ts"] for m in msgs]
    assert list(d["body_len"]) == [len(m["body"]) if m["kind"] else 0 for m in msgs]
    assert list(d["reply_to_len"]) == [len(m["reply_to"]) for m in msgs]
