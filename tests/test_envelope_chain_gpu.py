"""The envelope calls in front of the body decoders, on one stream: frames in HBM -> decode ->
route (the server) or join (the client) -> the existing device decoders, fed with the
device-built arrays as they stand.  No host wait lies between the envelope calls and the
decoders (the counts the decoders take as host scalars are known from how the batch was
built); the decoders' outputs equal those of the same decoders fed with host-built arrays."""
import numpy as np
import pytest

import envelope_model as E
import mochi_hip as mh
import result_encode_model as AM
import workload as W
import write1_decode_model as DM
import write1_request_model as QM

pytestmark = pytest.mark.gpu

FILL = 0xA5


@pytest.fixture(scope="module")
def ver():
    v = mh.Verifier([mh.pem_modulus(p) for p in W.load_keys(4)], 0)
    v.set_server_ids(DM.IDS)
    yield v
    v.close()


@pytest.fixture(scope="module")
def signer():
    s = mh.DeviceSigner(W.load_keys(1)[0], 0)
    yield s
    s.close()


def _sync():
    import torch

    torch.cuda.synchronize()


def _stream():
    import torch

    return torch.cuda.Stream().cuda_stream


def _body_slices(frames, fr):
    """(offset in the wire, length) of every frame's payload, by the model."""
    out = []
    for f, base in zip(frames, fr.frame_off):
        p = E.parse(f)
        assert p.status == E.OK
        out.append((int(base) + p.body[0], p.body[1]))
    return out


def _same_arrays(a: dict, b: dict):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_server_chain(ver, signer):
    """Mixed kinds 5, 7 and 10 -> decode -> route -> the Write1 request decoder on the kind-7 run."""
    bodies7 = [QM.write1(b"client-%d" % i, QM.transaction([QM.operation(QM.WRITE, b"key-%d" % (i % 5), b"v%d" % i),
                                                           QM.operation(QM.WRITE, b"other-%d" % i, b"w")]), i + 1, QM.HASH)
               for i in range(40)]
    frames, is7 = [], []
    for i in range(100):
        k = (7, 5, 10, 7, 7)[i % 5] if i < 65 else (5, 10)[i % 2]
        body = bodies7[len([x for x in is7 if x])] if k == 7 else E.body_of(k, i)
        frames.append(E.frame(k, body, ts=i + 1, server_id=b"s", msg_id=E.UUID % i))
        is7.append(k == 7)
    n5, n7 = sum(1 for f in frames if E.parse(f).kind == 5), sum(is7)
    assert n7 == 39 and n5 > 0
    fr = mh.EnvelopeFrames.pack(frames, pad=1)
    dfr = mh.DeviceEnvelopeFrames(fr)
    ddec, drt = mh.DeviceEnvelopeDecoded(100, fill=FILL), mh.DeviceEnvelopeRouted(100, fill=FILL)
    # host-built msg_off / msg_len of the same requests
    sl = [s for s, seven in zip(_body_slices(frames, fr), is7) if seven]
    host_reqs = mh.Write1Requests(wire=fr.wire, msg_off=np.array([o for o, n in sl], np.uint64),
                                  msg_len=np.array([n for o, n in sl], np.uint32))
    want = mh.write1_request_decode(host_reqs)
    out_dev = mh.DeviceWrite1RequestsDecoded(n7, want.n_ops, fill=FILL)
    out_ref = mh.DeviceWrite1RequestsDecoded(n7, want.n_ops, fill=FILL)
    dref = mh.DeviceWrite1Requests(host_reqs, 0)
    _sync()
    st = _stream()
    ver.envelope_decode_device(dfr, ddec, stream=st)
    ver.envelope_route_device(ddec, drt, stream=st)
    # the run of kind 7 begins behind the kind-5 frames (kinds 0..4 and 6 do not occur)
    chained = mh.DeviceWrite1Requests.from_tensors(n7, wire=dfr.wire, msg_off=drt.body_off[n5:n5 + n7],
                                                   msg_len=drt.body_len[n5:n5 + n7])
    signer.request_decode_device(chained, out_dev, stream=st)
    signer.request_decode_device(dref, out_ref, stream=st)
    _sync()
    kind_off = drt.to_host()["kind_off"]
    assert (int(kind_off[7]), int(kind_off[8])) == (n5, n5 + n7)
    got, ref = out_dev.to_host(), out_ref.to_host()
    assert (got.n_ops, got.n_keys) == (ref.n_ops, ref.n_keys) == (want.n_ops, want.n_keys) and got.n_ops == 2 * n7
    _same_arrays(got.arrays, ref.arrays)
    QM.assert_equal(got.trimmed(), want.trimmed())
    assert (got.arrays["req_status"] == mh.W1Q_OK).all()


def _interleaved(make, n_reqs=3, n_servers=4):
    """Frames server-major (request q's replies are every n_reqs-th frame); the ids asked for."""
    ids = [E.UUID % (40 + q) for q in range(n_reqs)]
    frames = [make(q, s, ids[q]) for s in range(n_servers) for q in range(n_reqs)]
    return ids, frames


def _join_inputs(ids, frames):
    """The frames and the request ids on the device, and the outputs of decode and join."""
    fr = mh.EnvelopeFrames.pack(frames, pad=3)
    dfr, dreq = mh.DeviceEnvelopeFrames(fr), mh.DeviceEnvelopeRequests(ids)
    ddec, dj = mh.DeviceEnvelopeDecoded(len(frames), fill=FILL), mh.DeviceEnvelopeJoined(len(frames), len(ids), fill=FILL)
    return fr, dfr, dreq, ddec, dj


def _host_grouped(frames, fr, n_reqs, n_servers):
    """Host-built: the responses grouped by request in frame order -> (frame index, offset, length)."""
    sl = _body_slices(frames, fr)
    order = [s * n_reqs + q for q in range(n_reqs) for s in range(n_servers)]
    return order, [sl[f] for f in order]


def test_client_chain_write1(ver):
    """Replies of kinds 8, 9 and 12 for 3 requests x 4 servers -> decode -> join -> the Write1 reply decoder."""
    keys = [[b"k-%d-0" % q, b"k-%d-1" % q] for q in range(3)]

    def make(q, s, to):
        kind = (8, 8, 9, 12)[s]
        if kind == 12:
            body = E.ld(1, b"failed")
        else:
            body = DM.reply(DM.multigrant([(k, DM.grant(k, 100 + q)) for k in keys[q]], server=DM.IDS[s]),
                            certs=[(keys[q][0], DM.writecert(keys[q][:1]))] if kind == 9 else ())
        return E.frame(kind, body, ts=s + 1, server_id=DM.IDS[s], msg_id=b"r-%d-%d" % (q, s), reply_to=to)

    ids, frames = _interleaved(make)
    fr, dfr, dreq, ddec, dj = _join_inputs(ids, frames)
    order, sl = _host_grouped(frames, fr, 3, 4)
    strings = b"".join(k for ks in keys for k in ks)
    klen = [len(k) for ks in keys for k in ks]
    ctx = dict(strings=np.frombuffer(strings, np.uint8).copy(), req_op_off=np.array([0, 2, 4, 6], np.uint32),
               op_key_off=np.concatenate([[0], np.cumsum(klen)[:-1]]).astype(np.uint64), op_key_len=np.array(klen, np.uint32))
    host_r = mh.Write1Replies(wire=fr.wire, resp_off=np.array([o for o, n in sl], np.uint64),
                              resp_len=np.array([n for o, n in sl], np.uint32),
                              resp_kind=np.array([(mh.W1_OK, mh.W1_OK, mh.W1_REFUSED, mh.W1_REQUEST_FAILED)[i % 4] for i in range(12)], np.uint8),
                              req_resp_off=np.array([0, 4, 8, 12], np.uint32), **ctx)
    want = mh.write1_reply_decode(host_r, DM.IDS)
    assert want.n_grants == 3 * 3 * 2
    dref = mh.DeviceWrite1Replies(host_r, 0)
    chained = mh.DeviceWrite1Replies.from_tensors(12, 3, 6, wire=dfr.wire, resp_off=dj.resp_off, resp_len=dj.resp_len,
                                                  resp_kind=dj.resp_w1_kind, req_resp_off=dj.req_resp_off, strings=dref.strings,
                                                  req_op_off=dref.req_op_off, op_key_off=dref.op_key_off, op_key_len=dref.op_key_len)
    out_dev = mh.DeviceWrite1Decoded(12, want.n_grants, want.n_certs, fill=FILL)
    out_ref = mh.DeviceWrite1Decoded(12, want.n_grants, want.n_certs, fill=FILL)
    _sync()  # uploads and fills went to the current stream; from here on one stream and no wait of the test's
    st = _stream()
    ver.envelope_decode_device(dfr, ddec, stream=st)
    ver.envelope_join_device(dreq, dfr, ddec, dj, stream=st)
    ver.write1_reply_decode_device(chained, out_dev, stream=st)
    ver.write1_reply_decode_device(dref, out_ref, stream=st)
    _sync()
    j = dj.to_host()
    assert list(j["resp_frame"]) == order and list(j["req_resp_off"]) == [0, 4, 8, 12]
    got, ref = out_dev.to_host(), out_ref.to_host()
    assert (got.n_grants, got.n_certs) == (ref.n_grants, ref.n_certs) == (want.n_grants, want.n_certs)
    _same_arrays(got.arrays, ref.arrays)
    DM.assert_equal(got.trimmed(), want.trimmed())


def test_client_chain_result(ver):
    """Answers of kinds 11 and 6 for 3 requests x 4 servers -> decode -> join -> the result reply decoder."""
    def make(q, s, to):
        kind = 11 if q != 1 else 6
        ops = (AM.OpR(0, b"value-%d" % q, True, AM.CERT), AM.OpR(1) if s == 3 else AM.OpR(0, b"", False, b""))
        body = AM.message(AM.Ans(AM.W2 if kind == 11 else AM.RD, ops, rid=b"rid-%d" % q, nonce=b"nonce-%d" % s))
        return E.frame(kind, body, ts=7, server_id=DM.IDS[s], msg_id=b"a-%d-%d" % (q, s), reply_to=to)

    ids, frames = _interleaved(make)
    fr, dfr, dreq, ddec, dj = _join_inputs(ids, frames)
    order, sl = _host_grouped(frames, fr, 3, 4)
    host_r = mh.ResultReplies(wire=fr.wire, resp_off=np.array([o for o, n in sl], np.uint64),
                              resp_len=np.array([n for o, n in sl], np.uint32),
                              resp_kind=np.array([mh.RR_READ if 4 <= i < 8 else mh.RR_WRITE2_ANS for i in range(12)], np.uint8),
                              req_resp_off=np.array([0, 4, 8, 12], np.uint32), n_ops=np.array([2, 2, 2], np.uint32),
                              slot_off=2 * np.arange(12, dtype=np.uint64))
    want = mh.result_reply_decode(host_r, fill=FILL)
    assert (want["resp_status"] == mh.RRS_OK).all() and (want["resp_n_ops"] == 2).all()
    dref = mh.DeviceResultReplies(host_r, 0)
    chained = mh.DeviceResultReplies(host_r, 0)
    chained.wire, chained.wire_len = dfr.wire, dfr.wire_len
    chained.resp_off, chained.resp_len, chained.resp_kind, chained.req_resp_off = dj.resp_off, dj.resp_len, dj.resp_rr_kind, dj.req_resp_off
    out_dev, out_ref = mh.DeviceResultDecoded(12, 24, fill=FILL), mh.DeviceResultDecoded(12, 24, fill=FILL)
    _sync()
    st = _stream()
    ver.envelope_decode_device(dfr, ddec, stream=st)
    ver.envelope_join_device(dreq, dfr, ddec, dj, stream=st)
    ver.result_reply_decode_device(chained, out_dev, stream=st)
    ver.result_reply_decode_device(dref, out_ref, stream=st)
    _sync()
    assert list(dj.to_host()["resp_frame"]) == order
    got, ref = out_dev.to_host(), out_ref.to_host()
    _same_arrays(got, ref)
    _same_arrays(got, want)
