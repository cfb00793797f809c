"""The server's read round with no host parser, and the client's round that consumes it.
ProtocolMessage frames of mixed payload cases in HBM (reads among Write1s) go, on one
stream, through envelope_decode_device -> envelope_route_device -> read_request_decode_device
on the case-105 run -> the host's one store lookup per distinct key -> read_answer_plan_device
-> result_reply_encode_device (ids = wire: the nonces are the decoder's slices) ->
envelope_encode_device.  The reply frames equal the host chain's, for three servers; fed to
the client chain (envelope_decode -> join -> result_reply_decode_device -> tally -> coalesce)
they yield the stored values."""
import numpy as np
import pytest

import envelope_model as E
import mochi_hip as mh
import read_request_model as RQ
import result_encode_model as AM
import workload as W
import write1_request_model as QM

pytestmark = pytest.mark.gpu

FILL = 0xA5
N_FRAMES, SERVERS = 40, (b"server-0", b"server-1", b"server-2")
READ_KIND, ANSWER_KIND = 5, 6  # payload cases 105 readToServer, 106 readFromServer
STORE = {b"key-%d" % i: RQ.KeyRec(True, True, i % 4 != 1, None if i % 4 == 1 else b"value-%d" % i, AM.padded_cert(30 + 7 * i))
         for i in range(12)}  # every fourth key was deleted: no value
STORE[b"key-5"] = RQ.KeyRec(True, True, True, b"", b"")  # an empty value under an empty certificate


def _lookup(key):
    return STORE[key]


@pytest.fixture(scope="module")
def ver():
    v = mh.Verifier([mh.pem_modulus(p) for p in W.load_keys(4)], 0)
    yield v
    v.close()


def _frames():
    """40 frames: a read of one to three keys where i % 5 is 0, 2 or 3, a Write1 elsewhere."""
    frames, reads = [], []
    for i in range(N_FRAMES):
        if i % 5 in (0, 2, 3):
            keys = [b"key-%d" % ((i + 5 * j) % 12) for j in range(1 + i % 3)]
            reads.append((E.UUID % i, keys))
            body, kind = RQ.read(b"client-%d" % (i % 4), RQ.transaction([RQ.operation(RQ.READ, k) for k in keys]), b"nonce-%d" % i), 5
        else:
            body, kind = QM.write1(b"client-%d" % (i % 4), QM.transaction([QM.operation(QM.WRITE, b"w-%d" % i)]), i + 1, QM.HASH), 7
        frames.append(E.frame(kind, body, ts=1000 + i, server_id=b"", msg_id=E.UUID % i))
    return frames, reads


def _received(frames, sid):
    """The frames packed, the server's id behind them in the same blob (ids = wire for both encoders)."""
    fr = mh.EnvelopeFrames.pack(frames, pad=1)
    wire = np.concatenate([fr.wire, np.frombuffer(sid, np.uint8)])
    return fr, wire, fr.wire.size


def _host_chain(frames, sid, n_reads):
    fr, wire, sid_off = _received(frames, sid)
    dec = mh.envelope_decode(fr)
    rt = mh.envelope_route(dec)
    lo, hi = int(rt["kind_off"][READ_KIND]), int(rt["kind_off"][READ_KIND + 1])
    assert (lo, hi) == (0, n_reads)
    reqs = mh.ReadRequests(wire=wire, msg_off=rt["body_off"][lo:hi], msg_len=rt["body_len"][lo:hi])
    rd = mh.read_request_decode(reqs)
    t = rd.trimmed()
    ks = RQ.key_state(reqs, t, _lookup)
    planned = mh.read_answer_plan(rd, ks)
    assert (planned["plan_status"] == mh.RDA_REPLY).all()
    bodies, b_off, b_len, st = mh.result_reply_encode(
        mh.read_planned_answers(wire, ks.store, planned, t["req_nonce_off"], t["req_nonce_len"]))
    assert (st == mh.ENC_OK).all()
    order = rt["order"][lo:hi]
    src = mh.EnvelopeSource(bodies=bodies, ids=wire, kind=np.full(n_reads, ANSWER_KIND, np.uint8), body_off=b_off, body_len=b_len,
                            msg_timestamp=dec["msg_timestamp"][order] + 1, reply_to_off=dec["msg_id_off"][order],
                            reply_to_len=dec["msg_id_len"][order], server_id_off=np.full(n_reads, sid_off, np.uint64),
                            server_id_len=np.full(n_reads, len(sid), np.uint32))
    out, off, ln, st = mh.envelope_encode(src)
    assert (st == mh.ENC_OK).all()
    return [out[int(o):int(o) + int(n)].tobytes() for o, n in zip(off, ln)], rd, ks


def _device_chain(ver, frames, sid, n_reads, host_rd):
    import torch

    dev = torch.device("cuda", 0)
    fr, wire, sid_off = _received(frames, sid)
    d_wire = mh._to_dev(wire, 0)
    dfr = mh.DeviceEnvelopeFrames.from_tensors(N_FRAMES, d_wire, mh._to_dev(fr.frame_off, 0), mh._to_dev(fr.frame_len, 0),
                                               wire_len=fr.wire.size)
    ddec, drt = mh.DeviceEnvelopeDecoded(N_FRAMES, fill=FILL), mh.DeviceEnvelopeRouted(N_FRAMES, fill=FILL)
    rd = mh.DeviceReadRequestsDecoded(n_reads, mh.read_request_decode_bound(wire.size, n_reads), fill=FILL)
    i64 = lambda n, v=0: torch.full((n,), v, dtype=torch.int64, device=dev)
    i32 = lambda n, v=0: torch.full((n,), v, dtype=torch.int32, device=dev)
    u8 = lambda n, v=0: torch.full((n,), v, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    torch.cuda.synchronize()  # uploads and fills went to the current stream; from here on one stream
    with torch.cuda.stream(stream):
        ver.envelope_decode_device(dfr, ddec, stream=st)
        ver.envelope_route_device(ddec, drt, stream=st)
        # the case-105 run is the first: no frame of the cases 101..104 was sent
        reqs = mh.DeviceReadRequests.from_tensors(n_reads, wire=d_wire, msg_off=drt.body_off[:n_reads], msg_len=drt.body_len[:n_reads])
        assert ver.read_request_decode_device(reqs, rd, stream=st) == mh.OK
        # the host's part: one lookup per distinct key (the decoder's call has waited for n_ops already)
        stream.synchronize()
        got = rd.to_host()
        RQ.assert_equal(got.trimmed(), host_rd.trimmed())
        ks = RQ.key_state(mh.ReadRequests(wire=wire, msg_off=np.zeros(0, np.uint64), msg_len=np.zeros(0, np.uint32)),
                          got.trimmed(), _lookup)
        dks = mh.DeviceReadKeyState(ks, 0)
        planned = mh.DeviceReadAnswerPlanned(n_reads, rd.n_ops, fill=FILL)
        mh.read_answer_plan_device(rd, dks, planned, stream=st)
        da = planned.answers(reqs, rd, dks)
        bodies = u8(max(mh.result_reply_encode_bound(da), 1), FILL)
        b_off, b_len, b_st = i64(n_reads), i32(n_reads), u8(n_reads, FILL)
        rc, total = ver.result_reply_encode_device(da, bodies, b_off, b_len, b_st, stream=st)
        assert rc == mh.OK
        order = drt.order[:n_reads].long()
        src = mh.DeviceEnvelopeSource.from_tensors(
            n_reads, bodies=bodies, ids=d_wire, kind=u8(n_reads, ANSWER_KIND), body_off=b_off, body_len=b_len,
            msg_timestamp=ddec.msg_timestamp[order] + 1, reply_to_off=ddec.msg_id_off[order], reply_to_len=ddec.msg_id_len[order],
            server_id_off=i64(n_reads, sid_off), server_id_len=i32(n_reads, len(sid)))
        out = u8(mh.envelope_encode_bound(n_reads, int(bodies.numel()), int(d_wire.numel())), FILL)
        f_off, f_len, f_st = i64(n_reads), i32(n_reads), u8(n_reads, FILL)
        rc, total = ver.envelope_encode_device(src, out, f_off, f_len, f_st, stream=st)
        assert rc == mh.OK
        stream.synchronize()
    assert (b_st.cpu().numpy() == mh.ENC_OK).all() and (f_st.cpu().numpy() == mh.ENC_OK).all()
    assert (planned.to_host()["plan_status"] == mh.RDA_REPLY).all()
    o = out.cpu().numpy()
    return [o[int(a):int(a) + int(n)].tobytes() for a, n in zip(f_off.cpu().numpy(), f_len.cpu().numpy())]


def test_read_chain_server_and_client(ver):
    import torch

    frames, reads = _frames()
    Q, R = len(reads), len(SERVERS)
    assert Q == 24 and len(frames) == N_FRAMES
    replies = []
    for sid in SERVERS:
        host_frames, host_rd, _ = _host_chain(frames, sid, Q)
        assert host_rd.n_keys == 12 < host_rd.n_ops
        dev_frames = _device_chain(ver, frames, sid, Q, host_rd)
        assert dev_frames == host_frames
        for (msg_id, keys), f in zip(reads, dev_frames):  # what the frames say, by the models
            p = E.parse(f)
            sl = lambda s: f[s[0]:s[0] + s[1]]
            assert (p.status, p.kind, sl(p.server_id), sl(p.reply_to)) == (E.OK, ANSWER_KIND, sid, msg_id)
            want = AM.Ans(AM.RD, tuple(AM.OpR(0, STORE[k].value or b"", STORE[k].available, STORE[k].cert) for k in keys),
                          nonce=b"nonce-%d" % int(msg_id[-2:]))
            assert sl(p.body) == AM.message(want)
        replies += dev_frames
    # the client: every server's reply frames in arrival order (server-major) -> the stored values
    dev = torch.device("cuda", 0)
    fr = mh.EnvelopeFrames.pack(replies, pad=3)
    dfr, dreq = mh.DeviceEnvelopeFrames(fr), mh.DeviceEnvelopeRequests([m for m, _ in reads])
    n = len(replies)
    ddec, dj = mh.DeviceEnvelopeDecoded(n, fill=FILL), mh.DeviceEnvelopeJoined(n, Q, fill=FILL)
    k = np.array([len(keys) for _, keys in reads], np.uint32)
    out_off = np.concatenate([[0], np.cumsum(k)[:-1]]).astype(np.uint64)
    slot_off = np.concatenate([[0], np.cumsum(np.repeat(k, R))[:-1]]).astype(np.uint64)
    n_out, n_slots = int(k.sum()), int(k.sum()) * R
    host_r = mh.ResultReplies(wire=fr.wire, resp_off=np.zeros(n, np.uint64), resp_len=np.zeros(n, np.uint32),
                              resp_kind=np.zeros(n, np.uint8), req_resp_off=np.zeros(Q + 1, np.uint32), n_ops=k, slot_off=slot_off)
    dr = mh.DeviceResultReplies(host_r, 0)  # n_ops and slot_off are the client's own; the rest comes from the join
    dr.wire, dr.resp_off, dr.resp_len, dr.resp_kind, dr.req_resp_off = dfr.wire, dj.resp_off, dj.resp_len, dj.resp_rr_kind, dj.req_resp_off
    drd, dco = mh.DeviceResultDecoded(n, n_slots, fill=FILL), mh.DeviceResultCoalesced(n_out, fill=FILL)
    d_off = mh._to_dev(out_off, 0)
    d_chosen = torch.full((n_out,), -1, dtype=torch.int32, device=dev)
    d_reason, d_bits = torch.zeros(Q, dtype=torch.uint8, device=dev), torch.zeros((Q + 31) // 32, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    torch.cuda.synchronize()
    ver.envelope_decode_device(dfr, ddec, stream=st)
    ver.envelope_join_device(dreq, dfr, ddec, dj, stream=st)
    ver.result_reply_decode_device(dr, drd, stream=st)
    rc = mh.load_library().mochi_tally_responses_device(Q, dr.req_resp_off.data_ptr(), dr.n_ops.data_ptr(), drd.resp_n_ops.data_ptr(),
                                                        dr.slot_off.data_ptr(), drd.op_status.data_ptr(), d_off.data_ptr(), R,
                                                        d_chosen.data_ptr(), d_reason.data_ptr(), d_bits.data_ptr(), st)
    assert rc == mh.OK
    mh.result_coalesce_device(dr, drd, d_chosen, d_off, d_bits, d_off, dco, stream=st)
    torch.cuda.synchronize()
    assert dj.to_host()["req_resp_off"].tolist() == [R * q for q in range(Q + 1)]
    assert mh.unpack_bits(d_bits.cpu().numpy().view(np.uint32), Q).all() and (d_reason.cpu().numpy() == 0).all()
    co, wire = dco.to_host(), fr.wire.tobytes()
    i = 0
    for _, keys in reads:
        for key in keys:
            rec = STORE[key]
            assert wire[int(co["result_off"][i]):][:int(co["result_len"][i])] == (rec.value or b""), key
            assert (int(co["status"][i]), bool(co["existed"][i])) == (0, rec.available), key
            assert co["flags"][i] & mh.RRO_HAS_CERT and wire[int(co["cert_off"][i]):][:int(co["cert_len"][i])] == rec.cert, key
            i += 1
    assert i == n_out
