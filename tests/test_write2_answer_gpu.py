"""Write2 answer plan on the GPU (mochi_write2_answer_plan_device) and the rounds it closes:
the device plan equals the host plan on the CPU case set; the server's Write2 round on one
stream -- bodies -> mochi_verify_write2_device -> plan -> mochi_result_reply_encode_device
in the device capacity mode, one synchronise at the end -- gives the bytes the Python
server model builds; and four such servers' answers go on, on the same stream, through
mochi_result_reply_decode_device -> mochi_tally_responses_device ->
mochi_result_coalesce_device to what the plain-Python client makes of the model's bytes."""
import numpy as np
import pytest

import mochi_hip as mh
import result_encode_model as E
import result_reply_model as RRM
import workload as W
import write1_decode_model as DM
import write2_answer_model as A

pytestmark = pytest.mark.gpu

FILL = A.FILL
R = 4


@pytest.fixture(scope="module")
def pool():
    return W.build_pool(R=R, k=2, P=256, P_f=64)


@pytest.fixture(scope="module")
def ver(pool):
    v = mh.Verifier(pool.moduli, 0)
    v.set_server_ids(W.SERVER_IDS[:R])
    yield v
    v.close()


# 1. device plan == host plan ---------------------------------------------------------------------
class _Verdicts:
    """Stands in for DeviceVerdicts: the two arrays the plan reads."""

    def __init__(self, bits, dec):
        self.cert_accept_bits, self.op_decision = mh._to_dev(bits, 0), mh._to_dev(dec, 0)


@pytest.mark.parametrize("slots", ["dense", "guarded"])
def test_device_plan_equals_host_plan(slots):
    import torch

    txs = A.cases()
    wb, ms, bits, dec, st = A.batch(txs, slots)
    host = mh.write2_answer_plan(wb, ms, bits, dec, st, fill=FILL)
    RRM.assert_equal(host, A.expected(txs, wb, st))
    dwb = mh.DeviceWireBatch(wb, 0)
    dwb.status = mh._to_dev(ms, 0)
    out = mh.DeviceWrite2AnswerPlanned(len(txs), st.n_slots, fill=FILL)
    dv, dst = _Verdicts(bits, dec), mh.DeviceWrite2AnswerStore(st, 0)  # referenced until the synchronise below
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    mh.write2_answer_plan_device(dwb, dv, dst, out, stream=s.cuda_stream)
    torch.cuda.synchronize()
    RRM.assert_equal(out.to_host(), host)


@pytest.mark.parametrize("M", [1, 255, 256, 257])
def test_message_counts_around_the_block_edge(M):
    import torch

    pool_ = A.cases()
    txs = [pool_[(5 * i) % len(pool_)] for i in range(M)]
    wb, ms, bits, dec, st = A.batch(txs, "guarded")
    host = mh.write2_answer_plan(wb, ms, bits, dec, st, fill=FILL)
    dwb = mh.DeviceWireBatch(wb, 0)
    dwb.status = mh._to_dev(ms, 0)
    out = mh.DeviceWrite2AnswerPlanned(M, st.n_slots, fill=FILL)
    dv, dst = _Verdicts(bits, dec), mh.DeviceWrite2AnswerStore(st, 0)
    torch.cuda.synchronize()
    mh.write2_answer_plan_device(dwb, dv, dst, out)
    torch.cuda.synchronize()
    RRM.assert_equal(out.to_host(), host)


# 2. the rounds --------------------------------------------------------------------------------------
def _grant_ts_of_ops(s):
    """Per op: the timestamp of its certificate's first grant for the op's key slot."""
    b = s.batch
    out = np.zeros(b.n_ops, np.int64)
    for c in range(b.n_certs):
        g0, g1 = int(b.cert_grant_off[c]), int(b.cert_grant_off[c + 1])
        for o in range(int(b.cert_op_off[c]), int(b.cert_op_off[c + 1])):
            for g in range(g0, g1):
                if b.grant_key[g] == b.op_key[o]:
                    gb = b.grant_bytes[int(b.grant_off[g]):int(b.grant_off[g]) + int(b.grant_len[g])].tobytes()
                    out[o] = DM.parse_grant(gb, 0, len(gb)).ts
                    break
    return out


def _messages(pool, n):
    """n Write2ToServer bodies at R = 4, two operations each; two of them carry two forged
    signatures (below the quorum), whatever faults the seeded stream holds besides."""
    s = W.make_batch(pool, n, first_cert=500)
    b = s.batch
    for c in (3, n - 5):
        g0 = int(b.cert_grant_off[c])
        b.sig[g0:g0 + 2 * pool.k, 17] ^= 0x40  # the grants of the first two replicas
    return s, W.encode_wire_batch(s, pad=3)


def _server_view(wb, base_ts, server, rng):
    """One server's snapshot: which ops it holds (LOCAL), which keys have a stored certificate
    and with what timestamp (read iff stored > the grant's), its stored values and certificates."""
    import copy

    O_ = int(wb.op_flags_off[-1])
    v = copy.copy(wb)
    flags = rng.choice(np.array([3, 3, 3, 7, 7, 7, 7, 2], np.uint8), O_)  # LOCAL|SVOC, +HAS_CURRENT_C, or another shard's
    flags[(np.arange(O_) + server) % 11 == 0] = 2
    v.op_flags = flags
    v.op_object_ts = base_ts + rng.integers(-2, 3, O_)
    store = tuple(A.Stored(b"stored-%d-%d" % (server, i) if i % 7 else b"", RRM.cert(1, 3) if flags[i] & 4 else None)
                  for i in range(O_))
    return v, store


def _enqueue_round(ver, v, store, rids, stream, cap, wire=None):
    """verify -> plan -> encode (device capacity mode) for one server's view, all on `stream`.
    Returns the device objects; nothing is waited for after the verify call's own totals."""
    import torch

    M, O_ = v.n_msgs, int(v.op_flags_off[-1])
    _, _, _, _, st = A.batch([A.Tx("", b"", (mh.OPD_APPLY,) * int(k), store[int(o):int(o) + int(k)])
                              for o, k in zip(v.op_flags_off[:-1], np.diff(v.op_flags_off.astype(np.int64)))], "guarded")
    dwb = mh.DeviceWireBatch(v, 0)
    dv = mh.DeviceVerdicts(0, M, 0, full=True, n_ops=O_)
    dst = mh.DeviceWrite2AnswerStore(st, 0)
    planned = mh.DeviceWrite2AnswerPlanned(M, st.n_slots, fill=FILL)
    rid_blob = b"".join(rids)
    rid_len = np.array([len(r) for r in rids], np.uint32)
    rid_off = np.concatenate([[0], np.cumsum(rid_len)[:-1]]).astype(np.uint64)
    ids, d_off, d_len = mh._to_dev(np.frombuffer(rid_blob, np.uint8), 0), mh._to_dev(rid_off, 0), mh._to_dev(rid_len, 0)
    dev = torch.device("cuda", 0)
    if wire is None:
        wire = torch.full((cap,), 0xEE, dtype=torch.uint8, device=dev)
    off = torch.zeros(M, dtype=torch.int64, device=dev)
    ln = torch.zeros(M, dtype=torch.int32, device=dev)
    status = torch.full((M,), 0xEE, dtype=torch.uint8, device=dev)
    total = torch.full((1,), -1, dtype=torch.int64, device=dev)
    torch.cuda.current_stream().synchronize()  # the uploads and fills above went there; `stream` is not waited for
    ver.verify_write2_device(dwb, dv, R, True, stream=stream)
    mh.write2_answer_plan_device(dwb, dv, dst, planned, stream=stream)
    answers = planned.answers(dwb, dst, ids=ids, rid_off=d_off, rid_len=d_len)
    rc, _ = ver.result_reply_encode_device(answers, wire, off, ln, status, stream=stream, wire_len_dev=total)
    assert rc == mh.OK
    # every device array stays referenced until the caller has synchronised: nothing waited for the kernels that read
    # them, and a freed tensor's memory would go to the next upload on the current stream
    return dict(dwb=dwb, dv=dv, st=st, planned=planned, wire=wire, off=off, ln=ln, status=status, total=total,
                keep=(dst, ids, d_off, d_len, answers))


def _model_answers(v, store, rids, d):
    """The Python server's answers for the view, from the verdicts the device gave (downloaded
    after the round's one synchronise): [E.Ans], OTHER where no reply is sent."""
    h = d["dv"].to_host()
    ms = d["dwb"].status.cpu().numpy()
    acc = mh.unpack_bits(h.cert_accept_bits, v.n_msgs)
    wire = v.wire.tobytes()
    out = []
    for m in range(v.n_msgs):
        o0, o1 = int(v.op_flags_off[m]), int(v.op_flags_off[m + 1])
        body = wire[int(v.msg_off[m]):int(v.msg_off[m]) + int(v.msg_len[m])]
        t = A.Tx("m%d" % m, body, tuple(h.op_decision[o0:o1].tolist()), store[o0:o1], int(ms[m]), bool(acc[m]))
        a = A.server_answer(t)
        out.append(a._replace(rid=rids[m]) if a is not None else E.Ans(E.OTHER))
    return out, h, acc


def test_the_servers_write2_round_on_one_stream(ver, pool):
    import torch

    n = 40
    s, wb = _messages(pool, n)
    v, store = _server_view(wb, _grant_ts_of_ops(s), 0, np.random.default_rng(5))
    rids = [b"rid-%d" % m for m in range(n)]
    stream = torch.cuda.Stream()
    d = _enqueue_round(ver, v, store, rids, stream.cuda_stream, cap=1 << 20)
    torch.cuda.synchronize()  # the one wait
    answers, h, acc = _model_answers(v, store, rids, d)
    w_wire, w_off, w_ln, w_st = E.expected_arrays(answers)
    need = int(d["total"].item())
    assert need == w_wire.size
    np.testing.assert_array_equal(d["ln"].cpu().numpy().view(np.uint32), w_ln)
    np.testing.assert_array_equal(d["off"].cpu().numpy().view(np.uint64), w_off)
    np.testing.assert_array_equal(d["status"].cpu().numpy(), w_st)
    got = d["wire"].cpu().numpy()
    assert got[:need].tobytes() == w_wire.tobytes() and (got[need:] == 0xEE).all()
    # the batch held what it was built to hold
    plan = d["planned"].to_host()["plan_status"]
    assert 0 < int((plan == mh.W2A_NO_REPLY).sum()) < n and not acc[3] and not acc[n - 5]
    replied = np.repeat(plan == mh.W2A_REPLY, 2)
    assert {mh.OPD_APPLY, mh.OPD_READ, mh.OPD_WRONG_SHARD} <= set(h.op_decision[replied].tolist())
    # and every answer reads back as the values the model holds
    for m, a in enumerate(answers):
        if a.kind == E.OTHER:
            continue
        body = got[int(w_off[m]):int(w_off[m]) + int(w_ln[m])].tobytes()
        assert RRM.decode_body(body, E.W2, len(a.ops)).status == mh.RRS_OK


def test_four_servers_answers_close_the_loop(ver, pool):
    """Q transactions, four servers each with its own shard map and store: every server's round,
    then the client's closing round over the 4 * Q answers where they lie, on one stream."""
    import torch

    lib = mh.load_library()
    Q, k, cap = 12, 2, 1 << 17
    s, wb = _messages(pool, Q)
    base_ts = _grant_ts_of_ops(s)
    rids = [b"rid-%d" % m for m in range(Q)]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream()
    wire = torch.full((R * cap,), 0, dtype=torch.uint8, device=dev)
    views = [_server_view(wb, base_ts, srv, np.random.default_rng(40 + srv)) for srv in range(R)]
    rounds = [_enqueue_round(ver, v, store, rids, stream.cuda_stream, cap, wire[srv * cap:(srv + 1) * cap])
              for srv, (v, store) in enumerate(views)]
    # response p = 4 * q + server: where the servers' answers lie in the one blob (stream-ordered tensor ops)
    with torch.cuda.stream(stream):
        resp_off = torch.stack([d["off"] + srv * cap for srv, d in enumerate(rounds)], 1).reshape(-1).contiguous()
        resp_len = torch.stack([d["ln"] for d in rounds], 1).reshape(-1).contiguous()
        resp_kind = torch.stack([d["planned"].resp_kind[:Q] for d in rounds], 1).reshape(-1).contiguous()
    P = R * Q
    slot_off = (np.arange(P, dtype=np.uint64) * np.uint64(k + 1))  # a guard slot between the runs
    n_slots = P * (k + 1)
    dr = mh.DeviceResultReplies.__new__(mh.DeviceResultReplies)
    dr.n_resps, dr.n_reqs, dr.wire_len = P, Q, R * cap
    dr.wire, dr.resp_off, dr.resp_len, dr.resp_kind = wire, resp_off, resp_len, resp_kind
    dr.req_resp_off = mh._to_dev(np.arange(Q + 1, dtype=np.uint32) * np.uint32(R), 0)
    dr.n_ops = mh._to_dev(np.full(Q, k, np.uint32), 0)
    dr.slot_off = mh._to_dev(slot_off, 0)
    dec = mh.DeviceResultDecoded(P, n_slots, fill=FILL)
    out_off = np.arange(Q, dtype=np.uint64) * np.uint64(k)
    chosen_off = out_off.copy()
    co = mh.DeviceResultCoalesced(Q * k, fill=FILL)
    d_out_off, d_chosen_off = mh._to_dev(out_off, 0), mh._to_dev(chosen_off, 0)
    chosen = torch.full((Q * k,), -1, dtype=torch.int32, device=dev)
    reason = torch.full((Q,), FILL, dtype=torch.uint8, device=dev)
    bits = torch.full(((Q + 31) // 32,), -1, dtype=torch.int32, device=dev)
    torch.cuda.current_stream().synchronize()  # the uploads above; the rounds' stream is not waited for
    ver.result_reply_decode_device(dr, dec, stream=stream.cuda_stream)
    rc = lib.mochi_tally_responses_device(Q, dr.req_resp_off.data_ptr(), dr.n_ops.data_ptr(), dec.resp_n_ops.data_ptr(),
                                          dr.slot_off.data_ptr(), dec.op_status.data_ptr(), d_chosen_off.data_ptr(), R,
                                          chosen.data_ptr(), reason.data_ptr(), bits.data_ptr(), stream.cuda_stream)
    assert rc == mh.OK
    mh.result_coalesce_device(dr, dec, chosen, d_chosen_off, bits, d_out_off, co, stream=stream.cuda_stream)
    torch.cuda.synchronize()
    assert all(0 < int(d["total"].item()) <= cap for d in rounds)
    # the model: every server's answers as bytes, laid out where the device put them
    blob = bytearray(R * cap)
    offs, lens, kinds = np.zeros((Q, R), np.uint64), np.zeros((Q, R), np.uint32), np.zeros((Q, R), np.uint8)
    for srv, ((v, store), d) in enumerate(zip(views, rounds)):
        answers, _, _ = _model_answers(v, store, rids, d)
        bodies, st = E.expected(answers)
        at = srv * cap
        for q, (a, b) in enumerate(zip(answers, bodies)):
            blob[at:at + len(b)] = b
            offs[q, srv], lens[q, srv], kinds[q, srv] = at, len(b), a.kind
            at += len(b)
    assert bytes(blob) == wire.cpu().numpy().tobytes()
    r = mh.ResultReplies(wire=np.frombuffer(bytes(blob), np.uint8), resp_off=offs.reshape(-1), resp_len=lens.reshape(-1),
                         resp_kind=kinds.reshape(-1), req_resp_off=np.arange(Q + 1, dtype=np.uint32) * np.uint32(R),
                         n_ops=np.full(Q, k, np.uint32), slot_off=slot_off)
    accept, why, want = RRM.client(r, R, out_off, Q * k, FILL)
    np.testing.assert_array_equal(mh.unpack_bits(bits.cpu().numpy().view(np.uint32), Q), accept)
    np.testing.assert_array_equal(reason.cpu().numpy(), why)
    RRM.assert_equal(co.to_host(), want)
    assert accept.any() and not accept.all()
