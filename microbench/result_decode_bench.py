"""Timing of the device result reply decoder (mochi_result_reply_decode_device).

python microbench/result_decode_bench.py [REQS] [OPS] : ONE server's Write2AnsFromServer
bodies to REQS requests (default 262,144) of OPS ops (2), every OperationResult with a
current certificate, a real WriteCertificate of four MultiGrants with one signed grant
each (about 2.9 KB), drawn from a pool of 131,072 distinct ones as in
write1_decode_bench.py.  Prints one JSON line:
  the decoder's per-kernel ms (mochi_ctx_read_result_decode_profile) and the wall ms of the
    whole call, three repetitions alternated with mochi_write1_reply_decode_device on a
    comparable wire volume (the replies of write1_decode_bench.py);
  wire bytes per second of both decoders' kernels;
  the wall ms of decode -> mochi_tally_responses_device -> mochi_result_coalesce_device on
    one stream, up to the return of the third call and up to a trailing synchronise;
  the host form's time on the first 1/16 of the responses, scaled."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "mochi-db_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mochi_hip as mh  # noqa: E402
import workload as W  # noqa: E402
from write1_decode_bench import DEV, POOL, cert_pool, i32, i64, wall  # noqa: E402


def varint(v):
    out = b""
    while v >= 0x80:
        out += bytes([v & 0x7F | 0x80])
        v >>= 7
    return out + bytes([v])


def ld(tag, payload):
    return bytes([tag]) + varint(len(payload)) + payload


def write2_answers(n_reqs, k, certs, cert_len, pool):
    """The bodies on the device: one template (k OperationResults with result, certificate and
    existed; a rid), the certificate of op (q, j) copied in from the pool."""
    marks = [bytes([0xC0 + j]) * cert_len for j in range(k)]
    ops = [ld(0x0A, b"value-%02d" % j) + ld(0x12, marks[j]) + b"\x18\x01" for j in range(k)]
    body = ld(0x0A, b"".join(ld(0x0A, o) for o in ops)) + ld(0x12, b"rid-00000001")
    at = [body.index(m) for m in marks]
    wire = torch.from_numpy(np.frombuffer(body, np.uint8).copy()).to(DEV).repeat(n_reqs, 1)
    cp = certs.reshape(pool, cert_len)
    for j, a in enumerate(at):
        idx = (torch.arange(n_reqs, device=DEV) * k + j) * 2654435761 % pool
        wire[:, a:a + cert_len] = cp[idx]
    return wire.reshape(-1), len(body)


def f8_replies(n_reqs, k, pems, st):
    """The Write1 replies of write1_decode_bench.py, ready for mochi_write1_reply_decode_device."""
    batch = W.make_write1_batch(n_reqs, k, 0.1)
    host = mh.write1_issue(batch)
    signer = mh.DeviceSigner(pems[0], 0)
    db = mh.DeviceWrite1Batch(batch, 0)
    certs, cert_len = cert_pool(min(POOL, max(n_reqs, 16)))
    pool = certs.numel() // cert_len
    obj = batch.op_obj.astype(np.int64)
    has = (obj * 2654435761 % 10) != 0
    S, Q = batch.n_stored, batch.n_reqs
    ids = np.frombuffer(b"server-0client-0001", np.uint8).copy()
    ds = mh.DeviceWrite1ReplySource.from_tensors(
        0, 8, ids=torch.from_numpy(ids).to(DEV), req_client_off=i64(np.full(Q, 8)), req_client_len=i32(np.full(Q, 11)),
        stored_bytes=torch.from_numpy(np.frombuffer(b"\x0a\x03old\x10\x05", np.uint8).copy()).to(DEV).repeat(max(S, 1)),
        stored_off=i64(np.arange(max(S, 1)) * 7), stored_len=i32(np.full(max(S, 1), 7)),
        stored_sig=torch.randint(0, 256, (max(S, 1), 256), dtype=torch.uint8, device=DEV), certs=certs,
        op_cert_off=i64((obj % pool) * cert_len), op_cert_len=i32(np.where(has, cert_len, 0)))
    out = mh.DeviceWrite1Issued(Q, batch.n_ops, host.grant_bytes_len, sign=False)
    signer.issue_device(db, out, stream=st)
    out.sig = torch.randint(0, 256, (batch.n_ops, 256), dtype=torch.uint8, device=DEV)
    off = torch.zeros(Q, dtype=torch.int64, device=DEV)
    ln = torch.zeros(Q, dtype=torch.int32, device=DEV)
    status = torch.zeros(Q, dtype=torch.uint8, device=DEV)
    rc, need = signer.reply_encode_device(db, out, ds, None, off, ln, status, stream=st, check=False)
    wire = torch.zeros(need, dtype=torch.uint8, device=DEV)
    signer.reply_encode_device(db, out, ds, wire, off, ln, status, stream=st)
    torch.cuda.synchronize()
    signer.close()
    dr = mh.DeviceWrite1Replies.from_tensors(Q, Q, batch.n_ops, wire=wire, resp_off=off, resp_len=ln,
                                             resp_kind=out.req_kind, req_resp_off=i32(np.arange(Q + 1)),
                                             strings=db.strings, req_op_off=db.req_op_off, op_key_off=db.op_key_off,
                                             op_key_len=db.op_key_len)
    return dr, need, (db, out)


def main():
    n_reqs = int(sys.argv[1]) if len(sys.argv) > 1 else 262144
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    reps = 3
    pems = W.load_keys(4)
    lib = mh.load_library()
    st = torch.cuda.current_stream().cuda_stream
    ver = mh.Verifier([mh.pem_modulus(p) for p in pems], 0)
    ver.set_server_ids([b"server-1", b"server-0", b"server-2", b"server-3"])
    # f8's input and outputs
    w1r, w1_bytes, keep = f8_replies(n_reqs, k, pems, st)
    probe = mh.DeviceWrite1Decoded(n_reqs, 0, 0)
    ver.write1_reply_decode_device(w1r, probe, stream=st, check=False)
    w1dec = mh.DeviceWrite1Decoded(n_reqs, probe.n_grants, probe.n_certs)
    assert ver.write1_reply_decode_device(w1r, w1dec, stream=st) == mh.OK  # warm-up
    # the Write2 answers: one response per request
    certs, cert_len = cert_pool(min(POOL, max(n_reqs, 16)))
    pool = certs.numel() // cert_len
    wire, body_len = write2_answers(n_reqs, k, certs, cert_len, pool)
    del certs
    Q = P = n_reqs
    r = mh.DeviceResultReplies.__new__(mh.DeviceResultReplies)
    r.n_resps, r.n_reqs, r.wire_len = P, Q, int(wire.numel())
    r.wire, r.resp_off, r.resp_len = wire, i64(np.arange(P, dtype=np.int64) * body_len), i32(np.full(P, body_len))
    r.resp_kind = torch.zeros(P, dtype=torch.uint8, device=DEV)
    r.req_resp_off, r.n_ops, r.slot_off = i32(np.arange(Q + 1)), i32(np.full(Q, k)), i64(np.arange(P, dtype=np.int64) * k)
    dec = mh.DeviceResultDecoded(P, P * k)
    co = mh.DeviceResultCoalesced(Q * k)
    chosen = torch.full((Q * k,), -1, dtype=torch.int32, device=DEV)
    reason = torch.zeros(Q, dtype=torch.uint8, device=DEV)
    bits = torch.zeros((Q + 31) // 32, dtype=torch.int32, device=DEV)
    ver.result_reply_decode_device(r, dec, stream=st)  # warm-up
    torch.cuda.synchronize()
    stat = torch.bincount(dec.resp_status[:P].to(torch.int64), minlength=3).cpu().numpy().tolist()
    assert stat == [P, 0, 0] and bool((dec.op_flags[:P * k] == mh.RRO_HAS_CERT).all())

    def chain():
        ver.result_reply_decode_device(r, dec, stream=st)
        # R = 1: the one server's answer is the majority
        rc = lib.mochi_tally_responses_device(Q, r.req_resp_off.data_ptr(), r.n_ops.data_ptr(), dec.resp_n_ops.data_ptr(),
                                              r.slot_off.data_ptr(), dec.op_status.data_ptr(), r.slot_off.data_ptr(), 1,
                                              chosen.data_ptr(), reason.data_ptr(), bits.data_ptr(), st)
        assert rc == mh.OK
        mh.result_coalesce_device(r, dec, chosen, r.slot_off, bits, r.slot_off, co, stream=st)

    chain()
    torch.cuda.synchronize()
    assert bool((co.resp[:Q * k].view(Q, k) == torch.arange(Q, device=DEV, dtype=torch.int32)[:, None]).all())

    ver.set_profiling(True)
    prof, call_ms, w1_prof, w1_call = [], [], [], []
    for _ in range(reps):  # alternated
        call_ms.append(wall(lambda: ver.result_reply_decode_device(r, dec, stream=st)))
        prof.append(ver.read_result_decode_profile())
        w1_call.append(wall(lambda: ver.write1_reply_decode_device(w1r, w1dec, stream=st)))
        w1_prof.append(ver.read_w1_decode_profile())
    ver.set_profiling(False)
    enq_ms, chain_ms = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        chain()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        enq_ms.append((t1 - t0) * 1e3)
        chain_ms.append((time.perf_counter() - t0) * 1e3)
    ver.close()
    kern = [sum(p.values()) for p in prof]
    w1_kern = [sum(p.values()) for p in w1_prof]

    # the host form on the first 1/16 of the responses, one thread
    P16 = max(P // 16, 1)
    h = lambda t, dt: t.cpu().numpy().view(dt)
    hr = mh.ResultReplies(wire=h(wire[:P16 * body_len], np.uint8), resp_off=h(r.resp_off[:P16], np.uint64),
                          resp_len=h(r.resp_len[:P16], np.uint32), resp_kind=np.zeros(P16, np.uint8),
                          req_resp_off=np.arange(P16 + 1, dtype=np.uint32), n_ops=np.full(P16, k, np.uint32),
                          slot_off=h(r.slot_off[:P16], np.uint64))
    t0 = time.perf_counter()
    hd = mh.result_reply_decode(hr)
    host_ms = (time.perf_counter() - t0) * 1e3
    assert not hd["resp_status"].any()
    need = int(wire.numel())
    r3 = lambda v: [round(x, 3) for x in v]
    print(json.dumps({
        "bench": "result_decode", "device": torch.cuda.get_device_name(0), "responses": P, "ops": P * k,
        "wire_bytes": need, "body_bytes": body_len, "cert_bytes": cert_len, "cert_pool": pool, "reps": reps,
        "kernel_ms": {x: r3([p[x] for p in prof]) for x in mh.RESULT_DECODE_STAGES}, "kernels_ms": r3(kern),
        "call_wall_ms": r3(call_ms), "decode_GBps": r3([need / (x * 1e-3) / 1e9 for x in kern]),
        "w1_wire_bytes": w1_bytes, "w1_kernel_ms": {x: r3([p[x] for p in w1_prof]) for x in mh.W1_DECODE_STAGES},
        "w1_kernels_ms": r3(w1_kern), "w1_call_wall_ms": r3(w1_call),
        "w1_decode_GBps": r3([w1_bytes / (x * 1e-3) / 1e9 for x in w1_kern]),
        "chain_enqueue_ms": r3(enq_ms), "chain_with_synchronise_ms": r3(chain_ms),
        "host_responses": P16, "host_ms": round(host_ms, 3), "host_ms_scaled_to_all": round(host_ms * P / P16, 1)}))


if __name__ == "__main__":
    main()
