"""Timing of the device Write1 reply decoder (mochi_write1_reply_decode_device).

python microbench/write1_decode_bench.py [REQS] [OPS] : the replies of ONE server to REQS
requests (default 262,144) of OPS ops (2), written by the device reply encoder: nine keys
in ten carry a current certificate, a real WriteCertificate of four MultiGrants with one
signed grant each (about 2.9 KB), drawn from a pool of 131,072 distinct ones (larger than
the Infinity Cache).  Prints one JSON line:
  the decoder's per-kernel ms (mochi_ctx_read_w1_decode_profile) and the wall ms of the
    whole call, three repetitions alternated with the Write2 decoder;
  wire bytes per second of the decoder's kernels, next to the Write2 decoder's on a
    comparable byte volume.  The library has no entry point that runs the Write2 decoder
    alone on device memory, so its time is DERIVED: the wall time of
    mochi_verify_write2_device minus that call's profiled verify stages;
  the host form's time on the first 1/16 of the responses, scaled."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "mochi-db_amd"))
import mochi_hip as mh  # noqa: E402
import workload as W  # noqa: E402

DEV = torch.device("cuda", 0)
POOL = 131072


def i64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int64)).to(DEV)


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(DEV)


def cert_pool(pool):
    """`pool` WriteCertificates of one length: a template of four MultiGrants whose
    signature bytes are redrawn per certificate (any bytes are a valid signature field)."""
    ids = W.SERVER_IDS[:4]
    g = W.encode_grant("W1_KEY_0000000", 123456789, "ab" * 64)
    sig = bytes(range(256))
    cert = b"".join(W.encode_map_entry(1, s.encode(), W.encode_multigrant([("W1_KEY_0000000", g)], s, "client-0001", "",
                                                                         [("W1_KEY_0000000", sig)])) for s in ids)
    t = np.frombuffer(cert, np.uint8)
    at = [i for i in range(len(cert) - 255) if cert[i:i + 256] == sig]
    assert len(at) == 4
    blob = torch.from_numpy(t.copy()).to(DEV).repeat(pool, 1)
    for a in at:
        blob[:, a:a + 256] = torch.randint(0, 256, (pool, 256), dtype=torch.uint8, device=DEV)
    return blob.reshape(-1), len(cert)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    n_reqs = int(sys.argv[1]) if len(sys.argv) > 1 else 262144
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    reps = 3
    pems = W.load_keys(4)
    st = torch.cuda.current_stream().cuda_stream
    # the replies, written by the device reply encoder (signatures: random bytes)
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
    del certs, ds
    ver = mh.Verifier([mh.pem_modulus(p) for p in pems], 0)
    ids4 = [b"server-1", b"server-0", b"server-2", b"server-3"]  # the replying server: key 1
    ver.set_server_ids(ids4)
    dr = mh.DeviceWrite1Replies.from_tensors(Q, Q, batch.n_ops, wire=wire, resp_off=off, resp_len=ln,
                                             resp_kind=out.req_kind, req_resp_off=i32(np.arange(Q + 1)),
                                             strings=db.strings, req_op_off=db.req_op_off, op_key_off=db.op_key_off,
                                             op_key_len=db.op_key_len)
    probe = mh.DeviceWrite1Decoded(Q, 0, 0)
    ver.write1_reply_decode_device(dr, probe, stream=st, check=False)
    dec = mh.DeviceWrite1Decoded(Q, probe.n_grants, probe.n_certs)
    assert ver.write1_reply_decode_device(dr, dec, stream=st) == mh.OK  # warm-up
    torch.cuda.synchronize()
    stat = torch.bincount(dec.resp_status[:Q].to(torch.int64), minlength=4).cpu().numpy().tolist()

    # the Write2 decoder on a comparable byte volume: 65,536 certificates' messages, tiled
    s = W.make_batch(W.build_pool(R=4, k=1, P=512, P_f=64), min(65536, max(n_reqs // 4, 32)), first_cert=1, faults=False)
    wb = W.encode_wire_batch(s)
    tiles = max(1, round(need / wb.wire.size))
    M = wb.n_msgs * tiles
    w2_wire = torch.from_numpy(wb.wire).to(DEV).repeat(tiles)
    w2_off = (i64(wb.msg_off.astype(np.int64)).repeat(tiles) +
              torch.arange(tiles, device=DEV).repeat_interleave(wb.n_msgs) * int(wb.wire.size)).contiguous()
    dwb = mh.DeviceWireBatch.from_encoded(w2_wire, w2_off, i32(wb.msg_len).repeat(tiles), M,
                                          torch.from_numpy(wb.expected_hash).to(DEV).repeat(tiles, 1))
    verdicts = mh.DeviceVerdicts(0, M, 0, full=True)
    ver.verify_write2_device(dwb, verdicts, 4, True, stream=st)  # warm-up
    torch.cuda.synchronize()
    assert bool((dwb.status[:M] == 0).all())

    ver.set_profiling(True)
    prof, call_ms, w2_wall, w2_verify = [], [], [], []
    for _ in range(reps):  # alternated
        call_ms.append(wall(lambda: ver.write1_reply_decode_device(dr, dec, stream=st)))
        prof.append(ver.read_w1_decode_profile())
        ver.read_profile()  # reset
        w2_wall.append(wall(lambda: ver.verify_write2_device(dwb, verdicts, 4, True, stream=st)))
        p = ver.read_profile()
        w2_verify.append(sum(p[x] for x in mh.Verifier.STAGES))
    ver.set_profiling(False)
    ver.close()
    kern = [sum(p.values()) for p in prof]
    w2_dec = [a - b for a, b in zip(w2_wall, w2_verify)]

    # the host form on the first 1/16 of the responses
    P16 = max(Q // 16, 1)
    h = lambda t, dt: t.cpu().numpy().view(dt)
    end = int(h(off, np.uint64)[P16 - 1]) + int(h(ln, np.uint32)[P16 - 1])
    hr = mh.Write1Replies(wire=h(wire[:end], np.uint8), resp_off=h(off[:P16], np.uint64), resp_len=h(ln[:P16], np.uint32),
                          resp_kind=h(out.req_kind[:P16], np.uint8), req_resp_off=np.arange(P16 + 1, dtype=np.uint32),
                          strings=np.asarray(batch.strings, np.uint8), req_op_off=batch.req_op_off[:P16 + 1],
                          op_key_off=batch.op_key_off[:int(batch.req_op_off[P16])],
                          op_key_len=batch.op_key_len[:int(batch.req_op_off[P16])])
    t0 = time.perf_counter()
    hd = mh.write1_reply_decode_into(hr, ids4, probe.n_grants, probe.n_certs)
    host_ms = (time.perf_counter() - t0) * 1e3
    assert hd.rc == mh.OK
    r3 = lambda v: [round(x, 3) for x in v]
    print(json.dumps({
        "bench": "write1_decode", "device": torch.cuda.get_device_name(0), "responses": Q, "ops": batch.n_ops,
        "grants": dec.n_grants, "certs": dec.n_certs, "status_counts": stat, "wire_bytes": need, "cert_bytes": cert_len,
        "cert_pool": pool, "reps": reps,
        "kernel_ms": {x: r3([p[x] for p in prof]) for x in mh.W1_DECODE_STAGES}, "kernels_ms": r3(kern),
        "call_wall_ms": r3(call_ms), "decode_GBps": r3([need / (x * 1e-3) / 1e9 for x in kern]),
        "w2_msgs": M, "w2_wire_bytes": int(w2_wire.numel()), "w2_call_wall_ms": r3(w2_wall),
        "w2_verify_stages_ms": r3(w2_verify), "w2_decode_derived_ms": r3(w2_dec),
        "w2_decode_derived_GBps": r3([w2_wire.numel() / (x * 1e-3) / 1e9 for x in w2_dec]),
        "host_responses": P16, "host_ms": round(host_ms, 3), "host_ms_scaled_to_all": round(host_ms * Q / P16, 1)}))


if __name__ == "__main__":
    main()
