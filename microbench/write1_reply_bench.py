"""Timing of the device Write1 reply encoder (mochi_write1_reply_encode_device)
behind the issue + sign call whose outputs it reads.

python microbench/write1_reply_bench.py [REQS] [OPS] [CERT_BYTES] : REQS requests
(default 262,144) of OPS ops (2); nine keys in ten have a current certificate of
CERT_BYTES bytes (2,900: four MultiGrants of one signed grant each), drawn from
a pool of 131,072 distinct certificates (larger than the Infinity Cache).
Prints one JSON line:
  wall ms per batch of issue+sign alone and of issue+sign+reply in both capacity
    modes (three alternated repetitions each, host clock around calls that end
    in a synchronise), and the reply's added share;
  the reply encoder's per-kernel ms (mochi_signer_read_reply_profile);
  k_w1r_copy's bytes read + written per second next to k_enc_copy's of the Write2
    encoder on a comparable byte volume (the same grants, eight times over),
    three alternated repetitions each;
  the single-request case: issue+sign against issue+sign+reply (no host wait)."""
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


def reply_source(batch, cert_bytes, pool=POOL):
    """Certificates by container (ops on one key share one), stored grants of 150
    opaque bytes, one client id for all, everything made on the device."""
    obj = batch.op_obj.astype(np.int64)
    has = (obj * 2654435761 % 10) != 0
    ids = np.frombuffer(b"server-0client-0001", np.uint8).copy()
    S, Q = batch.n_stored, batch.n_reqs
    return mh.DeviceWrite1ReplySource.from_tensors(
        0, 8, ids=torch.from_numpy(ids).to(DEV), req_client_off=i64(np.full(Q, 8)), req_client_len=i32(np.full(Q, 11)),
        stored_bytes=torch.randint(0, 256, (max(S, 1) * 150,), dtype=torch.uint8, device=DEV),
        stored_off=i64(np.arange(max(S, 1)) * 150), stored_len=i32(np.full(max(S, 1), 150)),
        stored_sig=torch.randint(0, 256, (max(S, 1), 256), dtype=torch.uint8, device=DEV),
        certs=torch.randint(0, 256, (pool * cert_bytes,), dtype=torch.uint8, device=DEV),
        op_cert_off=i64((obj % pool) * cert_bytes), op_cert_len=i32(np.where(has, cert_bytes, 0))), has


def payload_bytes(batch, host, cert_len, k):
    """Bytes of the grant, signature and certificate runs of every reply entry."""
    Q = batch.n_reqs
    kind = np.repeat(host.req_kind, k)
    d = host.op_decision
    listed = np.where(kind == mh.W1K_OK, (d == mh.W1D_NEW) | (d == mh.W1D_RETRY) | (d == mh.W1D_WRONG_SHARD),
                      (kind == mh.W1K_REFUSED) & (d == mh.W1D_REFUSED))
    first = listed.copy()
    j_in_req = np.tile(np.arange(k), Q)
    for j in range(1, k):  # an earlier listed op of the request with the same grant
        same = np.zeros_like(first)
        same[j:] = listed[:-j] & (host.op_grant[j:] == host.op_grant[:-j])
        first &= ~(same & (j_in_req >= j))
    assert int(first.sum()) == int(host.req_grant_off[Q])
    g = host.op_grant[first]
    st = (g & mh.W1_STORED) != 0
    glen = np.where(st, 150, host.grant_len[np.where(st, 0, g)]).astype(np.int64)
    return int(glen.sum() + 256 * first.sum() + cert_len[first].sum()), int(first.sum())


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    n_reqs = int(sys.argv[1]) if len(sys.argv) > 1 else 262144
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    cert_bytes = int(sys.argv[3]) if len(sys.argv) > 3 else 2900
    reps = 3
    pems = W.load_keys(4)
    batch = W.make_write1_batch(n_reqs, k, 0.1)
    host = mh.write1_issue(batch)
    signer = mh.DeviceSigner(pems[0], 0)
    db = mh.DeviceWrite1Batch(batch, 0)
    ds, has_cert = reply_source(batch, cert_bytes)
    out = mh.DeviceWrite1Issued(batch.n_reqs, batch.n_ops, host.grant_bytes_len, sign=True)
    st = torch.cuda.current_stream().cuda_stream
    Q = batch.n_reqs
    off = torch.zeros(Q, dtype=torch.int64, device=DEV)
    ln = torch.zeros(Q, dtype=torch.int32, device=DEV)
    status = torch.zeros(Q, dtype=torch.uint8, device=DEV)
    total = torch.zeros(1, dtype=torch.int64, device=DEV)
    # warm-up: allocations, code load, and the exact size
    signer.issue_device(db, out, stream=st)
    rc, need = signer.reply_encode_device(db, out, ds, None, off, ln, status, stream=st, check=False)
    wire = torch.zeros(need + 4096, dtype=torch.uint8, device=DEV)
    signer.reply_encode_device(db, out, ds, wire, off, ln, status, stream=st)
    signer.reply_encode_device(db, out, ds, wire, off, ln, status, stream=st, wire_len_dev=total)
    torch.cuda.synchronize()
    assert int(total.item()) == need and bool((status == 0).all()) and signer.rejected() == 0
    pay, n_ent = payload_bytes(batch, host, np.where(has_cert, cert_bytes, 0).astype(np.int64), k)

    def issue():
        signer.issue_device(db, out, stream=st)

    def issue_reply_wait():
        signer.issue_device(db, out, stream=st)
        signer.reply_encode_device(db, out, ds, wire, off, ln, status, stream=st)

    def issue_reply_nowait():
        signer.issue_device(db, out, stream=st)
        signer.reply_encode_device(db, out, ds, wire, off, ln, status, stream=st, wire_len_dev=total)

    t = {"issue_sign": [], "issue_sign_reply_wait": [], "issue_sign_reply_nowait": []}
    for _ in range(reps):  # alternated
        t["issue_sign"].append(wall(issue))
        t["issue_sign_reply_wait"].append(wall(issue_reply_wait))
        t["issue_sign_reply_nowait"].append(wall(issue_reply_nowait))

    # the Write2 encoder's k_enc_copy over the same grants, eight times over
    ver = mh.Verifier([mh.pem_modulus(p) for p in pems], 0)
    ver.set_server_ids(W.SERVER_IDS[:4])
    n_new = out.n_new
    rep = 8
    N = n_new // 8 * 8 * rep
    idx = torch.arange(N, device=DEV) % n_new
    glen = out.grant_len[:n_new][idx].contiguous()
    M, n_mgs = N // 8, N // 2
    w2 = mh.DeviceWrite2Source.from_tensors(
        M, n_mgs, N, 0, grant_bytes=out.grant_bytes, grant_off=out.grant_off[:n_new][idx].contiguous(), grant_len=glen,
        sig=torch.randint(0, 256, (N, 256), dtype=torch.uint8, device=DEV), cert_mg_off=i32(np.arange(M + 1) * 4),
        mg_grant_off=i32(np.arange(n_mgs + 1) * 2),
        mg_signer=torch.from_numpy(np.tile(np.arange(4, dtype=np.int16), M)).to(DEV),
        strings=torch.zeros(1, dtype=torch.uint8, device=DEV), cert_op_off=i32(np.zeros(M + 1)))
    w2_pay = int(glen.sum().item()) + 256 * N
    moff = torch.zeros(M, dtype=torch.int64, device=DEV)
    mln = torch.zeros(M, dtype=torch.int32, device=DEV)
    mst = torch.zeros(M, dtype=torch.uint8, device=DEV)
    rc, w2_need = ver.encode_write2_device(w2, None, moff, mln, mst, stream=st, check=False)
    w2_wire = torch.zeros(w2_need, dtype=torch.uint8, device=DEV)
    ver.encode_write2_device(w2, w2_wire, moff, mln, mst, stream=st)
    torch.cuda.synchronize()
    assert bool((mst == 0).all())
    signer.set_profiling(True)
    ver.set_profiling(True)
    prof, enc = [], []
    for _ in range(reps):  # alternated
        signer.reply_encode_device(db, out, ds, wire, off, ln, status, stream=st, wire_len_dev=total)
        prof.append(signer.read_reply_profile())
        ver.encode_write2_device(w2, w2_wire, moff, mln, mst, stream=st)
        enc.append(ver.read_encode_profile())
    signer.set_profiling(False)
    ver.set_profiling(False)
    torch.cuda.synchronize()
    copy_gbs = [2 * pay / (p["k_w1r_copy"] * 1e-3) / 1e9 for p in prof]
    enc_gbs = [2 * w2_pay / (p["k_enc_copy"] * 1e-3) / 1e9 for p in enc]

    # one request: what a flush of a single message pays
    b1 = W.make_write1_batch(1, k, 0.0)
    d1 = mh.DeviceWrite1Batch(b1, 0)
    s1, _ = reply_source(b1, cert_bytes, pool=16)
    o1 = mh.DeviceWrite1Issued(1, k, 4096, sign=True)
    w1 = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)

    def one_issue():
        signer.issue_device(d1, o1, stream=st)

    def one_reply():
        signer.issue_device(d1, o1, stream=st)
        signer.reply_encode_device(d1, o1, s1, w1, off, ln, status, stream=st, wire_len_dev=total)

    for f in (one_issue, one_reply):
        f()
    lat = {"issue_sign": [], "issue_sign_reply_nowait": []}
    for _ in range(20):
        lat["issue_sign"].append(wall(one_issue))
        lat["issue_sign_reply_nowait"].append(wall(one_reply))
    signer.close()
    ver.close()
    med = lambda v: float(np.median(v))
    base = med(t["issue_sign"])
    r3 = lambda v: [round(x, 3) for x in v]
    print(json.dumps({
        "bench": "write1_reply", "device": torch.cuda.get_device_name(0), "requests": n_reqs, "ops": batch.n_ops,
        "entries": n_ent, "new_grants": host.n_new, "cert_bytes": cert_bytes, "wire_bytes": need,
        "payload_bytes": pay, "reps": reps,
        "wall_ms": {s: r3(v) for s, v in t.items()},
        "reply_added_share": {s: round(med(v) / base - 1, 4) for s, v in t.items() if s != "issue_sign"},
        "kernel_ms": {s: r3([p[s] for p in prof]) for s in mh.W1_REPLY_STAGES},
        "k_w1r_copy_GBps": r3(copy_gbs), "k_enc_copy_GBps": r3(enc_gbs), "k_enc_copy_ms": r3([p["k_enc_copy"] for p in enc]),
        "k_enc_copy_payload_bytes": w2_pay,
        "one_request_ms": {s: round(med(v), 4) for s, v in lat.items()}}))


if __name__ == "__main__":
    main()
