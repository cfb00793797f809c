"""Timing of the server's closing steps behind the Write2 verifier: the answer plan
(mochi_write2_answer_plan_device) and the answer encoder (mochi_result_reply_encode_device).

python microbench/result_encode_bench.py [MSGS] : MSGS Write2ToServer bodies (default
250,000) at R = 4 with 1 to 4 operations each, replicated on the device from 2,048
distinct workload bodies (about a gigabyte of wire: larger than the Infinity Cache);
every message OK and accepted, eight ops in ten APPLY (they answer with the incoming
certificate), one in ten READ (a stored certificate of 2,900 bytes out of a pool of
131,072) and one in ten WRONG_SHARD.  The verdict arrays are made up: the verifier is
not part of what is timed.  Prints one JSON line:
  k_w2a_plan's ms (events around the call) and the encoder's per-kernel ms
    (mochi_ctx_read_result_encode_profile), three repetitions;
  k_rae_copy's bytes read + written per second;
  wall ms of plan + encode in the device capacity mode (no host wait)."""
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
POOL, CERT = 131072, 2900
DISTINCT = 512  # bodies per op count


def i64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int64)).to(DEV)


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(DEV)


def u8(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint8)).to(DEV)


def bodies():
    """(blob, offsets, lengths, op counts) of 4 * DISTINCT distinct bodies, 1 to 4 operations."""
    parts, ln, k_of = [], [], []
    for k in (1, 2, 3, 4):
        pool = W.build_pool(R=4, k=k, P=64, P_f=16)
        wb = W.encode_wire_batch(W.make_batch(pool, DISTINCT, first_cert=k * 1000, faults=False))
        for m in range(DISTINCT):
            parts.append(wb.wire[int(wb.msg_off[m]):int(wb.msg_off[m]) + int(wb.msg_len[m])])
            ln.append(int(wb.msg_len[m]))
            k_of.append(k)
    ln = np.array(ln, np.int64)
    return np.concatenate(parts), np.concatenate([[0], np.cumsum(ln)[:-1]]), ln, np.array(k_of, np.int64)


def main():
    M = int(sys.argv[1]) if len(sys.argv) > 1 else 250000
    reps = 3
    blob, b_off, b_len, b_k = bodies()
    D = b_off.size
    tiles = (M + D - 1) // D
    rng = np.random.default_rng(11)
    pick = rng.permutation(tiles * D)[:M]  # message m is body pick % D of tile pick // D
    wire = u8(blob).repeat(tiles)
    msg_off = (pick // D) * blob.size + b_off[pick % D]
    k = b_k[pick % D]
    fo = np.concatenate([[0], np.cumsum(k)])
    O = int(fo[-1])
    dwb = mh.DeviceWireBatch.from_encoded(wire, i64(msg_off), i32(b_len[pick % D]), M, np.zeros((M, 128), np.uint8),
                                          op_flags_off=fo.astype(np.uint32).view(np.int32), op_flags=np.full(O, 3, np.uint8))
    u = rng.integers(0, 10, O)
    dec = np.where(u == 0, mh.OPD_READ, np.where(u == 1, mh.OPD_WRONG_SHARD, mh.OPD_APPLY)).astype(np.uint8)

    class V:
        cert_accept_bits = i32(np.full((M + 31) // 32, 0xFFFFFFFF, np.uint32))
        op_decision = u8(dec)

    class S:
        store = torch.randint(0, 256, (POOL * CERT + 64,), dtype=torch.uint8, device=DEV)
        store_len = POOL * CERT + 64
        op_value_off = i64(np.full(O, POOL * CERT))
        op_value_len = i32(np.full(O, 16))
        op_stored_cert_off = i64(rng.integers(0, POOL, O) * CERT)
        op_stored_cert_len = i32(np.full(O, CERT))
        op_store_flags = u8(np.full(O, mh.W2A_HAS_STORED_CERT, np.uint8))
        slot_off = i64(fo[:-1])
        n_slots = O

    planned = mh.DeviceWrite2AnswerPlanned(M, O)
    ver = mh.Verifier([mh.pem_modulus(p) for p in W.load_keys(4)], 0)
    st = torch.cuda.current_stream().cuda_stream
    off = torch.zeros(M, dtype=torch.int64, device=DEV)
    ln = torch.zeros(M, dtype=torch.int32, device=DEV)
    status = torch.zeros(M, dtype=torch.uint8, device=DEV)
    total = torch.zeros(1, dtype=torch.int64, device=DEV)
    # warm-up: allocations, code load, and the exact size
    mh.write2_answer_plan_device(dwb, V, S, planned, stream=st)
    answers = planned.answers(dwb, S)
    rc, need = ver.result_reply_encode_device(answers, None, off, ln, status, stream=st, check=False)
    out = torch.zeros(need + 4096, dtype=torch.uint8, device=DEV)
    ver.result_reply_encode_device(answers, out, off, ln, status, stream=st, wire_len_dev=total)
    torch.cuda.synchronize()
    assert int(total.item()) == need and bool((status == 0).all())
    assert bool((planned.plan_status[:M] == mh.W2A_REPLY).all())
    pay = int(planned.op_result_len[:O].to(torch.int64).sum().item() + planned.op_cert_len[:O].to(torch.int64).sum().item())

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    plan_ms, prof, wall_ms = [], [], []
    ver.set_profiling(True)
    for _ in range(reps):
        e0.record()
        mh.write2_answer_plan_device(dwb, V, S, planned, stream=st)
        e1.record()
        ver.result_reply_encode_device(answers, out, off, ln, status, stream=st, wire_len_dev=total)
        prof.append(ver.read_result_encode_profile())
        torch.cuda.synchronize()
        plan_ms.append(e0.elapsed_time(e1))
    ver.set_profiling(False)
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mh.write2_answer_plan_device(dwb, V, S, planned, stream=st)
        ver.result_reply_encode_device(answers, out, off, ln, status, stream=st, wire_len_dev=total)
        torch.cuda.synchronize()
        wall_ms.append((time.perf_counter() - t0) * 1e3)
    ver.close()
    r3 = lambda v: [round(float(x), 3) for x in v]
    print(json.dumps({
        "bench": "result_encode", "device": torch.cuda.get_device_name(0), "messages": M, "ops": O, "request_wire_bytes": int(wire.numel()),
        "answer_wire_bytes": need, "payload_bytes": pay, "reps": reps, "k_w2a_plan_ms": r3(plan_ms),
        "kernel_ms": {s: r3([p[s] for p in prof]) for s in mh.RESULT_ENCODE_STAGES},
        "k_rae_copy_GBps": r3([2 * pay / (p["k_rae_copy"] * 1e-3) / 1e9 for p in prof]),
        "plan_encode_wall_ms": r3(wall_ms)}))


if __name__ == "__main__":
    main()
