"""Timing of the device read request decoder (mochi_read_request_decode_device) and the read
answer plan, next to the host twin on the same bodies.

python microbench/read_request_bench.py [REQS] [OPS] [REPS] : REQS requests (default
262,144) of OPS ops (2) on the keys of workload.make_write1_batch at its default contention
(the shape and the keys of write1_request_bench.py), encoded as ReadToServer bodies back to
back, each with a 36-byte nonce.  Two warm-up calls, then REPS (default 9) repetitions of
each figure, alternated; every list in the output holds the repetitions in order and the
*_median fields are their medians.  Prints one JSON line:
  kernel_ms: the decoder's per-stage device times (mochi_ctx_read_read_decode_profile), from
    profiled calls of their own;
  plan_ms: device time of k_rda_plan alone (events around the one launch), every key LOCAL,
    PRESENT, AVAILABLE and with a certificate;
  decode_wall_ms: host clock around one decode call (its one wait included) that ends in a
    synchronise, profiling off; decode_plan_wall_ms: the same with the plan behind it;
  host_wall_ms: the host twin, one thread, on the same bodies (REPS capped at 3);
  requests per second for each, from the medians."""
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


def varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append(v & 0x7F | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def ld(tag, p):
    return bytes([tag]) + varint(len(p)) + p


def bodies_of(b):
    """The batch's requests as ReadToServer bodies (every op a READ: no action field)."""
    s = np.asarray(b.strings, np.uint8).tobytes()
    ko, kl, off = b.op_key_off.tolist(), b.op_key_len.tolist(), b.req_op_off.tolist()
    out = []
    for q in range(b.n_reqs):
        tx = b"".join(ld(0x0A, ld(0x12, s[ko[o]:ko[o] + kl[o]])) for o in range(off[q], off[q + 1]))
        out.append(ld(0x0A, b"client-%d" % (q % 1000)) + ld(0x12, tx) + ld(0x1A, b"123e4567-e89b-12d3-a456-%012d" % q))
    return out


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    n_reqs = int(sys.argv[1]) if len(sys.argv) > 1 else 262144
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 9
    batch = W.make_write1_batch(n_reqs, k)
    bodies = bodies_of(batch)
    lens = np.array([len(x) for x in bodies], np.uint32)
    reqs = mh.ReadRequests(wire=np.frombuffer(b"".join(bodies), np.uint8),
                           msg_off=(np.cumsum(lens, dtype=np.uint64) - lens).astype(np.uint64), msg_len=lens)
    host_ms = []
    for _ in range(min(reps, 3)):
        t0 = time.perf_counter()
        host = mh.read_request_decode_into(reqs, batch.n_ops)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    assert host.rc == mh.OK and host.n_ops == batch.n_ops and host.n_keys == np.unique(batch.op_obj).size
    assert (host.arrays["req_status"] == 0).all()

    ver = mh.Verifier([mh.pem_modulus(p) for p in W.load_keys(1)], 0)
    dr = mh.DeviceReadRequests(reqs, 0)
    out = mh.DeviceReadRequestsDecoded(n_reqs, batch.n_ops)
    U = host.n_keys
    u = np.arange(U, dtype=np.uint64)
    ks = mh.ReadKeyState(store=np.zeros(4096, np.uint8),
                         key_flags=np.full(U, mh.RDK_LOCAL | mh.RDK_PRESENT | mh.RDK_AVAILABLE | mh.RDK_HAS_CERT, np.uint8),
                         key_value_off=u % 4000, key_value_len=np.full(U, 32, np.uint32), key_cert_off=u % 3000,
                         key_cert_len=np.full(U, 1024, np.uint32))
    dks = mh.DeviceReadKeyState(ks, 0)
    planned = mh.DeviceReadAnswerPlanned(n_reqs, batch.n_ops)
    st = torch.cuda.current_stream().cuda_stream

    def decode():
        ver.read_request_decode_device(dr, out, stream=st)

    def decode_plan():
        ver.read_request_decode_device(dr, out, stream=st)
        mh.read_answer_plan_device(out, dks, planned, stream=st)

    for _ in range(2):  # warm-up: allocations, code load
        decode_plan()
    torch.cuda.synchronize()
    got = out.to_host()
    for name, a in host.trimmed().items():
        assert np.array_equal(got.trimmed()[name], a), name
    want = mh.read_answer_plan(host, ks)
    for name, a in planned.to_host().items():
        assert np.array_equal(a, want[name]), name
    assert (want["plan_status"] == mh.RDA_REPLY).all()
    t = {"decode_wall_ms": [], "decode_plan_wall_ms": []}
    for _ in range(reps):  # alternated
        t["decode_wall_ms"].append(wall(decode))
        t["decode_plan_wall_ms"].append(wall(decode_plan))
    plan_ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        mh.read_answer_plan_device(out, dks, planned, stream=st)
        e1.record()
        e1.synchronize()
        plan_ms.append(e0.elapsed_time(e1))
    ver.set_profiling(True)
    prof = []
    for _ in range(reps):
        decode()
        prof.append(ver.read_read_decode_profile())
    ver.set_profiling(False)
    ver.close()
    med = lambda v: float(np.median(v))
    r3 = lambda v: [round(x, 3) for x in v]
    rate = lambda ms: round(n_reqs / (ms * 1e-3))
    print(json.dumps({
        "bench": "read_request", "device": torch.cuda.get_device_name(0), "requests": n_reqs, "ops": batch.n_ops,
        "keys": U, "wire_bytes": int(reqs.wire.size), "reps": reps,
        "kernel_ms": {s: r3([p[s] for p in prof]) for s in mh.READ_REQUEST_STAGES},
        "kernel_ms_median": {s: round(med([p[s] for p in prof]), 3) for s in mh.READ_REQUEST_STAGES},
        "kernel_ms_median_sum": round(sum(med([p[s] for p in prof]) for s in mh.READ_REQUEST_STAGES), 3),
        "plan_ms": r3(plan_ms), "plan_ms_median": round(med(plan_ms), 3),
        **{s: r3(v) for s, v in t.items()}, **{s + "_median": round(med(v), 3) for s, v in t.items()},
        "host_wall_ms": r3(host_ms), "host_wall_ms_median": round(med(host_ms), 3),
        "requests_per_s": {"device_decode": rate(med(t["decode_wall_ms"])),
                           "device_decode_plan": rate(med(t["decode_plan_wall_ms"])), "host_one_thread": rate(med(host_ms))}}))


if __name__ == "__main__":
    main()
