"""Timing of the device Write1 request decoder (mochi_write1_request_decode_device) and the
key-state join, next to the host twin on the same bodies.

python microbench/write1_request_bench.py [REQS] [OPS] [REPS] : REQS requests (default
262,144) of OPS ops (2) at workload.make_write1_batch's default contention, encoded as
Write1ToServer bodies back to back.  Two warm-up calls, then REPS (default 9) repetitions
of each figure, alternated; every list in the output holds the repetitions in order and the
*_median fields are their medians.  Prints one JSON line:
  kernel_ms: the decoder's per-stage device times (mochi_signer_read_request_profile), from
    profiled calls of their own;
  decode_wall_ms: host clock around one decode call (its one wait included) that ends in a
    synchronise, profiling off; decode_join_wall_ms: the same with the join behind it;
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
    """The batch's requests as Write1ToServer bodies (every op a WRITE with a one-byte value)."""
    s = np.asarray(b.strings, np.uint8).tobytes()
    ko, kl = b.op_key_off.tolist(), b.op_key_len.tolist()
    ho, hl, off, seed = b.req_hash_off.tolist(), b.req_hash_len.tolist(), b.req_op_off.tolist(), b.req_seed.tolist()
    out = []
    for q in range(b.n_reqs):
        tx = b"".join(ld(0x0A, b"\x08\x02" + ld(0x12, s[ko[o]:ko[o] + kl[o]]) + b"\x1a\x01v") for o in range(off[q], off[q + 1]))
        out.append(ld(0x0A, b"client-%d" % (q % 1000)) + ld(0x12, tx) + (b"\x18" + varint(seed[q]) if seed[q] else b"") +
                   ld(0x22, s[ho[q]:ho[q] + hl[q]]))
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
    reqs = mh.Write1Requests(wire=np.frombuffer(b"".join(bodies), np.uint8),
                             msg_off=(np.cumsum(lens, dtype=np.uint64) - lens).astype(np.uint64), msg_len=lens)
    host_ms = []
    for _ in range(min(reps, 3)):
        t0 = time.perf_counter()
        host = mh.write1_request_decode_into(reqs, batch.n_ops)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    assert host.rc == mh.OK and host.n_ops == batch.n_ops and host.n_keys == np.unique(batch.op_obj).size
    assert (host.arrays["req_status"] == 0).all()

    signer = mh.DeviceSigner(W.load_keys(1)[0], 0)
    dr = mh.DeviceWrite1Requests(reqs, 0)
    out = mh.DeviceWrite1RequestsDecoded(n_reqs, batch.n_ops)
    U = host.n_keys
    first = host.arrays["key_op"][:U]
    ks = mh.DeviceWrite1KeyState(mh.Write1KeyState(
        key_flags=np.full(U, mh.W1OP_LOCAL | mh.W1OP_HAS_SVOC, np.uint8), key_epoch=np.asarray(batch.op_epoch)[first],
        key_given_off=np.arange(U + 1, dtype=np.uint32), given_ts=np.asarray(batch.op_epoch)[first] + 17,
        given_stored=np.arange(U, dtype=np.uint32)), 0)
    op_epoch = torch.zeros(batch.n_ops, dtype=torch.int64, device=DEV)
    op_stored = torch.zeros(batch.n_ops, dtype=torch.int32, device=DEV)
    op_flags = torch.zeros(batch.n_ops, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def decode():
        signer.request_decode_device(dr, out, stream=st)

    def decode_join():
        signer.request_decode_device(dr, out, stream=st)
        signer.state_join_device(n_reqs, out.n_ops, out.req_op_off, out.req_seed, out.op_flags, out.op_obj, ks, op_flags,
                                 op_epoch, op_stored, stream=st)

    for _ in range(2):  # warm-up: allocations, code load
        decode_join()
    torch.cuda.synchronize()
    got = out.to_host()
    for name, a in host.trimmed().items():
        assert np.array_equal(got.trimmed()[name], a), name
    t = {"decode_wall_ms": [], "decode_join_wall_ms": []}
    for _ in range(reps):  # alternated
        t["decode_wall_ms"].append(wall(decode))
        t["decode_join_wall_ms"].append(wall(decode_join))
    signer.set_profiling(True)
    prof = []
    for _ in range(reps):
        decode()
        prof.append(signer.read_request_profile())
    signer.set_profiling(False)
    signer.close()
    med = lambda v: float(np.median(v))
    r3 = lambda v: [round(x, 3) for x in v]
    rate = lambda ms: round(n_reqs / (ms * 1e-3))
    print(json.dumps({
        "bench": "write1_request", "device": torch.cuda.get_device_name(0), "requests": n_reqs, "ops": batch.n_ops,
        "keys": U, "wire_bytes": int(reqs.wire.size), "reps": reps,
        "kernel_ms": {s: r3([p[s] for p in prof]) for s in mh.W1_REQUEST_STAGES},
        "kernel_ms_median": {s: round(med([p[s] for p in prof]), 3) for s in mh.W1_REQUEST_STAGES},
        "kernel_ms_median_sum": round(sum(med([p[s] for p in prof]) for s in mh.W1_REQUEST_STAGES), 3),
        **{s: r3(v) for s, v in t.items()}, **{s + "_median": round(med(v), 3) for s, v in t.items()},
        "host_wall_ms": r3(host_ms), "host_wall_ms_median": round(med(host_ms), 3),
        "requests_per_s": {"device_decode": rate(med(t["decode_wall_ms"])),
                           "device_decode_join": rate(med(t["decode_join_wall_ms"])), "host_one_thread": rate(med(host_ms))}}))


if __name__ == "__main__":
    main()
