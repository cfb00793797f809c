"""Timing of the envelope codec on the device: wrap (mochi_envelope_encode_device), decode,
route and join, per kernel (mochi_ctx_read_envelope_profile).

python microbench/envelope_bench.py [WRITE2_FRAMES] [REPLY_FRAMES] : two workloads.
  write2   WRITE2_FRAMES (default 250,000) frames of kind 10 carrying Write2ToServer bodies
           at R = 4 with 1 to 4 operations, replicated on the device from 2,048 distinct
           workload bodies (the bodies of microbench/result_encode_bench.py: about a gigabyte,
           larger than the Infinity Cache), each with a 36-byte msgId, a serverId and a
           timestamp: wrapped, then decoded and routed from the wrap's output in place.
  replies  REPLY_FRAMES (default 1,000,000) frames of kinds 8 / 9 / 11 / 6 / 12 with bodies
           of 24 to 87 bytes, msgId and replyToMsgId of 36 bytes, answering REPLY_FRAMES / 4
           outstanding requests in a shuffled order: wrapped, decoded, joined.
Prints one JSON line per workload: per-kernel ms of three repetitions, and bytes read +
written per second for the copy pass (2 x the body bytes), the header pass (the header
bytes written + the id bytes read) and the decode (the frame bytes: nominal, the walk
skips the bodies)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "mochi-db_amd"))
import mochi_hip as mh  # noqa: E402
import workload as W  # noqa: E402

DEV = torch.device("cuda", 0)
DISTINCT = 512  # bodies per op count
REPS = 3


def i64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int64)).to(DEV)


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(DEV)


def u8(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint8)).to(DEV)


def write2_bodies():
    parts, ln = [], []
    for k in (1, 2, 3, 4):
        pool = W.build_pool(R=4, k=k, P=64, P_f=16)
        wb = W.encode_wire_batch(W.make_batch(pool, DISTINCT, first_cert=k * 1000, faults=False))
        for m in range(DISTINCT):
            parts.append(wb.wire[int(wb.msg_off[m]):int(wb.msg_off[m]) + int(wb.msg_len[m])])
            ln.append(int(wb.msg_len[m]))
    ln = np.array(ln, np.int64)
    return np.concatenate(parts), np.concatenate([[0], np.cumsum(ln)[:-1]]), ln


def uuids(n, rng):
    """n distinct 36-byte ids in one blob: hex digits and dashes, as UUID.toString()."""
    hexd = np.frombuffer(b"0123456789abcdef", np.uint8)
    a = hexd[rng.integers(0, 16, (n, 36))]
    a[:, [8, 13, 18, 23]] = ord("-")
    a[:, 24:36] = hexd[(np.arange(n)[:, None] >> (4 * np.arange(11, -1, -1))) & 15]  # the index: distinct
    return a.reshape(-1)


def run(ver, name, src, M, body_bytes, id_bytes, request_ids=None, route=False):
    st = torch.cuda.current_stream().cuda_stream
    off = torch.zeros(M, dtype=torch.int64, device=DEV)
    ln = torch.zeros(M, dtype=torch.int32, device=DEV)
    status = torch.zeros(M, dtype=torch.uint8, device=DEV)
    total = torch.zeros(1, dtype=torch.int64, device=DEV)
    rc, need = ver.envelope_encode_device(src, None, off, ln, status, stream=st, check=False)
    out = torch.zeros(need + 4096, dtype=torch.uint8, device=DEV)
    ddec = mh.DeviceEnvelopeDecoded(M)
    drt = mh.DeviceEnvelopeRouted(M) if route else None
    dj = mh.DeviceEnvelopeJoined(M, request_ids.n_reqs) if request_ids is not None else None
    frames = mh.DeviceEnvelopeFrames.from_tensors(M, out, off, ln, wire_len=need)
    prof = {k: [] for k in ("encode", "decode", "route", "join")}
    ver.set_profiling(True)
    for rep in range(REPS + 1):  # the first repetition warms up: allocations, code load
        ver.envelope_encode_device(src, out, off, ln, status, stream=st, wire_len_dev=total)
        ver.envelope_decode_device(frames, ddec, stream=st)
        if route:
            ver.envelope_route_device(ddec, drt, stream=st)
        if dj is not None:
            ver.envelope_join_device(request_ids, frames, ddec, dj, stream=st)
        torch.cuda.synchronize()
        if rep:
            for k in prof:
                if k in ("encode", "decode") or (k == "route" and route) or (k == "join" and dj is not None):
                    prof[k].append(ver.read_envelope_profile(k))
    ver.set_profiling(False)
    assert int(total.item()) == need and bool((status == 0).all()) and bool((ddec.status == 0).all())
    res = {"bench": "envelope", "workload": name, "device": torch.cuda.get_device_name(0), "frames": M, "frame_bytes": need,
           "body_bytes": body_bytes, "id_bytes": id_bytes, "reps": REPS}
    r3 = lambda v: [round(float(x), 4) for x in v]
    for k, ps in prof.items():
        if ps:
            res[k + "_ms"] = {s: r3([p[s] for p in ps]) for s in mh.ENVELOPE_STAGES[k]}
    hdr = need - body_bytes
    res["k_env_copy_GBps"] = r3([2 * body_bytes / (p["k_env_copy"] * 1e-3) / 1e9 for p in prof["encode"]])
    res["k_env_hdr_GBps"] = r3([(hdr + id_bytes) / (p["k_env_hdr"] * 1e-3) / 1e9 for p in prof["encode"]])
    res["k_env_decode_GBps_nominal"] = r3([need / (p["k_env_decode"] * 1e-3) / 1e9 for p in prof["decode"]])
    res["k_env_decode_ns_per_frame"] = r3([p["k_env_decode"] * 1e6 / M for p in prof["decode"]])
    if route:
        assert int(drt.kind_off[13].item()) == M
        res["route_ns_per_frame"] = r3([sum(p.values()) * 1e6 / M for p in prof["route"]])
    if dj is not None:
        assert int(dj.n_resps.item()) == M
        res["join_ns_per_frame"] = r3([sum(p.values()) * 1e6 / M for p in prof["join"]])
    print(json.dumps(res), flush=True)


def main():
    M2 = int(sys.argv[1]) if len(sys.argv) > 1 else 250000
    M1 = int(sys.argv[2]) if len(sys.argv) > 2 else 1000000
    rng = np.random.default_rng(13)
    ver = mh.Verifier([mh.pem_modulus(p) for p in W.load_keys(4)], 0)

    if M2:
        blob, b_off, b_len = write2_bodies()
        D = b_off.size
        tiles = (M2 + D - 1) // D
        pick = rng.permutation(tiles * D)[:M2]
        ids = np.concatenate([uuids(M2, rng), np.frombuffer(b"server-0", np.uint8)])
        src = mh.DeviceEnvelopeSource.from_tensors(
            M2, 0, bodies=u8(blob).repeat(tiles), ids=u8(ids), kind=u8(np.full(M2, 10, np.uint8)),
            body_off=i64((pick // D) * blob.size + b_off[pick % D]), body_len=i32(b_len[pick % D]),
            msg_timestamp=i64(1_700_000_000_000 + np.arange(M2)), msg_id_off=i64(36 * np.arange(M2)),
            msg_id_len=i32(np.full(M2, 36)), server_id_off=i64(np.full(M2, 36 * M2)), server_id_len=i32(np.full(M2, 8)))
        run(ver, "write2", src, M2, int(b_len[pick % D].sum()), 44 * M2, route=True)
        del src
        torch.cuda.empty_cache()

    if M1:
        Q = max(M1 // 4, 1)
        req_blob = uuids(Q, rng)
        dreq = mh.DeviceEnvelopeRequests.__new__(mh.DeviceEnvelopeRequests)
        dreq.n_reqs, dreq.ids_len = Q, int(req_blob.size)
        dreq.ids, dreq.id_off, dreq.id_len = u8(req_blob), i64(36 * np.arange(Q)), i32(np.full(Q, 36))
        blen = rng.integers(24, 88, M1)
        boff = np.concatenate([[0], np.cumsum(blen)[:-1]])
        to = rng.permutation(M1) % Q
        ids = np.concatenate([req_blob, uuids(M1, rng), np.frombuffer(b"server-0", np.uint8)])
        src = mh.DeviceEnvelopeSource.from_tensors(
            M1, 0, bodies=torch.randint(0, 256, (int(blen.sum()),), dtype=torch.uint8, device=DEV), ids=u8(ids),
            kind=u8(np.array([8, 9, 11, 6, 12], np.uint8)[rng.integers(0, 5, M1)]), body_off=i64(boff), body_len=i32(blen),
            msg_timestamp=i64(1_700_000_000_000 + np.arange(M1)), msg_id_off=i64(36 * (Q + np.arange(M1))),
            msg_id_len=i32(np.full(M1, 36)), reply_to_off=i64(36 * to), reply_to_len=i32(np.full(M1, 36)),
            server_id_off=i64(np.full(M1, 36 * (Q + M1))), server_id_len=i32(np.full(M1, 8)))
        run(ver, "replies", src, M1, int(blen.sum()), 80 * M1, request_ids=dreq)
    ver.close()


if __name__ == "__main__":
    main()
