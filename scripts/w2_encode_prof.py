#!/usr/bin/env python3
"""Encoder profiling driver: the Write2ToServer bodies of 250k certificates
(R=4) encoded on the device a few times.  Prints, per call: the encoder's time
per kernel (HIP events, mochi_ctx_read_encode_profile), a device-to-device
hipMemcpyAsync of the same number of output bytes, and the device decoder's
count + emit time on the encoded messages, taken as the wire call (decode +
verify, mochi_verify_write2_device) minus the SoA call (verify alone) on the
same grants.  Under `rocprofv3 --kernel-trace --stats` the k_w2_* rows give the
decoder's kernels one by one."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mochi-db_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import mochi_hip as mh  # noqa: E402
import workload as W  # noqa: E402

n_certs = int(sys.argv[1]) if len(sys.argv) > 1 else 250000
reps = 5
pool = W.build_pool(R=4, k=1, P=256, P_f=64)
s = W.separate_copies(W.make_batch(pool, n_certs))  # every grant its own bytes, mixed alignments
src = W.write2_source(s)
ver = mh.Verifier(pool.moduli, 0)
ver.set_server_ids(W.SERVER_IDS[:4])
dsrc = mh.DeviceWrite2Source(src, 0)
dev = torch.device("cuda", 0)
M = src.n_msgs
off = torch.zeros(M, dtype=torch.int64, device=dev)
ln = torch.zeros(M, dtype=torch.int32, device=dev)
status = torch.zeros(M, dtype=torch.uint8, device=dev)
st = torch.cuda.current_stream()
rc, need = ver.encode_write2_device(dsrc, None, off, ln, status, stream=st.cuda_stream, check=False)  # size only
wire = torch.zeros(need, dtype=torch.uint8, device=dev)
copy_dst = torch.empty_like(wire)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    fn()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


ver.set_profiling(True)
enc = lambda: ver.encode_write2_device(dsrc, wire, off, ln, status, stream=st.cuda_stream)
for _ in range(2):
    enc()
torch.cuda.synchronize()
kern, total, copy = [], [], []
for _ in range(reps):
    total.append(timed(enc))
    kern.append(ver.read_encode_profile())
    copy.append(timed(lambda: copy_dst.copy_(wire, non_blocking=True)))  # hipMemcpyAsync D2D, the same bytes
ver.set_profiling(False)
assert bool((status == 0).all())

# the decoder on the same messages: wire call (decode + verify) minus the SoA call (verify) on the same grants
b = s.batch
dwb = mh.DeviceWireBatch.from_encoded(wire, off, ln, M, b.expected_hash)
out = mh.DeviceVerdicts(0, M, 0, full=True)
dbatch = mh.DeviceBatch(b, 0)
soa = mh.DeviceVerdicts(dbatch.n_grants, dbatch.n_certs, 0, full=True)
wire_call = lambda: ver.verify_write2_device(dwb, out, 4, True, stream=st.cuda_stream)
soa_call = lambda: ver.verify_device(dbatch, soa, 4, True, stream=st.cuda_stream)
for _ in range(2):
    wire_call()
    soa_call()
torch.cuda.synchronize()
tw = [timed(wire_call) for _ in range(reps)]
ts = [timed(soa_call) for _ in range(reps)]
assert np.array_equal(out.to_host().cert_accept_bits, soa.to_host().cert_accept_bits)

med = lambda v: float(np.median(v))
res = {
    "n_msgs": M, "n_grants": src.n_grants, "wire_bytes": need,
    "encode_kernel_ms": {k: round(med([d[k] for d in kern]), 4) for k in mh.Verifier.ENCODE_KERNELS},
    "encode_call_ms": round(med(total), 4),  # with the host wait for the total size in the middle
    "d2d_copy_ms": round(med(copy), 4),
    "wire_verify_ms": round(med(tw), 4), "soa_verify_ms": round(med(ts), 4),
    "decode_count_emit_ms": round(med(tw) - med(ts), 4),
}
res["encode_kernels_sum_ms"] = round(sum(res["encode_kernel_ms"].values()), 4)
res["encode_over_copy"] = round(res["encode_kernels_sum_ms"] / res["d2d_copy_ms"], 2)
print(json.dumps(res))
