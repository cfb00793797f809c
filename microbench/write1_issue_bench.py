"""Timing of device Write1 grant issuance (mochi_write1_issue_device) against
the signing of the same grants.

python microbench/write1_issue_bench.py [REQS] [OPS] [CONTENTION] : REQS requests
(default 65,536) of OPS ops (2), about CONTENTION (0.1) of the ops on a slot
another op wants too.  Checks the device outputs against the host form, then
prints one JSON line: the per-kernel ms of an issue call (median of the timed
calls), k_rsa_sign + the public-key check over the same new grants in the same
call, and issuance (decide + emit kernels) as a share of the signing time."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "mochi-db_amd"))
import mochi_hip as mh  # noqa: E402
import workload as W  # noqa: E402


def main():
    n_reqs = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    contention = float(sys.argv[3]) if len(sys.argv) > 3 else 0.1
    reps = 5
    batch = W.make_write1_batch(n_reqs, k, contention)
    host = mh.write1_issue(batch)
    signer = mh.DeviceSigner(W.load_keys(1)[0], 0)
    db = mh.DeviceWrite1Batch(batch, 0)
    out = mh.DeviceWrite1Issued(batch.n_reqs, batch.n_ops, host.grant_bytes_len, sign=True)
    st = torch.cuda.current_stream().cuda_stream
    signer.issue_device(db, out, stream=st)  # warm-up: allocations, code load
    torch.cuda.synchronize()
    got = out.to_host()
    for name in ("op_decision", "op_grant", "req_kind", "req_grant_off", "req_grant", "grant_off", "grant_len",
                 "grant_op", "grant_ts"):
        assert np.array_equal(getattr(got, name), getattr(host, name)), name
    assert got.grant_bytes[:host.grant_bytes_len].tobytes() == host.grant_bytes.tobytes()
    assert signer.rejected() == 0
    signer.set_profiling(True)
    runs = []
    for _ in range(reps):
        signer.issue_device(db, out, stream=st)
        runs.append(signer.read_issue_profile())
    signer.close()
    ms = {s: float(np.median([r[s] for r in runs])) for s in mh.W1_ISSUE_STAGES}
    issue = sum(v for s, v in ms.items() if s != "sign")
    d = np.bincount(host.op_decision, minlength=7)
    print(json.dumps({
        "bench": "write1_issue", "device": torch.cuda.get_device_name(0), "requests": n_reqs, "ops": batch.n_ops,
        "new_grants": host.n_new, "grant_bytes": host.grant_bytes_len,
        "contended_ops": int(d[mh.W1D_RETRY] + d[mh.W1D_REFUSED]), "reps": reps,
        "kernel_ms": {s: round(v, 4) for s, v in ms.items()}, "issue_ms": round(issue, 4),
        "sign_ms": round(ms["sign"], 3), "issue_over_sign": round(issue / ms["sign"], 5),
        "decide_emit_over_sign": round((ms["k_w1_decide"] + ms["k_w1_emit"]) / ms["sign"], 5)}))


if __name__ == "__main__":
    main()
