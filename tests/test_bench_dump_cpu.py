"""bench.py --dump-outputs / --full on the CPU: the writer of the verdict arrays
(float32 / float64 files, a fixed seeded sample of a long array, the 64 MB
budget) and the option defaults of a plain run."""
import os
import sys

import numpy as np

import bench
import mochi_hip as mh


def _verdicts(n_grants, n_certs, n_ops, seed):
    rng = np.random.default_rng(seed)
    v = mh.Verdicts.alloc(n_grants, n_certs, n_ops)
    for name in mh.DeviceVerdicts.NAMES:
        a = getattr(v, name)
        a[...] = rng.integers(0, 200, a.shape).astype(a.dtype)
    return v


def test_dump_outputs_small_arrays_whole(tmp_path):
    v = _verdicts(1001, 251, 251, 1)
    v.op_ts = None  # an output the path did not produce is not written
    bench.dump_outputs(str(tmp_path / "d"), v)
    got = sorted(os.listdir(tmp_path / "d"))
    assert got == sorted(n + ".npy" for n in mh.DeviceVerdicts.NAMES if n != "op_ts")
    for name in mh.DeviceVerdicts.NAMES:
        if name == "op_ts":
            continue
        src = getattr(v, name)
        a = np.load(tmp_path / "d" / (name + ".npy"))
        assert a.dtype == (np.float32 if src.dtype.itemsize == 1 else np.float64)
        assert np.array_equal(a, src.astype(np.float64))  # whole and exact


def test_dump_outputs_long_array_fixed_sample(tmp_path):
    n = bench.DUMP_SAMPLE + 12345
    a, b = _verdicts(n, 64, 0, 2), _verdicts(n, 64, 0, 3)
    bench.dump_outputs(str(tmp_path / "a"), a)
    bench.dump_outputs(str(tmp_path / "a2"), a)
    bench.dump_outputs(str(tmp_path / "b"), b)
    fa, fa2, fb = (np.load(tmp_path / d / "grant_ts.npy") for d in ("a", "a2", "b"))
    assert fa.shape == (bench.DUMP_SAMPLE,) and np.array_equal(fa, fa2)
    # the same elements of either run: the sample depends on the length alone
    idx = np.flatnonzero(np.isin(np.arange(n), np.sort(np.random.default_rng([bench.DUMP_SEED, n]).choice(
        n, bench.DUMP_SAMPLE, replace=False))))
    assert np.array_equal(fa, a.grant_ts[idx]) and np.array_equal(fb, b.grant_ts[idx])
    # every array at the cap stays inside the 64 MB budget
    assert (len(mh.DeviceVerdicts.NAMES) + 1) * bench.DUMP_SAMPLE * 8 <= 64e6


def test_plain_run_has_no_side_legs(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    args = bench.parse_args()
    assert args.full is False and args.dump_outputs is None and args.steps == 3 and args.warmup == 1
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "x"])
    args = bench.parse_args()
    assert args.full is True and args.dump_outputs == "x"
