"""Client-side aggregation on the device: MochiDBClient's Read /
Write2 response tally (MochiDBClient.java:148-175, 355-382) and Write1 round
classification (:195-219, 236-332), batched across thousands of in-flight
transactions -- bit-exact with the oracle restatement (and with the host C++).

The second half runs the case sets of client_model.py (a plain-Python restatement of the
Java; test_client_model_cpu.py shows what they cover) through the C entry points directly,
with caller-made tensors: every output is preset and has GUARD elements on either side, so
a bit the kernel should have cleared, an entry it should have written and a write outside
the contract's range all show."""
import functools

import numpy as np
import pytest

import client_model as M
import mochi_hip as mh
import oracle_ffi as O
from test_capi_cpu import _random_responses, _random_write1

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("R", [4, 5, 7])
def test_tally_responses_device_matches_oracle(R):
    rng = np.random.default_rng(4321 + R)
    resps, n_ops = _random_responses(rng, 20000)
    a1, r1, c1 = mh.tally_responses_device(resps, n_ops, R)
    a2, r2, c2 = O.tally_responses(resps, n_ops, R)
    np.testing.assert_array_equal(a1, a2)
    np.testing.assert_array_equal(r1, r2)
    for x, y in zip(c1, c2):
        np.testing.assert_array_equal(x, y)
    assert set(np.unique(r1).tolist()) == {0, 1, 2}


def test_tally_responses_device_reference_semantics():
    acc, why, ch = mh.tally_responses_device([[[0], [0], [0], [0]], [[0], [1], [0], [1]], [[0, 0], [0]]], [1, 1, 2], 4)
    assert acc.tolist() == [True, False, False]
    assert why.tolist() == [0, 2, 1]
    assert ch[0][0] == 3 and ch[1][0] == 2


def test_write1_classify_device_matches_oracle():
    rng = np.random.default_rng(78)
    reqs = _random_write1(rng, 20000)
    got = mh.write1_classify_device(reqs)
    np.testing.assert_array_equal(got, O.write1_classify(reqs))
    np.testing.assert_array_equal(got, mh.write1_classify(reqs))
    assert set(np.unique(got).tolist()) == {0, 1, 2, 3, 4}


def test_client_device_empty():
    acc, why, ch = mh.tally_responses_device([], [], 4)
    assert acc.size == 0
    assert mh.write1_classify_device([]).size == 0


# ---------------------------------------------------------------------------
# the case sets of client_model.py, with guarded outputs
# ---------------------------------------------------------------------------
GUARD = 64  # elements on either side of every output
BITS_FILL, BYTE_FILL, CHOSEN_FILL = 0xFFFFFFFF, 0xEE, -7
DEV = "cuda:0"


def to_dev(a):
    """numpy array -> device tensor of the same bytes (torch has no unsigned 32/64-bit arithmetic)."""
    import torch

    a = np.ascontiguousarray(a)
    signed = {1: np.uint8, 4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return torch.from_numpy(a.view(signed)).to(DEV)


class Guarded:
    """An output of n elements, preset to `fill`, between two guards of GUARD elements."""

    def __init__(self, n, np_dtype, fill):
        import torch

        self.n, self.np_dtype, self.fill = n, np.dtype(np_dtype), fill
        tdt = {np.dtype(np.uint8): torch.uint8, np.dtype(np.int32): torch.int32, np.dtype(np.uint32): torch.int32}
        tfill = fill - (1 << 32) if self.np_dtype == np.uint32 and fill >= 1 << 31 else fill
        self.t = torch.full((n + 2 * GUARD,), tfill, dtype=tdt[self.np_dtype], device=DEV)

    @property
    def ptr(self):
        return self.t.data_ptr() + GUARD * self.np_dtype.itemsize

    def read(self, what):
        """The n elements, after checking that both guards still hold the fill."""
        h = self.t.cpu().numpy().view(self.np_dtype)
        for side, g in (("before", h[:GUARD]), ("after", h[GUARD + self.n:])):
            assert (g == self.np_dtype.type(self.fill)).all(), \
                f"{what}: written {side} its range at guard elements {np.flatnonzero(g != self.fill).tolist()}"
        return h[GUARD:GUARD + self.n].copy()


class TallyOut:
    def __init__(self, nreq, nch):
        self.bits = Guarded((nreq + 31) // 32, np.uint32, BITS_FILL)
        self.reason = Guarded(nreq, np.uint8, BYTE_FILL)
        self.chosen = Guarded(nch, np.int32, CHOSEN_FILL)

    def read(self, what):
        return (self.bits.read(f"{what} accept_bits"), self.reason.read(f"{what} reason"),
                self.chosen.read(f"{what} chosen"))


def launch_tally(nreq, t, R, out, stream, chosen=True, chosen_off=True, reason=True):
    """One mochi_tally_responses_device call; t = the six input tensors in argument order."""
    rc = mh.load_library().mochi_tally_responses_device(
        nreq, *[x.data_ptr() for x in t[:5]], t[5].data_ptr() if chosen_off else None, R,
        out.chosen.ptr if chosen else None, out.reason.ptr if reason else None, out.bits.ptr, stream)
    assert rc == mh.OK, rc


def launch_classify(nreq, t, decision, stream, grants=True):
    """One mochi_write1_classify_device call; t = the seven input tensors in argument order."""
    g = [x.data_ptr() for x in t[4:7]] if grants else [None, None, None]
    rc = mh.load_library().mochi_write1_classify_device(nreq, *[x.data_ptr() for x in t[:4]], *g, decision.ptr, stream)
    assert rc == mh.OK, rc


def current_stream():
    import torch

    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def pack_bits(accept):
    bits = np.packbits(np.asarray(accept, bool), bitorder="little")
    return np.concatenate([bits, np.zeros(-bits.size % 4, np.uint8)]).view("<u4")


def tally_expectation(reason, chosen, n_ops, chosen_off, nch):
    """(accept_bits words, reason, the whole chosen array) from per-request model results:
    the tail bits of the last word are 0 and chosen keeps its fill outside every request's range."""
    full = np.full(nch, CHOSEN_FILL, np.int32)
    for r, ch in enumerate(chosen):
        assert len(ch) == n_ops[r]
        full[int(chosen_off[r]):int(chosen_off[r]) + n_ops[r]] = ch
    return pack_bits([w == 0 for w in reason]), np.asarray(reason, np.uint8), full


def assert_tally(got, want, names, what):
    for name, g, w in zip(("accept_bits", "reason", "chosen"), got, want):
        bad = np.flatnonzero(g != w)
        where = f" (request {names[bad[0]]})" if bad.size and name == "reason" else ""
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name}{where}")


@functools.lru_cache(maxsize=None)
def packed_tally(label):
    b = M.tally_batches()[label]
    arrs = mh._pack_responses(b.responses, b.n_ops)
    return b, arrs[:6], arrs[6]


@functools.lru_cache(maxsize=None)
def host_tally(label):
    b = M.tally_batches()[label]
    return mh.tally_responses(b.responses, b.n_ops, b.R)


def run_tally(nreq, arrs, R, nch, **kw):
    import torch

    out = TallyOut(nreq, nch)
    launch_tally(nreq, [to_dev(a) for a in arrs], R, out, current_stream(), **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("label", M.TALLY_LABELS)
def test_tally_sets_device_equals_model_and_host(label):
    """Every tally set: accept_bits word for word (tail bits 0), reason, and the whole chosen
    array == the model == the host C++; no guard element of any output is touched."""
    b, arrs, nch = packed_tally(label)
    nreq = len(b.names)
    got = run_tally(nreq, arrs, b.R, nch).read(label)
    want = tally_expectation(b.reason, b.chosen, b.n_ops, arrs[5], nch)
    assert_tally(got, want, b.names, f"device vs model, {label}")
    # the sentinel survives nowhere inside a request's [chosen_off[r], chosen_off[r] + k)
    assert (got[2][:sum(b.n_ops)] != CHOSEN_FILL).all()
    h_acc, h_reason, h_chosen = host_tally(label)
    assert_tally(got, tally_expectation(h_reason.tolist(), [c.tolist() for c in h_chosen], b.n_ops, arrs[5], nch),
                 b.names, f"device vs host, {label}")
    np.testing.assert_array_equal(mh.unpack_bits(got[0], nreq), h_acc)


def run_classify(requests, grants=True):
    import torch

    a = mh.pack_write1(requests)
    decision = Guarded(len(requests), np.uint8, BYTE_FILL)
    launch_classify(len(requests), [to_dev(x) for x in a], decision, current_stream(), grants)
    torch.cuda.synchronize()
    return decision


@pytest.mark.parametrize("label", M.CLASSIFY_LABELS)
def test_classify_sets_device_equals_model_and_host(label):
    """Every classify set: decision == the model (the oracle for dup_in_response, which is
    outside the model's contract) == the host C++; no guard element is touched."""
    b = M.classify_batches()[label]
    got = run_classify(b.responses).read(label)
    want = np.asarray(b.decision, np.uint8) if b.decision is not None else O.write1_classify(b.responses)
    bad = np.flatnonzero(got != want)
    assert not bad.size, f"{label}: {bad.size} differ, first {b.names[bad[0]]}: got {got[bad[0]]}, want {want[bad[0]]}"
    np.testing.assert_array_equal(got, mh.write1_classify(b.responses))


OPTIONAL_SET = "geometry_257"  # all three reasons, k = 1..3, a partial last word


def test_tally_optional_outputs():
    """chosen = NULL (chosen_off NULL or not), reason = NULL, both NULL: accept_bits and the
    outputs still asked for are those of the full call."""
    b, arrs, nch = packed_tally(OPTIONAL_SET)
    nreq = len(b.names)
    bits, reason, chosen = run_tally(nreq, arrs, b.R, nch).read("full")
    assert_tally((bits, reason, chosen), tally_expectation(b.reason, b.chosen, b.n_ops, arrs[5], nch), b.names, "full")
    untouched = (np.full(nreq, BYTE_FILL, np.uint8), np.full(nch, CHOSEN_FILL, np.int32))
    for kw in (dict(chosen=False), dict(chosen=False, chosen_off=False), dict(reason=False),
               dict(chosen=False, reason=False), dict(chosen=False, chosen_off=False, reason=False)):
        got = run_tally(nreq, arrs, b.R, nch, **kw).read(str(kw))
        want = (bits, reason if kw.get("reason", True) else untouched[0], chosen if kw.get("chosen", True) else untouched[1])
        assert_tally(got, want, b.names, str(kw))


def test_tally_layouts():
    """chosen_off descending with gaps (which keep their fill), status slices stored in
    reversed order, and every response aliasing one shared slice per distinct status vector."""
    b, arrs, nch = packed_tally(OPTIONAL_SET)
    nreq = len(b.names)
    resp_off, n_ops, rn, so, st, co = arrs
    # chosen_off: request r sits below request r-1, three untouched entries between them
    gap = 3
    co_desc = np.zeros(nreq, np.uint64)
    top = sum(b.n_ops) + gap * (nreq + 1)
    pos = top
    for r in range(nreq):
        pos -= b.n_ops[r] + gap
        co_desc[r] = pos
    assert pos == gap and (np.diff(co_desc.astype(np.int64)) < 0).all()
    got = run_tally(nreq, (resp_off, n_ops, rn, so, st, co_desc), b.R, top).read("descending chosen_off")
    want = tally_expectation(b.reason, b.chosen, b.n_ops, co_desc, top)
    assert (want[2] == CHOSEN_FILL).sum() == gap * (nreq + 1)
    assert_tally(got, want, b.names, "descending chosen_off")
    # status_off reversed: the slice of response q lies before that of response q-1
    so_rev = (st.size - so.astype(np.int64) - rn.astype(np.int64)).astype(np.uint64)
    st_rev = np.empty_like(st)
    for q in range(so.size):
        st_rev[int(so_rev[q]):int(so_rev[q]) + int(rn[q])] = st[int(so[q]):int(so[q]) + int(rn[q])]
    assert (np.diff(so_rev.astype(np.int64)) <= 0).all()
    want = tally_expectation(b.reason, b.chosen, b.n_ops, co, nch)
    got = run_tally(nreq, (resp_off, n_ops, rn, so_rev, st_rev, co), b.R, nch).read("reversed status_off")
    assert_tally(got, want, b.names, "reversed status_off")
    # aliasing: one stored slice per distinct status vector
    pool, where = [], {}
    so_alias = np.zeros_like(so)
    for q in range(so.size):
        v = tuple(st[int(so[q]):int(so[q]) + int(rn[q])].tolist())
        if v not in where:
            where[v] = len(pool)
            pool.extend(v)
        so_alias[q] = where[v]
    assert len(where) < so.size // 8
    got = run_tally(nreq, (resp_off, n_ops, rn, so_alias, np.asarray(pool, np.uint8), co), b.R, nch).read("aliased")
    assert_tally(got, want, b.names, "aliased status slices")


def test_tally_status_off_past_4gib():
    """status_off is 64-bit: statuses in the last 4 KiB of a buffer of 2^32 + 4096 bytes.  The
    first 4 KiB, where offsets narrowed to 32 bits would land, hold the opposite statuses."""
    import torch

    free, _ = torch.cuda.mem_get_info(torch.device(DEV))
    if free < 8 << 30:
        pytest.skip(f"{free >> 20} MiB of device memory free, the test wants 8 GiB")
    b, arrs, nch = packed_tally("geometry_31")
    nreq = len(b.names)
    assert set(b.reason) == {0, 1, 2}
    resp_off, n_ops, rn, so, st, co = arrs
    assert st.size <= 4096 and set(st.tolist()) <= {0, 1}
    size = (1 << 32) + 4096
    big = torch.empty(size, dtype=torch.uint8, device=DEV)
    big[:4096] = 1
    big[4096 - st.size:4096] = to_dev(1 - st)
    big[size - st.size:] = to_dev(st)
    so_far = so + np.uint64(size - st.size)
    assert so_far.min() >= 1 << 32
    out = TallyOut(nreq, nch)
    launch_tally(nreq, [to_dev(a) for a in (resp_off, n_ops, rn, so_far)] + [big, to_dev(co)], b.R, out, current_stream())
    torch.cuda.synchronize()
    got = out.read("status_off past 2^32")
    del big
    assert_tally(got, tally_expectation(b.reason, b.chosen, b.n_ops, co, nch), b.names, "status_off past 2^32")


def busy(work):
    """A few milliseconds of work on the current stream, so that a launch that did not wait
    for what the stream holds would run ahead of it."""
    for _ in range(24):
        work.mul_(1.0001)


def test_stream_order():
    """Inputs made on a non-default stream by a device-side copy behind other work, the call on
    that stream with no synchronisation in between; and two calls on two streams with
    different batches.  Until the copy lands the status / timestamp arrays hold values that
    give other results (all WRONG_SHARD; all timestamps equal) and are as valid to read."""
    import torch

    d = torch.device(DEV)
    s1, s2 = torch.cuda.Stream(d), torch.cuda.Stream(d)
    assert s1.cuda_stream != current_stream() and s1.cuda_stream != s2.cuda_stream
    tb, ta, tn = packed_tally("geometry_513")
    ub, ua, un = packed_tally("majority_line_R7")
    cb = M.classify_batches()["keys"]
    ca = mh.pack_write1(cb.responses)
    assert M.RETRY in cb.decision
    # everything but the stream-ordered input is in place, and synchronised, beforehand
    t_in, u_in, c_in = ([to_dev(a) for a in arrs] for arrs in (ta, ua, ca))
    t_real, u_real, c_real = t_in[4], u_in[4], c_in[5]
    t_in[4], u_in[4], c_in[5] = torch.ones_like(t_real), torch.ones_like(u_real), torch.zeros_like(c_real)
    t_out, u_out = TallyOut(len(tb.names), tn), TallyOut(len(ub.names), un)
    c_out = Guarded(len(cb.names), np.uint8, BYTE_FILL)
    work1, work2 = (torch.ones(32 << 20, dtype=torch.float32, device=d) for _ in range(2))
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        busy(work1)
        t_in[4].copy_(t_real)
        launch_tally(len(tb.names), t_in, tb.R, t_out, s1.cuda_stream)
        c_in[5].copy_(c_real + 0)
        launch_classify(len(cb.names), c_in, c_out, s1.cuda_stream)
    with torch.cuda.stream(s2):
        busy(work2)
        u_in[4].copy_(u_real)
        launch_tally(len(ub.names), u_in, ub.R, u_out, s2.cuda_stream)
    s1.synchronize()
    s2.synchronize()
    torch.cuda.synchronize()
    assert_tally(t_out.read("stream 1"), tally_expectation(tb.reason, tb.chosen, tb.n_ops, ta[5], tn), tb.names, "stream 1")
    assert_tally(u_out.read("stream 2"), tally_expectation(ub.reason, ub.chosen, ub.n_ops, ua[5], un), ub.names, "stream 2")
    np.testing.assert_array_equal(c_out.read("stream 1 classify"), np.asarray(cb.decision, np.uint8))


def test_zero_requests_touch_nothing():
    """n_requests = 0: MOCHI_OK with NULL pointers, and no prefilled output is written."""
    import torch

    lib = mh.load_library()
    stream = current_stream()
    assert lib.mochi_tally_responses_device(0, None, None, None, None, None, None, 4, None, None, None, stream) == mh.OK
    assert lib.mochi_write1_classify_device(0, None, None, None, None, None, None, None, None, stream) == mh.OK
    b, arrs, nch = packed_tally("geometry_33")
    out = TallyOut(len(b.names), nch)
    launch_tally(0, [to_dev(a) for a in arrs], b.R, out, stream)
    cb = M.classify_batches()["geometry_255"]
    decision = Guarded(len(cb.names), np.uint8, BYTE_FILL)
    launch_classify(0, [to_dev(x) for x in mh.pack_write1(cb.responses)], decision, stream)
    torch.cuda.synchronize()
    bits, reason, chosen = out.read("n_requests = 0")
    assert (bits == BITS_FILL).all() and (reason == BYTE_FILL).all() and (chosen == CHOSEN_FILL).all()
    assert (decision.read("n_requests = 0") == BYTE_FILL).all()


def test_classify_null_grant_arrays():
    """No response has a grant (resp_grant_off all zero): the grant arrays are never read and
    may be NULL, on the device as on the host."""
    import itertools

    options = [(kind, sid, []) for kind in (M.OK, M.REFUSED, M.REQUEST_FAILED, M.OTHER) for sid in (0, 1)]
    requests = [list(r) for n in range(4) for r in itertools.product(options, repeat=n)]
    a = mh.pack_write1(requests)
    assert not a[3].any()
    host = np.full(len(requests), BYTE_FILL, np.uint8)
    rc = mh.load_library().mochi_write1_classify(len(requests), *[x.ctypes.data for x in a[:4]], None, None, None,
                                                 host.ctypes.data)
    assert rc == mh.OK
    got = run_classify(requests, grants=False).read("NULL grant arrays")
    np.testing.assert_array_equal(got, host)
    np.testing.assert_array_equal(got, np.asarray([M.classify(r) for r in requests], np.uint8))
    assert set(got.tolist()) == {M.PROCEED, M.THROW_REFUSED, M.THROW_FAILED}
