"""Write1 reply decoder on the GPU (mochi_write1_reply_decode_device): the device form
equals the host form array for array on the reply encoder's bodies and the mutation
corpus (guard-filled outputs, a stream of its own); response counts around the block and
empty-batch edges of its launch sequence; optional outputs; the capacity rule; two
streams agree; the profile; and the client's round with no Python parsing -- four
servers' replies decoded, classified, assembled into Write2ToServer bodies and
accepted by the verifier -- with a second batch whose decisions equal the client
model's; and the parts only the device form has, at their edges: later passes of the
grid-stride level-2 kernel and its block cap, wire offsets past 4 GiB, requests without
responses or ops, a signature that ends the wire, scratch that grows between streams."""

import numpy as np
import pytest

import client_model as CM
import mochi_hip as mh
import workload as W
import write1_decode_model as DM
import write1_issue_model as M
import write1_reply_model as RM

pytestmark = pytest.mark.gpu

KIND_OF, SERVER_IDS, replies_of = DM.KIND_OF, DM.REPLY_SERVER_IDS, DM.replies_of

FILL = 0xA5


@pytest.fixture(scope="module")
def pems():
    return W.load_keys(4)


@pytest.fixture(scope="module")
def ver(pems):
    v = mh.Verifier([mh.pem_modulus(p) for p in pems], 0)
    v.set_server_ids(DM.IDS)
    yield v
    v.close()


@pytest.fixture(scope="module")
def corpus_batch():
    return DM.batch(DM.corpus())


def _decode_device(ver, replies, grant_cap, cert_cap, want_sig=True, stream=None, check=True, dr=None):
    """dr: the batch already on the device (`replies` is not read then)."""
    import torch

    s = stream or torch.cuda.Stream()
    dr = dr or mh.DeviceWrite1Replies(replies, 0)
    out = mh.DeviceWrite1Decoded(dr.n_resps, grant_cap, cert_cap, want_sig, fill=FILL)
    torch.cuda.synchronize()  # uploads and fills went to the current stream
    rc = ver.write1_reply_decode_device(dr, out, stream=s.cuda_stream, check=check)
    torch.cuda.synchronize()
    return out.to_host(rc)


def _assert_decoded(got, want, N, C, want_sig=True):
    """The guard-filled device outputs `got` hold the trimmed arrays `want` and nothing else."""
    assert got.rc == mh.OK and (got.n_grants, got.n_certs) == (N, C)
    DM.assert_equal(got.trimmed(), want)
    for k, (dt, w) in mh._W1D_OUT.items():  # nothing past the counts is written
        if w in ("N", "C"):
            assert (got.arrays[k][N if w == "N" else C:].view(np.uint8) == FILL).all(), k
    if want_sig:
        assert (got.arrays["sig"][N:] == FILL).all()


def _device_equals_host(ver, replies, ids, slack=3, want_sig=True, model=False):
    """model: the device outputs also equal the Python model's, compared directly."""
    host = mh.write1_reply_decode(replies, ids, want_sig)
    N, C = host.n_grants, host.n_certs
    got = _decode_device(ver, replies, N + slack, C + slack, want_sig)
    _assert_decoded(got, host.trimmed(), N, C, want_sig)
    if model:
        want = DM.decode(replies, ids)
        DM.assert_equal(got.trimmed(), want if want_sig else {k: v for k, v in want.items() if k != "sig"})
    return host


@pytest.fixture
def ver_ids(ver):
    """The shared context with another id table for one test."""
    def use(ids):
        ver.set_server_ids(ids)
        return ver
    yield use
    ver.set_server_ids(DM.IDS)


# 1. device == host ---------------------------------------------------------------------------
def test_corpus_device_equals_host(ver, corpus_batch):
    host = _device_equals_host(ver, corpus_batch, DM.IDS)
    assert set(host.arrays["resp_status"].tolist()) == {0, 1, 2, 3}


def test_corpus_in_aliased_slices_device_equals_host(ver):
    cases = DM.corpus()
    _device_equals_host(ver, DM.batch(cases + cases[::-1], layout="shared", per_req=3), DM.IDS)


@pytest.mark.parametrize("name", sorted(RM.reply_cases()))
def test_reply_encoder_bodies_device_equals_host(ver_ids, name):
    _device_equals_host(ver_ids(SERVER_IDS), replies_of(RM.reply_cases()[name]), SERVER_IDS)


# 2. the launch sequence's edges: no response at all, and one below / at / above a block of 256
@pytest.mark.parametrize("P", [0, 1, 255, 256, 257])
def test_response_counts_around_the_launch_edges(ver, P):
    cases = [c for c in DM.corpus() if not c.name.startswith("cut:")]
    cases = tuple(cases[i % len(cases)] for i in range(P))
    if P == 0:
        r = mh.Write1Replies(wire=np.zeros(1, np.uint8), resp_off=np.zeros(0, np.uint64), resp_len=np.zeros(0, np.uint32),
                             resp_kind=np.zeros(0, np.uint8), req_resp_off=np.zeros(1, np.uint32),
                             strings=np.zeros(1, np.uint8), req_op_off=np.zeros(1, np.uint32),
                             op_key_off=np.zeros(0, np.uint64), op_key_len=np.zeros(0, np.uint32))
    else:
        r = DM.batch(cases)
    _device_equals_host(ver, r, DM.IDS)


# 3. optional outputs, the capacity rule ----------------------------------------------------------
def test_signatures_not_wanted(ver, corpus_batch):
    _device_equals_host(ver, corpus_batch, DM.IDS, want_sig=False)


@pytest.mark.parametrize("short", ["grants", "certs"])
def test_capacity_one_short_touches_nothing(ver, corpus_batch, short):
    host = mh.write1_reply_decode(corpus_batch, DM.IDS)
    N, C = host.n_grants, host.n_certs
    got = _decode_device(ver, corpus_batch, N - (short == "grants"), C - (short == "certs"), check=False)
    assert got.rc == mh.EINVAL and (got.n_grants, got.n_certs) == (N, C)
    for k, (dt, w) in mh._W1D_OUT.items():
        if w in ("N", "C"):
            assert (got.arrays[k].view(np.uint8) == FILL).all(), k
        else:
            np.testing.assert_array_equal(got.arrays[k], host.arrays[k])
    assert (got.arrays["sig"] == FILL).all()


def test_needs_server_ids(pems, corpus_batch):
    v = mh.Verifier([mh.pem_modulus(p) for p in pems], 0)
    with pytest.raises(mh.MochiError, match="server ids not set"):
        v.write1_reply_decode_device(mh.DeviceWrite1Replies(corpus_batch, 0), mh.DeviceWrite1Decoded(corpus_batch.n_resps, 8, 8))
    v.close()


# 4. two streams, the profile ---------------------------------------------------------------------
def test_two_streams_give_equal_bytes(ver, corpus_batch):
    import torch

    host = mh.write1_reply_decode(corpus_batch, DM.IDS)
    dr = mh.DeviceWrite1Replies(corpus_batch, 0)
    outs = [mh.DeviceWrite1Decoded(corpus_batch.n_resps, host.n_grants, host.n_certs, fill=FILL) for _ in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for o, s in zip(outs, streams):
        assert ver.write1_reply_decode_device(dr, o, stream=s.cuda_stream) == mh.OK
    torch.cuda.synchronize()
    for k in list(mh._W1D_OUT) + ["sig"]:
        assert torch.equal(getattr(outs[0], k), getattr(outs[1], k)), k
    DM.assert_equal(outs[1].to_host().trimmed(), host.trimmed())


def test_profile_reader(ver, corpus_batch):
    host = mh.write1_reply_decode(corpus_batch, DM.IDS)
    ver.set_profiling(True)
    try:
        got = _decode_device(ver, corpus_batch, host.n_grants, host.n_certs)
        prof = ver.read_w1_decode_profile()
    finally:
        ver.set_profiling(False)
    assert got.rc == mh.OK and tuple(prof) == mh.W1_DECODE_STAGES
    assert all(v >= 0 for v in prof.values()) and prof["k_w1d_resp"] > 0 and prof["k_w1d_level2"] > 0 and prof["k_w1d_emit"] > 0


# 5. the client's round on the device -------------------------------------------------------------
R, Q, K = 4, 8, 2


def _four_servers(pems, batch_of=lambda s, plain: plain):
    """Every server issues, signs and encodes its replies for the batch; the four blobs
    concatenated ON THE DEVICE into one Write1Replies (request q's responses in server
    order).  Returns (device replies, the device batch, the host batch)."""
    import torch

    n_ops = Q * K
    plain = W.write1_batch(np.arange(n_ops), np.arange(Q + 1) * K, np.full(Q, 6), np.arange(Q))
    st = torch.cuda.current_stream().cuda_stream
    wires, offs, lens, kinds, d0 = [], [], [], [], None
    base = 0
    for s in range(R):
        b = batch_of(s, plain)
        src = RM.make_source(b, [b"\x0a\x03old\x10\x05"] * b.n_stored, certs=False, sigs=True,
                             server=W.SERVER_IDS[s].encode(), client_of=lambda q: b"")
        signer = mh.DeviceSigner(pems[s], 0)
        db, ds = mh.DeviceWrite1Batch(b, 0), mh.DeviceWrite1ReplySource(src, 0)
        d0 = d0 or db
        out = mh.DeviceWrite1Issued(Q, n_ops, mh.write1_issue_bound(b), sign=True)
        cap = mh.write1_reply_bound(b, src, out.grant_cap, True)
        wire = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
        off = torch.zeros(Q, dtype=torch.int64, device="cuda:0")
        ln = torch.zeros(Q, dtype=torch.int32, device="cuda:0")
        status = torch.zeros(Q, dtype=torch.uint8, device="cuda:0")
        assert signer.issue_device(db, out, stream=st) == mh.OK
        rc, total = signer.reply_encode_device(db, out, ds, wire, off, ln, status, stream=st)
        torch.cuda.synchronize()
        signer.close()
        assert rc == mh.OK and bool((status == 0).all())
        wires.append(wire[:total])
        offs.append(off + base)
        lens.append(ln)
        kinds.append(out.req_kind[:Q])  # W1K_* and W1_* number OK / REFUSED / THROWS -> REQUEST_FAILED alike
        base += total
    assert KIND_OF == {0: 0, 1: 1, 2: 2}
    i32 = lambda a: torch.from_numpy(np.asarray(a, np.uint32).view(np.int32)).to("cuda:0")
    dr = mh.DeviceWrite1Replies.from_tensors(
        Q * R, Q, n_ops, wire=torch.cat(wires), resp_off=torch.stack(offs, 1).reshape(-1).contiguous(),
        resp_len=torch.stack(lens, 1).reshape(-1).contiguous(), resp_kind=torch.stack(kinds, 1).reshape(-1).contiguous(),
        req_resp_off=i32(np.arange(Q + 1) * R), strings=d0.strings, req_op_off=d0.req_op_off,
        op_key_off=d0.op_key_off, op_key_len=d0.op_key_len)
    return dr, d0, plain


def _classify_device(ver, dr, dec):
    import torch

    decision = torch.full((Q,), 0xEE, dtype=torch.uint8, device="cuda:0")
    rc = ver.lib.mochi_write1_classify_device(Q, dr.req_resp_off.data_ptr(), dec.resp_kind_out.data_ptr(),
                                              dec.resp_server.data_ptr(), dec.resp_grant_off.data_ptr(),
                                              dec.grant_key.data_ptr(), dec.grant_ts.data_ptr(),
                                              dec.grant_status.data_ptr(), decision.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream)
    assert rc == mh.OK
    return decision


def test_chain_decode_classify_encode_verify(pems):
    import torch

    dr, d0, plain = _four_servers(pems)
    ver = mh.Verifier([mh.pem_modulus(p) for p in pems], 0)
    ver.set_server_ids(W.SERVER_IDS[:R])
    st = torch.cuda.current_stream().cuda_stream
    n_ops = Q * K
    dec = mh.DeviceWrite1Decoded(Q * R, Q * R * K, 1, fill=FILL)
    assert ver.write1_reply_decode_device(dr, dec, stream=st) == mh.OK
    assert (dec.n_grants, dec.n_certs) == (Q * R * K, 0)
    decision = _classify_device(ver, dr, dec)
    src = mh.DeviceWrite2Source.from_tensors(
        Q, Q * R, dec.n_grants, n_ops, grant_bytes=dr.wire, grant_off=dec.grant_off, grant_len=dec.grant_len, sig=dec.sig,
        cert_mg_off=dr.req_resp_off, mg_grant_off=dec.resp_grant_off, mg_signer=dec.mg_signer, strings=d0.strings,
        cert_op_off=d0.req_op_off, op_action=torch.full((n_ops,), M.WRITE, dtype=torch.uint8, device="cuda:0"),
        op1_off=d0.op_key_off, op1_len=d0.op_key_len)
    off = torch.zeros(Q, dtype=torch.int64, device="cuda:0")
    ln = torch.zeros(Q, dtype=torch.int32, device="cuda:0")
    status = torch.zeros(Q, dtype=torch.uint8, device="cuda:0")
    rc, cap = ver.encode_write2_device(src, None, off, ln, status, stream=st, check=False)
    assert rc == mh.EINVAL and cap > 0
    wire = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
    ver.encode_write2_device(src, wire, off, ln, status, stream=st)
    h0 = int(plain.req_hash_off[0])
    dwb = mh.DeviceWireBatch.from_encoded(wire, off, ln, Q, d0.strings[h0:h0 + Q * mh.TXN_HASH_BYTES], d0.req_op_off,
                                          np.full(n_ops, mh.OP_LOCAL | mh.OP_HAS_SVOC, np.uint8))
    verdicts = mh.DeviceVerdicts(0, Q, 0, full=True, n_ops=n_ops)
    ver.verify_write2_device(dwb, verdicts, R, True, stream=st)
    torch.cuda.synchronize()
    h = dec.to_host().trimmed()
    assert (h["resp_status"] == mh.W1R_OK).all() and h["mg_signer"].tolist() == list(range(R)) * Q
    assert (h["grant_flags"] == mh.W1G_HAS_SIG).all() and h["grant_key"].tolist() == list(range(K)) * (Q * R)
    assert decision.cpu().numpy().tolist() == [mh.W1_PROCEED] * Q
    assert bool((status == 0).all()) and bool((dwb.status[:Q] == 0).all())
    v = verdicts.to_host()
    ver.close()
    assert mh.unpack_bits(v.cert_accept_bits, Q).all() and (v.cert_reason == 0).all()


def test_classifier_on_a_mixed_batch_equals_the_client_model(pems):
    """Server 3's reply is REFUSED for request 1 (a stored grant with another hash), malformed
    for request 2 (its last byte cut off by the length) and a timestamp off for request 3
    (another seed); the device decisions equal client_model's on the MODEL-decoded arrays."""
    import torch

    n_ops = Q * K
    stored = np.full(n_ops, mh.W1_NONE, np.uint32)
    stored[1 * K] = 0
    seeds = np.full(Q, 6)
    seeds[3] = 7
    other = W.write1_batch(np.arange(n_ops), np.arange(Q + 1) * K, seeds, np.arange(Q), op_stored=stored,
                           stored_hash_id=[999])
    dr, d0, plain = _four_servers(pems, lambda s, plain: other if s == 3 else plain)
    dr.resp_len[2 * R + 3] -= 1  # request 2, server 3: truncated
    ver = mh.Verifier([mh.pem_modulus(p) for p in pems], 0)
    ver.set_server_ids(W.SERVER_IDS[:R])
    dec = mh.DeviceWrite1Decoded(Q * R, Q * R * K, 1, fill=FILL)
    assert ver.write1_reply_decode_device(dr, dec, stream=torch.cuda.current_stream().cuda_stream) == mh.OK
    decision = _classify_device(ver, dr, dec).cpu().numpy()
    torch.cuda.synchronize()
    ver.close()
    h = lambda t, dt: t.cpu().numpy().view(dt)
    host = mh.Write1Replies(wire=h(dr.wire, np.uint8), resp_off=h(dr.resp_off, np.uint64), resp_len=h(dr.resp_len, np.uint32),
                            resp_kind=h(dr.resp_kind, np.uint8), req_resp_off=h(dr.req_resp_off, np.uint32),
                            strings=h(d0.strings, np.uint8), req_op_off=h(d0.req_op_off, np.uint32),
                            op_key_off=h(d0.op_key_off, np.uint64), op_key_len=h(d0.op_key_len, np.uint32))
    want = DM.decode(host, W.SERVER_IDS[:R])
    DM.assert_equal(dec.to_host().trimmed(), want)
    assert want["resp_kind_out"][1 * R + 3] == mh.W1_REFUSED and want["resp_status"][2 * R + 3] == mh.W1R_MALFORMED
    model = []
    for q in range(Q):
        resps = []
        for p in range(q * R, (q + 1) * R):
            g0, g1 = int(want["resp_grant_off"][p]), int(want["resp_grant_off"][p + 1])
            resps.append((int(want["resp_kind_out"][p]), int(want["resp_server"][p]),
                          [(int(want["grant_key"][g]), int(want["grant_ts"][g]), int(want["grant_status"][g]))
                           for g in range(g0, g1)]))
        model.append(CM.classify(resps))
    assert decision.tolist() == model
    assert model[1] == mh.W1_THROW_REFUSED and model[2] == mh.W1_THROW_REFUSED and model[3] == mh.W1_RETRY
    assert all(model[q] == mh.W1_PROCEED for q in (0, 4, 5, 6, 7))


# 6. the level-2 grid: later passes of the grid-stride loop, the block cap ----------------------
def _l2_lanes(P):
    """Lanes of k_w1d_level2's grid: w1_decode.hip's l2_blocks(P) blocks, clamp(ceil(2P / 256), 1, 4096), of 256."""
    return 256 * min(max(-(-2 * P // 256), 1), 4096)


def _entry_bases(cases):
    """Index of each response's first level-2 entry, and the total last (from the model)."""
    return np.concatenate([[0], np.cumsum([DM.level2_entries(c.body, c.kind) for c in cases])]).tolist()


# shape -> (cases, full passes the entries exceed, a response whose entries all lie past the first pass but for its first `head`)
def _l2_shape(shape):
    ec = DM.edge_cases()
    if shape == "4_ok":  # the smallest second pass: 260 entries on 256 lanes (the four entries left are valid)
        return (ec["ok:heavy"],) * 4, 1, None
    if shape == "4_last_bad":  # ... and the last of them, entry 259, is the MALFORMED one
        return (ec["ok:heavy"],) * 3 + (ec["mal:heavy_bad_63"],), 1, None
    P = int(shape)
    return DM.pattern_cases(P), {12: 1, 300: 10}[P], 10  # response 10, bad at 0 and 63: entries 260..324


@pytest.mark.parametrize("layout", ["packed", "shared"])
@pytest.mark.parametrize("shape", ["4_ok", "4_last_bad", "12", "300"])
def test_level2_later_passes(ver, shape, layout):
    cases, passes, late = _l2_shape(shape)
    P, lanes, base = len(cases), _l2_lanes(len(cases)), _entry_bases(cases)
    # the preconditions, from the model: without them the test would pass without a later pass
    assert base[-1] > passes * lanes, (base[-1], lanes)
    if shape == "4_last_bad":
        assert base[3] + 64 >= lanes  # certificate entry 63 of response 3
    if late is not None:
        assert base[late] >= 256 and base[late + 1] - base[late] == 65 and base[late - 1] == base[late]
        assert base[1] == base[2] == 0 and base[3] == base[6] and base[11] == base[12]  # runs without entries
    if P == 300:
        assert lanes == 3 * 256
    r = DM.batch(cases, layout=layout, per_req=3)
    assert DM.n_level2_entries(r) == base[-1]
    host = _device_equals_host(ver, r, DM.IDS, model=P <= 12)
    st = host.arrays["resp_status"]
    assert st.tolist()[:P] == [{"ok": mh.W1R_OK, "mal": mh.W1R_MALFORMED, "fb": mh.W1R_FALLBACK, "kind": mh.W1R_OK}
                               [c.name.split(":")[0]] for c in cases]


@pytest.mark.parametrize("P, last, second_pass", [(524288, "small", False), (524289, "small", True), (524289, "heavy", True)])
def test_level2_block_cap(ver, P, last, second_pass):
    """4096 blocks: P = 524,288 fills them without the cap (2 entries a response, one pass);
    at P = 524,289 the cap holds and block 0 takes the last response's entries in a second
    pass.  The last response alone is MALFORMED, in its last entry."""
    body = DM.SMALL_BAD if last == "small" else DM.edge_cases()["mal:heavy_bad_63"].body
    r = DM.cap_batch(P, body)
    lanes, n = _l2_lanes(P), DM.n_level2_entries(r)
    assert lanes == 4096 * 256 == _l2_lanes(P + 1000) and n == 2 * (P - 1) + DM.level2_entries(body)
    assert (n > lanes) == second_pass and (second_pass or n == lanes)
    assert not second_pass or 2 * (P - 1) == lanes  # the last response's entries, and only they, are the second pass
    host = _device_equals_host(ver, r, DM.IDS, want_sig=False)
    st = host.arrays["resp_status"]
    assert st[-1] == mh.W1R_MALFORMED and (st[:-1] == mh.W1R_OK).all()
    assert host.n_grants == P - 1 == host.n_certs


# 7. wire offsets past 4 GiB -------------------------------------------------------------------------
def test_offsets_past_4_gib(ver):
    """Thirty-two bodies in the last 64 KiB of a wire of 2^32 + 64 KiB bytes: every offset the
    decoder emits is the low-offset decode's plus the displacement, the signatures its."""
    import torch

    size = (1 << 32) + (64 << 10)
    free, _ = torch.cuda.mem_get_info(torch.device("cuda", 0))
    if free < size + (512 << 20):
        pytest.skip(f"{free >> 20} MiB of device memory free, the test wants {(size >> 20) + 512}")
    cases = DM.far_cases()
    low = DM.batch(cases, per_req=3, mod=16)
    n = low.wire.size
    D = (size - n) // 16 * 16
    assert n <= 64 << 10 and D + int(low.resp_off.min()) >= 1 << 32
    assert {(int(o) + D) % 16 for o in low.resp_off} == set(range(16))
    host = mh.write1_reply_decode(low, DM.IDS)
    N, C = host.n_grants, host.n_certs
    want = {k: v.copy() for k, v in host.trimmed().items()}
    for k in ("grant_off", "cert_key_off", "cert_val_off"):
        want[k] += np.uint64(D)
    decoded = np.isin(low.resp_kind, [mh.W1_OK, mh.W1_REFUSED]) & np.isin(want["resp_status"], [mh.W1R_OK, mh.W1R_UNKNOWN_SERVER])
    want["resp_client_off"][decoded] += np.uint64(D)  # an undecoded response keeps 0 / 0
    assert decoded.any() and not decoded.all() and (want["resp_client_off"][~decoded] == 0).all()
    assert N > 16 and C > 64 and {s % 16 for s in DM.sig_sources(low, host.trimmed())} == set(range(16))
    small = mh.DeviceWrite1Replies(low, 0)
    big = torch.empty(size, dtype=torch.uint8, device="cuda:0")
    big[D:D + n] = small.wire
    dr = mh.DeviceWrite1Replies.from_tensors(
        low.n_resps, low.n_reqs, low.n_ops, wire=big, resp_off=small.resp_off + D, resp_len=small.resp_len,
        resp_kind=small.resp_kind, req_resp_off=small.req_resp_off, strings=small.strings, req_op_off=small.req_op_off,
        op_key_off=small.op_key_off, op_key_len=small.op_key_len)
    got = _decode_device(ver, None, N + 3, C + 3, dr=dr)
    del big, dr
    _assert_decoded(got, want, N, C)
    t = got.trimmed()
    for k in ("grant_off", "cert_key_off", "cert_val_off"):
        assert (t[k] >= 1 << 32).all(), k
    assert (t["resp_client_off"][decoded] >= 1 << 32).all()
    np.testing.assert_array_equal(t["sig"], host.trimmed()["sig"])


# 8. request grouping, the wire's end ------------------------------------------------------------------
def test_request_grouping_device_equals_host(ver):
    _device_equals_host(ver, DM.grouping_batch(), DM.IDS, model=True)


@pytest.mark.parametrize("residue", range(16))
def test_signature_ends_the_wire(ver, residue):
    """The last response ends on the wire's last byte and its signature is its last field:
    the gather's last chunk ends the buffer, the source at each position in a chunk."""
    by = {c.name: c for c in DM.corpus()}
    last = DM.Case("sig_last", DM.reply(DM.multigrant([(DM.K1, DM.grant(DM.K1, 11))])), (DM.K1,))
    cases = (by["rep:sigs"], by["mutate:2"], last)
    n0 = DM.batch(cases, per_req=2, lead=0, tail=0).wire.size
    r = DM.batch(cases, per_req=2, lead=(residue - (n0 - 256)) % 16, tail=0)
    assert int(r.resp_off[-1]) + int(r.resp_len[-1]) == r.wire.size and (r.wire.size - 256) % 16 == residue
    host = _device_equals_host(ver, r, DM.IDS, model=True)
    assert host.arrays["grant_flags"][-1] == mh.W1G_HAS_SIG
    np.testing.assert_array_equal(host.arrays["sig"][-1], r.wire[-256:])


# 9. scratch that grows between calls on two streams ------------------------------------------------------
@pytest.mark.parametrize("order", ["small_large_small", "large_small_large"])
def test_scratch_growth_across_streams(pems, order):
    """A fresh context; three calls alternating between two streams with nothing between them
    but what a call itself waits for; the second call's batch needs other scratch sizes
    than the first's.  Each call has guard-filled outputs of its own."""
    import torch

    small = DM.batch(tuple(c for c in DM.corpus() if c.name.startswith("mutate:"))[:8])
    large = DM.batch(DM.pattern_cases(300), per_req=3)
    seq = [small, large, small] if order == "small_large_small" else [large, small, large]
    hosts = [mh.write1_reply_decode(r, DM.IDS) for r in seq]
    assert hosts[0].n_grants > 0 and hosts[1].n_grants > 0
    drs = [mh.DeviceWrite1Replies(r, 0) for r in seq]
    outs = [mh.DeviceWrite1Decoded(r.n_resps, h.n_grants + 3, h.n_certs + 3, fill=FILL) for r, h in zip(seq, hosts)]
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    v = mh.Verifier([mh.pem_modulus(p) for p in pems], 0)
    v.set_server_ids(DM.IDS)
    torch.cuda.synchronize()
    rcs = [v.write1_reply_decode_device(dr, o, stream=s.cuda_stream) for dr, o, s in zip(drs, outs, (a, b, a))]
    torch.cuda.synchronize()
    v.close()
    for rc, o, h in zip(rcs, outs, hosts):
        _assert_decoded(o.to_host(rc), h.trimmed(), h.n_grants, h.n_certs)
