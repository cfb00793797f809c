"""Write2ToServer encoder on the GPU (mochi_write2_encode_device): the device
form equals the host form byte for byte, its output feeds
mochi_verify_write2_device without a host round trip, offsets are 64-bit, and
two calls on two streams give the same bytes."""
import numpy as np
import pytest

import mochi_hip as mh
import oracle_ffi as O
import w2_encode_cases as C
import workload as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ver7():
    """A context over the seven keys: its id table is the host tests' C.IDS."""
    v = mh.Verifier(C.pool(7, 2).moduli, 0)
    v.set_server_ids(C.IDS)
    yield v
    v.close()


@pytest.fixture(scope="module")
def sources():
    return C.device_sources()


def _outputs(M, cap, fill=0xEE):
    import torch

    dev = torch.device("cuda", 0)
    return (torch.full((max(cap, 1),), fill, dtype=torch.uint8, device=dev),
            torch.full((max(M, 1),), -1, dtype=torch.int64, device=dev),
            torch.full((max(M, 1),), -1, dtype=torch.int32, device=dev),
            torch.full((max(M, 1),), 0xEE, dtype=torch.uint8, device=dev))


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


# 1. device == host ----------------------------------------------------------
# align1023 / align1024: the single-block scan and the hipcub scan (the decoder's small-batch line)
# mutants / mutants1023: the grant mutation corpus on both paths.  The host form parses with wire_walk.h, the device
# form with proto_dev.h: the two Grant parsers against each other, group depths 16, 17, 100 and 101 included
@pytest.mark.parametrize("name", ["r4", "r7k2", "client", "nosig", "hand", "hand_nosig", "steps", "steps_nosig",
                                  "wc16383", "wc16384", "msg16383", "msg16384", "bad", "align1023", "align1024",
                                  "one", "none", "mutants", "mutants1023"])
def test_device_form_equals_host_form(ver7, sources, name):
    import torch

    src = sources[name]
    M = src.n_msgs
    rc, need, off, ln, st = mh.encode_write2_into(src, C.IDS, None)  # sizes
    hwire = np.zeros(max(need, 1), np.uint8)
    rc, need, off, ln, st = mh.encode_write2_into(src, C.IDS, hwire)
    assert rc == mh.OK
    dsrc = mh.DeviceWrite2Source(src, 0)
    wire, doff, dln, dst = _outputs(M, need + 64)
    rc, n = ver7.encode_write2_device(dsrc, wire, doff, dln, dst, stream=_stream())
    torch.cuda.synchronize()
    assert n == need
    w = wire.cpu().numpy()
    assert w[:need].tobytes() == hwire[:need].tobytes()
    assert (w[need:] == 0xEE).all()
    np.testing.assert_array_equal(doff.cpu().numpy().view(np.uint64)[:M], off)
    np.testing.assert_array_equal(dln.cpu().numpy().view(np.uint32)[:M], ln)
    np.testing.assert_array_equal(dst.cpu().numpy()[:M], st)
    if need:  # one byte short: refused, the size reported, nothing written
        wire2, doff, dln, dst = _outputs(M, need - 1)
        rc, n = ver7.encode_write2_device(dsrc, wire2, doff, dln, dst, stream=_stream(), check=False)
        torch.cuda.synchronize()
        assert rc == mh.EINVAL and n == need
        assert bool((wire2 == 0xEE).all())


def test_device_form_needs_server_ids():
    v = mh.Verifier(C.pool(4, 1).moduli, 0)
    src = C.hand_source()
    wire, off, ln, st = _outputs(src.n_msgs, 4096)
    rc, n = v.encode_write2_device(mh.DeviceWrite2Source(src, 0), wire, off, ln, st, check=False)
    assert rc == mh.EINVAL
    v.close()


# 2. encode -> verify, all on the device ----------------------------------------
@pytest.mark.parametrize("R,k", [(4, 1), (7, 2)])
def test_encoded_wire_verifies_like_the_soa_batch(R, k):
    import torch

    pool, s = C.pool(R, k), C.synth(R, k)
    b = s.batch
    ver = mh.Verifier(pool.moduli, 0)
    ver.set_server_ids(C.IDS[:R])
    src = W.write2_source(s)
    M, O_ = src.n_msgs, b.n_ops
    _, need, *_ = mh.encode_write2_into(src, C.IDS, None)
    wire, off, ln, st = _outputs(M, need)
    ver.encode_write2_device(mh.DeviceWrite2Source(src, 0), wire, off, ln, st, stream=_stream())
    dwb = mh.DeviceWireBatch.from_encoded(wire, off, ln, M, b.expected_hash, b.cert_op_off, b.op_flags)
    out = mh.DeviceVerdicts(0, M, 0, full=True, n_ops=O_)
    ver.verify_write2_device(dwb, out, R, True, stream=_stream())
    dev = mh.DeviceBatch(b, 0)
    soa = mh.DeviceVerdicts(dev.n_grants, dev.n_certs, 0, full=True, n_ops=dev.n_ops)
    ver.verify_device(dev, soa, R, True, stream=_stream())
    torch.cuda.synchronize()
    assert bool((st == 0).all()) and bool((dwb.status[:M] == 0).all())
    g, e = out.to_host(), soa.to_host()
    o = O.verify_batch(pool.moduli, b, R, True, 4)
    for key in ("cert_accept_bits", "cert_reason", "cert_fail_op", "op_decision", "op_g0", "op_ts"):
        np.testing.assert_array_equal(getattr(g, key), getattr(e, key), err_msg=key)
        np.testing.assert_array_equal(getattr(g, key), getattr(o, key), err_msg=key)
    acc = mh.unpack_bits(g.cert_accept_bits, M)
    assert acc.any() and not acc.all()
    ver.close()


# 3. 64-bit offsets --------------------------------------------------------------
def test_offsets_past_4_gib(ver7):
    """Message m carries the bytes of message m mod 64; M is just large enough
    for the wire to pass 2^32 bytes.  Only msg_off / msg_len come to the host."""
    import torch

    base = C.head(W.write2_source(C.synth(4, 1)), 64)
    hw, hoff, hln, _ = mh.encode_write2(base, C.IDS)
    M = 64 * (int((1 << 32) // hw.size) + 1)
    rep = M // 64
    tile = lambda a, step: (np.tile(a[:-1].astype(np.int64), rep) +
                            np.repeat(np.arange(rep, dtype=np.int64) * step, a.shape[0] - 1))
    nm, n, no = base.n_mgs, base.n_grants, base.n_ops
    src = mh.Write2Source(
        grant_bytes=base.grant_bytes, grant_off=np.tile(base.grant_off, rep), grant_len=np.tile(base.grant_len, rep),
        sig=None,
        cert_mg_off=np.append(tile(base.cert_mg_off, nm), rep * nm).astype(np.uint32),
        mg_grant_off=np.append(tile(base.mg_grant_off, n), rep * n).astype(np.uint32),
        mg_signer=np.tile(base.mg_signer, rep), strings=base.strings,
        cert_op_off=np.append(tile(base.cert_op_off, no), rep * no).astype(np.uint32),
        op_action=np.tile(base.op_action, rep), op1_off=np.tile(base.op1_off, rep), op1_len=np.tile(base.op1_len, rep),
        op2_off=np.tile(base.op2_off, rep), op2_len=np.tile(base.op2_len, rep))
    dsrc = mh.DeviceWrite2Source(src, 0)
    dsrc.sig = torch.from_numpy(base.sig).to(dsrc.grant_bytes.device).repeat(rep, 1)  # the 64 certificates' signatures
    need = rep * hw.size
    assert need > 1 << 32
    wire, off, ln, st = _outputs(M, need, fill=0)
    rc, got = ver7.encode_write2_device(dsrc, wire, off, ln, st, stream=_stream())
    torch.cuda.synchronize()
    assert got == need and bool((st == 0).all())
    h_off, h_ln = off.cpu().numpy().view(np.uint64), ln.cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(h_ln, np.tile(hln, rep))
    want = np.zeros(M, np.uint64)
    np.cumsum(h_ln[:-1].astype(np.uint64), out=want[1:])
    np.testing.assert_array_equal(h_off, want)
    assert int(h_off[-1]) > 1 << 32
    orig = torch.from_numpy(hw).to(wire.device)
    assert torch.equal(wire[:hw.size], orig)  # the 64 originals
    for m in range(M - 1024, M):  # the last 1,024 messages, past 4 GiB
        o, q = int(h_off[m]), int(hoff[m % 64])
        assert torch.equal(wire[o:o + int(h_ln[m])], orig[q:q + int(hln[m % 64])]), m


# 4. repeatability ----------------------------------------------------------------
def test_two_streams_give_equal_bytes(ver7, sources):
    import torch

    src = sources["align1024"]
    dsrc = mh.DeviceWrite2Source(src, 0)
    _, need, *_ = mh.encode_write2_into(src, C.IDS, None)
    outs = [_outputs(src.n_msgs, need + 64) for _ in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for (wire, off, ln, st), s in zip(outs, streams):
        ver7.encode_write2_device(dsrc, wire, off, ln, st, stream=s.cuda_stream)
    torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert bool((outs[0][0][need:] == 0xEE).all())


def test_per_kernel_profile(ver7, sources):
    src = sources["align1024"]
    dsrc = mh.DeviceWrite2Source(src, 0)
    _, need, *_ = mh.encode_write2_into(src, C.IDS, None)
    wire, off, ln, st = _outputs(src.n_msgs, need)
    ver7.encode_write2_device(dsrc, wire, off, ln, st, stream=_stream())
    with pytest.raises(mh.MochiError):  # that call was not profiled
        ver7.read_encode_profile()
    ver7.set_profiling(True)
    ver7.encode_write2_device(dsrc, wire, off, ln, st, stream=_stream())
    ver7.set_profiling(False)
    ms = ver7.read_encode_profile()
    assert list(ms) == list(mh.Verifier.ENCODE_KERNELS)
    assert all(0 <= v < 1000 for v in ms.values()) and ms["k_enc_copy"] > 0
