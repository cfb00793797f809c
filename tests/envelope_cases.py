"""Inputs the envelope tests share (tests/test_envelope_cpu.py, tests/test_envelope_gpu.py): the
join cases and the wrap's source batches, laid out as the library takes them, with what the
model (envelope_model.py) expects of them."""
from __future__ import annotations

import numpy as np

import envelope_model as E
import mochi_hip as mh


def join_cases():
    """name -> (request ids, frames)."""
    rep = lambda k, to, i=0: E.frame(k, E.body_of(k, i), ts=i + 1, msg_id=b"reply-%d" % i, reply_to=to)
    ids300 = [b"p" * 35 + bytes([65 + q % 50]) + (bytes([65 + q // 50]) if q >= 50 else b"") for q in range(300)]
    assert len(set(ids300)) == 300
    lens = [b"a", b"b" * 36, b"c" * 37, b"d" * 300]
    out = {
        "no_requests": ([], [rep(8, b"x"), rep(9, b"")]),
        "no_frames": ([b"id-0", b"id-1"], []),
        "one_request": ([b"id-0"], [rep(8, b"id-0", 0), rep(9, b"id-1", 1), rep(12, b"id-0", 2)]),
        "two_requests": ([b"id-0", b"id-1"], [rep(11, b"id-1", 0), rep(6, b"id-0", 1), rep(8, b"id-1", 2), rep(7, b"id-0", 3)]),
        "prefix_chains_300": (ids300, [rep((8, 9, 12, 11, 6)[i % 5], ids300[(i * 7) % 300], i) for i in range(450)]),
        "duplicate_table_id": ([b"same", b"other", b"same", b"same"], [rep(8, b"same", 0), rep(8, b"other", 1), rep(9, b"same", 2)]),
        "empty_ids": ([b"", b"id-1", b""], [rep(8, b"", 0), rep(8, b"id-1", 1), E.frame(8, b"b")]),
        "unmatched_and_prefix": ([b"request-id-long"], [rep(8, b"request-id", 0), rep(8, b"request-id-long", 1), rep(8, b"request-id-longer", 2),
                                                         rep(8, b"nobody", 3)]),
        "id_lengths": (lens, [rep(8, lens[i % 4], i) for i in range(9)]),
        "all_to_one": ([b"id-%d" % q for q in range(5)], [rep(8, b"id-3", i) for i in range(70)]),
        "reverse_order": ([b"id-%d" % q for q in range(70)], [rep(9, b"id-%d" % (69 - i), i) for i in range(70)]),
        "non_ok_dropped": ([b"id-0"], [rep(8, b"id-0", 0), E.ld(108, b"a") + E.ld(109, b"b") + E.ld(8, b"id-0"),
                                        E.ld(8, b"id-0") + b"\x3A\x05x", rep(11, b"id-0", 1)]),
    }
    return out


BODY_LENS = (0, 1, 15, 16, 17, 127, 128, 16384)


def encode_source(flags=0, n_extra=0):
    """Messages over every kind and the body lengths at which the length varint or the copy's
    chunking changes, ids and bodies at every misalignment; returns (source, per-message fields)."""
    rng = np.random.default_rng(7)
    msgs = []
    for i, bl in enumerate(BODY_LENS):
        msgs.append(dict(kind=1 + i % 12, body=bytes(rng.integers(0, 256, bl, dtype=np.uint8)), ts=(-1) ** i * (i << (7 * i)),
                         msg_id=E.UUID % i, reply_to=(E.UUID % (i + 1)) if i % 2 else b"", server_id=b"server-%d" % i))
    msgs.append(dict(kind=0, body=b"ignored", ts=0, msg_id=b"", reply_to=b"", server_id=b""))
    msgs.append(dict(kind=0, body=b"", ts=-(1 << 63), msg_id="é".encode(), reply_to=b"", server_id=b""))
    msgs.append(dict(kind=7, body=b"", ts=0, msg_id=b"", reply_to=b"", server_id=b""))  # DA 06 00
    msgs.append(dict(kind=12, body=b"x" * 300, ts=1, msg_id=b"m" * 130, reply_to=b"r" * 300, server_id=b"s"))
    for i in range(n_extra):
        k = int(rng.integers(0, 13))
        msgs.append(dict(kind=k, body=bytes(rng.integers(0, 256, int(rng.integers(0, 600)), dtype=np.uint8)), ts=int(rng.integers(-5, 5)),
                         msg_id=E.UUID % (i % 100), reply_to=b"" if i % 3 else E.UUID % ((i + 1) % 100), server_id=b"s%d" % (i % 7)))
    bodies, ids = bytearray(b"\x00"), bytearray(b"\x00\x00\x00")
    cols = {k: [] for k in ("body_off", "body_len", "msg_id_off", "msg_id_len", "reply_to_off", "reply_to_len", "server_id_off",
                            "server_id_len")}
    for i, m in enumerate(msgs):
        bodies += b"\x00" * (i % 3)
        cols["body_off"].append(len(bodies))
        cols["body_len"].append(len(m["body"]))
        bodies += m["body"]
        for nm in ("msg_id", "reply_to", "server_id"):
            cols[nm + "_off"].append(len(ids))
            cols[nm + "_len"].append(len(m[nm]))
            ids += m[nm] + b"\x00" * (i % 2)
    src = mh.EnvelopeSource(bodies=np.frombuffer(bytes(bodies), np.uint8), ids=np.frombuffer(bytes(ids), np.uint8),
                            kind=np.array([m["kind"] for m in msgs], np.uint8),
                            msg_timestamp=np.array([m["ts"] for m in msgs], np.int64), flags=flags, **cols)
    return src, msgs


def expected_wire(msgs, flags):
    frames = [E.frame(m["kind"], m["body"], m["ts"], m["server_id"], m["msg_id"], m["reply_to"]) for m in msgs]
    parts, off, pos = [], [], 0
    for f in frames:
        pre = E.varint(len(f)) if flags & mh.ENV_LENGTH_PREFIX else b""
        off.append(pos + len(pre))
        parts.append(pre + f)
        pos += len(pre) + len(f)
    return b"".join(parts), off, frames
