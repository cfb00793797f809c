"""The cluster harness with every message between a client and a server as protobuf bytes
that libmochi_hip produced and libmochi_hip consumes (test-side).

`WireCluster` subclasses cluster_harness.Cluster and overrides its seams.  The Python
`Server` / client model of the harness stays in place as the store and as the independent
reference: it runs on the same requests in the same order, and every stage of the wire chain
is held against it (a mismatch raises WireMismatch, naming stage, server, step and both
values).  Backends: "wire-host" (the host forms, CPU suite) and "wire-device" (the device
forms).  Per scheduler step each server handles all its deliveries of a kind as ONE batch, in
delivery order, Write1s before Write2s:

1. w1_server   Write1ToServer bodies (write1_request_model's encoder, client id "client-<n>")
               -> write1_request_decode -> the store's state per distinct key (key_op) as a
               Write1KeyState, as of the start of the step -> write1_state_join -> write1_issue
               (+ sign_grants; device: issue_device with signatures) -> write1_reply_encode.
               Shadow: Server.write1's kind, the grants it refers to and the grants it issues,
               as sets (the library lists a MultiGrant's grants in op order, the model in Java
               HashMap order).  The model's new grants take the library's signatures.
2. w1_client   the R reply bodies -> write1_reply_decode -> mochi_write1_classify on the
               decoded arrays.  Shadow: Cluster._classify on the model objects.
   w2_encode   on PROCEED, mochi_write2_encode from the decoded grants and signatures, the
               MultiGrants in java_hash_order of the server ids.  Shadow: byte-equal to the
               harness's Python encoding once each model MultiGrant lists its grants in wire
               (= op) order.
3. w2_server   the step's Write2ToServer bodies for a server as one WireBatch -> verdicts
               (device: verify_write2_device, re-checked by the oracle; host: the oracle's)
               -> write2_answer_plan -> result_reply_encode, on the device on one stream with
               no wait in between.  The per-op decisions applied into the model are the
               library's.  Shadow: the answer bytes equal result_encode_model.message of
               Server.write2_apply's results.
4. read_server Server.read decides; its results -> ResultAnswers -> result_reply_encode.
5. closing     answer bodies -> result_reply_decode -> mochi_tally_responses ->
               result_coalesce; the client's outcome is built from the coalesced slices.
               Shadow: Cluster._tally and the chosen servers' model results; certificate
               bytes equal the model certificate's encoding in wire order.

The wire backends draw nothing from Cluster.rng, so for a seed the schedule, and with it the
event log (plain_log), equals the "host" backend's.
"""
from __future__ import annotations

from typing import Dict, List

import numpy as np

import cluster_harness as H
import mochi_hip as mh
import result_encode_model as E
import result_reply_model as RRM
import workload as W
import write1_decode_model as DM
import write1_request_model as QM
import write2_answer_model as A

WRITE_STAGES = ("w1_server", "w1_client", "w2_encode", "w2_server", "closing")
READ_STAGES = ("read_server", "closing")
COUNTERS = ("w1_batches", "w1_multi", "w1_multi_shared_key", "w2_batches", "w2_multi", "refused_bodies",
            "refused_in_batch", "refused_stored", "retry_from_stored", "read_branch_answers")
STORED_MASK = 0x7FFFFFFF


class WireMismatch(AssertionError):
    pass


def grant_tuple(g) -> tuple:
    return (g.object_id, g.ts, g.txn_hash, g.status)


def _parsed(gb: bytes) -> tuple:
    g = DM.parse_grant(gb, 0, len(gb))
    return (g.object_id.decode(), g.ts, g.tx_hash.decode(), g.status)


def _csr(lens, dt=np.uint64):
    """Offsets of slices of the given lengths laid back to back, from `lens[0]`'s start 0."""
    return np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64))[:-1]]).astype(dt) if len(lens) else np.zeros(0, dt)


def _blob(parts: List[bytes], base: int = 0):
    """(bytes, off uint64, len uint32) of the parts back to back behind `base` bytes."""
    ln = np.array([len(x) for x in parts], np.uint32)
    return b"".join(parts), _csr(ln) + np.uint64(base), ln


def plain_log(c: H.Cluster) -> list:
    """The event log as plain values: (server, kind, client, ops, reply), no object identity."""
    cert = lambda x: None if x is None else tuple((sid, tuple(grant_tuple(g) for g in mg.grants)) for sid, mg in x.mgs)
    out = []
    for s, kind, p, got in c.log:
        if kind != "W1" and got is not None:
            got = [(r.status, r.result, r.existed, cert(r.cert)) for r in got]
        out.append((s, kind, p.client, tuple((o.action, o.key, o.value) for o in p.ops), got))
    return out


class WireCluster(H.Cluster):
    wire = True

    def __init__(self, backend: str = "wire-host", **kw):
        assert backend in ("wire-host", "wire-device")
        super().__init__(backend="device" if backend == "wire-device" else "host", **kw)
        self.form = backend
        self.dev = self.backend == "device"
        self.stats["wire"] = {k: 0 for k in WRITE_STAGES + READ_STAGES + COUNTERS}
        self.cert_bytes: Dict[int, bytes] = {}  # id(Cert) -> its WriteCertificate bytes on the wire
        self._certs: List[H.Cert] = []  # keeps those ids alive
        self.w1_bodies: List[tuple] = []  # (step, server, Pending, kind, reply body)
        self._w1_batch: Dict[int, list] = {}
        self._reads: Dict[int, list] = {}
        self._w2_answers: Dict[tuple, tuple] = {}
        self._w1_round = None
        self._closing = None
        self.stream = None
        if self.dev:
            import torch

            self.stream = torch.cuda.Stream(self.device)

    # --- helpers ------------------------------------------------------------------------
    def _check(self, stage: str, server, got, want, what: str):
        if got != want:
            raise WireMismatch(f"{stage} at server {server}, step {self.stats['steps']}: {what}: library {got!r} != "
                               f"model {want!r}")

    def _client_id(self, p: H.Pending) -> str:
        return f"client-{p.client}"

    def _on_stream(self):
        import torch

        return torch.cuda.stream(self.stream)

    def _sync(self):
        self.stream.synchronize()

    def cert_wire(self, cert: H.Cert, ops: List[H.Op]) -> bytes:
        """The model certificate's WriteCertificate bytes with every MultiGrant's grants in op order."""
        first: Dict[str, int] = {}
        for i, op in enumerate(ops):
            first.setdefault(op.key, i)
        out = b""
        for sid, mg in cert.mgs:
            gs = sorted(mg.grants, key=lambda g: first[g.object_id])
            body = W.encode_multigrant([(g.object_id, g.encode()) for g in gs], mg.server_id, mg.client_id, "",
                                       [(g.object_id, g.sig) for g in gs])
            out += W.encode_map_entry(1, sid.encode(), body)
        return out

    # --- 1. Write1 at a server ------------------------------------------------------------
    def _on_write1(self, srv, p, kind, mg, new):
        self._w1_batch.setdefault(srv.index, []).append((p, kind, mg, new))

    def _finish_write1(self, w1_new):
        batches, self._w1_batch = self._w1_batch, {}
        for s, reqs in batches.items():
            self._write1_at(self.servers[s], reqs)
        self.stats["signed"] += sum(len(g) for g in w1_new.values())

    def _write1_at(self, srv, reqs):
        st = self.stats["wire"]
        st["w1_server"] += 1
        st["w1_batches"] += 1
        if len(reqs) >= 2:
            st["w1_multi"] += 1
            keys = [{op.key for op in p.ops} for p, _, _, _ in reqs]
            if any(keys[i] & keys[j] for i in range(len(keys)) for j in range(i)):
                st["w1_multi_shared_key"] += 1
        Q = len(reqs)
        step_new = [g for _, _, _, new in reqs for g in new]
        assert all(op.action in (H.WRITE, H.DELETE) for p, _, _, _ in reqs for op in p.ops)
        # the client sends every Write1 op as a WRITE without value (MochiDBClient.java:256-261)
        bodies = [QM.write1(self._client_id(p).encode(),
                            QM.transaction([QM.operation(QM.WRITE, op.key.encode()) for op in p.ops]), p.seed,
                            p.thash.encode()) for p, _, _, _ in reqs]
        # the grants the server holds as of the start of the step
        stored = [g for sv in srv.store.values() for g in sv.given.values() if not any(g is n for n in step_new)]
        where = {id(g): i for i, g in enumerate(stored)}
        S = len(stored)
        body_blob, msg_off, msg_len = _blob(bodies)
        hash_blob, sh_off, sh_len = _blob([g.txn_hash.encode() for g in stored], len(body_blob))
        sid = srv.id.encode()
        sid_off = len(body_blob) + len(hash_blob)
        blob = np.frombuffer(body_blob + hash_blob + sid, np.uint8).copy()
        wreqs = mh.Write1Requests(wire=blob, msg_off=msg_off, msg_len=msg_len)
        stored_bytes, stored_off, stored_len = _blob([g.encode() for g in stored])
        stored_bytes = np.frombuffer(stored_bytes, np.uint8).copy()
        stored_sig = np.frombuffer(b"".join(g.sig for g in stored), np.uint8).reshape(S, mh.RSA_BYTES).copy() if S else \
            np.zeros((0, mh.RSA_BYTES), np.uint8)

        def key_state(t):
            """The host's one store lookup per distinct key of the decoded batch."""
            fl, ep, goff, gts, gst = [], [], [0], [], []
            for o in t["key_op"].tolist():
                ko, kl = int(t["op_key_off"][o]), int(t["op_key_len"][o])
                key = blob[ko:ko + kl].tobytes().decode()
                sv = srv.store.get(key)
                fl.append((mh.W1OP_LOCAL if srv.local(key) else 0) | (mh.W1OP_HAS_SVOC if sv is not None else 0))
                ep.append(sv.epoch if sv is not None else 0)
                for ts, g in (sv.given.items() if sv is not None else ()):
                    if id(g) in where:
                        gts.append(ts)
                        gst.append(where[id(g)])
                goff.append(len(gts))
            return mh.Write1KeyState(key_flags=np.array(fl, np.uint8), key_epoch=np.array(ep, np.int64),
                                     key_given_off=np.array(goff, np.uint32), given_ts=np.array(gts, np.int64),
                                     given_stored=np.array(gst, np.uint32))

        def reply_source(client_off, client_len):
            return mh.Write1ReplySource(ids=blob, server_id_off=sid_off, server_id_len=len(sid), req_client_off=client_off,
                                        req_client_len=client_len, stored_bytes=stored_bytes,
                                        stored_off=stored_off, stored_len=stored_len, stored_sig=stored_sig,
                                        certs=np.zeros(0, np.uint8), op_cert_off=None, op_cert_len=None)

        k = self.signer_of[srv.index]
        if not self.dev:
            dec = mh.write1_request_decode(wreqs)
            t = dec.trimmed()
            fl, ep, stt = mh.write1_state_join(t["req_op_off"], t["req_seed"], t["op_flags"], t["op_obj"], key_state(t))
            batch = mh.Write1Batch(strings=blob, req_op_off=t["req_op_off"], req_seed=t["req_seed"],
                                   req_hash_off=t["req_hash_off"], req_hash_len=t["req_hash_len"],
                                   op_key_off=t["op_key_off"], op_key_len=t["op_key_len"], op_flags=fl, op_obj=t["op_obj"],
                                   op_epoch=ep, op_stored=stt, stored_hash_off=sh_off, stored_hash_len=sh_len)
            issued = mh.write1_issue(batch)
            assert issued.rc == mh.OK
            issued.sig = mh.sign_grants(self.pems[k], issued.grant_bytes, issued.grant_off, issued.grant_len) \
                if issued.n_new else np.zeros((0, mh.RSA_BYTES), np.uint8)
            wire, off, ln, status = mh.write1_reply_encode(batch, issued, reply_source(t["req_client_off"],
                                                                                    t["req_client_len"]))
        else:
            t, issued, wire, off, ln, status = self._write1_device(self.signers[k], wreqs, Q, S, key_state, reply_source,
                                                                   sh_off, sh_len)
        self._check("w1_server", srv.index, t["req_status"].tolist(), [mh.W1Q_OK] * Q, "request decode status")
        self._check("w1_server", srv.index, status.tolist(), [mh.ENC_OK] * Q, "reply encode status")
        # the shadow: Server.write1 ran on the same requests in the same order
        req_op_off = t["req_op_off"].astype(np.int64)
        q_of_op = np.repeat(np.arange(Q), np.diff(req_op_off))
        new_lib = [_parsed(issued.grant(n)) for n in range(issued.n_new)]
        kinds = {mh.W1K_OK: "OK", mh.W1K_REFUSED: "REFUSED", mh.W1K_THROWS: "THROWS"}
        for q, (p, kind, mg, new) in enumerate(reqs):
            self._check("w1_server", srv.index, kinds[int(issued.req_kind[q])], kind, f"kind of request {q}")
            refs = issued.req_grant[int(issued.req_grant_off[q]):int(issued.req_grant_off[q + 1])].tolist()
            got = {grant_tuple(stored[r & STORED_MASK]) if r & mh.W1_STORED else new_lib[r] for r in refs}
            self._check("w1_server", srv.index, got, {grant_tuple(g) for g in mg.grants}, f"grants of request {q}")
            made = {new_lib[n] for n in range(issued.n_new) if q_of_op[int(issued.grant_op[n])] == q}
            self._check("w1_server", srv.index, made, {grant_tuple(g) for g in new}, f"new grants of request {q}")
            body = wire[int(off[q]):int(off[q]) + int(ln[q])].tobytes()
            if kind == "REFUSED":
                st["refused_bodies"] += 1
                st["refused_stored" if any(r & mh.W1_STORED for r in refs) else "refused_in_batch"] += 1
            p.wire[srv.index] = (mh.W1_OK if kind == "OK" else mh.W1_REFUSED, body)
            self.w1_bodies.append((self.stats["steps"], srv.index, p, kind, body))
        dec_, grant_ = issued.op_decision, issued.op_grant
        st["retry_from_stored"] += int(((dec_ == mh.W1D_RETRY) & ((grant_ & mh.W1_STORED) != 0) &
                                        (grant_ != mh.W1_NONE)).sum())
        # the new grants are stored with the library's bytes and signatures
        index = {(g[0], g[1]): n for n, g in enumerate(new_lib)}
        for g in step_new:
            n = index[(g.object_id, g.ts)]
            self._check("w1_server", srv.index, issued.grant(n), g.encode(), "bytes of a new grant")
            g.sig = issued.sig[n].tobytes()

    def _write1_device(self, signer, wreqs, Q, S, key_state, reply_source, sh_off, sh_len):
        import torch

        dev = torch.device("cuda", self.device)
        st = self.stream.cuda_stream
        blob = wreqs.wire
        with self._on_stream():
            dr = mh.DeviceWrite1Requests(wreqs, self.device)
            dec = mh.DeviceWrite1RequestsDecoded(Q, mh.write1_request_decode_bound(blob.size, Q), self.device)
            assert signer.request_decode_device(dr, dec, stream=st) == mh.OK
            O = dec.n_ops
            t = dec.to_host().trimmed()  # the host's part: one store lookup per distinct key
            dk = mh.DeviceWrite1KeyState(key_state(t), self.device)
            op_epoch = torch.zeros(max(O, 1), dtype=torch.int64, device=dev)
            op_stored = torch.zeros(max(O, 1), dtype=torch.int32, device=dev)
            signer.state_join_device(Q, O, dec.req_op_off, dec.req_seed, dec.op_flags, dec.op_obj, dk, dec.op_flags,
                                     op_epoch, op_stored, stream=st)
            db = mh.DeviceWrite1Batch.__new__(mh.DeviceWrite1Batch)
            db.n_reqs, db.n_ops, db.n_stored, db.strings_len = Q, O, S, int(blob.size)
            for k, v in dict(strings=dr.wire, req_op_off=dec.req_op_off, req_seed=dec.req_seed,
                             req_hash_off=dec.req_hash_off, req_hash_len=dec.req_hash_len, op_key_off=dec.op_key_off,
                             op_key_len=dec.op_key_len, op_flags=dec.op_flags, op_obj=dec.op_obj, op_epoch=op_epoch,
                             op_stored=op_stored, stored_hash_off=mh._to_dev(sh_off, self.device),
                             stored_hash_len=mh._to_dev(sh_len, self.device)).items():
                setattr(db, k, v)
            d_src = mh.DeviceWrite1ReplySource(reply_source(None, None), self.device)
            ds = mh.DeviceWrite1ReplySource.from_tensors(
                d_src.server_id_off, d_src.server_id_len, ids=dr.wire, req_client_off=dec.req_client_off,
                req_client_len=dec.req_client_len, stored_bytes=d_src.stored_bytes, stored_off=d_src.stored_off,
                stored_len=d_src.stored_len, stored_sig=d_src.stored_sig, certs=d_src.certs)
            ds.stored_bytes_len, ds.certs_len = d_src.stored_bytes_len, 0
            out = mh.DeviceWrite1Issued(Q, O, O * (2 * int(blob.size) + 64), sign=True, device=self.device)
            cap = mh.write1_reply_bound(db, ds, out.grant_cap, True)
            wire = torch.zeros(max(cap, 1), dtype=torch.uint8, device=dev)
            off = torch.zeros(Q, dtype=torch.int64, device=dev)
            ln = torch.zeros(Q, dtype=torch.int32, device=dev)
            status = torch.zeros(Q, dtype=torch.uint8, device=dev)
            assert signer.issue_device(db, out, stream=st) == mh.OK
            rc, total = signer.reply_encode_device(db, out, ds, wire, off, ln, status, stream=st)
            assert rc == mh.OK
            self._sync()
            issued = out.to_host()
            t["op_flags"] = dec.op_flags.cpu().numpy()[:O]  # joined in place
            return (t, issued, wire.cpu().numpy()[:total], off.cpu().numpy().view(np.uint64),
                    ln.cpu().numpy().view(np.uint32), status.cpu().numpy())

    # --- 2. the client's Write1 round -------------------------------------------------------
    def _classify(self, rounds):
        want = super()._classify(rounds)
        st = self.stats["wire"]
        st["w1_client"] += 1
        Q, R = len(rounds), self.R
        bodies, kinds, keys = [], [], []
        for p, _ in rounds:
            for s in self.send_order:
                kind, body = p.wire[s]
                kinds.append(kind)
                bodies.append(body)
            keys += [op.key.encode() for op in p.ops]
        wire, resp_off, resp_len = _blob(bodies)
        strings, key_off, key_len = _blob(keys)
        n_ops = [len(p.ops) for p, _ in rounds]
        replies = mh.Write1Replies(wire=np.frombuffer(wire, np.uint8).copy(), resp_off=resp_off, resp_len=resp_len,
                                   resp_kind=np.array(kinds, np.uint8), req_resp_off=(np.arange(Q + 1) * R).astype(np.uint32),
                                   strings=np.frombuffer(strings, np.uint8).copy(),
                                   req_op_off=np.concatenate([[0], np.cumsum(n_ops)]).astype(np.uint32),
                                   op_key_off=key_off, op_key_len=key_len)
        lib = mh.load_library()
        dev_keep = None
        if not self.dev:
            dec = mh.write1_reply_decode(replies, self.replica_ids)
            assert dec.rc == mh.OK
            t = dec.trimmed()
            pad = lambda a: np.ascontiguousarray(a if a.size else np.zeros(1, a.dtype))
            args = [pad(replies.req_resp_off), pad(t["resp_kind_out"]), pad(t["resp_server"]), pad(t["resp_grant_off"]),
                    pad(t["grant_key"]), pad(t["grant_ts"]), pad(t["grant_status"])]
            decision = np.zeros(Q, np.uint8)
            rc = lib.mochi_write1_classify(Q, *[mh._ptr(a) for a in args], mh._ptr(decision))
            assert rc == mh.OK, mh._err(lib)
        else:
            import torch

            with self._on_stream():
                dr = mh.DeviceWrite1Replies(replies, self.device)
                ddec = mh.DeviceWrite1Decoded(Q * R, max(R * sum(n_ops), 1), 1, device=self.device)
                assert self.verifier.write1_reply_decode_device(dr, ddec, stream=self.stream.cuda_stream) == mh.OK
                d_decision = torch.full((Q,), 0xEE, dtype=torch.uint8, device=dr.wire.device)
                rc = lib.mochi_write1_classify_device(Q, dr.req_resp_off.data_ptr(), ddec.resp_kind_out.data_ptr(),
                                                      ddec.resp_server.data_ptr(), ddec.resp_grant_off.data_ptr(),
                                                      ddec.grant_key.data_ptr(), ddec.grant_ts.data_ptr(),
                                                      ddec.grant_status.data_ptr(), d_decision.data_ptr(),
                                                      self.stream.cuda_stream)
                assert rc == mh.OK
                self._sync()
                decision = d_decision.cpu().numpy()
                t = ddec.to_host().trimmed()
                dev_keep = (dr, ddec)
        self._check("w1_client", "-", t["resp_status"].tolist(), [mh.W1R_OK] * (Q * R), "reply decode status")
        self._check("w1_client", "-", decision.tolist(), [int(d) for d in want], "Write1 round decisions")
        self._w1_round = dict(replies=replies, t=t, q_of={id(p): q for q, (p, _) in enumerate(rounds)}, dev=dev_keep)
        return decision

    def _write2_body(self, p):
        self.stats["wire"]["w2_encode"] += 1
        rd, R = self._w1_round, self.R
        t, q = rd["t"], rd["q_of"][id(p)]
        pos = {self.servers[s].id: i for i, s in enumerate(self.send_order)}
        resp = [q * R + pos[sid] for sid, _ in p.cert.mgs]  # the caller's order: java_hash_order of the server ids
        self._check("w2_encode", "-", [int(t["mg_signer"][r]) for r in resp],
                    [self.replica_ids.index(sid) for sid, _ in p.cert.mgs], "signers of the decoded MultiGrants")
        goff = t["resp_grant_off"].astype(np.int64)
        idx = np.concatenate([np.arange(goff[r], goff[r + 1]) for r in resp]).astype(np.int64)
        mg_grant_off = np.concatenate([[0], np.cumsum([goff[r + 1] - goff[r] for r in resp])]).astype(np.uint32)
        client = self._client_id(p).encode()
        parts = [op.key.encode() for op in p.ops] + [op.value.encode() for op in p.ops] + [client]
        strings, s_off, s_len = _blob(parts)
        k = len(p.ops)
        src = mh.Write2Source(
            grant_bytes=rd["replies"].wire, grant_off=t["grant_off"][idx], grant_len=t["grant_len"][idx], sig=t["sig"][idx],
            cert_mg_off=np.array([0, R], np.uint32), mg_grant_off=mg_grant_off,
            mg_signer=t["mg_signer"][np.array(resp)], strings=np.frombuffer(strings, np.uint8).copy(),
            cert_op_off=np.array([0, k], np.uint32), op_action=np.array([op.action for op in p.ops], np.uint8),
            op1_off=s_off[:k], op1_len=s_len[:k], op2_off=s_off[k:2 * k], op2_len=s_len[k:2 * k],
            client_off=s_off[2 * k:], client_len=s_len[2 * k:])
        if not self.dev:
            wire, off, ln, status = mh.encode_write2(src, self.replica_ids)
            status = status.tolist()
            msg = wire[int(off[0]):int(off[0]) + int(ln[0])].tobytes()
        else:
            import torch

            dr, ddec = rd["dev"]
            with self._on_stream():
                dev = dr.wire.device
                d_idx = torch.from_numpy(idx).to(dev)
                d_resp = torch.from_numpy(np.array(resp, np.int64)).to(dev)
                up = mh.DeviceWrite2Source(src, self.device)  # the small host-made arrays; the grants stay where they are
                dsrc = mh.DeviceWrite2Source.from_tensors(
                    1, R, int(idx.size), k, grant_bytes=dr.wire, grant_off=ddec.grant_off.index_select(0, d_idx),
                    grant_len=ddec.grant_len.index_select(0, d_idx), sig=ddec.sig.index_select(0, d_idx).contiguous(),
                    cert_mg_off=up.cert_mg_off, mg_grant_off=up.mg_grant_off, mg_signer=ddec.mg_signer.index_select(0, d_resp),
                    strings=up.strings, cert_op_off=up.cert_op_off, op_action=up.op_action, op1_off=up.op1_off,
                    op1_len=up.op1_len, op2_off=up.op2_off, op2_len=up.op2_len, client_off=up.client_off,
                    client_len=up.client_len)
                off = torch.zeros(1, dtype=torch.int64, device=dev)
                ln = torch.zeros(1, dtype=torch.int32, device=dev)
                d_status = torch.zeros(1, dtype=torch.uint8, device=dev)
                st = self.stream.cuda_stream
                rc, cap = self.verifier.encode_write2_device(dsrc, None, off, ln, d_status, stream=st, check=False)
                assert rc == mh.EINVAL and cap > 0
                wire = torch.zeros(cap, dtype=torch.uint8, device=dev)
                self.verifier.encode_write2_device(dsrc, wire, off, ln, d_status, stream=st)
                self._sync()
                status = d_status.cpu().numpy().tolist()
                o0, n0 = int(off[0]), int(ln[0])
                msg = wire.cpu().numpy()[o0:o0 + n0].tobytes()
        self._check("w2_encode", "-", status, [mh.ENC_OK], "Write2 encode status")
        wc = self.cert_wire(p.cert, p.ops)
        self._check("w2_encode", "-", msg, W._ld(1, wc) + W._ld(2, H.encode_txn(p.ops)), "Write2ToServer body")
        self.cert_bytes[id(p.cert)] = wc
        self._certs.append(p.cert)
        return msg

    # --- 3. Write2 at a server --------------------------------------------------------------
    def _stored(self, srv, op) -> "A.Stored":
        sv = srv.store.get(op.key)
        value = None if sv is None or sv.value is None else sv.value.encode()
        cert = None if sv is None or sv.current_c is None else self.cert_bytes[id(sv.current_c)]
        return A.Stored(value, cert)

    def _verify_write2(self, jobs):
        if not jobs:
            return []
        st = self.stats["wire"]
        out = [None] * len(jobs)
        by_server: Dict[int, list] = {}
        for i, j in enumerate(jobs):
            by_server.setdefault(j[0].index, []).append(i)
        for s, idx in by_server.items():
            group = [jobs[i] for i in idx]
            st["w2_server"] += 1
            st["w2_batches"] += 1
            st["w2_multi"] += len(group) >= 2
            wb = self._wire_batch(group)
            store = A.batch([A.Tx("", b"", (mh.OPD_APPLY,) * len(p.ops), tuple(self._stored(srv, op) for op in p.ops))
                             for srv, p, _, _ in group])[4]
            M, O = len(group), int(wb.op_flags_off[-1])
            if not self.dev:
                import oracle_ffi as ORA

                v, ms = ORA.verify_write2(self.moduli, self.ids_blob, self.ids_off, wb, self.R, True, 4)
                plan = mh.write2_answer_plan(wb, ms, v.cert_accept_bits, v.op_decision, store)
                ra = mh.planned_answers(wb.wire, store.store, np.zeros(0, np.uint8), plan, store.slot_off)
                wire, off, ln, status = mh.result_reply_encode(ra)
                plan_status = plan["plan_status"]
            else:
                v, plan_status, wire, off, ln, status = self._write2_device(wb, store, M, O)
            accept = mh.unpack_bits(v.cert_accept_bits, M)
            verdicts = []
            for m, (srv, p, f, _) in enumerate(group):
                o0 = int(wb.op_flags_off[m])
                per_op = [(int(v.op_decision[o0 + j]), int(v.op_g0[o0 + j]), int(v.op_ts[o0 + j])) for j in range(len(f))]
                verdicts.append((bool(accept[m]), int(v.cert_reason[m]), int(v.cert_fail_op[m]), per_op))
                body = wire[int(off[m]):int(off[m]) + int(ln[m])].tobytes()
                self._check("w2_server", s, int(status[m]), mh.ENC_OK, f"answer encode status of message {m}")
                self._w2_answers[(s, id(p))] = (int(plan_status[m]), body)
            if self.dev and self.check_oracle:
                self._oracle_check(group, verdicts)
            for i, vd in zip(idx, verdicts):
                out[i] = vd
        return out

    def _write2_device(self, wb, store, M, O):
        import torch

        st = self.stream.cuda_stream
        with self._on_stream():
            dev = torch.device("cuda", self.device)
            dwb = mh.DeviceWireBatch(wb, self.device)
            dv = mh.DeviceVerdicts(0, M, self.device, full=True, n_ops=O)
            dst = mh.DeviceWrite2AnswerStore(store, self.device)
            planned = mh.DeviceWrite2AnswerPlanned(M, store.n_slots, self.device)
            ids = torch.zeros(1, dtype=torch.uint8, device=dev)
            answers = planned.answers(dwb, dst, ids=ids)
            answers.ids_len = 0
            wire = torch.zeros(max(mh.result_reply_encode_bound(answers), 1), dtype=torch.uint8, device=dev)
            off = torch.zeros(M, dtype=torch.int64, device=dev)
            ln = torch.zeros(M, dtype=torch.int32, device=dev)
            status = torch.full((M,), 0xEE, dtype=torch.uint8, device=dev)
            total = torch.full((1,), -1, dtype=torch.int64, device=dev)
            # verify -> plan -> encode enqueued back to back: nothing waits for the one before
            self.verifier.verify_write2_device(dwb, dv, self.R, True, stream=st)
            mh.write2_answer_plan_device(dwb, dv, dst, planned, stream=st)
            rc, _ = self.verifier.result_reply_encode_device(answers, wire, off, ln, status, stream=st, wire_len_dev=total)
            assert rc == mh.OK
            self._sync()
            assert 0 <= int(total.item()) <= wire.numel()
            return (dv.to_host(), planned.to_host()["plan_status"], wire.cpu().numpy(), off.cpu().numpy().view(np.uint64),
                    ln.cpu().numpy().view(np.uint32), status.cpu().numpy())

    def _model_answer(self, kind: int, res) -> bytes:
        ops = tuple(E.OpR(1) if r.status == H.ST_WRONG_SHARD else
                    E.OpR(0, r.result.encode(), r.existed, None if r.cert is None else self.cert_bytes[id(r.cert)])
                    for r in res)
        return E.message(E.Ans(kind, ops))

    def _apply_w2(self, srv, p, verdict):
        super()._apply_w2(srv, p, verdict)
        res = self.log[-1][3]
        plan_status, body = self._w2_answers.pop((srv.index, id(p)))
        self.stats["wire"]["read_branch_answers"] += sum(1 for d, _, _ in verdict[3] if d == mh.OPD_READ) \
            if res is not None else 0
        if res is None:  # the reference threw: no answer is sent
            self._check("w2_server", srv.index, plan_status, mh.W2A_NO_REPLY, "plan status where the model sends no reply")
            return
        self._check("w2_server", srv.index, plan_status, mh.W2A_REPLY, "plan status where the model replies")
        self._check("w2_server", srv.index, body, self._model_answer(E.W2, res), "Write2AnsFromServer body")
        p.wire[srv.index] = body

    # --- 4. Read at a server ----------------------------------------------------------------
    def _on_read(self, srv, p, res):
        if res is not None:
            self._reads.setdefault(srv.index, []).append((p, res))

    def _finish_reads(self):
        reads, self._reads = self._reads, {}
        for s, group in reads.items():
            self.stats["wire"]["read_server"] += 1
            answers = [E.Ans(E.RD, tuple(
                E.OpR(1) if r.status == H.ST_WRONG_SHARD else
                E.OpR(0, r.result.encode(), r.existed, None if r.cert is None else self.cert_bytes[id(r.cert)], "s", "s")
                for r in res)) for _, res in group]
            ra = E.layout(answers, ids=False)
            if not self.dev:
                wire, off, ln, status = mh.result_reply_encode(ra)
            else:
                import torch

                with self._on_stream():
                    dev = torch.device("cuda", self.device)
                    da = mh.DeviceResultAnswers(ra, self.device)
                    P = len(group)
                    d_wire = torch.zeros(max(mh.result_reply_encode_bound(ra), 1), dtype=torch.uint8, device=dev)
                    d_off = torch.zeros(P, dtype=torch.int64, device=dev)
                    d_ln = torch.zeros(P, dtype=torch.int32, device=dev)
                    d_status = torch.full((P,), 0xEE, dtype=torch.uint8, device=dev)
                    rc, total = self.verifier.result_reply_encode_device(da, d_wire, d_off, d_ln, d_status,
                                                                         stream=self.stream.cuda_stream)
                    assert rc == mh.OK
                    self._sync()
                    wire, off, ln, status = (d_wire.cpu().numpy(), d_off.cpu().numpy().view(np.uint64),
                                             d_ln.cpu().numpy().view(np.uint32), d_status.cpu().numpy())
            for m, ((p, res), a) in enumerate(zip(group, answers)):
                body = wire[int(off[m]):int(off[m]) + int(ln[m])].tobytes()
                self._check("read_server", s, int(status[m]), mh.ENC_OK, f"answer encode status of read {m}")
                self._check("read_server", s, body, E.message(a), "ReadFromServer body")
                p.wire[s] = body

    # --- 5. the client's closing round ----------------------------------------------------------
    def _tally(self, rounds):
        want_acc, want_ch = super()._tally(rounds)
        self.stats["wire"]["closing"] += 1
        Q, R = len(rounds), self.R
        bodies = [p.wire[s] for p, _ in rounds for s in self.send_order]
        k = np.array([len(p.ops) for p, _ in rounds], np.int64)
        wire, resp_off, resp_len = _blob(bodies)
        r = mh.ResultReplies(wire=np.frombuffer(wire, np.uint8).copy(), resp_off=resp_off, resp_len=resp_len,
                             resp_kind=np.repeat([mh.RR_WRITE2_ANS if p.kind == "W2" else mh.RR_READ for p, _ in rounds],
                                                 R).astype(np.uint8),
                             req_resp_off=(np.arange(Q + 1) * R).astype(np.uint32), n_ops=k.astype(np.uint32),
                             slot_off=_csr(np.repeat(k, R)))
        out_off = _csr(k)
        n_out = int(k.sum())
        if not self.dev:
            dec = mh.result_reply_decode(r)
            chosen, reason, bits = RRM.tally_host(r, dec, R, out_off, n_out)
            co = mh.result_coalesce(r, dec, chosen, out_off, bits, out_off, n_out)
            resp_status = dec["resp_status"]
        else:
            import torch

            lib = mh.load_library()
            st = self.stream.cuda_stream
            with self._on_stream():
                dev = torch.device("cuda", self.device)
                dr = mh.DeviceResultReplies(r, self.device)
                ddec = mh.DeviceResultDecoded(r.n_resps, r.n_slots, self.device)
                dco = mh.DeviceResultCoalesced(n_out, self.device)
                d_off = mh._to_dev(out_off, self.device)
                d_chosen = torch.full((max(n_out, 1),), -1, dtype=torch.int32, device=dev)
                d_reason = torch.zeros(Q, dtype=torch.uint8, device=dev)
                d_bits = torch.zeros((Q + 31) // 32, dtype=torch.int32, device=dev)
                # decode -> tally -> coalesce enqueued back to back on one stream
                self.verifier.result_reply_decode_device(dr, ddec, stream=st)
                rc = lib.mochi_tally_responses_device(Q, dr.req_resp_off.data_ptr(), dr.n_ops.data_ptr(),
                                                      ddec.resp_n_ops.data_ptr(), dr.slot_off.data_ptr(),
                                                      ddec.op_status.data_ptr(), d_off.data_ptr(), R, d_chosen.data_ptr(),
                                                      d_reason.data_ptr(), d_bits.data_ptr(), st)
                assert rc == mh.OK
                mh.result_coalesce_device(dr, ddec, d_chosen, d_off, d_bits, d_off, dco, stream=st)
                self._sync()
                chosen, bits = d_chosen.cpu().numpy(), d_bits.cpu().numpy().view(np.uint32)
                co = dco.to_host()
                resp_status = ddec.resp_status.cpu().numpy()[:r.n_resps]
        self._check("closing", "-", resp_status.tolist(), [mh.RRS_OK] * r.n_resps, "answer decode status")
        acc = mh.unpack_bits(bits, Q)
        self._check("closing", "-", [bool(a) for a in acc], [bool(a) for a in want_acc], "acceptance")
        ch = [chosen[int(out_off[q]):int(out_off[q]) + int(k[q])] for q in range(Q)]
        for q in range(Q):
            if acc[q]:
                self._check("closing", "-", ch[q].tolist(), [int(x) for x in want_ch[q]], f"chosen servers of request {q}")
        self._closing = dict(co=co, wire=wire, out_off=out_off)
        return acc, ch

    def _merged_result(self, p, resps, ch, n):
        model = super()._merged_result(p, resps, ch, n)
        c = self._closing
        co, wire, base = c["co"], c["wire"], int(c["out_off"][n])
        sl = lambda o, l: wire[int(o):int(o) + int(l)]
        out = []
        for i, m in enumerate(model):
            d = base + i
            has_cert = bool(int(co["flags"][d]) & mh.RRO_HAS_CERT)
            got = (int(co["status"][d]), sl(co["result_off"][d], co["result_len"][d]).decode(), bool(co["existed"][d]),
                   sl(co["cert_off"][d], co["cert_len"][d]) if has_cert else None)
            want = (m.status, m.result, m.existed, None if m.cert is None else self.cert_bytes[id(m.cert)])
            self._check("closing", "-", got, want, f"coalesced result of op {i}")
            out.append(H.OpResult(got[0], got[1], got[2], m.cert, got[3]))
        return out
