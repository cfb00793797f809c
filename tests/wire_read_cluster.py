"""wire_cluster.WireCluster with the server's read stage on the library's read path: every
read delivered to a server -- those the model answers and those where it returns None --
is encoded as a ReadToServer body (read_request_model's encoder), decoded by the library
(host or device form by backend), looked up once per distinct key in srv.store, planned
(mochi_read_answer_plan[_device]) and encoded (mochi_result_reply_encode[_device], ids =
wire, the nonce the decoder's slice).  plan_status is NO_REPLY exactly where the model gave
None, and the body equals result_encode_model.message of the model's results.

One known difference: cluster_harness.Server.read answers a present key that has no
certificate (a container made by a Write1 grant, no Write2 yet) without a certificate
field; the reference throws there (InMemoryDataStore.java:100).  Such reads are counted
(read_no_cert), the plan must say NO_REPLY for them, and the parent's bytes are passed on
so that the event log stays the model's.
"""
from __future__ import annotations

import numpy as np

import cluster_harness as H
import mochi_hip as mh
import read_request_model as RQ
import result_encode_model as E
import wire_cluster as WC


class WireReadCluster(WC.WireCluster):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.read_no_cert = 0
        self.read_stats = dict(requests=0, no_reply=0, keys=0, ops=0)

    def _on_read(self, srv, p, res):
        self._reads.setdefault(srv.index, []).append((p, res))

    def _model_ops(self, res):
        return tuple(E.OpR(1) if r.status == H.ST_WRONG_SHARD else
                     E.OpR(0, r.result.encode(), r.existed,
                           None if r.cert is None else self.cert_bytes[id(r.cert)], "s", "s") for r in res)

    def _finish_reads(self):
        reads, self._reads = self._reads, {}
        for s, group in reads.items():
            srv = self.servers[s]
            self.stats["wire"]["read_server"] += 1
            nonces = [b"nonce-%d-%d-%d" % (p.client, self.stats["steps"], m) for m, (p, _) in enumerate(group)]
            bodies = [RQ.read(self._client_id(p).encode(),
                              RQ.transaction([RQ.operation(op.action, op.key.encode(), op.value.encode()) for op in p.ops]), n)
                      for (p, _), n in zip(group, nonces)]
            reqs = RQ.batch(bodies, lead=s % 3)

            def lookup(key: bytes) -> RQ.KeyRec:
                k = key.decode()
                sv = srv.store.get(k)
                if sv is None:
                    return RQ.KeyRec(srv.local(k))
                return RQ.KeyRec(srv.local(k), True, sv.available, None if sv.value is None else sv.value.encode(),
                                 None if sv.current_c is None else self.cert_bytes[id(sv.current_c)])

            plan_status, out = self._read_round_device(reqs, lookup) if self.dev else self._read_round_host(reqs, lookup)
            self.read_stats["requests"] += len(group)
            for m, ((p, res), nonce) in enumerate(zip(group, nonces)):
                st = int(plan_status[m])
                no_cert = res is not None and any(r.status == H.ST_OK and r.cert is None for r in res)
                if no_cert:
                    self.read_no_cert += 1
                if res is None or no_cert:
                    self.read_stats["no_reply"] += 1
                    self._check("read_server", s, st, mh.RDA_NO_REPLY, "plan status where the reference sends no reply")
                    self._check("read_server", s, out[m], b"", "body of a read without a reply")
                    if no_cert:  # the model answers: its bytes go on
                        p.wire[s] = E.message(E.Ans(E.RD, self._model_ops(res)))
                    continue
                self._check("read_server", s, st, mh.RDA_REPLY, "plan status where the model replies")
                self._check("read_server", s, out[m], E.message(E.Ans(E.RD, self._model_ops(res), nonce=nonce)),
                            "ReadFromServer body")
                p.wire[s] = out[m]

    def _read_round_host(self, reqs, lookup):
        dec = mh.read_request_decode(reqs)
        t = dec.trimmed()
        self._check("read_server", "-", t["req_status"].tolist(), [mh.RDQ_OK] * reqs.n_reqs, "request decode status")
        ks = RQ.key_state(reqs, t, lookup)
        self.read_stats["keys"] += dec.n_keys
        self.read_stats["ops"] += dec.n_ops
        planned = mh.read_answer_plan(dec, ks)
        wire, off, ln, status = mh.result_reply_encode(
            mh.read_planned_answers(reqs.wire, ks.store, planned, t["req_nonce_off"], t["req_nonce_len"]))
        self._check("read_server", "-", status.tolist(), [mh.ENC_OK] * reqs.n_reqs, "answer encode status")
        return planned["plan_status"], [wire[int(o):int(o) + int(n)].tobytes() for o, n in zip(off, ln)]

    def _read_round_device(self, reqs, lookup):
        import torch

        Q = reqs.n_reqs
        st = self.stream.cuda_stream
        with self._on_stream():
            dev = torch.device("cuda", self.device)
            dr = mh.DeviceReadRequests(reqs, self.device)
            dec = mh.DeviceReadRequestsDecoded(Q, mh.read_request_decode_bound(reqs.wire.size, Q), self.device)
            rc = self.verifier.read_request_decode_device(dr, dec, stream=st)
            assert rc == mh.OK
            self._sync()
            t = dec.to_host().trimmed()  # the host's lookup needs key_op and the key slices
            self._check("read_server", "-", t["req_status"].tolist(), [mh.RDQ_OK] * Q, "request decode status")
            ks = RQ.key_state(reqs, t, lookup)
            self.read_stats["keys"] += len(t["key_op"])
            self.read_stats["ops"] += dec.n_ops
            dks = mh.DeviceReadKeyState(ks, self.device)
            planned = mh.DeviceReadAnswerPlanned(Q, dec.n_ops, self.device)
            # plan -> encode back to back on the stream
            mh.read_answer_plan_device(dec, dks, planned, stream=st)
            da = planned.answers(dr, dec, dks)
            d_wire = torch.zeros(max(mh.result_reply_encode_bound(da), 1), dtype=torch.uint8, device=dev)
            d_off = torch.zeros(Q, dtype=torch.int64, device=dev)
            d_ln = torch.zeros(Q, dtype=torch.int32, device=dev)
            d_status = torch.full((Q,), 0xEE, dtype=torch.uint8, device=dev)
            rc, total = self.verifier.result_reply_encode_device(da, d_wire, d_off, d_ln, d_status, stream=st)
            assert rc == mh.OK
            self._sync()
            wire, off, ln = d_wire.cpu().numpy(), d_off.cpu().numpy().view(np.uint64), d_ln.cpu().numpy().view(np.uint32)
            self._check("read_server", "-", d_status.cpu().numpy().tolist(), [mh.ENC_OK] * Q, "answer encode status")
            return planned.to_host()["plan_status"], [wire[int(o):int(o) + int(n)].tobytes() for o, n in zip(off, ln)]
