"""A plain-Python model of the client's response aggregation, and the case sets
that pin mochi_tally_responses / mochi_write1_classify (host and device) to it.

The model restates MochiDBClient.java in the Java's own terms -- a count array
and a result list for the Read / Write2 tally (:148-175, :355-382); for the
Write1 round (:236-332) a list of kept messages, a HashMap<serverId, MultiGrant>
whose values are maps key -> grant, and isUniformTimeStampInMultiGrants (:195-219)
walking `for multiGrant in values(): for op in transactionOps: get(op.key)`.
It uses no numpy and shares no structure with the oracle (oracle/mochi_oracle.c),
the host C++ (capi.cpp) or the kernels (client.hip), which all work per grant
with a first-seen timestamp per key slot.

Formats are those of mochi_hip.tally_responses and mochi_hip.pack_write1:
  tally     responses = [[status, ...] per response], k = the transaction's op count
  classify  responses = [(kind, server_id, [(key_slot, ts, status), ...]) per response]
A key slot is the index of the grant's objectId among the transaction's op keys,
0xFF for an objectId no op names.

Contract of classify: the key slots inside one response are distinct (a
MultiGrant's grants are a map), 0xFF may repeat.  classify_dup_in_response()
steps outside it on purpose; those cases carry no model expectation.
"""
from __future__ import annotations

import functools
import itertools
from collections import namedtuple

WRONG_SHARD = 1
NO_OP_KEY = 0xFF

# payload kinds (MOCHI_W1_*) and round outcomes (enum mochi_write1_decision)
OK, REFUSED, REQUEST_FAILED, OTHER = 0, 1, 2, 3
PROCEED, RETRY, THROW_REFUSED, THROW_FAILED, THROW_UNSUPPORTED = 0, 1, 2, 3, 4

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def majority(R: int) -> int:
    """ClusterConfiguration.getServerMajority (:264-267)."""
    return 2 * (R // 3) + 1


def tally(responses, k: int, R: int):
    """-> (reason, chosen): reason 0 accept, 1 op-count mismatch, 2 below majority;
    chosen[j] = index of the response coalescedResult[j] came from, or -1 (null)."""
    count = [0] * k  # consistentTRCount
    chosen = [-1] * k  # coalescedResult
    for i, operations in enumerate(responses):
        if len(operations) != k:
            return 1, chosen  # throw new Inconsistent*Exception()  :159-161 / :366-368
        for index in range(k):
            if operations[index] != WRONG_SHARD:
                count[index] += 1
                chosen[index] = i
    for index in range(k):
        if count[index] < majority(R):
            return 2, chosen  # :171-175 / :378-381
    return 0, chosen


def classify(responses) -> int:
    # the transaction's op keys; an op key that no response grants is skipped by
    # `grantForCurrentKey == null` (:204-206), so the granted ones are all that matter
    ops = sorted({slot for _, _, grants in responses for slot, _, _ in grants if slot != NO_OP_KEY})
    all_write_ok = True
    kept = []  # messages1FromServers
    for kind, server_id, grants in responses:  # :273-289
        if kind == OK:
            kept.append((kind, server_id, grants))
        elif kind == REFUSED:
            all_write_ok = False
            kept.append((kind, server_id, grants))
        elif kind == REQUEST_FAILED:
            return THROW_FAILED
        else:
            all_write_ok = False
    ok = {}  # write1mutiGrants
    for kind, server_id, grants in kept:  # :294-308
        multigrant = {}
        for n, (slot, ts, status) in enumerate(grants):
            key = slot if slot != NO_OP_KEY else ("not an op key", n)
            assert key not in multigrant, "a MultiGrant's grants are a map: key slots are distinct"
            multigrant[key] = (ts, status)
        # removeWrongShardGrantFromMultiGrant: grants.remove() on protobuf's read-only map  :221-228
        if any(status == WRONG_SHARD for _, status in multigrant.values()):
            return THROW_UNSUPPORTED
        if kind == OK:
            ok[server_id] = {key: ts for key, (ts, _) in multigrant.items()}  # HashMap.put: the last one wins
    coalesced = {}  # coalescedTxnGrantMap  :195-219
    for multigrant in ok.values():
        for op in ops:
            if op not in multigrant:
                continue
            if op in coalesced:
                if coalesced[op] != multigrant[op]:
                    return RETRY
            else:
                coalesced[op] = multigrant[op]
    return PROCEED if all_write_ok else THROW_REFUSED


# ---------------------------------------------------------------------------
# case sets
# ---------------------------------------------------------------------------
TallyCase = namedtuple("TallyCase", "name R responses k")
# expect: the decision the set's description names (None: whatever the model says;
# for classify_dup_in_response, whatever the oracle says)
ClassifyCase = namedtuple("ClassifyCase", "name responses expect")

EXHAUSTIVE_R = (0, 1, 2, 3, 4, 6)
MAJORITY_LINE_R = (1, 3, 4, 6, 7, 9, 10)
TALLY_GEOMETRY_N = (1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 255, 256, 257, 511, 513)
CLASSIFY_GEOMETRY_N = (1, 255, 256, 257, 513)
SERVER_IDS = (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF)
STATUS_VALUES = (0, 1, 2, 3, 0x7F, 0x80, 0xFF)
TS_PAIRS = ((1, 1 + (1 << 32)), (-1, I64_MAX), (I64_MIN, I64_MIN), (0, I64_MIN), (1 << 32, 1 << 33))
MAX_OPS = 64  # MOCHI_MAX_OPS_PER_CERT


def tally_exhaustive():
    """k in {0,1,2}, 0-4 responses, each any status vector over {0,1,2}^k or a vector of
    k+1 or (k > 0) k-1 zeros: 16,917 requests, to be run at every R of EXHAUSTIVE_R."""
    cases = []
    for k in (0, 1, 2):
        options = [list(v) for v in itertools.product((0, 1, 2), repeat=k)] + [[0] * (k + 1)]
        if k > 0:
            options.append([0] * (k - 1))
        for n in range(5):
            for resps in itertools.product(options, repeat=n):
                cases.append(TallyCase(f"exhaustive k={k} {list(resps)}", None, list(resps), k))
    return cases


def _wrong_shard_places(n: int, ws: int):
    """Where the ws WRONG_SHARD results sit among n responses: first, last, alternating."""
    alternating = (list(range(0, n, 2)) + list(range(1, n, 2)))[:ws]
    return (("first", set(range(ws))), ("last", set(range(n - ws, n))), ("alternating", set(alternating)))


def tally_majority_line():
    """k = 2; one op has exactly M-1 or M non-WRONG_SHARD results, the other is all OK."""
    cases = []
    for R in MAJORITY_LINE_R:
        M = majority(R)
        for n in sorted({M - 1, M, M + 1, R}):
            for c in (M - 1, M):
                if c > n:
                    continue
                for where, ws in _wrong_shard_places(n, n - c):
                    for short in (0, 1):
                        resps = [[0, 0] for _ in range(n)]
                        for q in ws:
                            resps[q][short] = WRONG_SHARD
                        cases.append(TallyCase(f"majority R={R} n={n} c={c} ws {where} short op {short}", R, resps, 2))
    return cases


def tally_status_values():
    """Every status byte but 1 is a result; only 1 is WRONG_SHARD."""
    cases = []
    others = [v for v in STATUS_VALUES if v != WRONG_SHARD]
    for v in others:
        cases.append(TallyCase(f"status {v:#x} x3", 4, [[v], [v], [v]], 1))  # accept
        cases.append(TallyCase(f"status {v:#x} with one WRONG_SHARD", 4, [[v], [WRONG_SHARD], [v]], 1))  # 2 < 3
        cases.append(TallyCase(f"status {v:#x} last", 4, [[0], [0], [WRONG_SHARD], [v]], 1))  # accept, chosen 3
    n = len(STATUS_VALUES)
    rotations = [[STATUS_VALUES[(q + j) % n] for j in range(n)] for q in range(n)]  # one WRONG_SHARD per op
    cases.append(TallyCase("status rotations R=7", 7, rotations, n))  # 6 >= 5
    cases.append(TallyCase("status rotations R=10", 10, rotations, n))  # 6 < 7
    cases.append(TallyCase("status rotations reversed R=7", 7, rotations[::-1], n))
    return cases


def tally_wide():
    """k = 64 ops, 10 responses at R = 10 (M = 7): op i lacks response i % 10; in request j
    op j lacks four responses (6 < M).  One request is left whole.  Then op-count mismatches
    at response 0, in the middle and at the last response."""
    k, n, R = MAX_OPS, 10, 10

    def whole():
        return [[WRONG_SHARD if q == i % n else 0 for i in range(k)] for q in range(n)]

    cases = [TallyCase("wide whole", R, whole(), k)]
    for j in range(k):
        resps = whole()
        for d in range(4):
            resps[(j + d) % n][j] = WRONG_SHARD
        cases.append(TallyCase(f"wide op {j} below majority", R, resps, k))
    for at in (0, 5, n - 1):
        for length in (k - 1, k + 1):
            resps = whole()
            resps[at] = [0] * length
            cases.append(TallyCase(f"wide mismatch ({length} results) at response {at}", R, resps, k))
    return cases


def tally_geometry_accepts(i: int) -> bool:
    """Lanes 0, 31, 32 and 63 of every wave accept; between them the even lanes of the low
    half-word and the odd lanes of the high one, so that the two words of a ballot differ."""
    lane = i % 64
    return lane in (0, 31, 32, 63) or (lane + lane // 32) % 2 == 0


def tally_geometry(n: int):
    """n requests at R = 4 (M = 3) with the acceptance pattern of tally_geometry_accepts; the
    rejections alternate between the two reasons; k cycles through 1..3."""
    cases = []
    for i in range(n):
        k = 1 + i % 3
        if tally_geometry_accepts(i):
            resps = [[0] * k for _ in range(3 + i % 2)]
            if i % 2:
                resps[i % 4][i % k] = WRONG_SHARD  # 3 of 4 left
        elif (i // 2) % 2:
            resps = [[0] * k, [0] * k, [0] * (k + 1), [0] * k]  # reason 1
        else:
            resps = [[0] * k, [0] * k, [0] * k]
            resps[i % 3][i % k] = WRONG_SHARD  # reason 2
        cases.append(TallyCase(f"geometry n={n} i={i}", 4, resps, k))
    return cases


def _ok(server_id, grants):
    return (OK, server_id, grants)


def classify_exhaustive():
    """0-3 responses, each kind x server id {0,1} x grants {none, (0,5,OK), (0,6,OK),
    (0,5,WRONG_SHARD)}: 33,825 requests."""
    grant_sets = ([], [(0, 5, 0)], [(0, 6, 0)], [(0, 5, WRONG_SHARD)])
    options = [(kind, sid, g) for kind in (OK, REFUSED, REQUEST_FAILED, OTHER) for sid in (0, 1) for g in grant_sets]
    cases = []
    for n in range(4):
        for resps in itertools.product(options, repeat=n):
            cases.append(ClassifyCase(f"exhaustive {list(resps)}", list(resps), None))
    return cases


def classify_timestamps():
    """Two OK servers grant one key with 64-bit timestamps that agree in their low words, sit
    at the ends of the range, or are equal there."""
    cases = []
    for a, b in TS_PAIRS:
        want = PROCEED if a == b else RETRY
        cases.append(ClassifyCase(f"ts ({a}, {b})", [_ok(0, [(0, a, 0)]), _ok(1, [(0, b, 0)])], want))
        cases.append(ClassifyCase(f"ts ({a}, {b}) on slot 1, slot 0 uniform",
                                  [_ok(0, [(0, 7, 0), (1, a, 0)]), _ok(1, [(0, 7, 0), (1, b, 0)])], want))
    return cases


def classify_keys():
    """Every key slot 0..0xFE, in transactions of up to 8 ops; the skip of exactly 0xFF."""
    cases = []
    for lo in range(0, NO_OP_KEY, 8):
        slots = list(range(lo, min(lo + 8, NO_OP_KEY)))
        uniform = [(s, 1000 + s, 0) for s in slots]
        cases.append(ClassifyCase(f"keys {lo}..{slots[-1]} uniform", [_ok(0, uniform), _ok(1, uniform[::-1])], PROCEED))
        for s in slots:
            off = [(t, ts + (t == s), st) for t, ts, st in uniform]
            cases.append(ClassifyCase(f"keys {lo}..{slots[-1]}, slot {s} differs", [_ok(0, uniform), _ok(1, off)], RETRY))
    cases.append(ClassifyCase("slot 0xFE differs", [_ok(0, [(0xFE, 5, 0)]), _ok(1, [(0xFE, 6, 0)])], RETRY))
    cases.append(ClassifyCase("slot 0xFF differs", [_ok(0, [(NO_OP_KEY, 5, 0)]), _ok(1, [(NO_OP_KEY, 6, 0)])], PROCEED))
    cases.append(ClassifyCase("slot 0xFF differs beside a uniform key",
                              [_ok(0, [(0, 5, 0), (NO_OP_KEY, 5, 0)]), _ok(1, [(NO_OP_KEY, 6, 0), (0, 5, 0)])], PROCEED))
    cases.append(ClassifyCase("a response of 0xFF grants only",
                              [_ok(0, [(NO_OP_KEY, 1, 0), (NO_OP_KEY, 2, 0), (NO_OP_KEY, 3, 0)]), _ok(1, [(0, 5, 0)]),
                               _ok(2, [(0, 5, 0)])], PROCEED))
    cases.append(ClassifyCase("a response of 0xFF grants only, the others differ",
                              [_ok(0, [(NO_OP_KEY, 5, 0), (NO_OP_KEY, 6, 0)]), _ok(1, [(0, 5, 0)]), _ok(2, [(0, 6, 0)])],
                              RETRY))
    cases.append(ClassifyCase("each key granted by one server only",
                              [_ok(0, [(0, 5, 0)]), _ok(1, [(1, 6, 0)]), _ok(2, [(2, 7, 0)])], PROCEED))
    cases.append(ClassifyCase("one key granted by one server only, another by two that differ",
                              [_ok(0, [(0, 5, 0), (1, 8, 0)]), _ok(1, [(1, 9, 0)])], RETRY))
    return cases


def classify_servers():
    """Server ids with high bits set; HashMap.put per id: the last OK response of an id
    stands, whatever came before it, and only an OK response replaces one."""
    cases = []
    same = [(0, 5, 0)]
    cases.append(ClassifyCase("five ids uniform", [_ok(s, same) for s in SERVER_IDS], PROCEED))
    for odd in SERVER_IDS:
        resps = [_ok(s, [(0, 6 if s == odd else 5, 0)]) for s in SERVER_IDS]
        cases.append(ClassifyCase(f"five ids, {odd:#x} differs", resps, RETRY))
    for a, b in ((0x7FFFFFFF, 0xFFFFFFFF), (0, 0x80000000)):
        cases.append(ClassifyCase(f"ids {a:#x} and {b:#x} are two servers", [_ok(a, [(0, 5, 0)]), _ok(b, [(0, 6, 0)])],
                                  RETRY))
        cases.append(ClassifyCase(f"ids {a:#x} and {b:#x} are two servers, a third sides with the first",
                                  [_ok(a, [(0, 5, 0)]), _ok(b, [(0, 6, 0)]), _ok(1, [(0, 5, 0)])], RETRY))
    for s in SERVER_IDS:
        other = 0 if s else 1
        for chain in (3, 4):
            rising = [_ok(s, [(0, 5 + i, 0)]) for i in range(chain)]
            last = 5 + chain - 1
            cases.append(ClassifyCase(f"{chain} OK responses from {s:#x}, the last agrees",
                                      rising + [_ok(other, [(0, last, 0)])], PROCEED))
            cases.append(ClassifyCase(f"{chain} OK responses from {s:#x}, only the first agrees",
                                      rising + [_ok(other, [(0, 5, 0)])], RETRY))
            cases.append(ClassifyCase(f"{chain} OK responses from {s:#x} around another server's",
                                      rising[:1] + [_ok(other, [(0, last, 0)])] + rising[1:], PROCEED))
    for kind, name, want in ((REFUSED, "REFUSED", RETRY), (OTHER, "OTHER", RETRY),
                             (REQUEST_FAILED, "REQUEST_FAILED", THROW_FAILED)):
        cases.append(ClassifyCase(f"a later {name} response with the same id does not supersede",
                                  [_ok(0, [(0, 5, 0)]), _ok(1, [(0, 6, 0)]), (kind, 0, [(0, 6, 0)])], want))
        cases.append(ClassifyCase(f"a later {name} response with the same id and no grants does not supersede",
                                  [_ok(0x80000000, [(0, 5, 0)]), _ok(1, [(0, 6, 0)]), (kind, 0x80000000, [])], want))
    cases.append(ClassifyCase("an earlier REFUSED response with the same id is not what stands",
                              [(REFUSED, 0, [(0, 6, 0)]), _ok(0, [(0, 5, 0)]), _ok(1, [(0, 5, 0)])], THROW_REFUSED))
    cases.append(ClassifyCase("a superseded response's non-uniform grant is ignored",
                              [_ok(0, [(0, 5, 0)]), _ok(1, [(0, 6, 0)]), _ok(0, [(0, 6, 0)])], PROCEED))
    cases.append(ClassifyCase("a superseding response carries no grants",
                              [_ok(0, [(0, 5, 0)]), _ok(1, [(0, 6, 0)]), _ok(0, [])], PROCEED))
    cases.append(ClassifyCase("a superseding response grants another key",
                              [_ok(0, [(0, 5, 0)]), _ok(1, [(0, 6, 0), (1, 7, 0)]), _ok(0, [(1, 7, 0)])], PROCEED))
    cases.append(ClassifyCase("a superseding response brings the disagreement",
                              [_ok(0, [(0, 5, 0)]), _ok(1, [(0, 5, 0)]), _ok(0, [(0, 6, 0)])], RETRY))
    return cases


def classify_kinds():
    """Which payload kinds have their grants looked at, and in what order the outcomes win."""
    cases = []
    ws = [(0, 5, WRONG_SHARD)]
    cases.append(ClassifyCase("WRONG_SHARD grant in an OTHER response is not looked at",
                              [_ok(0, [(0, 5, 0)]), (OTHER, 1, ws)], THROW_REFUSED))
    cases.append(ClassifyCase("WRONG_SHARD grant in a REQUEST_FAILED response is not looked at",
                              [_ok(0, [(0, 5, 0)]), (REQUEST_FAILED, 1, ws)], THROW_FAILED))
    cases.append(ClassifyCase("WRONG_SHARD grant in a REFUSED response is looked at",
                              [_ok(0, [(0, 5, 0)]), (REFUSED, 1, ws)], THROW_UNSUPPORTED))
    cases.append(ClassifyCase("WRONG_SHARD grant in an OK response", [_ok(0, [(0, 5, 0), (1, 5, WRONG_SHARD)])],
                              THROW_UNSUPPORTED))
    cases.append(ClassifyCase("WRONG_SHARD grant for no op key is looked at", [_ok(0, [(NO_OP_KEY, 5, WRONG_SHARD)])],
                              THROW_UNSUPPORTED))
    cases.append(ClassifyCase("WRONG_SHARD grant in a superseded response is looked at",
                              [_ok(0, ws), _ok(0, [(0, 5, 0)])], THROW_UNSUPPORTED))
    cases.append(ClassifyCase("WRONG_SHARD wins over differing timestamps",
                              [_ok(0, [(0, 5, 0)]), _ok(1, [(0, 6, 0)]), _ok(2, ws)], THROW_UNSUPPORTED))
    cases.append(ClassifyCase("grant statuses other than 1 are no WRONG_SHARD",
                              [_ok(0, [(0, 5, 2), (1, 5, 0xFF)]), _ok(1, [(0, 5, 3), (1, 5, 0x80)])], PROCEED))
    cases.append(ClassifyCase("a REFUSED response's differing timestamp does not cause RETRY",
                              [_ok(0, [(0, 5, 0)]), (REFUSED, 1, [(0, 9, 0)])], THROW_REFUSED))
    cases.append(ClassifyCase("two REFUSED responses that differ do not cause RETRY",
                              [(REFUSED, 0, [(0, 5, 0)]), (REFUSED, 1, [(0, 9, 0)])], THROW_REFUSED))
    cases.append(ClassifyCase("differing OK timestamps win over a REFUSED response",
                              [_ok(0, [(0, 5, 0)]), (REFUSED, 2, []), _ok(1, [(0, 6, 0)])], RETRY))
    cases.append(ClassifyCase("differing OK timestamps win over an OTHER response",
                              [(OTHER, 2, []), _ok(0, [(0, 5, 0)]), _ok(1, [(0, 6, 0)])], RETRY))
    everything = [_ok(0, ws), _ok(1, [(0, 6, 0)]), (REFUSED, 2, [(0, 7, 0)]), (OTHER, 3, [])]
    cases.append(ClassifyCase("REQUEST_FAILED last wins over everything else",
                              everything + [(REQUEST_FAILED, 4, [])], THROW_FAILED))
    cases.append(ClassifyCase("REQUEST_FAILED first wins over everything else",
                              [(REQUEST_FAILED, 4, [])] + everything, THROW_FAILED))
    cases.append(ClassifyCase("REQUEST_FAILED alone", [(REQUEST_FAILED, 0, [])], THROW_FAILED))
    cases.append(ClassifyCase("OTHER alone", [(OTHER, 0, [])], THROW_REFUSED))
    cases.append(ClassifyCase("zero responses", [], PROCEED))
    cases.append(ClassifyCase("one OK response with no grants", [_ok(0, [])], PROCEED))
    # 64 responses x 8 grants: the kernel rescans the earlier responses per grant
    big = [_ok(100 + q, [((s + q) % 8, 1000 + (s + q) % 8, 0) for s in range(8)]) for q in range(64)]
    cases.append(ClassifyCase("64 responses x 8 grants uniform", big, PROCEED))
    off = big[:-1] + [_ok(163, big[-1][2][:-1] + [(big[-1][2][-1][0], 999, 0)])]
    cases.append(ClassifyCase("64 responses x 8 grants, the last grant differs", off, RETRY))
    twice = [_ok(100 + q % 32, [(s, (1000 if q >= 32 else 2000 + q) + s, 0) for s in range(8)]) for q in range(64)]
    cases.append(ClassifyCase("64 responses x 8 grants from 32 ids, the first of each differs", twice, PROCEED))
    return cases


def classify_dup_in_response():
    """One key slot twice in a single response: outside the model's contract (a MultiGrant's
    grants are a map); host and device must do what the oracle does."""
    cases = []
    for a, b in ((5, 5), (5, 6)):
        cases.append(ClassifyCase(f"dup slot ts ({a}, {b}) alone", [_ok(0, [(0, a, 0), (0, b, 0)])], None))
        cases.append(ClassifyCase(f"dup slot ts ({a}, {b}) before another server",
                                  [_ok(0, [(0, a, 0), (0, b, 0)]), _ok(1, [(0, 5, 0)])], None))
        cases.append(ClassifyCase(f"dup slot ts ({a}, {b}) after another server",
                                  [_ok(1, [(0, 5, 0)]), _ok(0, [(0, a, 0), (1, 7, 0), (0, b, 0)])], None))
        cases.append(ClassifyCase(f"dup slot ts ({a}, {b}) in a superseded response",
                                  [_ok(0, [(0, a, 0), (0, b, 0)]), _ok(0, [(0, 5, 0)])], None))
        cases.append(ClassifyCase(f"dup slot ts ({a}, {b}) in a REFUSED response",
                                  [(REFUSED, 0, [(0, a, 0), (0, b, 0)]), _ok(1, [(0, 5, 0)])], None))
    return cases


def classify_geometry(n: int):
    """n requests whose decision is the request index mod 5."""
    cases = []
    for i in range(n):
        want = i % 5
        t = 10 + i
        resps = {
            PROCEED: [_ok(0, [(0, t, 0)]), _ok(1, [(0, t, 0)])],
            RETRY: [_ok(0, [(0, t, 0)]), _ok(1, [(0, t + 1, 0)])],
            THROW_REFUSED: [_ok(0, [(0, t, 0)]), (REFUSED, 1, [(0, t + 1, 0)])],
            THROW_FAILED: [_ok(0, [(0, t, 0)]), (REQUEST_FAILED, 1, [])],
            THROW_UNSUPPORTED: [_ok(0, [(0, t, WRONG_SHARD)]), _ok(1, [(0, t, 0)])],
        }[want]
        cases.append(ClassifyCase(f"geometry n={n} i={i}", resps + [_ok(2, [(NO_OP_KEY, i, 0)])] * (i % 3), want))
    return cases


# One batch = one call of the function under test.  reason / chosen / decision are the
# model's, computed once per process and shared by every test (leave them unchanged).
TallyBatch = namedtuple("TallyBatch", "label R names responses n_ops reason chosen")
ClassifyBatch = namedtuple("ClassifyBatch", "label names responses expect decision")


def _tally_batch(label, R, cases):
    out = [tally(c.responses, c.k, R) for c in cases]
    return TallyBatch(label, R, [c.name for c in cases], [c.responses for c in cases], [c.k for c in cases],
                      [o[0] for o in out], [o[1] for o in out])


@functools.lru_cache(maxsize=None)
def tally_batches():
    """label -> TallyBatch: every tally set, one batch per replication factor."""
    batches = {}
    exhaustive = tally_exhaustive()
    for R in EXHAUSTIVE_R:
        batches[f"exhaustive_R{R}"] = _tally_batch(f"exhaustive_R{R}", R, exhaustive)
    sets = {"majority_line": tally_majority_line(), "status_values": tally_status_values(), "wide": tally_wide()}
    for n in TALLY_GEOMETRY_N:
        sets[f"geometry_{n}"] = tally_geometry(n)
    for name, cases in sets.items():
        groups = {}
        for c in cases:
            groups.setdefault(c.R, []).append(c)
        for R, group in groups.items():
            label = name if len(groups) == 1 else f"{name}_R{R}"
            batches[label] = _tally_batch(label, R, group)
    return batches


@functools.lru_cache(maxsize=None)
def classify_batches():
    """label -> ClassifyBatch: every classify set; dup_in_response has decision None."""
    sets = {"exhaustive": classify_exhaustive(), "timestamps": classify_timestamps(), "keys": classify_keys(),
            "servers": classify_servers(), "kinds": classify_kinds()}
    for n in CLASSIFY_GEOMETRY_N:
        sets[f"geometry_{n}"] = classify_geometry(n)
    batches = {}
    for label, cases in sets.items():
        batches[label] = ClassifyBatch(label, [c.name for c in cases], [c.responses for c in cases],
                                       [c.expect for c in cases], [classify(c.responses) for c in cases])
    dup = classify_dup_in_response()
    batches["dup_in_response"] = ClassifyBatch("dup_in_response", [c.name for c in dup], [c.responses for c in dup],
                                               [None] * len(dup), None)
    return batches


TALLY_LABELS = ([f"exhaustive_R{R}" for R in EXHAUSTIVE_R] + [f"majority_line_R{R}" for R in MAJORITY_LINE_R] +
                ["status_values_R4", "status_values_R7", "status_values_R10", "wide"] +
                [f"geometry_{n}" for n in TALLY_GEOMETRY_N])
CLASSIFY_LABELS = (["exhaustive", "timestamps", "keys", "servers", "kinds"] +
                   [f"geometry_{n}" for n in CLASSIFY_GEOMETRY_N] + ["dup_in_response"])
