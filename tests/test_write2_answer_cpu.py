"""Write2 answer plan, host form (mochi_write2_answer_plan): the host plan equals the
plain-Python server model (write2_answer_model) array for array on the named cases, alone
and in one batch with dense and guarded slots; plan -> mochi_result_reply_encode equals the
Write2AnsFromServer the model's server builds for the same transaction; argument errors."""
import ctypes

import numpy as np
import pytest

import mochi_hip as mh
import result_encode_model as E
import result_reply_model as RRM
import write2_answer_model as A

NAMES = [t.name for t in A.cases()]


def plan_checked(txs, slots="dense", what=""):
    wb, ms, bits, dec, st = A.batch(txs, slots)
    got = mh.write2_answer_plan(wb, ms, bits, dec, st, fill=A.FILL)
    RRM.assert_equal(got, A.expected(txs, wb, st), what)
    return wb, st, got


def test_case_names_are_unique_and_cover_every_verdict():
    assert len(set(NAMES)) == len(NAMES)
    assert {A.plan(t)[0] for t in A.cases()} == {mh.W2A_REPLY, mh.W2A_NO_REPLY, mh.W2A_HOST}


@pytest.mark.parametrize("name", NAMES)
def test_named_case(name):
    t = next(t for t in A.cases() if t.name == name)
    plan_checked([t], what=name)
    plan_checked([t], "guarded", what=name)


@pytest.mark.parametrize("slots", ["dense", "guarded"])
def test_all_cases_in_one_batch(slots):
    wb, st, got = plan_checked(A.cases(), slots)
    if slots == "guarded":
        assert (np.diff(st.slot_off.astype(np.int64)) < 0).all()


def test_the_verdicts_by_name():
    v = {t.name: A.plan(t)[0] for t in A.cases()}
    R, N, H = mh.W2A_REPLY, mh.W2A_NO_REPLY, mh.W2A_HOST
    want = {"apply:all": R, "ws:all_no_cert": R, "mixed": R, "delete": R, "read:no_stored_cert": R, "read:value_null": N,
            "apply:value_null_is_fine": R, "not_accepted": N, "failed:middle": N, "skipped:first": N, "status:malformed": N,
            "status:malformed_accepted": N, "status:ops_mismatch": N, "status:fallback_accepted": H,
            "status:fallback_rejected": N, "operand2:twice": R, "cert:after_transaction": R, "unknown:in_tx_and_op": R,
            "count:one_more_on_the_wire": N, "count:one_fewer_on_the_wire": N, "count:none_of_none": R,
            "walk:truncated": N, "walk:bad_op_inside": N}
    assert {k: v[k] for k in want} == want


def test_values_of_the_special_shapes():
    """The slices by value: last operand2, last action, the later certificate, DELETE."""
    by = {t.name: A.server_answer(t) for t in A.cases()}
    assert [o.result for o in by["operand2:twice"].ops] == [b"the-last-one", b"value-1"]
    assert [o.result for o in by["operand2:foreign_wire_type"].ops] == [b"", b"kept"]
    assert [o.existed for o in by["action:twice"].ops] == [False, True]
    assert [o.existed for o in by["action:foreign_wire_type"].ops] == [False, True]
    assert [o.existed for o in by["action:10_byte_varint"].ops] == [True]
    assert [o.existed for o in by["delete"].ops] == [False, True]
    assert by["cert:after_transaction"].ops[0].cert == A.CERT == by["cert:twice_last_wins"].ops[0].cert
    assert by["ws:all_no_cert"].ops == (E.OpR(1),) * 3
    assert by["cert:empty"].ops[0].cert == b"" and by["read:no_stored_cert"].ops[0].cert is None
    assert by["read:stored_cert"].ops[0] == E.OpR(0, b"stored-value", True, A.STORED, "s", "s")


@pytest.mark.parametrize("slots", ["dense", "guarded"])
def test_plan_then_encode_equals_the_server_models_answers(slots):
    txs = A.cases()
    wb, st, got = plan_checked(txs, slots)
    ra = mh.planned_answers(wb.wire, st.store, np.zeros(0, np.uint8), got, st.slot_off)
    wire, off, ln, status = mh.result_reply_encode(ra)
    answers = [A.server_answer(t) or E.Ans(E.OTHER) for t in txs]
    w_wire, w_off, w_ln, w_st = E.expected_arrays(answers)
    np.testing.assert_array_equal(status, w_st)
    np.testing.assert_array_equal(ln, w_ln)
    np.testing.assert_array_equal(off, w_off)
    assert wire.tobytes() == w_wire.tobytes()
    assert int((ln > 0).sum()) == sum(A.plan(t)[0] == mh.W2A_REPLY for t in txs)


def test_empty_batch_needs_no_pointer():
    lib = mh.load_library()
    b, s, o = mh.Write2Batch_C(), mh.Write2AnswerSource_C(), mh.Write2AnswerPlanned_C()
    assert lib.mochi_write2_answer_plan(ctypes.addressof(b), ctypes.addressof(s), ctypes.addressof(o)) == mh.OK


def _call(mutate):
    """The host form on the `mixed` case with one argument changed: (rc, error text)."""
    lib = mh.load_library()
    t = [next(t for t in A.cases() if t.name == "mixed")]
    wb, ms, bits, dec, st = A.batch(t)
    b, keep = mh.write2_batch_c(wb)
    arrs = st.arrays()
    s = mh.Write2AnswerSource_C()
    s.msg_status, s.cert_accept_bits, s.op_decision = mh._ptr(ms), mh._ptr(bits), mh._ptr(dec)
    for k in tuple(mh._W2A_STORE) + ("slot_off",):
        setattr(s, k, mh._ptr(arrs[k]))
    s.store_len, s.n_slots = int(arrs["store"].size), int(st.n_slots)
    out = {k: np.zeros(8, dt) for k, (dt, w) in mh._W2A_OUT.items()}
    o = mh.Write2AnswerPlanned_C()
    for k, a in out.items():
        setattr(o, k, mh._ptr(a))
    mutate(b, s, o, arrs, keep)
    rc = lib.mochi_write2_answer_plan(ctypes.addressof(b), ctypes.addressof(s), ctypes.addressof(o))
    return rc, mh._err(lib)


def test_the_unchanged_call_succeeds():
    assert _call(lambda *a: None)[0] == mh.OK


@pytest.mark.parametrize("where,field", [("b", "op_flags_off"), ("b", "msg_off"), ("b", "msg_len"), ("b", "wire"),
                                         ("s", "msg_status"), ("s", "cert_accept_bits"), ("s", "op_decision"),
                                         ("s", "op_value_off"), ("s", "op_stored_cert_len"), ("s", "op_store_flags"),
                                         ("s", "slot_off"), ("o", "plan_status"), ("o", "resp_kind"), ("o", "op_cert_off")])
def test_einval_for_a_null_array(where, field):
    def mutate(b, s, o, arrs, keep):
        setattr(dict(b=b, s=s, o=o)[where], field, None)
    assert _call(mutate)[0] == mh.EINVAL


def test_einval_for_inconsistent_inputs():
    def slice_outside(b, s, o, arrs, keep):
        b.wire_len = 5
    rc, err = _call(slice_outside)
    assert rc == mh.EINVAL and "message slice" in err

    def not_a_csr(b, s, o, arrs, keep):
        keep[3][0] = 1
    rc, err = _call(not_a_csr)
    assert rc == mh.EINVAL and "CSR" in err

    def slots_short(b, s, o, arrs, keep):
        s.n_slots = 3
    rc, err = _call(slots_short)
    assert rc == mh.EINVAL and "slot run" in err

    def value_outside(b, s, o, arrs, keep):
        arrs["op_value_len"][1] = 1 << 20
    rc, err = _call(value_outside)
    assert rc == mh.EINVAL and "stored value" in err

    def cert_outside(b, s, o, arrs, keep):
        arrs["op_stored_cert_off"][1] = 1 << 40
    rc, err = _call(cert_outside)
    assert rc == mh.EINVAL and "stored certificate" in err
