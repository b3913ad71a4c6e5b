"""One step of the iterated landmark observation update against the 50-digit reference of tests/iterate_exact.py, on the numpy statement
(consistency.observe_iterated_step / observe_iterated_host) and without a GPU: the statement inside the bounds on every committed case of
tests/iterate_cases.py, K_ITER re-measured, six injected faults outside the checks, and the behaviour the iteration is for -- a lower MAP
cost and a smaller gradient than the one-shot update, reached in fewer than the allowed linearisations."""
import numpy as np
import pytest

import iterate_cases as ic
import iterate_exact as ix
from eqf_vio_amd import consistency as cs

STEPS = 2  # the steps taken on their own per case: from g = 0 and from the first trial point


@pytest.fixture(scope="module")
def runs():
    """{case: (inputs, the statement's run, the entries that take part)}"""
    out = {}
    for c in ic.CASES:
        kind, st, ids, meas, R, cam = ic.case(c)
        host = cs.observe_iterated_host(kind, st["sigma"], st, ids, meas, R, cam, max_lin=ic.MAX_LIN, tol=ic.TOL)
        out[c] = ((kind, st, ids, meas, R, cam), host, [int(k) for k in np.flatnonzero(host["used"] == 1)])
    return out


@pytest.fixture(scope="module")
def refs(runs):
    """{(case, k): the one-step reference from g_trace[k]}, shared and left unchanged"""
    out = {}
    for c, ((kind, st, ids, meas, R, cam), host, on) in runs.items():
        for k in range(STEPS):
            out[c, k] = ix.one_step(kind, st["sigma"], st, ids, meas, R, host["g_trace"][k], on, cam)
    return out


def test_the_statement_is_inside_the_bounds_and_k_iter_is_what_was_measured(runs, refs):
    worst_rows, worst = 0.0, 0.0
    for (c, k), ref in refs.items():
        (kind, st, ids, meas, R, cam), host, on = runs[c]
        Ht, rt, gn, stalled = cs.observe_iterated_step(kind, st["sigma"], st, ids, meas, R, host["g_trace"][k], on, cam)
        assert not stalled
        rh, rr = ix.row_ratios(Ht, rt, ref)
        r = ix.step_ratio(gn, ref, k_iter=1.0)
        print(f"{c} step {k}: statement / bound: Ht {rh:.3f}, r~ {rr:.3f}; g_next / unit form {r:.3e}")
        worst_rows, worst = max(worst_rows, rh, rr), max(worst, r)
    assert worst_rows <= 1.0
    print(f"worst g_next ratio to the unit form {worst:.4e} (recorded: {ix.K_ITER_MEASURED:.4e})")
    assert 4.0 * worst <= ix.K_ITER and ix.K_ITER == 2.0 ** np.ceil(np.log2(4.0 * ix.K_ITER_MEASURED))


def test_the_first_linearisation_is_the_one_shot_rows(runs):
    for c, ((kind, st, ids, meas, R, cam), host, on) in runs.items():
        Ht, resid, used = cs.observe_rows_host(kind, st, ids, meas, cam)
        H0, r0, _, _ = cs.observe_iterated_step(kind, st["sigma"], st, ids, meas, R, np.zeros((len(ids), 3)), on, cam)
        assert np.array_equal(Ht, H0) and np.array_equal(resid, r0) and np.array_equal(used, host["used"])
        assert not host["g_trace"][0].any()


@pytest.mark.parametrize("fault", ix.FAULTS)
def test_a_faulty_step_lands_outside_the_checks(runs, refs, fault):
    caught = 0
    for c in (ic.CASES[1], ic.CASES[5], ic.CASES[9]):   # N = 22, identity offset: a bearing, a range, a position
        (kind, st, ids, meas, R, cam), host, on = runs[c]
        consider = [int(ids[on[1]]), int(ids[on[4]])] if fault == "considered_moved" else None
        ref = refs[c, 1] if consider is None else ix.one_step(kind, st["sigma"], st, ids, meas, R, host["g_trace"][1], on, cam, consider)
        good = ix.model_step(kind, st["sigma"], st, ids, meas, R, host["g_trace"][1], on, cam, consider)
        assert max(ix.row_ratios(good[0], good[1], ref)) <= 1.0 and ix.step_ratio(good[2], ref) <= 1.0
        Ht, rt, gn = ix.model_step(kind, st["sigma"], st, ids, meas, R, host["g_trace"][1], on, cam, consider, fault=fault)
        out = max(max(ix.row_ratios(Ht, rt, ref)), ix.step_ratio(gn, ref))
        print(f"{fault} on {c}: {out:.3g} x the bound")
        caught += out > 1.0
    assert caught == 3


@pytest.mark.parametrize("fault", ix.RUN_FAULTS)
def test_a_faulty_sequence_lands_outside_the_checks(runs, fault):
    # a gate between an entry's own distance at linearisation 0 and at linearisation 1: gating again would change the verdicts (the second
    # camera's bearings have an entry whose distance grows on the way, the ranges' all shrink; the stop rule is checked where the statement
    # converges)
    c = ic.CASES[3] if fault == "regate" else ic.CASES[5]
    (kind, st, ids, meas, R, cam), _, _ = runs[c]
    K = len(ids)
    sid = [int(i) for i in st["ids"]]
    idx = np.array([sid.index(int(i)) if int(i) in sid else -1 for i in ids])
    Ht0, r0, _ = cs.observe_rows_host(kind, st, ids, meas, cam)
    d0 = cs.update_landmarks_host(st["sigma"], idx, Ht0, r0, R)["d2"]
    on = [k for k in range(K) if idx[k] >= 0]
    H1, r1, g1, _ = cs.observe_iterated_step(kind, st["sigma"], st, ids, meas, R, np.zeros((K, 3)), on, cam)
    H2, r2, _, _ = cs.observe_iterated_step(kind, st["sigma"], st, ids, meas, R, g1, on, cam)
    d1 = cs.update_landmarks_host(st["sigma"], idx, H2, r2, R)["d2"]
    k = max(on, key=lambda e: d1[e] / d0[e])
    lm_gate = 0.5 * (d0[k] + d1[k]) if fault == "regate" else np.inf
    assert fault != "regate" or d1[k] > 1.01 * d0[k]
    host = cs.observe_iterated_host(kind, st["sigma"], st, ids, meas, R, cam, max_lin=ic.MAX_LIN, tol=ic.TOL, lm_gate=lm_gate)
    want = (list(host["used"]), host["n_lin"], host["status"])
    good = ix.model_run(kind, st["sigma"], st, ids, meas, R, cam, ic.MAX_LIN, ic.TOL, lm_gate)
    assert (list(good[0]), good[1], good[2]) == want and host["used"][k] == 1
    bad = ix.model_run(kind, st["sigma"], st, ids, meas, R, cam, ic.MAX_LIN, ic.TOL, lm_gate, fault=fault)
    assert (list(bad[0]), bad[1], bad[2]) != want


@pytest.mark.parametrize("c", ic.BEHAVIOUR)
def test_the_iteration_lowers_the_map_cost_and_its_gradient_and_stops_early(runs, c):
    (kind, st, ids, meas, R, cam), host, _ = runs[c]
    one = cs.observe_iterated_host(kind, st["sigma"], st, ids, meas, R, cam, max_lin=1)
    assert one["n_lin"] == 1 and one["status"] == cs.ITER_EXHAUSTED and np.array_equal(one["used"], host["used"])
    ci, gi = cs.map_cost(kind, st["sigma"], st, ids, meas, R, host["gamma"], host["used"], cam, gradient=True)
    co, go = cs.map_cost(kind, st["sigma"], st, ids, meas, R, one["gamma"], one["used"], cam, gradient=True)
    print(f"{c}: n_lin {host['n_lin']}, cost {ci:.6g} (one-shot {co:.6g}), |gradient| {np.linalg.norm(gi):.3g} (one-shot {np.linalg.norm(go):.3g})")
    assert host["status"] == cs.ITER_CONVERGED and host["n_lin"] < ic.MAX_LIN and host["last_step"] <= ic.TOL
    assert ci <= co and np.linalg.norm(gi) < np.linalg.norm(go)


def test_the_stall_case_is_a_stall_on_the_statement(runs):
    (kind, st, ids, meas, R, cam), _, _ = runs[ic.CASES[4]]
    st2, ids2, meas2, R2 = ix.stall_case(st)
    host = cs.observe_iterated_host(cs.OBS_RANGE, st2["sigma"], st2, ids2, meas2, R2, max_lin=4)
    assert host["status"] == cs.ITER_STALLED and host["n_lin"] == 1 and host["last_step"] > 0 and not host["g_trace"].any()
    one = cs.observe_rows_host(cs.OBS_RANGE, st2, ids2, meas2)
    assert np.array_equal(host["Ht"], one[0]) and np.array_equal(host["resid"], one[1])
    # the construction: the first increment drives the scale's exponent below what exp can hold
    p0 = np.asarray(st2["origin"]["p"], dtype=float).reshape(-1, 3)[0]
    _, _, g1, _ = cs.observe_iterated_step(cs.OBS_RANGE, st2["sigma"], st2, ids2, meas2, R2, np.zeros((1, 3)), [0])
    assert -float(p0 @ g1[0]) / float(p0 @ p0) < -745.0
