"""The innovation lift of the non-vision calls (csrc/eqf_lift.hpp) on the CPU: the fp64 numpy oracle and consistency.bundle_lift_host against
the 50-digit reference of tests/lift_exact.py on every case of tests/lift_cases.py, inside the measured bound; a table of injected faults
outside it.  No case is skipped.  The worst ratios are printed (pytest -s) so that the stored ORACLE_* constants can be re-read off a run."""
import numpy as np
import pytest

import lift_cases as lc
import lift_exact as le
import linear_cases
from eqf_vio_amd import consistency as cs


@pytest.fixture(scope="module")
def refs():
    """{(N, discrete, increment): (gamma, Sigma+, snapshot, settings, reference)}, computed once"""
    out = {}
    for N, disc in lc.CASES:
        d = lc.settings(disc)
        snap = lc.snapshot(N)
        for inc in lc.INCREMENTS:
            gamma, Sp = lc.increment(N, inc, snap)
            out[(N, disc, inc)] = (gamma, Sp, snap, d, le.reference(gamma, snap, snap["sigma"], d["cameraOffset_q"], d["cameraOffset_x"], disc))
    return out


def test_constants_are_four_times_the_measured_ratios():
    assert lc.K_LIFT == 4 * max(lc.ORACLE_DU.values()) > 0 and lc.K_STEP == 4 * max(lc.ORACLE_X.values()) > 0
    assert set(lc.ORACLE_DU) == set(lc.SIZES)


def test_cases_cover_what_they_claim():
    assert [6 + 3 * N for N in lc.SIZES] == [12, 15, 63, 66, 129, 261]
    assert {d for _, d in lc.CASES} == {0, 1} and len(lc.CASES) == 2 * len(lc.SIZES)
    snap = lc.snapshot(max(lc.SIZES))
    Aq = snap["group"]["Aq"]
    assert 2 * np.arccos(abs(Aq[0]) / np.linalg.norm(Aq)) > 1.0                       # rotations beyond 1 rad
    Qa = snap["group"]["Qa"]
    assert Qa.max() / Qa.min() > 100.0                                                 # scales over two decades
    for N in lc.SIZES:
        S = lc.own_sigma(N)
        assert np.array_equal(S, S.T) and np.linalg.eigvalsh(S[6:, 6:]).min() > 0.0


@pytest.mark.parametrize("who", ["oracle", "host"])
def test_fp64_lifts_lie_inside_the_bound_on_every_case(refs, who):
    worst_du, worst_x = {}, {}
    for (N, disc, inc), (gamma, _, snap, d, ref) in refs.items():
        if who == "oracle":
            got = lc.oracle_lift(gamma, snap, snap["sigma"], d)
        else:
            got = cs.bundle_lift_host(gamma, lc.lift_state(snap, d), snap["sigma"])
        worst_du[N] = max(worst_du.get(N, 0.0), le.ratio_dU(got["DeltaU"], ref))
        for k, v in le.ratios_X(got["group"], got["bias"], ref, lc.K_LIFT).items():
            worst_x[k] = max(worst_x.get(k, 0.0), v)
    print(who, "DeltaU ratios per size:", worst_du, " X ratios:", worst_x)
    assert max(worst_du.values()) <= lc.K_LIFT, worst_du
    assert max(worst_x.values()) <= lc.K_STEP, worst_x
    if who == "oracle":  # the stored constants are this machine's to a few digits (another BLAS rounds differently, not by a factor)
        assert max(worst_du.values()) >= 0.25 * max(lc.ORACLE_DU.values())


def test_host_statement_reports_the_pivots(refs):
    gamma, _, snap, d, ref = refs[(20, 1, "zupt")]
    got = cs.bundle_lift_host(gamma, lc.lift_state(snap, d), snap["sigma"])
    L = np.linalg.cholesky(snap["sigma"][6:, 6:])
    assert got["min_pivot"] == float(np.min(np.diag(L)) ** 2) and 0.0 < got["pivot_ratio"] <= 1.0
    assert abs(1.0 / got["pivot_ratio"] - ref["kM"]) <= 10.0 * ref["kM"]


@pytest.mark.parametrize("fault", le.FAULTS)
def test_injected_faults_leave_the_bound(refs, fault):
    """each on a case where it can show, discrete lift, N = 20: the zupt increment (its gamma_e has a top part) -- but the stereo increment
    for the post-update Sigma: rows on the velocity alone leave the landmark block of Sigma_e^-1, all the weight D^T Sigma_e^-1 D reads,
    exactly as it was (information form: Sigma_e+^-1 = Sigma_e^-1 + H^T R^-1 H), so a ZUPT cannot tell the two"""
    gamma, Sp, snap, d, ref = refs[(20, 1, "stereo" if fault == "post_sigma" else "zupt")]
    bad = le.faulty(fault, gamma, snap, snap["sigma"], Sp, d["cameraOffset_q"], d["cameraOffset_x"], 1)
    du = [float(v) for v in bad["DeltaU"]]
    r_du = le.ratio_dU(du, ref)
    g = linear_cases.group_dict(bad["X"])
    r_x = le.ratios_X(g, [float(v) for v in bad["bias"]], ref, lc.K_LIFT)
    print(fault, "DeltaU ratio / K_LIFT: %.3g" % (r_du / lc.K_LIFT), " X ratios / K_STEP:", {k: "%.3g" % (v / lc.K_STEP) for k, v in r_x.items()})
    assert r_du > lc.K_LIFT or max(r_x.values()) > lc.K_STEP, (fault, r_du, r_x)


def test_unprojected_fixed_part_is_inert(refs):
    """`dU_f not projected` cannot leave the bound, and does not: dUw = -eta0 x t is orthogonal to eta0 already, and a component along eta0 in
    dU_f is a multiple of K_par's first column, which the least squares takes back out.  (The fault that CAN show there, the G6 dU_f term
    dropped from the right-hand side, is in the table above.)"""
    assert len(le.FAULTS) >= 8 and le.INERT == ("no_projection",)
    gamma, Sp, snap, d, ref = refs[(20, 1, "zupt")]
    same = le.faulty("no_projection", gamma, snap, snap["sigma"], Sp, d["cameraOffset_q"], d["cameraOffset_x"], 1)
    assert le.ratio_dU([float(v) for v in same["DeltaU"]], ref) <= lc.K_LIFT
