"""The low-rank linear measurement update on the CPU (csrc/eqf_linear.hpp: eqf_update_linear; consistency.linear_update_host and the
rows helpers): the reference and the bound of tests/linear_exact.py on every committed case of tests/linear_cases.py.

  * consistency.linear_update_host (LAPACK) and linear_exact.model (numpy, the kernels' blocking) sit inside every bound;
  * the longdouble reference against mpmath at 50 digits (n <= 60) takes a negligible share of any bound;
  * every injected fault of linear_exact.FAULTS leaves some bound by >= 100 on some case (the table is printed);
  * consistency.chi2_gate_threshold: dof = 2 unchanged bit for bit, dof 1..16 against the regularised gamma function in mpmath;
  * sign and chart from the reference alone: a velocity and a landmark measurement pull the estimate onto the truth.
R is handed over with its upper triangle negated everywhere: only the lower triangle may be read."""
import numpy as np
import pytest
from mpmath import mp, mpf

import consistency_cases as cc
import consistency_exact as cx
import lie_exact as lx
import linear_cases as lc
import linear_exact as le
from eqf_vio_amd import consistency as cs


@pytest.fixture(scope="module")
def master_J():
    s = cc.local_state(max(lc.SIZES + lc.RAGGED), lc.THETA)
    return cx.jacobian_mp(s["origin"], s["group"])


def _poison(R):
    return np.tril(R) - np.triu(R, 1)


def _cases(sizes=lc.SIZES):
    for N in sizes:
        for fam, local, m, hfam, rkind in lc.plan(N):
            if fam != "own":
                yield N, fam, local, m, hfam, rkind


def _operands(N, fam, local, m, hfam, rkind):
    snap = lc.snapshot(N, fam)
    Sg = snap["sigma"]
    blocks = cs.local_jacobian_blocks(snap["origin"], snap["group"])
    H = lc.rows(N, m, hfam)
    Ht64 = H @ cs.jacobian_matrix(blocks) if local else H
    R = lc.noise(Sg, Ht64, H.shape[0], rkind)
    r = lc.residual(Sg, Ht64, R)
    return snap, Sg, blocks, H, Ht64, R, r


@pytest.fixture(scope="module")
def references(master_J):
    """{case: (operands, reference, bounds)}: computed once, shared, never changed"""
    out = {}
    for case in _cases():
        ops = _operands(*case)
        Ht, dHt = le.rows(ops[3], case[2], master_J)
        ref = le.reference(ops[1], Ht, ops[6], ops[5])
        out[case] = (ops, ref, le.bounds(ref, dHt))
    return out


def test_host_update_and_blocking_model_inside_every_bound(references):
    worst = {}
    for case, ((snap, Sg, blocks, H, Ht64, R, r), ref, bnd) in references.items():
        assert bnd["validity"] <= le.VALIDITY, (case, bnd["validity"])
        host = cs.linear_update_host(Sg, Ht64, r, _poison(R))
        mod = le.model(Sg, H, r, _poison(R), case[2], blocks)
        assert mod["info"] == 0 and mod["pad_zero"], case
        assert np.array_equal(mod["Sigma"], mod["Sigma"].T) or not np.array_equal(Sg, Sg.T), case
        for name, got in (("host", host), ("model", mod)):
            rt = le.ratios(got, ref, bnd)
            for k, v in rt.items():
                worst[(name, k)] = max(worst.get((name, k), 0.0), v)
                assert v <= 1.0, (case, name, k, v)
    print("worst |value - reference| / bound over the committed cases:")
    for name in ("host", "model"):
        print(f"  {name:6s}", "  ".join(f"{k} {worst[(name, k)]:.3f}" for k in ("Sp", "gamma", "nis", "logdet_S", "loglik")))


def test_longdouble_reference_against_mpmath(master_J):
    """n <= 60: N = 0, 1 of the committed sizes and the ragged handle's N = 5"""
    share = 0.0
    for case in _cases((0, 1, 5)):
        snap, Sg, blocks, H, Ht64, R, r = _operands(*case)
        assert len(Sg) <= le.MP_MAX_ORDER
        Ht, dHt = le.rows(H, case[2], master_J)
        ref = le.reference(Sg, Ht, r, R)
        bnd = le.bounds(ref, dHt)
        Hm, _ = le.rows(H, case[2], master_J, use_mp=True)
        rmp = le.reference(Sg, Hm, r, R, use_mp=True)
        for k, key in (("Sp", "Sp"), ("gamma", "gamma")):
            d = np.array([[abs(mpf(float(a)) + mpf(float(a - le.LD(float(a)))) - b) for a, b in zip(ra, rb)]
                          for ra, rb in zip(np.atleast_2d(ref[k]), np.atleast_2d(rmp[k]))], dtype=object)
            q = np.array([[float(x) for x in row] for row in d]) / np.where(np.atleast_2d(bnd[key]) > 0, np.atleast_2d(bnd[key]), np.inf)
            assert not d[np.atleast_2d(bnd[key]) == 0].any(), (case, k)
            share = max(share, float(q.max()))
        for k in ("nis", "logdet_S", "loglik"):
            a = ref[k]
            share = max(share, float(abs(mpf(float(a)) + mpf(float(a - le.LD(float(a)))) - rmp[k])) / bnd[k])
    print(f"longdouble against 50 digits: largest share of a bound {share:.2e}")
    assert share < 0.01


def test_every_injected_fault_leaves_a_bound_by_100(references):
    table = {}
    for case, ((snap, Sg, blocks, H, Ht64, R, r), ref, bnd) in references.items():
        N, fam, local, m, hfam, rkind = case
        for fault in le.FAULTS:
            if fault in ("j_left", "scale_not_inverted") and not local:
                continue
            if fault == "y_last_row_dropped" and m != 15:
                continue
            if fault == "gated_downdated":
                mod = le.model(Sg, H, r, _poison(R), local, blocks, gate=0.5 * float(ref["nis"]), fault=fault)
                assert mod["info"] == 2
                bad = 0.0 if np.array_equal(mod["Sigma"], Sg) else np.inf  # (a gated filter keeps every bit: the bound is zero)
                honest = le.model(Sg, H, r, _poison(R), local, blocks, gate=0.5 * float(ref["nis"]))
                assert honest["info"] == 2 and np.array_equal(honest["Sigma"], Sg) and not honest["gamma"].any()
            else:
                mod = le.model(Sg, H, r, _poison(R), local, blocks, fault=fault)
                bad = max(le.ratios(mod, ref, bnd).values()) if mod["info"] == 0 else np.inf
            if bad >= 100.0:
                table.setdefault(fault, []).append((case, bad))
    print("fault -> cases on which some bound is left by >= 100 (count, first case, its ratio):")
    for fault in le.FAULTS:
        hits = table.get(fault, [])
        print(f"  {fault:22s} {len(hits):3d}", (hits[0][0], f"{hits[0][1]:.3g}") if hits else "")
        assert hits, f"fault {fault} is not seen on any committed case"


def test_chi2_gate_threshold():
    for p in (0.5, 0.95, 0.99, 0.999):
        assert cs.chi2_gate_threshold(p) == -2.0 * float(np.log1p(-p)) == cs.chi2_gate_threshold(p, dof=2)
    mp.dps = 50
    worst = 0.0
    for dof in range(1, 17):
        for p in (0.01, 0.5, 0.95, 0.99, 0.999):
            x = cs.chi2_gate_threshold(p, dof)
            # the quantile is held to the CDF: P(dof / 2, x / 2) = p to a few roundings of p, and x is the first double at or above it
            cdf = mp.gammainc(mpf(dof) / 2, 0, mpf(x) / 2, regularized=True)
            worst = max(worst, float(abs(cdf - mpf(p))))
            assert abs(cdf - mpf(p)) <= 64 * 2.0 ** -53, (dof, p, float(cdf))
            assert abs(mpf(cs.chi2_cdf(x, dof)) - cdf) <= 64 * 2.0 ** -53, (dof, p)
    print(f"chi2_gate_threshold, dof 1..16: largest |CDF(x) - p| {worst:.2e}")
    with pytest.raises(ValueError):
        cs.chi2_gate_threshold(0.5, dof=0)


# ---- sign and chart, from the reference alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["velocity", "landmark"])
def test_sign_and_chart_from_the_reference_alone(what):
    d = cc.settings()
    for N in (5, 18):
        snap, H, resid, R, truth, est, sl, J = lc.sign_and_chart_case(N, what, 0)
        before = lc.measured_error(est, truth, snap["bias"], truth["bias"], sl)
        gam = cs.linear_update_host(snap["sigma"], H @ J, resid, R)["gamma"]
        xi0 = lx.State.from_dict(snap["origin"], d["cameraOffset_q"], d["cameraOffset_x"])
        X = lx.apply_innovation(lx.Group.from_dict(snap["group"]), xi0, None, gam[8:11], gam[11:], "nolift", gg=gam[6:8])
        est1 = lc.estimate_of(snap["origin"], lc.group_dict(X), d)
        after = lc.measured_error(est1, truth, snap["bias"] + gam[:6], truth["bias"], sl)
        ratio = float(np.linalg.norm(after) / np.linalg.norm(before))
        wrong = cs.linear_update_host(snap["sigma"], H @ J, -resid, R)["gamma"]
        Xw = lx.apply_innovation(lx.Group.from_dict(snap["group"]), xi0, None, wrong[8:11], wrong[11:], "nolift", gg=wrong[6:8])
        rw = float(np.linalg.norm(lc.measured_error(lc.estimate_of(snap["origin"], lc.group_dict(Xw), d), truth, snap["bias"], truth["bias"], sl))
                   / np.linalg.norm(before))
        print(f"{what} N={N}: measured error after / before {ratio:.2e} (wrong sign {rw:.2f})")
        assert ratio < 0.1, (what, N, ratio)
        assert rw > 1.5
