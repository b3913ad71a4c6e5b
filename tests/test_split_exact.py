"""The deterministic split on the host, without a GPU: consistency.split_host against the 50-digit reference of split_exact.py inside its
a-priori bound over the committed cases of split_cases.py; the measurement K_SPLIT was taken from; the moment identity of
consistency.split_components inside the same bound; injected faults outside it; and what split_components and depth_axis_row refuse."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import split_cases as sc  # noqa: E402
import split_exact as sx  # noqa: E402
from eqf_vio_amd import consistency as cs  # noqa: E402

_CACHE = {}


def _case(name):
    """the case's operands, reference and bounds, computed once"""
    if name not in _CACHE:
        case = next(c for c in sc.CASES if c["name"] == name)
        Sigma, a, J, shift, shrink = sc.build(case)
        Ht, Hbar = sx.row_mp(a, J)
        ref = sx.exact(Sigma, Ht, shift, shrink)
        _CACHE[name] = dict(Sigma=Sigma, a=a, J=J, Ht64=a if J is None else a @ J, Hbar=Hbar, shift=shift, shrink=shrink, ref=ref)
    return _CACHE[name]


NAMES = [c["name"] for c in sc.CASES]
SMALL = [c["name"] for c in sc.CASES if c["N"] <= 21]


def test_cases_cover_what_they_are_meant_to():
    assert len(set(NAMES)) == len(NAMES)
    ill = sc.build(next(c for c in sc.CASES if c["name"] == "ill_scaled_21"))[0]
    d = np.sqrt(np.diag(ill))
    assert d.max() / d.min() > 100.0  # (more than two decades)
    one = sc.build(next(c for c in sc.CASES if c["name"] == "one_landmark"))[1]
    assert np.flatnonzero(one).tolist() == [20, 21, 22]
    assert any(c.get("local") for c in sc.CASES) and any(c["row"] == "dense_mixed" for c in sc.CASES)
    # the local cases' rotations are large: J's velocity block is a rotation by 2 to 3 rad
    J = sc.build(next(c for c in sc.CASES if c["name"] == "local_dense"))[2]
    ang = np.arccos(np.clip((np.trace(J[8:11, 8:11]) - 1.0) / 2.0, -1.0, 1.0))
    assert 2.0 <= ang <= 3.0
    shift, shrink = sc.children()
    assert (0.0, 0.0) in zip(shift, shrink) and 1.0 in shrink and 0.0 in shrink[shift != 0.0] and 0.0 in shift[shrink != 0.0]


@pytest.mark.parametrize("name", NAMES)
def test_split_host_lies_inside_the_bound(name):
    c = _case(name)
    got = cs.split_host(c["Sigma"], c["Ht64"], c["shift"], c["shrink"])
    bS, bG = sx.bound(c["Sigma"], c["Hbar"], c["shift"], c["shrink"])
    r = sx.ratios(got["Sigma"], got["gamma"], c["ref"], bS, bG)
    print(name, "worst ratio (of K_SPLIT = %g):" % sx.K_SPLIT, r)
    assert r["Sigma"] <= 1.0 and r["gamma"] <= 1.0
    # what the measurement of K_SPLIT rests on: with the constant 1 no case is beyond the worst written down in split_exact.py
    assert r["Sigma"] * sx.K_SPLIT <= sx.MEASURED_WORST["Sigma"] and r["gamma"] * sx.K_SPLIT <= sx.MEASURED_WORST["gamma"]
    assert abs(float(c["ref"]["S"]) - got["S"]) <= sx.K_SPLIT * sx.EPS * float(c["Hbar"] @ (np.abs(c["Sigma"]) @ c["Hbar"]))
    # exactness of the statement itself: no shrink keeps Sigma's bits, no shift gives a zero increment, Sigma_k is symmetric
    for k, (s, q) in enumerate(zip(c["shift"], c["shrink"])):
        if q == 0.0:
            assert np.array_equal(got["Sigma"][k], c["Sigma"])
        if s == 0.0:
            assert not got["gamma"][k].any()
        assert np.array_equal(got["Sigma"][k], got["Sigma"][k].T)


def test_constant_is_the_measurement_with_a_margin_of_four():
    assert sx.K_SPLIT == np.ceil(4.0 * max(sx.MEASURED_WORST.values()))
    assert sx.EPS == np.finfo(np.float64).eps


@pytest.mark.parametrize("name", SMALL)
@pytest.mark.parametrize("fault", sx.FAULTS)
def test_injected_faults_fall_outside_the_bound(name, fault):
    c = _case(name)
    sg, gm = sx.faulty(c["Sigma"], c["Ht64"], c["shift"], c["shrink"], fault)
    bS, bG = sx.bound(c["Sigma"], c["Hbar"], c["shift"], c["shrink"])
    r = sx.ratios(sg, gm, c["ref"], bS, bG)
    assert max(r.values()) > 1.0, (name, fault, r)
    # ... and without the fault the same code is inside
    sg, gm = sx.faulty(c["Sigma"], c["Ht64"], c["shift"], c["shrink"], None)
    r = sx.ratios(sg, gm, c["ref"], bS, bG)
    assert max(r.values()) <= 1.0, (name, r)


COMPONENTS = [(2, 0.3, None), (2, 1.0, None), (3, 0.9, None), (3, 1.5, 0.2), (3, 1.0, 0.5 - 1e-9), (3, 2.0, 0.125), (2, 0.0, None)]


@pytest.mark.parametrize("K, spread, q", COMPONENTS)
def test_split_components_satisfy_the_three_constraints(K, spread, q):
    w, shift, shrink = cs.split_components(K, spread, outer_weight=q)
    assert len(w) == len(shift) == len(shrink) == K
    assert abs(w.sum() - 1.0) <= 2e-16 and abs(w @ shift) <= 2e-16 * spread and abs(w @ (shift ** 2 - shrink)) <= 4e-16 * max(spread ** 2, 1.0)
    assert (shrink >= 0.0).all() and (shrink <= 1.0).all() and (w > 0.0).all()
    if K == 2:
        assert w.tolist() == [0.5, 0.5] and shift.tolist() == [-spread, spread] and shrink.tolist() == [spread ** 2] * 2
    else:
        qq = 0.25 if q is None else q
        assert w.tolist() == [qq, 1.0 - 2.0 * qq, qq] and shift.tolist() == [-spread, 0.0, spread]
        assert len(set(shrink.tolist())) == 1 and abs(shrink[0] - 2.0 * qq * spread ** 2) <= 4e-16 * max(spread ** 2, 1.0)


@pytest.mark.parametrize("args", [(2, 1.01, None), (3, 1.5, None), (3, 2.0, 0.2), (4, 0.5, None), (1, 0.5, None), (3, 0.5, 0.0), (3, 0.5, 0.5),
                                  (3, 0.5, -0.1), (2, 0.5, 0.3), (2, -0.5, None), (2, float("nan"), None), (3, float("inf"), None)])
def test_split_components_refuse_what_would_leave_the_unit_interval(args):
    with pytest.raises(ValueError):
        cs.split_components(args[0], args[1], outer_weight=args[2])


@pytest.mark.parametrize("name", ["ill_scaled_5", "one_landmark_ill", "dense_mixed_21", "local_dense"])
@pytest.mark.parametrize("K, spread, q", [(2, 0.8, None), (3, 1.2, 0.2), (3, 1.0, None)])
def test_moment_identity_inside_the_bound(name, K, spread, q):
    """sum_k w_k (Sigma_k + gamma_k gamma_k^T) = Sigma from split_host's children, summed at 50 digits"""
    c = _case(name)
    w, shift, shrink = cs.split_components(K, spread, outer_weight=q)
    got = cs.split_host(c["Sigma"], c["Ht64"], shift, shrink)
    bS, bG = sx.bound(c["Sigma"], c["Hbar"], shift, shrink)
    r = sx.moment_ratio(w, got["Sigma"], got["gamma"], c["Sigma"], bS, bG)
    print(name, K, spread, "moment identity, worst ratio:", r)
    assert r <= 1.0
    # a triple that is not moment-matched is outside: the identity is a property of the components, not of the bound's width
    bad = sx.moment_ratio(w, got["Sigma"], 1.01 * got["gamma"], c["Sigma"], bS, bG)
    assert bad > 1.0


def test_split_host_refuses_a_functional_without_variance():
    Sg = np.eye(14)
    with pytest.raises(np.linalg.LinAlgError):
        cs.split_host(Sg, np.zeros(14), [0.0], [0.0])
    Sg[3, 3] = -1.0
    with pytest.raises(np.linalg.LinAlgError):
        cs.split_host(Sg, np.eye(14)[3], [0.0], [0.0])


def test_depth_axis_row():
    p = np.array([0.3, -0.4, 1.2])
    r = cs.depth_axis_row(p, 2, 11 + 3 * 4)
    assert r.shape == (23,) and np.flatnonzero(r).tolist() == [17, 18, 19]
    assert np.array_equal(r[17:20], p / np.linalg.norm(p)) and abs(np.linalg.norm(r) - 1.0) <= 2e-16
    # it measures the position along the bearing: a displacement along p changes the functional by its length
    assert abs(r[17:20] @ (0.25 * p / np.linalg.norm(p)) - 0.25) <= 1e-16
    for bad in ((p, 4, 23), (p, -1, 23), (np.zeros(3), 0, 23)):
        with pytest.raises(ValueError):
            cs.depth_axis_row(*bad)
