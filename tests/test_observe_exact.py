"""The rows of eqf_observe_landmarks without a GPU: consistency.observe_rows_host (the numpy statement) against the 50-digit reference of
tests/observe_exact.py on every entry of every committed case of tests/observe_cases.py, inside K_OBS u (sum of absolute terms); K_OBS
re-measured; exact zeros where the reference's are; and the restatement's faults outside the bound.  The host build of
csrc/eqf_observe_host.hpp is held to the same bound in tests/test_observe_host.py, the device in tests/test_gpu_observe.py."""
import numpy as np
import pytest
from mpmath import mpf

import lie_exact as lx
import observe_cases as oc
import observe_exact as ox
from eqf_vio_amd import consistency as cs


@pytest.fixture(scope="module")
def refs():
    out = {}
    for c in oc.CASES:
        kind, st, ids, meas, cam = oc.case(c)
        out[c] = (kind, st, ids, meas, cam, ox.reference(kind, st, ids, meas, cam))
    return out


def _floats(ref, rows):
    Ht = [np.zeros((rows, 3)) if h is None else np.array([[float(x) for x in r] for r in h]) for h in ref["Ht"]]
    rs = [np.zeros(rows) if r is None else np.array([float(x) for x in r]) for r in ref["resid"]]
    return Ht, rs


def test_cases_cover_what_they_claim():
    depths, scales, angles = [], [], []
    for c in oc.CASES:
        kind, st, ids, meas, cam = oc.case(c)
        J = cs.landmark_jacobian_blocks(st["group"])
        p_hat = np.einsum("nij,nj->ni", J, st["origin"]["p"])
        depths += list(np.linalg.norm(p_hat, axis=1))
        scales += list(st["group"]["Qa"])
        if kind == cs.OBS_BEARING:
            Rc, tc = (np.eye(3), np.zeros(3)) if cam is None else (cs.quat_to_matrix(cam[0]), cam[1])
            for i in range(len(p_hat)):
                yh = Rc.T @ (p_hat[i] - tc)
                yh /= np.linalg.norm(yh)
                angles.append(np.arctan2(np.linalg.norm(np.cross(yh, meas[i])), yh @ meas[i]))
    assert {c[0] for c in oc.CASES} == {0, 1, 2} and {c[2] for c in oc.CASES} == {5, 22} and {c[1] for c in oc.CASES} == {"identity", "offset"}
    assert min(depths) <= 0.31 and max(depths) >= 299.0 and max(scales) / min(scales) >= 99.0
    assert min(angles) <= 1.1e-6 and max(angles) >= 1.19
    q, t = oc.camera("offset")
    assert abs(2 * np.arccos(q[0]) - 0.3) < 1e-12 and abs(np.linalg.norm(t) - 0.1) < 1e-12


def test_numpy_statement_inside_the_bound_and_k_obs_is_what_was_measured(refs):
    worst = 0.0
    for c, (kind, st, ids, meas, cam, ref) in refs.items():
        Ht, resid, used = cs.observe_rows_host(kind, st, ids, meas, cam)
        rh, rr = ox.ratios(Ht, resid, used, ref, k_obs=1.0)
        print(f"{c}: numpy statement / unit form: Ht {rh:.3f}, resid {rr:.3f}")
        worst = max(worst, rh, rr)
        assert max(ox.ratios(Ht, resid, used, ref)) <= 1.0, c
        if c[2] == 22:
            assert used[-1] == 0 and np.all(Ht[-1] == 0) and np.all(resid[-1] == 0)
    print(f"worst ratio of the numpy statement to the unit form: {worst!r} (K_OBS_MEASURED {ox.K_OBS_MEASURED!r}, K_OBS {ox.K_OBS})")
    assert worst <= 1.05 * ox.K_OBS_MEASURED  # (numpy's sums may be ordered differently on another host)
    assert ox.K_OBS == 2.0 ** np.ceil(np.log2(4.0 * ox.K_OBS_MEASURED)) and ox.K_OBS > 4.0 * ox.K_OBS_MEASURED


def test_residual_is_exactly_zero_where_the_references_is():
    """On the chart's axis (p_hat on -e3: R_s = I exactly), with a power-of-two scale and no rotation, every stage is exact: a measurement
    with the bits of the reference's prediction rounded gives resid = 0 exactly, for every kind.  Off the axis the reference's own resid
    for y = fl(y_hat) is a rounding of y_hat, and the statement stays inside the bound."""
    st = dict(ids=np.array([7], dtype=np.int32), origin=dict(p=np.array([[0.0, 0.0, -6.0]])),
              group=dict(Qq=np.array([[1.0, 0, 0, 0]]), Qa=np.array([4.0])))
    for kind, m in ((cs.OBS_BEARING, [0.0, 0.0, -1.0]), (cs.OBS_RANGE, [1.5, 0, 0]), (cs.OBS_POSITION, [0.0, 0.0, -1.5])):
        ref = ox.reference(kind, st, [7], [m])
        assert all(x == 0 for x in ref["resid"][0])
        Ht, resid, used = cs.observe_rows_host(kind, st, [7], [m])
        assert used[0] == 1 and np.all(resid == 0.0)
        assert max(ox.ratios(Ht, resid, used, ref)) <= 1.0
    kind, st, ids, meas, cam = oc.case((cs.OBS_BEARING, "offset", 5))
    ref = ox.reference(kind, st, ids, meas, cam)
    y = np.array([[float(x) for x in _yhat(st, k, cam)] for k in range(5)])
    ref0 = ox.reference(kind, st, ids, y, cam)
    Ht, resid, used = cs.observe_rows_host(kind, st, ids, y, cam)
    assert np.all(np.abs(resid) < 1e-15) and max(ox.ratios(Ht, resid, used, ref0)) <= 1.0
    assert ref["used"].tolist() == [1] * 5


def _yhat(st, i, cam):
    camv = np.concatenate([cam[0], cam[1]])
    R, Rc = lx.rot_of_quat(st["group"]["Qq"][i]), lx.rot_of_quat(camv[:4])
    ph = lx.scl(1 / mpf(float(st["group"]["Qa"][i])), lx.mv(lx.tr(R), lx.vec(st["origin"]["p"][i])))
    return lx.unit(lx.mv(lx.tr(Rc), lx.sub(ph, lx.vec(camv[4:]))))


# where each fault shows: (kind, offset) -- a fault of the offset needs one, a fault of the chart a bearing
FAULT_CASES = {"rc_transposed": (cs.OBS_BEARING, "offset"), "tc_sign": (cs.OBS_RANGE, "offset"), "inv_d_squared": (cs.OBS_BEARING, "identity"),
               "pole_at_y": (cs.OBS_BEARING, "offset"), "j_without_scale": (cs.OBS_POSITION, "identity"),
               "h_left_in_camera_frame": (cs.OBS_RANGE, "offset"), "resid_sign": (cs.OBS_POSITION, "offset"),
               "j_transposed": (cs.OBS_RANGE, "identity")}


@pytest.mark.parametrize("fault", ox.FAULTS)
def test_injected_faults_are_outside_the_bound(refs, fault):
    assert set(FAULT_CASES) == set(ox.FAULTS) and len(ox.FAULTS) >= 6
    kind, camname = FAULT_CASES[fault]
    for N in oc.SIZES:
        _, st, ids, meas, cam, ref = refs[(kind, camname, N)]
        Ht, resid = _floats(ox.reference(kind, st, ids, meas, cam, fault=fault), ox.ROWS[kind])
        rh, rr = ox.ratios(Ht, resid, ref["used"], ref)
        print(f"{fault} N={N}: Ht / bound {rh:.3g}, resid / bound {rr:.3g}")
        assert max(rh, rr) > 1.0


def test_the_projector_changes_nothing_at_the_charts_own_base_point(refs):
    """(I - y_hat y_hat^T) in the bearing's H is the differential of p / |p|; behind chart_diff(y_hat, y_hat) it is algebraically the
    identity, because the chart's differential at its base point annihilates y_hat: leaving it out is no fault the rows can show, and
    the restatement without it stays inside the bound."""
    for N in oc.SIZES:
        kind, st, ids, meas, cam, ref = refs[(cs.OBS_BEARING, "offset", N)]
        for i in range(N):
            yh = _yhat(st, i, cam)
            assert all(abs(x) < mpf(10) ** -45 for x in lx.mv(lx.chart_diff(yh, yh), yh))
        Ht, resid = _floats(ox.reference(kind, st, ids, meas, cam, fault="projector_missing"), 2)
        assert max(ox.ratios(Ht, resid, ref["used"], ref)) <= 1.0


def test_not_observable_entries_of_the_statement():
    st = dict(ids=np.array([1, 2, 3, 4], dtype=np.int32),
              origin=dict(p=np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 2.0], [0.0, 0.0, -2.0], [np.inf, 0.0, 1.0]])),
              group=dict(Qq=np.tile([1.0, 0, 0, 0], (4, 1)), Qa=np.ones(4)))
    y = np.array([[0.0, 0, 1], [0.0, 0, 1], [0.0, 0, 1], [0.0, 0, 1]])
    for kind, want in ((cs.OBS_BEARING, [3, 3, 3, 3]), (cs.OBS_RANGE, [3, 1, 1, 3]), (cs.OBS_POSITION, [3, 1, 1, 3])):
        Ht, resid, used = cs.observe_rows_host(kind, st, [1, 2, 3, 4], y)
        assert used.tolist() == want  # d = 0 | y_hat at the chart's pole e3 | y at the antipode of y_hat | p0 not finite
        assert np.all(Ht[used == 3] == 0) and np.all(resid[used == 3] == 0)
        assert ox.reference(kind, st, [1, 2, 3, 4], y)["used"].tolist() == want
