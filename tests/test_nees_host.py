"""consistency.nees_joint / error_vector (pure numpy, the host counterpart of FilterBatch.nees) against e @ solve(A, e) and slogdet on the
numpy oracle's N = 30 states, 1e-10 relative."""
import numpy as np
import pytest

from consistency_helpers import np_imu, numpy_filter, origin_group_of
from eqf_vio_amd import consistency, synth
from oracle import eqf_numpy as O


@pytest.fixture(scope="module")
def states():
    N = 30
    st = synth.make_stream(N, duration=0.4)
    fo = numpy_filter(synth.template_settings_dict())
    out = []
    for kind, k in st.events():
        if kind == "imu":
            np_imu(fo, st.imu[k])
        else:
            fo.processVisionData(st.vision_stamps[k], st.ids, st.bearings[k])
            origin, group = origin_group_of(fo)
            J = consistency.jacobian_matrix(consistency.local_jacobian_blocks(origin, group))
            est = O.state_group_action(fo.X, fo.xi0)
            out.append(dict(k=k, Sigma=fo.Sigma.copy(), Sl=J @ fo.Sigma @ J.T, estimate=dict(q=est.pose.q, v=est.velocity, p=est.p),
                            bias=fo.inputBias.copy()))
            if len(out) == 5:
                break
    assert len(out) == 5
    return st, out


def _truth(st, f):
    t = np.array([st.vision_stamps[f]])
    p, pd, _, R, _ = synth._trajectory(t)
    R, p, pd = R[0], p[0], pd[0]
    RIC = synth._quat_to_matrix(synth.CAM_OFFSET_Q)
    body = (R.T @ (st.landmarks_world - p).T).T
    cam = (RIC.T @ (body - synth.CAM_OFFSET_X).T).T
    return dict(q=O.quat_from_matrix(R), v=R.T @ pd, p=cam)


def test_error_vector_follows_the_reference_index_map(states):
    st, out = states
    s = out[-1]
    err = consistency.local_error(s["estimate"], _truth(st, s["k"]), bias=s["bias"], true_bias=np.array([0.01] * 3 + [0.05] * 3))
    e = consistency.error_vector(err)
    assert e.shape == (11 + 3 * 30,)
    assert np.array_equal(e[0:6], err["bias"]) and np.array_equal(e[6:8], err["gravity"]) and np.array_equal(e[8:11], err["velocity"])
    for i in range(30):
        assert np.array_equal(e[11 + 3 * i: 14 + 3 * i], err["lm"][i])
    e5 = consistency.error_vector(err, with_bias=False)
    assert np.all(e5[0:6] == 0.0) and np.array_equal(e5[6:], e[6:])


@pytest.mark.parametrize("first", [0, 6, 11])
def test_nees_joint_against_solve_and_slogdet(states, first):
    st, out = states
    rng = np.random.default_rng(1)
    for s in out:
        for S in (s["Sigma"], s["Sl"]):
            A = np.tril(S[first:, first:])
            A = A + np.tril(A, -1).T  # (the lower triangle is what is factored)
            err = consistency.local_error(s["estimate"], _truth(st, s["k"]), bias=s["bias"], true_bias=np.array([0.01] * 3 + [0.05] * 3))
            E = np.vstack([consistency.error_vector(err), rng.standard_normal((3, S.shape[0])) * np.sqrt(np.diag(S))])
            got = consistency.nees_joint(S, E, first=first)
            want = np.array([e[first:] @ np.linalg.solve(A, e[first:]) for e in E])
            sign, logdet = np.linalg.slogdet(A)
            assert sign == 1.0 and got["dof"] == 11 + 3 * 30 - first
            assert np.all(np.abs(got["nees"] - want) <= 1e-10 * want), (s["k"], got["nees"], want)
            assert abs(got["logdet"] - logdet) <= 1e-10 * abs(logdet)
            L = np.linalg.cholesky(A)
            assert got["min_pivot"] == float((np.diag(L) ** 2).min())
            one = consistency.nees_joint(S, E[0], first=first)
            assert isinstance(one["nees"], float) and abs(one["nees"] - got["nees"][0]) <= 1e-12 * got["nees"][0]


def test_nees_joint_edge_cases():
    S = np.diag(np.arange(1.0, 12.0))
    r = consistency.nees_joint(S, np.ones(11), first=11)
    assert r == dict(nees=0.0, logdet=0.0, min_pivot=np.inf, dof=0)
    r = consistency.nees_joint(S, np.ones(11), first=6)
    assert abs(r["nees"] - sum(1.0 / d for d in range(7, 12))) < 1e-14 and r["min_pivot"] == pytest.approx(7.0, rel=1e-15)
    S[3, 3] = -1.0
    with pytest.raises(np.linalg.LinAlgError):
        consistency.nees_joint(S, np.ones(11))
    # only the lower triangle is read
    S = np.diag(np.arange(1.0, 12.0))
    S[0, 5] = 123.0
    assert consistency.nees_joint(S, np.ones(11))["logdet"] == consistency.nees_joint(np.diag(np.arange(1.0, 12.0)), np.ones(11))["logdet"]
