"""eqf_vio_amd/consistency.py (pure numpy) against the numpy oracle: the block-diagonal map J between the covariance's coordinates (around
the origin xi0, VIOFilter.cpp:306-309) and the coordinates of the estimate, by finite differences of the oracle's own chart functions,
and the marginal NEES against the direct expression on J Sigma J^T."""
import numpy as np

from consistency_helpers import chart_jacobian_blocks_oracle, fd_jacobian, np_imu, numpy_filter, origin_group_of
from eqf_vio_amd import consistency, synth
from oracle import eqf_numpy as O


def _states_after_vision_frames(N, frames, duration):
    st = synth.make_stream(N, duration=duration)
    fo = numpy_filter(synth.template_settings_dict())
    out = []
    for kind, k in st.events():
        if kind == "imu":
            np_imu(fo, st.imu[k])
        else:
            fo.processVisionData(st.vision_stamps[k], st.ids, st.bearings[k])
            out.append((k, fo.xi0.copy(), fo.X.copy(), fo.Sigma.copy(), fo.inputBias.copy()))
            if len(out) == frames:
                break
    assert len(out) == frames
    return st, fo, out


def test_local_jacobian_blocks_against_finite_differences_of_the_oracle_charts():
    """The numpy oracle's state after each of the first 8 vision frames of the N = 30 stream.  Off-block part of the finite-difference
    Jacobian exactly 0; blocks within 1e-7 absolute (h = 1e-6 measures 2.9e-11 .. 7.7e-10 here for |J| <= 6.8: the factor 100 covers other
    seeds and the u / h rounding term)."""
    N = 30
    _, fo, states = _states_after_vision_frames(N, 8, 0.45)
    worst = 0.0
    for k, xi0, X, _, _ in states:
        fo.xi0, fo.X = xi0, X
        origin, group = origin_group_of(fo)
        blk = consistency.local_jacobian_blocks(origin, group)
        J = consistency.jacobian_matrix(blk)[6:, 6:]
        Jfd = fd_jacobian(xi0, X)
        mask = np.zeros_like(J, dtype=bool)
        mask[0:2, 0:2] = True
        mask[2:5, 2:5] = True
        for i in range(N):
            mask[5 + 3 * i: 8 + 3 * i, 5 + 3 * i: 8 + 3 * i] = True
        assert np.all(Jfd[~mask] == 0.0), k
        assert np.all(J[~mask] == 0.0), k
        err = float(np.abs(J - Jfd)[mask].max())
        worst = max(worst, err)
        print(f"frame {k}: |J|max {np.abs(J).max():.3f}, |J - J_fd|max {err:.2e}")
        assert err <= 1e-7, (k, err)
        # the same blocks from the oracle's chart functions
        assert np.abs(consistency.jacobian_matrix(blk) - chart_jacobian_blocks_oracle(origin, group, fo.xi0.ids)).max() < 1e-14
    print(f"worst |J - J_fd| {worst:.2e}")


def _truth(st, f):
    """The stream's analytic truth at vision frame f as a state dict (body velocity, camera-frame landmarks)."""
    t = np.array([st.vision_stamps[f]])
    p, pd, _, R, _ = synth._trajectory(t)
    R, p, pd = R[0], p[0], pd[0]
    RIC = synth._quat_to_matrix(synth.CAM_OFFSET_Q)
    body = (R.T @ (st.landmarks_world - p).T).T
    cam = (RIC.T @ (body - synth.CAM_OFFSET_X).T).T
    return dict(q=O.quat_from_matrix(R), v=R.T @ pd, p=cam)


def test_nees_marginal_and_local_error_against_the_direct_expression():
    """nees_marginal(local_error(...)) from the marginal blocks against e^T (J Sigma J^T)_block^-1 e formed directly with the oracle's chart
    functions: the same arithmetic in another order, 1e-12 relative."""
    N = 30
    st, fo, states = _states_after_vision_frames(N, 8, 0.45)
    for k, xi0, X, Sigma, bias in states[1:]:
        fo.xi0, fo.X = xi0, X
        origin, group = origin_group_of(fo)
        J = consistency.jacobian_matrix(consistency.local_jacobian_blocks(origin, group))
        Sl = J @ Sigma @ J.T
        est = O.state_group_action(X, xi0)
        estimate = dict(q=est.pose.q, v=est.velocity, p=est.p)
        truth = _truth(st, k)
        true_bias = np.array([0.01] * 3 + [0.05] * 3)
        marg = dict(base=Sl[:11, :11].copy(), lm=np.array([Sl[11 + 3 * i: 14 + 3 * i, 11 + 3 * i: 14 + 3 * i] for i in range(N)]))
        err = consistency.local_error(estimate, truth, bias=bias, true_bias=true_bias)
        got = consistency.nees_marginal(marg, err)
        got5 = consistency.nees_marginal(marg, err, with_bias=False)
        # direct
        etaHat = O.quat_rotate(O.quat_inverse(est.pose.q), O.E3)
        eta = O.quat_rotate(O.quat_inverse(truth["q"]), O.E3)
        e = np.concatenate([true_bias - bias, O.stereo_sphere_chart(eta, etaHat), truth["v"] - est.velocity])
        want = float(e @ np.linalg.solve(Sl[:11, :11], e))
        want5 = float(e[6:] @ np.linalg.solve(Sl[6:11, 6:11], e[6:]))
        assert got["nav_dof"] == 11 and got5["nav_dof"] == 5 and got["lm_dof"] == 3
        assert abs(got["nav"] - want) <= 1e-12 * abs(want), (k, got["nav"], want)
        assert abs(got5["nav"] - want5) <= 1e-12 * abs(want5), (k, got5["nav"], want5)
        for i in range(N):
            el = truth["p"][i] - est.p[i]
            w = float(el @ np.linalg.solve(Sl[11 + 3 * i: 14 + 3 * i, 11 + 3 * i: 14 + 3 * i], el))
            assert abs(got["lm"][i] - w) <= 1e-12 * abs(w), (k, i)
        print(f"frame {k}: NEES nav/11 {got['nav'] / 11:.3g}, nav/5 {got5['nav'] / 5:.3g}, landmarks/3 mean {got['lm'].mean() / 3:.3g}")
