"""Helpers shared by the tests of the estimate-frame covariance and the innovation statistics (test_consistency.py, test_gpu_local.py,
test_gpu_innovation.py): the numpy oracle behind the dict interfaces of the binding, state injection into it, and reference values."""
import numpy as np

from oracle import eqf_numpy as O


def numpy_settings(d):
    dd = dict(d)
    cx, cq = dd.pop("cameraOffset_x"), dd.pop("cameraOffset_q")
    s = O.Settings(**dd)
    s.cameraOffset = O.SE3(np.asarray(cq, dtype=float), np.asarray(cx, dtype=float))
    return s


def numpy_filter(d):
    return O.VIOFilter(numpy_settings(d))


def np_imu(fo, r):
    fo.processIMUData(O.IMUVelocity(r[0], r[1:4], r[4:7]))


def inject(fo, snap):
    """A FilterBatch.dump_state() snapshot into a numpy VIOFilter."""
    o, g = snap["origin"], snap["group"]
    ids = np.asarray(snap["ids"], dtype=np.int64)
    N = len(ids)
    fo.xi0.pose = O.SE3(np.array(o["q"], dtype=float), np.array(o["x"], dtype=float))
    fo.xi0.velocity = np.array(o["v"], dtype=float)
    fo.xi0.p = np.array(o["p"], dtype=float).reshape(N, 3)
    fo.xi0.ids = ids.copy()
    fo.X = O.VIOGroup(O.SE3(np.array(g["Aq"], dtype=float), np.array(g["Ax"], dtype=float)), np.array(g["w"], dtype=float),
                      [O.SOT3(np.array(g["Qq"][i], dtype=float), float(g["Qa"][i])) for i in range(N)], ids.copy())
    fo.inputBias = np.array(snap["bias"], dtype=float)
    fo.Sigma = np.array(snap["sigma"], dtype=float)
    fo.currentTime = float(snap["time"])
    cv, av = snap["currentVelocity"], snap["accumulatedVelocity"]
    fo.currentVelocity = O.IMUVelocity(0.0, cv[0:3], cv[3:6])
    fo.accumulatedVelocity = O.IMUVelocity(0.0, av[0:3], av[3:6])
    fo.accumulatedTime = float(snap["accumulatedTime"])
    fo.initialisedFlag = bool(snap["initialised"])
    return fo


def origin_group_of(fo):
    """origin / group of a numpy VIOFilter as the dicts FilterBatch.origin() / group() return."""
    N = len(fo.xi0.ids)
    origin = dict(q=fo.xi0.pose.q.copy(), x=fo.xi0.pose.x.copy(), v=fo.xi0.velocity.copy(), p=fo.xi0.p.copy())
    group = dict(Aq=fo.X.A.q.copy(), Ax=fo.X.A.x.copy(), w=fo.X.w.copy(), Qq=np.array([Q.q for Q in fo.X.Q]).reshape(N, 4),
                 Qa=np.array([Q.a for Q in fo.X.Q]).reshape(N))
    return origin, group


def state_of_dicts(origin, group, ids):
    """(xi0, X) of the numpy oracle from the binding's dicts."""
    N = len(ids)
    xi0 = O.VIOState(O.SE3(np.array(origin["q"]), np.array(origin["x"])), origin["v"], np.array(origin["p"]).reshape(N, 3), ids)
    X = O.VIOGroup(O.SE3(np.array(group["Aq"]), np.array(group["Ax"])), group["w"],
                   [O.SOT3(np.array(group["Qq"][i], dtype=float), float(group["Qa"][i])) for i in range(N)], ids)
    return xi0, X


def chart_jacobian_blocks_oracle(origin, group, ids):
    """The J blocks from the ORACLE's chart functions (the formulas of include/eqf_vio_amd.h: eqf_get_sigma_local) -> dense J."""
    xi0, X = state_of_dicts(origin, group, ids)
    N = len(ids)
    RAt = O.quat_to_matrix(O.quat_inverse(X.A.q))
    eta0 = O.project_to_manifold(xi0).gravityDir
    etaHat = O.quat_rotate(O.quat_inverse(X.A.q), eta0)
    G = O.stereo_sphere_chart_diff(etaHat, etaHat) @ RAt @ O.stereo_sphere_chart_inv_diff(np.zeros(2), eta0)
    J = np.zeros((11 + 3 * N, 11 + 3 * N))
    J[0:6, 0:6] = np.eye(6)
    J[6:8, 6:8] = G
    J[8:11, 8:11] = RAt
    for i in range(N):
        J[11 + 3 * i: 14 + 3 * i, 11 + 3 * i: 14 + 3 * i] = O.quat_to_matrix(X.Q[i].q).T / X.Q[i].a
    return J


def fd_jacobian(xi0, X, h=1e-6):
    """Central finite differences of eps -> chart_xiHat(phi_X(chart_xi0^-1(eps))) at 0, (5 + 3N) square (no bias coordinates)."""
    m0 = O.project_to_manifold(xi0)
    mHat = O.project_to_manifold(O.state_group_action(X, xi0))
    n = 5 + 3 * len(xi0.ids)

    def f(eps):
        return O.euclid_coordinate_chart(O.state_group_action(X, O.euclid_coordinate_chart_inv(eps, m0)), mHat)

    J = np.zeros((n, n))
    for k in range(n):
        e = np.zeros(n)
        e[k] = h
        J[:, k] = (f(e) - f(-e)) / (2 * h)
    return J


def lower_cholesky(S):
    """Cholesky factor from the LOWER triangle of S only (what the device's chain reads; the oracle's S is not exactly symmetric)."""
    L = np.tril(S)
    return np.linalg.cholesky(L + np.tril(S, -1).T)


def innovation_reference(S, delta):
    """nis, logdet_S, nis_lm and the condition numbers of S and of its 2 x 2 diagonal blocks, from the oracle's S and delta."""
    L = lower_cholesky(S)
    z = np.linalg.solve(L, delta)
    N = len(delta) // 2
    nis_lm, kap_lm = np.zeros(N), np.zeros(N)
    for i in range(N):
        Sii = S[2 * i: 2 * i + 2, 2 * i: 2 * i + 2]
        Li = lower_cholesky(Sii)
        w = np.linalg.solve(Li, delta[2 * i: 2 * i + 2])
        nis_lm[i] = w @ w
        kap_lm[i] = np.linalg.cond(Sii)
    return dict(nis=float(z @ z), logdet_S=float(2 * np.log(np.diag(L)).sum()), nis_lm=nis_lm, kappa=float(np.linalg.cond(S)), kappa_lm=kap_lm,
                m=len(delta))
