"""TEST INFRASTRUCTURE ONLY -- the cases tests/test_lift_exact.py (CPU) and tests/test_gpu_lift.py (MI355X) share for the innovation lift of
eqf_update_linear / eqf_update_landmarks / eqf_apply_increment (csrc/eqf_lift.hpp), so that every bound is checked on the CPU for exactly the
cases the device is held to.

The state is consistency_cases.local_state (theta = 0.5): A turned by 2.5 rad, Q_i random rotations of up to pi - 0.1 and scales log-uniform
in [0.05, 20] (over two decades).  Sizes N = 2, 3, 19, 20, 41, 85: Sigma_e's internal order 6 + 3 N is 12, 15, 63, 66, 129, 261 -- both sides
of one, two and three 64-wide block columns of the factorisation and past the 256-stride of the tail's pivot loop.  Capacity N + 7.
Sigma is a filter's own: the fp64 oracle after five vision frames of synth.make_stream(N), so that cond(Sigma_e) is what a filter meets.
Every case (N, discrete) carries three increments:
    zupt     three unit rows on the velocity (origin chart), a residual of a few cm/s, R = 1e-4 I          -> eqf_update_linear
    stereo   2 x 3 blocks from a committed seed for min(N, 40) landmarks (every second one beyond), R_k = 1e-4 I  -> eqf_update_landmarks
    raw      gamma = 1e-2 chol(Sigma) z, z standard normal from a committed seed                            -> eqf_apply_increment
and both settings of useDiscreteInnovationLift are met at every size.  On the CPU the lift is taken of all three increments (as numpy
forms them); on the device each call forms its own gamma, which the reference then takes as its input.

THE CONSTANTS.  K_LIFT and K_STEP are MEASURED, not chosen: 4 x the largest ratio of (the fp64 numpy oracle -- oracle.eqf_numpy.bundle_lift
and its group step -- minus the 50-digit reference of lift_exact.py) to the bound forms of lift_exact.py over all cases.  The factor 4:
LAPACK's order and the kernels' 64-wide blocks with fixed trees are both O(n u) summations that differ in order, not in kind.
tests/test_lift_exact.py recomputes the oracle's ratios on every run and holds them, consistency.bundle_lift_host and (on the MI355X) the
kernels to the same K; the fault table there shows that the factor is not too loose."""
import numpy as np

import consistency_cases as cc

SIZES = (2, 3, 19, 20, 41, 85)
CASES = tuple((N, d) for N in SIZES for d in (1, 0))
INCREMENTS = ("zupt", "stereo", "raw")
RAGGED = (1, 20, 41)
THETA = cc.LOCAL_THETAS[0]
CAP_EXTRA = cc.CAP_EXTRA
FRAMES = 5
STEREO_MAX = 40
MEAS_VAR = 1e-4

# The numpy oracle's worst ratios as tests/test_lift_exact.py measures them (x86-64, OpenBLAS), per size for DeltaU and over all sizes for the
# entries of X; K = 4 x the largest, unrounded.
ORACLE_DU = {2: 2.602762746446091e-07, 3: 3.4183248669893833e-06, 19: 0.00011272465897361609, 20: 8.343960077492135e-05,
             41: 0.00012694052890302752, 85: 4.330328474764998e-05}
ORACLE_X = {"A.R": 0.0521827737475301, "A.x": 0.07136905415955169, "w": 0.02369382928531038, "bias": 0.05738043668114245,
            "Q.R": 1.8745535652834875, "Q.a": 2.3287403146519234}
# ORACLE-END
K_LIFT = 4 * max(ORACLE_DU.values())
K_STEP = 4 * max(ORACLE_X.values())


def settings(discrete=1, lift=1):
    d = dict(cc.settings())
    d["useInnovationLift"] = bool(lift)
    d["useDiscreteInnovationLift"] = bool(discrete)
    return d


_OWN = {}


def own_sigma(N):
    """The fp64 oracle's Sigma after FRAMES vision frames of a stream of N landmarks, mirrored."""
    if N not in _OWN:
        from eqf_vio_amd import synth
        from oracle import binding as ob

        st = synth.make_stream(N, duration=0.05 * FRAMES + 0.02)
        fo = ob.OracleFilter(cc.settings())
        for kind, k in st.events():
            if kind == "imu":
                r = st.imu[k]
                fo.processIMUData(r[0], r[1:4], r[4:7])
            else:
                fo.processVisionData(st.vision_stamps[k], st.ids, st.bearings[k])
        S = fo.stateCovariance()
        assert S.shape == (11 + 3 * N,) * 2
        _OWN[N] = np.triu(S) + np.triu(S, 1).T
    return _OWN[N]


def snapshot(N):
    snap = cc.local_state(N, THETA)
    snap["sigma"] = own_sigma(N)
    return snap


def zupt(N):
    """(H (3 x n), resid (3), R (3 x 3)): unit rows on the velocity in the origin chart"""
    H = np.zeros((3, 11 + 3 * N))
    H[0, 8] = H[1, 9] = H[2, 10] = 1.0
    return H, np.array([0.03, -0.02, 0.015]), MEAS_VAR * np.eye(3)


def stereo(N, ids):
    """(ids (K), H (K, 2, 3), resid (K, 2), R (K, 2, 2)) in the origin chart; the landmark positions in the state are idx"""
    idx = np.arange(N) if N <= STEREO_MAX else np.arange(0, N, 2)[:STEREO_MAX]
    rng = np.random.default_rng([2500, N])
    H = rng.standard_normal((len(idx), 2, 3))
    r = 1e-2 * rng.standard_normal((len(idx), 2))
    return np.asarray(ids)[idx], idx, H, r, np.broadcast_to(MEAS_VAR * np.eye(2), (len(idx), 2, 2)).copy()


def raw(N, Sigma):
    return 1e-2 * (np.linalg.cholesky(Sigma) @ np.random.default_rng([2501, N]).standard_normal(len(Sigma)))


def kalman(Sigma, H, resid, R):
    """(gamma, Sigma+) of a linear update, dense numpy"""
    B = Sigma @ H.T
    S = H @ B + R
    return B @ np.linalg.solve(S, resid), Sigma - B @ np.linalg.solve(S, B.T)


def stereo_dense(N, idx, Hb, rb, Rb):
    K = len(idx)
    H = np.zeros((2 * K, 11 + 3 * N))
    R = np.zeros((2 * K, 2 * K))
    for k, i in enumerate(idx):
        H[2 * k:2 * k + 2, 11 + 3 * i:14 + 3 * i] = Hb[k]
        R[2 * k:2 * k + 2, 2 * k:2 * k + 2] = Rb[k]
    return H, rb.reshape(-1), R


def increment(N, which, snap):
    """(gamma, Sigma after the update or None) as dense numpy forms them"""
    S = snap["sigma"]
    if which == "zupt":
        return kalman(S, *zupt(N))
    if which == "stereo":
        _, idx, Hb, rb, Rb = stereo(N, snap["ids"])
        return kalman(S, *stereo_dense(N, idx, Hb, rb, Rb))
    return raw(N, S), None


def lift_state(snap, d):
    """consistency.bundle_lift_host's `state` of a snapshot under the settings d"""
    return dict(origin=snap["origin"], group=snap["group"], bias=snap["bias"], camera=dict(q=d["cameraOffset_q"], x=d["cameraOffset_x"]),
                discrete=bool(d["useDiscreteInnovationLift"]))


def oracle_state(snap, d):
    """(xi0, X) of a snapshot as the numpy oracle's objects"""
    from oracle import eqf_numpy as en

    o, g = snap["origin"], snap["group"]
    ids = list(snap["ids"])
    cam = en.SE3(d["cameraOffset_q"], d["cameraOffset_x"])
    xi0 = en.VIOState(pose=en.SE3(o["q"], o["x"]), velocity=np.array(o["v"], dtype=float), p=np.array(o["p"], dtype=float).reshape(-1, 3), ids=ids,
                      cameraOffset=cam)
    X = en.VIOGroup(en.SE3(g["Aq"], g["Ax"]), np.array(g["w"], dtype=float),
                    [en.SOT3(q, a) for q, a in zip(np.asarray(g["Qq"]).reshape(-1, 4), np.asarray(g["Qa"]).reshape(-1))], ids)
    return xi0, X


def oracle_output_blocks(snap, d):
    """C0_i (N, 2, 3): the diagonal blocks of the oracle's output matrix (EqFMatrices.cpp:319-344)"""
    from oracle import eqf_numpy as en

    N = len(snap["ids"])
    C0 = en.eqf_output_matrix_C(oracle_state(snap, d)[0])
    return np.array([C0[2 * i:2 * i + 2, 5 + 3 * i:8 + 3 * i] for i in range(N)]).reshape(N, 2, 3)


def oracle_lift(gamma, snap, Sigma, d):
    """oracle.eqf_numpy.bundle_lift and the reference's group step (VIOFilter.cpp:292-296) on a snapshot: dict(DeltaU, group, bias)"""
    from oracle import eqf_numpy as en

    xi0, X = oracle_state(snap, d)
    Gamma = en.bundle_lift(np.asarray(gamma, dtype=float)[6:], xi0, X, np.asarray(Sigma, dtype=float)[6:, 6:])
    if d["useDiscreteInnovationLift"]:
        Delta = en.lift_total_space_innovation_discrete(Gamma, xi0)
    else:
        Delta = en.vio_exp(en.lift_total_space_innovation(Gamma, xi0))
    Xn = Delta * X
    group = dict(Aq=Xn.A.q, Ax=Xn.A.x, w=Xn.w, Qq=np.array([Q.q for Q in Xn.Q]).reshape(-1, 4), Qa=np.array([Q.a for Q in Xn.Q]))
    return dict(DeltaU=Gamma[0:6], group=group, bias=np.asarray(snap["bias"], dtype=float) + np.asarray(gamma, dtype=float)[0:6])
