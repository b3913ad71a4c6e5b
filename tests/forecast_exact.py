"""TEST INFRASTRUCTURE ONLY -- the forecast (include/eqf_vio_amd.h: eqf_forecast) entry by entry: a reference and a-priori bounds, composed
from the references the project already has.  Nothing here comes from the device.

THE REFERENCE.  riccati_exact.ExactFilter walks the samples exactly as processIMUData does (a call with dt <= 0 integrates nothing and
replaces sample and time); the closing integrateUpToTime(t1) is the same step with the held sample and replaces nothing.  The group moves at
50 digits (lie_exact.group_step), Sigma in longdouble through riccati_exact.Step / reference_sigma.  From the state reached:
    pose, velocity, p    lie_exact.state_group_action;  bearing = p / |p|
    base, lm             blocks of Sigma_ref; in the estimate's chart J Sigma_ref J^T with the 50-digit J of the state REACHED
    S_i                  C0i Sigma_ref,ii C0i^T + r I, C0i = lie_exact.landmark_constants (update_exact.Geometry's)
    ycov_i               D J_i Sigma_ref,ii J_i^T D^T, D = (I - y y^T) / |p| at 50 digits, the products in longdouble

THE BOUNDS, entrywise.
    Sigma    riccati_exact.step_bound pushed through the steps as reference_run does (K_OPS, TAU_BLK as they stand).  One addition: a state
             whose gravity chart lies theta from its pole has the base blocks -T Bg and T Avg (and Bg in the noise) only to K (u / theta^2)
             scale -- lie_edge_cases.K_POLE["Bg"] (scale 1) and ["Avg"] (scale 2 g), the bound form of DESIGN.md section 5 -- which is added to
             |dF|, |dB| on those blocks; it is below TAU_BLK's share unless theta < 0.3.
             TAU: TAU_BLK was measured over states at most four steps from a snapshot.  tests/test_forecast_exact.py measures the fp64
             oracle's blocks against the 50-digit ones at every step of every case here (17 steps included): FC_TAU_MEASURED; the bound uses
             max(TAU_BLK, 10 x FC_TAU_MEASURED) (the ten-fold margin of NOTES.md R13.1).
    state    K u (1 + magnitude) per quantity (lie_edge_cases.K_STEP, by lift and angle class), times the number of integrating steps
             (at least 1): every step adds one such error, and a step moves an earlier error by a rotation and a scale a in [0.5, 2].
    bearing  dy = (I - y y^T) dp / |p| to first order: |dy| <= 2 sqrt(3) max|dp| / |p| + 4 u (twice the first order; 4 u for the dot product,
             the root and the division).
    local    consistency_exact's form: (gamma_6 + slack) |J||S||J|^T + |dJ||S||J|^T + |J||S||dJ|^T, |dJ| = K_J u max|block| (G: u / theta^2)
             plus the drift of the group over the steps, steps x (K_STEP["A.R"] resp. K_STEP["Q.R"] + K_STEP["Q.a"]) u max|block| -- and the
             Sigma bound pushed through |J| . |J|^T.
    S        update_exact's dS: dB = gamma_3 |C||S| + dC |S|, dS = dB |C^T| + gamma_4 |B||C^T| + |B| dC^T + u |S_out|, plus |C| E |C|^T for the
             Sigma bound E.  dC = TAU u max|C0i| + K_POLE["C0"] (u / theta_i^2) / |p0_i|: a landmark theta_i from the optical axis has its
             chart's rotation R_s(-y0 -> e3) that close to the half turn, and C0i only to lie_edge_cases' pole form;
             update_cases keeps its landmarks away from the axis, the states here (30 degree cone, up to 257 landmarks) do not.
    ycov     gamma_6 |D||P||D|^T + dD |P||D|^T + |D||P| dD^T + |D| E_loc |D|^T; dD = TAU_D u max|D| + 3 sqrt(3) max|dp| / |p|^2 max-normwise (D's
             derivative along dp is at most 3 |dp| / |p|^2).  TAU_D = 10 x TAU_D_MEASURED, the worst error of the fp64 D that
             consistency.bearing_cov_host forms against the 50-digit D over every landmark of every case, in units of u max|D|."""
import numpy as np
from mpmath import mp, mpf

import consistency_cases as cc
import consistency_exact as cx
import lie_edge_cases as ec
import lie_exact as lx
import riccati_exact as rx
import update_exact as ux

LD, U = rx.LD, rx.U64
FC_TAU_MEASURED = 17.53076966726239   # (x86-64, OpenBLAS; worst on a landmark's Lv at the 18th step of case k17t) units of u max|block| over every step of forecast_cases (tests/test_forecast_exact.py prints and checks it)
TAU = max(rx.TAU_BLK, 10.0 * FC_TAU_MEASURED)
TAU_D_MEASURED = 2.8701484189513113     # units of u max|D| (tests/test_forecast_exact.py prints and checks it)
TAU_D = max(1.0, 10.0 * TAU_D_MEASURED)


def walk(snap, d, imu, t1):
    """(ExactFilter at the state reached, the Steps that integrated, the largest rotation angle of a step)."""
    f = rx.ExactFilter(snap, d)
    steps, theta = [], 0.0
    for r in np.asarray(imu, dtype=float).reshape(-1, 7):
        dt = float(r[0]) - f.time
        if f.time >= 0 and dt > 0:
            theta = max(theta, float(np.linalg.norm(f.cur[0:3])) * dt)
        s = f.process_imu(r[0], r[1:4], r[4:7])
        if s is not None:
            steps.append(s)
    if t1 is not None:
        dt = float(t1) - f.time
        if f.time >= 0 and dt > 0:
            theta = max(theta, float(np.linalg.norm(f.cur[0:3])) * dt)
            steps.append(rx.Step(rx.blocks_mp(f.X, f.xi0, f.cur[0:3], f.acc_w, f.acc_T, mpf(dt)), d))
            f.X = lx.group_step(f.X, f.xi0, f.cur[0:3], f.cur[3:6], dt, bool(d["useDiscreteVelocityLift"]))
            f.acc_w, f.acc_T = [mpf(0)] * 3, mpf(0)
            f.time = float(t1)
    return f, steps, theta


def pole_angle(xi0):
    eta0 = lx.mv(lx.tr(xi0.R), lx.E3())
    return float(mp.atan2(mp.sqrt(eta0[0] ** 2 + eta0[1] ** 2), eta0[2]))


def step_bound(step, S_abs, theta0, tau):
    """riccati_exact.step_bound (fp64) with the pole allowance of the module docstring on the blocks built from the gravity chart."""
    aF, aB = rx._absF(step.F), np.abs(step.Bt)
    dF, dB = step.block_errors(tau, U, 0.0)
    T = float(step.T)
    pole = U / theta0 ** 2
    dF[0][6:8, 0:3] += T * ec.K_POLE["Bg"] * pole
    dF[0][8:11, 6:8] += T * ec.K_POLE["Avg"] * pole * 2 * 9.81
    dB[6:8, 0:3] += ec.K_POLE["Bg"] * pole
    S_abs = np.asarray(S_abs).astype(LD)
    main = rx.sandwich(aF, S_abs, aF)
    E = rx.gamma(rx.K_OPS, U) * (main + np.abs(rx.noise(step)))
    Y = rx.sandwich(dF, S_abs, aF)
    E += Y + Y.T + rx.sandwich(dF, S_abs, dF)
    Z = (dB * step.R) @ aB.T
    E += step.T * (Z + Z.T + (dB * step.R) @ dB.T)
    return E


def run_sigma(steps, S0, theta0, tau=None):
    """riccati_exact.reference_run with step_bound above."""
    tau = TAU if tau is None else tau
    S = np.asarray(S0).astype(LD)
    e = np.zeros_like(S)
    for st in steps:
        aF = rx._absF(st.F)
        e = rx.sandwich(aF, e, aF) + step_bound(st, np.abs(S) + e, theta0, tau)
        S = rx.reference_sigma(st, S)
    return S, e


def jacobian_of(X, xi0):
    """consistency_exact.jacobian_mp's dictionary from a 50-digit state (lie_exact.Group / State) instead of the binding's doubles."""
    RAt = lx.tr(X.AR)
    eta0 = lx.mv(lx.tr(xi0.R), lx.E3())
    etaHat = lx.mv(RAt, eta0)
    G = lx.mm(lx.mm(lx.chart_diff(etaHat, etaHat), RAt), lx.chart_inv_diff_at_zero(eta0))
    ang = lambda e: float(mp.atan2(mp.sqrt(e[0] ** 2 + e[1] ** 2), e[2]))  # noqa: E731
    return dict(G=G, RAt=RAt, lm=[lx.mscl(1 / a, lx.tr(RQ)) for RQ, a in X.Q], theta0=ang(eta0), thetaHat=ang(etaHat))


def _mx(A):
    return float(max(abs(x) for r in A for x in r))


def blocks_of(S, N):
    return np.array([S[11 + 3 * i:14 + 3 * i, 11 + 3 * i:14 + 3 * i] for i in range(N)]).reshape(N, 3, 3)


class Reference:
    """Everything eqf_forecast returns for one filter, with its bound: ref[name], bound[name] (longdouble / float64 arrays), `steps`, `time`."""

    def __init__(self, snap, d, imu, t1, local, tau=None):
        f, steps, theta = walk(snap, d, imu, t1)
        N = self.N = len(snap["ids"])
        n_int = self.steps = len(steps)
        self.time = f.time
        m = max(1, n_int)
        K = ec.K_STEP[bool(d["useDiscreteVelocityLift"])][ec.angle_class(theta)]
        est = lx.state_group_action(f.X, f.xi0)
        ref, bound = {}, {}
        self.ref, self.bound = ref, bound
        self.est = est
        ref["pose_R"], bound["pose_R"] = cx.ldm(est.R), np.full((3, 3), m * K["est.R"] * U * (1 + _mx(est.R)))
        for name, v, k in (("pose_x", est.x, "est.x"), ("velocity", est.v, "est.v")):
            ref[name], bound[name] = np.array([cx.ld(x) for x in v], dtype=LD), np.full(3, m * K[k] * U * (1 + float(max(abs(x) for x in v))))
        p = np.array([[cx.ld(x) for x in q] for q in est.p], dtype=LD).reshape(N, 3)
        dp = np.array([m * K["est.p"] * U * (1 + float(max(abs(x) for x in q))) for q in est.p]).reshape(N)
        ref["p"], bound["p"] = p, np.repeat(dp[:, None], 3, axis=1)
        nrm = [lx.norm(q) for q in est.p]
        ref["bearing"] = np.array([[cx.ld(x / nr) for x in q] for q, nr in zip(est.p, nrm)], dtype=LD).reshape(N, 3)
        bound["bearing"] = np.repeat((2 * np.sqrt(3.0) * dp / np.array([float(x) for x in nrm]).reshape(N) + 4 * U)[:, None], 3, axis=1)
        # ---- Sigma
        theta0 = pole_angle(f.xi0)
        S, E = run_sigma(steps, snap["sigma"], theta0, tau)
        self.S, self.E = S, E
        Jmp = self.Jmp = jacobian_of(f.X, f.xi0)
        Jb, Jl = cx.jacobian_ld(Jmp, N)
        Ab, Al = np.abs(Jb).astype(np.float64), np.abs(Jl).astype(np.float64)
        Db, Dl = cx.jacobian_tol(Jmp, cc.K_J, N)
        th = min(Jmp["theta0"], Jmp["thetaHat"], 1.0)
        Db[6:8, 6:8] += m * K["A.R"] * U / th ** 2 * _mx(Jmp["G"])
        Db[8:11, 8:11] += m * K["A.R"] * U * _mx(Jmp["RAt"])
        for i in range(N):
            Dl[i] += m * (K["Q.R"] + K["Q.a"]) * U * _mx(Jmp["lm"][i])
        aS = (np.abs(S) + E).astype(np.float64)
        Ef = E.astype(np.float64)
        Sloc = cx.bd_sandwich(Jb, Jl, S, Jb, Jl)
        core = cx.bd_sandwich(Ab, Al, aS, Ab, Al)
        Eloc = ((rx.gamma(cx.K_LOCAL, U) + cx.REF_SLACK) * core + cx.bd_sandwich(Db, Dl, aS, Ab, Al) + cx.bd_sandwich(Ab, Al, aS, Db, Dl)
                + cx.bd_sandwich(Db, Dl, aS, Db, Dl) + cx.bd_sandwich(Ab, Al, Ef, Ab, Al))
        self.Sloc, self.Eloc = Sloc, Eloc
        ref["base"], bound["base"] = (Sloc[:11, :11], Eloc[:11, :11]) if local else (S[:11, :11], Ef[:11, :11])
        ref["lm"], bound["lm"] = (blocks_of(Sloc, N), blocks_of(Eloc, N)) if local else (blocks_of(S, N), blocks_of(Ef, N))
        # ---- S_i = C0i Sigma_ii C0i^T + r I
        r = LD(d["measurementVariance"])
        tau_c = TAU if tau is None else tau
        Sii, Eii = blocks_of(S, N), blocks_of(Ef, N)
        ref["S"], bound["S"] = np.zeros((N, 2, 2), dtype=LD), np.zeros((N, 2, 2))
        for i in range(N):
            C = cx.ldm(lx.landmark_constants([float(v) for v in f.xi0.p[i]])[0])
            aC = np.abs(C).astype(np.float64)
            a = (np.abs(Sii[i]) + Eii[i]).astype(np.float64)
            p0 = [float(v) for v in f.xi0.p[i]]
            th_i = float(np.arctan2(np.hypot(p0[0], p0[1]), p0[2]))  # the landmark's angle from e3, the pole of ITS chart (R_s(-y0 -> e3))
            dC = np.full((2, 3), tau_c * U * aC.max() + ec.K_POLE["C0"] * U / th_i ** 2 / float(np.linalg.norm(p0)))
            ref["S"][i] = C @ Sii[i] @ C.T + r * np.eye(2, dtype=LD)
            dB = rx.gamma(ux.OPS_C, U) * (aC @ a) + dC @ a
            bound["S"][i] = (dB @ aC.T + rx.gamma(ux.OPS_S, U) * ((aC @ a) @ aC.T) + (aC @ a) @ dC.T + U * np.abs(ref["S"][i]).astype(np.float64)
                             + aC @ Eii[i] @ aC.T)
        # ---- ycov_i = D Sigma_loc,ii D^T
        Pl, El = blocks_of(Sloc, N), blocks_of(Eloc, N)
        ref["ycov"], bound["ycov"] = np.zeros((N, 3, 3), dtype=LD), np.zeros((N, 3, 3))
        self.D = []
        for i in range(N):
            y = [x / nrm[i] for x in est.p[i]]
            Dmp = lx.mscl(1 / nrm[i], lx.madd(lx.eye(), lx.mscl(mpf(-1), lx.outer(y, y))))
            self.D.append(Dmp)
            D = cx.ldm(Dmp)
            aD = np.abs(D).astype(np.float64)
            a = (np.abs(Pl[i]) + El[i]).astype(np.float64)
            dD = np.full((3, 3), TAU_D * U * aD.max() + 3 * np.sqrt(3.0) * dp[i] / float(nrm[i]) ** 2)
            ref["ycov"][i] = D @ Pl[i] @ D.T
            bound["ycov"][i] = (rx.gamma(6, U) * (aD @ a @ aD.T) + dD @ a @ aD.T + aD @ a @ dD.T + dD @ a @ dD.T
                                + aD @ El[i].astype(np.float64) @ aD.T)


def rotation_of(q):
    """quaternion (w, x, y, z) of doubles -> its matrix, exact to 50 digits then rounded"""
    return lx.to_np(lx.rot_of_quat(q))


def ratios(got, R, names=("pose_R", "pose_x", "velocity", "p", "bearing", "base", "lm", "S", "ycov")):
    """{name: worst |got - ref| / bound}: got is one filter's part of FilterBatch.forecast's / consistency.forecast_host's dictionary (pose_q
    is compared through its matrix).  An entry whose bound is 0 must be exact."""
    out = {}
    for k in names:
        g = rotation_of(got["pose_q"]) if k == "pose_R" else np.asarray(got[k], dtype=float)
        ref, b = R.ref[k], np.asarray(R.bound[k], dtype=LD)
        if ref.size == 0:
            out[k] = 0.0
            continue
        err = np.abs(g.astype(LD).reshape(ref.shape) - ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0, LD(0), err / b)
        out[k] = float(np.max(q)) if np.all(np.isfinite(g)) else np.inf
    return out
