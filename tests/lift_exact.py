"""TEST INFRASTRUCTURE ONLY -- the innovation lift of eqf_update_linear / eqf_update_landmarks / eqf_apply_increment (csrc/eqf_lift.hpp;
include/eqf_vio_amd.h: eqf_get_lift_report) from its DEFINITION, the reference's bundleLift (EqFMatrices.cpp:173-252), in mpmath at 50
digits; the Lie maps come from tests/lie_exact.py.  Nothing of oracle/ and nothing of the product is imported.

THE REFERENCE (reference()).  gamma (the increment, exact doubles), the snapshot's origin / group / bias (exact doubles) and the Sigma the
call started from (exact doubles) are the inputs.  With xiHat = X acting on xi0, eta0 the unit gravity direction of xi0, R_C = R_Phat R_IC,
PC = Phat T_IC and Ad the adjoint of xi0's pose:
    dU0 = (-eta0 x cInv g2 ; 0)         K_par = [(eta0;0) | (0;I3)]        dU_f = ((I - eta0 eta0^T) dU0_w ; 0)
    per landmark   pHat_i = PC xiHat.p_i    alpha_i = -R_C Q_i^-1 gamma_i    P_i = [-pHat_i^x, I]
                   obs_i = alpha_i - P_i Ad dU_f        C_i = P_i Ad K_par        D_i = Q_i.asMatrix R_C^T   (rows 5 + 3 i .. of D)
    W = D^T Sigma_e^-1 D        x = (C^T W C)^-1 C^T W obs        DeltaU = dU_f + K_par x
This is the definition's form, NOT the kernels' (Z_P = D C-with-Ad folded in, h, the seven right-hand sides): the two must agree because
D alpha = -[0; gamma_L], which is what the test then shows.  Sigma_e^-1 is applied exactly: Sigma_e = L L^T at 50 digits and
W-products as (L^-1 D C)^T (L^-1 D .), which is D^T Sigma_e^-1 D to the working precision (a 50-digit inverse of a matrix of condition
1e12 keeps 38 digits; so does this) at a sixtieth of the operations for N = 85.
Then Delta = lie_exact.innovation_element(xi0, DeltaU, gamma_v, gamma_L, "discrete" | "continuous"), X+ = Delta X, bias+ = bias + gamma[0:6].

THE BOUND.  u = 2^-53, n = 5 + 3 N, kS = cond_2(Sigma_e), kM = cond_2(K_par^T G6 K_par):
    |d DeltaU|_max <= K_LIFT u n kS kM max(|DeltaU|_max, |dU_f|_max, TINY)                                            (bound_dU)
        the solved rows L^-1 [Z_P | g] carry a relative error n u kS at the most [Higham, Thm 8.5 with Thm 10.3], G6 and h are sums of n
        products of them, and the 4 x 4 solve multiplies a relative perturbation of its matrix and right-hand side by kM.
    |d entry of X+| <= K_STEP (bound_dU (1 + |x0| + |v0| + |A.x|) + u (1 + magnitude))                                (bound_X)
        A+ = exp(DeltaU) A and w+ depend on DeltaU with derivatives bounded by the lengths named; the landmark part and the bias do not depend
        on DeltaU at all (bound_dU drops out: u (1 + magnitude) alone).
K_LIFT and K_STEP are measured on the numpy oracle, never on the code under test: lift_cases.py."""
import numpy as np
from mpmath import mp, mpf

import lie_exact as lx
import update_exact as ux

mp.dps = 50
U = 2.0 ** -53
TINY = 1e-300


def _obj(A):
    A = np.asarray(A, dtype=float)
    return np.array([mpf(float(v)) for v in A.reshape(-1)], dtype=object).reshape(A.shape)


def _mpmat(rows):
    return np.array([[x for x in r] for r in rows], dtype=object)


def pieces(gamma, origin, group, camq, camx, faults=()):
    """(dUf, Kpar, C (3N x 4), obs (3N), D (n x 3N)) of the definition, object arrays of mpf.  faults: see FAULTS."""
    xi0 = lx.State.from_dict(origin, camq, camx)
    X = lx.Group.from_dict(group)
    est = lx.state_group_action(X, xi0)
    N = len(xi0.p)
    ge = [mpf(float(v)) for v in np.asarray(gamma, dtype=float)[6:]]
    eta0, _, ci = lx.pose_constants(xi0.R)
    eta0 = lx.unit(eta0)
    g2 = ge[0:2]
    dUw = lx.scl(-1, lx.cross(eta0, [ci[i][0] * g2[0] + ci[i][1] * g2[1] for i in range(3)]))
    proj = lx.sub(dUw, lx.scl(lx.dot(eta0, dUw), eta0))
    # no_projection: K_perp left out, and with it a component along eta0 let in (here as long as dUw itself).  INERT by construction:
    # dUw = -eta0 x t has no such component in the first place, and any that dU_f carried is a multiple of K_par's first column, which the
    # least squares takes back out through x[0].  The table keeps it to show exactly that.
    if "no_projection" in faults:
        proj = lx.add(dUw, lx.scl(lx.norm(dUw), eta0))
    dUf = proj + [mpf(0)] * 3
    Kpar = np.array([[mpf(0)] * 4 for _ in range(6)], dtype=object)
    for i in range(3):
        Kpar[i, 0] = eta0[i]
        Kpar[3 + i, 1 + i] = mpf(1)
    RC = lx.mm(est.R, est.camR)
    PC = lx.se3_mul((est.R, est.x), (est.camR, est.camx))
    n = 5 + 3 * N
    C = np.array([[mpf(0)] * 4 for _ in range(3 * N)], dtype=object)
    obs = np.array([mpf(0)] * (3 * N), dtype=object)
    D = np.array([[mpf(0)] * (3 * N) for _ in range(n)], dtype=object)

    def P_Ad(pHat, u6):  # [-pHat^x, I] Ad_P0 u
        w, v = lx.se3_adjoint_apply((xi0.R, xi0.x), list(u6[0:3]), list(u6[3:6]))
        return lx.add(lx.scl(-1, lx.cross(pHat, w)), v)

    for i in range(N):
        g = ge[5 + 3 * i:8 + 3 * i]
        pHat = lx.se3_apply(PC, est.p[i])
        alpha = lx.scl(-1, lx.mv(RC, lx.sot3_apply_inv(X.Q[i], g)))
        o = alpha if "dUf_dropped" in faults else lx.sub(alpha, P_Ad(pHat, dUf))   # (the G6 dU_f term of the right-hand side left out)
        for r in range(3):
            obs[3 * i + r] = o[r]
        for c in range(4):
            col = P_Ad(pHat, list(Kpar[:, c]))
            for r in range(3):
                C[3 * i + r, c] = col[r]
        QR, Qa = X.Q[i]
        scale = mpf(1) if ("unit_scale" in faults and i == N - 1) else Qa
        Dm = lx.mscl(scale, lx.mm(QR, lx.tr(RC)))
        for r in range(3):
            for c in range(3):
                D[5 + 3 * i + r, 3 * i + c] = Dm[r][c]
    return dUf, Kpar, C, obs, D, xi0, X


_CHOL = {}


def _chol(Se):
    """the 50-digit factor of Sigma_e, computed once per matrix (the increments and calls of a case share it)"""
    key = hash(np.ascontiguousarray(Se).tobytes())
    if key not in _CHOL:
        _CHOL[key] = ux.chol(_obj(Se), mp.sqrt)
    return _CHOL[key]


def reference(gamma, snap, Sigma, camq, camx, discrete, faults=()):
    """The lift from its definition.  Returns a dict: DeltaU (6 mpf), X (lie_exact.Group after the step), bias (6 mpf), dUf, and the
    doubles kS = cond_2(Sigma_e), kM = cond_2 of the 4 x 4 matrix, n."""
    gamma = np.asarray(gamma, dtype=float)
    dUf, Kpar, C, obs, D, xi0, X = pieces(gamma, snap["origin"], snap["group"], camq, camx, faults)
    Se = np.asarray(Sigma, dtype=float)[6:, 6:]
    L = _chol(Se)
    DC = D @ C                       # n x 4
    Do = D @ obs                     # n
    if "gamma_e_rhs" in faults:      # gamma_e where [0; gamma_L] belongs (D obs = -[0; gamma_L] - Z_P dU_f: the top five rows are zero)
        for k in range(5):
            Do[k] = Do[k] - mpf(float(gamma[6 + k]))
    if "top_rows" in faults:         # the top five rows of Z_P not zeroed
        for k in range(5):
            for c in range(4):
                DC[k, c] = mpf(1)
    Zt = ux.solve_lower(L, DC)
    zo = ux.solve_lower(L, Do)
    M = Zt.T @ Zt
    rhs = Zt.T @ zo
    if "sign_h" in faults:           # h with the wrong sign: rhs = -h - G6 dU_f  ->  +h - G6 dU_f
        zg = ux.solve_lower(L, np.array([mpf(0)] * 5 + [mpf(float(v)) for v in gamma[11:]], dtype=object))
        rhs = rhs + 2 * (Zt.T @ zg)
    x = ux.solve4(M, rhs)
    dU = [dUf[i] + sum(Kpar[i, c] * x[c] for c in range(4)) for i in range(6)]
    gv = gamma[8:11]
    gq = gamma[11:].reshape(-1, 3)
    mode = "discrete" if discrete else "continuous"
    Delta = lx.innovation_element(xi0, dU, gv, gq, mode)
    if "continuous_w" in faults:     # the continuous velocity term inside the discrete lift
        Delta.w = lx.sub(lx.scl(-1, lx.vec(gv)), lx.cross(dU[0:3], xi0.v))
    Xn = Delta * X
    bias = [mpf(float(snap["bias"][i])) + mpf(float(gamma[i])) for i in range(6)]
    Mf = np.array([[float(v) for v in row] for row in M])
    return dict(DeltaU=dU, X=Xn, bias=bias, dUf=dUf, kS=float(np.linalg.cond(Se)), kM=float(np.linalg.cond(Mf)), n=len(Se),
                lens=1.0 + float(np.linalg.norm(snap["origin"]["x"])) + float(np.linalg.norm(snap["origin"]["v"]))
                + float(np.linalg.norm(snap["group"]["Ax"])))


# ---- the bound forms ---------------------------------------------------------------------------------------------------------------------------
def form_dU(ref):
    """u n kS kM max(|DeltaU|, |dU_f|, TINY): bound_dU / K_LIFT"""
    mag = max(max(abs(float(v)) for v in ref["DeltaU"]), max(abs(float(v)) for v in ref["dUf"]), TINY)
    return U * ref["n"] * ref["kS"] * ref["kM"] * mag


def err_dU(dU, ref):
    return max(abs(mpf(float(dU[i])) - ref["DeltaU"][i]) for i in range(6))


def ratio_dU(dU, ref):
    return float(err_dU(dU, ref) / mpf(form_dU(ref)))


def _quat_R(q):
    return lx.rot_of_quat(q)


def ratios_X(group, bias, ref, k_lift):
    """The entries of X+ and of the bias against the reference, as ratios to the bound form (bound_X / K_STEP) with bound_dU = k_lift x
    form_dU: {"A.R", "A.x", "w", "Q.R", "Q.a", "bias"}"""
    bd = k_lift * form_dU(ref) * ref["lens"]
    X = ref["X"]

    def r(got, want, with_dU):
        w = want if isinstance(want[0], list) else [want]
        g = [[mpf(float(v)) for v in row] for row in (got if isinstance(want[0], list) else [got])]
        err = max(abs(g[i][j] - w[i][j]) for i in range(len(w)) for j in range(len(w[0])))
        mag = max(abs(v) for row in w for v in row)
        return float(err / ((mpf(bd) if with_dU else 0) + mpf(U) * (1 + mag)))

    out = {"A.R": r(_quat_R(group["Aq"]), X.AR, True), "A.x": r(list(group["Ax"]), X.Ax, True), "w": r(list(group["w"]), X.w, True),
           "bias": r(list(bias), ref["bias"], False), "Q.R": 0.0, "Q.a": 0.0}
    Qq, Qa = np.asarray(group["Qq"]).reshape(-1, 4), np.asarray(group["Qa"]).reshape(-1)
    for i, Q in enumerate(X.Q):
        out["Q.R"] = max(out["Q.R"], r(_quat_R(Qq[i]), Q[0], False))
        out["Q.a"] = max(out["Q.a"], r([Qa[i]], [Q[1]], False))
    return out


# ---- injected faults: each is a wrong lift somebody could write; every one must leave the bound -----------------------------------------------
FAULTS = ("post_sigma", "dUf_dropped", "top_rows", "gamma_e_rhs", "sign_h", "continuous_w", "unit_scale", "pad_column")
INERT = ("no_projection",)   # mathematically without effect (see pieces()): must stay INSIDE the bound


def faulty(name, gamma, snap, Sigma, Sigma_post, camq, camx, discrete):
    """The reference with one fault.  post_sigma: Sigma after the update's downdate; pad_column: the pad's column of the solved rows summed
    into G6 and h."""
    if name == "post_sigma":
        return reference(gamma, snap, Sigma_post, camq, camx, discrete)
    if name == "pad_column":
        return _with_pad(gamma, snap, Sigma, camq, camx, discrete)
    return reference(gamma, snap, Sigma, camq, camx, discrete, faults=(name,))


def _with_pad(gamma, snap, Sigma, camq, camx, discrete):
    gamma = np.asarray(gamma, dtype=float)
    dUf, Kpar, C, obs, D, xi0, X = pieces(gamma, snap["origin"], snap["group"], camq, camx)
    L = _chol(np.asarray(Sigma, dtype=float)[6:, 6:])
    # the solved rows have one more column, the pad's, which the factorisation treats as a row of the identity: what lies there is whatever
    # the right-hand side's memory held (here 1 in every row), and a tail that sums over it adds its products to G6 and h
    one = np.array([[mpf(1)] * 4], dtype=object)
    Zt = np.concatenate([ux.solve_lower(L, D @ C), one], axis=0)
    zo = np.concatenate([ux.solve_lower(L, D @ obs), np.array([mpf(1)], dtype=object)])
    x = ux.solve4(Zt.T @ Zt, Zt.T @ zo)
    dU = [dUf[i] + sum(Kpar[i, c] * x[c] for c in range(4)) for i in range(6)]
    Delta = lx.innovation_element(xi0, dU, gamma[8:11], gamma[11:].reshape(-1, 3), "discrete" if discrete else "continuous")
    return dict(DeltaU=dU, X=Delta * X, bias=[mpf(float(snap["bias"][i])) + mpf(float(gamma[i])) for i in range(6)])
