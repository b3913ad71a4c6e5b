"""TEST INFRASTRUCTURE ONLY -- ONE step of the iterated landmark observation update (csrc/eqf_iterate.hpp, eqf_iterate_host.hpp;
consistency.observe_iterated_step is the numpy statement): given Sigma, the state and the increment g_k on each entry's landmark block, the
rows at the trial point, r~_k and g_{k+1}, from the definitions at 50 digits (mpmath, through tests/lie_exact.py and
tests/observe_exact.py), an a-priori first-order bound, and a restatement with switchable faults.  Nothing of oracle/ is imported.

THE REFERENCE (one_step()).  Sigma, p0_i, Q_i = (q_i, a_i), g, meas and R are exact doubles.  Per entry that takes part
    Q_trial = (exp(-(p0 x g) / |p0|^2) R(q), exp(-p0 . g / |p0|^2) a)      Rodrigues and mp.exp at 50 digits
    (Ht, resid) = observe_exact.entry at Q_trial                            its quaternion and scale rounded ONCE to doubles
    r~ = resid + Ht g
and with M the landmark 3-blocks of the entries `on`, Hd the block-diagonal rows over M, Rd = blockdiag(R_e) (lower triangles mirrored):
    T = Sigma_MM Hd^T,   S = Hd T + Rd,   w = S^-1 r~,   g_next = T w   (zero on an entry whose landmark is considered)

THE BOUND, first order, u = 2^-53.  Rows and r~: observe_exact's sums of absolute terms s_Ht, s_resid with K_OBS, at the estimate and at
a moved trial point alike (the sums carry T(q) / |a|, the absolute terms of the rotation, which is what the trial point's own
evaluation enters the rows through).  r~ adds its one product:
    s_rt = s_resid + s_Ht |g| + |Ht||g| + |resid|
g_next, in the form score_exact.py uses for a factorisation with a carried right-hand side (dS into the solve, the factorisation's
(m + 1) u |L||L^T| with both triangular solves, the right-hand side's own error), with e_H = K_OBS s_Ht laid out as Hd, e_r = K_OBS s_rt:
    dT = |Sigma_MM| e_H^T + 4 |Sigma_MM||Hd^T|
    dS = e_H |Sigma_MM||Hd^T| + |Hd||Sigma_MM| e_H^T + 8 |Hd||Sigma_MM||Hd^T| + |Rd| + 3 (m + 1) |L||L^T|
    |d g_next| <= K_ITER u ( dT |w| + |T||S^-1| (e_r + dS |w|) + (m + 4) |T||w| )
K_ITER is the next power of two above 4 x the worst ratio of consistency.observe_iterated_step (numpy, fp64) to the unit form
(K_ITER = 1) over the committed cases of tests/iterate_cases.py, as K_SPLIT and K_OBS were set; tests/test_iterate_exact.py re-measures
the ratio and NOTES.md records it.  A zero bound means an exact value.

THE SOLVE AT 50 DIGITS.  Hd is block diagonal, so S's block (p, q) = Ht_p Sigma_pq Ht_q^T and g_next = Sigma_MM (Hd^T w) are formed block
by block, never as dense products, and in exact integer arithmetic: doubles and mpf values are dyadic rationals, so a product of blocks
is a sum of integers at one common exponent, rounded to 50 digits once.  w solves the 50-digit system by iterative refinement: the correction comes from an fp64
factorisation of S, the residual r~ - S w is taken at 50 digits, and the loop ends when that residual is below 1e-44 of the right-hand
side -- the solution of the 50-digit system to about 44 digits minus the condition's, whatever the fp64 solver did; where the
refinement does not get there (a condition beyond 1e14) mp.lu_solve takes over.  An order of 260 then costs seconds, not a minute."""
import numpy as np
from mpmath import mp, mpf

import lie_exact as lx
import observe_exact as ox
from eqf_vio_amd import consistency as cs

U = 2.0 ** -53
K_ITER_MEASURED = 0.0011959473478962972  # the numpy statement's worst ratio to the unit form over the committed cases (test_iterate_exact.py re-measures it)
K_ITER = 2.0 ** -7  # the next power of two above 4 x K_ITER_MEASURED = 0.00478 (the unit form is that loose: it carries K_OBS on every row)
FAULTS = ("htg_sign", "g_wrong_entry", "q_already_moved", "considered_moved")
RUN_FAULTS = ("regate", "stop_off_by_one")


def trial_state(state, ids, g):
    """the state whose named landmarks sit at Q_trial, taken at 50 digits and rounded once"""
    sid = [int(i) for i in state["ids"]]
    p0 = np.asarray(state["origin"]["p"], dtype=float).reshape(-1, 3)
    Qq = np.array(state["group"]["Qq"], dtype=float).reshape(-1, 4)
    Qa = np.array(state["group"]["Qa"], dtype=float).reshape(-1)
    g = np.asarray(g, dtype=float).reshape(-1, 3)
    for k, lid in enumerate(ids):
        if int(lid) not in sid or not g[k].any():
            continue
        i = sid.index(int(lid))
        p, gg = lx.vec(p0[i]), lx.vec(g[k])
        n2 = lx.dot(p, p)
        w = lx.scl(-1 / n2, lx.cross(p, gg))
        th = lx.norm(w)
        dq = [mpf(1), mpf(0), mpf(0), mpf(0)] if th == 0 else [mp.cos(th / 2)] + lx.scl(mp.sin(th / 2) / th, w)
        q = lx.unit(lx.vec(Qq[i]))
        a, b = dq, q
        qt = [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
              a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]]
        Qq[i] = [float(x) for x in qt]
        Qa[i] = float(mp.exp(-lx.dot(p, gg) / n2) * mpf(float(Qa[i])))
    return dict(state, group=dict(state["group"], Qq=Qq, Qa=Qa))


def _dense(blocks, on, rows, cols):
    out = np.zeros((rows * len(on), cols * len(on)))
    for p, k in enumerate(on):
        out[rows * p:rows * (p + 1), cols * p:cols * (p + 1)] = blocks[k]
    return out


def one_step(kind, Sigma, state, ids, meas, R, g, on, cam=None, consider=None):
    """dict(Ht, rt: per entry lists of mpf (None where not formed), used, s_Ht, s_rt: the unit sums as float arrays, k_rows,
    g_next (K, 3) mpf in an object array, bound (K, 3): the UNIT form of |d g_next| (times K_ITER u is the bound))"""
    ids = np.asarray(ids, dtype=int).reshape(-1)
    K, rows = len(ids), ox.ROWS[kind]
    g = np.asarray(g, dtype=float).reshape(K, 3)
    R = np.asarray(R, dtype=float).reshape(K, rows, rows)
    ref = ox.reference(kind, trial_state(state, ids, g), ids, meas, cam)
    k_rows = ox.K_OBS
    rt, s_rt = [None] * K, np.zeros((K, rows))
    for k in range(K):
        if ref["Ht"][k] is None:
            continue
        gv = lx.vec(g[k])
        rt[k] = [ref["resid"][k][r] + lx.dot(ref["Ht"][k][r], gv) for r in range(rows)]
        aH = np.array([[abs(float(x)) for x in row] for row in ref["Ht"][k]])
        s_rt[k] = ref["s_resid"][k] + ref["s_Ht"][k] @ np.abs(g[k]) + aH @ np.abs(g[k]) + np.array([abs(float(x)) for x in ref["resid"][k]])
    out = dict(Ht=ref["Ht"], rt=rt, used=ref["used"], s_Ht=ref["s_Ht"], s_rt=s_rt, k_rows=k_rows)
    gn = np.array([[mpf(0)] * 3 for _ in range(K)], dtype=object)
    bound = np.zeros((K, 3))
    on = [int(k) for k in on]
    if on and all(ref["used"][k] == 1 for k in on):
        sid = [int(i) for i in state["ids"]]
        M = [11 + 3 * sid.index(int(ids[k])) + c for k in on for c in range(3)]
        Sg = np.tril(np.asarray(Sigma, dtype=float))
        Sg = (Sg + np.tril(Sg, -1).T)[np.ix_(M, M)]
        c, m = len(on), rows * len(on)
        Rl = np.tril(R) + np.transpose(np.tril(R, -1), (0, 2, 1))
        Rd = _dense(Rl, on, rows, rows)
        # exact integer arithmetic: every input is a dyadic rational (a double, or an mpf of the reference), so the block products are
        # sums of integers at one common exponent, rounded to 50 digits once when they come back
        HI, eH = _ints([x for k in on for row in ref["Ht"][k] for x in row])
        HI = np.array(HI, dtype=object).reshape(c, rows, 3)
        SI, eS = _ints([mpf(float(x)) for x in Sg.reshape(-1)])
        SI = np.array(SI, dtype=object).reshape(3 * c, 3 * c)
        A = np.concatenate([HI[p].dot(SI[3 * p:3 * p + 3]) for p in range(c)])            # Hd Sigma_MM: (m, 3 c)
        SX = np.concatenate([A[:, 3 * q:3 * q + 3].dot(HI[q].T) for q in range(c)], axis=1)  # ... Hd^T: (m, m), block column by block column
        two = mpf(2) ** (2 * eH + eS)
        S = [[mpf(int(SX[i, j])) * two + mpf(float(Rd[i, j])) for j in range(m)] for i in range(m)]
        rhs = [x for k in on for x in rt[k]]
        Sf = np.array([[float(x) for x in row] for row in S])
        w = _refined_solve(S, Sf, rhs)
        WI, eW = _ints(w)
        WI = np.array(WI, dtype=object).reshape(c, rows)
        V = np.concatenate([HI[p].T.dot(WI[p]) for p in range(c)])                        # Hd^T w: (3 c,)
        two = mpf(2) ** (eS + eH + eW)
        gx = [mpf(int(x)) * two for x in SI.dot(V)]
        Hf = _dense([np.array([[float(x) for x in row] for row in ref["Ht"][k]]) if ref["Ht"][k] is not None else np.zeros((rows, 3))
                     for k in range(K)], on, rows, 3)
        aH, aS, aw = np.abs(Hf), np.abs(Sg), np.abs(np.array([float(x) for x in w]))
        aT = np.abs(Sg @ Hf.T)                               # (|T| for the bound: fp64 is plenty)
        eH = k_rows * _dense(ref["s_Ht"], on, rows, 3)
        er = k_rows * np.concatenate([s_rt[k] for k in on])
        L = np.linalg.cholesky(Sf)
        dT = aS @ eH.T + 4 * aS @ aH.T
        dS = eH @ aS @ aH.T + aH @ aS @ eH.T + 8 * aH @ aS @ aH.T + np.abs(Rd) + 3 * (m + 1) * (np.abs(L) @ np.abs(L).T)
        b = dT @ aw + aT @ np.abs(np.linalg.inv(Sf)) @ (er + dS @ aw) + (m + 4) * aT @ aw
        cons = [] if consider is None else [int(x) for x in consider]
        for p, k in enumerate(on):
            if int(ids[k]) in cons:
                continue
            for a in range(3):
                gn[k, a], bound[k, a] = gx[3 * p + a], b[3 * p + a]
    out.update(g_next=gn, bound=bound)
    return out


def _ints(xs):
    """(integers, e) with x = integer * 2^e exactly for every mpf x of the list"""
    t = [x._mpf_ for x in xs]
    e = min([v[2] for v in t if v[1]] or [0])
    return [(-v[1] if v[0] else v[1]) << (v[2] - e) if v[1] else 0 for v in t], e


def _refined_solve(S, Sf, rhs):
    """w with S w = rhs at 50 digits (S: lists of mpf, Sf its fp64 rounding): iterative refinement, the residual from exact integer
    products rounded once to 50 digits"""
    m = len(rhs)
    w = [mpf(0)] * m
    top = max(abs(x) for x in rhs)
    if top == 0:
        return w
    SI, eS = _ints([x for row in S for x in row])
    SI = np.array(SI, dtype=object).reshape(m, m)
    for _ in range(16):
        WI, eW = _ints(w)
        two = mpf(2) ** (eS + eW)
        res = [rhs[i] - mpf(int(x)) * two for i, x in enumerate(SI.dot(np.array(WI, dtype=object)))]
        worst = max(abs(x) for x in res)
        if worst <= mpf(10) ** -44 * top:
            return w
        scale = worst                                         # (the residual shrinks far below what fp64 holds next to the first one)
        dx = np.linalg.solve(Sf, np.array([float(x / scale) for x in res]))
        w = [w[i] + scale * mpf(float(dx[i])) for i in range(m)]
    sol = mp.lu_solve(mp.matrix([[x for x in row] for row in S]), mp.matrix(rhs))
    return [sol[i] for i in range(m)]


def row_ratios(Ht, rt, ref):
    """(worst |Ht - ref| / bound, worst |r~ - ref| / bound), the bound K_OBS u s"""
    return ox.ratios(Ht, rt, ref["used"], dict(Ht=ref["Ht"], resid=ref["rt"], used=ref["used"], s_Ht=ref["s_Ht"], s_resid=ref["s_rt"]),
                     k_obs=ref["k_rows"])


def step_ratio(g_next, ref, k_iter=None):
    """worst |g_next - ref| / (K_ITER u bound); a zero bound wants the reference's value exactly; a value that is not finite is outside"""
    k_iter = K_ITER if k_iter is None else k_iter
    g_next = np.asarray(g_next, dtype=float).reshape(-1, 3)
    worst = 0.0
    for k in range(len(g_next)):
        for c in range(3):
            v, b = float(g_next[k, c]), mpf(k_iter) * mpf(U) * mpf(float(ref["bound"][k, c]))
            if not np.isfinite(v):
                return np.inf
            err = abs(mpf(v) - ref["g_next"][k, c])
            if b == 0:
                if err != 0:
                    return np.inf
            else:
                worst = max(worst, float(err / b))
    return worst


# ---- a restatement with switchable faults --------------------------------------------------------------------------------------------------
def model_step(kind, Sigma, state, ids, meas, R, g, on, cam=None, consider=None, fault=None):
    """consistency.observe_iterated_step with one of FAULTS: (Ht, rt, g_next)"""
    ids = np.asarray(ids, dtype=int).reshape(-1)
    g = np.asarray(g, dtype=float).reshape(len(ids), 3)
    at, st = g, state
    if fault == "g_wrong_entry":
        at = np.roll(g, 1, axis=0)
    if fault == "q_already_moved":
        st = cs.landmark_step_state(state, ids, g)       # the trial point built on a Q that has already taken the step
    if fault == "considered_moved":
        consider = None
    Ht, rt, gn, _ = cs.observe_iterated_step(kind, Sigma, st, ids, meas, R, at, on, cam, consider)
    if fault == "htg_sign":
        rt = rt - 2 * np.einsum("krc,kc->kr", Ht, at)
        Ht2, rt2, gn, _ = _with_rt(kind, Sigma, state, ids, R, Ht, rt, on, consider)
    return Ht, rt, gn


def _with_rt(kind, Sigma, state, ids, R, Ht, rt, on, consider):
    _, Hd, Smm, Rd = cs._iter_blocks(np.asarray(Sigma, dtype=float), state, ids, on, Ht, np.asarray(R, dtype=float))
    T = Smm @ Hd.T
    w = np.linalg.solve(Hd @ T + Rd, rt[on].reshape(-1))
    gn = np.zeros((len(ids), 3))
    gn[on] = (T @ w).reshape(len(on), 3)
    for k in on:
        if consider is not None and int(ids[k]) in [int(c) for c in consider]:
            gn[k] = 0.0
    return Ht, rt, gn, False


def model_run(kind, Sigma, state, ids, meas, R, cam, max_lin, tol, lm_gate, fault=None):
    """the sequence of consistency.observe_iterated_host -- (used, n_lin, status) -- with one of RUN_FAULTS"""
    ids = np.asarray(ids, dtype=int).reshape(-1)
    K, rows = len(ids), ox.ROWS[kind]
    R = np.asarray(R, dtype=float).reshape(K, rows, rows)
    sid = [int(i) for i in state["ids"]]
    idx = np.array([sid.index(int(i)) if int(i) in sid else -1 for i in ids])

    def verdicts(Ht, rt, u3):
        f = cs.update_landmarks_host(Sigma, np.where(u3 == 1, idx, -1), Ht, rt, R, lm_gate=lm_gate)
        return np.where(u3 == 3, 3, f["used"]).astype(np.uint8)

    Ht, rt, u3 = cs.observe_rows_host(kind, state, ids, meas, cam)
    used = verdicts(Ht, rt, u3)
    g = np.zeros((K, 3))
    for k in range(max_lin - 1):
        on = [int(e) for e in np.flatnonzero(used == 1)]
        _, _, gn, _ = _with_rt(kind, Sigma, state, ids, R, Ht, rt, on, None)
        step = float(np.max(np.abs(gn - g)))
        if tol > 0 and step <= tol:
            return used, (k + 2 if fault == "stop_off_by_one" else k + 1), cs.ITER_CONVERGED
        Hn, rn, u = cs.observe_rows_host(kind, cs.landmark_step_state(state, ids, gn), ids, meas, cam)
        if any(u[e] != 1 for e in on):
            return used, k + 1, cs.ITER_STALLED
        for e in on:
            Ht[e], rt[e] = Hn[e], rn[e] + Hn[e] @ gn[e]
        if fault == "regate":
            used = verdicts(Ht, rt, u3)
        g = gn
    return used, max_lin, cs.ITER_EXHAUSTED


# ---- the case of a stall ---------------------------------------------------------------------------------------------------------------------
def stall_case(st):
    """(state, ids, meas, R) from a dumped one-filter state: a range 1000 times the predicted one on landmark 0 under a depth prior wide
    enough to follow it (sigma = 1e4 |p0| along p0, in the chart's coordinates), so that the first increment has -p0 . g / |p0|^2 below
    -745, exp underflows to zero, the trial scale is 0 and the trial point is not finite"""
    st = dict(st)
    S = np.array(st["sigma"], dtype=float)
    p0 = np.asarray(st["origin"]["p"], dtype=float).reshape(-1, 3)[0]
    S[11:14, :] = 0.0
    S[:, 11:14] = 0.0
    S[11:14, 11:14] = (1e4 * np.linalg.norm(p0)) ** 2 * np.eye(3)
    st["sigma"] = S
    ids = np.array([int(st["ids"][0])], dtype=np.int32)
    Ht, r, _ = cs.observe_rows_host(cs.OBS_RANGE, st, ids, np.ones((1, 3)))
    d = 1.0 - float(r[0, 0])
    meas = np.array([[1000.0 * d, 0.0, 0.0]])
    return st, ids, meas, np.array([[[1e-4 * d * d]]])
