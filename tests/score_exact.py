"""TEST INFRASTRUCTURE ONLY -- the record of eqf_score_vision (csrc/eqf_score.hpp) for one candidate: an exact reference, an a-priori bound
on what any fp64 implementation of it may differ from that reference by, and a numpy model of the kernels' blocking.  Built from what is
already there; nothing here comes from the device.

THE REFERENCE.  A candidate is the list `slots` of matched state slots in the state's order, with one bearing each.  From the DEFINITIONS:
    delta_i, C0i            update_exact.Geometry at 50 digits from the snapshot's group and origin, rounded ONCE to np.longdouble
    Sigma                   the filter's own sigma() (fp64, taken as exact: the score is taken at the handle's present Sigma, there is no
                            propagate and so no E_ric); its LOWER triangle is read and mirrored
    S = C_M Sigma_MM C_M^T + r I = L L^T,   z = L^-1 delta_M      update_exact.chol / solve_lower in longdouble, or -- use_mp, |M| <= MP_MAX_N -- in
                                                                  mpmath at 50 digits on the unrounded inputs
    nis = z^T z,  logdet_S = 2 sum log L_kk,  loglik = -(nis + logdet_S + m log 2 pi) / 2,  m = 2 |M|,
    nis_lm[i] = delta_i^T S_ii^-1 delta_i from the 2 x 2 diagonal block of S in closed form.

THE BOUND, first order.  u = 2^-53, gamma_k = k u / (1 - k u), w = S^-1 delta, T = chol_bounds.block_T(L), p = chol_bounds.P; dC, dB, dS and
ddelta are exactly the forms and constants of update_exact's docstring (TAU_BLK, OPS_C, OPS_S, K_DELTA), on the matched landmarks:
    dC = tau_blk u max|C0i|,  dB = gamma_3 |C||Sigma| + dC |Sigma|,  dS = dB |C^T| + gamma_4 |B||C^T| + |B| dC^T + u |S|,
    E1 = mirror(((m + 1) u + p)(|L||L^T|) T^T),   E2z = (m + 16) u T (|L||z| + |delta|),   ddelta = K_DELTA u (1 + |delta|),   D = dS + E1
and the statistics follow consistency_exact.innovation_stats_reference (part C) with consistency_cases.C_LOG, without its propagate term:
    |d nis|       <= 2 |w|^T (ddelta + E2z) + |w|^T D |w| + gamma_s nis,   s = ceil(m / 256) + 8   (k_score_tail: thread t takes the terms t, t + 256,
                     ... with one fma each, then the tree w = 128 .. 1 -- k_innov_stats' order)
    |d logdet_S|  <= sum_ij |S^-1|_ij D_ij + 2 sum_k c_log u (1 + |log L_kk|) + gamma_s 2 sum_k |log L_kk|
    |d nis_lm[i]| <= 2 |w_i|^T ddelta_i + |w_i|^T (dS_ii + gamma_8 |S_ii|) |w_i| + gamma_8 nis_lm[i]      (gateMahalanobis: the 2 x 2 factor itself)
    |d loglik|    <= (d nis + d logdet_S) / 2 + 2 u (|nis| + |logdet_S| + m log 2 pi)
The bound stays a CONDITION: a case is committed only if bound <= consistency_exact.VALIDITY (1 + |value|) for every statistic
(tests/score_cases.py says which states were rejected; tests/test_score_exact.py asserts it for every committed case)."""
import numpy as np
from mpmath import mp, mpf

import chol_bounds as cb
import consistency_cases as cc
import consistency_exact as cx
import lie_exact as lx
import mergecost_exact as gx
import riccati_exact as rx
import update_exact as ux

LD = rx.LD
U = cx.U
MP_MAX_N = ux.MP_MAX_N
LOG_2PI = cx.LOG_2PI


def geometry(snap, d, y):
    """update_exact.Geometry of a snapshot (dict with origin, group) under the settings d, y (N, 3) one bearing per landmark of the state."""
    xi0 = lx.State.from_dict(snap["origin"], d["cameraOffset_q"], d["cameraOffset_x"])
    return ux.Geometry(lx.Group.from_dict(snap["group"]), xi0, y)


def _sub_sigma(Sigma, slots, conv):
    """the rows / columns of the matched landmarks behind an empty 11-coordinate base, from the LOWER triangle of Sigma, in conv's arithmetic"""
    S = np.tril(np.asarray(Sigma, dtype=np.float64))
    S = S + np.tril(S, -1).T
    idx = [11 + 3 * s + c for s in slots for c in range(3)]
    k = len(idx)
    out = np.array([[conv(0.0)] * (11 + k) for _ in range(11 + k)], dtype=object if conv is not LD else LD)
    sub = S[np.ix_(idx, idx)]
    for i in range(k):
        for j in range(k):
            out[11 + i, 11 + j] = conv(float(sub[i, j]))
    return out


def reference(Sigma, geo, r, slots, use_mp=False):
    """The record of the module docstring and every intermediate the bound needs, in longdouble (or mpf with use_mp): dict(m, nis, logdet_S,
    loglik, nis_lm, S, L, z, delta, C0, SM, B)."""
    slots = [int(s) for s in slots]
    M = len(slots)
    m = 2 * M
    g = geo.arrays(ux._same if use_mp else rx._ld)
    conv = (lambda v: mpf(v)) if use_mp else LD
    sqrt, log = (mp.sqrt, mp.log) if use_mp else (np.sqrt, np.log)
    zero = conv(0.0)
    if M == 0:
        return dict(m=0, nis=zero, logdet_S=zero, loglik=zero, nis_lm=np.zeros(0, dtype=object if use_mp else LD))
    C0 = g["C0"][slots]
    delta = np.concatenate([g["delta"][2 * s:2 * s + 2] for s in slots])
    SM = _sub_sigma(Sigma, slots, conv)
    B = ux.c_times(C0, SM, M)
    S = ux.times_ct(B, C0, M)
    rr = conv(float(r))
    for i in range(m):
        S[i, i] = S[i, i] + rr
    L = ux.chol(S, sqrt)
    z = ux.solve_lower(L, delta)
    nis = sum(z[i] * z[i] for i in range(m))
    logdet = 2 * sum(log(L[i, i]) for i in range(m))
    nis_lm = np.array([zero] * M, dtype=object if use_mp else LD)
    for i in range(M):
        k = slice(2 * i, 2 * i + 2)
        Sii, di = S[k, k], delta[k]
        det = Sii[0, 0] * Sii[1, 1] - Sii[1, 0] * Sii[1, 0]
        w0, w1 = (Sii[1, 1] * di[0] - Sii[1, 0] * di[1]) / det, (Sii[0, 0] * di[1] - Sii[1, 0] * di[0]) / det
        nis_lm[i] = w0 * di[0] + w1 * di[1]
    loglik = -(nis + logdet + m * conv(LOG_2PI)) / 2
    return dict(m=m, nis=nis, logdet_S=logdet, loglik=loglik, nis_lm=nis_lm, S=S, L=L, z=z, delta=delta, C0=C0, SM=SM, B=B)


def bounds(ref, c_log=None, tau=None, k_delta=None):
    """{nis, logdet_S, loglik, nis_lm (|M|,)}: the bounds of the module docstring (fp64) from reference()'s longdouble result."""
    c_log = cc.C_LOG if c_log is None else c_log
    tau = rx.TAU_BLK if tau is None else tau
    k_delta = ux.K_DELTA if k_delta is None else k_delta
    m = ref["m"]
    M = m // 2
    if m == 0:
        return dict(nis=0.0, logdet_S=0.0, loglik=0.0, nis_lm=np.zeros(0))
    u = U
    a = lambda k: np.abs(ux.f64(ref[k]))  # noqa: E731
    aSM, aB, aS, aL, az, adelta, aC0 = a("SM"), a("B"), a("S"), a("L"), a("z"), a("delta"), a("C0")
    L = ref["L"]
    w = ux.solve_upper_t(L, ref["z"])
    aw = np.abs(ux.f64(w))
    dC0 = np.stack([np.full((2, 3), tau * u * aC0[i].max()) for i in range(M)])
    T = cb.block_T(ux.f64(L))
    ddelta = k_delta * u * (1 + adelta)
    dB = ux.gamma(ux.OPS_C) * ux.c_times(aC0, aSM, M) + ux.c_times(dC0, aSM, M)
    dS = ux.times_ct(dB, aC0, M) + ux.gamma(ux.OPS_S) * ux.times_ct(aB, aC0, M) + ux.times_ct(aB, dC0, M) + u * aS
    dS = np.maximum(dS, dS.T)
    E1 = ux._mirror_lower(((m + 1) * u + cb.P) * ((aL @ aL.T) @ T.T))
    E2z = (m + 16) * u * (T @ (aL @ az + adelta))
    D = dS + E1
    nis = float(ref["nis"])
    logs = np.log(np.diag(L))
    al = np.abs(logs).astype(np.float64)
    s = cx.ops_innov(m)
    b_nis = float(2 * aw @ (ddelta + E2z) + aw @ D @ aw + cx.gamma(s, u) * nis)
    Linv = cb.inv_lower(L).astype(np.float64)
    b_ld = float((np.abs(Linv.T @ Linv) * D).sum() + 2 * c_log * u * (1 + al).sum() + cx.gamma(s, u) * 2 * al.sum())
    b_lm = np.zeros(M)
    for i in range(M):
        k = slice(2 * i, 2 * i + 2)
        Sii, di = ref["S"][k, k], ref["delta"][k]
        det = Sii[0, 0] * Sii[1, 1] - Sii[1, 0] * Sii[1, 0]
        wi = np.array([Sii[1, 1] * di[0] - Sii[1, 0] * di[1], Sii[0, 0] * di[1] - Sii[1, 0] * di[0]], dtype=LD) / det
        awi = np.abs(wi).astype(np.float64)
        Dii = dS[k, k] + cx.gamma(cx.OPS_LM, u) * np.abs(Sii).astype(np.float64)
        b_lm[i] = 2 * awi @ ddelta[k] + awi @ Dii @ awi + cx.gamma(cx.OPS_LM, u) * float(ref["nis_lm"][i])
    b_ll = (b_nis + b_ld) / 2 + 2 * u * (abs(nis) + abs(float(ref["logdet_S"])) + m * LOG_2PI)
    return dict(nis=b_nis, logdet_S=b_ld, loglik=float(b_ll), nis_lm=b_lm)


def condition(ref, bnd):
    """worst bound / (VALIDITY (1 + |value|)) over the statistics: a case may be committed only where this is <= 1"""
    worst = 0.0
    for k in ("nis", "logdet_S", "loglik"):
        worst = max(worst, bnd[k] / (cx.VALIDITY * (1 + abs(float(ref[k])))))
    for i in range(len(bnd["nis_lm"])):
        worst = max(worst, bnd["nis_lm"][i] / (cx.VALIDITY * (1 + abs(float(ref["nis_lm"][i])))))
    return worst


def ratios(got, ref, bnd):
    """{nis, logdet_S, loglik, nis_lm}: worst |got - ref| / bound (got: dict with fp64 values, nis_lm in the reference's order).  Where a
    bound is exactly 0 (an empty candidate) the value must be exactly the reference's; a value that is not a number is outside every bound."""
    out = {}
    for k in ("nis", "logdet_S", "loglik"):
        err = abs(LD(got[k]) - LD(ref[k]))
        out[k] = 0.0 if err == 0 else (float(err) / bnd[k] if bnd[k] > 0 else np.inf)
    d = np.abs(np.asarray(got["nis_lm"], dtype=LD) - np.asarray(ref["nis_lm"], dtype=LD)).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(d == 0, 0.0, np.where(bnd["nis_lm"] > 0, d / bnd["nis_lm"], np.inf))
    out["nis_lm"] = float(q.max()) if len(q) else 0.0
    return {k: (np.inf if np.isnan(v) else v) for k, v in out.items()}


def mp_share(ref_ld, ref_mp, bnd):
    """the largest |longdouble - mpmath| / bound over the statistics: the share of the bound the reference's own arithmetic could take"""
    def diff(a, b):  # a longdouble, b mpf
        a = LD(a)
        hi = float(a)
        return abs(mpf(hi) + mpf(float(a - LD(hi))) - b)

    share = 0.0
    for k in ("nis", "logdet_S", "loglik"):
        share = max(share, float(diff(ref_ld[k], ref_mp[k]) / mpf(bnd[k])))
    for i in range(len(bnd["nis_lm"])):
        share = max(share, float(diff(ref_ld["nis_lm"][i], ref_mp["nis_lm"][i]) / mpf(float(bnd["nis_lm"][i]))))
    return share


def model(Sigma, C0, delta, r, slots):
    """The record as the kernels block it, in fp64 numpy: S formed block by block from the LOWER triangle of Sigma (C Sigma first), the
    64-wide right-looking factorisation with delta carried along (mergecost_exact.blocked_cholesky), the 2 x 2 factor per landmark.
    C0 (N, 2, 3) and delta (N, 2) per landmark of the state."""
    slots = [int(s) for s in slots]
    M = len(slots)
    if M == 0:
        return dict(nis=0.0, logdet_S=0.0, loglik=0.0, dof=0, nis_lm=np.zeros(0))
    Sg = np.asarray(Sigma, dtype=np.float64)
    S = np.zeros((2 * M, 2 * M))
    for a_, sa in enumerate(slots):
        for b_, sb in enumerate(slots[:a_ + 1]):
            S[2 * a_:2 * a_ + 2, 2 * b_:2 * b_ + 2] = (C0[sa] @ Sg[11 + 3 * sa:14 + 3 * sa, 11 + 3 * sb:14 + 3 * sb]) @ C0[sb].T
    S = np.tril(S) + r * np.eye(2 * M)
    dm = np.concatenate([np.asarray(delta, dtype=np.float64).reshape(-1, 2)[s] for s in slots])
    L, z = gx.blocked_cholesky(S, dm)
    nis, logdet = float(z @ z), 2.0 * float(np.sum(np.log(np.diag(L))))
    lm = np.zeros(M)
    for i in range(M):
        s00, s10, s11 = S[2 * i, 2 * i], S[2 * i + 1, 2 * i], S[2 * i + 1, 2 * i + 1]
        l00 = np.sqrt(s00)
        l10 = s10 / l00
        l11 = np.sqrt(s11 - l10 * l10)
        w0 = dm[2 * i] / l00
        w1 = (dm[2 * i + 1] - l10 * w0) / l11
        lm[i] = w1 * w1 + w0 * w0
    return dict(nis=nis, logdet_S=logdet, loglik=-0.5 * (nis + logdet + 2 * M * LOG_2PI), dof=2 * M, nis_lm=lm)
