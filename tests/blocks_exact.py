"""TEST INFRASTRUCTURE ONLY -- the per-landmark block measurement update (csrc/eqf_blocks.hpp: eqf_update_landmarks) entry by entry: a
reference from the definitions, an a-priori first-order componentwise bound, and a numpy model of the update with switchable faults.
np.longdouble with J's blocks from mpmath at 50 digits; nothing of oracle/ is imported.

THE REFERENCE (reference()).  Sigma is the device's own sigma() (exact doubles) TAKEN BY ITS LOWER TRIANGLE, H_k, resid_k, R_k the caller's
(exact doubles; every R_k's lower triangle mirrored), quaternions as stored.  Ht_k = H_k (local = 0) or H_k J_i with J_i at 50 digits
(consistency_exact.jacobian_mp from the device's own origin() and group()), each entry rounded once to longdouble.  Per entry, in
longdouble: d2_k = resid_k^T (Ht_k Sigma_ii Ht_k^T + R_k)^-1 resid_k and the verdict 1 (applied), 0 (id not in the state), 2 (d2_k >
lm_gate).  The entries that take part are the block rows of the dense m x n matrix Ht, m = rows * (their number); then linear_exact.reference
(longdouble, update_exact.chol / solve_lower):
    B = Sigma Ht^T   S = Ht B + blockdiag(R_k) = L L^T   Y = L^-1 B^T   z = L^-1 resid   gamma = Y^T z   Sigma+ = Sigma - Y^T Y
    nis = z^T z   logdet_S = 2 sum log L_kk   loglik = -(nis + logdet_S + m log 2 pi) / 2
A decoupled block (H = 0, resid = 0, R = I) changes nothing of these, adds 0 to nis and logdet_S and is not counted in dof: it is left out.

THE BOUND (bounds()) is K_BLOCKS times linear_exact.bounds' first-order form (Higham's componentwise forms for products, the Cholesky
factorisation and the triangular solves, propagated through K = Y^T L^-1 and w = L^-T z) taken with UNIT operation counts, every gamma_k
replaced by gamma_1 = u: the update is implemented three times over -- LAPACK on the host, 64-wide blocks with inverse diagonal blocks on
the matrix cores on the device -- and no single set of counts describes them all, so the count is one constant in front of the form,
    K_BLOCKS = 4 x the worst ratio of consistency.update_landmarks_host (fp64) to the unit form over the committed cases
(tests/test_blocks_exact.py re-measures it, as test_update_exact.py does K_DELTA; stored unrounded).  u = 2^-53; the unit form:
    dHt   = 0 (local = 0)  |  u |H||J| + |H||dJ| (local = 1; |dJ| = consistency_exact.jacobian_tol with consistency_cases.K_J)
    dB    = u |Ht||Sigma| + dHt |Sigma|
    dS    = dB |Ht^T| + u (|B||Ht^T| + |R|) + |B| dHt^T, mirrored
    E1    = u |L||L^T|, mirrored       E2 = u |L||Y|       E2z = u |L||z|       E3 = u |Y|^T |Y| + u |Sigma+|
    |dSigma+| <= G + G^T + |K|(dS + E1)|K|^T + E3,  G = |K|(dB + E2)
    |dgamma|  <= |K| E2z + (dB + E2)^T |w| + |K|(dS + E1)|w| + u |Y|^T |z|
    |d nis|      <= 2 |w|^T E2z + |w|^T (dS + E1) |w| + u nis
    |d logdet_S| <= sum_ij |S^-1|_ij (dS + E1)_ij + 2 sum_k c_log u (1 + |log L_kk|) + u 2 sum_k |log L_kk|
    |d loglik|   <= (d nis + d logdet_S) / 2 + 4 u (|nis| + |logdet_S| + m log 2 pi) / 2
used and dof are exact (a case keeps every d2_k well away from lm_gate); Sigma+ must be bit-for-bit symmetric.
First order is licensed per case by VALIDITY: K_BLOCKS max |L^-1| (dS + E1) |L^-T| <= 1e-3."""
import numpy as np

import consistency_cases as cc
import consistency_exact as cx
import linear_exact as le
import update_exact as ux
from riccati_exact import LD

U = 2.0 ** -53
K_BLOCKS_MEASURED = 8.781955146049086  # the host statement's worst ratio to the unit form; test_blocks_exact.py re-measures it
K_BLOCKS = 4.0 * K_BLOCKS_MEASURED
VALIDITY = cx.VALIDITY
LOG2PI = le.LOG2PI


def mirror_lower(S):
    S = np.asarray(S)
    return np.tril(S) + np.tril(S, -1).T


def entry_rows(ops, Jmp, N):
    """(Ht (K, rows, 3) longdouble, dHt (K, rows, 3)): every entry's rows in Sigma's coordinates and the entrywise bound on the device's"""
    H = np.asarray(ops["H"], dtype=np.float64)
    Ht, dHt = H.astype(LD), np.zeros(H.shape)
    if not ops["local"]:
        return Ht, dHt
    _, Jl = cx.jacobian_ld(Jmp, N)
    _, Dl = cx.jacobian_tol(Jmp, cc.K_J, N)
    for k, i in enumerate(ops["idx"]):
        if i < 0:
            continue
        Ht[k] = H[k].astype(LD) @ Jl[i]
        dHt[k] = U * (np.abs(H[k]) @ np.abs(Jl[i]).astype(np.float64)) + np.abs(H[k]) @ Dl[i]
    return Ht, dHt


def dense(N, idx, blocks, dtype):
    K, rows = blocks.shape[0], blocks.shape[1]
    out = np.zeros((rows * K, 11 + 3 * N), dtype=dtype)
    for k in range(K):
        out[rows * k:rows * (k + 1), 11 + 3 * idx[k]:14 + 3 * idx[k]] = blocks[k]
    return out


def reference(Sigma, ops, Jmp):
    """dict: linear_exact.reference's entries for the entries that take part (None of them: m = 0, Sp = Sigma, gamma = 0, nis = logdet_S =
    loglik = 0) plus used (K,), d2 (K,), dof, dHt (m x n), R_dense"""
    Sg = mirror_lower(np.asarray(Sigma, dtype=np.float64))
    n = len(Sg)
    N = (n - 11) // 3
    rows, idx = ops["rows"], [int(i) for i in ops["idx"]]
    K = len(idx)
    Ht, dHt = entry_rows(ops, Jmp, N)
    Rl = np.array([mirror_lower(ops["R"][k]) for k in range(K)], dtype=np.float64).reshape(K, rows, rows)
    resid = np.asarray(ops["resid"], dtype=np.float64).reshape(K, rows)
    used, d2 = np.zeros(K, dtype=np.int32), np.full(K, np.nan)
    for k, i in enumerate(idx):
        if not 0 <= i < N:
            continue
        Skk = Ht[k] @ Sg[11 + 3 * i:14 + 3 * i, 11 + 3 * i:14 + 3 * i].astype(LD) @ Ht[k].T + Rl[k].astype(LD)
        zk = ux.solve_lower(ux.chol(Skk, np.sqrt), resid[k].astype(LD))
        d2[k] = float(zk @ zk)
        used[k] = 2 if d2[k] > ops["lm_gate"] else 1
    on = [k for k in range(K) if used[k] == 1]
    m = rows * len(on)
    if m == 0:
        return dict(m=0, S1=Sg.astype(LD), Sp=Sg.astype(LD), gamma=np.zeros(n, dtype=LD), nis=LD(0), logdet_S=LD(0), loglik=LD(0), used=used,
                    d2=d2, dof=0, dHt=np.zeros((0, n)), R_dense=np.zeros((0, 0)))
    Hd = dense(N, [idx[k] for k in on], Ht[on], LD)
    Rd = np.zeros((m, m))
    for p, k in enumerate(on):
        Rd[rows * p:rows * (p + 1), rows * p:rows * (p + 1)] = Rl[k]
    ref = le.reference(Sg, Hd, resid[on].reshape(-1), Rd)
    ref.update(used=used, d2=d2, dof=m, dHt=dense(N, [idx[k] for k in on], dHt[on], np.float64), R_dense=Rd)
    return ref


def bounds(ref, k_blocks=K_BLOCKS, c_log=cc.C_LOG):
    """{"Sp", "gamma", "nis", "logdet_S", "loglik", "validity"}: the module docstring's bound (fp64) from reference()'s result"""
    n = ref["S1"].shape[0]
    if ref["m"] == 0:  # (nothing runs: every bit stays)
        return dict(Sp=np.zeros((n, n)), gamma=np.zeros(n), nis=0.0, logdet_S=0.0, loglik=0.0, validity=0.0)
    u = g = U
    f64 = ux.f64
    m, dHt = ref["m"], ref["dHt"]
    a = lambda k: np.abs(f64(ref[k]))  # noqa: E731
    aS1, aH, aB, aL, aY, az = a("S1"), a("Ht"), a("B"), a("L"), a("Y"), a("z")
    L = ref["L"]
    Kt = ux.solve_upper_t(L, ref["Y"])            # L^-T Y = K^T (m x n)
    w = ux.solve_upper_t(L, ref["z"])
    aK, aw = np.abs(f64(Kt)).T, np.abs(f64(w))
    dB = g * (aH @ aS1.T) + dHt @ aS1.T
    dS = dB @ aH.T + g * (aB @ aH.T + np.abs(ref["R_dense"])) + aB @ dHt.T
    dS = np.maximum(dS, dS.T)
    E1 = ux._mirror_lower(g * (aL @ aL.T))
    E2 = g * (aL @ aY)
    E2z = g * (aL @ az)
    E3 = g * (aY.T @ aY) + u * np.abs(f64(ref["Sp"]))
    D = dS + E1
    Gm = aK @ (dB + E2)
    out = {"Sp": Gm + Gm.T + aK @ D @ aK.T + E3}
    out["gamma"] = aK @ E2z + (dB + E2).T @ aw + aK @ (D @ aw) + g * (aY.T @ az)
    nis, logdet = float(ref["nis"]), float(ref["logdet_S"])
    out["nis"] = float(2 * aw @ E2z + aw @ D @ aw + g * abs(nis))
    Linv = f64(ux.solve_lower(L, np.eye(m, dtype=LD)))
    aSinv = np.abs(Linv.T @ Linv)
    logs = np.abs(np.log(np.diag(f64(L))))
    out["logdet_S"] = float(np.sum(aSinv * D) + 2 * np.sum(c_log * u * (1 + logs)) + g * 2 * np.sum(logs))
    out["loglik"] = 0.5 * (out["nis"] + out["logdet_S"]) + 0.5 * 4 * u * (abs(nis) + abs(logdet) + m * LOG2PI)
    aLinv = np.abs(Linv)
    out["validity"] = float((aLinv @ D @ aLinv.T).max())
    return {k: k_blocks * v for k, v in out.items()}


def ratios(got, ref, bnd):
    """{"Sp", "gamma", "nis", "logdet_S", "loglik", "used", "dof"} -> worst |got - ref| / bound (update_exact.worst_ratio's rules: a zero
    bound wants the reference's value exactly, a NaN is outside every bound; used and dof: 0 if equal, inf if not)"""
    out = le.ratios(got, ref, bnd)
    out["used"] = 0.0 if np.array_equal(np.asarray(got["used"], dtype=np.int32), ref["used"]) else np.inf
    out["dof"] = 0.0 if int(got["dof"]) == ref["dof"] else np.inf
    return out


# ---- a numpy (fp64) model of the update with switchable faults ------------------------------------------------------------------------------
FAULTS = ("j_omitted", "r_upper_read", "r_next", "gated_coupled", "dof_counts_gated", "y_with_L", "mirror_skipped", "gamma_bias_dropped",
          "absent_as_landmark_0")


def model(Sigma, ops, J, fault=None):
    """consistency.update_landmarks_host's arithmetic restated with one fault of FAULTS switched on.  J: the fp64 landmark blocks
    (local_jacobian_blocks(...)["lm"]) for local rows.  Returns dict(Sigma, gamma, nis, logdet_S, loglik, dof, used)."""
    S0 = np.asarray(Sigma, dtype=np.float64)
    Sg = mirror_lower(S0)
    n = len(Sg)
    N = (n - 11) // 3
    rows, K = ops["rows"], len(ops["idx"])
    H, resid, R = np.asarray(ops["H"], dtype=float), np.asarray(ops["resid"], dtype=float).reshape(K, rows), np.asarray(ops["R"], dtype=float)
    Jl = None if J is None else np.asarray(J, dtype=float).reshape(-1, 3, 3)
    used, Ht, Rl, idx = np.zeros(K, dtype=np.int32), np.zeros((K, rows, 3)), np.zeros((K, rows, rows)), np.zeros(K, dtype=int)
    for k in range(K):
        i = int(ops["idx"][k])
        if i < 0 and fault == "absent_as_landmark_0":
            i = 0
        if not 0 <= i < N:
            continue
        idx[k] = i
        Ht[k] = H[k] @ Jl[i] if (ops["local"] and fault != "j_omitted") else H[k]
        Rk = R[k + 1] if (fault == "r_next" and k + 1 < K) else R[k]
        Rl[k] = mirror_lower(Rk.T if fault == "r_upper_read" else Rk)
        Skk = Ht[k] @ Sg[11 + 3 * i:14 + 3 * i, 11 + 3 * i:14 + 3 * i] @ Ht[k].T + Rl[k]
        try:
            zk = np.linalg.solve(np.linalg.cholesky(Skk), resid[k])
            d2 = float(zk @ zk)
        except np.linalg.LinAlgError:
            d2 = np.nan
        used[k] = 2 if d2 > ops["lm_gate"] else 1
    on = [k for k in range(K) if used[k] == 1 or (used[k] == 2 and fault == "gated_coupled")]
    reported = used.copy()
    if fault == "absent_as_landmark_0":
        reported[[k for k in range(K) if ops["idx"][k] < 0]] = 0
    dof = rows * (int(np.sum(used >= 1)) if fault == "dof_counts_gated" else len([k for k in on if used[k] == 1]))
    out = dict(Sigma=Sg.copy(), gamma=np.zeros(n), nis=0.0, logdet_S=0.0, loglik=0.0, dof=dof, used=reported)
    m = rows * len(on)
    if m == 0:
        return out
    Hd = dense(N, [idx[k] for k in on], Ht[on], np.float64)
    Rd = np.zeros((m, m))
    for p, k in enumerate(on):
        Rd[rows * p:rows * (p + 1), rows * p:rows * (p + 1)] = Rl[k]
    B = Sg @ Hd.T
    S = mirror_lower(Hd @ B + Rd)
    try:
        L = np.linalg.cholesky(S)
    except np.linalg.LinAlgError:
        out.update(nis=np.nan, logdet_S=np.nan, loglik=np.nan)
        return out
    Y = L @ B.T if fault == "y_with_L" else np.linalg.solve(L, B.T)
    z = np.linalg.solve(L, resid[on].reshape(-1))
    gam = Y.T @ z
    if fault == "gamma_bias_dropped":
        gam[:6] = 0.0
    Sp = np.tril(Sg - Y.T @ Y)
    Sp = Sp + (np.triu(S0, 1) if fault == "mirror_skipped" else np.tril(Sp, -1).T)
    nis, logdet = float(z @ z), 2.0 * float(np.sum(np.log(np.diag(L))))
    out.update(Sigma=Sp, gamma=gam, nis=nis, logdet_S=logdet, loglik=-0.5 * (nis + logdet + m * LOG2PI))
    return out
