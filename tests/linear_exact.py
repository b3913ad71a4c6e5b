"""TEST INFRASTRUCTURE ONLY -- the low-rank linear measurement update (csrc/eqf_linear.hpp: eqf_update_linear) entry by entry: a reference
from the definitions, an a-priori first-order bound on what an fp64 implementation with the kernels' operation counts may differ from it by,
and a numpy model of the kernels' blocking with switchable faults.  mpmath (50 digits) and np.longdouble; nothing of oracle/ is imported.

THE REFERENCE (reference()).  Sigma is the device's own sigma() (exact doubles), H, resid, R the caller's (exact doubles; R's lower triangle
mirrored).  Ht = H (local = 0) or H J (local = 1) with J's blocks at 50 digits (consistency_exact.jacobian_mp from the device's own origin()
and group()), each entry rounded once to longdouble.  Then, in longdouble with update_exact.chol / solve_lower (or, use_mp, in mpmath at 50
digits on the unrounded J; n <= consistency_exact.MP_MAX_ORDER):
    Bt = (Sigma Ht^T)^T   S = Ht Bt^T + R = L L^T   Y = L^-1 Bt   z = L^-1 resid   gamma = Y^T z   Sigma+ = Sigma - Y^T Y
    nis = z^T z   logdet_S = 2 sum log L_kk   loglik = -(nis + logdet_S + m log 2 pi) / 2

THE BOUND (bounds()) takes update_exact.update_bounds' forms with C <- Ht, dC <- dHt, E_ric <- 0 and ddelta <- 0 (resid is an input), the
dot-product constants recounted for dense rows and the factorisation constants for the kernel's own 16 x 16 Cholesky (divisions, no
explicit inverses).  u = 2^-53, gamma_k = k u / (1 - k u), n = 11 + 3 N, K = Y^T L^-1 (n x m), w = L^-T z.  Every count is read off
csrc/eqf_linear.hpp:
    dHt   = 0                                          local = 0: k_lin_rows copies
          = gamma_3 |H||J| + |H||dJ|                   local = 1: dot3 = one product and two fused multiply-adds per entry (the 2 x 2 gravity
                                                       block has two terms: covered); |dJ| = consistency_exact.jacobian_tol with
                                                       consistency_cases.K_J, the rounding of the blocks k_local_jacobian builds
    dB    = gamma_n |Ht||Sigma| + dHt |Sigma|          k_lin_gain: n products summed in one fixed order on the matrix cores, one rounding per
                                                       product and one per addition at the most (the pad column and the zero fill of the
                                                       last chunk add exact zeros); gamma_n holds for any order of an n-term sum
    dS    = dB |Ht^T| + gamma_{n+1} |B||Ht^T| + |B| dHt^T
                                                       k_lin_solve: s = R_kl, then n fused multiply-adds in sequence: n + 1 terms, each
                                                       through at most n roundings (gamma_{n+1} as the issue counts it).  Mirrored.
    E1    = gamma_{m+1} |L||L^T|, mirrored             the 16 x 16 right-looking Cholesky with one fused multiply-add per update, a square
                                                       root and divisions [Higham, Thm 10.3]; the identity rows m.. are exact
    E2    = gamma_m |L||Y|,  E2z = gamma_m |L||z|      forward substitution, fused multiply-adds and one division per entry [Higham, Thm 8.5]
    E3    = gamma_m |Y|^T |Y| + u |Sigma+|             k_lin_downdate: m products summed from a zero accumulator (rows m..15 of Y are exact
                                                       zeros), then ONE subtraction from Sigma_ij, stored as it is
    |dSigma+| <= G + G^T + |K|(dS + E1)|K|^T + E3,     G = |K|(dB + E2)
    |dgamma|  <= |K| E2z + (dB + E2)^T |w| + |K|(dS + E1)|w| + gamma_m |Y|^T |z|         gamma_i: m fused multiply-adds in sequence
    with D = dS + E1 (consistency_exact part C's forms):
    |d nis|      <= 2 |w|^T E2z + |w|^T D |w| + gamma_m nis                               m fused multiply-adds in sequence
    |d logdet_S| <= sum_ij |S^-1|_ij D_ij + 2 sum_k c_log u (1 + |log L_kk|) + gamma_m 2 sum_k |log L_kk|      a serial sum of m logarithms
    |d loglik|   <= (d nis + d logdet_S) / 2 + 4 u (|nis| + |logdet_S| + m log 2 pi) / 2   two additions, one product, the constant
The pad row and column of the device's image and entry 11 of its padded gamma must be exactly zero; Sigma+ must be bit-for-bit symmetric.
First order is licensed per case by VALIDITY: max |L^-1| (dS + E1) |L^-T| <= 1e-3 (validity())."""
import numpy as np
from mpmath import mp, mpf

import consistency_cases as cc
import consistency_exact as cx
import update_exact as ux
from riccati_exact import LD, gamma

U = 2.0 ** -53
OPS_J = 3          # dot3: one product, two fused multiply-adds
LOG2PI = float(np.log(2.0 * np.pi))
MP_MAX_ORDER = cx.MP_MAX_ORDER
VALIDITY = cx.VALIDITY
ROWS = 16
TILE = 64


# ---- Ht -------------------------------------------------------------------------------------------------------------------------------------
def _bd_right(H, Jb, Jl):
    """H J for the block-diagonal J = diag(Jb, Jl[0], ...), in the operands' dtype"""
    N = len(Jl)
    out = np.empty(H.shape, dtype=np.result_type(H.dtype, Jb.dtype))
    out[:, :11] = H[:, :11] @ Jb
    for i in range(N):
        out[:, 11 + 3 * i:14 + 3 * i] = H[:, 11 + 3 * i:14 + 3 * i] @ Jl[i]
    return out


def _obj(A):
    return np.array([[mpf(float(v)) for v in row] for row in np.atleast_2d(np.asarray(A, dtype=float))], dtype=object)


def rows(H, local, Jmp=None, use_mp=False):
    """(Ht, dHt): the rows in Sigma's coordinates (longdouble, or mpf objects with use_mp) and the entrywise bound on the device's own (fp64)"""
    H = np.atleast_2d(np.asarray(H, dtype=np.float64))
    N = (H.shape[1] - 11) // 3
    if not local:
        return (_obj(H) if use_mp else H.astype(LD)), np.zeros(H.shape)
    if use_mp:
        Jb = np.array([[mpf(int(i == j)) for j in range(11)] for i in range(11)], dtype=object)
        for r in range(2):
            for c in range(2):
                Jb[6 + r, 6 + c] = Jmp["G"][r][c]
        for r in range(3):
            for c in range(3):
                Jb[8 + r, 8 + c] = Jmp["RAt"][r][c]
        Jl = [np.array(Jmp["lm"][i], dtype=object).reshape(3, 3) for i in range(N)]
        Ht = _bd_right(_obj(H), Jb, Jl)
    else:
        Jb, Jl = cx.jacobian_ld(Jmp, N)
        Ht = _bd_right(H.astype(LD), Jb, Jl)
    Jb, Jl = cx.jacobian_ld(Jmp, N)
    Db, Dl = cx.jacobian_tol(Jmp, cc.K_J, N)
    aH = np.abs(H)
    dHt = gamma(OPS_J, U) * _bd_right(aH, np.abs(Jb).astype(np.float64), np.abs(Jl).astype(np.float64)) + _bd_right(aH, Db, Dl)
    dHt[:, :6] = 0.0  # (the bias columns are copied)
    return Ht, dHt


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------
def reference(Sigma, Ht, resid, R, use_mp=False):
    """Steps 1-5 from the definitions in longdouble (or mpmath).  Sigma (n x n doubles, read as stored), Ht from rows(), resid (m), R (m x m:
    lower triangle).  Returns a dict of arrays in the arithmetic used."""
    m = Ht.shape[0]
    Rl = np.tril(np.asarray(R, dtype=np.float64).reshape(m, m))
    Rl = Rl + np.tril(Rl, -1).T
    if use_mp:
        S1, Rm, r = _obj(Sigma), _obj(Rl), _obj(np.asarray(resid, dtype=float).reshape(1, -1))[0]
        sqrt, log = mp.sqrt, mp.log
    else:
        S1, Rm, r = np.asarray(Sigma, dtype=LD), Rl.astype(LD), np.asarray(resid, dtype=LD).reshape(-1)
        sqrt, log = np.sqrt, np.log
    Bt = (S1 @ Ht.T).T
    S = Ht @ Bt.T + Rm
    S = np.tril(S) + np.tril(S, -1).T
    L = ux.chol(S, sqrt)
    Y = ux.solve_lower(L, Bt)
    z = ux.solve_lower(L, r)
    gam = Y.T @ z
    Sp = S1 - Y.T @ Y
    nis = z @ z
    logdet = 2 * sum(log(L[k, k]) for k in range(m))
    c = mp.log(2 * mp.pi) if use_mp else cx.ld(mp.log(2 * mp.pi))
    return dict(m=m, S1=S1, Ht=Ht, R=Rm, resid=r, B=Bt, S=S, L=L, Y=Y, z=z, gamma=gam, Sp=Sp, nis=nis, logdet_S=logdet,
                loglik=-(nis + logdet + m * c) / 2)


# ---- the bound -------------------------------------------------------------------------------------------------------------------------------
def bounds(ref, dHt, c_log=cc.C_LOG):
    """{"Sp", "gamma", "nis", "logdet_S", "loglik", "validity"}: the entrywise bounds of the module docstring (fp64) from reference()'s
    longdouble result and rows()' dHt."""
    u = U
    f64 = ux.f64
    m = ref["m"]
    a = lambda k: np.abs(f64(ref[k]))  # noqa: E731
    aS1, aH, aB, aL, aY, az = a("S1"), a("Ht"), a("B"), a("L"), a("Y"), a("z")
    n = aS1.shape[0]
    L = ref["L"]
    Kt = ux.solve_upper_t(L, ref["Y"])            # L^-T Y = K^T (m x n)
    w = ux.solve_upper_t(L, ref["z"])
    aK, aw = np.abs(f64(Kt)).T, np.abs(f64(w))
    dB = gamma(n, u) * (aH @ aS1.T) + dHt @ aS1.T  # (B = Sigma Ht^T: row k of Bt is sum_j Sigma_ij Ht_kj)
    dS = dB @ aH.T + gamma(n + 1, u) * (aB @ aH.T) + aB @ dHt.T
    dS = np.maximum(dS, dS.T)
    E1 = ux._mirror_lower(gamma(m + 1, u) * (aL @ aL.T))
    E2 = gamma(m, u) * (aL @ aY)
    E2z = gamma(m, u) * (aL @ az)
    E3 = gamma(m, u) * (aY.T @ aY) + u * np.abs(f64(ref["Sp"]))
    D = dS + E1
    Gm = aK @ (dB + E2)
    out = {"Sp": Gm + Gm.T + aK @ D @ aK.T + E3}
    out["gamma"] = aK @ E2z + (dB + E2).T @ aw + aK @ (D @ aw) + gamma(m, u) * (aY.T @ az)
    nis, logdet = float(ref["nis"]), float(ref["logdet_S"])
    out["nis"] = float(2 * aw @ E2z + aw @ D @ aw + gamma(m, u) * abs(nis))
    Linv = f64(ux.solve_lower(L, np.eye(m, dtype=LD)))
    aSinv = np.abs(Linv.T @ Linv)
    logs = np.abs(np.log(np.diag(f64(L))))
    out["logdet_S"] = float(np.sum(aSinv * D) + 2 * np.sum(c_log * u * (1 + logs)) + gamma(m, u) * 2 * np.sum(logs))
    out["loglik"] = 0.5 * (out["nis"] + out["logdet_S"]) + 0.5 * 4 * u * (abs(nis) + abs(logdet) + m * LOG2PI)
    aLinv = np.abs(Linv)
    out["validity"] = float((aLinv @ D @ aLinv.T).max())
    return out


def ratios(got, ref, bnd):
    """{"Sp", "gamma", "nis", "logdet_S", "loglik"} -> worst |got - ref| / bound (update_exact.worst_ratio's rules: a zero bound wants the
    reference's value exactly, a NaN is outside every bound); got: dict with Sigma (n x n), gamma (n), nis, logdet_S, loglik."""
    out = {"Sp": ux.worst_ratio(got["Sigma"], ref["Sp"], bnd["Sp"])[0], "gamma": ux.worst_ratio(got["gamma"], ref["gamma"], bnd["gamma"])[0]}
    for k in ("nis", "logdet_S", "loglik"):
        out[k] = ux.worst_ratio(np.array([got[k]]), np.array([ref[k]], dtype=LD), np.array([bnd[k]]))[0]
    return out


# ---- a numpy (fp64) model of the kernels' blocking ----------------------------------------------------------------------------------------
FAULTS = ("j_left", "scale_not_inverted", "h11_on_pad", "last_tile_dropped", "mirror_not_written", "y_last_row_dropped", "r_upper_read",
          "gamma_sign", "gated_downdated")


def _to_padded(v):
    """last axis: reference index map -> padded (a zero at 11)"""
    v = np.asarray(v, dtype=np.float64)
    return np.concatenate([v[..., :11], np.zeros(v.shape[:-1] + (1,)), v[..., 11:]], axis=-1)


def model(Sigma, H, resid, R, local, blocks=None, gate=np.inf, fault=None):
    """The launches of csrc/eqf_linear.hpp in numpy fp64, with their tiles, chunks and loop orders (numpy's own summation inside a chunk): H
    (m x n, reference map), blocks = the fp64 J blocks (dict G, RAt, lm) for local.  Returns dict(Sigma (n x n, reference map), gamma (n),
    nis, logdet_S, loglik, info, pad_zero: the padded image's row / column 11 and gamma's entry 11 are exact zeros).  `fault`: one of FAULTS."""
    H = np.atleast_2d(np.asarray(H, dtype=np.float64))
    m, nref = H.shape
    N = (nref - 11) // 3
    n = nref + 1
    Sg = np.asarray(Sigma, dtype=np.float64)
    S = np.zeros((n, n))
    keep = [i for i in range(n) if i != 11]
    S[np.ix_(keep, keep)] = Sg
    # k_lin_rows
    Hp = np.zeros((ROWS, n))
    Hr = np.zeros((ROWS, nref))
    Hr[:m] = H
    if local:
        G, RAt, lm = np.asarray(blocks["G"]), np.asarray(blocks["RAt"]), np.asarray(blocks["lm"]).reshape(-1, 3, 3)
        if fault == "scale_not_inverted":  # a_i R^T in place of a_i^-1 R^T
            sc = np.array([np.linalg.norm(lm[i][:, 0]) for i in range(N)])
            lm = lm / (sc ** 2)[:, None, None]
        Hp[:, :6] = Hr[:, :6]
        if fault == "j_left":
            Hp[:, 6:8] = Hr[:, 6:8] @ G.T
            Hp[:, 8:11] = Hr[:, 8:11] @ RAt.T
            for i in range(N):
                Hp[:, 12 + 3 * i:15 + 3 * i] = Hr[:, 11 + 3 * i:14 + 3 * i] @ lm[i].T
        else:
            Hp[:, 6:8] = Hr[:, 6:8] @ G
            Hp[:, 8:11] = Hr[:, 8:11] @ RAt
            for i in range(N):
                Hp[:, 12 + 3 * i:15 + 3 * i] = Hr[:, 11 + 3 * i:14 + 3 * i] @ lm[i]
    else:
        Hp = _to_padded(Hr)
    if fault == "h11_on_pad" and nref > 11:  # the reference map's column 11 lands on the pad, everything behind it one to the left
        Hp[:, 11:n - 1] = Hp[:, 12:n].copy()
        Hp[:, n - 1] = 0.0
    # k_lin_gain: 64-row tiles, 64-column chunks ascending
    Bt = np.zeros((ROWS, n))
    nt = -(-n // TILE)
    for t in range(nt):
        if fault == "last_tile_dropped" and t == nt - 1 and n % TILE:
            continue
        r0, r1 = TILE * t, min(TILE * (t + 1), n)
        acc = np.zeros((r1 - r0, ROWS))
        for c0 in range(0, n, TILE):
            c1 = min(c0 + TILE, n)
            acc = acc + S[r0:r1, c0:c1] @ Hp[:, c0:c1].T
        Bt[:, r0:r1] = acc.T
    # k_lin_solve
    Rp = np.eye(ROWS)
    Rm = np.asarray(R, dtype=np.float64).reshape(m, m)
    Rp[:m, :m] = np.tril(Rm.T if fault == "r_upper_read" else Rm)
    A = Rp.copy()
    for c0 in range(0, n, TILE):
        c1 = min(c0 + TILE, n)
        A = A + Hp[:, c0:c1] @ Bt[:, c0:c1].T
    A = np.tril(A)
    Lm = A.copy()
    bad = False
    for j in range(ROWS):
        d = Lm[j, j]
        if not (d > 0 and np.isfinite(d)):
            bad = True
            break
        Lm[j, j] = np.sqrt(d)
        Lm[j + 1:, j] = Lm[j + 1:, j] / Lm[j, j]
        for l in range(j + 1, ROWS):
            Lm[l:, l] = Lm[l:, l] - Lm[l:, j] * Lm[l, j]
    info = 1 if bad else 0
    out = dict(Sigma=Sg.copy(), gamma=np.zeros(nref), nis=np.nan, logdet_S=np.nan, loglik=np.nan, info=info, pad_zero=True)
    if bad:
        return out
    rp = np.zeros(ROWS)
    rp[:m] = np.asarray(resid, dtype=np.float64).reshape(-1)
    z = np.zeros(ROWS)
    Y = np.zeros((ROWS, n))
    for r in range(ROWS):
        z[r] = (rp[r] - Lm[r, :r] @ z[:r]) / Lm[r, r]
        Y[r] = (Bt[r] - Lm[r, :r] @ Y[:r]) / Lm[r, r]
    if fault == "y_last_row_dropped" and m == 15:
        Y[m - 1] = 0.0
    gam = np.zeros(n)
    for r in range(ROWS):
        gam = gam + Y[r] * z[r]
    if fault == "gamma_sign":
        gam = -gam
    nis = 0.0
    for r in range(m):
        nis = nis + z[r] * z[r]
    logdet = 2.0 * float(np.sum(np.log(np.diag(Lm)[:m])))
    out.update(nis=nis, logdet_S=logdet, loglik=-0.5 * (nis + logdet + m * 1.8378770664093453))
    if not (np.isfinite(nis) and np.isfinite(Y).all() and np.isfinite(gam).all()):
        out["info"] = 1
        return out
    if nis > gate:
        out["info"] = 2
        if fault != "gated_downdated":
            return out
    # k_lin_downdate: the lower triangle of 64 x 64 tiles, mirror from the same numbers
    Sp = S.copy()
    for I in range(nt):
        for J in range(I + 1):
            i0, i1, j0, j1 = TILE * I, min(TILE * (I + 1), n), TILE * J, min(TILE * (J + 1), n)
            T = S[i0:i1, j0:j1] - Y[:, i0:i1].T @ Y[:, j0:j1]
            if I == J:
                T = np.tril(T)
                Sp[i0:i1, j0:j1] = T + np.tril(T, -1).T if fault != "mirror_not_written" else T + np.triu(S[i0:i1, j0:j1], 1)
            else:
                Sp[i0:i1, j0:j1] = T
                if fault != "mirror_not_written":
                    Sp[j0:j1, i0:i1] = T.T
    out["pad_zero"] = bool(not Sp[11].any() and not Sp[:, 11].any() and gam[11] == 0.0)
    out["Sigma"] = Sp[np.ix_(keep, keep)]
    if out["info"] == 0:
        out["gamma"] = gam[keep]
    return out
