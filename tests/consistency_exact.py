"""TEST INFRASTRUCTURE ONLY -- references and a-priori, per-entry bounds for the getters a filter is JUDGED by.  mpmath (50 digits) and
np.longdouble only; nothing of oracle/ is imported here.

PART A.  Sigma_loc = J Sigma J^T (csrc/eqf_local.hpp: eqf_get_sigma_local, eqf_get_marginals, eqf_get_local_jacobian).

THE REFERENCE.  J is block diagonal: I (6, bias), G (2 x 2, gravity direction), R_A^T (velocity), a_i^-1 R(q_i)^T per landmark.  Its blocks
come from the DEFINITIONS with the primitives of tests/lie_exact.py at 50 digits,
    eta0 = R_P0^T e3, etaHat = R_A^T eta0,   G = chart_diff(etaHat, etaHat) R_A^T chart_inv_diff_at_zero(eta0),
each entry rounded ONCE to np.longdouble; Sigma_loc is then formed block by block in longdouble.  Its own error is
(gamma_6(2^-64) + 2 x 2^-64) |J| |Sigma| |J|^T, 2^-11 of the first term of the bound below: neglected (REF_SLACK adds it back).

THE BOUND, per entry.  Write the device's blocks as J + dJ:
    |Sigma_loc_dev - Sigma_loc_ref| <= gamma_k (|J| |Sigma| |J|^T) + |dJ| |Sigma| |J|^T + |J| |Sigma| |dJ|^T
(first order in dJ: the dropped |dJ| |Sigma| |dJ|^T is K_J u times the terms kept).
k counts the rounded operations through which one term J_ia Sigma_ab J_jb reaches the output entry in eqf_local.hpp:
    3   the left stage:  T_ib = dot3(J_i0, S_0b, J_i1, S_1b, J_i2, S_2b) = fma(., ., fma(., ., . * .)): one product and two fused steps
        (localBlock's first loop; U[r][k] for Sigma_Jb; baseApply for a base row: two roundings for the gravity rows, three for the
        velocity rows, none for the bias rows)
    3   the right stage: out_ij = dot3(T_i0, J_j0, ...) likewise (localBlock's second loop; colOut's dot3; baseApply on the stage's result)
    k = K_LOCAL = 6: two three-term product stages, one per side.  Nothing else is rounded: J_J sits in registers, J_I in LDS, as stored.
|dJ| <= K_J u max|block| on the positions that block occupies (zero on the bias identity), one constant each for G, R_A^T and the landmark
blocks, measured from the numpy ORACLE and stored in consistency_cases.py.  G's takes the form K_J (u / theta^2) max|G| of DESIGN section 5,
theta the smaller of the angles of eta0 and etaHat from e3, the point where the minimal rotation -pole -> e3 is a half turn.
Where the bound is exactly zero (family c: every Sigma block that could reach the entry is zero) the value must be exactly zero.

PART B.  eqf_get_nees, eqf_sample_sigma, eqf_perturb_filters (csrc/eqf_nees.hpp, csrc/eqf_sample.hpp).

THE REFERENCE.  A is the lower triangle of the device's own sigma(b) / sigma_local(b), cut at `first` and mirrored (n = 11 + 3 N - first).
L = chol(A), z = L^-1 e, x = L^-T z = A^-1 e in np.longdouble with update_exact.chol / solve_lower / solve_upper_t; for n <= MP_MAX_ORDER the
same in mpmath at 50 digits, and |longdouble - mpmath| is asserted below 1 % of every bound (FactorRef.mp_share).

THE BOUNDS, first order and componentwise.  The kernels factor the matrix with the structural pad row (a row of the identity at internal
index 11, when first < 11) in place: m = n + 1 (first = 0, 6) or n (first = 11) is the order they see, and the 16 x 16 diagonal blocks of
chol_bounds.block_T are those of the PADDED matrix (T below is block_T of the padded factor with the pad row and column removed).
u = 2^-53, p = chol_bounds.P, gamma_k = k u / (1 - k u).
    E1  = mirror(((m + 1) u + p)(|L||L|^T) T^T)        the factorisation bound of tests/chol_bounds.py: Lh Lh^T = A + dA, |dA| <= E1
    E2  = (m + 16) u T (|L||z| + |e|)                  its left-solve bound: Lh zh = e + r, |r| <= E2   (the error vectors ride as sixteen more
                                                       rows of the panel: e^T Lh^-T, the same solve transposed)
    Phi(X) = the lower triangle of X with its diagonal halved;   dL = |L| Phi(|L^-1| E1 |L^-T|)
        [Lh = L + dL':  L^-1 dA L^-T = L^-1 dL' + (L^-1 dL')^T to first order, L^-1 dL' lower triangular, so L^-1 dL' = Phi(L^-1 dA L^-T)]
  NEES.  zh^T zh = (e + r)^T (A + dA)^-1 (e + r) = e^T A^-1 e - x^T dA x + 2 x^T r + second order, then the sum of squares of the tail:
    |d nees| <= |x|^T E1 |x| + 2 |x|^T E2 + gamma_s nees,    s = ceil(m / 16) + 4
        k_nees_tail: vector k is summed by sixteen lanes, lane l takes the entries l, l + 16, ... with one fma each (ceil(m / 16) roundings;
        the square is fused), then the tree w = 8, 4, 2, 1 (four additions)
  LOG DET.  log det(A + dA) = log det A + tr(A^-1 dA) + second order; then the logarithms and their sum:
    |d logdet| <= sum_ij |A^-1|_ij E1_ij + 2 sum_k c_log u (1 + |log L_kk|) + gamma_t 2 sum_k |log L_kk|,    t = ceil(m / 256) + 8
        k_nees_tail: thread t takes the pivots t, t + 256, ... in sequence (ceil(m / 256) additions), then the tree w = 128 .. 1 (eight); the
        factor 2 is exact.  c_log = 4 x the worst error of numpy's log against mp.log over the committed pivots in units of u (1 + |log l|),
        stored in consistency_cases.py (C_LOG) and re-measured by tests/test_consistency_exact.py
  MIN PIVOT.  in [min_k (L_kk^2 - d_k), min_k (L_kk^2 + d_k)],  d_k = 2 L_kk dL_kk + 2 u L_kk^2  (the pad's 1.0 is no pivot)
  DRAWS.  eps = s Lh zeta:   |eps - s L zeta| <= |s| (dL |zeta| + gamma_{m+2} |L||zeta|) + u |eps|   per entry
        (k_sample_trmm: m products summed in a fixed order on the matrix cores, one more for the split over block columns, one for the scale)
  Entries of eps below `first` must be exactly 0, entries from 11 + 3 N_b on untouched.
First order is licensed per case by the asserted condition  max(|L^-1| E1 |L^-T|) <= 1e-3  (FactorRef.validity).

PART C.  eqf_get_innovation_stats (csrc/eqf_innov.hpp) of ONE vision call.

THE REFERENCE is update_exact.Case / update_reference for the same call (S, L, z, delta in longdouble, the propagate's entrywise bound E_ric):
nis = z^T z, logdet_S = 2 sum log L_kk, nis_lm[i] = delta_i^T S_ii^-1 delta_i from the 2 x 2 diagonal block of S, loglik from the three.
THE BOUNDS are made of the parts update_exact.update_bounds already computes (bounds["parts"]: dS, E1, E2z, ddelta, aw = |S^-1 delta|, CEC =
|C| E_ric |C|^T, T); nothing of them is derived again.  With D = dS + E1 + CEC:
    |d nis|       <= 2 |w|^T (ddelta + E2z) + |w|^T D |w| + gamma_s nis,   s = ceil(m / 256) + 8
                     k_innov_stats: lane t takes the terms t, t + 256, ... with one fma each, then the tree w = 128 .. 1
    |d logdet_S|  <= sum_ij |S^-1|_ij D_ij + 2 sum_k c_log u (1 + |log L_kk|) + gamma_s 2 sum_k |log L_kk|      (the same order of summation)
    |d nis_lm[i]| <= 2 |w_i|^T ddelta_i + |w_i|^T (dS_ii + gamma_8 |S_ii|) |w_i| + gamma_8 nis_lm[i],   w_i = S_ii^-1 delta_i
                     dS_ii WITHOUT E1: the kernel factors the 2 x 2 block itself.  8 = the rounded operations on the longest path from the
                     block to the output in k_innov_stats: sqrt (l00), division (l10), fma and sqrt (l11), division (w0), fma and division
                     (w1), fma (w1^2 + w0^2); |L||L^T| = |S_ii| exactly for a 2 x 2 factor.  The propagate's E_ric is NOT in this bound, as
                     the check was specified, although the kernel reads the propagated Sigma: (|C| E_ric |C|^T)_ii reaches 5 dS_ii on the
                     committed cases (tests/test_consistency_exact.py prints it).  The fp64 oracle and the device use a tenth of the bound.
    loglik = -(nis + logdet_S + m log 2 pi) / 2:  (d nis + d logdet_S) / 2 + 4 u (|nis| + |logdet_S| + m log 2 pi) / 2"""
import numpy as np
from mpmath import mp, mpf

import chol_bounds as cb
import lie_exact as lx
import update_exact as ux
from riccati_exact import LD, gamma

U = 2.0 ** -53
K_LOCAL = 6
MP_MAX_ORDER = 60
VALIDITY = 1e-3
REF_SLACK = 8 * 2.0 ** -64


def ld(x):
    """mpf -> longdouble, one rounding"""
    hi = float(x)
    return LD(hi) + LD(float(x - hi))


def ldm(A):
    return np.array([[ld(x) for x in row] for row in A], dtype=LD)


# ---- part A ---------------------------------------------------------------------------------------------------------------------------------
def jacobian_mp(origin, group):
    """The blocks of J at 50 digits from the dictionaries of FilterBatch.origin() / group() (exact doubles):
    dict(G (2 x 2), RAt (3 x 3), lm [N of 3 x 3] -- lists of mpf -- and theta0, thetaHat: the angles of eta0 and etaHat from e3)."""
    RP0, RA = lx.rot_of_quat(origin["q"]), lx.rot_of_quat(group["Aq"])
    RAt = lx.tr(RA)
    eta0 = lx.mv(lx.tr(RP0), lx.E3())
    etaHat = lx.mv(RAt, eta0)
    G = lx.mm(lx.mm(lx.chart_diff(etaHat, etaHat), RAt), lx.chart_inv_diff_at_zero(eta0))
    lm = []
    for q, a in zip(np.asarray(group["Qq"]).reshape(-1, 4), np.asarray(group["Qa"]).reshape(-1)):
        lm.append(lx.mscl(1 / mpf(float(a)), lx.tr(lx.rot_of_quat(q))))
    ang = lambda e: float(mp.atan2(mp.sqrt(e[0] ** 2 + e[1] ** 2), e[2]))  # noqa: E731
    return dict(G=G, RAt=RAt, lm=lm, theta0=ang(eta0), thetaHat=ang(etaHat))


def jacobian_ld(Jmp, N=None):
    """(Jb (11 x 11), Jl (N, 3, 3)) in longdouble from jacobian_mp's blocks (the first N landmarks)."""
    N = len(Jmp["lm"]) if N is None else N
    Jb = np.eye(11, dtype=LD)
    Jb[6:8, 6:8] = ldm(Jmp["G"])
    Jb[8:11, 8:11] = ldm(Jmp["RAt"])
    Jl = np.zeros((N, 3, 3), dtype=LD)
    for i in range(N):
        Jl[i] = ldm(Jmp["lm"][i])
    return Jb, Jl


def jacobian_tol(Jmp, K, N=None):
    """|dJ| as (Db (11 x 11), Dl (N, 3, 3)), fp64: K u max|block| on the block's positions, G's with u / theta^2."""
    N = len(Jmp["lm"]) if N is None else N
    th = min(Jmp["theta0"], Jmp["thetaHat"])
    Db = np.zeros((11, 11))
    Db[6:8, 6:8] = K["G"] * U / th ** 2 * float(max(abs(x) for r in Jmp["G"] for x in r))
    Db[8:11, 8:11] = K["RAt"] * U * float(max(abs(x) for r in Jmp["RAt"] for x in r))
    Dl = np.zeros((N, 3, 3))
    for i in range(N):
        Dl[i] = K["lm"] * U * float(max(abs(x) for r in Jmp["lm"][i] for x in r))
    return Db, Dl


def jacobian_ratios(blocks, Jmp):
    """A set of fp64 J blocks (dict G, RAt, lm (N, 3, 3)) against the 50-digit ones: {"G", "RAt", "lm"} -> worst error in units of u max|block|
    (G: (u / theta^2) max|G|)."""
    th = min(Jmp["theta0"], Jmp["thetaHat"])

    def err(got, want):
        g = np.asarray(got, dtype=float)
        e = max(abs(mpf(float(g[i, j])) - want[i][j]) for i in range(len(want)) for j in range(len(want[0])))
        return e / max(abs(x) for r in want for x in r)

    out = {"G": float(err(blocks["G"], Jmp["G"]) * mpf(th) ** 2 / mpf(U)), "RAt": float(err(blocks["RAt"], Jmp["RAt"]) / mpf(U)), "lm": 0.0}
    for i in range(len(blocks["lm"])):
        out["lm"] = max(out["lm"], float(err(blocks["lm"][i], Jmp["lm"][i]) / mpf(U)))
    return out


def bd_left(Jb, Jl, M):
    """J M for the block-diagonal J = diag(Jb, Jl[0], Jl[1], ...), in the dtype of the operands, O(3 n^2)."""
    N = len(Jl)
    out = np.empty((11 + 3 * N, M.shape[1]), dtype=np.result_type(Jb.dtype, M.dtype))
    out[:11] = Jb @ M[:11]
    if N:
        out[11:] = np.einsum("iab,ibc->iac", Jl, M[11:].reshape(N, 3, M.shape[1])).reshape(3 * N, M.shape[1])
    return out


def bd_sandwich(Ab, Al, M, Bb, Bl):
    """A M B^T for block-diagonal A, B."""
    return bd_left(Bb, Bl, bd_left(Ab, Al, M).T).T


def sigma_local_reference(Jmp, S):
    """(Sigma_loc in longdouble, the dense fp64 J for reporting) from jacobian_mp's blocks and the device's own sigma()."""
    N = (len(S) - 11) // 3
    Jb, Jl = jacobian_ld(Jmp, N)
    return bd_sandwich(Jb, Jl, np.asarray(S, dtype=LD), Jb, Jl)


def sigma_local_bound(Jmp, S, K):
    """The per-entry bound of the module docstring (fp64) and the older yardstick 256 u |J| |Sigma| |J|^T, for S = the device's sigma()."""
    N = (len(S) - 11) // 3
    Jb, Jl = jacobian_ld(Jmp, N)
    Ab, Al = np.abs(Jb).astype(np.float64), np.abs(Jl).astype(np.float64)
    Db, Dl = jacobian_tol(Jmp, K, N)
    aS = np.abs(np.asarray(S, dtype=np.float64))
    core = bd_sandwich(Ab, Al, aS, Ab, Al)
    bound = (gamma(K_LOCAL, U) + REF_SLACK) * core + bd_sandwich(Db, Dl, aS, Ab, Al) + bd_sandwich(Ab, Al, aS, Db, Dl)
    return bound, 256 * U * core


def bound_ratio(got, ref, bound):
    """(worst |got - ref| / bound over the entries with bound > 0, number of entries with bound == 0 whose value is not exactly zero)."""
    diff = np.abs(np.asarray(got, dtype=LD) - ref)
    pos = bound > 0
    r = float((diff[pos] / bound[pos]).max()) if pos.any() else 0.0
    return (np.inf if np.isnan(r) else r), int(np.count_nonzero(np.asarray(got)[~pos]))


def dense_J(blocks, N):
    """dense fp64 J from a dict of fp64 blocks"""
    J = np.zeros((11 + 3 * N, 11 + 3 * N))
    J[:6, :6] = np.eye(6)
    J[6:8, 6:8] = blocks["G"]
    J[8:11, 8:11] = blocks["RAt"]
    for i in range(N):
        J[11 + 3 * i:14 + 3 * i, 11 + 3 * i:14 + 3 * i] = blocks["lm"][i]
    return J


# ---- part B ---------------------------------------------------------------------------------------------------------------------------------
def cut(S, first):
    """the trailing principal submatrix from reference index `first`, from the LOWER triangle of S, mirrored"""
    A = np.tril(np.asarray(S, dtype=np.float64)[first:, first:])
    return A + np.tril(A, -1).T


def pad_index(first):
    """index of the structural pad row inside the submatrix the kernels factor (-1: not part of it)"""
    return 11 - first if first < 11 else -1


def embed(M, pad):
    """M with a row and column of the identity inserted at `pad`"""
    if pad < 0:
        return np.array(M, copy=True)
    n = len(M)
    keep = [i for i in range(n + 1) if i != pad]
    out = np.zeros((n + 1, n + 1), dtype=M.dtype)
    out[np.ix_(keep, keep)] = M
    out[pad, pad] = 1
    return out


def strip(M, pad):
    return M if pad < 0 else np.delete(np.delete(M, pad, 0), pad, 1)


def mirror_lower(E):
    return np.tril(E) + np.tril(E, -1).T


def phi(X):
    out = np.tril(X)
    out[np.diag_indices(len(X))] *= 0.5
    return out


def ops_nees(m):
    return -(-m // 16) + 4


def ops_logdet(m):
    return -(-m // 256) + 8


class FactorRef:
    """The reference factor of A (fp64, symmetric, order n >= 1) and everything the bounds of part B need from it."""

    def __init__(self, A, first, c_log):
        self.A, self.first, self.n = A, first, len(A)
        self.pad = pad_index(first)
        self.m = m = self.n + (1 if self.pad >= 0 else 0)
        self.L = L = ux.chol(A.astype(LD), np.sqrt)
        self.Linv = cb.inv_lower(L)
        self.aL, aLi = np.abs(L).astype(np.float64), np.abs(self.Linv).astype(np.float64)
        self.T = strip(cb.block_T(embed(L, self.pad)), self.pad)
        self.E1 = mirror_lower(((m + 1) * U + cb.P) * np.tril((self.aL @ self.aL.T) @ self.T.T))
        M = aLi @ self.E1 @ aLi.T
        self.validity = float(M.max())
        self.dL = self.aL @ phi(M)
        self.absAinv = np.abs(self.Linv.T @ self.Linv).astype(np.float64)
        d = np.diag(L)
        self.logs = np.log(d)
        self.logdet = 2 * self.logs.sum()
        al = np.abs(self.logs).astype(np.float64)
        self.logdet_bound = float((self.absAinv * self.E1).sum() + 2 * c_log * U * (1 + al).sum() + gamma(ops_logdet(m), U) * 2 * al.sum())
        d64 = d.astype(np.float64)
        dk = 2 * d64 * np.diag(self.dL) + 2 * U * d64 ** 2
        self.min_pivot = (float((d64 ** 2 - dk).min()), float((d64 ** 2 + dk).min()))
        self.kappa = float(np.linalg.cond(A))
        self.old = self.n * U * self.kappa

    def nees(self, E):
        """E (k, n): (nees in longdouble (k,), bound (k,), x (n, k))"""
        Et = np.asarray(E, dtype=LD).T
        z = ux.solve_lower(self.L, Et)
        x = ux.solve_upper_t(self.L, z)
        ne = (z * z).sum(axis=0)
        az, ax, aE = (np.abs(v).astype(np.float64) for v in (z, x, Et))
        E2 = (self.m + 16) * U * (self.T @ (self.aL @ az + aE))
        bound = np.einsum("ik,ij,jk->k", ax, self.E1, ax) + 2 * (ax * E2).sum(axis=0) + gamma(ops_nees(self.m), U) * ne.astype(np.float64)
        return ne, bound

    def draw(self, Z, scale):
        """Z (k, n): (scale L z in longdouble (k, n), bound without the u |eps| term (k, n))"""
        Zt = np.asarray(Z, dtype=LD).T
        eps = LD(scale) * (self.L @ Zt)
        az = np.abs(Zt).astype(np.float64)
        bound = abs(scale) * (self.dL @ az + gamma(self.m + 2, U) * (self.aL @ az))
        return eps.T, bound.T

    def mp_share(self, E):
        """n <= MP_MAX_ORDER: the factorisation and the solve once more in mpmath at 50 digits; the largest |longdouble - mpmath| / bound over
        nees, logdet and the pivots' squares (against d_k): the share of the bound that the reference's own arithmetic could take."""
        assert self.n <= MP_MAX_ORDER
        A = np.array([[mpf(float(v)) for v in row] for row in self.A], dtype=object)
        L = ux.chol(A, mp.sqrt)
        Et = np.array([[mpf(float(v)) for v in row] for row in np.asarray(E, dtype=np.float64).T], dtype=object)
        z = ux.solve_lower(L, Et)
        ne_ld, nb = self.nees(E)
        share = 0.0
        for k in range(Et.shape[1]):
            ne = sum(z[i, k] * z[i, k] for i in range(self.n))
            share = max(share, float(abs(ne - mpf(float(ne_ld[k])) - mpf(float(ne_ld[k] - LD(float(ne_ld[k]))))) / mpf(float(nb[k]))))
        ld_ = 2 * sum(mp.log(L[i, i]) for i in range(self.n))
        share = max(share, float(abs(ld_ - mpf(float(self.logdet)) - mpf(float(self.logdet - LD(float(self.logdet))))) / mpf(self.logdet_bound)))
        d64 = np.diag(self.L).astype(np.float64)
        dk = 2 * d64 * np.diag(self.dL) + 2 * U * d64 ** 2
        for i in range(self.n):
            li = np.diag(self.L)[i]
            share = max(share, float(abs(L[i, i] ** 2 - (mpf(float(li)) + mpf(float(li - LD(float(li))))) ** 2) / mpf(float(dk[i]))))
        return share


def nees_ratios(ref, got_nees, got_logdet, got_min_pivot, E):
    """A result (nees (k,), logdet, min_pivot) against FactorRef: dict of ratios to the new bounds (<= 1 passes; min_pivot: distance outside
    the interval in units of its half width, 0 inside) and, under "old", to the yardstick n u kappa_2 the older tests use."""
    ne, nb = ref.nees(E)
    dn = np.abs(np.asarray(got_nees, dtype=LD) - ne).astype(np.float64)
    out = {"nees": float((dn / nb).max()), "logdet": float(abs(LD(got_logdet) - ref.logdet)) / ref.logdet_bound}
    lo, hi = ref.min_pivot
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    out["min_pivot"] = abs(got_min_pivot - mid) / half
    mp_ref = float((np.diag(ref.L) ** 2).min())
    out["old"] = {"nees": float((dn / (ref.old * ne.astype(np.float64))).max()), "logdet": float(abs(LD(got_logdet) - ref.logdet)) / ref.old,
                  "min_pivot": abs(got_min_pivot - mp_ref) / (ref.old * mp_ref)}
    out["bound_vs_old"] = {"nees": float((nb / (ref.old * ne.astype(np.float64))).max()), "logdet": ref.logdet_bound / ref.old}
    for k in ("nees", "logdet", "min_pivot"):
        if np.isnan(out[k]):
            out[k] = np.inf
    return out


def draw_ratios(ref, got_eps, Z, scale):
    """eps (k, n) against FactorRef.draw: {"draw": worst entry / bound, "old": worst |.|_2 / (n u kappa |L|_2 |z|_2 |s|), "bound_vs_old"}"""
    eps, bound = ref.draw(Z, scale)
    got = np.asarray(got_eps, dtype=np.float64)
    bound = bound + U * np.abs(got)
    diff = np.abs(got.astype(LD) - eps).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bound > 0, diff / bound, np.where(diff == 0, 0.0, np.inf))
    q = np.where(np.isnan(q), np.inf, q)
    nL = float(np.linalg.norm(ref.aL, 2))
    old = ref.old * nL * np.linalg.norm(np.asarray(Z, dtype=np.float64), axis=1) * abs(scale)
    return {"draw": float(q.max()), "old": float((np.linalg.norm(diff, axis=1) / old).max()),
            "bound_vs_old": float((np.linalg.norm(bound, axis=1) / old).max())}


def log_error_units(pivots):
    """worst |numpy log - mp.log| / (u (1 + |log l|)) over an array of fp64 pivots"""
    worst = 0.0
    for l in np.asarray(pivots, dtype=np.float64):
        t = mp.log(mpf(float(l)))
        worst = max(worst, float(abs(mpf(float(np.log(l))) - t) / (mpf(U) * (1 + abs(t)))))
    return worst


# ---- part C ---------------------------------------------------------------------------------------------------------------------------------
OPS_LM = 8
LOG_2PI = 1.8378770664093453


def ops_innov(m):
    return -(-m // 256) + 8


def innovation_stats_reference(ref, bounds, c_log):
    """{nis, logdet_S, loglik, nis_lm} in longdouble and {..} their bounds (fp64) from update_exact's reference and update_bounds' parts."""
    P = bounds["parts"]
    N = ref["N"]
    m = 2 * N
    L, z, S, delta = ref["L"], ref["z"], ref["S"], ref["delta"]
    D = P["dS"] + P["E1"] + P["CEC"]
    aw = P["aw"]
    nis = (z * z).sum()
    logs = np.log(np.diag(L))
    logdet = 2 * logs.sum()
    al = np.abs(logs).astype(np.float64)
    s = ops_innov(m)
    b_nis = 2 * aw @ (P["ddelta"] + P["E2z"]) + aw @ D @ aw + gamma(s, U) * float(nis)
    Linv = cb.inv_lower(L).astype(np.float64)
    b_ld = float((np.abs(Linv.T @ Linv) * D).sum() + 2 * c_log * U * (1 + al).sum() + gamma(s, U) * 2 * al.sum())
    nis_lm, b_lm = np.zeros(N, dtype=LD), np.zeros(N)
    for i in range(N):
        k = slice(2 * i, 2 * i + 2)
        Sii, di = S[k, k], delta[k]
        det = Sii[0, 0] * Sii[1, 1] - Sii[1, 0] * Sii[1, 0]
        wi = np.array([Sii[1, 1] * di[0] - Sii[1, 0] * di[1], Sii[0, 0] * di[1] - Sii[1, 0] * di[0]], dtype=LD) / det
        nis_lm[i] = wi @ di
        awi = np.abs(wi).astype(np.float64)
        Dii = P["dS"][k, k] + gamma(OPS_LM, U) * np.abs(Sii).astype(np.float64)
        b_lm[i] = 2 * awi @ P["ddelta"][k] + awi @ Dii @ awi + gamma(OPS_LM, U) * float(nis_lm[i])
    loglik = -(nis + logdet + m * LD(LOG_2PI)) / 2
    b_ll = (b_nis + b_ld) / 2 + 2 * U * (abs(float(nis)) + abs(float(logdet)) + m * LOG_2PI)
    return (dict(nis=nis, logdet_S=logdet, loglik=loglik, nis_lm=nis_lm),
            dict(nis=float(b_nis), logdet_S=b_ld, loglik=float(b_ll), nis_lm=b_lm))


def innovation_ratios(got, val, bnd):
    """a dict with nis, logdet_S, loglik, nis_lm against the reference: {key: worst |got - ref| / bound}"""
    out = {}
    for k in ("nis", "logdet_S", "loglik"):
        out[k] = float(abs(LD(got[k]) - val[k])) / bnd[k]
    d = np.abs(np.asarray(got["nis_lm"], dtype=LD) - val["nis_lm"]).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bnd["nis_lm"] > 0, d / bnd["nis_lm"], np.where(d == 0, 0.0, np.inf))
    out["nis_lm"] = float(q.max()) if len(q) else 0.0
    return {k: (np.inf if np.isnan(v) else v) for k, v in out.items()}
