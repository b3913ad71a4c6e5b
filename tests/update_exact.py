"""TEST INFRASTRUCTURE ONLY -- one vision update entry by entry: a reference, and an a-priori bound on what any fp64 (or fp32-storage)
implementation of it may differ from that reference by.

A vision call is "integrate to the stamp, then update" (a call with dt <= 0 is skipped).  The reference composes
  the propagate   riccati_exact.ExactFilter / reference_run as they are: Sigma' in longdouble with its entrywise bound E_ric, the group
                  stepped at 50 digits;
  the update      from the DEFINITIONS (oracle/eqf_numpy.py:877-918 processVisionData, :632-684 bundle_lift), nothing rearranged the way
                  csrc/eqf_update.hpp does:
      delta_i = chart(R_Qi y_i, p0_i / |p0_i|)     C0i = chart_diff(y0, y0)(I - y0 y0^T) / |p0_i|       (lie_exact's 50-digit primitives)
      B = C Sigma'    S = B C^T + r I = L L^T    Y = L^-1 B    z = L^-1 delta    gamma = Y^T z    Sigma+ = Sigma' - Y^T Y
      Z_P (rows of landmark i) = a_i R_Qi R_C^T [ (x0 - pHat_i)^ R0 , R0 ]    K_par = [eta0 0; 0 I]    dU_fixed = [P_d gamma_e[0:2]; 0],
      P_d = -(I - eta0 eta0^T) eta0^ cInv    G = Z_P K_par    h = -[0; gamma_landmarks] - Z_P dU_fixed     (D alpha_i = -gamma_i exactly)
      Sigma_e = Sigma'[6:, 6:] = Le Le^T    M = (Le^-1 G)^T (Le^-1 G)    b = (Le^-1 G)^T (Le^-1 h)    M sol = b (one residual refinement)
      Gamma[0:6] = dU_fixed + K_par sol    Gamma[6:] = gamma[8:]
  The geometric inputs are rounded ONCE from 50 digits to np.longdouble; the linear algebra (a hand-written Cholesky, forward and backward
  substitution) runs in longdouble, or -- update_reference(..., use_mp=True), N <= 17 -- in mpmath at 50 digits on the unrounded inputs with
  Sigma' propagated at 50 digits too.  tests/test_update_exact.py asserts that the two differ by < 1 % of the bound wherever a quantity is
  asserted: that licenses longdouble at the larger sizes.

THE BOUND, first order and entrywise; nothing in it comes from the device.  m = 2 N, n = 11 + 3 N, n_e = 5 + 3 N, u = 2^-53,
gamma_k = k u / (1 - k u), K = Y^T L^-1 (the gain), w = L^-T z = S^-1 delta, T = chol_bounds.block_T(L), p = chol_bounds.P.
    dC    = tau_blk u max|C0i| on C0i's positions (riccati_exact.TAU_BLK: the rounding of a block any fp64 implementation computes from
            the state)
    dB    = gamma_3 |C||Sigma'| + dC |Sigma'|                                   3: a row of C has three non-zeros (2 additions + 1 product)
    dS    = dB |C^T| + gamma_4 |B||C^T| + |B| dC^T + u |S|                      4: the three-term dot product and the addition of r;
                                                                                u |S|: S stored once
    E1    = ((m + 1) u + p)(|L||L^T|) T^T   mirrored from the lower triangle    the factorisation bound of tests/chol_bounds.py
    E2    = (m + 16) u T (|L||Y| + |B|)                                         its left-solve bound; E2z the same for the column delta
    E3    = gamma_{m+2} |Y|^T |Y|                                               m products summed in any order, the subtraction from
                                                                                Sigma' and one more for a split of the sum over tiles
    |dSigma+| <= G + G^T + |K|(dS + E1)|K|^T + E3 + u (|Sigma'| + |Sigma+|) + |I - K C| E_ric |I - K C|^T,   G = |K|(dB + E2)
    |dgamma|  <= |K|(E2z + ddelta) + (dB + E2)^T |w| + |K|(dS + E1)|w| + gamma_{m+2} |Y|^T |z| + |I - K C| E_ric |C^T w|
    ddelta    =  K_delta u (1 + |delta|),  K_DELTA = 4 x the numpy oracle's worst ratio to the 50-digit delta over the committed cases
                 (tests/test_update_exact.py re-measures it and asserts 4 x ratio <= K_DELTA; the constant is stored unrounded)
  (m + 1, m + 16 and p are chol_bounds' counts for factor64 / solveStrip; 3, 4 and m + 2 are counted above from the structure of the
  products, 12, 6, 3 and 14 below from updateFinishBody; none is tuned to a result.)
  Gamma[0:6].  Every implementation needs the 11 x 11 Gram matrix G11 = A^T Sigma_e^-1 A of A = [Z_P | E_top] (E_top: the first five unit
  columns), hV = (C_e Z_P)^T w and gamma_e[0:5]: with them  b6 = Z_P^T Sigma_e^-1 h = -(hV - T65 gamma_e[0:5]) - G6 dU_fixed, G6 and T65
  blocks of G11, M = K_par^T G6 K_par, b = K_par^T b6.  The definitions' own  b = G^T Sigma_e^-1 h  is the same number with the same
  first-order sensitivity to gamma, because Sigma_e^-1 [0; gamma_landmarks] = C_e^T w - Sigma_e^-1 E_top gamma_e[0:5].  With V_e = Sigma_e^-1 A,
  Gt = Le^-1 A, T_e = block_T(Le), dZ = tau_blk u max|block| on every 3 x 6 block of Z_P:
    dG11  = |V_e|^T (E2_e + dZ) + (...)^T + gamma_{n_e+2} |Gt|^T |Gt|          the solves' and the products' own errors, column by column
    dV    = dC |Z_P| + |C_e| dZ + gamma_3 |C_e||Z_P|,   Kv = S^-1 V,  Yv = L^-1 V
    dhV   = (dV + E2v)^T |w| + |Kv|^T (E2z + ddelta) + |Kv|^T (dS + E1 + |C| E_ric |C^T|) |w| + gamma_{m+2} |Yv|^T |z|
    ddU   = |P_d| dgamma[6:8] + tau_blk u max|P_d| sum|gamma[6:8]|
    db6   = dhV + dT65 |g5| + dG6 |dU| + gamma_12 (|hV| + |T65||g5| + |G6||dU|)
                                                                                12 terms (hV, five of T65 g5, six of G6 dU): a product and <= 11 additions
    dM    = |K_par|^T dG6 |K_par| + gamma_6 |K_par|^T |G6| |K_par|              a column of K_par has <= 3 non-zeros: 3 + 3 for the two contractions
    The SYMMETRIC perturbations of Sigma_e -- the backward error E1_e of its ONE factor (E1_e = ((n_e + 1) u + p)(|Le||Le^T|) T_e^T) and the
    propagate's E_ric[6:, 6:] -- reach M and b together: with Sigma_e + E in place of Sigma_e, to first order
        db - dM sol = -V_G^T E Sigma_e^-1 (h - G sol),        V_G = Sigma_e^-1 G,
    the weighted least-squares RESIDUAL r = h - G sol in place of h and G sol bounded one by one.  An implementation that forms b through
    hV, T65 and G6 (the device) has hV free of Sigma_e^-1 and sees r + gamma_e, Sigma_e^-1 gamma_e = C_e^T w; the bound takes the larger
    entry of the two:   dsym = |V_G|^T (E1_e + E_ric[6:,6:]) max(|Sigma_e^-1 r|, |Sigma_e^-1 r + C_e^T w|).
    The errors of g5 = gamma_e[0:5] and of dU enter sol LINEARLY through exact matrices, which are multiplied out before the absolute value:
    with Pk = M^-1 K_par^T
    dsol  = |Pk| db6 + |Pk T65| dgamma[6:11] + |Pk G6| ddU + |M^-1| (dM |sol| + gamma_3 |K_par|^T |b6| + dsym + gamma_14 P |L||U| |sol|)
                                                                                M = P L U with partial pivoting (solve4 in csrc/eqf_update.hpp, the oracles'
                                                                                QR is no worse): gamma_n |L||U| for the elimination and gamma_n for each of the
                                                                                two substitutions [Higham, Thm 9.4: 3 n = 12], + 2 for the multipliers and
                                                                                the back substitution formed with a reciprocal.
    |dGamma[0:6]| <= ddU + |K_par| dsol + 2 u |Gamma|                           (ddU: Gamma = dU_fixed + K_par sol)
    The specification of this check wrote  |dsol| <= |M^-1|(|dM||sol| + |db| + gamma_8 |M||sol|)  with every perturbation of M and b bounded
    apart.  That form is valid and 2 .. 22 times looser: it forgets that one perturbed Sigma_e stands behind M and b (at N = 2 the E_ric term
    alone was 2e-7 |Gamma|), and it does not meet the condition bound <= 1e-7 max|Gamma[0:6]| the same specification sets.  The form above is
    the same first-order expansion with the contractions done before the absolute values; the 4 x 4 solve was recounted from the kernel.
"downdate_slices" = S (csrc/eqf_i8.hpp: Y's columns cut into S 7-bit slices, exact int32 accumulation, dropped slice pairs): E3 is
i8_emulator.bound(m, e, e, S), the rigorous bound of that construction from the exponent words e of Y's columns (about m (S + 1) 2^-7S
2^(e_i + e_j)), plus gamma_2 |Y|^T |Y| for the recombination's last addition and the subtraction.
fp32 handles (Sigma stored as float, the downdate on Y rounded to float, the factorisations and solves fp64): E3 = (gamma_{m+2}(2^-24) +
2 x 2^-24) |Y|^T |Y| and the storage term 2^-24 (|Sigma'| + |Sigma+|); E_ric is riccati_exact's fp32 bound, which already holds the rounding
of Sigma'.

The partitioned filter (csrc/eqf_tiledf.hip, Chain::step and enqueueUpdate; update_bounds(block_rows=, split_levels=, inverse_blocks=), all
defaulting to the single-GPU bound; update_cases.tiled_schedule counts them from (N, bl) and the options).  Its two factorisations are
right-looking by block ROWS of 2 bl (S) and 3 bl (Sigma_e's landmark part) rows; re-read against the counts above:
    trailing updates    X_ij -= U_ki^T U_kj is ONE LAUNCH per block row k < i: the bk products of an entry are summed from zero on the
                        matrix cores and the sum is added to X_ij by one atomic addition.  Over nbr block rows an entry's m products still
                        meet m additions in all, and no term passes more than bk + nbr - 1 <= m of them, so "m products in any order"
                        (E1, E3) holds as it stands; the addition per block row is counted on top all the same -- block_rows = nbr more
                        roundings in EVERY count (m + 1, m + 16, m + 2 and the E-chain's n_e + 1, n_e + 16, n_e + 2) -- because the
                        right-hand sides [C Sigma' | delta | V] ride through the same launches and chol_bounds' m + 16 was counted for one
                        strip kernel, not for a solve whose rows arrive in nbr instalments.  nbr / m < 2 % at the committed sizes.
    reductions          the base panel's downdate, gamma and hV are Yn_k^T [Y_k | Yn_k] added into an accumulator once per block row
                        (S.hook), the downdate of the landmark blocks one product over all m rows -- or, with "downdate_early", one product
                        per block row for the first shares: the same count, one addition per block row, covered by block_rows.
    the split solve     trsmLeft: [L11 0; L21 L22], X1 = L11^-1 B1, B2 -= L21 X1 as one product, X2 = L22^-1 B2; once from six 64-row
                        blocks and 256 columns on, recursively with "trsm_leaf".  A leaf is the strip kernel with its own (rows + 16) u;
                        each level adds the one rounding of B2 - (L21 X1): split_levels more in the same counts.
    "solve_inverse"     R <- (L_kk^-T)^T R with the explicit inverse of the WHOLE diagonal factor, itself the strip kernel's right solve of
                        the identity: |Wh L_kk^T - I| <= (bk + 16) u (|Wh||L_kk^T| + I) T^T (chol_bounds, right solve) and the product's
                        gamma_bk |Wh^T||R| give, with |R| <= |L_kk||Y_k| and T_b = blockdiag(|L_kk||L_kk^-1|) over whole diagonal blocks,
                            |L_kk Yh_k - R| <= (bk + 16) u (T (T_b + I) + T_b) |L_kk||Y_k|,
                        chol_bounds' T = |L_jj||L_jj^-1| argument taken over the whole block: inverse_blocks = (2 bl, 3 bl) puts
                        T (T_b + I) + T_b in T's place in E1, E2 and their E-chain twins (the factor's off-diagonal blocks ARE solved
                        block rows).  The five base coordinates of Sigma_e, which k_tl_eprep eliminates on their own, are a block of T_b.
  No term is fitted to a device result; tests/test_update_exact.py holds a numpy restatement of the schedule to these bounds and sees three
  injected schedule faults leave them."""
import numpy as np
import scipy.linalg
from mpmath import mp, mpf

import chol_bounds as cb
import i8_emulator as i8
import lie_exact as lx
import riccati_exact as rx

LD = rx.LD
U64, U32 = rx.U64, rx.U32
OPS_C, OPS_S, OPS_RHS6, OPS_M, OPS_B, OPS_SOLVE4 = 3, 4, 12, 6, 3, 14   # counted in the module docstring
K_DELTA_MEASURED = 27.38084221112257   # the numpy oracle's worst |delta - delta_exact| / (u (1 + |delta|)); test_update_exact.py re-measures it
K_DELTA = 4.0 * K_DELTA_MEASURED
MP_MAX_N = 17


def gamma(k, u=U64):
    return rx.gamma(k, u)


# ---- the geometric inputs at 50 digits ------------------------------------------------------------------------------------------------------
class Geometry:
    """delta (2 N), C0 (N of 2 x 3), ZP (N of 3 x 6), eta0, Pd (3 x 2), Kpar (6 x 4) as mpf lists, from the stepped group X (lie_exact.Group),
    the origin xi0 (lie_exact.State) and the bearings y (N x 3 doubles, taken as exact)."""

    def __init__(self, X, xi0, y):
        N = self.N = len(xi0.p)
        y = np.asarray(y, dtype=float).reshape(N, 3)
        self.delta, self.C0, self.ZP = [], [], []
        est = lx.state_group_action(X, xi0)
        RC = lx.mm(est.R, xi0.camR)
        xC = lx.add(lx.mv(est.R, xi0.camx), est.x)
        RCt = lx.tr(RC)
        for i in range(N):
            self.delta += lx.residual(y[i], X.Q[i][0], xi0.p[i])
            self.C0.append(lx.landmark_constants([float(v) for v in xi0.p[i]])[0])
            pHat = lx.add(lx.mv(RC, est.p[i]), xC)
            Dm = lx.mscl(X.Q[i][1], lx.mm(X.Q[i][0], RCt))
            left = lx.mm(lx.hat(lx.sub(xi0.x, pHat)), xi0.R)
            blk = lx.mm(Dm, [left[r] + xi0.R[r] for r in range(3)])
            self.ZP.append(blk)
        eta0, _, cinv = lx.pose_constants(xi0.R)
        self.eta0 = eta0
        proj = lx.madd(lx.eye(), lx.mscl(mpf(-1), lx.outer(eta0, eta0)))
        self.Pd = lx.mscl(mpf(-1), lx.mm(lx.mm(proj, lx.hat(eta0)), cinv))
        z = mpf(0)
        self.Kpar = [[eta0[r], z, z, z] for r in range(3)] + [[z, mpf(int(c == 1)), mpf(int(c == 2)), mpf(int(c == 3))] for c in (1, 2, 3)]

    def arrays(self, conv):
        """{delta (m), C0 (N, 2, 3), ZP (n_e, 6), Pd (3, 2), Kpar (6, 4)} as arrays of conv(mpf) (object arrays for conv = identity)."""
        N = self.N
        dt = object if conv is _same else LD
        out = {"delta": np.array([conv(v) for v in self.delta], dtype=dt)}
        out["C0"] = np.array([[[conv(v) for v in row] for row in blk] for blk in self.C0], dtype=dt).reshape(N, 2, 3)
        ZP = np.array([[conv(mpf(0))] * 6 for _ in range(5 + 3 * N)], dtype=dt)
        for i, blk in enumerate(self.ZP):
            ZP[5 + 3 * i:8 + 3 * i] = np.array([[conv(v) for v in row] for row in blk], dtype=dt)
        out["ZP"] = ZP
        out["Pd"] = np.array([[conv(v) for v in row] for row in self.Pd], dtype=dt)
        out["Kpar"] = np.array([[conv(v) for v in row] for row in self.Kpar], dtype=dt)
        return out


def _same(x):
    return x


def f64(A):
    """longdouble or mpf array -> float64"""
    A = np.asarray(A)
    if A.dtype == object:
        return np.array([float(v) for v in A.flat]).reshape(A.shape)
    return A.astype(np.float64)


def to_ld(A):
    A = np.asarray(A)
    if A.dtype == object:
        return np.array([rx._ld(v) for v in A.flat], dtype=LD).reshape(A.shape)
    return A.astype(LD)


# ---- linear algebra in longdouble or mpf (object arrays) -------------------------------------------------------------------------------------
def chol(A, sqrt):
    n = len(A)
    L = np.zeros_like(A)
    if A.dtype == object:
        L[...] = mpf(0)
    for j in range(n):
        d = A[j, j] - (L[j, :j] @ L[j, :j] if j else 0)
        if not d > 0:
            raise np.linalg.LinAlgError("not positive definite")
        L[j, j] = sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - (L[j + 1:, :j] @ L[j, :j] if j else 0)) / L[j, j]
    return L


def solve_lower(L, B):
    """L^-1 B by forward substitution"""
    X = np.array(B, copy=True)
    for i in range(len(L)):
        if i:
            X[i] = X[i] - L[i, :i] @ X[:i]
        X[i] = X[i] / L[i, i]
    return X


def solve_upper_t(L, B):
    """L^-T B by backward substitution"""
    X = np.array(B, copy=True)
    n = len(L)
    for i in range(n - 1, -1, -1):
        if i + 1 < n:
            X[i] = X[i] - L[i + 1:, i] @ X[i + 1:]
        X[i] = X[i] / L[i, i]
    return X


def solve4(M, b):
    """Gaussian elimination with partial pivoting and one residual refinement, in M's own arithmetic"""
    def ge(M, b):
        A = np.concatenate([np.array(M, copy=True), np.array(b, copy=True).reshape(-1, 1)], axis=1)
        n = len(M)
        for c in range(n):
            pv = c + int(np.argmax([abs(A[r, c]) for r in range(c, n)]))
            A[[c, pv]] = A[[pv, c]]
            for r in range(c + 1, n):
                A[r] = A[r] - A[c] * (A[r, c] / A[c, c])
        x = np.array(b, copy=True)
        for r in range(n - 1, -1, -1):
            x[r] = (A[r, n] - (A[r, r + 1:n] @ x[r + 1:] if r + 1 < n else 0)) / A[r, r]
        return x
    x = ge(M, b)
    return x + ge(M, b - M @ x)


def c_times(C0, S, N):
    """C S for C's 2 x 3 blocks at the landmark columns: (2 N, columns of S)"""
    return np.concatenate([C0[i] @ S[11 + 3 * i:14 + 3 * i] for i in range(N)], axis=0)


def times_ct(B, C0, N):
    """B C^T"""
    return np.concatenate([B[:, 11 + 3 * i:14 + 3 * i] @ C0[i].T for i in range(N)], axis=1)


# ---- the propagate at 50 digits (N <= 17) ----------------------------------------------------------------------------------------------------
def propagate_mp(steps, S0):
    """Sigma' through the Steps in mpmath from their unrounded blocks (Step.mp / Step.smp): an object array of mpf"""
    S = np.array([[mpf(float(v)) for v in row] for row in np.asarray(S0, dtype=float)], dtype=object)
    for st in steps:
        s, b, N, n = st.smp, st.mp, st.N, st.n
        F = np.array([[mpf(int(i == j)) for j in range(n)] for i in range(n)], dtype=object)
        Bt = np.array([[mpf(0)] * 6 for _ in range(n)], dtype=object)

        def put(dst, r, c, blk):
            for i, row in enumerate(blk):
                for j, v in enumerate(row):
                    dst[r + i, c + j] = v
        put(F, 6, 0, s["TBg"]), put(F, 8, 0, s["TBvw"]), put(F, 8, 3, s["TRA"]), put(F, 8, 6, s["TAvg"])
        put(Bt, 6, 0, b["Bg"]), put(Bt, 8, 0, b["Bvw"]), put(Bt, 8, 3, b["RA"])
        for i in range(N):
            put(F, 11 + 3 * i, 0, s["Lw"][i]), put(F, 11 + 3 * i, 8, s["Lv"][i]), put(Bt, 11 + 3 * i, 0, b["Bi"][i])
            put(F, 11 + 3 * i, 11 + 3 * i, s["D"][i])
        R = np.array([mpf(float(v)) for v in st.R], dtype=object)
        P = np.array([mpf(float(v)) for v in st.P], dtype=object)
        Q = (Bt * R) @ Bt.T
        for i in range(n):
            Q[i, i] += P[i]
        S = F @ S @ F.T + b["T"] * Q
    return S


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------
def update_reference(S1, geo, r, use_mp=False):
    """The update of the module docstring from Sigma' = S1 (longdouble array, or an object array of mpf with use_mp) and a Geometry; r the
    measurement variance.  Returns a dictionary of arrays in the arithmetic used: Sp (Sigma+), gamma, Gamma6, delta and every intermediate
    the bound needs (B, S, L, Y, z, Le, C0, ZP, Pd, Kpar, sol, M, b)."""
    N = geo.N
    g = geo.arrays(_same if use_mp else rx._ld)
    sqrt = mp.sqrt if use_mp else np.sqrt
    r = mpf(float(r)) if use_mp else LD(float(r))
    m = 2 * N
    B = c_times(g["C0"], S1, N)
    S = times_ct(B, g["C0"], N)
    for i in range(m):
        S[i, i] = S[i, i] + r
    L = chol(S, sqrt)
    Y = solve_lower(L, B)
    z = solve_lower(L, g["delta"])
    gam = Y.T @ z
    Sp = S1 - Y.T @ Y
    Le = chol(np.array(S1[6:, 6:], copy=True), sqrt)
    dU = np.concatenate([g["Pd"] @ gam[6:8], g["Pd"][0:3, 0] * 0])
    G = g["ZP"] @ g["Kpar"]
    h = -(g["ZP"] @ dU)
    h[5:] = h[5:] - gam[11:]
    Gt, ht = solve_lower(Le, G), solve_lower(Le, h)
    M, b = Gt.T @ Gt, Gt.T @ ht
    sol = solve4(M, b)
    out = dict(g, N=N, S1=S1, B=B, S=S, L=L, Y=Y, z=z, gamma=gam, Sp=Sp, Le=Le, dU=dU, M=M, b=b, sol=sol, Gamma6=dU + g["Kpar"] @ sol, r=r)
    return out


# ---- the bound -------------------------------------------------------------------------------------------------------------------------------
def _mirror_lower(E):
    return np.tril(E) + np.tril(E, -1).T


def whole_block_T(L, starts):
    """blockdiag(|L_kk| |L_kk^-1|) over the diagonal blocks that begin at `starts` (ascending, the first 0), fp64: chol_bounds.block_T with the
    kernels' 16 x 16 blocks replaced by whole diagonal blocks of a block-row schedule"""
    n = len(L)
    T = np.zeros((n, n))
    edges = list(starts) + [n]
    for a, e in zip(edges[:-1], edges[1:]):
        if e > a:
            T[a:e, a:e] = (np.abs(cb._ld(L[a:e, a:e])) @ np.abs(cb.inv_lower(L[a:e, a:e]))).astype(np.float64)
    return T


def update_bounds(ref, E_ric, fp32=False, tau=None, k_delta=None, slices=0, block_rows=0, split_levels=0, inverse_blocks=None):
    """{"Sp", "gamma", "delta", "Gamma6"}: the entrywise bounds of the module docstring (float64) from update_reference's longdouble result and
    the propagate's bound E_ric.  block_rows, split_levels, inverse_blocks: the counted terms of the partitioned filter's block-row schedule
    (module docstring, "The partitioned filter"); their defaults give the bound of the single-GPU routes."""
    tau = rx.TAU_BLK if tau is None else tau
    k_delta = K_DELTA if k_delta is None else k_delta
    u = U64
    N = ref["N"]
    m, ne = 2 * N, 5 + 3 * N
    extra = int(block_rows) + int(split_levels)   # rounded additions per entry on top of the counts m + 1, m + 16, m + 2 (and n_e + ...)
    a = lambda k: np.abs(f64(ref[k]))  # noqa: E731
    aS1, aB, aS, aL, aY, az, aSp, agam, adelta = a("S1"), a("B"), a("S"), a("L"), a("Y"), a("z"), a("Sp"), a("gamma"), a("delta")
    aC0, aZP, aPd, aKp = a("C0"), a("ZP"), a("Pd"), a("Kpar")
    E_ric = f64(E_ric)
    L, Le = ref["L"], ref["Le"]
    Kt = solve_upper_t(L, ref["Y"])                  # L^-T Y = K^T  (m x n)
    w = solve_upper_t(L, ref["z"])
    aK, aw = np.abs(f64(Kt)).T, np.abs(f64(w))
    dC0 = np.stack([np.full((2, 3), tau * u * aC0[i].max()) for i in range(N)]) if N else aC0
    T = cb.block_T(f64(L))
    if inverse_blocks:  # a block row solved as ONE product with the explicit inverse of its whole diagonal factor
        Tb = whole_block_T(f64(L), range(0, m, int(inverse_blocks[0])))
        T = T @ (Tb + np.eye(m)) + Tb
    ddelta = k_delta * u * (1 + adelta)

    dB = gamma(OPS_C) * c_times(aC0, aS1, N) + c_times(dC0, aS1, N)
    dS = times_ct(dB, aC0, N) + gamma(OPS_S) * times_ct(aB, aC0, N) + times_ct(aB, dC0, N) + u * aS
    dS = np.maximum(dS, dS.T)
    E1 = _mirror_lower(((m + 1 + extra) * u + cb.P) * ((aL @ aL.T) @ T.T))
    E2 = (m + 16 + extra) * u * (T @ (aL @ aY + aB))
    E2z = (m + 16 + extra) * u * (T @ (aL @ az + adelta))
    u3 = U32 if fp32 else U64
    E3 = (gamma(m + 2 + extra, u3) + (2 * U32 if fp32 else 0.0)) * (aY.T @ aY)
    if slices:  # the rigorous bound of tests/i8_emulator.py from the exponent words of Y's columns, and the subtraction
        words = i8.exponent_words(f64(ref["Y"]) * (1 + 2.0 ** -30))   # (the device's Y is not the reference's to the last bit)
        live = i8.bound(m, np.maximum(words, 1), np.maximum(words, 1), slices) * ((words > 0)[:, None] & (words > 0)[None, :])
        E3 = live + gamma(2) * (aY.T @ aY)
    Gm = aK @ (dB + E2)
    KC = f64(ref["Y"].T @ solve_lower(L, _dense_C(ref["C0"], N)))   # K C  (n x n)
    aJ = np.abs(np.eye(11 + 3 * N) - KC)
    dSE = dS + E1
    out = {"delta": ddelta}
    out["Sp"] = Gm + Gm.T + aK @ dSE @ aK.T + E3 + u3 * (aS1 + aSp) + aJ @ E_ric @ aJ.T
    aCtw = _ct_vec(aC0, aw, N)
    dgam = aK @ (E2z + ddelta) + (dB + E2).T @ aw + aK @ (dSE @ aw) + gamma(m + 2 + extra) * (aY.T @ az) + aJ @ (E_ric @ aCtw)
    out["gamma"] = dgam

    # ---- Gamma[0:6]
    A = np.zeros((ne, 11), dtype=LD)
    A[:, 0:6] = ref["ZP"]
    A[0:5, 6:11] = np.eye(5, dtype=LD)
    Gt = solve_lower(Le, A)
    Ve = solve_upper_t(Le, Gt)
    aGt, aVe, aA, aLe = np.abs(f64(Gt)), np.abs(f64(Ve)), np.abs(f64(A)), np.abs(f64(Le))
    G11 = f64(Gt.T @ Gt)
    Te = cb.block_T(f64(Le))
    if inverse_blocks:  # (the E-chain's blocks start behind the five base coordinates, which k_tl_eprep eliminates on their own)
        Tbe = whole_block_T(f64(Le), [0] + list(range(5, ne, int(inverse_blocks[1]))))
        Te = Te @ (Tbe + np.eye(ne)) + Tbe
    E1e = _mirror_lower(((ne + 1 + extra) * u + cb.P) * ((aLe @ aLe.T) @ Te.T))
    E2e = (ne + 16 + extra) * u * (Te @ (aLe @ aGt + aA))
    dZ = np.zeros((ne, 11))
    for i in range(N):
        dZ[5 + 3 * i:8 + 3 * i, 0:6] = tau * u * aZP[5 + 3 * i:8 + 3 * i].max()
    X = aVe.T @ (E2e + dZ)
    dG11 = X + X.T + gamma(ne + 2 + extra) * (aGt.T @ aGt)
    # the symmetric perturbations of Sigma_e (its factorisation's backward error and the propagate's error) reach M and b together
    Esym = E1e + E_ric[6:, 6:]
    sol_ld = ref["sol"]
    resid = -(ref["ZP"] @ ref["dU"]) - (ref["ZP"] @ ref["Kpar"]) @ sol_ld
    resid[5:] = resid[5:] - ref["gamma"][11:]
    Vr = f64(solve_upper_t(Le, solve_lower(Le, resid)))
    Vr_dev = Vr + _ct_vec(f64(ref["C0"]), f64(w), N)[6:]
    aVG = np.abs(f64(Ve[:, 0:6] @ ref["Kpar"]))
    dsym = aVG.T @ (Esym @ np.maximum(np.abs(Vr), np.abs(Vr_dev)))
    dG6, dT65 = dG11[0:6, 0:6], dG11[0:6, 6:11]
    G6, T65 = G11[0:6, 0:6], G11[0:6, 6:11]
    # hV = V^T w, V = C_e Z_P (m x 6)
    Vm = np.concatenate([ref["C0"][i] @ ref["ZP"][5 + 3 * i:8 + 3 * i] for i in range(N)], axis=0)
    aVabs = np.concatenate([aC0[i] @ aZP[5 + 3 * i:8 + 3 * i] for i in range(N)], axis=0)
    dV = np.concatenate([dC0[i] @ aZP[5 + 3 * i:8 + 3 * i] + aC0[i] @ dZ[5 + 3 * i:8 + 3 * i, 0:6] for i in range(N)], axis=0) + gamma(OPS_C) * aVabs
    Yv = solve_lower(L, Vm)
    Kv = solve_upper_t(L, Yv)
    aYv, aKv = np.abs(f64(Yv)), np.abs(f64(Kv))
    hV = f64(Yv.T @ ref["z"])
    E2v = (m + 16 + extra) * u * (T @ (aL @ aYv + np.abs(f64(Vm))))
    CEC = times_ct(c_times(aC0, E_ric, N), aC0, N)
    dhV = (dV + E2v).T @ aw + aKv.T @ (E2z + ddelta) + aKv.T @ ((dSE + CEC) @ aw) + gamma(m + 2 + extra) * (aYv.T @ az)
    g5, dg5 = f64(ref["gamma"])[6:11], dgam[6:11]
    dUw = f64(ref["dU"])
    ddU = np.zeros(6)
    ddU[0:3] = aPd @ dgam[6:8] + tau * u * aPd.max() * np.abs(g5[0:2]).sum()
    # rhs6 = -hV + T65 g5 - G6 dU: the errors of g5 and dU enter sol through the exact matrices M^-1 K^T T65 and M^-1 K^T G6
    db6 = (dhV + dT65 @ np.abs(g5) + dG6 @ np.abs(dUw)
           + gamma(OPS_RHS6) * (np.abs(hV) + np.abs(T65) @ np.abs(g5) + np.abs(G6) @ np.abs(dUw)))
    b6 = -(hV - T65 @ g5) - G6 @ dUw
    dM = aKp.T @ dG6 @ aKp + gamma(OPS_M) * (aKp.T @ np.abs(G6) @ aKp)
    M, sol = f64(ref["M"]), f64(ref["sol"])
    with np.errstate(all="ignore"):
        try:
            Minv = np.linalg.inv(M)
        except np.linalg.LinAlgError:
            Minv = np.full((4, 4), np.inf)
        Pk = Minv @ f64(ref["Kpar"]).T
        lin = np.abs(Pk @ T65) @ dg5 + np.abs(Pk @ G6) @ ddU
    aMinv = np.abs(Minv)
    Pm, Lm, Um = scipy.linalg.lu(M)
    dsol = (np.abs(Pk) @ db6 + np.where(np.isfinite(lin), lin, np.inf)
            + aMinv @ (dM @ np.abs(sol) + gamma(OPS_B) * (aKp.T @ np.abs(b6)) + dsym + gamma(OPS_SOLVE4) * (Pm @ (np.abs(Lm) @ np.abs(Um)) @ np.abs(sol))))
    out["Gamma6"] = ddU + aKp @ dsol + 2 * u * np.abs(f64(ref["Gamma6"]))
    # (dS .. T: what the bounds of the innovation statistics, tests/consistency_exact.py part C, are made of)
    out["parts"] = dict(cond_M=float(np.linalg.cond(M)), hV=hV, G6=G6, T65=T65, dS=dS, E1=E1, E2z=E2z, ddelta=ddelta, aw=aw, CEC=CEC, T=T, E_ric=E_ric)
    return out


def _dense_C(C0, N):
    C = np.zeros((2 * N, 11 + 3 * N), dtype=C0.dtype)
    for i in range(N):
        C[2 * i:2 * i + 2, 11 + 3 * i:14 + 3 * i] = C0[i]
    return C


def _ct_vec(aC0, aw, N):
    """|C^T| |w|  (n)"""
    out = np.zeros(11 + 3 * N)
    for i in range(N):
        out[11 + 3 * i:14 + 3 * i] = aC0[i].T @ aw[2 * i:2 * i + 2]
    return out


# ---- a whole vision call ----------------------------------------------------------------------------------------------------------------------
class Case:
    """The reference of one vision call (and of the IMU calls queued in front of it) from a snapshot: `imu_calls` [(stamp, omega, accel)],
    then the update at `stamp` with the bearings y.  Holds the geometry (independent of Sigma); reference(S0) gives the numbers."""

    def __init__(self, snap, d, stamp, y, imu_calls=()):
        f = rx.ExactFilter(snap, d)
        steps = [f.process_imu(t, w, acc) for t, w, acc in imu_calls]
        steps.append(f.process_imu(stamp, np.zeros(3), np.zeros(3)))
        self.steps = [s for s in steps if s is not None]
        assert self.steps and steps[-1] is not None, "the vision call must integrate"
        self.geo = Geometry(f.X, f.xi0, y)
        self.X, self.xi0 = f.X, f.xi0
        self.r = float(d["measurementVariance"])
        self.N = self.geo.N

    def reference(self, S0, fp32=False, slices=0):
        """(ref, bounds): update_reference in longdouble on reference_run's Sigma', and update_bounds"""
        S1, E = rx.reference_run(self.steps, S0, fp32)
        ref = update_reference(S1, self.geo, self.r)
        return ref, update_bounds(ref, E, fp32, slices=slices)

    def reference_mp(self, S0):
        assert self.N <= MP_MAX_N
        return update_reference(propagate_mp(self.steps, S0), self.geo, self.r, use_mp=True)


# ---- comparison --------------------------------------------------------------------------------------------------------------------------------
def worst_ratio(got, ref, bound):
    """(max |got - ref| / bound, its index); where the bound is exactly 0 the value must be exactly the reference's (ratio inf otherwise), and
    a value that is not a number is outside every bound."""
    got = np.asarray(got)
    err = np.abs(to_ld(got) - to_ld(ref))
    b = np.asarray(bound, dtype=np.float64).astype(LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, LD(0), np.where(b > 0, err / b, LD(np.inf)))
    r = np.where(np.isnan(r), LD(np.inf), r)
    k = int(np.argmax(r))
    return float(r.flat[k]), tuple(int(v) for v in np.unravel_index(k, r.shape))


def symmetry_ratio(S, bound):
    """max |S - S^T| / (bound + bound^T); exactly symmetric where the bound is 0"""
    S = to_ld(S)
    err = np.abs(S - S.T)
    b = np.asarray(bound, dtype=np.float64).astype(LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, LD(0), np.where(b + b.T > 0, err / (b + b.T), LD(np.inf)))
    return float(np.where(np.isnan(r), LD(np.inf), r).max())
