"""Inputs, error bounds and a numpy model for the tests of the Cholesky building blocks (csrc/eqf_chol64.hpp: factor64, potrf16v2, solveStrip,
mmTile; csrc/eqf_tile.hpp: k_tile_potrf, k_tile_potrf_trail, k_tile_trsm).  numpy only: tests/test_chol_bounds.py holds LAPACK and the
model against the bounds on the CPU, tests/test_gpu_tile_factor.py the kernels.

Notation.  u = 2^-53.  p = 2 x 2.4e-16: the measured accuracy of a refined pivot (v_rsq_f64 + the refinement of scaleRsqrtPivot; comment above
potrf16v2), doubled because the pivot enters the product L L^T squared.

What the kernels do differently from a textbook Cholesky: every panel block outside the diagonal 64-block, and every right-hand side, is
MULTIPLIED with the explicit inverse W_j = L_jj^-1 of a 16 x 16 diagonal block instead of being substituted.  A panel block is
fl(A'_ij W_j^T) with error gamma_16 |A'_ij| |W_j^T|, and |A'_ij| <= |L_ij| |L_jj^T|, so the error of block column j is that of
substitution times T_j = |L_jj| |L_jj^-1| >= I (elementwise).  With T = blockdiag(T_j) over the diagonal blocks at multiples of 16:

  factorisation (lower triangle)   |A - Lh Lh^T|  <= ((n + 1) u + p) (|L| |L^T|) T^T      L, T from LAPACK's factor of the same matrix
  left solve                       |Lh Xh - B|    <= (n + 16) u  T (|Lh| |Xh| + |B|)      Lh the factor the solve was given, T from Lh
  right solve                      |Xh Lh^T - B|  <= (n + 16) u  (|Xh| |Lh^T| + |B|) T^T
  record                           |Wh_j Lh_jj - I| <= (17 u + p) |Wh_j| |Lh_jj|

Every function returns (ratio to that bound, ratio to the same bound with T = I); the second is for reporting.  Residuals are formed in
np.longdouble (64-bit mantissa on x86): a residual formed in fp64 carries the very error it measures.  The bounds themselves (products of
absolute values) are formed in fp64: their own relative error, n u, is nothing next to the factor they are compared at."""
import numpy as np

U = 2.0 ** -53
P = 2 * 2.4e-16
QB = 16  # the kernels' sub-block: one MFMA tile
SB = 64  # their block column

assert np.finfo(np.longdouble).eps < 2e-19, "np.longdouble is not wider than fp64 here: the residuals of this helper would be meaningless"


def _ld(a):
    return np.asarray(a, dtype=np.longdouble)


# ---- seeded matrix families ---------------------------------------------------------------------------------------------------------------
def _sym(A):
    return (A + A.T) / 2


def _rng(tag, n, par):
    return np.random.default_rng([tag, n, int(round(-np.log10(par) if par < 1 else par))])


def graded(n, c):
    """Q diag(logspace(0, -c, n)) Q^T: condition number 10^c, eigenvalues spread evenly on the log scale"""
    rng = _rng(1, n, c)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return _sym((Q * np.logspace(0, -c, n)) @ Q.T)


def one_small(n, c):
    """eigenvalues 1 except one 10^-c"""
    rng = _rng(2, n, c)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    d = np.ones(n)
    d[-1] = 10.0 ** -c
    return _sym((Q * d) @ Q.T)


def equicorrelated(n, eps):
    """D ((1 - eps) 1 1^T + eps I) D with D = diag(10^U(-3, 3)): the shape of S when every bearing shares the pose uncertainty.  Condition
    number up to 1e23, yet every one of these factors (the diagonal scaling is harmless to Cholesky; tests/test_chol_bounds.py)."""
    rng = _rng(3, n, eps)
    d = 10.0 ** rng.uniform(-3, 3, n)
    return _sym((np.full((n, n), 1 - eps) + eps * np.eye(n)) * np.outer(d, d))


FAMILIES = (("graded", graded, (2, 8, 13)), ("one_small", one_small, (6, 10, 13)), ("equicorrelated", equicorrelated, (1e-2, 1e-6, 1e-10)))
POTRF_SIZES = (1, 2, 15, 16, 17, 33, 63, 64, 65, 100, 127, 128, 129, 192, 193, 384)


def family_cases(n):
    """[(label, A)] over all families and parameters at size n"""
    return [(f"{name}({n}, {par:g})", fn(n, par)) for name, fn, pars in FAMILIES for par in pars]


def spd_base(n, seed=0):
    """M M^T + n I: the well-conditioned matrix the failure cases are cut from"""
    M = np.random.default_rng([4, n, seed]).standard_normal((n, n))
    return _sym(M @ M.T + n * np.eye(n))


def bad_positions(n):
    return sorted({q for q in (0, 7, 15, 16, n - 1, 64, 64 * (n // 64)) if q < n})


def bad_inputs(n):
    """[(label, A)]: matrices that are not positive definite, each from spd_base(n) -- a negative diagonal entry, an exact zero pivot (row and
    column zeroed), a NaN on the diagonal, at every position of bad_positions(n); and indefinite matrices whose diagonal is untouched."""
    A0, out = spd_base(n), []
    for q in bad_positions(n):
        A = A0.copy()
        A[q, q] = -1.0
        out.append((f"neg[{q}]", A))
        A = A0.copy()
        A[q, :] = 0.0
        A[:, q] = 0.0
        out.append((f"zero[{q}]", A))
        A = A0.copy()
        A[q, q] = np.nan
        out.append((f"nan[{q}]", A))
    for a, b in ((3, 12), (5, 70)):
        if b < n:
            A = A0.copy()
            A[a, b] = A[b, a] = 2 * np.sqrt(A[a, a] * A[b, b])
            out.append((f"offdiag[{a},{b}]", A))
    return out


def control_inputs(n):
    """[(label, A)]: positive definite and as close to singular as fp64 factors: must NOT raise the flag"""
    return [(f"one_small({n}, 13)", one_small(n, 13)), (f"equicorrelated({n}, 1e-10)", equicorrelated(n, 1e-10))]


def lapack_outcome(A):
    """What np.linalg.cholesky does with A: ("raises", None), ("nan_factor", L) -- it returned a factor that holds a NaN -- or
    ("factors", L).  Reference LAPACK tests `pivot <= 0 or isnan(pivot)`; the optimised dpotrf of some numpy builds tests `pivot <= 0`
    alone, which a NaN passes: such a build hands the NaN on instead of raising."""
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return "raises", None
    return ("nan_factor" if np.isnan(L).any() else "factors"), L


# ---- bounds -------------------------------------------------------------------------------------------------------------------------------
def inv_lower(L):
    """inverse of a lower triangular matrix by forward substitution in longdouble"""
    L = _ld(L)
    n = len(L)
    W = np.zeros((n, n), dtype=np.longdouble)
    for i in range(n):
        W[i, i] = 1 / L[i, i]
        W[i, :i] = -(L[i, :i] @ W[:i, :i]) / L[i, i]
    return W


def block_T(L):
    """T = blockdiag(|L_jj| |L_jj^-1|) over the 16 x 16 diagonal blocks at multiples of 16 (the last one smaller), fp64"""
    n = len(L)
    T = np.zeros((n, n))
    for j in range(0, n, QB):
        e = min(n, j + QB)
        T[j:e, j:e] = (np.abs(_ld(L[j:e, j:e])) @ np.abs(inv_lower(L[j:e, j:e]))).astype(np.float64)
    return T


def block_inverses(L):
    """[L_jj^-1] of the 16 x 16 diagonal blocks at multiples of 16, rounded to fp64: the W_j a solve against ANY lower factor L needs"""
    return [inv_lower(L[j:j + QB, j:j + QB]).astype(np.float64) for j in range(0, len(L), QB)]


def _ratios(R, aware, plain, c, mask=None):
    """max R / (c bound) for the two bounds; an entry whose bound is zero must have a zero residual"""
    out = []
    for Bd in (aware, plain):
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(Bd > 0, R / (c * _ld(Bd)), np.where(R == 0, 0.0, np.inf))
        q = np.where(np.isnan(q), np.inf, q)  # a residual that is not a number is outside every bound
        out.append(float(q[mask].max() if mask is not None else q.max()))
    return tuple(out)


def _tril_mm(L, X, lower_only=False):
    """L @ X in longdouble for a lower triangular L, 64 rows at a time without the products with L's zeros (lower_only: X is square and only
    the result's lower triangle is wanted, the rest stays zero): a half to a third of the time of the full product, which is what the
    tests that use this helper spend theirs on"""
    L, X = _ld(L), _ld(X)
    n = len(L)
    out = np.zeros((n, X.shape[1]), dtype=np.longdouble)
    for i0 in range(0, n, SB):
        i1 = min(n, i0 + SB)
        c = i1 if lower_only else X.shape[1]
        out[i0:i1, :c] = L[i0:i1, :i1] @ X[:i1, :c]
    return out


def potrf_ratio(A, Lh, Lref=None, T=None):
    """(aware, plain): |A - Lh Lh^T| over ((n + 1) u + p) (|L| |L^T|) T^T and over the same with T = I, lower triangle; L = Lref, LAPACK's factor;
    T = block_T(Lref), for callers that hold several factors against one matrix"""
    n = len(A)
    if Lref is None:
        Lref = np.linalg.cholesky(A)
    Lh = np.tril(Lh)
    R = np.abs(_ld(A) - _tril_mm(Lh, Lh.T, lower_only=True))  # (above the diagonal: masked out below)
    G = np.abs(Lref) @ np.abs(Lref).T
    return _ratios(R, G @ (block_T(Lref) if T is None else T).T, G, (n + 1) * U + P, np.tril(np.ones((n, n), dtype=bool)))


def trsm_left_ratio(Lh, Xh, B, T=None):
    """(aware, plain): |Lh Xh - B| over (n + 16) u T (|Lh| |Xh| + |B|), T = block_T(Lh)"""
    n = len(Lh)
    Lh = np.tril(Lh)
    R = np.abs(_tril_mm(Lh, Xh) - _ld(B))
    E = np.abs(Lh) @ np.abs(Xh) + np.abs(B)
    return _ratios(R, (block_T(Lh) if T is None else T) @ E, E, (n + QB) * U)


def trsm_right_ratio(Lh, Xh, B, T=None):
    """(aware, plain): |Xh Lh^T - B| over (n + 16) u (|Xh| |Lh^T| + |B|) T^T, T = block_T(Lh)"""
    n = len(Lh)
    Lh = np.tril(Lh)
    R = np.abs(_tril_mm(Lh, np.asarray(Xh).T).T - _ld(B))
    E = np.abs(Xh) @ np.abs(Lh).T + np.abs(B)
    return _ratios(R, E @ (block_T(Lh) if T is None else T).T, E, (n + QB) * U)


def record_ratio(Wh, Ljj):
    """|Wh Ljj - I| over (17 u + p) |Wh| |Ljj| for one 16 x 16 inverse block of a record (the plain ratio is the same: there is no T here)"""
    R = np.abs(_ld(Wh) @ _ld(Ljj) - np.eye(len(Ljj)))
    Bd = np.abs(Wh) @ np.abs(Ljj)
    return _ratios(R, Bd, Bd, 17 * U + P)[0]


# ---- the model ----------------------------------------------------------------------------------------------------------------------------
def model_chol16(A, fault=None, block=QB):
    """The blocked algorithm of the kernels in numpy fp64: 16-wide right-looking; per stage the sixteen columns of the diagonal block and of
    sixteen identity rows are eliminated, which leaves W_j^T = L_jj^-T (potrf16v2); the rows below are multiplied with W_j^T (solveStrip);
    then the trailing update.  Returns (L, [W_j]).
    block = 16: EVERY panel row goes through W_j -- the explicit-inverse algorithm at its worst.  block = 64 is what the kernels do: the
    pivot wave eliminates the rows of its own 64-block along with the diagonal block (substitution), only the rows below that block are
    multiplied with W_j^T.
    fault (the negative cases of tests/test_chol_bounds.py): "drop_trailing" leaves one 16 x 16 block of one trailing update out,
    "transpose_w" multiplies one panel with W_j instead of W_j^T, "wrong_lane" takes one pivot's square root from the neighbouring lane."""
    n = len(A)
    A = np.array(A, dtype=np.float64)
    L = np.zeros((n, n))
    Ws = []
    for j in range(0, n, QB):
        e = min(n, j + QB)
        w = e - j
        sub = e if block == QB else min(n, block * (j // block + 1))  # rows [j, sub): eliminated by the pivot wave
        M = np.vstack([A[j:sub, j:e], np.eye(w)])
        for c in range(w):
            d = M[c, c]
            if fault == "wrong_lane" and j == 0 and c == 1 and w > 2:
                d = M[c + 1, c + 1]
            with np.errstate(invalid="ignore", divide="ignore"):
                l = M[:, c] / np.sqrt(d)
            M[:, c] = l
            M[:, c + 1:] -= np.outer(l, l[c + 1: w])
        L[j:sub, j:e] = np.vstack([np.tril(M[:w]), M[w: sub - j]])
        W = M[sub - j:].T.copy()  # (the identity rows hold W^T)
        Ws.append(W)
        if sub < n:
            L[sub:, j:e] = A[sub:, j:e] @ (W if fault == "transpose_w" and j == 0 else W.T)
        if e < n:
            upd = L[e:, j:e] @ L[e:, j:e].T
            if fault == "drop_trailing" and j == 0:
                upd[-min(QB, n - e):, :QB] = 0.0  # the last block row's first block
            A[e:, e:] -= upd
    return L, Ws


def model_trsm16(L, Ws, B, right=False, fault=None):
    """The solves in numpy fp64, in 16-wide blocks and in the kernel's order (k_tile_trsm: block kb of the strip first takes the products
    with the solved blocks j < kb, then the explicit inverse).  Left, B n x m:  X_kb = W_kb (B_kb - sum_j L_kb,j X_j).  Right, B m x n:
    X_kb = (B_kb - sum_j X_j L_kb,j^T) W_kb^T.  fault "transpose_w": the first block multiplied with the transposed inverse."""
    n = len(L)
    X = np.array(B, dtype=np.float64)
    for k, j in enumerate(range(0, n, QB)):
        e = min(n, j + QB)
        W = Ws[k].T if fault == "transpose_w" and j == 0 else Ws[k]
        if right:
            for i in range(0, j, QB):
                X[:, j:e] -= X[:, i:i + QB] @ L[j:e, i:i + QB].T
            X[:, j:e] = X[:, j:e] @ W.T
        else:
            for i in range(0, j, QB):
                X[j:e] -= L[j:e, i:i + QB] @ X[i:i + QB]
            X[j:e] = W @ X[j:e]
    return X
