"""Test helper: a numpy model of the int8-slice products, operation for operation (CPU only; like tiled_double.py for the tile kernels).

Three entry points share one construction (csrc/eqf_i8.hpp: k_i8_colexp / k_i8_split / k_i8_gemm behind eqf_tile_downdate_i8 and
eqf_tile_gemm_tn_i8; k_i8dd_split / k_i8dd_syrk behind eqf_tile_syrk_i8 and the handles' "downdate_slices"):

  1. exponent word per column: 0 = all zero, NONFINITE = holds a NaN / Inf, else frexp(max |entry|) + 2048;
  2. every entry scaled to r = ldexp(x, -e) (|r| < 1, correctly rounded) and cut into S signed slices, q_t = rint(r 2^(6 + 7 t)) (ties to
     even, |q_t| <= 64), r -= q_t 2^-(6 + 7 t) (exact);
  3. per d = ta + tb < S the exact integer accumulator acc_d = sum over k and over the pairs (ta, tb) of q_ta q_tb;
  4. v = sum_d acc_d 2^-(12 + 7 d) in fp64, d = S - 1 down to 0 (every term exact, S - 1 roundings);
  5. the epilogue: tile C += alpha ldexp(v, e_i + e_j) (NaN for a flagged row / column), syrk Sout = Sin - ldexp(v, e_i + e_j) on the
     upper triangle, mirrored.

Every step is reproduced with the same IEEE operations, so a correct kernel equals this model BIT FOR BIT.  (The kernels' fma(-q, 2^-w, r) is
exact, hence equal to the plain subtraction here; their "*dst += alpha * t" with alpha = -1 may be contracted to an fma, which is exact in the
product and so gives the same result as the subtraction here.)  The int32 accumulators are formed as float64 matrix products of the slices:
every partial sum is an integer below 2^53, so BLAS forms them exactly whatever its order.

Error bound (rigorous).  For finite, non-zero columns i of A and j of B with exponents e_i, e_j and k rows, let a = x 2^-e_i (|a| < 1) and
likewise b.  The scaled value is rounded only when it underflows (|fl(a) - a| <= eta = 2^-1075).  After S slices the remainder of the last
rint is at most half a unit of 2^-(6 + 7 (S - 1)): |a - a^| <= tau = 2^-7S + eta, the same for b.  The pairs with ta + tb >= S are dropped;
with |q| <= 64 each dropped d contributes at most (2 S - 1 - d) 64^2 2^-(12 + 7 d), together DROP_S = sum_{d=S}^{2S-2} (2 S - 1 - d) 2^-7d
per row.  So the exact kept sum V = sum_d acc_d 2^-(12 + 7 d) obeys
    |V - sum_k a_k b_k| <= k (|a - a^| |b| + |a^| |b - b^| + DROP_S) <= k (2 tau + tau^2 + DROP_S).
The fp64 sum of the S exact terms adds at most gamma_{S-1} sum_d |acc_d| 2^-(12 + 7 d) <= gamma_{S-1} k THETA_S with THETA_S =
sum_{d<S} (d + 1) 2^-7d and gamma_n = n u / (1 - n u), u = 2^-53; ldexp(v, e_i + e_j) is exact unless it underflows (2^-1075 more).  Hence
    |ldexp(v, e_i + e_j) - (A^T B)_ij| <= 2^(e_i + e_j) k (2 tau + tau^2 + DROP_S + gamma_{S-1} THETA_S) + 2^-1075          (bound())
which is about (2 + (S - 1)) 2^-7S k 2^(e_i + e_j): the truncation gives the 2, the dropped pairs the (S - 1).  The suite's older bound,
k ca cb 2^-(5 + 7 (S - 1)) = 4 k ca cb 2^-7S (ca, cb the columns' largest |entry|, in [2^(e-1), 2^e)), holds for random data, where the
errors of the k rows largely cancel, but not for every input: all-63 digits (all63()) exceed it (test_i8_emulator.py)."""
from fractions import Fraction

import numpy as np

BITS = 7
NONFINITE = 4096  # the exponent word of a column holding a NaN / Inf (eqf_i8.hpp kI8NonFinite): above every exponent + 2048


def exponent_words(X, skip_col=-1):
    """Exponent word of every column of X (k x n): 0 all zero, NONFINITE holds a NaN / Inf, else frexp's exponent of the largest |entry| +
    2048.  skip_col: a column that is not part of the operand (the handles' z column of Y): word 0."""
    X = np.asarray(X, dtype=np.float64)
    fin = np.isfinite(X)
    mx = np.where(fin, np.abs(X), 0.0).max(axis=0, initial=0.0)
    e = np.frexp(mx)[1].astype(np.int64)
    w = np.where(~fin.all(axis=0), NONFINITE, np.where(mx > 0, e + 2048, 0)).astype(np.int64)
    if skip_col >= 0 and skip_col < w.size:
        w[skip_col] = 0
    return w


def slices(X, words, S):
    """The S slices of X's columns as float64 integers, shape (S, k, n); columns with word 0 or NONFINITE are all zero."""
    X = np.asarray(X, dtype=np.float64)
    live = (words > 0) & (words != NONFINITE)
    e = np.where(live, words - 2048, 0)
    r = np.ldexp(np.where(live[None, :], X, 0.0), -e[None, :])  # correctly rounded: exact unless it underflows
    out = np.empty((S,) + X.shape)
    w = 64.0
    for t in range(S):
        q = np.rint(r * w)  # ties to even, |q| <= 64
        out[t] = q
        r = r - q / w       # exact (the kernel's fma(-q, 1 / w, r))
        w *= 128.0
    return out


def accumulators(qa, qb):
    """acc_d = sum_{ta + tb = d} qa[ta]^T qb[tb], d < S: int64, shape (S, m, n).  Exact (integers below 2^53 throughout)."""
    S = qa.shape[0]
    acc = np.zeros((S, qa.shape[2], qb.shape[2]))
    for ta in range(S):
        for tb in range(S - ta):
            acc[ta + tb] += qa[ta].T @ qb[tb]
    return acc.astype(np.int64)


def recombine(acc):
    """v = sum_d acc_d 2^-(12 + 7 d) in fp64, in the kernels' order (d = S - 1 first)."""
    S = acc.shape[0]
    v = np.zeros(acc.shape[1:])
    for d in range(S - 1, -1, -1):
        v = v + np.ldexp(acc[d].astype(np.float64), -(12 + BITS * d))
    return v


class Product:
    """The int8-slice product A^T B (A k x m, B k x n) up to the epilogue: exponent words eA / eB, accumulators acc, recombined v and
    the product term P = ldexp(v, e_i + e_j) (0 where a column is zero, NaN where one is flagged)."""

    def __init__(self, A, B, S, skip_col=-1):
        self.S = S
        self.eA = exponent_words(A, skip_col)
        self.eB = exponent_words(B, skip_col)
        self.acc = accumulators(slices(A, self.eA, S), slices(B, self.eB, S))
        self.v = recombine(self.acc)
        bad = (self.eA == NONFINITE)[:, None] | (self.eB == NONFINITE)[None, :]
        zero = (self.eA == 0)[:, None] | (self.eB == 0)[None, :]
        live = ~bad & ~zero
        ee = np.where(live, (self.eA - 2048)[:, None] + (self.eB - 2048)[None, :], 0)
        with np.errstate(over="ignore"):
            self.P = np.where(live, np.ldexp(self.v, ee), 0.0)
        self.P[bad] = np.nan
        self.live, self.bad = live, bad

    @property
    def max_acc(self):
        return int(np.abs(self.acc).max()) if self.acc.size else 0


def tile_skipped(m, n, mask, mask_cols):
    """k_i8_gemm's workgroup skip (128 rows x 64 columns of C): True where a whole workgroup tile lies inside the first mask_cols columns and
    entirely below the block diagonal of GemmMask (rb, cb, rblk0, Pr, pr, cblk0, Pc, pc)."""
    skip = np.zeros((m, n), dtype=bool)
    if mask is None or mask[0] <= 0:
        return skip
    rb, cb, rblk0, Pr, pr, cblk0, Pc, pc = mask
    for y in range((m + 127) // 128):
        for x in range((n + 63) // 64):
            c0, r0 = 64 * x, 128 * y
            if c0 + 63 < mask_cols:
                ilo = (rblk0 + r0 // rb) * Pr + pr
                jhi = (cblk0 + (c0 + 63) // cb) * Pc + pc
                if ilo > jhi:
                    skip[r0: r0 + 128, c0: c0 + 64] = True
    return skip


def tile_gemm(C, A, B, S, alpha=-1.0, mask=None, mask_cols=0):
    """eqf_tile_gemm_tn_i8 / eqf_tile_downdate_i8 (alpha = -1): C (m x n) after C += alpha A^T B.  Elements of skipped workgroup tiles and
    of all-zero columns are untouched; a flagged row / column is NaN.  (A as a column range of B cut once gives the same result: the
    exponent words and slices of a column do not depend on which operand it was cut with.)"""
    C = np.array(C, dtype=np.float64)
    p = Product(A, B, S)
    keep = ~tile_skipped(C.shape[0], C.shape[1], mask, mask_cols)
    upd = keep & p.live
    C[upd] = C[upd] + alpha * p.P[upd]
    C[keep & p.bad] = np.nan
    return C


def syrk(Sin, Y, S, skip_col=-1):
    """eqf_tile_syrk_i8 / k_i8dd_syrk for one filter: Sin (nv x nv), Y (mp x nv), mp == 0 copies.  Sout = Sin - P on and above the diagonal,
    the lower triangle the mirror image of the upper one; a flagged column's row and column NaN."""
    Sin = np.asarray(Sin, dtype=np.float64)
    if Y.shape[0] == 0:
        return Sin.copy()
    p = Product(Y, Y, S, skip_col)
    out = Sin - p.P
    low = np.tril_indices(out.shape[0], -1)
    out[low] = out.T[low]  # (assigned, not added: -0.0 keeps its sign)
    return out


def drop_s(S):
    return sum((2 * S - 1 - d) * Fraction(1, 2 ** (7 * d)) for d in range(S, 2 * S - 1))


def theta_s(S):
    return sum((d + 1) * Fraction(1, 2 ** (7 * d)) for d in range(S))


def bound_factor(S):
    """The rigorous bound of the module docstring per row and per unit of 2^(e_i + e_j), as a Fraction."""
    u = Fraction(1, 2 ** 53)
    tau = Fraction(1, 2 ** (7 * S)) + Fraction(1, 2 ** 1075)
    gamma = (S - 1) * u / (1 - (S - 1) * u)
    return 2 * tau + tau * tau + drop_s(S) + gamma * theta_s(S)


def bound(k, ea, eb, S):
    """Rigorous |ldexp(v, e_i + e_j) - (A^T B)_ij| bound for exponent words ea, eb (both live) over k rows (float64 matrix, rounded up)."""
    f = float(bound_factor(S)) * (1 + 2.0 ** -50)
    ee = (np.asarray(ea) - 2048)[:, None] + (np.asarray(eb) - 2048)[None, :]
    return np.ldexp(k * f, ee) + 2.0 ** -1074


def old_bound(A, B, S):
    """The suite's statistical bound k ca cb 2^-(5 + 7 (S - 1)) (tests/test_gpu_tiled.py, without its 1.01 slack)."""
    return A.shape[0] * np.outer(np.abs(A).max(axis=0), np.abs(B).max(axis=0)) * 2.0 ** -(5 + 7 * (S - 1))


def exact_product(A, B):
    """A^T B exactly, as a matrix of Fractions (small shapes: Python integers at the scale 2^-1074 of the smallest subnormal)."""
    def ints(X):
        out = np.empty(X.shape, dtype=object)
        for idx, x in np.ndenumerate(np.asarray(X, dtype=np.float64)):
            num, den = float(x).as_integer_ratio()  # (den a power of two <= 2^1074)
            out[idx] = num * (2 ** 1074 // den)
        return out

    s = ints(A).T.dot(ints(B))
    scale = Fraction(1, 2 ** 2148)
    return np.array([[Fraction(int(x)) * scale for x in row] for row in s], dtype=object)


def max_error_ratio(p, exact, S, k):
    """max over live elements of |P - exact| / bound (Fractions: exact comparison)."""
    f = bound_factor(S)
    worst = Fraction(0)
    m, n = p.P.shape
    for i in range(m):
        for j in range(n):
            if not p.live[i, j]:
                continue
            b = k * f * Fraction(2) ** int(p.eA[i] + p.eB[j] - 4096) + Fraction(1, 2 ** 1075)
            worst = max(worst, abs(Fraction(float(p.P[i, j])) - exact[i, j]) / b)
    return float(worst)


def all63(k, n, S_digits=7, e=0):
    """k x n, every entry 2^e sum_{t < S_digits} 63 2^-(6 + 7 t): every 7-bit digit of the scaled entries is 63 (the largest that rounds
    down), so every slice is 63 and the truncation and the dropped pairs all have the same sign -- the near-worst case of the bound and
    the largest accumulators (k S 63^2) a finite input gives."""
    x = sum(63.0 * 2.0 ** -(6 + 7 * t) for t in range(S_digits))
    return np.full((k, n), np.ldexp(x, e))


def bits_equal(a, b):
    """Same NaN pattern and, elsewhere, the same bits (so -0.0 != 0.0)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return False
    return bool(np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64)))
