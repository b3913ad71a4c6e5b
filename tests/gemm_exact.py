"""TEST INFRASTRUCTURE ONLY -- the fp64 tile product C <- C + alpha A^T B (csrc/eqf_tile.hpp: k_tile_gemm_tn; A is k x m, B is k x n, C is
m x n, all row-major) entry by entry: a reference, an a-priori bound, seeded operand families and a numpy model of the kernel's order with
injected faults.  numpy only, no GPU, nothing from oracle/.  tests/test_gemm_exact.py holds numpy's own product and the model against the
bound on the CPU, tests/test_gpu_tile_product.py the kernel.

Reference: C_ref = C + alpha A^T B in np.longdouble (64-bit mantissa on x86).

THE BOUND, entrywise, derived and not measured.  u = 2^-53, gamma_j = j u / (1 - j u):
    E = gamma_{k+2} |alpha| |A|^T |B| + u |C_ref|
      k      the k products of an entry summed in ANY order, with or without FMA, on the matrix cores or not: every product passes through
             its own rounding (none with FMA) and at most k - 1 additions -- (1 + theta_k) on each term [Higham, section 3.1]
      + 1    the rounding of alpha * acc (none for alpha = +-1: the bound does not use that)
      + 1    the addition to C (the L2's atomic add): its rounding relative to the SUM, whose two parts are then bounded apart -- the product
             part joins the gamma term, the other is u |C_ref| to first order (u |C_hat| <= u |C_ref| + u E, and u E is second order; the
             bound is formed with gamma_j = j u / (1 - j u), which absorbs it at these k)
    The zero fill of ragged chunks and tiles adds exact zeros.  Where E == 0 the result must be bit-equal to the reference rounded to fp64.
    INTEGER operands: if A, B, C and alpha hold integers and |alpha| |A|^T |B| + |C| < 2^53 at every entry, every product, every partial sum
    in any order, alpha * acc and the addition are exact in fp64: E = 0 everywhere (bound() tests this itself).
    The bound is formed in fp64: its own relative error, k u, is nothing next to the factor it is compared at.

Operand families (operands(family, m, n, k)), all seeded:
    normal      N(0, 1)
    scaled      N(0, 1) with the columns of A and of B scaled by 10^U(-6, 6), C by both: a normwise test sees only the few largest columns
    cancelling  row r + k // 2 of A is minus row r and row r + k // 2 of B is row r (1 + 1e-9 N(0, 1)): A^T B is nine orders below
                |A|^T |B| -- an entry is decided by the ORDER-independent part of the sum, and a lost or doubled k row is an O(1) miss
    integers    uniform integers in [-8, 8]: fp64 is exact, the bound is zero
    zero_column N(0, 1) with column m // 2 of A and column n // 3 of B all zero: those rows / columns of C keep their bits

The model (model(C, A, B, alpha, fault=None)) is the kernel's order in numpy fp64: 128 x 128 tiles, 16-row chunks zero-filled past k, four
products per step added to ONE accumulator per entry (the 16 x 16 x 4 matrix instruction), then alpha, then the addition.  Faults:
    drop_last_chunk   the last, ragged chunk is left out
    stale_buffer      chunk 1 is read from the buffer of chunk 0 (a missing barrier / a wrong buffer index)
    no_zero_fill      the rows past k of the ragged last chunk are not zeroed: they keep what the LDS buffer held, the same rows of chunk
                      nc - 3 (ones where there is no such chunk).  (The issue that asked for this module named the rows >= m of a ragged TILE;
                      those rows of C are never written -- the kernel tests R < m at the store -- and an operand column reaches only its own
                      row or column of C, so that fault cannot be seen.  k is the dimension on which the zero fill carries the result.)
    alpha_twice       C += alpha (alpha acc)
    transposed_tile   tile (0, 1) is added at tile (1, 0)'s place (needs two tile rows and two tile columns)
    column_shift      column m // 3 of A is read one column to the right"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
TILE, KC, STEP = 128, 16, 4
FAMILIES = ("normal", "scaled", "cancelling", "integers", "zero_column")
FAULTS = ("drop_last_chunk", "stale_buffer", "no_zero_fill", "alpha_twice", "transposed_tile", "column_shift")

assert np.finfo(LD).eps < 2e-19, "np.longdouble is not wider than fp64 here: the reference of this helper would be meaningless"

# ---- the shapes (m, n, k) both test modules use: each the smallest that reaches its edge of k_tile_gemm_tn -----------------------------------
LOOP = ((128, 128, 16), (128, 128, 32), (128, 128, 48), (128, 128, 49))   # nFast = 0 / one fast chunk / both LDS buffers reused / fast, then ragged
SHORT_K = tuple((s, s, k) for s in (128, 20) for k in (1, 3, 4, 5, 17))
MIXED = ((257, 129, 33),)                                                  # whole, ragged-row, ragged-column and corner tiles in one launch
EDGES = (1, 16, 17, 64, 65, 80, 81, 127)                                   # mu / nv: the 16-row sub-tiles of a wave's 64 x 64
EDGE_K = 20
SHAPES = LOOP + SHORT_K + MIXED + tuple((e, f, EDGE_K) for e, f in zip(EDGES, EDGES[::-1])) + tuple((e, e, EDGE_K) for e in (1, 65, 127))
ALPHAS = (-1.0, 1.0, 0.5, 0.3)


def gamma(j):
    return j * U / (1 - j * U)


def operands(family, m, n, k, seed=0):
    """(C (m, n), A (k, m), B (k, n)) in fp64"""
    rng = np.random.default_rng([11, FAMILIES.index(family), m, n, k, seed])
    if family == "integers":
        return tuple(rng.integers(-8, 9, s).astype(np.float64) for s in ((m, n), (k, m), (k, n)))
    C, A, B = rng.standard_normal((m, n)), rng.standard_normal((k, m)), rng.standard_normal((k, n))
    if family == "scaled":
        sa, sb = 10.0 ** rng.uniform(-6, 6, m), 10.0 ** rng.uniform(-6, 6, n)
        A, B, C = A * sa, B * sb, C * sa[:, None] * sb[None, :]
    if family == "cancelling":
        h = k // 2
        A[h:2 * h] = -A[:h]
        B[h:2 * h] = B[:h] * (1 + 1e-9 * rng.standard_normal((h, n)))
        C = C * 1e-9
    if family == "zero_column":
        A[:, m // 2] = 0.0
        B[:, n // 3] = 0.0
    return C, A, B


def reference(C, A, B, alpha):
    return C.astype(LD) + LD(alpha) * (A.astype(LD).T @ B.astype(LD))


def bound(C_ref, A, B, alpha, C=None):
    """E of the module docstring (fp64); all zeros for integer operands that fp64 holds exactly (needs C, the matrix the call started from)"""
    k = A.shape[0]
    G = abs(alpha) * (np.abs(A).T @ np.abs(B))
    if C is not None and all(np.array_equal(X, np.rint(X)) for X in (A, B, C)) and alpha == np.rint(alpha) and (G + np.abs(C)).max() < 2.0 ** 53:
        return np.zeros(G.shape)
    return gamma(k + 2) * G + U * np.abs(np.asarray(C_ref, dtype=np.float64))


def worst_ratio(got, C_ref, E):
    """(max |got - C_ref| / E, its index): where E is 0 the value must be C_ref exactly (ratio inf otherwise); a value that is not a number is
    outside every bound"""
    err = np.abs(np.asarray(got).astype(LD) - C_ref)
    b = np.asarray(E, dtype=np.float64).astype(LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, LD(0), np.where(b > 0, err / b, LD(np.inf)))
    r = np.where(np.isnan(r), LD(np.inf), r)
    at = int(np.argmax(r))
    return float(r.flat[at]), tuple(int(v) for v in np.unravel_index(at, r.shape))


def model(C, A, B, alpha, fault=None):
    """The kernel's order in numpy fp64 (module docstring); returns the new C"""
    assert fault is None or fault in FAULTS
    k, m = A.shape
    n = B.shape[1]
    nc = (k + KC - 1) // KC
    if fault == "column_shift":
        A = A.copy()
        j = m // 3
        A[:, j] = A[:, j + 1] if j + 1 < m else 0.0
    # the chunks as the LDS buffers hold them: zero-filled past k
    pad = nc * KC - k
    Ap, Bp = np.vstack([A, np.zeros((pad, m))]), np.vstack([B, np.zeros((pad, n))])
    chunks = [(Ap[c * KC:(c + 1) * KC], Bp[c * KC:(c + 1) * KC]) for c in range(nc)]
    if fault == "no_zero_fill" and pad:
        a, b = (x.copy() for x in chunks[-1])
        old = chunks[nc - 3] if nc >= 3 else (np.ones((KC, m)), np.ones((KC, n)))
        a[KC - pad:], b[KC - pad:] = old[0][KC - pad:], old[1][KC - pad:]
        chunks[-1] = (a, b)
    if fault == "stale_buffer" and nc >= 2:
        chunks[1] = chunks[0]
    if fault == "drop_last_chunk" and pad:
        chunks = chunks[:-1]
    out = np.array(C, dtype=np.float64)
    tm, tn = (m + TILE - 1) // TILE, (n + TILE - 1) // TILE
    for ti in range(tm):
        for tj in range(tn):
            I, J = slice(ti * TILE, min(m, (ti + 1) * TILE)), slice(tj * TILE, min(n, (tj + 1) * TILE))
            acc = np.zeros((I.stop - I.start, J.stop - J.start))
            for a, b in chunks:
                for s in range(0, KC, STEP):
                    acc = acc + a[s:s + STEP, I].T @ b[s:s + STEP, J]
            upd = alpha * acc
            if fault == "alpha_twice":
                upd = alpha * upd
            if fault == "transposed_tile" and (ti, tj) == (0, 1) and tm >= 2:
                r, c = min(I.stop - I.start, m - TILE), min(J.stop - J.start, TILE)
                out[TILE:TILE + r, 0:c] += upd[:r, :c]
                continue
            out[I, J] += upd
    return out


# ---- the block mask (csrc/eqf_device.hpp: GemmMask; csrc/eqf_tile.hpp: gemmTileActive) -------------------------------------------------------
def mask_kept(m, n, mask):
    """boolean (m, n): the entries on or above the staircase -- row block I <= column block J in the global block numbering"""
    rb, cb, rblk0, Pr, pr, cblk0, Pc, pc = mask
    I = (rblk0 + np.arange(m) // rb) * Pr + pr
    J = (cblk0 + np.arange(n) // cb) * Pc + pc
    return I[:, None] <= J[None, :]
