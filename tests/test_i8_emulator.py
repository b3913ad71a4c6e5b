"""The numpy model of the int8-slice products (tests/i8_emulator.py) on the CPU: against the exact product within its rigorous bound, the
suite's older bound shown to be statistical only, and the integer accumulators at the two exactness limits (eqf_tile_gemm_tn_i8's
k <= 70 000, eqf_tile_syrk_i8's i8Exact) -- what tests/test_gpu_i8_exact.py drives the kernels to, bit for bit."""
import numpy as np
import pytest

import i8_emulator as E

K_MAX_TILE = 70000  # eqf_tile_gemm_tn_i8 / eqf_tile_downdate_i8 reject k > 70 000 (eqf_tiled.hip)


def mp_limit(S):
    """The largest multiple of 32 that eqf_i8.hpp's i8Exact accepts: mp S 64^2 < 2^31."""
    mp = (2 ** 31 - 1) // (S * 4096)
    return mp // 32 * 32


def _exact_ratio(A, B, S):
    p = E.Product(A, B, S)
    return E.max_error_ratio(p, E.exact_product(A, B), S, A.shape[0]), p


@pytest.mark.parametrize("S", [5, 6, 7])
def test_emulator_within_the_rigorous_bound(S):
    """N(0, 1) data, columns spanning 10^-150 .. 10^150, subnormal columns against huge ones, and the all-63 input: the emulated product
    term never leaves bound() (exact rational comparison).  The all-63 input comes within 10 % of it at S = 5, 6: the bound is sharp."""
    rng = np.random.default_rng(S)
    k, m, n = 40, 6, 5
    A = rng.standard_normal((k, m))
    B = rng.standard_normal((k, n))
    r, _ = _exact_ratio(A, B, S)
    assert r <= 1.0, r
    A = rng.standard_normal((k, m)) * 10.0 ** rng.uniform(-150, 0, size=(1, m))
    B = rng.standard_normal((k, n)) * 10.0 ** rng.uniform(-150, 150, size=(1, n))
    A[:, 0] = rng.standard_normal(k) * 1e-318  # subnormal entries, a subnormal maximum
    B[:, 1] = rng.standard_normal(k) * 1e300   # (against A's columns <= ~1: no overflow)
    B[3, 2] = 1e-310                         # a column whose largest entry dwarfs a subnormal one
    r, p = _exact_ratio(A, B, S)
    assert r <= 1.0, r
    assert p.eA[0] - 2048 < -1023            # (what the old splitters turned into an infinite scale factor)
    A, B = E.all63(64, 3, e=2), E.all63(64, 2, e=-5)
    r, _ = _exact_ratio(A, B, S)
    assert (0.9 if S < 7 else 0.6) <= r <= 1.0, r  # (S = 7 holds all seven digits: only the dropped pairs are left)


@pytest.mark.parametrize("S,over", [(5, 1.4), (6, 1.6), (7, 1.4)])
def test_all63_exceeds_the_old_bound(S, over):
    """The suite's older bound k ca cb 2^-(5 + 7 (S - 1)) is statistical: on random columns the k rows' errors cancel, but with every
    scaled digit 63 the truncation (up to 2 x 2^-7S per row) and the dropped slice pairs ((S - 1) x 2^-7S) all add up with one sign, and a
    CORRECT kernel exceeds it -- by 1.49, 1.73 and 1.48 at S = 5, 6, 7 (1.47, 1.72, 1.46 over the tests' bound with its 1.01 slack; at S = 7
    all seven digits are kept and the dropped pairs alone do it), while staying inside the rigorous bound.  The GPU tests therefore
    compare bit for bit with the emulator rather than with a bound."""
    k = 64
    A, B = E.all63(k, 2), E.all63(k, 2)
    p = E.Product(A, B, S)
    exact = E.exact_product(A, B)
    err = np.array([[abs(float(p.P[i, j] - float(exact[i, j]))) for j in range(2)] for i in range(2)])
    ratio = float((err / E.old_bound(A, B, S)).max())
    assert ratio >= over, ratio
    assert E.max_error_ratio(p, exact, S, k) <= 1.0


def test_the_model_is_the_documented_arithmetic():
    """Small hand-checked cases: ties to even in every slice, the q0 = 64 column maximum 2^e (1 - 2^-53), an exact power of two, the flag
    words, zero / -0.0 columns, the syrk mirror and copy."""
    x = 1.0 - 2.0 ** -53
    w = E.exponent_words(np.array([[x, 0.0, -0.0, 4.0, np.nan], [0.5, 0.0, 0.0, -1.0, 1.0]]))
    assert list(w) == [2048, 0, 0, 2048 + 3, E.NONFINITE]
    q = E.slices(np.array([[x], [2.5 / 64], [3.5 / 64], [-2.5 / 64], [1.5 * 2.0 ** -13]]), np.array([2048]), 3)
    assert q[0, 0, 0] == 64 and q[1, 0, 0] == 0                              # q0 = 64, the rest exact
    assert q[0, 1, 0] == 2 and q[0, 2, 0] == 4 and q[0, 3, 0] == -2         # ties to even
    assert q[1, 1, 0] == 64 and q[1, 3, 0] == -64                            # (their remainders, exact)
    assert q[0, 4, 0] == 0 and q[1, 4, 0] == 2                               # a tie one slice down
    Y = np.array([[1.0, 0.0, 2.0], [3.0, 0.0, -1.0]])
    Sin = np.arange(9.0).reshape(3, 3) - 4.0
    Sin = Sin + Sin.T
    Sin[1, 1] = -0.0
    out = E.syrk(Sin, Y, 6)
    assert E.bits_equal(out[1], Sin[1]) and np.array_equal(out, out.T)      # a zero column: its row copied, -0.0 kept
    assert np.allclose(out, np.triu(Sin) + np.triu(Sin, 1).T - Y.T @ Y, rtol=0, atol=1e-9)
    assert E.bits_equal(E.syrk(Sin, Y[:0], 6), Sin)                        # mp = 0: a copy
    Y[1, 2] = np.inf
    out = E.syrk(Sin, Y, 6)
    assert np.isnan(out[2]).all() and np.isnan(out[:, 2]).all() and np.isfinite(out[:2, :2]).all()
    C = np.zeros((3, 3))
    A = np.ones((4, 3))
    A[0, 1] = np.nan
    got = E.tile_gemm(C, A, np.zeros((4, 3)), 5)
    assert np.isnan(got[1]).all() and E.bits_equal(got[[0, 2]], C[[0, 2]])  # NaN poisons even against a zero column


@pytest.mark.parametrize("S", [5, 6, 7])
def test_tile_skip_matches_the_staircase(S):
    """tile_skipped only ever drops elements strictly below the block diagonal, inside the masked columns."""
    mask = (100, 100, 2, 2, 1, 1, 2, 0)
    m, n, mc = 500, 509, 500
    sk = E.tile_skipped(m, n, mask, mc)
    I = (2 + np.arange(m) // 100) * 2 + 1
    J = (1 + np.arange(n) // 100) * 2 + 0
    below = I[:, None] > J[None, :]
    below[:, mc:] = False
    assert sk.any() and not (sk & ~below).any()


def test_accumulators_at_the_exactness_limits():
    """The all-63 input makes acc_{S-1} = k S 63^2, the largest a finite input gives: at eqf_tile_gemm_tn_i8's k = 70 000 (S = 7) and at
    the largest mp eqf_tile_syrk_i8 accepts (S = 5, 6, 7) it stays below 2^31 and above 0.9 x 2^31 -- the GPU test at those sizes sits at
        the edge of int32.  One step further for the syrk (mp + 32) the bound the host checks, mp S 64^2, is past 2^31; the tile entry
    points' k limit is a round number below theirs (74 898 at S = 7)."""
    k = K_MAX_TILE
    acc = k * 7 * 63 * 63
    assert 0.9 * 2 ** 31 <= acc < 2 ** 31
    p = E.Product(E.all63(k, 2), E.all63(k, 2), 7)
    assert p.max_acc == acc
    for S in (5, 6, 7):
        mp = mp_limit(S)
        assert mp * S * 4096 < 2 ** 31 <= (mp + 32) * S * 4096
        acc = mp * S * 63 * 63
        assert 0.9 * 2 ** 31 <= acc < 2 ** 31, S
        p = E.Product(E.all63(mp, 1), E.all63(mp, 1), S)
        assert p.max_acc == acc, S
