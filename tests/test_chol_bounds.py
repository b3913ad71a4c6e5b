"""The bounds of tests/chol_bounds.py on the CPU: LAPACK and the numpy model of the kernels' blocked, explicit-inverse algorithm lie inside
them on every input meant for the device tests of these kernels, the model does NOT lie inside the textbook bound (which is why that one is
not asserted), and a model with one block left out, one inverse transposed or one pivot from the wrong lane breaks them.

Measured (worst over all families, sizes and both variants of the model): the model 0.31 of the factorisation bound -- at n = 1, where the
pivot's own p is most of the bound; 0.12 from n = 16 on -- (the plain, T = I, bound: exceeded, 1.33 times on graded(17, 8)), 0.09 of the
solve bounds, 0.39 of the record bound; LAPACK 0.18 of the factorisation bound."""
import numpy as np
import pytest

import chol_bounds as cb

_TRSM_M = 70


def _rhs(A, m, seed):
    """right-hand sides whose rows have the scale of the factor's rows: B scaled row-wise by sqrt(diag A)"""
    rng = np.random.default_rng([5, len(A), m, seed])
    return rng.standard_normal((len(A), m)) * np.sqrt(np.diag(A))[:, None]


@pytest.mark.parametrize("n", cb.POTRF_SIZES)
def test_lapack_and_the_model_lie_inside_the_bounds(n):
    """Both variants of the model -- block = 16, every panel row through the explicit inverse, and block = 64, the kernels' mix -- with
    their own factor and inverse blocks in the factorisation, both solves and the records"""
    worst = dict(lapack=0.0, model=0.0, model_plain=0.0, left=0.0, right=0.0, record=0.0)
    up = lambda k, v: worst.__setitem__(k, max(worst[k], v))
    for label, A in cb.family_cases(n):
        Lref = np.linalg.cholesky(A)  # (raises if LAPACK does not factor it)
        Tref = cb.block_T(Lref)
        up("lapack", cb.potrf_ratio(A, Lref, Lref, Tref)[0])
        for block in (16, 64):
            L, Ws = cb.model_chol16(A, block=block)
            aware, plain = cb.potrf_ratio(A, L, Lref, Tref)
            up("model", aware)
            up("model_plain", plain)
            T = cb.block_T(L)
            for m in (1, _TRSM_M):
                B = _rhs(A, m, 0)
                up("left", cb.trsm_left_ratio(L, cb.model_trsm16(L, Ws, B), B, T)[0])
                Bt = np.ascontiguousarray(B.T)
                up("right", cb.trsm_right_ratio(L, cb.model_trsm16(L, Ws, Bt, right=True), Bt, T)[0])
            for k, W in enumerate(Ws):
                up("record", cb.record_ratio(W, L[16 * k: 16 * k + len(W), 16 * k: 16 * k + len(W)]))
        assert max(worst[k] for k in ("lapack", "model", "left", "right", "record")) <= 1.0, (label, worst)
    print(f"n={n}: worst ratio to bound {worst}")


def test_the_model_exceeds_the_plain_bound():
    """graded(17, 8): the one-row second block column is a product with the inverse of a 16 x 16 block of condition 1e4 -- outside
    gamma_{n+1} |L| |L^T|, inside the bound that knows T.  LAPACK, which substitutes, is inside both."""
    A = cb.graded(17, 8)
    Lref = np.linalg.cholesky(A)
    aware, plain = cb.potrf_ratio(A, cb.model_chol16(A)[0], Lref)
    assert plain > 1.0 and aware <= 1.0, (aware, plain)
    assert cb.potrf_ratio(A, Lref, Lref)[1] <= 1.0


@pytest.mark.parametrize("fault,n", [("drop_trailing", 17), ("drop_trailing", 100), ("drop_trailing", 193), ("transpose_w", 65),
                                     ("transpose_w", 193), ("wrong_lane", 16), ("wrong_lane", 100)])
def test_a_faulty_factorisation_breaks_the_bound(fault, n):
    """one 16 x 16 block of one trailing update left out / one panel multiplied with W instead of W^T / one pivot's square root taken from the
    neighbouring lane: outside the factorisation bound on EVERY family -- the bound is not so wide that it forgives a wrong kernel"""
    block = 64 if fault == "transpose_w" else 16  # (as in the kernels, a panel is only multiplied with W below the 64-block)
    for label, A in cb.family_cases(n):
        assert cb.potrf_ratio(A, cb.model_chol16(A, fault=fault, block=block)[0])[0] > 1.0, label


@pytest.mark.parametrize("n", [17, 65, 193])
def test_a_faulty_solve_or_record_breaks_its_bound(n):
    for label, A in cb.family_cases(n):
        L, Ws = cb.model_chol16(A)
        B = _rhs(A, 5, 1)
        assert cb.trsm_left_ratio(L, cb.model_trsm16(L, Ws, B, fault="transpose_w"), B)[0] > 1.0, label
        Bt = np.ascontiguousarray(B.T)
        assert cb.trsm_right_ratio(L, cb.model_trsm16(L, Ws, Bt, right=True, fault="transpose_w"), Bt)[0] > 1.0, label
        assert cb.record_ratio(Ws[0].T, L[:16, :16]) > 1.0, label
        # a solve against ANOTHER factor (LAPACK's: the same matrix to rounding) is still inside: the bound follows its operand
        Lref = np.linalg.cholesky(A)
        assert cb.trsm_left_ratio(Lref, cb.model_trsm16(Lref, cb.block_inverses(Lref), B), B)[0] <= 1.0, label


@pytest.mark.parametrize("n", [16, 40, 64, 100, 128, 200])
def test_failure_inputs_are_refused_and_controls_factor(n):
    for label, A in cb.bad_inputs(n):
        outcome, L = cb.lapack_outcome(A)
        if not label.startswith("nan"):
            assert outcome == "raises", label
            continue
        # A NaN on the diagonal: reference LAPACK raises (its test is `pivot <= 0 or isnan(pivot)`), an optimised dpotrf that tests
        # `pivot <= 0` alone lets the NaN through (cb.lapack_outcome).  Either refuses the matrix; which of the two this numpy does is
        # pinned down, so that neither branch can quietly become "anything goes": a factor that came back holds the NaN AT the bad pivot.
        assert outcome in ("raises", "nan_factor"), (label, outcome)
        if outcome == "nan_factor":
            q = int(label[4:-1])
            assert np.isnan(L[q, q]) and np.isfinite(L[:q, :q]).all(), label
    labels = [l for l, _ in cb.bad_inputs(n)]
    assert len(labels) == len(set(labels)) and len(labels) >= 3 * 3 + 1
    for label, A in cb.control_inputs(n):
        L = np.linalg.cholesky(A)
        assert np.isfinite(L).all() and (np.diag(L) > 0).all(), label
    np.linalg.cholesky(cb.spd_base(n))
