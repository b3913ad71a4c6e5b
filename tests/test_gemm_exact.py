"""The reference, the bound and the model of tests/gemm_exact.py on the CPU, for exactly the shapes and families tests/test_gpu_tile_product.py
holds k_tile_gemm_tn to -- no GPU.

(a) numpy's own A.T @ B (BLAS: another summation order, FMA or not) and the model of the kernel's order stay at ratio <= 1 on every family,
    shape and alpha; on the integer family both are bit-equal to the exact product (the bound is zero there).
(b) every fault of gemm_exact.FAULTS leaves the bound on the scaled-column family, where a normwise gate (1e-12 max|want|, the gate of
    test_tile_gemm_tn_against_numpy) sees only the largest columns; the table says for each fault and family whether that gate passes it.
(c) the mask helper agrees with the staircase of a 2 x 2 grid's rank (1, 0) written out by hand."""
import numpy as np
import pytest

import gemm_exact as gx


def _case(family, shape, alpha):
    m, n, k = shape
    C, A, B = gx.operands(family, m, n, k)
    ref = gx.reference(C, A, B, alpha)
    return C, A, B, ref, gx.bound(ref, A, B, alpha, C)


@pytest.mark.parametrize("family", gx.FAMILIES)
def test_numpy_and_the_model_stay_inside_the_bound(family):
    worst = {"numpy": 0.0, "model": 0.0}
    for shape in gx.SHAPES:
        for alpha in gx.ALPHAS if shape in gx.LOOP + gx.MIXED else (-1.0,):
            C, A, B, ref, E = _case(family, shape, alpha)
            for name, got in (("numpy", C + alpha * (A.T @ B)), ("model", gx.model(C, A, B, alpha))):
                r, at = gx.worst_ratio(got, ref, E)
                assert r <= 1.0, (family, shape, alpha, name, r, at)
                worst[name] = max(worst[name], r)
            if family == "integers" and alpha in (-1.0, 1.0):
                assert not E.any()
    print(f"family {family}: worst ratio to the bound  numpy {worst['numpy']:.3g}  model {worst['model']:.3g}")


def test_the_integer_family_has_a_zero_bound_only_where_fp64_is_exact():
    C, A, B = gx.operands("integers", 20, 20, 17)
    ref = gx.reference(C, A, B, -1.0)
    assert not gx.bound(ref, A, B, -1.0, C).any()
    assert gx.bound(ref, A, B, 0.3, C).all()                 # alpha * acc rounds
    assert gx.bound(ref, A * 2.0 ** 30, B * 2.0 ** 30, -1.0, C).all()   # the sums leave 2^53
    got = np.array(ref, dtype=np.float64)
    got[3, 4] += 1.0
    assert gx.worst_ratio(got, ref, np.zeros(got.shape)) == (np.inf, (3, 4))
    got[3, 4] = np.nan
    assert gx.worst_ratio(got, ref, np.ones(got.shape))[0] == np.inf


@pytest.mark.parametrize("shape,alpha", [((257, 129, 33), -1.0), ((257, 129, 33), 0.3), ((130, 130, 49), -1.0)])
def test_injected_faults_leave_the_bound(shape, alpha):
    """Every fault is outside the bound on the scaled-column family (and, printed, on the others); beside it what the normwise gate
    |got - want| <= 1e-12 max|want| makes of it."""
    missed = []
    for fault in gx.FAULTS:
        row = []
        for family in gx.FAMILIES:
            C, A, B, ref, E = _case(family, shape, alpha)
            got = gx.model(C, A, B, alpha, fault=fault)
            r, _ = gx.worst_ratio(got, ref, E)
            want = np.asarray(ref, dtype=np.float64)
            gate = np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
            row.append(f"{family} {r:.3g}{' (PASSES the normwise gate)' if gate else ''}")
            if family == "scaled" and not r > 1.0:
                missed.append((fault, family, r))
        print(f"shape {shape} alpha {alpha} fault {fault:16s} ratio to the bound  " + "   ".join(row))
    assert not missed, missed


def test_the_scaled_family_hides_small_columns_from_a_normwise_gate():
    """A 16 x 16 sub-tile of the scaled family's product dropped altogether -- the one at the sixteen smallest columns of A and of B -- passes
    1e-12 max|want| and is a miss of many orders entry by entry: why the kernel is held to the bound and not to a norm."""
    C, A, B, ref, E = _case("scaled", (128, 128, 48), -1.0)
    want = np.asarray(ref, dtype=np.float64)
    ix = np.ix_(np.argsort(np.abs(A).max(axis=0))[:16], np.argsort(np.abs(B).max(axis=0))[:16])
    got = want.copy()
    got[ix] = C[ix]
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert gx.worst_ratio(got, ref, E)[0] > 1e6


def test_mask_helper_on_a_two_by_two_grid():
    kept = gx.mask_kept(300, 300, (100, 100, 0, 2, 1, 0, 2, 0))   # rank (1, 0): row blocks 1, 3, 5; column blocks 0, 2, 4
    want = np.zeros((300, 300), dtype=bool)
    want[0:100, 100:300] = True
    want[100:200, 200:300] = True
    assert np.array_equal(kept, want)
