"""The partitioned filter's vision update entry by entry at block sizes that reach its production code paths -- the protocol and check() of
tests/test_gpu_update.py::test_partitioned_filter (one processVisionData on a 1 x 1 grid after initialise_from(snapshot); Sigma+, gamma,
delta and, where asserted, Gamma[0:6] at ratio <= 1 at every entry; symmetry, finiteness, the bias step, both error flags) on
update_cases.TILED_BIG, where tests/riccati_cases.TILED (block rows of 16 .. 48 rows) stops short of them.

The bound is update_exact.update_bounds with the counted terms of the block-row schedule (update_cases.tiled_schedule; derivation in
update_exact's docstring, "The partitioned filter"): one addition per block row, one per level of a split solve, and under "solve_inverse"
the whole-block T.  Nothing in it comes from the device; tests/test_update_exact.py holds a numpy restatement of the schedule to the same
bounds on the CPU and sees three schedule faults leave them.

Measured on an MI355X (each test prints its own; NOTES.md R35.2): every ratio <= 0.27, every bit-equality holds; the figures are in the tests'
docstrings.  The device sits where the CPU restatement of the schedule sits (Sigma+ 0.005 / 0.004 / 0.05 / 0.005 on a / b / c / e at (200, 64))."""
import numpy as np
import pytest

import test_gpu_update as gu
import update_cases as uc
import update_exact as ux

pytestmark = pytest.mark.gpu

_BOUNDS = {}
KEYS = ("Sp", "gamma", "Gamma", "bias_after")


@pytest.fixture(scope="module")
def hip():
    from eqf_vio_amd import binding

    return binding


def reference(hip, N, bl, fam, solve_inverse=False, trsm_leaf=0):
    """(S0, call, ref, bounds of the schedule): the reference once per (N, family) for the whole session (test_gpu_update's cache), the
    bound once per schedule"""
    S0, call, ref, bd = gu.reference(hip, N, fam)
    sched = uc.tiled_schedule(N, bl, solve_inverse, trsm_leaf)
    key = (N, fam) + tuple(sorted(sched.items()))
    if key not in _BOUNDS:
        _BOUNDS[key] = ux.update_bounds(ref, bd["parts"]["E_ric"], **sched)
    return S0, call, ref, _BOUNDS[key]


def one_update(hip, N, bl, fam, options=()):
    """test_partitioned_filter's protocol with `options` ((name, value), ...) set on the filter -> what check() reads"""
    from eqf_vio_amd import tiled

    S0, (stamp, ids, y), _, _ = reference(hip, N, bl, fam)
    be = tiled.HipBackend(uc.settings(), capacity=N + 5)
    tf = tiled.TiledFilter(tiled.ProcessGrid(None, 1, 1, device=be.device), be, bl)
    try:
        tf.burst = False
        for name, value in options:
            tf._opt(name, value)
        tf.initialise_from(dict(gu.snapshot(hip, N), sigma=S0))
        before = tf.bias()
        assert tf.processVisionData(stamp, ids, y) == 0
        tf.check()
        lu = tf.lastUpdate()
        out = dict(Sp=tf.stateCovariance(), delta=lu["delta"], gamma=lu["gamma"], Gamma=lu["Gamma"], bias_before=before, bias_after=tf.bias())
        assert be.device_error() == 0 and tf.device_error() == 0
    finally:
        tf.close()
    return out


def held(hip, N, bl, fams, options, what, solve_inverse=False, trsm_leaf=0):
    worst, bad = {}, []
    for fam in fams:
        _, _, ref, bd = reference(hip, N, bl, fam, solve_inverse, trsm_leaf)
        gu.check(one_update(hip, N, bl, fam, options), N, fam, ref, bd, (what, N, bl), worst, bad)
    gu.report(f"partitioned filter, N = {N}, blocks of {bl}, {what}", worst)
    assert not bad, bad[:10]


@pytest.mark.parametrize("N,bl", uc.TILED_BIG)
def test_partitioned_filter_at_production_block_sizes(hip, N, bl):
    """Default options, all four families.  What each case reaches (csrc/eqf_tiledf.hip: Chain::step, trsmLeft; csrc/eqf_tile.hpp;
    csrc/eqf_tiled.hip: eqf_tile_potrf):
    (200, 64): block rows of 64, 64, 64 and 8 landmarks -- more than two, the last one ragged.  S-chain: diagonal blocks of 128 rows, so the
        trailing products have whole 128 x 128 tiles and, with k = 128, seven straight-line chunks each (k_tile_gemm_tn: whole, nFast =
        k / 16 - 1); eqf_tile_potrf with two 64-blocks in one workgroup.  E-chain: diagonal blocks of 192 rows -- the blocked potrf with
        nb = 3 (nb > 2): k_tile_trsm on the panel and k_tile_potrf_trail per block column.
    (230, 108): block rows of 108, 108 and 14 landmarks.  E-chain: diagonal blocks of 324 rows, nb = 6 = kTrsmSplit, and the first block
        row's right-hand side is 701 - 324 = 377 >= 256 columns wide: trsmLeft splits with h = 64 (6 / 2) = 192 -- the strip solve on 192
        rows, L21 (132 x 192) transposed, one product, the strip solve on 132 rows.  S-chain: diagonal blocks of 216 rows, blocked potrf
        with nb = 4.
    Measured worst ratios on families a / b / c / e:
    (200, 64)   Sigma+ 0.0059 / 0.0056 / 0.027 / 0.0059, gamma 0.00058 / 0.00034 / 0.14 / 0.00022, delta 0.19 .. 0.25, Gamma[0:6] 9.1e-5 / - /
                0.0053 / 8.6e-6, symmetry <= 0.0024
    (230, 108)  Sigma+ 0.0063 / 0.0053 / 0.021 / 0.0063, gamma 0.00097 / 0.00030 / 0.19 / 0.00026, delta 0.22 .. 0.25, Gamma[0:6] 0.00012 / - /
                0.0076 / 1.0e-5, symmetry <= 0.009"""
    held(hip, N, bl, uc.FAMILIES, (), "default")


SOLVE_OPTIONS = {
    "solve_inverse": ((("solve_inverse", 1),), dict(solve_inverse=True)),
    "trsm_leaf": ((("trsm_leaf", 1),), dict(trsm_leaf=1)),
    "downdate_early": ((("downdate_early", 50),), {}),
    "solve_inverse+downdate_early": ((("solve_inverse", 1), ("downdate_early", 50)), dict(solve_inverse=True)),
}


@pytest.mark.parametrize("name", list(SOLVE_OPTIONS))
def test_options_that_change_the_arithmetic(hip, name):
    """(200, 64), all four families, each against the bound of ITS schedule:
    solve_inverse = 1     a block row's solve is one product with the explicit inverse of the 128- / 192-row diagonal factor
                          (invertFactor: k_tf_eye + the strip kernel's right solve); the bound carries the whole-block T
    trsm_leaf = 1         every solve of 256 columns or more splits down to 64-row leaves: one level at 128 rows, two at 192
    downdate_early = 50   the shares Y_k^T Y_k of block rows 0 and 1 are subtracted on the E-chain's stream as masked products of their own,
                          rows 2 and 3 in one product behind them: one addition per block row, which block_rows counts already
    Measured worst ratios (Sigma+ on a / b / c / e; gamma, delta and Gamma[0:6] as in the default run to two digits unless noted):
    solve_inverse 0.0059 / 0.00085 / 0.015 / 0.0059 (gamma c 0.13; on the graded family b the whole-block T widens the bound);
    trsm_leaf 0.0059 / 0.0056 / 0.027 / 0.0059; downdate_early 0.0059 / 0.0060 / 0.027 / 0.0059; both 0.0059 / 0.0011 / 0.015 / 0.0059."""
    options, sched = SOLVE_OPTIONS[name]
    N, bl = uc.TILED_BIG[0]
    held(hip, N, bl, uc.FAMILIES, options, name, **sched)


STREAM_OPTIONS = (("lookahead", 0), ("overlap_chains", 0), ("panel_ahead", 1), ("check_every", 0))


def test_options_that_only_move_work_between_streams(hip):
    """(200, 64), family a: Sigma+, gamma, Gamma and the bias bit for bit the default run's under each of
    lookahead = 0       the diagonal block is factored from X behind the trailing update instead of from a copy on the side stream: the same
                        product on the same elements (the copy takes the unmasked product, X the masked one, which keeps diagonal blocks)
    overlap_chains = 0  the E-chain is enqueued behind the downdate instead of next to the S-chain
    panel_ahead = 1     the rows of block k + 1 are updated by a launch of their own, in front of the rest: an entry of C still has one
                        writer and sums its k rows in the same order wherever its tile begins
    check_every = 0     the update does not read the pivot flag (the test does, afterwards)
    By the code none of them reorders arithmetic; every one is held to bit-equality.  Measured: all four bit-equal to the default run."""
    N, bl = uc.TILED_BIG[0]
    base = one_update(hip, N, bl, "a")
    again = one_update(hip, N, bl, "a")
    assert all(np.array_equal(base[k], again[k]) for k in KEYS), "the default run does not repeat itself bit for bit"
    differs = []
    for opt in STREAM_OPTIONS:
        out = one_update(hip, N, bl, "a", (opt,))
        differs += [(opt, k, float(np.abs(out[k] - base[k]).max())) for k in KEYS if not np.array_equal(out[k], base[k])]
    print(f"stream options at N = {N}, blocks of {bl}: {'all bit-equal to the default run' if not differs else differs}")
    assert not differs, differs
