"""The dense tile kernels of the partitioned filter (csrc/eqf_tile.hpp: k_tile_potrf, k_tile_potrf_trail, k_tile_trsm, k_tile_mirror,
k_tile_propagate) and, through them, the Cholesky building blocks every factorisation of the project shares (csrc/eqf_chol64.hpp: factor64,
potrf16v2, solveStrip, mmTile) on ragged sizes, padded views and ill-conditioned input, against the componentwise bounds of
tests/chol_bounds.py (derived there, residuals in longdouble); what the kernels do with a matrix that is not positive definite; and bit 4 of
eqf_device_error through the public calls.

Every padding cell around a view holds a FINITE sentinel: np.array_equal calls a NaN unequal to itself, so a NaN sentinel would fail "nothing
outside the view changed" although no write strayed.

Measured on an MI355X, worst ratio to the asserted bound (and to the same bound with T = I) over all families, sizes and widths below:
eqf_tile_potrf 0.19 (0.19) at n = 2 and 0.12 (0.14) from n = 15 on, 0.058 (0.060) on the scaled copies, bit for bit the same for 4^100 and
4^-100; records 0.15; eqf_tile_trsm left 0.073 (0.55, at n = 128), the split solve included; right 0.073 (0.21, at n = 17).  The kernels
stay inside the plain factorisation bound, unlike the model that sends every panel through an explicit inverse: inside a 64-block they
substitute.  The solves do need T: they are within a factor of two of the plain bound where a diagonal block is ill-conditioned."""
import ctypes

import numpy as np
import pytest

import chol_bounds as cb

pytestmark = pytest.mark.gpu

SENTINEL = -7.25  # finite, exactly representable, and nothing a kernel would compute


@pytest.fixture(scope="module")
def be():
    from eqf_vio_amd import tiled

    b = tiled.HipBackend({}, capacity=8)
    yield b
    b.close()


def _dev():
    import torch

    return torch.device("cuda", 0)


class _View:
    """An r x c matrix inside a larger device buffer of sentinels: offset rows and columns, leading dimension > c"""

    def __init__(self, A, top=3, left=5, bottom=2, right=4):
        import torch

        r, c = A.shape
        self.host = np.full((r + top + bottom, c + left + right), SENTINEL)
        self.host[top: top + r, left: left + c] = A
        self.inside = np.zeros(self.host.shape, dtype=bool)
        self.inside[top: top + r, left: left + c] = True
        self.dev = torch.from_numpy(self.host).to(_dev())
        self.view = self.dev[top: top + r, left: left + c]
        self.shape = (r, c)

    def fetch(self):
        """the view's content now; asserts that nothing outside it changed, bit for bit"""
        got = self.dev.cpu().numpy()
        assert np.array_equal(got[~self.inside], self.host[~self.inside]), "a write strayed outside the view"
        return got[self.inside].reshape(self.shape)


def _factor(be, A):
    """eqf_tile_potrf in place on a view of A -> (the view object, the view's content afterwards, the records, info)"""
    v = _View(A)
    drec = be.potrf(v.view)
    info = be.factor_info()
    return v, v.fetch(), drec, info


def _check_factor(A, got, label, Lref=None, T=None):
    """the strict upper triangle is the stale input, the lower one a factor inside the bound; returns (ratio, plain ratio)"""
    iu = np.triu_indices(len(A), 1)
    assert np.array_equal(got[iu], A[iu]), label
    aware, plain = cb.potrf_ratio(A, got, Lref, T)
    assert aware <= 1.0, (label, aware, plain)
    return aware, plain


# ---- accuracy -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cb.POTRF_SIZES)
def test_potrf_inside_the_factorisation_bound(be, n):
    """n = 1 .. 64: factor64 alone, with one to four real stages and a ragged last one; 65 .. 128: the single workgroup's own panel and
    trailing code, with a one-row second block at 65; 129 on: three launches per block column, a one-row last block at 129 and 193"""
    worst = (0.0, 0.0)
    for label, A in cb.family_cases(n):
        _, got, _, info = _factor(be, A)
        assert info == 0, label
        worst = tuple(max(w, r) for w, r in zip(worst, _check_factor(A, got, label)))
    print(f"potrf n={n}: worst ratio to bound {worst[0]:.3f}, to the plain bound {worst[1]:.3f}")


@pytest.mark.parametrize("e", [100, -100])
def test_potrf_of_scaled_copies(be, e):
    """4^e A is A with another exponent: the same bound holds if nothing in the pivot's scaling (scaleRsqrtPivot) depends on the magnitude"""
    for name, fn, pars in cb.FAMILIES:
        A = fn(100, pars[-1]) * 4.0 ** e
        _, got, _, info = _factor(be, A)
        assert info == 0, name
        print(f"potrf 4^{e} {name}: ratio to bound {_check_factor(A, got, name)}")


@pytest.mark.parametrize("n", [17, 64, 100, 193])
def test_records_hold_the_diagonal_block_and_its_inverses(be, n):
    """Per 64-wide block column: cells [0, 4096) are L_kk as stored in the matrix -- lower triangle, zeros above, identity past n --, cells
    [4096, 5120) the row-major inverses of its four 16 x 16 diagonal blocks (of the identity padding: the identity)"""
    worst = 0.0
    for label, A in cb.family_cases(n):
        _, got, drec, info = _factor(be, A)
        assert info == 0, label
        rec = drec.cpu().numpy().reshape(-1, be.DREC)
        assert len(rec) == (n + 63) // 64
        for kb in range(len(rec)):
            w = min(64, n - 64 * kb)
            want = np.eye(64)
            want[:w, :w] = np.tril(got[64 * kb: 64 * kb + w, 64 * kb: 64 * kb + w])
            Lkk = rec[kb, :4096].reshape(64, 64)
            assert np.array_equal(Lkk, want), (label, kb)
            for j in range(4):
                W = rec[kb, 4096 + 256 * j: 4096 + 256 * (j + 1)].reshape(16, 16)
                r = cb.record_ratio(W, Lkk[16 * j: 16 * j + 16, 16 * j: 16 * j + 16])
                assert r <= 1.0, (label, kb, j, r)
                worst = max(worst, r)
    print(f"records n={n}: worst ratio to bound {worst:.3f}")


def _solve_cases(be, n):
    """[(label, A, factor on the device (view), the same on the host, records, T)] over all families and parameters at size n"""
    out = []
    for label, A in cb.family_cases(n):
        v, got, drec, info = _factor(be, A)
        assert info == 0, label
        Lh = np.tril(got)
        out.append((label, A, v, Lh, drec, cb.block_T(Lh)))
    return out


@pytest.mark.parametrize("n", [17, 65, 128, 193, 384])
def test_trsm_left_inside_the_solve_bound(be, n):
    """B <- L^-1 B with the device's own factor and records, B's rows scaled like the factor's; m = 300 at n = 384 is split by trsm_left
    (two short chains and one product), and the same case through one launch must meet the bound as well"""
    worst = (0.0, 0.0)
    for label, A, v, Lh, drec, T in _solve_cases(be, n):
        for m in (1, 63, 64, 65, 300):
            B = np.random.default_rng([6, n, m]).standard_normal((n, m)) * np.sqrt(np.diag(A))[:, None]
            split = (n + 63) // 64 >= be.TRSM_SPLIT and m >= 256
            assert split == (n == 384 and m == 300)
            for solve in (be.trsm_left,) + ((be._trsm_launch,) if split else ()):
                bv = _View(B, 2, 4, 3, 1)
                solve(v.view, drec, bv.view)
                r = cb.trsm_left_ratio(Lh, bv.fetch(), B, T)
                assert r[0] <= 1.0, (label, m, solve.__name__, r)
                worst = tuple(max(a, b) for a, b in zip(worst, r))
    print(f"trsm left n={n}: worst ratio to bound {worst[0]:.3f}, to the plain bound {worst[1]:.3f}")


@pytest.mark.parametrize("n", [17, 64, 65, 193])
def test_trsm_right_inside_the_solve_bound(be, n):
    """B <- B L^-T on an m x n view: from n = 65 on the strip's later blocks first take X_kb -= X_j L_kb,j^T, which the blocked potrf
    (n <= 64 per call) never reaches"""
    worst = (0.0, 0.0)
    for label, A, v, Lh, drec, T in _solve_cases(be, n):
        for m in (1, 64, 70, 130):
            B = np.random.default_rng([7, n, m]).standard_normal((m, n)) * np.sqrt(np.diag(A))[None, :]
            bv = _View(B, 1, 3, 2, 6)
            be.trsm_right(v.view, drec, bv.view)
            r = cb.trsm_right_ratio(Lh, bv.fetch(), B, T)
            assert r[0] <= 1.0, (label, m, r)
            worst = tuple(max(a, b) for a, b in zip(worst, r))
    print(f"trsm right n={n}: worst ratio to bound {worst[0]:.3f}, to the plain bound {worst[1]:.3f}")


# ---- failure detection --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16, 40, 64, 100, 128, 200])
def test_a_matrix_that_is_not_positive_definite_raises_the_flag(be, n):
    """The kernels test ONE entry per 16-column stage and rely on NaN / inf travelling there from the bad pivot: a negative, a zero and a
    NaN pivot in the first, a middle and the last lane of a stage, in the ragged last stage, in every 64-block, and an indefinite matrix
    with a spotless diagonal.  The flag is per call: a clean matrix afterwards factors inside its bound with the flag down."""
    A0 = cb.spd_base(n)
    L0 = np.linalg.cholesky(A0)
    T0 = cb.block_T(L0)
    for label, A in cb.bad_inputs(n):
        _, _, _, info = _factor(be, A)  # (asserts that nothing outside the view was written)
        assert info == 1, label
        _, got, _, info = _factor(be, A0)
        assert info == 0, label
        _check_factor(A0, got, label, L0, T0)
    for label, A in cb.control_inputs(n):  # as close to singular as fp64 factors: no false alarm
        _, got, _, info = _factor(be, A)
        assert info == 0, label
        _check_factor(A, got, label)


def _frames(fg, st, first, count):
    """events of `st` from index `first` on until `count` more vision frames are through; returns the index behind the last one"""
    ev = list(st.events())
    done = 0
    for at in range(first, len(ev)):
        kind, k = ev[at]
        if kind == "imu":
            r = st.imu[k]
            fg.process_imu([r[0]], r[1:4], r[4:7])
        else:
            fg.process_vision([st.vision_stamps[k]], st.ids, st.bearings[k])
            done += 1
            if done == count:
                return at + 1
    raise AssertionError("the stream is too short")


@pytest.mark.parametrize("landmark", [7, 50])
@pytest.mark.parametrize("resident", ["default", "0"])
def test_bit_4_of_the_device_error_through_the_public_calls(monkeypatch, resident, landmark):
    """One landmark's block of Sigma made negative definite, one vision update: S (2 N = 140 rows, three 64-blocks) gets its bad pivots at
    rows 2 lm, 2 lm + 1 -- landmark 7 in the first block, landmark 50 in the second.  Bit 4, and not the hand-off timeout (bit 128); the
    call returns; after eqf_reset the handle cannot be told from a new one."""
    from eqf_vio_amd import binding, synth

    if resident == "default":
        monkeypatch.delenv("EQF_CHOL_RESIDENT", raising=False)
    else:
        monkeypatch.setenv("EQF_CHOL_RESIDENT", resident)
    N = 70
    d = synth.template_settings_dict()
    st = synth.make_stream(N, duration=0.4)
    fg = binding.FilterBatch(d, capacity=N, batch=1)
    at = _frames(fg, st, 0, 2)
    assert fg.device_error() == 0
    S = fg.sigma()
    blk = slice(11 + 3 * landmark, 14 + 3 * landmark)
    S[blk, blk] = -1e3 * np.eye(3)
    fg.set_sigma(S)
    try:
        _frames(fg, st, at, 1)
    except binding.EqfError as e:
        assert e.code == -6, e  # EQF_ERR_NUMERIC from the call that found the flag, and no other error: it returned, which is all that is asked
    err = fg.device_error()
    assert err & 4 and not err & 128, err
    fg.reset()
    fresh = binding.FilterBatch(d, capacity=N, batch=1)
    for h in (fg, fresh):
        _frames(h, st, 0, 3)
        assert h.device_error() == 0
    assert np.array_equal(fg.sigma(), fresh.sigma())
    fg.close()
    fresh.close()


# ---- smaller pieces -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,rb", [(1, 1), (63, 7), (64, 64), (65, 64), (130, 50), (193, 1), (200, 300), (384, 96)])
def test_mirror_is_exact_and_stays_below_the_block_diagonal(be, n, rb):
    """every element below the block diagonal (blocks of rb) <- its mirror image, as tests/tiled_double.py defines it; everything else --
    on and above the block diagonal, outside the view -- keeps its bits; one block (rb >= n) changes nothing"""
    C = np.random.default_rng([8, n, rb]).standard_normal((n, n))
    v = _View(C)
    be.mirror_lower(v.view, rb)
    blk = np.arange(n) // rb
    low = blk[:, None] > blk[None, :]
    got = v.fetch()
    assert np.array_equal(got, np.where(low, C.T, C))
    assert np.array_equal(got[~low], C[~low])
    if rb >= n:
        assert np.array_equal(got, C)


@pytest.mark.parametrize("nI,nJ", [(1, 1), (15, 17), (16, 16), (17, 33)])
def test_propagate_on_ragged_tiles_against_longdouble(nI, nJ):
    """One Riccati step of a tile with fewer, exactly and more landmarks than a workgroup's 16 x 16, on padded buffers, against the dense
    formula in longdouble: the off-diagonal tile (rows I, columns J) and the diagonal tiles (I, I) and (J, J), which get the process noise
    and must come out symmetric"""
    import torch

    from eqf_vio_amd import binding

    lib = binding.lib()
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    rng = np.random.default_rng([9, nI, nJ])
    N = nI + nJ
    n = 11 + 3 * N
    M = rng.standard_normal((n, n))
    S = M @ M.T + n * np.eye(n)
    F = np.eye(n)
    F[:11, :11] += 0.01 * rng.standard_normal((11, 11))
    F[11:, :11] = 0.02 * rng.standard_normal((3 * N, 11))
    D = np.stack([np.eye(3) + 0.01 * rng.standard_normal((3, 3)) for _ in range(N)])
    for i in range(N):
        F[11 + 3 * i: 14 + 3 * i, 11 + 3 * i: 14 + 3 * i] = D[i]
    Bn = np.zeros((n, 6))
    Bn[6:] = rng.standard_normal((n - 6, 6))
    R6 = np.array([1e-4, 1e-4, 1e-4, 2e-4, 2e-4, 2e-4])
    T, pv = 0.005, 0.001
    P = np.concatenate([np.full(11, 0.01), np.full(3 * N, pv)])
    ld_ = lambda a: np.asarray(a, dtype=np.longdouble)
    ref = (ld_(F) @ ld_(S) @ ld_(F).T + ld_(T) * (np.diag(ld_(P)) + (ld_(Bn) * ld_(R6)) @ ld_(Bn).T)).astype(np.float64)
    Dd, Ld, Bd, Sbb = t(D), t(F[11:, :11]), t(Bn), t(S[:11, :11])
    panel = np.full((11, 3 * N + 5), SENTINEL)  # the base panel with a leading dimension larger than any tile needs
    panel[:, : 3 * N] = S[:11, 11:]
    Sb = t(panel)
    r6 = (ctypes.c_double * 6)(*R6)
    for (i0, ni, j0, nj) in {(0, nI, nI, nJ), (0, nI, 0, nI), (nI, nJ, nI, nJ)}:
        rows, cols = slice(11 + 3 * i0, 11 + 3 * (i0 + ni)), slice(11 + 3 * j0, 11 + 3 * (j0 + nj))
        tin, tout = _View(S[rows, cols]), _View(np.full((3 * ni, 3 * nj), SENTINEL))
        assert tin.view.stride(0) == tout.view.stride(0) > 3 * nj
        diag = int(i0 == j0 and ni == nj)
        rc = lib.eqf_tile_propagate(0, None, p(tout.view), p(tin.view), tin.view.stride(0), ni, nj, p(Dd[i0:]), p(Ld[3 * i0:]), p(Dd[j0:]),
                                    p(Ld[3 * j0:]), p(Sbb), p(Sb[:, 3 * i0:]), Sb.stride(0), p(Sb[:, 3 * j0:]), Sb.stride(0), p(Bd[11 + 3 * i0:]),
                                    p(Bd[11 + 3 * j0:]), ctypes.cast(r6, ctypes.POINTER(ctypes.c_double)), T, T * pv, diag)
        assert rc == 0
        torch.cuda.synchronize()
        want, got = ref[rows, cols], tout.fetch()
        assert np.array_equal(tin.fetch(), S[rows, cols])  # (the input tile is only read)
        tol = 1e-12 * np.abs(want).max()
        assert np.abs(got - want).max() <= tol, (i0, j0)
        if diag:
            assert np.abs(got - got.T).max() <= tol, (i0, j0)
