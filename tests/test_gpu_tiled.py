"""BASELINE configs[4] on the MI355X: the 2-D block-partitioned filter (eqf_vio_amd/tiled.py + csrc/eqf_tiled.hpp / eqf_tile.hpp) on a
1 x 1 process grid -- CLOSED LOOP, nothing of the oracle inside the loop: processIMUData / processVisionData run the replicated state,
the base panel, the local blocks and the two distributed factorisations through the C ABI; the oracle and the single-GPU product path
are the checkers.  Plus the dense tile kernels against numpy.  (The multi-rank exchange schedule is validated on CPU with gloo,
tests/test_tiled.py.)"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _t(dev):
    import torch

    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def test_tile_downdate_on_the_integer_pipe_against_numpy():
    """C -= A^T B from 7-bit slices of the operands' columns on v_mfma_i32_32x32x32_i8 with exact int32 accumulation (round 6,
    eqf_tile_downdate_i8): against numpy within k (ca_i cb_j) 2^-(5 + 7 (S - 1)), ca / cb the columns' largest entries.  That bound is
    STATISTICAL, not what the construction guarantees: the rounding to slices (up to 2 x 2^-7S per term) and the dropped slice pairs
    ta + tb >= S (up to (S - 1) x 2^-7S) exceed it on inputs whose errors share a sign (tests/test_i8_emulator.py); random data stay inside.
    The bit-exact check against the kernels' model is tests/test_gpu_i8_exact.py.  On ragged sizes around the 128 x 64 x 32 tiling, views with leading dimensions, columns of very different scales, an
    all-zero column, the same matrix on both sides, and the block-upper mask."""
    import torch

    from eqf_vio_amd import tiled

    dev = torch.device("cuda", 0)
    be = tiled.HipBackend({}, capacity=8)
    t = _t(dev)
    rng = np.random.default_rng(5)
    for (m, n, k, S) in ((128, 64, 32, 5), (75, 130, 50, 5), (200, 96, 448, 6), (257, 513, 129, 7), (300, 300, 1000, 5)):
        A = rng.standard_normal((k, m + 5)) * 10.0 ** rng.uniform(-3, 3, size=(1, m + 5))
        B = rng.standard_normal((k, n + 3)) * 10.0 ** rng.uniform(-3, 3, size=(1, n + 3))
        A[:, 4] = 0.0
        C = rng.standard_normal((m, n + 7))
        Ad, Bd, Cd = t(A), t(B), t(C)
        be.downdate_i8(Cd[:, 2: 2 + n], Ad[:, 1: 1 + m], Bd[:, 3: 3 + n], S)
        Av, Bv = A[:, 1: 1 + m], B[:, 3: 3 + n]
        want = C.copy()
        want[:, 2: 2 + n] -= Av.T @ Bv
        bound = k * np.outer(np.abs(Av).max(axis=0), np.abs(Bv).max(axis=0)) * 2.0 ** -(5 + 7 * (S - 1)) * 1.01 + 1e-12 * np.abs(want[:, 2: 2 + n])
        got = Cd.cpu().numpy()
        assert np.array_equal(got[:, :2], C[:, :2]) and np.array_equal(got[:, 2 + n:], C[:, 2 + n:])  # nothing outside the view
        assert (np.abs(got[:, 2: 2 + n] - want[:, 2: 2 + n]) <= bound).all(), (m, n, k, S)
    # the same matrix on both sides + the block-upper mask of a symmetric local matrix (blocks of 96): on and above the block diagonal as
    # above, below it whatever the tiles that were not skipped left -- eqf_tile_mirror overwrites it
    n, k, rb, S = 384, 200, 96, 5
    Y = rng.standard_normal((k, n))
    C = rng.standard_normal((n, n))
    C = C + C.T
    Yd, Cd = t(Y), t(C)
    be.downdate_i8(Cd, Yd, Yd, S, mask_rb=rb)
    be.mirror_lower(Cd, rb)
    torch.cuda.synchronize()
    want = C - Y.T @ Y
    bound = k * np.outer(np.abs(Y).max(axis=0), np.abs(Y).max(axis=0)) * 2.0 ** -(5 + 7 * (S - 1)) * 1.01
    got = Cd.cpu().numpy()
    assert (np.abs(got - want) <= bound + 1e-12).all()
    assert np.array_equal(np.tril(got, -rb), np.tril(got.T, -rb))  # (strictly below the block diagonal: exact mirror images)


def test_tile_gemm_tn_on_the_integer_pipe_behind_the_block_mask():
    """eqf_tile_gemm_tn_i8 (round 6, what "chain_slices" runs for a block row's trailing products): C -= A^T B from slices, behind
    eqf_tile_gemm_tn's block mask over the first mask_cols columns (the matrix part) with the columns behind them (right-hand sides) always
    formed; A as a column range of B (cut once: offsets that are a multiple of 32) and as a matrix of its own; the same statistical error
    bound as the downdate's product (see there; bit for bit: tests/test_gpu_i8_exact.py).  Below the staircase an element is untouched or the whole product, never garbage."""
    import torch

    from eqf_vio_amd import tiled

    dev = torch.device("cuda", 0)
    be = tiled.HipBackend({}, capacity=8)
    t = _t(dev)
    rng = np.random.default_rng(11)
    #        m    n (incl. rhs)  k   rb  rblk0 Pr pr cblk0 Pc pc  mask_cols  A's offset in B (None: separate)  slices
    cases = ((600, 600 + 37, 150, 150, 0, 1, 0, 0, 1, 0, 600, 0, 5),
             (450, 600 + 18, 150, 150, 1, 1, 0, 0, 1, 0, 600, None, 5),     # (rows start one block further down than the columns)
             (512, 640 + 5, 128, 128, 0, 1, 0, 0, 1, 0, 640, 128, 6),       # (A = B's columns 128 .. 640: an aligned offset, cut once)
             (500, 500 + 9, 96, 100, 2, 2, 1, 1, 2, 0, 500, None, 5),       # (a 2 x 2 grid's rank (1, 0) with block offsets)
             (300, 77, 64, 0, 0, 1, 0, 0, 1, 0, 0, None, 7),                # (no mask: right-hand sides only)
             (260, 300, 40, 100, 0, 1, 0, 0, 1, 0, 300, 20, 5))             # (an offset that is NOT a multiple of 32: cut separately)
    for (m, n, k, rb, rblk0, Pr, pr, cblk0, Pc, pc, mcols, aoff, S) in cases:
        B = rng.standard_normal((k, n + 3)) * 10.0 ** rng.uniform(-2, 2, size=(1, n + 3))
        Bd = t(B)
        Bv, Bdv = B[:, 1: 1 + n], Bd[:, 1: 1 + n]
        if aoff is None:
            A = rng.standard_normal((k, m)) * 10.0 ** rng.uniform(-2, 2, size=(1, m))
            Adv = t(A)
        else:
            A, Adv = Bv[:, aoff: aoff + m], Bdv[:, aoff: aoff + m]
        C = rng.standard_normal((m, n + 4))
        Cd = t(C)
        mask = (rb, rb, rblk0, Pr, pr, cblk0, Pc, pc) if rb else None
        be.gemm_tn_i8(Cd[:, 2: 2 + n], Adv, Bdv, S, mask=mask, mask_cols=mcols)
        got = Cd.cpu().numpy()
        assert np.array_equal(got[:, :2], C[:, :2]) and np.array_equal(got[:, 2 + n:], C[:, 2 + n:])
        got, C0 = got[:, 2: 2 + n], C[:, 2: 2 + n]
        want = C0 - A.T @ Bv
        bound = k * np.outer(np.abs(A).max(axis=0), np.abs(Bv).max(axis=0)) * 2.0 ** -(5 + 7 * (S - 1)) * 1.01 + 1e-12 * np.abs(want)
        keep = np.ones((m, n), dtype=bool)
        if rb:
            I = (rblk0 + np.arange(m) // rb) * Pr + pr
            J = (cblk0 + np.arange(n) // rb) * Pc + pc
            keep = I[:, None] <= J[None, :]
            keep[:, mcols:] = True
        assert (np.abs(got - want) <= bound)[keep].all(), (m, n, k, S)
        assert ((got == C0) | (np.abs(got - want) <= bound))[~keep].all(), (m, n, k, S)
        if rb and m >= 384:
            assert (got == C0)[~keep].any()  # (whole tiles below the staircase really are skipped)


def test_tile_gemm_tn_against_numpy():
    """C += alpha A^T B (eqf_tile_gemm_tn): ragged sizes around the 128 x 128 x 16 tiling, narrow products, views with leading
    dimensions, both signs, and the block-upper mask of a block-cyclic local matrix."""
    import torch

    from eqf_vio_amd import tiled

    dev = torch.device("cuda", 0)
    be = tiled.HipBackend({}, capacity=8)
    t = _t(dev)
    rng = np.random.default_rng(3)
    for (m, n, k, alpha) in ((128, 128, 16, -1.0), (75, 130, 50, -1.0), (12, 12, 7, 1.0), (200, 96, 448, -1.0), (18, 777, 100, 1.0),
                             (300, 18, 33, 1.0), (257, 513, 129, -1.0)):
        A, B, C = rng.standard_normal((k, m + 5)), rng.standard_normal((k, n + 3)), rng.standard_normal((m, n + 7))
        Ad, Bd, Cd = t(A), t(B), t(C)
        be.gemm_tn(Cd[:, 2: 2 + n], Ad[:, 1: 1 + m], Bd[:, 3: 3 + n], alpha)
        want = C.copy()
        want[:, 2: 2 + n] += alpha * A[:, 1: 1 + m].T @ B[:, 3: 3 + n]
        assert np.abs(Cd.cpu().numpy() - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (m, n, k)
    # downdate entry point (alpha = -1)
    A, B, C = rng.standard_normal((40, 70)), rng.standard_normal((40, 90)), rng.standard_normal((70, 90))
    Cd = t(C)
    assert be.lib.eqf_tile_downdate(0, None, be._p(Cd), 90, 70, 90, be._p(t(A)), 70, be._p(t(B)), 90, 40) == 0
    torch.cuda.synchronize()
    assert np.abs(Cd.cpu().numpy() - (C - A.T @ B)).max() <= 1e-12 * 100
    # mask: local matrix of process (pr, pc) = (1, 0) on a 2 x 2 grid, blocks of 100: rows are global blocks 1, 3, 5, columns 0, 2, 4;
    # everything on or above the block diagonal must be exact, tiles strictly below may be skipped
    rb, nbl = 100, 3
    m = n = rb * nbl
    k = 64
    A, B, C = rng.standard_normal((k, m)), rng.standard_normal((k, n)), rng.standard_normal((m, n))
    Cd = t(C)
    be.gemm_tn(Cd, t(A), t(B), -1.0, mask=(rb, rb, 0, 2, 1, 0, 2, 0))
    got, want = Cd.cpu().numpy(), C - A.T @ B
    skipped = 0
    for ib in range(nbl):
        for jb in range(nbl):
            I, J = ib * 2 + 1, jb * 2
            blk = (slice(ib * rb, (ib + 1) * rb), slice(jb * rb, (jb + 1) * rb))
            if I <= J:
                assert np.abs(got[blk] - want[blk]).max() <= 1e-12 * 100, (I, J)
            else:
                skipped += int(np.array_equal(got[blk], C[blk]))
    assert skipped >= 1  # (whole tiles below the diagonal really are skipped)
    # masked launches walk only the active tiles (GemmPlan): staircases of several shapes -- blocks that are no multiple of the 128-wide tile,
    # ragged last blocks, a non-square process grid with offsets into the local matrix, a mask that leaves nothing
    for (m, n, k, rb, cb, rblk0, Pr, pr, cblk0, Pc, pc) in ((1500, 1500, 40, 750, 750, 0, 1, 0, 0, 1, 0), (1000, 1380, 33, 300, 300, 0, 1, 0, 0, 1, 0),
                                                            (900, 700, 20, 150, 100, 1, 2, 1, 2, 4, 3), (640, 512, 16, 128, 128, 0, 2, 0, 0, 2, 1),
                                                            (300, 260, 8, 100, 100, 2, 1, 0, 0, 1, 0)):
        A, B, C = rng.standard_normal((k, m)), rng.standard_normal((k, n)), rng.standard_normal((m, n))
        Cd = t(C)
        be.gemm_tn(Cd, t(A), t(B), -1.0, mask=(rb, cb, rblk0, Pr, pr, cblk0, Pc, pc))
        got, want = Cd.cpu().numpy(), C - A.T @ B
        I = (rblk0 + np.arange(m) // rb) * Pr + pr
        J = (cblk0 + np.arange(n) // cb) * Pc + pc
        keep = I[:, None] <= J[None, :]
        assert np.abs(got - want)[keep].max(initial=0.0) <= 1e-12 * 100, (m, n, rb, cb)
        # below the staircase an element is either untouched or the full product (tiles are skipped or computed whole), never garbage
        low = ~keep
        assert (np.isclose(got, C, rtol=0, atol=0) | (np.abs(got - want) <= 1e-10))[low].all(), (m, n, rb, cb)


def test_tile_propagate_against_dense_formula():
    import torch

    from eqf_vio_amd import binding

    dev = torch.device("cuda", 0)
    t = _t(dev)
    lib = binding.lib()
    import ctypes

    p = lambda x: ctypes.c_void_p(x.data_ptr())
    rng = np.random.default_rng(3)
    N = 45
    n = 11 + 3 * N
    M = rng.standard_normal((n, n))
    S = M @ M.T + n * np.eye(n)
    F = np.eye(n)
    F[:11, :11] += 0.01 * rng.standard_normal((11, 11))
    F[11:, :11] = 0.02 * rng.standard_normal((3 * N, 11))
    D = np.stack([np.eye(3) + 0.01 * rng.standard_normal((3, 3)) for _ in range(N)])
    for i in range(N):
        F[11 + 3 * i:14 + 3 * i, 11 + 3 * i:14 + 3 * i] = D[i]
    Bn = np.zeros((n, 6))
    Bn[6:] = rng.standard_normal((n - 6, 6))
    R6 = np.array([1e-4, 1e-4, 1e-4, 2e-4, 2e-4, 2e-4])
    T, pv = 0.005, 0.001
    P = np.concatenate([np.full(11, 0.01), np.full(3 * N, pv)])
    ref = F @ S @ F.T + T * (np.diag(P) + (Bn * R6) @ Bn.T)
    Sd, Dd, Ld, Bd = t(S), t(D), t(F[11:, :11]), t(Bn)
    Sbb, Sb = Sd[:11, :11].contiguous(), Sd[:11, 11:].contiguous()
    r6 = (ctypes.c_double * 6)(*R6)
    for (i0, ni, j0, nj) in ((0, 20, 20, 25), (20, 25, 20, 25), (25, 20, 0, 25)):
        tile = Sd[11 + 3 * i0:11 + 3 * (i0 + ni), 11 + 3 * j0:11 + 3 * (j0 + nj)].contiguous()
        out = torch.empty_like(tile)
        rc = lib.eqf_tile_propagate(0, None, p(out), p(tile), tile.stride(0), ni, nj, p(Dd[i0:]), p(Ld[3 * i0:]), p(Dd[j0:]), p(Ld[3 * j0:]), p(Sbb),
                                    p(Sb[:, 3 * i0:]), Sb.stride(0), p(Sb[:, 3 * j0:]), Sb.stride(0), p(Bd[11 + 3 * i0:]), p(Bd[11 + 3 * j0:]),
                                    ctypes.cast(r6, ctypes.POINTER(ctypes.c_double)), T, T * pv, int(i0 == j0 and ni == nj))
        assert rc == 0
        want = ref[11 + 3 * i0:11 + 3 * (i0 + ni), 11 + 3 * j0:11 + 3 * (j0 + nj)]
        assert np.abs(out.cpu().numpy() - want).max() <= 1e-12 * np.abs(want).max(), (i0, j0)


@pytest.mark.parametrize("n", [16, 64, 96, 200, 384, 500, 750])
def test_tile_potrf_and_trsm_against_lapack(n):
    """eqf_tile_potrf / eqf_tile_trsm (the diagonal block and the block-row solve of the distributed factorisation) against numpy, in place
    on views with a leading dimension: block sizes below, at and between multiples of the 64-wide block column, up to the 2 bl = 500 and
    3 bl = 750 of the N = 4000 configuration."""
    import torch

    from eqf_vio_amd import tiled

    dev = torch.device("cuda", 0)
    be = tiled.HipBackend({}, capacity=8)
    t = _t(dev)
    rng = np.random.default_rng(100 + n)
    M = rng.standard_normal((n, n))
    A = M @ M.T + n * np.eye(n)
    big = t(np.pad(A, ((3, 2), (5, 4))))
    Ad = big[3: 3 + n, 5: 5 + n]
    drec = be.potrf(Ad)
    assert be.factor_info() == 0
    Lref = np.linalg.cholesky(A)
    Lg = np.tril(Ad.cpu().numpy())
    assert np.abs(Lg - Lref).max() <= 1e-12 * np.abs(Lref).max()
    L = Ad.clone()
    for m in (1, 64, 70, 150):
        B2 = rng.standard_normal((n, m + 6))
        Bd = t(B2)
        be.trsm_left(L, drec, Bd[:, 4: 4 + m])  # L^-1 B on a view
        want = B2.copy()
        want[:, 4: 4 + m] = np.linalg.solve(Lref, B2[:, 4: 4 + m])
        assert np.abs(Bd.cpu().numpy() - want).max() <= 1e-11 * max(1.0, np.abs(want).max()), (n, m)
    Abad = A.copy()
    Abad[n // 2, n // 2] = -1.0
    be.potrf(t(Abad))
    assert be.factor_info() == 1  # a matrix that is not positive definite raises the flag instead of producing NaNs silently


def _drive(tf, fo, fg, st, frames_checked, tolS):
    """Same stream into the tiled filter `tf`, the oracle `fo` and (optionally) the single-GPU product path `fg`; after every vision
    call: Sigma, pose, landmarks, bias against the oracle (and the product path)."""
    rel = lambda A, B: float(np.linalg.norm(A - B) / np.linalg.norm(B))
    worst = {"S_oracle": 0.0, "S_product": 0.0, "pose": 0.0}
    n_upd = 0
    for kind, k in st.events():
        if kind == "imu":
            r = st.imu[k]
            tf.processIMUData(r[0], r[1:4], r[4:7])
            if fo is not None:
                fo.processIMUData(r[0], r[1:4], r[4:7])
            if fg is not None:
                fg.process_imu([r[0]], r[1:4], r[4:7])
        else:
            stamp = st.vision_stamps[k]
            assert tf.processVisionData(stamp, st.ids, st.bearings[k]) == 0
            if fo is not None:
                fo.processVisionData(stamp, st.ids, st.bearings[k])
            if fg is not None:
                fg.process_vision([stamp], st.ids, st.bearings[k])
            n_upd += 1
            if n_upd > frames_checked:
                continue
            St = tf.stateCovariance()
            et = tf.stateEstimate()
            assert np.abs(St - St.T).max() <= 1e-9 * np.abs(St).max()
            if fo is not None:
                worst["S_oracle"] = max(worst["S_oracle"], rel(St, fo.stateCovariance()))
                eo = fo.stateEstimate()
                worst["pose"] = max(worst["pose"], float(np.abs(eo["x"] - et["x"]).max()), float(np.abs(eo["q"] - et["q"]).max()),
                                    float(np.abs(eo["p"] - et["p"]).max()), float(np.abs(fo.bias() - tf.be.bias()).max()))
            if fg is not None:
                worst["S_product"] = max(worst["S_product"], rel(St, fg.sigma()))
                eg = fg.state_estimate()
                worst["pose"] = max(worst["pose"], float(np.abs(eg["x"] - et["x"]).max()), float(np.abs(eg["q"] - et["q"]).max()))
    assert tf.be.device_error() == 0
    assert worst["S_oracle"] <= tolS and worst["S_product"] <= tolS and worst["pose"] <= 1e-8, worst
    return worst, n_upd


@pytest.mark.parametrize("N,bl", [(48, 16), (50, 16), (37, 8), (200, 64)])
def test_tiled_filter_closed_loop_small(oracle_lib, N, bl):
    """1 x 1 grid, whole blocks and a ragged last block: first frame (landmarks appended), IMU steps, updates -- against the dense oracle
    and the single-GPU product path after every frame.  Also delta / gamma / Gamma of the last update against the oracle's."""
    from eqf_vio_amd import binding, synth, tiled

    d = synth.template_settings_dict()
    st = synth.make_stream(N, duration=0.26)
    be = tiled.HipBackend(d, capacity=N)
    tf = tiled.TiledFilter(tiled.ProcessGrid(None, 1, 1, device=be.device), be, bl)
    fo = oracle_lib.OracleFilter(d)
    fg = binding.FilterBatch(d, capacity=N, batch=1)
    worst, n_upd = _drive(tf, fo, fg, st, 99, 1e-9)
    assert n_upd >= 5
    lt, lo = be.last_update(), fo.last_update()
    for key, tol in (("delta", 1e-10), ("gamma", 1e-8), ("Gamma", 1e-8)):
        assert np.abs(lt[key] - lo[key]).max() <= tol * max(1.0, np.abs(lo[key]).max()), key


def test_tiled_filter_restart_from_a_single_gpu_snapshot(oracle_lib):
    """initialise_from(FilterBatch.dump_state()): the tiled filter continues a stream the product path started, and stays with it."""
    from eqf_vio_amd import binding, synth, tiled

    N, bl = 64, 16
    d = synth.template_settings_dict()
    st = synth.make_stream(N, duration=0.36)
    fg = binding.FilterBatch(d, capacity=N, batch=1)
    ev = list(st.events())
    cut = next(i for i, (kind, k) in enumerate(ev) if kind == "vision" and k == 2) + 4
    for kind, k in ev[:cut]:
        if kind == "imu":
            r = st.imu[k]
            fg.process_imu([r[0]], r[1:4], r[4:7])
        else:
            fg.process_vision([st.vision_stamps[k]], st.ids, st.bearings[k])
    be = tiled.HipBackend(d, capacity=N)
    tf = tiled.TiledFilter(tiled.ProcessGrid(None, 1, 1, device=be.device), be, bl)
    tf.initialise_from(fg.dump_state())
    S0, Sg0 = tf.stateCovariance(), fg.sigma()
    # bitwise the same rows and blocks; the tiled filter keeps only the base ROWS (the single-GPU path's base columns are its rows'
    # transpose up to rounding when its fused tile kernel wrote them)
    assert np.array_equal(S0[:11], Sg0[:11]) and np.array_equal(S0[11:, 11:], Sg0[11:, 11:])
    assert np.abs(S0 - Sg0).max() <= 1e-12 * np.abs(Sg0).max()
    rel = lambda A, B: float(np.linalg.norm(A - B) / np.linalg.norm(B))
    for kind, k in ev[cut:]:
        if kind == "imu":
            r = st.imu[k]
            fg.process_imu([r[0]], r[1:4], r[4:7])
            tf.processIMUData(r[0], r[1:4], r[4:7])
        else:
            fg.process_vision([st.vision_stamps[k]], st.ids, st.bearings[k])
            assert tf.processVisionData(st.vision_stamps[k], st.ids, st.bearings[k]) == 0
            assert rel(tf.stateCovariance(), fg.sigma()) <= 1e-9
    e1, e2 = tf.stateEstimate(), fg.state_estimate()
    assert np.abs(e1["x"] - e2["x"]).max() <= 1e-9 and np.abs(e1["q"] - e2["q"]).max() <= 1e-9 and be.device_error() == 0


def test_tiled_filter_N1000_against_the_structured_oracle(oracle_lib):
    """BASELINE cfg 3's size on the partitioned path: N = 1000, blocks of 125 (8 x 8 blocks), three updates against the structured fp64
    oracle (pinned to the dense one by tests/test_oracle_structured.py)."""
    from eqf_vio_amd import synth, tiled

    N, bl = 1000, 125
    d = synth.template_settings_dict()
    st = synth.make_stream(N, duration=0.16)
    be = tiled.HipBackend(d, capacity=N)
    tf = tiled.TiledFilter(tiled.ProcessGrid(None, 1, 1, device=be.device), be, bl)
    fo = oracle_lib.OracleFilter(d, structured=True)
    worst, n_upd = _drive(tf, fo, None, st, 99, 1e-7)
    assert n_upd >= 3 and worst["S_oracle"] <= 1e-8, worst


@pytest.mark.parametrize("N,bl,dur,slices,tol", [(200, 64, 2.0, 6, 1e-5), (200, 64, 1.0, 7, 1e-7), (1000, 125, 0.26, 6, 5e-5)])
def test_downdate_on_the_integer_pipe_holds_the_tolerance(N, bl, dur, slices, tol):
    """Round 6, north_star's "low-precision MFMA for the dense Sigma contractions, Sigma within 1e-4": the partitioned filter with its covariance
    downdate on the integer matrix pipe (eqf_tf_set_option "downdate_slices": Y's columns cut into 7-bit slices, int8 MFMA, exact accumulation,
    fp64 recombination) against the fp64 single-GPU product path on the bench stream, Sigma after EVERY update: SIX slices (21 integer products)
    stay inside north_star's 1e-4 with a margin -- measured 2.2e-6 at N = 200, 1.5e-5 at N = 1000, 5.8e-5 at N = 4000, the worst frame being
    the fifth, while the landmarks converge -- seven slices at 1e-8, FIVE do not (1.4e-4 / 9e-4: the slice pairs the kernel drops, ta + tb >= S,
    are of the truncation's size but add up coherently over Y's correlated columns; scripts/slice_precision_study.py reproduces all three
    figures on the CPU to three digits, profiles/r06_slice_precision_study_2s_with_pairs.txt).  Pose to 1e-6; the error flag stays clear and
    Sigma symmetric.  (The default, 0 slices, is the fp64 downdate every other test of this file runs.)"""
    from eqf_vio_amd import binding, synth, tiled

    d = synth.template_settings_dict()
    st = synth.make_stream(N, duration=dur)
    be = tiled.HipBackend(d, capacity=N)
    tf = tiled.TiledFilter(tiled.ProcessGrid(None, 1, 1, device=be.device), be, bl)
    tf.downdate_slices = slices
    fg = binding.FilterBatch(d, capacity=N, batch=1)
    worst, n_upd = 0.0, 0
    for kind, k in st.events():
        if kind == "imu":
            r = st.imu[k]
            tf.processIMUData(r[0], r[1:4], r[4:7])
            fg.process_imu([r[0]], r[1:4], r[4:7])
        else:
            fg.process_vision([st.vision_stamps[k]], st.ids, st.bearings[k])
            assert tf.processVisionData(st.vision_stamps[k], st.ids, st.bearings[k]) == 0
            S1, S0 = tf.stateCovariance(), fg.sigma()
            worst = max(worst, float(np.linalg.norm(S1 - S0) / np.linalg.norm(S0)))
            assert np.abs(S1 - S1.T).max() <= 1e-9 * np.abs(S1).max()
            n_upd += 1
    e1, e0 = tf.stateEstimate(), fg.state_estimate()
    print(f"N={N} slices={slices}: worst Sigma rel-Frobenius difference to the fp64 path over {n_upd} updates {worst:.2e}")
    assert n_upd >= 4 and worst <= tol, worst
    assert worst > 1e-14  # (the integer pipe really ran: the fp64 downdate would agree to rounding)
    assert np.abs(e1["x"] - e0["x"]).max() <= 1e-6 and np.abs(e1["q"] - e0["q"]).max() <= 1e-6 and be.device_error() == 0


@pytest.mark.parametrize("N,bl,dur,chain,dd,tol", [(200, 64, 2.0, 5, 0, 1e-6), (200, 64, 1.0, 5, 6, 1e-5), (1000, 125, 0.26, 5, 0, 1e-6)])
def test_factorisations_on_the_integer_pipe_hold_the_tolerance(N, bl, dur, chain, dd, tol):
    """Round 6: the trailing products of the update's two factorisations (the S-chain with its right-hand sides, the E-chain of bundleLift's
    Sigma_e) on the integer matrix pipe (eqf_tf_set_option "chain_slices"), against the fp64 single-GPU product path on the bench stream, Sigma
    after every update.  The factorisations forgive more than the downdate: FIVE slices (15 integer products) keep Sigma to ~1e-8 -- what the
    CPU study predicted (scripts/slice_precision_study_chain.py: 1.0e-8 at N = 200) -- so the bound here is 1e-6, two orders inside
    north_star's 1e-4; with the downdate on six slices as well the downdate's error (2e-6) is what is left.  Pose to 1e-6."""
    from eqf_vio_amd import binding, synth, tiled

    d = synth.template_settings_dict()
    st = synth.make_stream(N, duration=dur)
    be = tiled.HipBackend(d, capacity=N)
    tf = tiled.TiledFilter(tiled.ProcessGrid(None, 1, 1, device=be.device), be, bl)
    tf.chain_slices = chain
    tf.downdate_slices = dd
    fg = binding.FilterBatch(d, capacity=N, batch=1)
    worst, n_upd = 0.0, 0
    for kind, k in st.events():
        if kind == "imu":
            r = st.imu[k]
            tf.processIMUData(r[0], r[1:4], r[4:7])
            fg.process_imu([r[0]], r[1:4], r[4:7])
        else:
            fg.process_vision([st.vision_stamps[k]], st.ids, st.bearings[k])
            assert tf.processVisionData(st.vision_stamps[k], st.ids, st.bearings[k]) == 0
            S1, S0 = tf.stateCovariance(), fg.sigma()
            worst = max(worst, float(np.linalg.norm(S1 - S0) / np.linalg.norm(S0)))
            assert np.abs(S1 - S1.T).max() <= 1e-9 * np.abs(S1).max()
            n_upd += 1
    e1, e0 = tf.stateEstimate(), fg.state_estimate()
    print(f"N={N} chain_slices={chain} downdate_slices={dd}: worst Sigma rel-Frobenius difference to the fp64 path over {n_upd} updates {worst:.2e}")
    assert n_upd >= 4 and worst <= tol, worst
    assert worst > 1e-14  # (the integer pipe really ran)
    assert np.abs(e1["x"] - e0["x"]).max() <= 1e-6 and np.abs(e1["q"] - e0["q"]).max() <= 1e-6 and be.device_error() == 0


@pytest.mark.parametrize("opts,tol", [({"solve_inverse": 1}, 1e-9), ({"solve_inverse": 1, "downdate_early": 50}, 1e-9), ({"downdate_early": 100}, 1e-9),
                                      ({"trsm_leaf": 1}, 1e-9), ({"trsm_leaf": 2, "solve_inverse": 0, "downdate_early": 30}, 1e-9),
                                      ({"panel_ahead": 1, "chain_slices": 5}, 1e-6), ({"panel_ahead": 1, "solve_inverse": 1}, 1e-9)])
def test_update_options_of_round_6_hold_the_tolerance(opts, tol):
    """The host-loop options that round 6 added (eqf_tf_set_option), each against the fp64 single-GPU product path on the bench stream, Sigma after
    every update: "solve_inverse" (a block row's solve as one product with the explicit inverse of its diagonal factor), "downdate_early" (the
    downdate's shares of the first block rows on the E-chain's stream while the chains are going), "trsm_leaf" (recursive split of the solves),
    "panel_ahead" on one rank (the multi-rank schedule's streams) with the integer-pipe products.  All but the integer pipe are the same
    arithmetic in another order: 1e-9."""
    from eqf_vio_amd import binding, synth, tiled

    N, bl = 200, 24  # (nine block rows, the last one ragged; diagonal blocks of 48 / 72 rows: one and two 64-row strips)
    d = synth.template_settings_dict()
    st = synth.make_stream(N, duration=0.5)
    be = tiled.HipBackend(d, capacity=N)
    tf = tiled.TiledFilter(tiled.ProcessGrid(None, 1, 1, device=be.device), be, bl)
    for name, v in opts.items():
        tf._opt(name, v)
    fg = binding.FilterBatch(d, capacity=N, batch=1)
    worst, n_upd = 0.0, 0
    for kind, k in st.events():
        if kind == "imu":
            r = st.imu[k]
            tf.processIMUData(r[0], r[1:4], r[4:7])
            fg.process_imu([r[0]], r[1:4], r[4:7])
        else:
            fg.process_vision([st.vision_stamps[k]], st.ids, st.bearings[k])
            assert tf.processVisionData(st.vision_stamps[k], st.ids, st.bearings[k]) == 0
            S1, S0 = tf.stateCovariance(), fg.sigma()
            worst = max(worst, float(np.linalg.norm(S1 - S0) / np.linalg.norm(S0)))
            assert np.abs(S1 - S1.T).max() <= 1e-9 * np.abs(S1).max()
            n_upd += 1
    e1, e0 = tf.stateEstimate(), fg.state_estimate()
    print(f"{opts}: worst Sigma rel-Frobenius difference to the product path over {n_upd} updates {worst:.2e}")
    assert n_upd >= 8 and worst <= tol, worst
    assert np.abs(e1["x"] - e0["x"]).max() <= 1e-6 and np.abs(e1["q"] - e0["q"]).max() <= 1e-6 and be.device_error() == 0


def test_product_kernel_builds_agree_bitwise(tmp_path):
    """k_tile_gemm_tn's two builds -- operand rows global -> LDS directly (the default) and through registers (EQF_GEMM_DIRECT=0) -- do the same
    arithmetic in the same order: bitwise the same C, on a whole-tile shape, a ragged one, a view at an odd column and a masked launch.  The
    switch is read once per process, so two processes."""
    import subprocess
    import sys

    code = (
        "import sys, hashlib, numpy as np, torch\n"
        "sys.path.insert(0, %r)\n"
        "from eqf_vio_amd import tiled\n"
        "be = tiled.HipBackend({}, capacity=8)\n"
        "rng = np.random.default_rng(9)\n"
        "h = hashlib.sha256()\n"
        "for (m, n, k, off, mask) in ((512, 640, 96, 0, None), (300, 513, 129, 1, None), (768, 768, 200, 0, (256, 256, 0, 1, 0, 0, 1, 0))):\n"
        "    A = torch.from_numpy(rng.standard_normal((k, m + 3))).cuda(); B = torch.from_numpy(rng.standard_normal((k, n + 3))).cuda()\n"
        "    C = torch.from_numpy(rng.standard_normal((m, n))).cuda()\n"
        "    be.gemm_tn(C, A[:, off: off + m], B[:, off: off + n], -1.0, mask)\n"
        "    torch.cuda.synchronize(); h.update(C.cpu().numpy().tobytes())\n"
        "print(h.hexdigest())\n"
    ) % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))),)
    out = []
    for direct in ("1", "0"):
        env = dict(os.environ, EQF_GEMM_DIRECT=direct)
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        out.append(r.stdout.strip().splitlines()[-1])
    assert len(out[0]) == 64 and out[0] == out[1], out


def test_a_process_does_not_slow_down_with_the_handles_it_has_closed():
    """Round 6: the fifth partitioned filter a process creates runs as fast as the first.  It did not: every handle made eleven CU-masked streams
    (hardware queues of their own), seven of them never used on one rank, and the GPU serves a process at full speed only while the queues it
    has ever put work on stay a handful -- the frame went 68 -> 88 -> 100 -> 128 -> 150 ms over five handles whether the streams were destroyed,
    kept or leaked (profiles/r06_handle_age.txt).  Now a stream is made when it is first needed (four per one-rank handle) and a closed
    handle's streams serve the next one.  One frame (10 IMU calls + the update) of N = 4000 per handle, five handles; 15 % of slack."""
    import gc
    import time

    import torch

    from eqf_vio_amd import synth, tiled

    N, bl = 4000, 250
    d = synth.template_settings_dict()
    st = synth.make_stream(N, duration=0.11)
    ev = list(st.events())
    first_vis = next(i for i, (kind, _) in enumerate(ev) if kind == "vision")
    warm, timed = ev[: first_vis + 1], ev[first_vis + 1: first_vis + 12]
    assert sum(1 for kind, _ in timed if kind == "vision") == 1
    ms = []
    for cycle in range(5):
        be = tiled.HipBackend(d, capacity=N)
        tf = tiled.TiledFilter(tiled.ProcessGrid(None, 1, 1, device=be.device), be, bl)
        assert len(be._raw) == 0  # (a backend that only answers for the filter's handle makes no streams of its own)
        tf.check_every = 0
        for part in (warm, timed):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for kind, k in part:
                if kind == "imu":
                    r = st.imu[k]
                    tf.processIMUData(r[0], r[1:4], r[4:7])
                else:
                    assert tf.processVisionData(st.vision_stamps[k], st.ids, st.bearings[k]) == 0
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        ms.append(dt * 1e3)
        tf.check()
        assert be.device_error() == 0
        tf.close()
        be.close()
        del tf, be
        gc.collect()
    print("ms per frame of the 1st .. 5th handle of the process:", [round(x, 1) for x in ms])
    assert max(ms[1:]) <= 1.15 * ms[0], ms


def test_tiled_filter_N4000_against_the_single_gpu_product_path():
    """BASELINE configs[4] at its size: N = 4000 (Sigma 12011 x 12011, 1.15 GB), blocks of 250 (16 x 16 blocks of 750 x 750), on the 1 x 1
    grid: the first frame (4000 landmarks appended + update), a burst of IMU steps, the second frame's update -- Sigma against the
    single-GPU product path to 1e-9 AND against the committed vectors of the structured fp64 oracle (tests/golden/large_N4000.npz), symmetry,
    positive definiteness (Cholesky succeeds), and the trace going down in every update."""
    import torch

    from eqf_vio_amd import binding, synth, tiled

    from helpers import check_large_golden, load_golden

    N, bl = 4000, 250
    d = synth.template_settings_dict()
    st = synth.make_stream(N, duration=0.11)
    gold, _ = load_golden("large_N4000")
    be = tiled.HipBackend(d, capacity=N)
    tf = tiled.TiledFilter(tiled.ProcessGrid(None, 1, 1, device=be.device), be, bl)
    fg = binding.FilterBatch(d, capacity=N, batch=1)
    rel = lambda A, B: float(np.linalg.norm(A - B) / np.linalg.norm(B))
    n_upd = 0
    for kind, k in st.events():
        if kind == "imu":
            r = st.imu[k]
            tf.processIMUData(r[0], r[1:4], r[4:7])
            fg.process_imu([r[0]], r[1:4], r[4:7])
        else:
            stamp = st.vision_stamps[k]
            fg.process_vision([stamp], st.ids, st.bearings[k])
            n_upd += 1
            assert tf.processVisionData(stamp, st.ids, st.bearings[k]) == 0
            if n_upd == 1:
                prior_tr = 11.0 + 3 * N * d["initialPointVariance"]  # (an upper bound of the prior's trace: the new landmarks' variance)
            St, Sg = tf.stateCovariance(), fg.sigma()
            assert rel(St, Sg) <= 1e-9, (k, rel(St, Sg))
            # ... and against the committed vectors of the structured fp64 oracle for exactly this stream (tests/golden/large_N4000.npz)
            assert np.array_equal(st.bearings[k], gold["bearings"][n_upd - 1]) and st.vision_stamps[k] == gold["vision_stamps"][n_upd - 1]
            check_large_golden(gold, n_upd - 1, tf.stateEstimate(), be.bias(), St, be.last_update(), what="partitioned N=4000")
            assert np.abs(St - St.T).max() <= 1e-9 * np.abs(St).max()
            assert float(np.trace(St)) < prior_tr  # Sigma - K C Sigma takes a positive semi-definite matrix away (the ten Riccati steps in
            prior_tr = float(np.trace(St))          # between add 3 N * 0.05 s * pointProcessVariance: nothing next to what an update removes)
            if n_upd == 2:
                Sd = torch.from_numpy(St).to(be.device)
                torch.linalg.cholesky(Sd)  # raises if Sigma is not positive definite
                del Sd
    assert n_upd >= 2 and be.device_error() == 0 and fg.device_error() == 0
    et, eg = tf.stateEstimate(), fg.state_estimate()
    assert np.abs(et["x"] - eg["x"]).max() <= 1e-9 and np.abs(et["q"] - eg["q"]).max() <= 1e-9 and np.abs(et["p"] - eg["p"]).max() <= 1e-8


def _multi_rank_worker(rank, world, port, Pr, Pc, N, bl, out_dir, opts=""):
    """One of `world` processes that SHARE the one GPU: HipBackend on cuda:0, the grid's broadcasts over gloo (device tensors)."""
    import os
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import torch
    import torch.distributed as dist

    from eqf_vio_amd import synth, tiled
    from oracle import binding as ob

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    d = synth.template_settings_dict()
    be = tiled.HipBackend(d, capacity=N, device_index=0, reserve_cus=0)  # (no CU reservation: eight processes share the chip)
    tf = tiled.TiledFilter(tiled.ProcessGrid(dist, Pr, Pc, device=be.device), be, bl)
    tf.lookahead = False  # (one stream per process: several processes time-share the GPU's hardware queues here)
    for item in filter(None, opts.split(",")):
        name, v = item.split("=")
        tf._opt(name, int(v))
    fo = ob.OracleFilter(d)
    st = synth.make_stream(N, duration=0.16)
    rel = lambda A, B: float(np.linalg.norm(A - B) / np.linalg.norm(B))
    worst, n_upd = dict(S=0.0, pose=0.0, gamma=0.0), 0
    for kind, k in st.events():
        if kind == "imu":
            r = st.imu[k]
            fo.processIMUData(r[0], r[1:4], r[4:7])
            tf.processIMUData(r[0], r[1:4], r[4:7])
        else:
            fo.processVisionData(st.vision_stamps[k], st.ids, st.bearings[k])
            assert tf.processVisionData(st.vision_stamps[k], st.ids, st.bearings[k]) == 0
            n_upd += 1
            worst["S"] = max(worst["S"], rel(tf.stateCovariance(), fo.stateCovariance()))
            eo, et = fo.stateEstimate(), tf.stateEstimate()
            worst["pose"] = max(worst["pose"], float(np.abs(eo["x"] - et["x"]).max()), float(np.abs(eo["q"] - et["q"]).max()),
                                float(np.abs(eo["p"] - et["p"]).max()), float(np.abs(fo.bias() - be.bias()).max()))
            lo, lt = fo.last_update(), be.last_update()
            worst["gamma"] = max(worst["gamma"], float(np.abs(lo["gamma"] - lt["gamma"]).max() / max(1.0, np.abs(lo["gamma"]).max())))
    np.save(os.path.join(out_dir, f"w_{rank}.npy"), np.array([worst["S"], worst["pose"], worst["gamma"], n_upd, be.device_error()]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("Pr,Pc,N,bl,opts,tolS", [(1, 2, 50, 8, "", 1e-9), (2, 2, 44, 8, "", 1e-9), (2, 4, 76, 8, "", 1e-9),
                                                  (2, 2, 44, 8, "solve_inverse=1,downdate_early=50", 1e-9), (2, 4, 76, 8, "solve_inverse=1,downdate_early=100", 1e-9),
                                                  (2, 4, 76, 8, "chain_slices=5", 1e-6), (2, 2, 44, 8, "chain_slices=6,downdate_slices=7", 1e-6)])
def test_tiled_filter_multi_rank_grids_with_the_hip_kernels(tmp_path, Pr, Pc, N, bl, opts, tolS):
    """The multi-rank schedule WITH the HIP backend (block-cyclic local matrices with Pr, Pc > 1, the block-upper mask of the trailing
    products, the interleaved row operand of non-square grids): Pr x Pc processes share the one MI355X, the grid's broadcasts go over
    gloo on device tensors.  Closed loop against the dense oracle on every rank.  (What this cannot show is RCCL over xGMI itself.)
    Round 6: the same with the options that change the schedule's products -- the inverse of the diagonal factor travelling with the
    factor, the downdate's early shares on non-symmetric ranks (Y_I and Y_J different matrices), the integer-pipe products behind the block
    mask of a 2 x 4 grid (operands cut separately: the row operand is not a column range of the other)."""
    import socket

    import torch.multiprocessing as mp

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    world = Pr * Pc
    import gc

    import torch

    gc.collect()  # (handles of earlier tests hold HIP streams = hardware queues the spawned processes would have to share)
    torch.cuda.synchronize()
    mp.spawn(_multi_rank_worker, args=(world, port, Pr, Pc, N, bl, str(tmp_path), opts), nprocs=world, join=True)
    for r in range(world):
        S, pose, gamma, n_upd, err = np.load(tmp_path / f"w_{r}.npy")
        assert n_upd >= 3 and err == 0
        assert S < tolS and pose < max(1e-8, 1e-2 * tolS) and gamma < max(1e-8, 1e-2 * tolS), (r, S, pose, gamma)


# ---- landmark churn in the partitioned filter (VIOFilter.cpp:345-443 on slots: eqf_tiled_edit_landmarks) ----------------------------------
def _drive_churn(tf, fo, st, meas, fg=None):
    """closed loop with a changing landmark set; after every frame ids (reference order), Sigma, state, bias, innovation against the oracle
    (and Sigma against the single-GPU product path), and the inactive slots decoupled exactly"""
    rel = lambda A, B: float(np.linalg.norm(A - B) / np.linalg.norm(B))
    worst = dict(S=0.0, S_product=0.0, pose=0.0, gamma=0.0, Gamma=0.0, delta=0.0, hole=0.0)
    n_upd, sizes = 0, set()
    for kind, k in st.events():
        if kind == "imu":
            r = st.imu[k]
            fo.processIMUData(r[0], r[1:4], r[4:7])
            tf.processIMUData(r[0], r[1:4], r[4:7])
            if fg is not None:
                fg.process_imu([r[0]], r[1:4], r[4:7])
            continue
        ids, y = meas[k]
        fo.processVisionData(st.vision_stamps[k], ids, y)
        assert tf.processVisionData(st.vision_stamps[k], ids, y) == 0
        if fg is not None:
            fg.process_vision([st.vision_stamps[k]], ids, y)
        n_upd += 1
        assert np.array_equal(tf.ids, fo.ids()), (k, tf.ids, fo.ids())
        sizes.add(len(tf.ids))
        St = tf.stateCovariance()
        worst["S"] = max(worst["S"], rel(St, fo.stateCovariance()))
        if fg is not None:
            worst["S_product"] = max(worst["S_product"], rel(St, fg.sigma()))
        eo, et = fo.stateEstimate(), tf.stateEstimate()
        worst["pose"] = max(worst["pose"], float(np.abs(eo["x"] - et["x"]).max()), float(np.abs(eo["q"] - et["q"]).max()),
                            float(np.abs(eo["p"] - et["p"]).max()), float(np.abs(fo.bias() - tf.bias()).max()))
        lo, lt = fo.last_update(), tf.lastUpdate()
        for key in ("delta", "gamma", "Gamma"):
            worst[key] = max(worst[key], float(np.abs(lo[key] - lt[key]).max() / max(1.0, np.abs(lo[key]).max())))
        Sfull = tf.slotCovariance()
        for s_ in np.nonzero(~tf.taken[: tf.nslots])[0]:
            blk = Sfull[11 + 3 * s_: 14 + 3 * s_].copy()
            dg = blk[:, 11 + 3 * s_: 14 + 3 * s_].copy()
            blk[:, 11 + 3 * s_: 14 + 3 * s_] = 0.0
            worst["hole"] = max(worst["hole"], float(np.abs(blk).max()), float(np.abs(dg - dg[0, 0] * np.eye(3)).max()))
            assert dg[0, 0] >= 1.0
    return worst, n_upd, sizes


@pytest.mark.parametrize("N,bl,cap", [(40, 8, 40), (150, 32, 160), (150, 64, 150)])
def test_tiled_filter_landmark_churn_and_outlier_gate_on_the_gpu(oracle_lib, N, bl, cap):
    """1 x 1 grid, HIP kernels: landmarks enter and leave the field of view, three frames carry a bearing 0.05 rad off, the gate at the
    reference default 0.01 -- the slots of the partitioned filter against the dense oracle AND against the single-GPU product path (which
    compacts its Sigma instead, csrc/eqf_churn.hpp)."""
    from eqf_vio_amd import binding, synth, tiled

    d = synth.template_settings_dict()
    d["outlierThreshold"] = 0.01
    st = synth.make_stream(N, duration=0.66)
    meas = synth.churn_measurements(st, seed=11, outlier_frames=(4, 7, 8), outlier_angle=0.05)
    be = tiled.HipBackend(d, capacity=cap)
    tf = tiled.TiledFilter(tiled.ProcessGrid(None, 1, 1, device=be.device), be, bl)
    fo = oracle_lib.OracleFilter(d)
    fg = binding.FilterBatch(d, capacity=N, batch=1)
    worst, n_upd, sizes = _drive_churn(tf, fo, st, meas, fg)
    cs = tf.churn_stats
    assert n_upd >= 12 and cs["removed_old"] >= 3 and cs["removed_outliers"] >= 2 and cs["added"] > N // 3 and len(sizes) >= 3, (cs, sizes)
    assert be.device_error() == 0 and fg.device_error() == 0
    assert worst["S"] <= 1e-9 and worst["S_product"] <= 1e-9 and worst["pose"] <= 1e-8, worst
    assert worst["delta"] <= 1e-10 and worst["gamma"] <= 1e-8 and worst["Gamma"] <= 1e-8, worst
    assert worst["hole"] == 0.0  # exact zeros: a hole never couples to anything


def test_tiled_edit_landmarks_argument_errors_come_before_any_effect():
    """eqf_tiled_edit_landmarks through the C ABI: removing an empty slot, adding into a taken one, leaving an active slot above the new
    slot count, exceeding the capacity -- refused with the handle untouched; then a valid edit."""
    import ctypes

    import torch

    import tiled_reference as tref  # (the Python twin of the host loop: this test drives the per-rank entry points by hand)
    from eqf_vio_amd import binding, synth, tiled

    d = synth.template_settings_dict()
    be = tiled.HipBackend(d, capacity=12)
    tf = tref.TiledFilter(tref.ProcessGrid(None, 1, 1, device=be.device), be, 4)
    st = synth.make_stream(8, duration=0.06)
    for kind, k in st.events():
        if kind == "imu":
            r = st.imu[k]
            tf.processIMUData(r[0], r[1:4], r[4:7])
        else:
            assert tf.processVisionData(st.vision_stamps[k], st.ids, st.bearings[k]) == 0
            break
    S0, e0 = tf.stateCovariance(), tf.stateEstimate()
    lib, ip = be.lib, ctypes.POINTER(ctypes.c_int)
    y = np.ascontiguousarray(st.bearings[0][:2])
    Sll = tf.Sll

    def edit(rem, add, nb, depth=1.0):
        r = np.asarray(rem, dtype=np.int32)
        a = np.asarray(add, dtype=np.int32)
        return lib.eqf_tiled_edit_landmarks(be._h, len(r), r.ctypes.data_as(ip), len(a), a.ctypes.data_as(ip), be._dp(y), depth, nb, be._p(Sll), Sll.stride(0))

    tf._set_slots(12)
    Sll = tf.Sll
    assert edit([9], [], 8) == -1            # slot 9 is empty
    assert edit([], [3], 8) == -1            # slot 3 is taken
    assert edit([2, 2], [], 8) == -1         # twice
    assert edit([], [8, 8], 10) == -1        # twice
    assert edit([], [], 6) == -1             # slots 6, 7 hold landmarks
    assert edit([], [9], 10) == -1           # the working set would grow over slot 8, which nobody fills (never initialised: advisor r4)
    assert edit([], [8], 13) == -4           # EQF_ERR_CAPACITY
    assert edit([], [8], 9, depth=0.0) == -1
    tf._set_slots(8)
    assert np.array_equal(tf.stateCovariance(), S0) and np.array_equal(tf.stateEstimate()["p"], e0["p"])
    assert be.num_landmarks() == 8
    tf._set_slots(9)
    Sll = tf.Sll
    assert edit([3], [3, 8], 9, depth=2.0) == 0  # a slot freed by the call may be refilled by it
    torch.cuda.synchronize()
    assert be.num_landmarks() == 9
    p = be.state_estimate()["p"]
    assert np.allclose(p[3], 2.0 * y[0], atol=1e-14) and np.allclose(p[8], 2.0 * y[1], atol=1e-14)


def _multi_rank_churn_worker(rank, world, port, Pr, Pc, N, bl, cap, out_dir):
    import os
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import torch.distributed as dist

    from eqf_vio_amd import synth, tiled
    from oracle import binding as ob
    from test_gpu_tiled import _drive_churn

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    d = synth.template_settings_dict()
    d["outlierThreshold"] = 0.01
    be = tiled.HipBackend(d, capacity=cap, device_index=0, reserve_cus=0)
    tf = tiled.TiledFilter(tiled.ProcessGrid(dist, Pr, Pc, device=be.device), be, bl)
    tf.lookahead = False
    fo = ob.OracleFilter(d)
    st = synth.make_stream(N, duration=0.46)
    meas = synth.churn_measurements(st, seed=11, outlier_frames=(3, 6), outlier_angle=0.05)
    worst, n_upd, sizes = _drive_churn(tf, fo, st, meas)
    cs = tf.churn_stats
    np.save(os.path.join(out_dir, f"c_{rank}.npy"), np.array([worst["S"], worst["pose"], worst["gamma"], worst["hole"], n_upd, be.device_error(),
                                                              cs["removed_old"], cs["removed_outliers"], cs["added"]]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("Pr,Pc,N,bl,cap", [(2, 2, 44, 8, 48), (2, 4, 70, 8, 70)])
def test_tiled_filter_landmark_churn_on_multi_rank_grids_with_the_hip_kernels(tmp_path, Pr, Pc, N, bl, cap):
    """The slot edits on block-cyclic local matrices with Pr, Pc > 1 (every rank clears its own blocks of a marked slot, nothing moves
    between ranks): Pr x Pc processes share the one MI355X, broadcasts over gloo; every rank against the dense oracle."""
    import gc
    import socket

    import torch
    import torch.multiprocessing as mp

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    world = Pr * Pc
    gc.collect()
    torch.cuda.synchronize()
    mp.spawn(_multi_rank_churn_worker, args=(world, port, Pr, Pc, N, bl, cap, str(tmp_path)), nprocs=world, join=True)
    for r in range(world):
        S, pose, gamma, hole, n_upd, err, rem_old, rem_out, added = np.load(tmp_path / f"c_{r}.npy")
        assert n_upd >= 8 and err == 0 and rem_old >= 2 and rem_out >= 1 and added > N // 3
        assert S < 1e-9 and pose < 1e-8 and gamma < 1e-8 and hole == 0.0, (r, S, pose, gamma, hole)


@pytest.mark.parametrize("N,bl,frames", [(1000, 125, 4), (4000, 250, 2)])
def test_tiled_filter_churn_at_size_against_the_single_gpu_product_path(N, bl, frames):
    """cfg 5's size (and N = 1000): every frame 1 % of the landmarks are out of view and the ones hidden a frame earlier come back as new
    landmarks, gate at 0.01 -- the slots of the partitioned filter against the single-GPU product path's compacting churn
    (csrc/eqf_churn.hpp), two HIP implementations that share no churn code; plus symmetry and the trace of the result."""
    import torch

    from eqf_vio_amd import binding, synth, tiled

    d = synth.template_settings_dict()
    d["outlierThreshold"] = 0.01
    st = synth.make_stream(N, duration=(frames + 1) / 20.0 + 0.011)
    be = tiled.HipBackend(d, capacity=N)
    tf = tiled.TiledFilter(tiled.ProcessGrid(None, 1, 1, device=be.device), be, bl)
    fg = binding.FilterBatch(d, capacity=N, batch=1)
    turn, f = N // 100, 0
    rel = lambda A, B: float(np.linalg.norm(A - B) / np.linalg.norm(B))
    for kind, k in st.events():
        if kind == "imu":
            r = st.imu[k]
            tf.processIMUData(r[0], r[1:4], r[4:7])
            fg.process_imu([r[0]], r[1:4], r[4:7])
            continue
        vis = np.ones(N, dtype=bool)
        vis[(np.arange(turn) + f * turn) % N] = False
        f += 1
        ids, y = st.ids[vis], st.bearings[k][vis]
        assert tf.processVisionData(st.vision_stamps[k], ids, y) == 0
        fg.process_vision([st.vision_stamps[k]], ids, y)
        assert np.array_equal(tf.ids, fg.ids()), f
        St, Sg = tf.stateCovariance(), fg.sigma()
        assert rel(St, Sg) <= 1e-9, (f, rel(St, Sg))
        assert np.abs(St - St.T).max() <= 1e-9 * np.abs(St).max() and abs(np.trace(St) - np.trace(Sg)) <= 1e-9 * np.trace(Sg)
        et, eg = tf.stateEstimate(), fg.state_estimate()
        assert np.abs(et["x"] - eg["x"]).max() <= 1e-9 and np.abs(et["q"] - eg["q"]).max() <= 1e-9 and np.abs(et["p"] - eg["p"]).max() <= 1e-8
        del St, Sg
    cs = tf.churn_stats  # (a landmark the gate took out earlier is not there to leave the field of view)
    assert f >= frames and cs["removed_old"] + cs["removed_outliers"] >= (f - 1) * turn and cs["added"] >= N - turn + (f - 1) * turn and tf.nslots <= N
    assert be.device_error() == 0 and fg.device_error() == 0
    torch.cuda.synchronize()


def test_tiled_filter_restart_from_a_churned_single_gpu_snapshot_and_churn_on(oracle_lib):
    """The product path runs a stream with landmarks entering / leaving / gated out (its state order is no longer id order), its snapshot
    restarts the partitioned filter (slot i = landmark i of the snapshot), and both go on through more churn: ids, Sigma and state stay
    together, and a later snapshot of the tiled filter's covariance equals the oracle's."""
    from eqf_vio_amd import binding, synth, tiled

    N, bl = 60, 16
    d = synth.template_settings_dict()
    d["outlierThreshold"] = 0.01
    st = synth.make_stream(N, duration=0.66)
    meas = synth.churn_measurements(st, seed=11, outlier_frames=(4, 7, 8), outlier_angle=0.05)
    fg = binding.FilterBatch(d, capacity=N, batch=1)
    fo = oracle_lib.OracleFilter(d)
    ev = list(st.events())
    cut = next(i for i, (kind, k) in enumerate(ev) if kind == "vision" and k == 5) + 3
    for kind, k in ev[:cut]:
        if kind == "imu":
            r = st.imu[k]
            fg.process_imu([r[0]], r[1:4], r[4:7])
            fo.processIMUData(r[0], r[1:4], r[4:7])
        else:
            fg.process_vision([st.vision_stamps[k]], *meas[k])
            fo.processVisionData(st.vision_stamps[k], *meas[k])
    snap = fg.dump_state()
    assert not np.array_equal(np.sort(snap["ids"]), snap["ids"]) or len(snap["ids"]) < N  # (the set did change before the cut)
    be = tiled.HipBackend(d, capacity=N)
    tf = tiled.TiledFilter(tiled.ProcessGrid(None, 1, 1, device=be.device), be, bl)
    tf.initialise_from(snap)
    assert np.array_equal(tf.ids, fo.ids())
    rel = lambda A, B: float(np.linalg.norm(A - B) / np.linalg.norm(B))
    n_upd = 0
    for kind, k in ev[cut:]:
        if kind == "imu":
            r = st.imu[k]
            fg.process_imu([r[0]], r[1:4], r[4:7])
            fo.processIMUData(r[0], r[1:4], r[4:7])
            tf.processIMUData(r[0], r[1:4], r[4:7])
        else:
            fg.process_vision([st.vision_stamps[k]], *meas[k])
            fo.processVisionData(st.vision_stamps[k], *meas[k])
            assert tf.processVisionData(st.vision_stamps[k], *meas[k]) == 0
            n_upd += 1
            assert np.array_equal(tf.ids, fg.ids()) and np.array_equal(tf.ids, fo.ids())
            S = tf.stateCovariance()
            assert rel(S, fg.sigma()) <= 1e-9 and rel(S, fo.stateCovariance()) <= 1e-9
    cs = tf.churn_stats
    assert n_upd >= 5 and cs["removed_old"] + cs["removed_outliers"] >= 2 and cs["added"] >= 2, (n_upd, cs)
    e1, e2 = tf.stateEstimate(), fo.stateEstimate()
    assert np.abs(e1["x"] - e2["x"]).max() <= 1e-9 and np.abs(e1["p"] - e2["p"]).max() <= 1e-8 and be.device_error() == 0


@pytest.mark.parametrize("N,bl,imu_rate", [(50, 16, 200.0), (150, 64, 400.0), (37, 8, 1000.0)])
def test_tiled_imu_bursts_equal_the_single_calls_bitwise(oracle_lib, N, bl, imu_rate):
    """eqf_tiled_propagate_burst: the IMU calls between two vision frames + the vision call's integration as ONE pass over the local blocks
    (every call its own linearisation and base panel) against one launch sequence per call -- Sigma, state, bias bitwise equal after every
    frame, with queues that overflow (20 and 50 calls per frame against 15 per burst), with churn and the gate; and against the oracle."""
    from eqf_vio_amd import synth, tiled

    d = synth.template_settings_dict()
    d["outlierThreshold"] = 0.01
    st = synth.make_stream(N, duration=0.36, imu_rate=imu_rate)
    meas = synth.churn_measurements(st, seed=5, outlier_frames=(3,), outlier_angle=0.05)
    fo = oracle_lib.OracleFilter(d)
    tfs = []
    for burst in (True, False):
        be = tiled.HipBackend(d, capacity=N)
        tf = tiled.TiledFilter(tiled.ProcessGrid(None, 1, 1, device=be.device), be, bl)
        tf.burst = burst
        tfs.append(tf)
    n_upd, statuses = 0, [[], []]
    for kind, k in st.events():
        if kind == "imu":
            r = st.imu[k]
            fo.processIMUData(r[0], r[1:4], r[4:7])
            for q, tf in enumerate(tfs):
                statuses[q].append(tf.processIMUData(r[0], r[1:4], r[4:7]))
        else:
            fo.processVisionData(st.vision_stamps[k], *meas[k])
            for q, tf in enumerate(tfs):
                statuses[q].append(tf.processVisionData(st.vision_stamps[k], *meas[k]))
            n_upd += 1
            Sa, Sb = tfs[0].stateCovariance(), tfs[1].stateCovariance()
            assert np.array_equal(Sa, Sb), (n_upd, float(np.abs(Sa - Sb).max()))
            ea, eb = tfs[0].stateEstimate(), tfs[1].stateEstimate()
            assert all(np.array_equal(ea[key], eb[key]) for key in ("q", "x", "v", "p")) and np.array_equal(tfs[0].bias(), tfs[1].bias())
            So = fo.stateCovariance()
            assert np.linalg.norm(Sa - So) / np.linalg.norm(So) <= 1e-9
    assert statuses[0] == statuses[1] and n_upd >= 6
    # a trailing queue is flushed by a getter
    r = st.imu[-1]
    for tf in tfs:
        tf.processIMUData(r[0] + 0.001, r[1:4], r[4:7])
    assert np.array_equal(tfs[0].stateCovariance(), tfs[1].stateCovariance()) and tfs[0].getTime() == tfs[1].getTime() == r[0] + 0.001
    assert tfs[0].be.device_error() == 0 and tfs[1].be.device_error() == 0


@pytest.mark.parametrize("N,bl,cap,panel_ahead", [(50, 16, 60, 0), (200, 64, 200, 0), (37, 8, 48, 0), (50, 16, 60, 1), (150, 32, 150, 1)])
def test_cpp_host_loop_equals_the_python_reference_bitwise(oracle_lib, N, bl, cap, panel_ahead):
    """Round 5: the partitioned filter's host loop is C++ behind the C ABI (csrc/eqf_tiledf.hip, eqf_tf_*).  It was written after the Python
    loop of rounds 3-4, which stays as tests/tiled_reference.py: the same kernels in the same order on the same operands.  On a stream with
    landmarks entering, leaving and failing the gate the two must agree BIT FOR BIT after every frame -- covariance, state, bias, the update's
    internals, the landmark order and the slots behind it -- and the C++ loop's statuses must be the reference's."""
    import tiled_reference as tref
    from eqf_vio_amd import synth, tiled

    d = synth.template_settings_dict()
    d["outlierThreshold"] = 0.01
    st = synth.make_stream(N, duration=0.41)
    meas = synth.churn_measurements(st, seed=9, outlier_frames=(2, 5), outlier_angle=0.05)
    bp = tiled.HipBackend(d, capacity=cap)
    tp = tiled.TiledFilter(tiled.ProcessGrid(None, 1, 1, device=bp.device), bp, bl)
    # panel_ahead = 1: block row k + 1 solved (and, on several ranks, exchanged) on its own stream next to block row k's products, the trailing
    # update split in two launches -- the schedule of grids with more than one rank (csrc/eqf_tiledf.hip, Chain::step), forced onto one rank
    tp._opt("panel_ahead", panel_ahead)
    br = tiled.HipBackend(d, capacity=cap)
    tr = tref.TiledFilter(tref.ProcessGrid(None, 1, 1, device=br.device), br, bl)
    fo = oracle_lib.OracleFilter(d)
    n_upd = 0
    for kind, k in st.events():
        if kind == "imu":
            r = st.imu[k]
            fo.processIMUData(r[0], r[1:4], r[4:7])
            assert tp.processIMUData(r[0], r[1:4], r[4:7]) == tr.processIMUData(r[0], r[1:4], r[4:7])
        else:
            ids, y = meas[k]
            fo.processVisionData(st.vision_stamps[k], ids, y)
            assert tp.processVisionData(st.vision_stamps[k], ids, y) == tr.processVisionData(st.vision_stamps[k], ids, y) == 0
            n_upd += 1
            assert np.array_equal(tp.ids, tr.ids) and np.array_equal(tp.slot_of, tr.slot_of) and tp.nslots == tr.nslots
            assert np.array_equal(tp.ids, fo.ids())
            Sp, Sr = tp.stateCovariance(), tr.stateCovariance()
            assert np.array_equal(Sp, Sr), (n_upd, float(np.abs(Sp - Sr).max()))
            assert np.array_equal(tp.slotCovariance(), tr.slotCovariance())
            ep, er = tp.stateEstimate(), tr.stateEstimate()
            assert all(np.array_equal(ep[key], er[key]) for key in ("q", "x", "v", "p")) and np.array_equal(tp.bias(), tr.bias())
            lp, lr = tp.lastUpdate(), tr.lastUpdate()
            assert all(np.array_equal(lp[key], lr[key]) for key in ("delta", "gamma", "Gamma"))
            So = fo.stateCovariance()
            assert np.linalg.norm(Sp - So) / np.linalg.norm(So) <= 1e-9
    assert n_upd >= 7 and tp.churn_stats == tr.churn_stats and tp.churn_stats["removed_outliers"] > 0
    assert tp.device_error() == 0 and br.device_error() == 0
    assert tp.getTime() == tr.getTime()


def test_cpp_tiled_facade_matches_the_oracle(oracle_lib):
    """The C++ host facade of the partitioned filter (eqf_vio_amd/cpp/VIOFilterTiled.h: the reference's class interface over eqf_tf_*),
    driven by a plain g++ program on a 1 x 1 grid with landmarks leaving and coming back, reproduces the oracle on the same inputs."""
    import os
    import re
    import subprocess

    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eqf_vio_amd", "cpp", "eqf_example_tiled")
    assert os.path.exists(exe), "build it with __graft_entry__.build()"
    N, frames, bl = 30, 9, 8
    out = subprocess.run([exe, str(N), str(frames), str(bl)], capture_output=True, text=True, check=True).stdout
    nums = [float(x) for x in re.findall(r"[-+]?\d+\.\d+(?:e[-+]?\d+)?", out)]
    t, pos, q, fro = nums[0], nums[1:4], nums[4:8], nums[8]
    nlm = int(re.search(r"N=(\d+)", out).group(1))
    i = np.arange(N)
    lm = np.stack([2 * np.sin(1.3 * i), 2 * np.cos(0.7 * i), 5 + np.sin(0.37 * i)], axis=1)
    y = lm / np.linalg.norm(lm, axis=1, keepdims=True)
    fo = oracle_lib.OracleFilter(dict(initialPointVariance=5000.0, measurementVariance=0.003, velOmegaVariance=1e-4,
                                      velAccelVariance=1e-4, outlierThreshold=1e9))
    k = 0
    for f in range(frames):
        stamp = 0.05 * f + 0.0025
        while 0.005 * k < stamp:
            fo.processIMUData(0.005 * k, [0, 0, 0], [9.81, 0, 0])
            k += 1
        vis = (f + i) % 7 != 0
        fo.processVisionData(stamp, i[vis].astype(np.int32), y[vis])
    e = fo.stateEstimate()
    assert nlm == fo.N and abs(t - fo.getTime()) < 1e-9
    assert np.abs(np.array(pos) - e["x"]).max() < 2e-6 and np.abs(np.array(q) - e["q"]).max() < 2e-6  # printed with 6 digits
    assert abs(fro / np.linalg.norm(fo.stateCovariance()) - 1) < 1e-6


def test_update_replayed_from_a_hipgraph_equals_the_plain_launches():
    """One rank: an update's launch sequence -- prep, the two factorisations on four streams, downdate, finish -- can be captured as a hipGraph
    and replayed with ONE launch (option "graphs"; off by default: the replay is slower on the GPU, csrc/eqf_tiledf.hip).  Through the plain
    C++ example (the system's HIP runtime): the same printed pose and |Sigma|_F as the plain launches, and the replay must actually happen."""
    import os
    import re
    import subprocess

    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eqf_vio_amd", "cpp", "eqf_example_tiled")
    outs = []
    for graphs in ("1", "0"):
        r = subprocess.run([exe, "150", "14", "64", "timing", "graphs=" + graphs], capture_output=True, text=True, check=True)
        outs.append(r.stdout)
    first = [o.splitlines()[0] for o in outs]
    assert first[0] == first[1] and "N=150" in first[0], outs
    replays = [int(re.search(r"(\d+) updates replayed from a hipGraph", o).group(1)) for o in outs]
    assert replays[0] >= 8 and replays[1] == 0, replays


def _multi_rank_golden_worker(rank, world, port, Pr, Pc, N, bl, out_dir):
    import os
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import torch.distributed as dist

    from eqf_vio_amd import tiled
    from helpers import check_large_golden, events_of, load_golden

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    d, settings = load_golden(f"large_N{N}")
    be = tiled.HipBackend(settings, capacity=N, device_index=0, reserve_cus=0)  # (no CU reservation: the processes share the chip)
    tf = tiled.TiledFilter(tiled.ProcessGrid(dist, Pr, Pc, device=be.device), be, bl)
    tf.lookahead = False
    worst, f = 0.0, 0
    g = tf.g
    upd_bytes = []  # bytes this rank RECEIVED through the broadcast callback during each vision call (frame 0 adds the landmarks: no exchange yet)
    for kind, k in events_of(d["imu"], d["vision_stamps"]):
        if kind == "imu":
            r = d["imu"][k]
            tf.processIMUData(r[0], r[1:4], r[4:7])
        else:
            b0 = g.bcast_bytes_received
            assert tf.processVisionData(d["vision_stamps"][k], d["ids"], d["bearings"][k]) == 0
            tf.synchronize()
            upd_bytes.append(g.bcast_bytes_received - b0)
            S = tf.stateCovariance()
            worst = max(worst, check_large_golden(d, f, tf.stateEstimate(), tf.bias(), S, tf.lastUpdate(), what=f"{Pr} x {Pc} grid, N={N}, rank {rank}"))
            del S
            f += 1
    np.save(os.path.join(out_dir, f"g_{rank}.npy"), np.array([worst, f, tf.device_error(), max(upd_bytes)]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("Pr,Pc,N,bl", [(2, 4, 2000, 125), (2, 4, 4000, 250)])
def test_tiled_filter_on_the_node_grid_at_size_against_the_committed_oracle_vectors(tmp_path, Pr, Pc, N, bl):
    """The grid of one 8-GPU node, 2 x 4, AT SIZE: N = 2000 (Sigma 6011 x 6011, 16 x 16 landmark blocks of 125) as eight processes sharing the
    one MI355X, the C++ host loop on every rank with the schedule of grids larger than one rank (block row k + 1 solved and exchanged next
    to block row k's products, every exchange on one ordered stream), the broadcasts over gloo on device memory -- against the committed
    vectors of the structured fp64 oracle (tests/golden/large_N2000.npz, three updates; round 6: also BASELINE configs[4]'s own size, N = 4000 with
    blocks of 250, tests/golden/large_N4000.npz, two updates) after every update, on every rank; the bytes every rank received through the
    broadcast callback during an update are held against DESIGN.md section 7's SUMMA-restricted volume.  (What this
    cannot show is RCCL over xGMI itself, nor a frame time: eight processes time-share the chip.)"""
    import gc
    import socket

    import torch
    import torch.multiprocessing as mp

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    world = Pr * Pc
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from helpers import load_golden

    nframes = len(load_golden(f"large_N{N}")[0]["vision_stamps"])  # (three updates at N = 2000, two at N = 4000)
    assert nframes >= 2
    gc.collect()
    torch.cuda.synchronize()
    mp.spawn(_multi_rank_golden_worker, args=(world, port, Pr, Pc, N, bl, str(tmp_path)), nprocs=world, join=True)
    recv = []
    for r in range(world):
        worst, f, err, nbytes = np.load(tmp_path / f"g_{r}.npy")
        assert f == nframes and err == 0 and worst < 1e-8, (r, worst, f, err)
        recv.append(nbytes)
    # Exchange volume of an update, per rank, against DESIGN.md section 7: SUMMA-restricted, a rank receives (1 / Pr + 1 / Pc) of every solved
    # block row [U_k | Y_k] of both chains -- upper block triangle of m x m plus the m x (n + 18) right-hand sides for the S-chain (m = 2 N, n =
    # 11 + 3 N), upper block triangle of n_e x n_e plus 11 columns for the E-chain (n_e = 5 + 3 N padded to blocks) -- minus what it holds itself.
    n, m, ne = 11 + 3 * N, 2 * N, 3 * N
    rows = 8.0 * (m * m / 2 + m * (n + 18) + ne * ne / 2 + ne * 11)
    model = (1.0 / Pr + 1.0 / Pc) * rows
    print(f"N={N} grid {Pr}x{Pc}: bytes received per update and rank: min {min(recv) / 1e9:.3f} GB, max {max(recv) / 1e9:.3f} GB; "
          f"(1/Pr + 1/Pc) x solved block rows = {model / 1e9:.3f} GB (DESIGN.md section 7: 0.75 x (0.26 + 0.77) GB at N = 4000)")
    assert 0.4 * model < min(recv) and max(recv) < 1.05 * model, (recv, model)  # (a rank does not receive the pieces it holds itself)
