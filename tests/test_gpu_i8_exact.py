"""The int8-slice products on the MI355X BIT FOR BIT against their numpy model (tests/i8_emulator.py): eqf_tile_downdate_i8 and
eqf_tile_gemm_tn_i8 (the partitioned filter's "downdate_slices" / "chain_slices", csrc/eqf_i8.hpp) and eqf_tile_syrk_i8 (the handles'
"downdate_slices", the same header), five to seven slices.  An error bound cannot see a kernel bug smaller than the slicing error itself
(a truncating splitter, one lost half-chunk of the lowest slice pair); equality with the emulator can.  Ragged shapes around the 32-row
chunks and the 128 x 64 / 64 x 64 tiles, views with leading dimensions and sentinels around them, the block mask, A as a column range of B,
column maxima at powers of two and at 2^e (1 - 2^-53), exact ties, subnormal and near-overflow columns, zero and -0.0 columns, NaN / Inf,
and the int32 accumulators at the exactness limits.  Plus the partitioned filter with a NaN block in Sigma: the integer-pipe options leave
the same pattern as fp64."""
import ctypes as C

import numpy as np
import pytest

import i8_emulator as E

pytestmark = pytest.mark.gpu

MN = (1, 31, 32, 33, 127, 128, 129, 257)
KS = (1, 16, 17, 31, 32, 33, 500)
EQF_ERR_INVALID = -1


def _env():
    import torch

    from eqf_vio_amd import binding

    return torch, torch.device("cuda", 0), binding.lib()


def _stream(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _tile(Cd, Ad, Bd, S, mask=None, mask_cols=0, k=None):
    """eqf_tile_gemm_tn_i8 on torch views (unit column stride); returns the status code."""
    torch, dev, L = _env()
    m, n = Cd.shape
    k = Ad.shape[0] if k is None else k
    need = int(L.eqf_tile_i8_workspace_bytes(m, n, k, S, 0))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    mk = mask if mask is not None else (0, 0, 0, 1, 0, 0, 1, 0)
    rc = L.eqf_tile_gemm_tn_i8(0, _stream(torch), C.c_void_p(Cd.data_ptr()), Cd.stride(0), m, n, C.c_void_p(Ad.data_ptr()), Ad.stride(0),
                               C.c_void_p(Bd.data_ptr()), Bd.stride(0), k, S, *[int(x) for x in mk], int(mask_cols), C.c_void_p(ws.data_ptr()),
                               need)
    torch.cuda.synchronize()
    return rc


def _downdate(Cd, Ad, Bd, S, mask_rb=0):
    torch, dev, L = _env()
    m, n = Cd.shape
    k = Ad.shape[0]
    same = Ad.data_ptr() == Bd.data_ptr() and Ad.shape == Bd.shape
    need = int(L.eqf_tile_i8_workspace_bytes(m, n, k, S, int(same)))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rc = L.eqf_tile_downdate_i8(0, _stream(torch), C.c_void_p(Cd.data_ptr()), Cd.stride(0), m, n, C.c_void_p(Ad.data_ptr()), Ad.stride(0),
                                C.c_void_p(Bd.data_ptr()), Bd.stride(0), k, S, int(mask_rb), C.c_void_p(ws.data_ptr()), need)
    torch.cuda.synchronize()
    return rc


def _syrk(Yd, Sd, Sout, nv, mp, S):
    """eqf_tile_syrk_i8 on torch tensors Y [B, mpMax, ldY], Sin / Sout [B, nvMax, ld]; returns the status code."""
    torch, dev, L = _env()
    B = Yd.shape[0]
    nva, mpa = (C.c_int * B)(*nv), (C.c_int * B)(*mp)
    need = int(L.eqf_tile_syrk_i8_workspace_bytes(B, max(nv), max(mp), S))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rc = L.eqf_tile_syrk_i8(0, _stream(torch), B, nva, mpa, C.c_void_p(Yd.data_ptr()), Yd.stride(1), Yd.stride(0), C.c_void_p(Sd.data_ptr()),
                            C.c_void_p(Sout.data_ptr()), Sd.stride(1), Sd.stride(0), S, C.c_void_p(ws.data_ptr()), need)
    torch.cuda.synchronize()
    return rc


def _special_columns(rng, k, n):
    """k x n operand whose first columns are the edge cases (as many as fit), the rest N(0, 1) x 10^U(-3, 3)."""
    X = rng.standard_normal((k, n)) * 10.0 ** rng.uniform(-3, 3, size=(1, n))
    cols = []
    x = np.clip(rng.standard_normal(k), -7.9, 7.9)
    x[rng.integers(k)] = 8.0                                       # largest |entry| an exact power of two (scaled: 0.5)
    cols.append(x)
    x = rng.uniform(-1, 1, k) * 2.0 ** 5
    x[0] = (1.0 - 2.0 ** -53) * 2.0 ** 5                           # 2^e (1 - 2^-53): q0 = 64
    cols.append(x)
    t = rng.integers(0, 5, size=k)                                 # exact ties: odd multiples of half a unit of slice t
    x = (2 * rng.integers(-40, 40, size=k) + 1) * np.ldexp(1.0, -(7 + 7 * t))
    x[0] = 0.75
    cols.append(x)
    cols.append(rng.standard_normal(k) * 1e-318)                   # subnormal maximum (scale factor 2^-e would overflow)
    cols.append(rng.standard_normal(k) * 2.0 ** -1060)             # (subnormal, larger)
    cols.append(rng.standard_normal(k) * 1e-300)                   # tiny, normal
    cols.append(np.zeros(k))                                       # all zero
    cols.append(np.full(k, -0.0))                                  # all -0.0
    x = np.zeros(k)
    x[k // 2] = -3.0                                               # one entry
    cols.append(x)
    for j, c in enumerate(cols[:n]):
        X[:, j] = c
    return X


def _huge_tiny(rng, k, m, n):
    """A column near 2^1023 against tiny ones: A (k x m) with column 0 ~ 1e307, B (k x n) with every column <= 1e-290."""
    A = rng.standard_normal((k, m)) * 10.0 ** rng.uniform(-2, 2, size=(1, m))
    A[:, 0] = rng.uniform(-1, 1, k) * 1.7e308
    B = rng.standard_normal((k, n)) * 10.0 ** rng.uniform(-320, -290, size=(1, n))
    return A, B


def _check_view(got, C0, r0, c0, m, n, want, what):
    """Inside the view: bit for bit the emulator; outside: the sentinels untouched."""
    inside = np.zeros(C0.shape, dtype=bool)
    inside[r0: r0 + m, c0: c0 + n] = True
    assert E.bits_equal(got[~inside], C0[~inside]), ("written outside the view", what)
    g = got[r0: r0 + m, c0: c0 + n]
    if not E.bits_equal(g, want):
        bad = ~((g == want) | (np.isnan(g) & np.isnan(want))) | (np.signbit(g) != np.signbit(want))
        i, j = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {int(bad.sum())} of {m * n} elements differ from the emulator, first ({i}, {j}): {g[i, j]!r} vs {want[i, j]!r}")


def _tile_case(rng, m, n, k, S, special=True, downdate=False):
    torch, dev, _ = _env()
    A = _special_columns(rng, k, m + 5) if special else rng.standard_normal((k, m + 5))
    B = _special_columns(rng, k, n + 3) if special else rng.standard_normal((k, n + 3))
    A = A[:, ::-1].copy()  # (the edge columns at the END of A: other tiles than B's)
    C0 = rng.standard_normal((m + 3, n + 7))
    C0[0, 0] = -0.0
    C0[1, 2] = -0.0
    Ad, Bd, Cd = (torch.from_numpy(x).to(dev) for x in (A, B, C0))
    Av, Bv = A[:, 1: 1 + m], B[:, 3: 3 + n]
    if downdate:
        rc = _downdate(Cd[1: 1 + m, 2: 2 + n], Ad[:, 1: 1 + m], Bd[:, 3: 3 + n], S)
    else:
        rc = _tile(Cd[1: 1 + m, 2: 2 + n], Ad[:, 1: 1 + m], Bd[:, 3: 3 + n], S)
    assert rc == 0
    want = E.tile_gemm(C0[1: 1 + m, 2: 2 + n], Av, Bv, S)
    _check_view(Cd.cpu().numpy(), C0, 1, 2, m, n, want, (m, n, k, S, downdate))


@pytest.mark.parametrize("S", [5, 6, 7])
def test_tile_product_bitwise_ragged_shapes(S):
    """C -= A^T B (eqf_tile_gemm_tn_i8, eqf_tile_downdate_i8) on every m, n in {1, 31, 32, 33, 127, 128, 129, 257} and every k in
    {1, 16, 17, 31, 32, 33, 500}, views with ld > width and sentinels around them, random data and the edge-case columns."""
    rng = np.random.default_rng(100 + S)
    for i in range(len(MN)):
        for j in range(len(MN)):
            if (i + j) % 3 and not (i == j == len(MN) - 1):
                continue
            m, n, k = MN[i], MN[j], KS[(i + 2 * j) % len(KS)]
            _tile_case(rng, m, n, k, S, special=bool((i + j) % 2), downdate=(i + j) % 4 == 0)
    for k in KS:
        _tile_case(rng, 129, 33, k, S)


@pytest.mark.parametrize("S", [5, 6, 7])
def test_tile_product_bitwise_extreme_scales(S):
    """A column near 2^1023 against tiny columns (the product is ordinary), subnormal columns against huge ones, and products that
    under- and overflow: bit for bit."""
    torch, dev, _ = _env()
    rng = np.random.default_rng(200 + S)
    for (m, n, k) in ((33, 40, 17), (128, 64, 500)):
        A, B = _huge_tiny(rng, k, m, n)
        C0 = rng.standard_normal((m, n))
        C0[:, n // 2:] = 0.0  # (zero entries: tiny products are not absorbed)
        Cd = torch.from_numpy(C0).to(dev)
        assert _tile(Cd, torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev), S) == 0
        _check_view(Cd.cpu().numpy(), C0, 0, 0, m, n, E.tile_gemm(C0, A, B, S), ("huge x tiny", m, n, k))
        A2 = _special_columns(rng, k, m)
        B2 = rng.standard_normal((k, n)) * 10.0 ** rng.uniform(-300, 300, size=(1, n))
        Cd = torch.from_numpy(C0).to(dev)
        assert _tile(Cd, torch.from_numpy(A2).to(dev), torch.from_numpy(B2).to(dev), S) == 0
        _check_view(Cd.cpu().numpy(), C0, 0, 0, m, n, E.tile_gemm(C0, A2, B2, S), ("wide scales", m, n, k))


@pytest.mark.parametrize("S", [5, 6, 7])
def test_tile_product_bitwise_masks_and_column_ranges(S):
    """The block mask (the existing cases of test_tile_gemm_tn_on_the_integer_pipe_behind_the_block_mask, smaller k), A as a column range
    of B at offsets 0 and 32 (cut once) and 20 (cut separately), the downdate's symmetric mask with A == B: bit for bit, skipped tiles
    untouched."""
    torch, dev, _ = _env()
    rng = np.random.default_rng(300 + S)
    #        m    n (incl. rhs)  k  rb  rblk0 Pr pr cblk0 Pc pc  mask_cols  A's offset in B (None: separate)
    cases = ((600, 600 + 37, 33, 150, 0, 1, 0, 0, 1, 0, 600, 0),
             (450, 600 + 18, 31, 150, 1, 1, 0, 0, 1, 0, 600, None),
             (512, 640 + 5, 17, 128, 0, 1, 0, 0, 1, 0, 640, 128),
             (500, 500 + 9, 16, 100, 2, 2, 1, 1, 2, 0, 500, None),
             (300, 77, 64, 0, 0, 1, 0, 0, 1, 0, 0, None),
             (257, 300, 40, 100, 0, 1, 0, 0, 1, 0, 300, 32),
             (260, 300, 40, 100, 0, 1, 0, 0, 1, 0, 300, 20),
             (129, 129, 500, 0, 0, 1, 0, 0, 1, 0, 0, 0))
    for (m, n, k, rb, rblk0, Pr, pr, cblk0, Pc, pc, mcols, aoff) in cases:
        B = _special_columns(rng, k, n + 3)
        Bd = torch.from_numpy(B).to(dev)
        Bv, Bdv = B[:, 1: 1 + n], Bd[:, 1: 1 + n]
        if aoff is None:
            A = _special_columns(rng, k, m)[:, ::-1].copy()
            Adv = torch.from_numpy(A).to(dev)
        else:
            A, Adv = Bv[:, aoff: aoff + m], Bdv[:, aoff: aoff + m]
        C0 = rng.standard_normal((m, n + 4))
        Cd = torch.from_numpy(C0).to(dev)
        mask = (rb, rb, rblk0, Pr, pr, cblk0, Pc, pc) if rb else None
        assert _tile(Cd[:, 2: 2 + n], Adv, Bdv, S, mask=mask, mask_cols=mcols) == 0
        want = E.tile_gemm(C0[:, 2: 2 + n], A, Bv, S, mask=mask, mask_cols=mcols)
        _check_view(Cd.cpu().numpy(), C0, 0, 2, m, n, want, (m, n, k, rb, aoff))
        if rb and m >= 384:
            assert E.tile_skipped(m, n, mask, mcols).any()
    # the downdate's symmetric local matrix: the same view on both sides, blocks of 96
    n, k, rb = 384, 200, 96
    Y = _special_columns(rng, k, n)
    C0 = rng.standard_normal((n, n + 3))
    Yd, Cd = torch.from_numpy(Y).to(dev), torch.from_numpy(C0).to(dev)
    assert _downdate(Cd[:, :n], Yd, Yd, S, mask_rb=rb) == 0
    want = E.tile_gemm(C0[:, :n], Y, Y, S, mask=(rb, rb, 0, 1, 0, 0, 1, 0), mask_cols=n)
    _check_view(Cd.cpu().numpy(), C0, 0, 0, n, n, want, ("downdate mask", S))


def test_tile_product_at_the_k_limit():
    """k = 70 000 with every scaled digit 63 (S = 7): the accumulators reach k S 63^2 = 0.906 x 2^31 -- bit for bit; k = 70 001 is
    rejected with EQF_ERR_INVALID before anything is written."""
    torch, dev, _ = _env()
    k, m, n, S = 70000, 33, 40, 7
    rng = np.random.default_rng(7)
    A = E.all63(k, m, e=3)
    B = E.all63(k, n, e=-2)
    B[:, 5] *= -1.0
    C0 = rng.standard_normal((m, n + 2))
    p = E.Product(A, B, S)
    assert p.max_acc >= 0.9 * 2 ** 31
    Ad, Bd, Cd = (torch.from_numpy(x).to(dev) for x in (A, B, C0))
    assert _tile(Cd[:, 1: 1 + n], Ad, Bd, S) == 0
    _check_view(Cd.cpu().numpy(), C0, 0, 1, m, n, E.tile_gemm(C0[:, 1: 1 + n], A, B, S), "k = 70000")
    A1 = torch.from_numpy(E.all63(k + 1, m)).to(dev)
    B1 = torch.from_numpy(E.all63(k + 1, n)).to(dev)
    Cd = torch.from_numpy(C0).to(dev)
    assert _tile(Cd[:, 1: 1 + n], A1, B1, S) == EQF_ERR_INVALID
    assert _downdate(Cd[:, 1: 1 + n], A1, B1, S) == EQF_ERR_INVALID
    assert E.bits_equal(Cd.cpu().numpy(), C0)


def _fp64_nonfinite(C0, A, B):
    """Where fp64 C - A^T B is not finite (products formed one by one: a BLAS may skip the zeros that turn Inf into NaN)."""
    with np.errstate(all="ignore"):
        P = (A[:, :, None] * B[:, None, :]).sum(axis=0)
        return ~np.isfinite(C0 - P)


@pytest.mark.parametrize("S", [5, 6, 7])
def test_tile_product_non_finite_columns(S):
    """NaN, +Inf and -Inf in a column of A, of B and of both -- inside the masked columns and in the right-hand sides, and with A == B
    (the downdate): every element fp64 makes non-finite is non-finite, every other one equals the emulator with the bad columns as
    zero (bit for bit, the emulator writes NaN for a flagged row / column), skipped tiles untouched."""
    torch, dev, _ = _env()
    rng = np.random.default_rng(400 + S)
    m, n, k, rb, mcols = 256, 256 + 37, 40, 64, 256
    mask = (rb, rb, 0, 1, 0, 0, 1, 0)
    for trial, bads in enumerate((
            [("A", 5, 3, np.nan)],
            [("B", 200, 0, np.inf)],
            [("B", 270, k - 1, -np.inf)],                               # a right-hand-side column
            [("A", 70, 7, np.inf), ("B", 70, 9, -np.inf)],              # both operands, same index
            [("A", 130, 39, -np.inf), ("B", 3, 20, np.nan), ("B", 280, 1, np.inf)],
            [("A", 200, 600, np.nan)])):                                # (row past k: NOT part of the product)
        A = _special_columns(rng, k + 1, m)[:, ::-1].copy()
        B = _special_columns(rng, k + 1, n)
        A[k, :] = np.nan  # (row k lies outside the product's k rows: must not be read)
        B[k, :] = np.inf
        for (w, col, row, val) in bads:
            if row < k:
                (A if w == "A" else B)[row, col] = val
        A, B = A[:k + 1], B[:k + 1]
        C0 = rng.standard_normal((m, n))
        Ad, Bd, Cd = (torch.from_numpy(x).to(dev) for x in (A, B, C0))
        assert _tile(Cd, Ad[:k], Bd[:k], S, mask=mask, mask_cols=mcols) == 0
        got = Cd.cpu().numpy()
        want = E.tile_gemm(C0, A[:k], B[:k], S, mask=mask, mask_cols=mcols)
        _check_view(got, C0, 0, 0, m, n, want, ("non-finite", trial))
        keep = ~E.tile_skipped(m, n, mask, mcols)
        nf = _fp64_nonfinite(C0, A[:k], B[:k]) & keep
        assert nf.any() == any(row < k for (_, _, row, _) in bads)
        assert not np.isfinite(got[nf]).any(), trial
    # the downdate with one operand (cut once): a NaN column poisons its row and column
    Y = _special_columns(rng, k, 200)
    Y[4, 150] = np.nan
    Y[0, 33] = -np.inf
    C0 = rng.standard_normal((200, 200))
    Yd, Cd = torch.from_numpy(Y).to(dev), torch.from_numpy(C0).to(dev)
    assert _downdate(Cd, Yd, Yd, S) == 0
    got = Cd.cpu().numpy()
    _check_view(got, C0, 0, 0, 200, 200, E.tile_gemm(C0, Y, Y, S), "downdate non-finite")
    assert not np.isfinite(got[_fp64_nonfinite(C0, Y, Y)]).any()


def _syrk_case(rng, nv, mp, S, special=True, bad=()):
    torch, dev, _ = _env()
    B, nvM, mpM = len(nv), max(nv), max(max(mp), 32)
    ld, ldY = nvM + 3, nvM + 5
    Y = np.empty((B, mpM, ldY))
    for b in range(B):
        Y[b] = _special_columns(rng, mpM, ldY)[:, ::(1 if b % 2 else -1)] if special else rng.standard_normal((mpM, ldY))
    for (b, row, col, val) in bad:
        Y[b, row, col] = val
    Sin = rng.standard_normal((B, nvM, ld))
    Sin[-1] = 0.0  # (the last filter's Sigma zero: tiny and subnormal products are not absorbed into O(1) entries)
    Sin[:, 0, 0] = -0.0
    Yd, Sd = torch.from_numpy(Y).to(dev), torch.from_numpy(Sin).to(dev)
    Sout = torch.full_like(Sd, 7.0)
    assert _syrk(Yd, Sd, Sout, nv, mp, S) == 0
    got = Sout.cpu().numpy()
    for b in range(B):
        want = E.syrk(Sin[b, :nv[b], :nv[b]], Y[b, :mp[b], :nv[b]], S)
        sent = np.full((nvM, ld), 7.0)
        _check_view(got[b], sent, 0, 0, nv[b], nv[b], want, ("syrk", nv, mp, S, b))
        if mp[b] and any(bb == b and r < mp[b] and c < nv[b] for (bb, r, c, _) in bad):
            Yb = Y[b, :mp[b], :nv[b]]
            with np.errstate(all="ignore"):
                nf = ~np.isfinite(Sin[b, :nv[b], :nv[b]] - (Yb[:, :, None] * Yb[:, None, :]).sum(axis=0))
            assert nf.any() and not np.isfinite(got[b, :nv[b], :nv[b]][nf]).any()


@pytest.mark.parametrize("S", [5, 6, 7])
def test_syrk_bitwise_batches(S):
    """eqf_tile_syrk_i8 over batches with ragged nv / mp, filters that are only copied (mp = 0), the edge-case columns and NaN / +Inf /
    -Inf: every filter's Sout bit for bit the emulator's (upper triangle formed, lower mirrored), nothing written outside nv x nv."""
    rng = np.random.default_rng(500 + S)
    _syrk_case(rng, (257, 31, 1, 129), (64, 32, 96, 0), S)
    _syrk_case(rng, (33, 32, 128, 127), (512, 0, 32, 96), S, special=False)
    _syrk_case(rng, (129, 64, 300, 40, 77, 31, 200, 33), (32, 64, 160, 500 // 32 * 32, 32, 64, 96, 128), S)
    _syrk_case(rng, (100, 90, 65), (64, 96, 32), S, bad=((0, 3, 17, np.nan), (1, 95, 40, np.inf), (2, 0, 64, -np.inf),
                                                         (2, 31, 2, np.nan), (0, 70, 5, np.nan)))  # (row 70 >= mp of filter 0: not read)


@pytest.mark.parametrize("S", [5, 6, 7])
def test_syrk_at_the_mp_limit(S):
    """The largest mp eqf_tile_syrk_i8 accepts (mp S 64^2 < 2^31) with every scaled digit 63: accumulators mp S 63^2 >= 0.9 x 2^31, bit
    for bit; one chunk more is rejected with EQF_ERR_INVALID and Sout is left as it was."""
    torch, dev, _ = _env()
    mp = (2 ** 31 - 1) // (S * 4096) // 32 * 32
    nv = 37
    Y = E.all63(mp + 32, nv + 3, e=1)
    Y[:, 4] *= -1.0
    Y[:, 9] = E.all63(mp + 32, 1, e=-20)[:, 0]
    assert E.Product(Y[:mp, :nv], Y[:mp, :nv], S).max_acc >= 0.9 * 2 ** 31
    rng = np.random.default_rng(S)
    Sin = rng.standard_normal((1, nv, nv + 1))
    Yd, Sd = torch.from_numpy(Y[None]).to(dev), torch.from_numpy(Sin).to(dev)
    Sout = torch.full_like(Sd, 7.0)
    assert _syrk(Yd, Sd, Sout, (nv,), (mp,), S) == 0
    _check_view(Sout.cpu().numpy()[0], np.full((nv, nv + 1), 7.0), 0, 0, nv, nv, E.syrk(Sin[0, :, :nv], Y[:mp, :nv], S), ("mp limit", S))
    Sout = torch.full_like(Sd, 7.0)
    assert _syrk(Yd, Sd, Sout, (nv,), (mp + 32,), S) == EQF_ERR_INVALID
    assert (Sout.cpu().numpy() == 7.0).all()


# ---- the partitioned filter with a non-finite Sigma

def test_partitioned_non_finite_sigma_same_pattern_as_fp64():
    """The partitioned filter's counterpart of test_non_finite_sigma_same_pattern_as_fp64: a NaN block loaded through initialise_from, then
    one update with "downdate_slices" 6 and "chain_slices" 5 and one on the fp64 path: the same return code, the same device_error and the
    same pattern of finite entries in Sigma."""
    from eqf_vio_amd import binding, synth, tiled

    N, bl = 40, 16
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
    snap = fg.dump_state()
    snap["sigma"] = snap["sigma"].copy()
    snap["sigma"][11 + 3 * 7: 11 + 3 * 8, 11 + 3 * 7: 11 + 3 * 8] = np.nan
    res = []
    for opts in ({}, {"downdate_slices": 6, "chain_slices": 5}):
        be = tiled.HipBackend(d, capacity=N)
        tf = tiled.TiledFilter(tiled.ProcessGrid(None, 1, 1, device=be.device), be, bl)
        for key, v in opts.items():
            setattr(tf, key, v)
        tf.initialise_from(snap)
        rc, Sg = None, None
        for kind, k in ev[cut:]:
            if kind == "imu":
                r = st.imu[k]
                tf.processIMUData(r[0], r[1:4], r[4:7])
            else:
                try:
                    rc = tf.processVisionData(st.vision_stamps[k], st.ids, st.bearings[k])
                except (binding.EqfError, ArithmeticError) as e:
                    rc = (type(e).__name__, getattr(e, "code", None))
                break
        try:
            Sg = tf.stateCovariance()
        except binding.EqfError as e:
            Sg = e.code
        res.append((rc, be.device_error(), Sg))
    (rc0, err0, S0), (rc8, err8, S8) = res
    print(f"fp64: rc {rc0}, device_error {err0}; integer pipe: rc {rc8}, device_error {err8}")
    assert rc8 == rc0 and err8 == err0
    if isinstance(S0, int) or isinstance(S8, int):
        assert S8 == S0
    else:
        assert np.array_equal(np.isfinite(S8), np.isfinite(S0))
        assert not np.isfinite(S0).all()  # (the NaN did reach the update)
