"""k_tile_gemm_tn (csrc/eqf_tile.hpp: C += alpha A^T B on the fp64 matrix cores, every dense product of the partitioned update) entry by
entry against the longdouble reference of tests/gemm_exact.py, within its a-priori bound E = gamma_{k+2} |alpha| |A|^T |B| + u |C_ref|
(derived there; bit-equality where it is zero), through tiled.HipBackend.gemm_tn and lib.eqf_tile_downdate.  The same shapes, families and
alphas hold numpy's product and a model of the kernel's order inside the bound on the CPU (tests/test_gemm_exact.py), where six injected
faults leave it.

Operands are views at odd column offsets inside larger buffers with odd leading dimensions, so that a row starts 8 or 16 bytes aligned in
turn.  The padding around C holds a finite sentinel and must keep its bits (np.array_equal calls a NaN unequal to itself); the padding
around A and B holds NaN, which must not reach C -- a ragged tile or chunk that read one element past its operand would.

What each shape reaches is written from the code beside gemm_exact's tuples: LOOP the straight-line chunk loop (whole tile, k >= 32) with
zero, one, two fast chunks and a ragged chunk behind them; SHORT_K one chunk, full and ragged, on a whole and on a ragged tile; MIXED whole,
ragged-row, ragged-column and corner tiles in one launch; EDGES every count mu / nv of 16-row sub-tiles of a wave; the mask with a plan
(gemmMakePlan's staircase walk) and without one (more than kGemmPlanRows = 256 tile rows: round-robin, inactive tiles leave at once).

Measured on an MI355X, worst ratio to the bound per family (NOTES.md R35.1 has the table per shape): from k = 16 on normal 0.19, scaled
0.19, cancelling 0.11, zero_column 0.21; at k = 1 .. 5, where the bound is three to seven roundings, normal 0.97, scaled 0.94, cancelling
0.48, zero_column 0.92 (k = 1: 0.97 of gamma_3 |a b| + u |C_ref|).  integers: bit-equal at alpha = +-1 (the bound is zero), 0.053 where
alpha rounds.  Mask with a plan 0.092, and 29584 of the 60000 entries below the staircase untouched (the others lie in tiles that hold a
kept entry); mask without a plan bit-equal, 130 whole tiles skipped."""
import ctypes

import numpy as np
import pytest

import gemm_exact as gx

pytestmark = pytest.mark.gpu

SENTINEL = -7.25  # finite, exactly representable, and nothing a kernel would compute


@pytest.fixture(scope="module")
def be():
    from eqf_vio_amd import tiled

    b = tiled.HipBackend({}, capacity=8)
    yield b
    b.close()


class _View:
    """An r x c matrix inside a larger device buffer filled with `fill`: offset rows, an ODD column offset and an ODD leading dimension"""

    def __init__(self, A, fill, top=1, left=3, bottom=2, right=4):
        import torch

        r, c = A.shape
        if (c + left + right) % 2 == 0:
            right += 1
        assert left % 2 == 1 and (c + left + right) % 2 == 1
        self.host = np.full((r + top + bottom, c + left + right), fill)
        self.host[top: top + r, left: left + c] = A
        self.inside = np.zeros(self.host.shape, dtype=bool)
        self.inside[top: top + r, left: left + c] = True
        self.dev = torch.from_numpy(self.host).to(torch.device("cuda", 0))
        self.view = self.dev[top: top + r, left: left + c]
        self.shape = (r, c)

    def fetch(self):
        """the view's content now; asserts that nothing outside it changed, bit for bit (finite fills only)"""
        got = self.dev.cpu().numpy()
        assert np.array_equal(got[~self.inside], self.host[~self.inside]), "a write strayed outside the view"
        return got[self.inside].reshape(self.shape)


def _product(be, C, A, B, alpha, mask=None, downdate=False):
    """C += alpha A^T B on padded views -> the new C (after the check that C's padding kept its bits)"""
    import torch

    cv, av, bv = _View(C, SENTINEL), _View(A, np.nan, 2, 1, 1, 2), _View(B, np.nan, 1, 5, 3, 6)
    assert cv.view.stride(0) % 2 == av.view.stride(0) % 2 == bv.view.stride(0) % 2 == 1
    if downdate:
        assert alpha == -1.0 and mask is None
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        m, n = C.shape
        rc = be.lib.eqf_tile_downdate(be.dev, be._cur(), p(cv.view), cv.view.stride(0), m, n, p(av.view), av.view.stride(0), p(bv.view),
                                      bv.view.stride(0), A.shape[0])
        assert rc == 0
    else:
        be.gemm_tn(cv.view, av.view, bv.view, alpha, mask=mask)
    torch.cuda.synchronize()
    return cv.fetch()


def _held(be, family, shape, alpha, worst, downdate=False):
    m, n, k = shape
    C, A, B = gx.operands(family, m, n, k)
    ref = gx.reference(C, A, B, alpha)
    E = gx.bound(ref, A, B, alpha, C)
    got = _product(be, C, A, B, alpha, downdate=downdate)
    r, at = gx.worst_ratio(got, ref, E)
    worst[family] = max(worst.get(family, 0.0), r)
    assert r <= 1.0, (family, shape, alpha, r, at)
    if family == "zero_column":  # an all-zero operand column leaves its row / column of C alone, bit for bit
        assert np.array_equal(got[m // 2], C[m // 2]) and np.array_equal(got[:, n // 3], C[:, n // 3])
    return got


def _report(what, worst):
    print(f"{what}: worst ratio to the bound  " + "  ".join(f"{f} {v:.3g}" for f, v in worst.items()))


@pytest.mark.parametrize("shape", gx.LOOP + gx.MIXED)
def test_straight_line_loop_and_mixed_tiles(be, shape):
    """(128, 128, 16): nFast = 0, the predicated body alone; 32: one straight-line chunk whose global -> LDS copies fill buffer 1; 48: two, the
    second into buffer 0 again; 49: the straight-line chunks, then the predicated body on a ragged chunk whose buffer was last written by a
    straight-line one.  (257, 129, 33): tiles (0, 0) and (1, 0) whole, (2, 0) one row, column tile 1 one column.  Every alpha, every family."""
    worst = {}
    for family in gx.FAMILIES:
        for alpha in gx.ALPHAS:
            _held(be, family, shape, alpha, worst)
    _report(f"product {shape}", worst)


@pytest.mark.parametrize("shape", gx.SHORT_K)
def test_short_k(be, shape):
    """k = 1, 3, 4, 5, 17: less than one k step, one, one and a ragged one, one chunk and one row -- on a whole tile and on a 20 x 20 one;
    through eqf_tile_downdate (alpha = -1, no mask) and through gemm_tn"""
    worst = {}
    for family in gx.FAMILIES:
        a = _held(be, family, shape, -1.0, worst, downdate=True)
        b = _held(be, family, shape, -1.0, worst)
        assert np.array_equal(a, b)
    _report(f"product {shape}", worst)


@pytest.mark.parametrize("m", gx.EDGES)
def test_sub_tile_edges(be, m):
    """m against every n of {1, 16, 17, 64, 65, 80, 81, 127} at k = 20: mu and nv from 1 to 4 in both waves of a tile row / column, a wave
    with nothing to do (m <= 64), one row or column past a sub-tile and past a wave"""
    worst = {}
    for n in gx.EDGES:
        for family in ("scaled", "cancelling", "integers"):
            _held(be, family, (m, n, gx.EDGE_K), -1.0, worst)
    _report(f"product m = {m}", worst)


def test_the_same_call_twice_gives_the_same_bits(be):
    """one writer per element and a fixed order inside it: nothing in a launch depends on which workgroup runs first"""
    for shape in ((257, 129, 33), (128, 128, 49)):
        C, A, B = gx.operands("scaled", *shape)
        assert np.array_equal(_product(be, C, A, B, 0.3), _product(be, C, A, B, 0.3))


@pytest.mark.parametrize("shape", [(128, 128, 49), (257, 129, 33), (20, 20, 5)])
def test_one_nan_in_b_stays_in_its_column(be, shape):
    """A NaN at B[k - 1, j] (the ragged chunk's last live row): column j of C is NaN from top to bottom, every other column is within the
    bound of the reference -- a product that let operand columns mix (a wrong LDS column, a shifted sub-tile) would spread it."""
    m, n, k = shape
    C, A, B = gx.operands("normal", m, n, k)
    j = n - 3
    ref = gx.reference(C, A, B, -1.0)
    E = gx.bound(ref, A, B, -1.0, C)
    B = B.copy()
    B[k - 1, j] = np.nan
    got = _product(be, C, A, B, -1.0)
    assert np.all(np.isnan(got[:, j]))
    keep = np.arange(n) != j
    r, at = gx.worst_ratio(got[:, keep], ref[:, keep], E[:, keep])
    assert r <= 1.0, (shape, r, at)


def test_mask_with_a_plan(be):
    """Rank (1, 0) of a 2 x 2 grid, blocks of 100, (300, 300, 40): three tile rows whose staircases start at column tiles 0, 1 and -- the
    last block row keeps nothing -- 3 (none).  On and above the staircase every entry is within the bound; below it an entry is either
    bit-equal to what C held (its tile was skipped) or within the bound of the full product (its tile holds a kept entry)."""
    m = n = 300
    k, mask = 40, (100, 100, 0, 2, 1, 0, 2, 0)
    kept = gx.mask_kept(m, n, mask)
    worst = {}
    for family in gx.FAMILIES:
        C, A, B = gx.operands(family, m, n, k)
        ref = gx.reference(C, A, B, -1.0)
        E = gx.bound(ref, A, B, -1.0, C)
        got = _product(be, C, A, B, -1.0, mask=mask)
        err = np.abs(got.astype(gx.LD) - ref)
        inside = (err <= E) & ~np.isnan(got)
        assert np.all(inside[kept]), (family, "above the staircase")
        assert np.all(inside[~kept] | (got == C)[~kept]), (family, "below the staircase")
        worst[family] = gx.worst_ratio(got[kept], ref[kept], E[kept])[0]
        print(f"mask with a plan, {family}: {int((got == C)[~kept].sum())} of {int((~kept).sum())} entries below the staircase untouched")
    _report("mask with a plan", worst)


def test_mask_without_a_plan(be):
    """257 tile rows (m = 257 * 128 > kGemmPlanRows * 128): gemmMakePlan declines, the launch covers the whole rectangle round-robin and an
    inactive tile's workgroup returns at once.  Row blocks of 16384 (128 tile rows), column blocks of 128, integer operands, k = 4: every
    kept entry is bit-equal to the exact product, every entry below the staircase is untouched or the exact product, and the tiles of the
    second row block under the first column block -- and the last tile row -- are skipped whole."""
    m, n, k = 257 * gx.TILE, 256, 4
    mask = (16384, 128, 0, 1, 0, 0, 1, 0)
    C, A, B = gx.operands("integers", m, n, k)
    want = C - A.T @ B            # exact: integers below 2^53
    assert not gx.bound(gx.reference(C, A, B, -1.0), A, B, -1.0, C).any()
    got = _product(be, C, A, B, -1.0, mask=mask)
    kept = gx.mask_kept(m, n, mask)
    assert np.array_equal(got[kept], want[kept])
    below = ~kept
    assert np.all((got == C)[below] | (got == want)[below])
    skipped = 0
    for ti in range(m // gx.TILE):
        for tj in range(n // gx.TILE):
            t = (slice(ti * gx.TILE, (ti + 1) * gx.TILE), slice(tj * gx.TILE, (tj + 1) * gx.TILE))
            if not kept[t].any() and np.array_equal(got[t], C[t]) and not np.array_equal(C[t], want[t]):
                skipped += 1
    print(f"mask without a plan: {skipped} whole tiles skipped")
    assert skipped >= 1
