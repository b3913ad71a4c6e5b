"""TEST INFRASTRUCTURE ONLY -- the sizes, covariance families and the vision call that tests/test_update_exact.py (CPU) and
tests/test_gpu_update.py (MI355X) share, so that the bound is checked on the CPU for exactly the cases the device is held to.

State: riccati_cases.device_snapshot / oracle_snapshot unchanged (three IMU calls behind the fourth vision frame, accumulators set).  The call
under test is the stream's NEXT vision frame, the fifth, with its own bearings; it integrates about 25 ms first.
Sizes: the S-chain has 2 N columns and the E-chain 5 + 3 N, in block columns of 64.
    1 (singular normal equations), 2, 5   19, 20, 21 (E-chain 62 / 65 / 68 columns; from N = 20 the one-launch kernel is the default)
    32, 33 (S-chain 64 / 66)   41, 42 (E-chain 128 / 131)   64, 65, 70 (three and four block columns: interior tiles)
Sigma families, all exactly symmetric and positive definite:
    a  the filter's own Sigma                          b  riccati_cases' graded D C D (Sigma+ and gamma only: cond(Sigma_e) reaches 1e14)
    c  block-sparse: an 11 x 11 SPD base block, independent 3 x 3 SPD landmark blocks, one coupling accel bias <-> landmark min(N - 1, 15),
       one coupling landmark 15 <-> 16 across the tile edge -- few-term products, a mis-indexed block is an O(1) miss
    e  family a with the bearings rotated by about 0.05 rad, so that delta and gamma are not small"""
import numpy as np

import riccati_cases as rc

SIZES = (1, 2, 5, 19, 20, 21, 32, 33, 41, 42, 64, 65, 70)
FAMILIES = ("a", "b", "c", "e")
GAMMA6_FAMILIES = ("a", "c", "e")       # Gamma[0:6] is asserted on these for N >= 2; family b and N = 1 are reported
FOLD_PREP0 = (21, 33, 70)
PER_COLUMN = (5, 21, 33, 70)
SLICES = (33, 70)
F32 = (17, 70)
F32_FAMILIES = ("a", "c")
BURST = (33, 70)
RAGGED = (5, 21, 33)
BATCH_N = 200
TILED = rc.TILED
TILED_BIG = rc.TILED_BIG
CPU_SIZES = tuple(sorted(set(SIZES + F32 + RAGGED)))
ROTATION = 0.05
FRAME = 4


def settings():
    return rc.settings()


TRSM_SPLIT = 6   # csrc/eqf_tiledf.hip kTrsmSplit: 64-row blocks of a diagonal factor from which a block row's solve is split once


def tiled_schedule(N, bl, solve_inverse=False, trsm_leaf=0):
    """The keyword arguments of update_exact.update_bounds for the partitioned filter on (N, bl), counted from the schedule of
    csrc/eqf_tiledf.hip (update_exact's docstring, "The partitioned filter"): one addition per block row, one per level of the split solve of
    the larger chain's largest diagonal block (none under solve_inverse, which does not solve), and the whole-block inverse."""
    def levels(nb):
        if trsm_leaf > 0:
            return 0 if nb <= trsm_leaf else 1 + levels(nb - nb // 2)
        return 1 if nb >= TRSM_SPLIT else 0

    b = min(bl, N)
    out = dict(block_rows=-(-N // bl), split_levels=0 if solve_inverse else max(levels(-(-unit * b // 64)) for unit in (2, 3)))
    if solve_inverse:
        out["inverse_blocks"] = (2 * bl, 3 * bl)
    return out


def gamma6_asserted(N, fam):
    return N >= 2 and fam in GAMMA6_FAMILIES


def _mirror(S):
    return np.triu(S) + np.triu(S, 1).T


def _spd(k, rng, scale):
    M = rng.standard_normal((k, k))
    return scale * (M @ M.T / k + np.eye(k))


def sigma_family(snap, fam):
    N = len(snap["ids"])
    n = 11 + 3 * N
    if fam in ("a", "e"):
        return rc.sigma_family(snap, "a")
    if fam == "b":
        return rc.sigma_family(snap, "b")
    rng = np.random.default_rng(2000 + N)
    S = np.zeros((n, n))
    S[:11, :11] = _spd(11, rng, 0.05)
    for i in range(N):
        S[11 + 3 * i:14 + 3 * i, 11 + 3 * i:14 + 3 * i] = _spd(3, rng, 10.0 ** rng.uniform(-2, 1))
    d = np.sqrt(np.diag(S))
    i0 = min(N - 1, 15)
    S[4, 11 + 3 * i0 + 1] = -0.4 * d[4] * d[11 + 3 * i0 + 1]           # accel bias y x landmark i0
    if N >= 17:
        S[11 + 3 * 15, 11 + 3 * 16 + 2] = 0.3 * d[11 + 45] * d[11 + 50]   # landmark 15 x landmark 16: across the tile edge
    return _mirror(S)


def _rotate(y, angle):
    a = np.array([0.48, -0.6, 0.64])
    return np.array([v * np.cos(angle) + np.cross(a, v) * np.sin(angle) + a * (a @ v) * (1 - np.cos(angle)) for v in y])


def vision_call(N, fam):
    """(stamp, ids, bearings (N, 3)) of the fifth vision frame"""
    st = rc.plan(N)[0]
    y = st.bearings[FRAME].copy()
    if fam == "e":
        y = _rotate(y, ROTATION)
        y /= np.linalg.norm(y, axis=1, keepdims=True)
    return float(st.vision_stamps[FRAME]), st.ids, y


def imu_calls_before(N, k=3):
    """The stream's next k IMU calls behind the snapshot (the burst case queues them in front of the vision call)"""
    r = rc.plan(N)[2]
    return [(float(r[j][0]), r[j][1:4].copy(), r[j][4:7].copy()) for j in range(k)]
