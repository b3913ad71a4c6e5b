"""TEST INFRASTRUCTURE ONLY -- the states, covariance families, sizes and stored constants that tests/test_consistency_exact.py (CPU) and
tests/test_gpu_consistency_exact.py (MI355X) share, so that every bound is checked on the CPU for exactly the cases the device is held to.

PART A (csrc/eqf_local.hpp: Sigma in the coordinates of the estimate).  The states are made here, no stream runs: A rotated by 2.5 rad about a
general axis, Q_i random rotations of up to pi - 0.1, scales a_i log-uniform in [0.05, 20], and an origin pose whose gravity direction
eta0 = R_P0^T e3 lies 0.5 rad or 1e-2 rad from e3, the pole of its chart (both outside the 1e-8 threshold: no error bit).  One master state
of 273 landmarks; the state of N landmarks is its prefix, so one reference J serves every size.
    Sizes: 1, 15, 16, 17 (the 16-row chunk of k_sigma_local), 255, 256, 257 (its 256-lane column chunk), 272, 273 (both edges at once);
    capacity N + 7, so that the strides of Q[5][cap] and of the J record differ from N.
    Sigma families:
      a  a filter's own Sigma after five vision frames of synth.make_stream (N <= 17 only; the caller supplies it)
      b  riccati_cases' graded D C D, six decades
      c  sparse +-1 indicators, mirrored: base x base, gravity x gravity, base x landmark, landmark x landmark across the 16-row edge (15 | 16),
         across the 256-lane edge (255 | 256), across both (16 | 256) and corner to corner (0 | N - 1), and full 3 x 3 diagonal blocks -- every
         output entry is a product of a few J entries, so a mis-indexed block names its row / column landmark and its entry
      d  family b with the strictly lower triangle doubled (exact): Sigma_Jb != Sigma_bJ^T, which pins "read as stored, not as the
         transpose" (eqf_set_sigma stores what it is given: k_sigma_import copies entry by entry)

PART B (csrc/eqf_nees.hpp, csrc/eqf_sample.hpp: eqf_get_nees, eqf_sample_sigma, eqf_perturb_filters).  The state is part A's (theta = 0.5), so
the local chart mixes every 3 x 3 block with a rotation and a scale; the matrices go in through set_sigma:
      own        a filter's own Sigma after five vision frames (the caller supplies it)
      graded     chol_bounds.graded(n, 6)           one_small  chol_bounds.one_small(n, 8)
      coupled    update_cases' family c: an SPD base block, independent SPD landmark blocks, +- couplings across the tile edge
      lifted     2^28 x one_small(n, 8) (an exact scaling): every pivot exceeds 1, so min_pivot is the one case in which the pad row's 1.0
                 would win if it were counted -- the four families above all have a pivot below 1 and cannot tell
    N = 1, 17, 18, 39, 43, 64, 82: the kernels' internal orders with first = 0 are 15, 63, 66, 129, 141, 204, 258 (258 > 256: the stride of the
    tail's sums); with first = 11, N = 43 gives 129, a one-row last block.  first = 0 | 6 | 11: the pad row sits at index 11 or 5 of the first
    block, or is absent.  Both charts; 1, 15, 16 error vectors; 1, 16, 17, 64 draws; scale 1 and -0.5.  nees_plan(N) walks the families and
    charts and turns the other arguments so that every value of each is met at every size (N = 43 with first = 11 and N = 82 with first = 0
    among them); the ragged handle [0, 5, 18, 70] takes all three `first`, with first = 11 its empty filter has order 0.

PART C (csrc/eqf_innov.hpp: eqf_get_innovation_stats).  update_cases' state, call and families a, c, e at N = 1, 5, 21, 64, 65, 70; N = 130
(m = 260 crosses the 256-stride of the sums of nis and logdet_S) and N = 257 (the stride of nis_lm), family a.  Routes: update_cases' sets.

THE CONSTANTS.  K_J (one each for G, R_A^T and the landmark blocks) is 4 x the worst error of consistency_helpers.chart_jacobian_blocks_oracle
(the numpy ORACLE's chart functions, plain fp64) against the 50-digit J of consistency_exact.jacobian_mp over the two master states, in units
of u max|block| (G: (u / theta^2) max|G|, theta the smaller angle of eta0 and etaHat from e3).  tests/test_consistency_exact.py recomputes
the oracle's ratios on every run and asserts ratio <= stored (the rule of lie_edge_cases.py); the device's number is never the yardstick.
C_LOG is 4 x the worst error of numpy's log against mp.log over the pivots L_kk of every committed case of part B, in units of
u (1 + |log L_kk|); same rule."""
import numpy as np

import chol_bounds as cb
import lie_edge_cases as ec
import riccati_cases as rc
import update_cases as uc

LOCAL_SIZES = (1, 15, 16, 17, 255, 256, 257, 272, 273)
LOCAL_MASTER = 273
LOCAL_THETAS = (0.5, 1e-2)
LOCAL_RAGGED = (0, 5, 257, 17)
LOCAL_OWN_MAX = 17          # family a up to here
LOCAL_FAMILIES = ("a", "b", "c", "d")
CAP_EXTRA = 7

# The numpy oracle's worst ratios as tests/test_consistency_exact.py measures them (x86-64, glibc), to the last digit; K = 4 x ratio, unrounded.
ORACLE_J = {"G": 2.1046352390343714, "RAt": 1.0533443029750047, "lm": 7.68425737744045}
ORACLE_LOG = 0.8136791266918791
# ORACLE-END
C_LOG = 4 * ORACLE_LOG
K_J = {k: 4 * v for k, v in ORACLE_J.items()}


def settings():
    return rc.settings()


def _qmul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                     w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


_MASTER = {}


def _master(theta):
    if theta not in _MASTER:
        M = LOCAL_MASTER
        rng = np.random.default_rng(1700)
        ang, az = rng.uniform(0.1, 0.6, M), rng.uniform(0, 2 * np.pi, M)
        p = np.stack([np.sin(ang) * np.cos(az), np.sin(ang) * np.sin(az), np.cos(ang)], axis=1) * rng.uniform(2.0, 8.0, M)[:, None]
        Qq = np.array([ec._quat(rng.standard_normal(3), rng.uniform(0.0, np.pi - 0.1)) for _ in range(M)])
        Qa = np.exp(rng.uniform(np.log(0.05), np.log(20.0), M))
        # R_P0 takes y (theta from e3, azimuth 1.3) to e3, then turns about e3: eta0 = R_P0^T e3 = y
        y = np.array([np.sin(theta) * np.cos(1.3), np.sin(theta) * np.sin(1.3), np.cos(theta)])
        q0 = _qmul(ec._quat([0.0, 0.0, 1.0], 0.7), ec._quat(np.cross(y, [0.0, 0.0, 1.0]), theta))
        origin = dict(q=q0, x=np.array([0.4, -0.7, 1.2]), v=np.array([0.3, -0.2, 0.5]), p=p)
        group = dict(Aq=ec._quat([-0.5, 0.2, 0.9], 2.5), Ax=np.array([0.3, 0.1, -0.2]), w=np.array([0.05, -0.08, 0.03]), Qq=Qq, Qa=Qa)
        _MASTER[theta] = (origin, group)
    return _MASTER[theta]


def local_state(N, theta):
    """A snapshot (FilterBatch.dump_state format) of the first N landmarks of the master state; sigma is the identity until a family is set."""
    o, g = _master(theta)
    origin = dict(q=o["q"].copy(), x=o["x"].copy(), v=o["v"].copy(), p=o["p"][:N].copy())
    group = dict(Aq=g["Aq"].copy(), Ax=g["Ax"].copy(), w=g["w"].copy(), Qq=g["Qq"][:N].copy(), Qa=g["Qa"][:N].copy())
    return dict(ids=np.arange(10, 10 + N, dtype=np.int32), origin=origin, group=group, bias=np.array([0.01, -0.02, 0.005, 0.1, -0.05, 0.02]),
                sigma=np.eye(11 + 3 * N), time=1.0, currentVelocity=np.zeros(6), accumulatedVelocity=np.zeros(6), accumulatedTime=0.0,
                initialised=1)


def local_families(N):
    return tuple(f for f in LOCAL_FAMILIES if f != "a" or 1 <= N <= LOCAL_OWN_MAX)


def local_indicators(N):
    """[(row, column, value)] of family c above the diagonal, in the coordinates of sigma(); the diagonal blocks come on top."""
    lm = lambda i, c: 11 + 3 * i + c  # noqa: E731
    out = [(2, 9, 1.0), (6, 7, -1.0), (7, 10, 1.0)]
    if N >= 1:
        out += [(4, lm(min(N - 1, 15), 1), -1.0), (6, lm(N - 1, 2), 1.0), (9, lm(0, 0), -1.0)]
    if N >= 17:
        out += [(lm(15, 0), lm(16, 2), 1.0), (lm(0, 1), lm(N - 1, 0), -1.0)]
    if N >= 257:
        out += [(lm(255, 0), lm(256, 1), 1.0), (lm(16, 2), lm(256, 0), -1.0), (lm(15, 1), lm(255, 2), 1.0), (8, lm(256, 2), 1.0), (3, lm(255, 1), -1.0)]
    return out


def local_sigma(snap, fam, own=None):
    """Sigma of family `fam` for the snapshot's size (family a: `own`, the filter's own Sigma, mirrored)."""
    N = len(snap["ids"])
    n = 11 + 3 * N
    if fam == "a":
        assert own is not None and own.shape == (n, n)
        return rc._mirror(np.asarray(own, dtype=float))
    if fam == "b":
        return rc.sigma_family(snap, "b")
    if fam == "d":
        S = rc.sigma_family(snap, "b")
        return np.triu(S) + 2.0 * np.tril(S, -1)
    S = np.zeros((n, n))
    for r, c, v in local_indicators(N):
        S[r, c] = v
    blk = np.array([[1.0, -1.0, 1.0], [-1.0, 1.0, -1.0], [1.0, -1.0, 1.0]])
    for i in sorted({min(N - 1, 16), N - 1, min(N - 1, 255)} - {-1}):
        S[11 + 3 * i:14 + 3 * i, 11 + 3 * i:14 + 3 * i] = blk
    S[6:8, 6:8] += np.array([[1.0, 0.0], [0.0, -1.0]])
    return rc._mirror(S)


def local_spd(N):
    """A well-conditioned SPD Sigma (lie_edge_cases._spd: a diagonal in [0.5, 2] plus rank six) whose image J Sigma J^T every chain factors: the
    ragged handle's, where the many-filter launch is compared through nees / sample_sigma."""
    return rc._mirror(ec._spd(11 + 3 * N, np.random.default_rng(1800 + N)))


# ---- part B ---------------------------------------------------------------------------------------------------------------------------------
NEES_SIZES = (1, 17, 18, 39, 43, 64, 82)
NEES_RAGGED = (0, 5, 18, 70)
NEES_FAMILIES = ("own", "graded", "one_small", "coupled", "lifted")
NEES_FIRSTS = (0, 6, 11)
NEES_NRHS = (1, 15, 16)
NEES_NSAMP = (1, 16, 17, 64)
NEES_SCALES = (1.0, -0.5)
NEES_THETA = LOCAL_THETAS[0]


def nees_sigma(N, fam, own=None):
    n = 11 + 3 * N
    if fam == "own":
        assert own is not None and own.shape == (n, n)
        return rc._mirror(np.asarray(own, dtype=float))
    if fam == "graded":
        return cb.graded(n, 6)
    if fam == "one_small":
        return cb.one_small(n, 8)
    if fam == "lifted":
        return 2.0 ** 28 * cb.one_small(n, 8)
    return uc.sigma_family(dict(ids=np.arange(N)), "c")


def nees_plan(N):
    """[(family, local, first, nrhs, nsamp, scale)]"""
    out, idx = [], 0
    for fam in NEES_FAMILIES[:4]:
        for local in (0, 1):
            out.append((fam, local, NEES_FIRSTS[(idx + N) % 3], NEES_NRHS[idx % 3], NEES_NSAMP[(idx + N) % 4], NEES_SCALES[idx % 2]))
            idx += 1
    have = {(f, l, fi) for f, l, fi, _, _, _ in out}
    for j, first in enumerate(NEES_FIRSTS):  # every `first` on the graded family in the origin chart, at every size
        if ("graded", 0, first) not in have:
            out.append(("graded", 0, first, NEES_NRHS[(j + 1) % 3], NEES_NSAMP[(j + 2) % 4], NEES_SCALES[j % 2]))
    out.append(("lifted", 0, NEES_FIRSTS[N % 2], NEES_NRHS[N % 3], NEES_NSAMP[N % 4], NEES_SCALES[N % 2]))  # (first = 0 | 6: the pad is there)
    return out


def nees_vectors(N, fam, local, first, k, what):
    """k seeded standard normal vectors in the reference index map (11 + 3 N entries; those below `first` are ignored by the device)"""
    seed = [N, NEES_FAMILIES.index(fam), local, first, k, 0 if what == "err" else 1]
    return np.random.default_rng(seed).standard_normal((k, 11 + 3 * N))


# ---- part C ---------------------------------------------------------------------------------------------------------------------------------
INNOV_SIZES = (1, 5, 21, 64, 65, 70)
INNOV_FAMILIES = ("a", "c", "e")
INNOV_BIG = ((130, ("a", "c", "e")), (257, ("a",)))
INNOV_PER_COLUMN = (5, 21, 70)
INNOV_SLICES = (70,)
INNOV_BATCH = 21            # one handle of three filters of this size, one family each


def innov_cases():
    """[(N, family)]"""
    return [(N, f) for N in INNOV_SIZES for f in INNOV_FAMILIES] + [(N, f) for N, fams in INNOV_BIG for f in fams]
