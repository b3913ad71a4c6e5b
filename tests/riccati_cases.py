"""TEST INFRASTRUCTURE ONLY -- the states, covariance families, sizes and IMU calls that tests/test_riccati_exact.py (CPU) and
tests/test_gpu_riccati.py (MI355X) share, so that the bound is checked on the CPU for exactly the cases the device is held to.

State: a filter driven over synth.make_stream(N) to three IMU calls behind the fourth vision frame (FilterBatch on the GPU, the C++ oracle on the
CPU: the same state up to rounding; the bound is computed from whichever snapshot is used), then given a non-zero accumulatedTime /
accumulatedVelocity (the state IMU calls under fastRiccati leave; every route reads it, and T = accumulatedTime + dt != dt is what tells the
accumulated time from this call's dt).
Sigma families, all exactly symmetric (the upper triangle is mirrored):
    a  the filter's own Sigma                          b  graded: D C D, C a random correlation matrix, D = 10^uniform(-4, 2) per coordinate
    c  sparse indicators: +-1 at (gyro bias, velocity), (accel bias, landmark i0), (landmark 15, landmark 16) across the tile edge, and one full
       3 x 3 diagonal block -- every output entry is a product of a few F entries, so a mis-indexed block is an O(1) miss
    d  family a with a gap of dt = 0.1 s, so that the terms of second order in T are not small"""
import numpy as np

from eqf_vio_amd import synth

SIZES = (1, 15, 16, 17, 33, 49, 70)   # 16: kTileLm; 15 / 17 / 33 / 49: one off the tile edges; 70: more than one 64-column ring tile
BIG = 130                             # four rows per wavefront with more than two ring columns
RAGGED = (5, 17, 33)                  # one handle, three filters
TILED = ((37, 8), (50, 16))           # (N, landmarks per block) of the partitioned filter
# The same at block sizes that reach its production paths (whole 128 x 128 product tiles, the blocked potrf, the split solve); GPU tests
# and one CPU test only -- kept out of ALL_SIZES / CPU_SIZES, whose parametrised tests keep their cost
TILED_BIG = ((200, 64), (230, 108))
KSTEP = (17, 70)
F32 = (17, 70)
ALL_SIZES = tuple(sorted(set(SIZES + (BIG,) + RAGGED + tuple(n for n, _ in TILED))))
FAMILIES = ("a", "b", "c", "d")
FAMILIES_FOUR = ("a", "b", "c")           # the bursts of four calls (d is a gap before ONE call)
GAP = 0.1
ACC_T = 0.003
ACC_W = np.array([0.02, -0.01, 0.03, 0.1, -0.2, 0.05])


def settings():
    return synth.template_settings_dict()


_PLAN = {}


def plan(N):
    """(stream, the events up to three IMU calls behind the fourth vision frame, the four IMU records after them)."""
    if N not in _PLAN:
        st = synth.make_stream(N, duration=0.3)
        ev = list(st.events())
        v4 = [i for i, (kind, k) in enumerate(ev) if kind == "vision"][3]
        head = ev[:v4 + 4]
        assert [kind for kind, _ in head[-3:]] == ["imu"] * 3
        k = head[-1][1]
        _PLAN[N] = (st, head, [st.imu[k + 1 + j].copy() for j in range(4)])
    return _PLAN[N]


def with_accumulators(snap):
    snap = dict(snap)
    snap["accumulatedTime"] = ACC_T
    snap["accumulatedVelocity"] = ACC_T * (np.asarray(snap["currentVelocity"], dtype=float) + ACC_W)
    return snap


def device_snapshot(hip, N):
    st, head, _ = plan(N)
    f = hip.FilterBatch(settings(), capacity=N + 5, batch=1)
    for kind, k in head:
        if kind == "imu":
            f.process_imu([st.imu[k, 0]], st.imu[k, 1:4], st.imu[k, 4:7])
        else:
            assert np.all(f.process_vision([st.vision_stamps[k]], st.ids, st.bearings[k]) == 0)
    snap = f.dump_state()
    assert f.device_error() == 0 and len(snap["ids"]) == N
    f.close()
    return with_accumulators(snap)


def oracle_snapshot(oracle_lib, N):
    """The same state from the C++ fp64 oracle (no GPU)."""
    st, head, _ = plan(N)
    f = oracle_lib.OracleFilter(settings())
    for kind, k in head:
        if kind == "imu":
            f.processIMUData(st.imu[k, 0], st.imu[k, 1:4], st.imu[k, 4:7])
        else:
            f.processVisionData(st.vision_stamps[k], st.ids, st.bearings[k])
    assert f.N == N
    bias = f.bias()
    return with_accumulators(dict(ids=f.ids(), origin=f.xi0(), group=f.group(), bias=bias, sigma=f.stateCovariance(), time=f.getTime(),
                                  currentVelocity=st.imu[head[-1][1], 1:7] - bias, accumulatedVelocity=np.zeros(6), accumulatedTime=0.0, initialised=1))


def _mirror(S):
    return np.triu(S) + np.triu(S, 1).T


def sigma_family(snap, fam):
    N = len(snap["ids"])
    n = 11 + 3 * N
    if fam in ("a", "d"):
        return _mirror(np.asarray(snap["sigma"], dtype=float))
    if fam == "b":
        rng = np.random.default_rng(1000 + N)
        G = rng.standard_normal((n, n + 3))
        C = G @ G.T
        s = np.sqrt(np.diag(C))
        D = 10.0 ** rng.uniform(-4, 2, n)
        return _mirror(C / s[:, None] / s[None, :] * D[:, None] * D[None, :])
    S = np.zeros((n, n))
    S[2, 9] = 1.0                                   # base x base: gyro bias z, velocity y
    i0 = min(N - 1, 15)
    S[4, 11 + 3 * i0 + 1] = -1.0                    # base x landmark
    if N >= 17:
        S[11 + 3 * 15, 11 + 3 * 16 + 2] = 1.0       # landmark 15 x landmark 16: across the tile edge (kTileLm = 16)
    m = min(N - 1, 16)
    S[11 + 3 * m:14 + 3 * m, 11 + 3 * m:14 + 3 * m] = [[1, -1, 1], [-1, 1, -1], [1, -1, 1]]
    return _mirror(S)


def one_call(snap, fam):
    """The next IMU call of the stream (family d: 0.1 s behind the state's time)."""
    r = plan(len(snap["ids"]))[2][0]
    return [(float(snap["time"]) + GAP if fam == "d" else r[0], r[1:4], r[4:7])]


def four_calls(snap):
    """A burst of four: the second call repeats the first's stamp with another sample (it integrates nothing, but its sample is the one the
    third call integrates)."""
    r = plan(len(snap["ids"]))[2]
    return [(r[0][0], r[0][1:4], r[0][4:7]), (r[0][0], r[1][1:4], r[1][4:7]), (r[2][0], r[2][1:4], r[2][4:7]), (r[3][0], r[3][1:4], r[3][4:7])]
