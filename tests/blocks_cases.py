"""TEST INFRASTRUCTURE ONLY -- the cases tests/test_blocks_exact.py (CPU), tests/test_blocks_host.py (CPU, sanitized host program) and
tests/test_gpu_landmark_blocks.py (MI355X) share for the per-landmark block measurement update (csrc/eqf_blocks.hpp: eqf_update_landmarks), so that
every bound is checked on the CPU for the cases the device is held to.

The state is consistency_cases.local_state (theta = 0.5): A turned by 2.5 rad, Q_i random rotations and scales in [0.05, 20], so that local
blocks are mixed by every J_i.  Capacity N + 7.  The shapes sit on the kernels' edges: the order of S, m = rows * (entries that take part),
at 1, 63, 64, 66 and 129 around the 64-wide block columns of the factorisation, and the state order n = 11 + 3 N at N = 4, 43, 86 past
the first, second and fourth 64-row tile of Sigma.
    name        N   rows  entries  local  Sigma      what
    one         4   1     1        1      graded     a single range (m = 1)
    position63  43  3     21       1      own        surveyed positions, m = 63
    dense64     43  2     32       0      coupled    dense blocks in the origin chart, m = 64
    stereo66    43  2     33       1      one_small  stereo rows of a rig, every R_k correlated, m = 66
    mixed129    86  3     45       1      own        positions, one id that is not in the state and one entry beyond lm_gate: 43 take part, m = 129
    twins       4   1     2        0      twins      two near-duplicate range rows (the same row on landmark 0 and on its copy to 1e-4, landmark 1) with R 1e-10 relative
    small8      4   2     4        0      graded     correlated R_k, m = 8: also given to eqf_update_linear as dense rows
    depth3      43  1     3        1      own        three ranges, one gated
"own" is a filter's own Sigma after five vision frames of a synth stream (the CPU tests take it from the fp64 oracle, the device tests from
the device), mirrored from its lower triangle.  Residuals are standard normal times the square root of the entry's own S_kk diagonal (a
plausible innovation); the gated entries' are a hundred times that.  lm_gate = 60 where an entry is to be gated, else +inf: every d2 of an
entry that stays is below 40, of one that leaves above 1e3 (asserted by the tests: no verdict hangs on a rounding)."""
import numpy as np

import consistency_cases as cc
import linear_cases as lc

THETA = cc.NEES_THETA
CAP_EXTRA = cc.CAP_EXTRA
SIZES = (4, 43, 86)
LM_GATE = 60.0
Q_21 = np.array([0.9987502603949663, 0.0, 0.04997916927067833, 0.0])  # the rig: camera 2 turned by 0.1 rad about y ...
T_21 = np.array([0.12, 0.0, 0.005])                                     # ... 12 cm to the right
# name: (N, rows, kind, entries, local, Sigma family, R kind, absent entry or None, gated entries)
CASES = {
    "one": (4, 1, "depth", (2,), 1, "graded", "diag", None, ()),
    "position63": (43, 3, "position", tuple(range(1, 43, 2)), 1, "own", "diag", None, ()),
    "dense64": (43, 2, "dense", tuple(range(5, 37)), 0, "coupled", "diag", None, ()),
    "stereo66": (43, 2, "stereo", tuple(range(0, 33)), 1, "one_small", "corr", None, ()),
    "mixed129": (86, 3, "position", tuple(range(0, 86, 2)) + (85,), 1, "own", "corr", 20, (31,)),
    "twins": (4, 1, "same", (0, 1), 0, "twins", "tiny", None, ()),
    "small8": (4, 2, "dense", (0, 1, 2, 3), 0, "graded", "corr", None, ()),
    "depth3": (43, 1, "depth", (16, 17, 42), 1, "own", "diag", None, (1,)),
}
CPU_CASES = tuple(CASES)
ABSENT_ID = 5000


def p_hat(snap):
    """camera-frame landmark positions of the estimate: Q_i^-1 p0_i = J_i p0_i"""
    from eqf_vio_amd import consistency as cs

    J = np.asarray(cs.local_jacobian_blocks(snap["origin"], snap["group"])["lm"]).reshape(-1, 3, 3)
    return np.einsum("irc,ic->ir", J, snap["origin"]["p"])


def twins_sigma(N):
    """graded, with landmark 1's error a copy of landmark 0's plus 1e-4 of its own"""
    S = cc.nees_sigma(N, "graded")
    n = len(S)
    T = np.eye(n)
    T[14:17, 14:17] = 1e-4 * np.eye(3)
    T[14:17, 11:14] = np.eye(3)
    S = T @ S @ T.T
    return np.tril(S) + np.tril(S, -1).T


def snapshot(name, own=None):
    N, fam = CASES[name][0], CASES[name][5]
    snap = cc.local_state(N, THETA)
    snap["sigma"] = twins_sigma(N) if fam == "twins" else cc.nees_sigma(N, fam, own)
    return snap


def operands(name, snap, Sigma=None):
    """dict(rows, local, ids (K,), idx (K,: -1 absent), H (K, rows, 3), resid (K, rows), R (K, rows, rows), lm_gate, gated: entry numbers,
    absent: entry number or None) for the snapshot (Sigma: the covariance the device holds, default the snapshot's)"""
    from eqf_vio_amd import consistency as cs

    N, rows, kind, lms, local, fam, rkind, absent, gated = CASES[name]
    Sg = snap["sigma"] if Sigma is None else Sigma
    rng = np.random.default_rng([1900, N, rows, len(lms)])
    K = len(lms)
    ph = p_hat(snap)
    J = np.asarray(cs.local_jacobian_blocks(snap["origin"], snap["group"])["lm"]).reshape(-1, 3, 3)
    ids = snap["ids"][list(lms)].astype(np.int32)
    idx = np.array(lms, dtype=np.int32)
    if absent is not None:  # one id that the state does not hold: the largest, so the list stays ascending
        ids = np.concatenate([ids, [ABSENT_ID]]).astype(np.int32)
        idx = np.concatenate([idx, [-1]]).astype(np.int32)
        K += 1
    H = np.zeros((K, rows, 3))
    for k in range(K):
        i = int(idx[k]) if idx[k] >= 0 else 0
        if kind == "depth":
            H[k] = cs.depth_rows(ph[i], 1.0)[0]
        elif kind == "position":
            H[k] = np.eye(3)
        elif kind == "same":
            H[k] = np.array([[0.6, -0.48, 0.64]])
        elif kind == "stereo":
            y2 = cs.quat_to_matrix(Q_21).T @ (ph[i] - T_21)
            H[k] = cs.stereo_rows(ph[i], Q_21, T_21, y2 / np.linalg.norm(y2))[0]
        else:
            H[k] = rng.standard_normal((rows, 3))
    R = np.zeros((K, rows, rows))
    resid = np.zeros((K, rows))
    for k in range(K):
        i = int(idx[k]) if idx[k] >= 0 else 0
        Ht = H[k] @ J[i] if local else H[k]
        P = Ht @ Sg[11 + 3 * i:14 + 3 * i, 11 + 3 * i:14 + 3 * i] @ Ht.T
        d = float(np.mean(np.abs(np.diag(P)))) or 1.0
        if rkind == "diag":
            R[k] = np.diag(d * 10.0 ** np.linspace(-1.0, 0.0, rows))
        elif rkind == "tiny":
            R[k] = 1e-10 * d * np.eye(rows)
        else:
            A = rng.standard_normal((rows, rows))
            R[k] = d * (A @ A.T + 0.5 * rows * np.eye(rows)) / rows
        resid[k] = np.sqrt(np.diag(P + R[k])) * rng.standard_normal(rows) * (100.0 if k in gated else 1.0)
    return dict(rows=rows, local=local, ids=ids, idx=idx, H=H, resid=resid, R=R, lm_gate=LM_GATE if gated else np.inf, gated=tuple(gated),
                absent=(K - 1 if absent is not None else None))


def poison(R):
    """the upper triangles negated: only the lower ones may be read"""
    return np.tril(R) - np.triu(R, 1)


def own_sigma_oracle(N):
    """a filter's own Sigma after five vision frames of a synth stream, from the fp64 CPU oracle"""
    from eqf_vio_amd import synth
    from oracle import binding as ob

    st = synth.make_stream(N, duration=0.4)
    fo = ob.OracleFilter(cc.settings())
    seen = 0
    for kind, k in st.events():
        if kind == "imu":
            r = st.imu[k]
            fo.processIMUData(r[0], r[1:4], r[4:7])
        else:
            fo.processVisionData(st.vision_stamps[k], st.ids, st.bearings[k])
            seen += 1
            if seen == 5:
                break
    S = np.asarray(fo.stateCovariance(), dtype=float)
    assert S.shape == (11 + 3 * N, 11 + 3 * N)
    return S


def snapshot_of(N, fam, own=None):
    return lc.snapshot(N, fam, own)
