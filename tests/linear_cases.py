"""TEST INFRASTRUCTURE ONLY -- the cases tests/test_linear_exact.py (CPU) and tests/test_gpu_linear.py (MI355X) share for the low-rank linear
measurement update (csrc/eqf_linear.hpp: eqf_update_linear), so that every bound is checked on the CPU for the cases the device is held to.

The state is consistency_cases.local_state (theta = 0.5): A turned by 2.5 rad, Q_i random rotations and scales in [0.05, 20], so that local
rows are mixed by every block of J.  Sizes N = 0, 1, 17, 18, 39, 43, 82: internal orders 12, 15, 63, 66, 129, 141, 258 -- both sides of the
64-row tile edge, the second edge, and past one 256-lane chunk of k_lin_solve's column loop.  Capacity N + 7.
    Sigma families  consistency_cases.nees_sigma: own (a filter's own Sigma after five vision frames: the device tests supply it, the CPU
                    tests leave those cases out), graded, one_small, coupled
    m               1, 3, 15, 16
    H families      unit      unit rows at reference indices 0, 10, 11 and the last, then evenly spread ones (indices repeat when m > n)
                    dense     standard normal rows from a committed seed
                    velocity  consistency.velocity_rows (m = 3)
                    landmark  consistency.landmark_rows of the landmark that straddles the first 64-row tile edge when there is one (internal
                              rows 63..65: landmark 17), else the last (m = 3); N = 0 has none and takes dense rows
    R               diag (a graded diagonal) | dense (A A^T + m I), both scaled to the size of H Sigma H^T's diagonal so that neither S = R nor
                    S = H Sigma H^T to rounding
plan(N) is eight cases per size; the families, both charts and both kinds of R turn with the size so that every value of each is met at every
size.  resid is standard normal times the square root of S's mean diagonal (a plausible innovation)."""
import numpy as np

import consistency_cases as cc
import lie_exact as lx

SIZES = (0, 1, 17, 18, 39, 43, 82)
RAGGED = cc.NEES_RAGGED          # (0, 5, 18, 70)
RAGGED_MASK = (1, 0, 1, 1)
FAMILIES = ("own", "graded", "one_small", "coupled")
THETA = cc.NEES_THETA
CAP_EXTRA = cc.CAP_EXTRA
_SHAPES = (("unit", 16, "diag"), ("dense", 15, "dense"), ("velocity", 3, "diag"), ("landmark", 3, "dense"), ("dense", 1, "diag"),
           ("dense", 16, "dense"), ("unit", 15, "dense"), ("dense", 3, "diag"))


def plan(N):
    """[(family, local, m, hfam, rkind)]"""
    out = []
    for idx, (hfam, m, rkind) in enumerate(_SHAPES):
        if hfam == "landmark" and N == 0:
            hfam = "dense"
        fam = FAMILIES[(idx + N) % 4]
        if fam == "own" and N == 0:
            fam = "graded"  # (a filter without landmarks has run no vision update: no Sigma of its own)
        out.append((fam, (idx // 4 + idx + N) % 2, m, hfam, rkind))
    return out


def edge_landmark(N):
    return 17 if N > 17 else N - 1


def rows(N, m, hfam, seed=0):
    """H (m x (11 + 3 N)) in the reference index map"""
    from eqf_vio_amd import consistency as cs

    n = 11 + 3 * N
    if hfam == "velocity":
        return cs.velocity_rows(N)
    if hfam == "landmark":
        return cs.landmark_rows(N, edge_landmark(N))
    if hfam == "dense":
        return np.random.default_rng([1800, N, m, seed]).standard_normal((m, n))
    idx = [0, 10] + ([11] if n > 11 else []) + [n - 1]
    idx += [int(v) for v in np.linspace(1, n - 2, 16)]
    H = np.zeros((m, n))
    for k in range(m):
        H[k, idx[k] % n] = 1.0
    return H


def noise(Sigma, Ht, m, rkind, seed=0):
    """R (m x m) for the rows Ht in Sigma's own coordinates"""
    d = float(np.mean(np.abs(np.diag(Ht @ Sigma @ Ht.T)))) or 1.0
    rng = np.random.default_rng([1801, m, seed])
    if rkind == "diag":
        return np.diag(d * 10.0 ** np.linspace(-2.0, 0.0, m))
    A = rng.standard_normal((m, m))
    return d * (A @ A.T + m * np.eye(m)) / m


def residual(Sigma, Ht, R, seed=0):
    m = Ht.shape[0]
    s = float(np.mean(np.abs(np.diag(Ht @ Sigma @ Ht.T + R))))
    return np.sqrt(s) * np.random.default_rng([1802, m, seed]).standard_normal(m)


def snapshot(N, fam, own=None):
    snap = cc.local_state(N, THETA)
    snap["sigma"] = cc.nees_sigma(N, fam, own)
    return snap


# ---- sign and chart: a truth drawn around the estimate, a measurement of it, and what the update has to do to the measured error -------------
def _cs():
    from eqf_vio_amd import consistency

    return consistency


def estimate_of(origin, group, d):
    """the estimate phi_X(xi0) as the dict of FilterBatch.state_estimate(), through the 50-digit group action"""
    xi0 = lx.State.from_dict(origin, d["cameraOffset_q"], d["cameraOffset_x"])
    est = lx.state_group_action(lx.Group.from_dict(group), xi0)
    R = np.array([[float(v) for v in row] for row in est.R])
    return dict(q=_cs()._quat_from_matrix(R), x=np.array([float(v) for v in est.x]), v=np.array([float(v) for v in est.v]),
                p=np.array([[float(v) for v in p] for p in est.p]).reshape(-1, 3))


def group_dict(X):
    return dict(Aq=_cs()._quat_from_matrix(np.array([[float(v) for v in row] for row in X.AR])), Ax=np.array([float(v) for v in X.Ax]),
                w=np.array([float(v) for v in X.w]),
                Qq=np.array([_cs()._quat_from_matrix(np.array([[float(v) for v in row] for row in Q[0]])) for Q in X.Q]).reshape(-1, 4),
                Qa=np.array([float(Q[1]) for Q in X.Q]))


def sign_and_chart_case(N, what, seed, scale=1e-3):
    """(snapshot with an SPD Sigma, H, resid, R, truth, estimate, measured slice of the error vector)"""
    snap = cc.local_state(N, THETA)
    snap["sigma"] = cc.local_spd(N)
    d = cc.settings()
    est = estimate_of(snap["origin"], snap["group"], d)
    J = _cs().jacobian_matrix(_cs().local_jacobian_blocks(snap["origin"], snap["group"]))
    Sl = J @ snap["sigma"] @ J.T
    eps = scale * (np.linalg.cholesky(Sl) @ np.random.default_rng([1803, N, seed]).standard_normal(len(Sl)))
    truth = _cs().local_retract(est, eps, bias=snap["bias"])
    if what == "velocity":
        H, sl = _cs().velocity_rows(N), slice(8, 11)
        resid = truth["v"] - est["v"]
    else:
        i = edge_landmark(N)
        H, sl = _cs().landmark_rows(N, i), slice(11 + 3 * i, 14 + 3 * i)
        resid = truth["p"][i] - est["p"][i]
    R = 1e-3 * float(np.linalg.eigvalsh(Sl[sl, sl]).min()) * np.eye(3)
    return snap, H, resid, R, truth, est, sl, J


def measured_error(est, truth, bias, true_bias, sl):
    return _cs().error_vector(_cs().local_error(est, truth, bias, true_bias))[sl]
