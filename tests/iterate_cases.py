"""TEST INFRASTRUCTURE ONLY -- the committed cases of the iterated landmark observation update (tests/iterate_exact.py,
test_iterate_exact.py, test_gpu_iterate.py): the shapes of tests/observe_cases.py (N = 5 and 22, the three kinds, both camera offsets)
under WIDE priors, where one linearisation is a poor approximation: each landmark's depth with a standard deviation of 0.5 .. 3 times the
depth itself (2 % of the depth sideways), a common-mode depth error that correlates the landmarks (so that Sigma_MM's off-diagonal blocks
matter), ranges 30 .. 60 % out and surveyed positions a few metres off."""
import numpy as np

import observe_cases as oc
from eqf_vio_amd import consistency as cs

CASES = oc.CASES
MAX_LIN, TOL = 16, 1e-7
# the cases whose numpy statement must show what the iteration is for (test_iterate_exact.py): a lower MAP cost and a smaller gradient than
# the one-shot update, reached in fewer than MAX_LIN linearisations
BEHAVIOUR = tuple(c for c in CASES if c[0] == cs.OBS_RANGE or (c[0] == cs.OBS_BEARING and c[1] == "identity"))


def sigma(st, seed=0):
    """(n, n): the wide prior of the module docstring in eqf_get_sigma's coordinates (the chart error eps with d p_hat = J eps)"""
    N = len(st["ids"])
    rng = np.random.default_rng(8800 + N + seed)
    J = cs.landmark_jacobian_blocks(st["group"])
    S = np.zeros((11 + 3 * N, 11 + 3 * N))
    S[:11, :11] = np.diag(np.full(11, 1e-4))
    v = np.zeros(3 * N)
    f = rng.permutation(np.linspace(0.5, 3.0, N))
    for i in range(N):
        ph = J[i] @ st["origin"]["p"][i]
        d = np.linalg.norm(ph)
        y = ph / d
        Ji = np.linalg.inv(J[i])
        C = (f[i] * d) ** 2 * np.outer(y, y) + (0.02 * d) ** 2 * (np.eye(3) - np.outer(y, y))
        S[11 + 3 * i:14 + 3 * i, 11 + 3 * i:14 + 3 * i] = Ji @ C @ Ji.T
        v[3 * i:3 * i + 3] = 0.5 * f[i] * d * (Ji @ y)
    S[11:, 11:] += np.outer(v, v)
    return np.tril(S) + np.tril(S, -1).T


def case(c, seed=0):
    """(kind, state with sigma, ids, meas, R (K, rows, rows), cam) of a member of CASES"""
    kind, st, ids, meas, cam = oc.case(c, seed)
    st = dict(st, sigma=sigma(st, seed))
    rng = np.random.default_rng(8900 + 13 * len(ids) + kind + seed)
    rows = cs.OBS_ROWS[kind]
    K = len(ids)
    R = np.zeros((K, rows, rows))
    J = cs.landmark_jacobian_blocks(st["group"])
    sid = [int(i) for i in st["ids"]]
    for k in range(K):
        i = sid.index(int(ids[k])) if int(ids[k]) in sid else 0
        d = np.linalg.norm(J[i] @ st["origin"]["p"][i])
        if kind == cs.OBS_BEARING:
            R[k] = 1e-4 * np.eye(2)
        elif kind == cs.OBS_RANGE:
            meas[k, 0] *= 1.0 + rng.uniform(0.3, 0.6)
            R[k] = (0.02 * d) ** 2
        else:
            meas[k] += rng.uniform(2.0, 5.0) * rng.standard_normal(3) / np.sqrt(3.0) + 0.4 * meas[k]
            R[k] = (0.02 * d) ** 2 * np.eye(3)
    return kind, st, ids, meas, R, cam
