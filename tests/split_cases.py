"""TEST INFRASTRUCTURE ONLY -- the committed cases of the split's exact test (split_exact.py, test_split_exact.py): covariances, rows,
shifts and shrinks, each built from a fixed seed by build().  K_SPLIT of split_exact.py is measured over exactly these.

    ill_scaled_*     Sigma = D C D with a well-conditioned correlation-like C and D spread over three decades (variances over six)
    one_landmark     a row that touches one landmark only (the depth axis of landmark 3)
    dense_positive   a dense row of one sign
    dense_mixed_*    dense rows of mixed sign: the functional's terms cancel (orders 11 to 266, the largest the device test uses)
    local_*          rows against the estimate's chart, Ht = a J, J from a group element with rotations of 2 to 3 rad (A and every Q_i)
                     and scales a_i between 1/3 and 3
Every case splits into the K = 2 and K = 3 components of consistency.split_components plus the children (0, 0), (0.7, 0), (0, 0.5),
(-1.3, 1): no shrink, no shift, and the singular end shrink = 1."""
import numpy as np

from eqf_vio_amd import consistency as cs

CASES = [
    dict(name="ill_scaled_5", seed=11, N=5, sigma="ill", row="dense_mixed"),
    dict(name="ill_scaled_21", seed=12, N=21, sigma="ill", row="dense_positive"),
    dict(name="one_landmark", seed=13, N=7, sigma="plain", row="one_landmark"),
    dict(name="one_landmark_ill", seed=14, N=7, sigma="ill", row="one_landmark"),
    dict(name="dense_positive", seed=15, N=7, sigma="plain", row="dense_positive"),
    dict(name="dense_mixed_7", seed=16, N=7, sigma="plain", row="dense_mixed"),
    dict(name="dense_mixed_21", seed=17, N=21, sigma="plain", row="dense_mixed"),
    dict(name="dense_mixed_0", seed=18, N=0, sigma="plain", row="dense_mixed"),
    dict(name="dense_mixed_85", seed=22, N=85, sigma="ill", row="dense_mixed"),  # (the largest order the device test uses)
    dict(name="local_dense", seed=19, N=7, sigma="plain", row="dense_mixed", local=True),
    dict(name="local_one_landmark", seed=20, N=7, sigma="ill", row="one_landmark", local=True),
    dict(name="local_gravity", seed=21, N=3, sigma="plain", row="gravity", local=True),
]


def children():
    """(shift, shrink): the K = 2 and K = 3 components and the edge children"""
    _, s2, k2 = cs.split_components(2, 0.8)
    _, s3, k3 = cs.split_components(3, 1.2, outer_weight=0.2)
    shift = np.concatenate([s2, s3, [0.0, 0.7, 0.0, -1.3]])
    shrink = np.concatenate([k2, k3, [0.0, 0.0, 0.5, 1.0]])
    return shift, shrink


def _unit(rng, k):
    v = rng.standard_normal(k)
    return v / np.linalg.norm(v)


def _rot_quat(rng, lo=2.0, hi=3.0):
    ang = rng.uniform(lo, hi)
    ax = _unit(rng, 3)
    return np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * ax])


def sigma(rng, n, kind):
    A = rng.standard_normal((n, n + 4))
    C = A @ A.T / (n + 4) + 0.5 * np.eye(n)
    if kind == "ill":
        d = 10.0 ** rng.uniform(-1.5, 1.5, n)
        C = C * np.outer(d, d)
    return np.tril(C) + np.tril(C, -1).T  # (bit-for-bit symmetric)


def row(rng, N, kind):
    n = 11 + 3 * N
    if kind == "one_landmark":
        return cs.depth_axis_row(rng.standard_normal(3) + [0.0, 0.0, 4.0], 3, n)
    if kind == "dense_positive":
        return np.abs(rng.standard_normal(n)) + 0.1
    if kind == "gravity":
        a = np.zeros(n)
        a[6:8] = _unit(rng, 2)
        return a
    return rng.standard_normal(n)


def jacobian(rng, N):
    origin = dict(q=_unit(rng, 4))
    group = dict(Aq=_rot_quat(rng), Qq=np.array([_rot_quat(rng) for _ in range(N)]).reshape(N, 4), Qa=3.0 ** rng.uniform(-1.0, 1.0, N))
    return cs.jacobian_matrix(cs.local_jacobian_blocks(origin, group))


def build(case):
    """(Sigma (n, n), a (n,), J (n, n) or None, shift (K,), shrink (K,))"""
    rng = np.random.default_rng(case["seed"])
    N = case["N"]
    n = 11 + 3 * N
    Sg = sigma(rng, n, case["sigma"])
    a = row(rng, N, case["row"])
    J = jacobian(rng, N) if case.get("local") else None
    shift, shrink = children()
    return Sg, a, J, shift, shrink
