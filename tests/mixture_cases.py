"""The committed cases of the moment-matched mixture (tests/test_mixture_exact.py, tests/test_gpu_mixture.py) and the measured constant K_E.

Members are variations of consistency_cases.local_state(N, theta): the origin attitude tilted by up to 0.3 rad about varying axes, origin
velocity, group velocity and bias shifted, the origin landmarks moved by a few percent; the landmark scales Q_a of the master state span
0.05 .. 20 (2.6 decades).  Every member has its own well-conditioned SPD Sigma.  n = 3 has a weight that is exactly 0, n = 5 a repeated
member (the same dict twice: a repeated index)."""
import numpy as np

import consistency_cases as cc
import lie_edge_cases as ec
from eqf_vio_amd import consistency as cs

SIZES = (0, 1, 16, 17, 33)
MEMBERS = (1, 2, 3, 5)
THETA = cc.LOCAL_THETAS[0]
MAX_TILT = 0.3

# The numpy statement's (consistency.mixture_moments_host / merge_host) worst |e - e_50digits| / (u scale) over the cases below, as
# tests/test_mixture_exact.py measures it (x86-64, glibc); K_E = 4 x ratio: the device's fused operations differ from numpy's.
ORACLE_E = 2.9921516720817407
# ORACLE-END
K_E = 4 * ORACLE_E


def estimate_np(origin, group):
    """state_estimate() of a snapshot in numpy: stateGroupAction(X, xi0) (VIOGroup.cpp:23-45)."""
    q0, Aq = np.asarray(origin["q"], dtype=float), np.asarray(group["Aq"], dtype=float)
    q = cs._quat_mul(q0, Aq)
    x = np.asarray(origin["x"], dtype=float) + cs._quat_rotate(q0, np.asarray(group["Ax"], dtype=float))
    v = cs._quat_rotate(cs._quat_inverse(Aq), np.asarray(origin["v"], dtype=float) - np.asarray(group["w"], dtype=float))
    Qq, Qa = np.asarray(group["Qq"], dtype=float).reshape(-1, 4), np.asarray(group["Qa"], dtype=float).reshape(-1)
    p0 = np.asarray(origin["p"], dtype=float).reshape(-1, 3)
    p = np.array([cs._quat_rotate(cs._quat_inverse(Qq[i]), p0[i]) / Qa[i] for i in range(len(Qa))]).reshape(-1, 3)
    return dict(q=q, x=x, v=v, p=p)


def member(N, k):
    """Member k of the case family of size N (k = 0: the master state itself)."""
    rng = np.random.default_rng(4100 + 37 * N + k)
    s = cc.local_state(N, THETA)
    o, g = s["origin"], s["group"]
    if k:
        tilt = MAX_TILT * (k % 4 + 1) / 4.0
        o["q"] = cc._qmul(o["q"], ec._quat(rng.standard_normal(3), tilt))
        o["v"] = o["v"] + 0.2 * rng.standard_normal(3)
        o["x"] = o["x"] + 0.1 * rng.standard_normal(3)
        g["w"] = g["w"] + 0.05 * rng.standard_normal(3)
        o["p"] = o["p"] * (1.0 + 0.03 * rng.standard_normal((N, 1))) + 0.02 * rng.standard_normal((N, 3))
        s["bias"] = s["bias"] + 0.01 * rng.standard_normal(6)
    S = ec._spd(11 + 3 * N, np.random.default_rng(5200 + 11 * N + k), scale=1.0 + 0.5 * k)
    s["sigma"] = np.tril(S) + np.tril(S, -1).T
    s["estimate"] = estimate_np(o, g)
    return s


def case(N, n):
    """(members, weights, ref) of the case with N landmarks and n members."""
    ms = [member(N, k) for k in range(n)]
    w = np.random.default_rng(6300 + 7 * N + n).uniform(0.2, 1.5, n)
    if n == 3:
        w[1] = 0.0
    if n == 5:
        ms[4] = ms[1]
    return ms, w, (n - 1) // 2


def cases():
    return [(N, n) for N in SIZES for n in MEMBERS]
