"""The committed cases of the pairwise merge costs (tests/test_mergecost_exact.py, tests/test_gpu_merge_costs.py) and the measured constant
K_LOG1P.

Members are mixture_cases.member(N, k), k = 0 .. 4, for N in SIZES: with first = 0 the kernels factor internal orders 12, 15, 63, 66, 129 and
258, each side of the 64-wide block column edges.  A case names six positions: the five members, member 1 once more (the same dict: a
repeated index), and position 2 with a weight of exactly 0.  unsymmetric(N) is the same case with every member's Sigma moved ABOVE its block
diagonal, where no kernel reads.  cluster_case(N) is the greedy reduction's: three well-separated members with near-copies around them --
the member's origin velocity, landmarks and bias moved by 1e-3 of the standard deviations of its own Sigma, Sigma scaled by 1 + O(1e-3) --
so that every decision of the reduction has a margin by construction (tests assert it)."""
import numpy as np

import mixture_cases as mc

SIZES = (0, 1, 17, 18, 39, 82)
FIRSTS = (0, 6, 11)
POOL = 5
IDX = (0, 1, 2, 3, 4, 1)
REF = 3  # position of the chart centre

# numpy's worst |log1p t - mp.log1p t| / (u (1 + log1p t)) over the arguments t = alpha (1 - alpha) maha of the cases below, as
# tests/test_mergecost_exact.py measures it (x86-64, glibc); K_LOG1P = 4 x that: the device's log1p is another implementation.
ORACLE_LOG1P = 0.3030377085573136
# ORACLE-END
K_LOG1P = 4 * ORACLE_LOG1P

CLUSTER_SIZES = (1, 17)
CLUSTER_SHAPE = (3, 2, 2)   # members per cluster: 7 in all
CLUSTER_TARGET = 3
MARGIN = 100.0


def weights(N):
    w = np.random.default_rng(7400 + 13 * N).uniform(0.2, 1.5, len(IDX))
    w[2] = 0.0
    return w


def pool(N):
    return [mc.member(N, k) for k in range(POOL)]


def case(N, members=None):
    """(members by position, weights, position of the centre)"""
    p = pool(N) if members is None else members
    return [p[b] for b in IDX], weights(N), REF


def unsymmetric(N):
    p = pool(N)
    blk = np.concatenate([np.zeros(11, dtype=int), 1 + np.repeat(np.arange(N), 3)])
    for k, m in enumerate(p):
        S = m["sigma"]
        m["sigma"] = S + (blk[:, None] < blk[None, :]) * S * 1e-6 * (k + 1)
    return case(N, p)


def near_copy(m, rng, rel=1e-3):
    """member m moved by `rel` of its own spread"""
    c = dict(m)
    sd = np.sqrt(np.diag(m["sigma"]))
    N = (len(sd) - 11) // 3
    c["origin"] = dict(m["origin"])
    c["origin"]["v"] = m["origin"]["v"] + rel * sd[8:11] * rng.standard_normal(3)
    c["origin"]["p"] = m["origin"]["p"] + rel * sd[11:].reshape(N, 3) * rng.standard_normal((N, 3))
    c["bias"] = m["bias"] + rel * sd[0:6] * rng.standard_normal(6)
    c["sigma"] = m["sigma"] * (1.0 + rel * rng.uniform(0.5, 1.5))
    c["estimate"] = mc.estimate_np(c["origin"], c["group"])
    return c


def cluster_case(N):
    """(members, weights): CLUSTER_SHAPE near-copies around members 0, 1, 2 of size N, interleaved"""
    rng = np.random.default_rng(8800 + N)
    ms, lab = [], []
    for k, cnt in enumerate(CLUSTER_SHAPE):
        base = mc.member(N, k)
        for c in range(cnt):
            ms.append(base if c == 0 else near_copy(base, rng))
            lab.append(k)
    order = rng.permutation(len(ms))
    w = rng.uniform(0.5, 1.5, len(ms))
    return [ms[i] for i in order], w, [lab[i] for i in order]
