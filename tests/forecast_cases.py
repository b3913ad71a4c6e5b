"""TEST INFRASTRUCTURE ONLY -- the states, samples and horizons that tests/test_forecast_exact.py (CPU: the fp64 statements against the exact
reference, and the fault table) and tests/test_gpu_forecast.py (the device against the same reference) share, so that the bound is checked on
the CPU for exactly the cases the device is held to.

Every state is synthetic and cheap (no stream is run): snapshot(N) is lie_edge_cases.base_snapshot's construction at any N -- landmarks 2 .. 8 m
in front of the camera, non-trivial A and Q_i, a symmetric positive definite Sigma of diagonal + rank 6 -- with a bias, a held sample and a
velocity, in the format of FilterBatch.dump_state / restore_state.  Cases (name -> Case):
    n{N}          N = 0, 1, 63, 64, 65, 257 (lane, wavefront and workgroup edges of the landmark kernel): one sample and t1 (two steps)
    k0t, k1, k1t, k16, k16t, k17, k17t      N = 5: K samples without / with the closing step to t1 (k0t: the K = 0 forecast of a frame's stamp)
    k17t-exp      ... with the exponential velocity lift (useDiscreteVelocityLift = 0); k1t-exp likewise
    back          N = 5, five samples: the second repeats the first's stamp, the fourth lies BEFORE the state's time -- neither integrates, both
                  replace the held sample
    turn          N = 5: the held sample turns the body by 0.5 rad over the first step (lie_edge_cases' large-angle class)
    pole          N = 5: the origin's gravity direction 1e-2 rad from the pole of its chart
    graded        N = 5: Sigma = D C D with D = 10^uniform(-1, 1) per coordinate: scales over two decades"""
import numpy as np

import lie_edge_cases as ec

T0 = ec.T0
DT = 0.005
SIZES = (0, 1, 63, 64, 65, 257)
POLE_THETA = 1e-2


def snapshot(N, seed=7):
    """lie_edge_cases.base_snapshot's state at any N (the first 21 landmarks are NOT that function's: one generator call per array here)."""
    rng = np.random.default_rng(1000 * seed + N)
    M = max(N, 1)
    ang = np.deg2rad(30.0) * np.sqrt(rng.uniform(size=M))
    az = rng.uniform(0, 2 * np.pi, M)
    p = np.stack([np.sin(ang) * np.cos(az), np.sin(ang) * np.sin(az), np.cos(ang)], axis=1) * rng.uniform(2.0, 8.0, M)[:, None]
    origin = dict(q=ec._quat([0.3, 1.0, -0.2], 1.1), x=np.array([0.4, -0.7, 1.2]), v=0.2 * ec._unit([0.5, -0.3, 0.8]), p=p[:N].copy())
    Qq = np.array([ec._quat(rng.standard_normal(3), rng.uniform(0.1, 0.6)) for _ in range(M)])
    group = dict(Aq=ec._quat([-0.5, 0.2, 0.9], 2.4), Ax=np.array([0.3, 0.1, -0.2]), w=np.array([0.05, -0.08, 0.03]), Qq=Qq[:N].copy(),
                 Qa=rng.uniform(0.7, 1.4, M)[:N].copy())
    n = 11 + 3 * N
    L = 0.3 * rng.standard_normal((n, 6))
    S = np.diag(rng.uniform(0.5, 2.0, n)) + L @ L.T
    S = np.triu(S) + np.triu(S, 1).T
    return dict(ids=np.arange(10, 10 + N, dtype=np.int32), origin=origin, group=group, bias=np.array([0.01, -0.02, 0.015, 0.1, -0.05, 0.08]),
                sigma=S, time=T0, currentVelocity=np.array([0.3, -0.2, 0.25, 0.4, -0.3, 9.6]), accumulatedVelocity=np.zeros(6),
                accumulatedTime=0.0, initialised=1)


def samples(K, seed=3, t0=T0, dt=DT):
    """K IMU samples (K, 7) at t0 + dt, t0 + 2 dt, ...: rates of a gentle turn, specific force near gravity."""
    rng = np.random.default_rng(seed)
    out = np.zeros((K, 7))
    for k in range(K):
        out[k, 0] = t0 + (k + 1) * dt
        out[k, 1:4] = np.array([0.3, -0.2, 0.25]) + 0.2 * rng.standard_normal(3)
        out[k, 4:7] = np.array([0.4, -0.3, 9.6]) + 0.5 * rng.standard_normal(3)
    return out


class Case:
    def __init__(self, name, snap, imu, t1, discrete=True):
        self.name, self.snap, self.imu, self.t1, self.discrete = name, snap, np.asarray(imu, dtype=float).reshape(-1, 7), t1, discrete
        self.N = len(snap["ids"])

    def settings(self):
        return ec.settings(self.discrete)

    def after(self):
        """The stamp of the last sample (the state's time without samples) plus 3 ms: where a closing step goes."""
        return (self.imu[-1, 0] if len(self.imu) else float(self.snap["time"])) + 0.003


def _graded(snap):
    n = len(snap["sigma"])
    rng = np.random.default_rng(77)
    G = rng.standard_normal((n, n + 3))
    C = G @ G.T
    s = np.sqrt(np.diag(C))
    D = 10.0 ** rng.uniform(-1, 1, n)
    S = C / s[:, None] / s[None, :] * D[:, None] * D[None, :]
    return dict(snap, sigma=np.triu(S) + np.triu(S, 1).T)


def _turn(snap):
    w = 0.5 * ec._unit(ec.AXES["g"]) / ((T0 + DT) - T0)
    return dict(snap, currentVelocity=np.concatenate([w, snap["currentVelocity"][3:6]]))


def _pole(snap):
    o = dict(snap["origin"])
    o["q"] = ec._quat([np.cos(1.3), np.sin(1.3), 0.0], POLE_THETA)  # R^T e3 lies POLE_THETA from e3, the pole of the gravity chart
    return dict(snap, origin=o)


_CASES = {}


def cases():
    if not _CASES:
        def add(name, snap, K, with_t1, discrete=True, imu=None):
            imu = samples(K) if imu is None else imu
            c = Case(name, snap, imu, None, discrete)
            if with_t1:
                c.t1 = c.after()
            _CASES[name] = c

        for N in SIZES:
            add(f"n{N}", snapshot(N), 1, True)
        s5 = snapshot(5)
        add("k0t", s5, 0, True)
        for K in (1, 16, 17):
            add(f"k{K}", s5, K, False)
            add(f"k{K}t", s5, K, True)
        add("k1t-exp", s5, 1, True, discrete=False)
        add("k17t-exp", s5, 17, True, discrete=False)
        back = samples(5)
        back[1, 0] = back[0, 0]
        back[3, 0] = T0 - 0.002
        add("back", s5, 5, True, imu=back)
        add("turn", _turn(s5), 2, True)
        add("pole", _pole(s5), 2, True)
        add("graded", _graded(s5), 1, True)
    return _CASES


GPU_SIZES = tuple(f"n{N}" for N in SIZES)
