"""The edge inputs of tests/test_lie_exact.py (CPU: the numpy oracle against the mpmath reference -- the yardstick) and of
tests/test_gpu_lie_edges.py (the device against the same reference), and the constants K of the bound forms.

Everything here is deterministic and cheap; the snapshots have the format of FilterBatch.dump_state / restore_state.

THE CONSTANTS K.  For each bound form K is 4 x the worst ratio the NUMPY ORACLE (oracle/eqf_numpy.py: the reference's
formulas in plain fp64, libm sin / cos, no FMA) shows against tests/lie_exact.py over the very inputs below; the factor 4 is the allowance for
the device's FMA contraction and its own sin / cos.  tests/test_lie_exact.py recomputes the oracle's ratios on every run and asserts
4 x ratio <= K (K is not rounded), so a K cannot drift away from its yardstick; the device's own ratio is never the yardstick."""
import numpy as np

from eqf_vio_amd import synth

THETAS = (0.4999, 0.5, 0.5001, 1.0, 2.2, 3.0, 3.3)
AXES = {"x": np.array([1.0, 0.0, 0.0]), "y": np.array([0.0, 1.0, 0.0]), "z": np.array([0.0, 0.0, 1.0]),
        "g": np.array([0.36, -0.48, 0.8])}
DTS = (0.005, 0.5)
NS = (5, 21)
T0 = 1.0

POLE_THETAS = (0.5, 0.1, 1e-2, 1e-3, 3e-4, 2e-4)
POLE_AZIMUTHS = (0.0, 1.3, 2.5132741228718345, 3.9, 5.4)
POLE_DEPTHS = (1.0, 10.0)
FLAG_THETAS = (0.0, 1e-5, 1e-4)

# Bound forms  K u (1 + magnitude)  of the state after one group step, per quantity and velocity lift (True: discrete), and after one
# X <- Delta X per innovation mode; bound form  K (u / theta^2) scale  near the chart pole.  Oracle ratios: see the table in DESIGN.md section 5.
# The group step's K come in two classes of the step's rotation angle, split by a known cause: at theta >= 3.0 the discrete lift's
# SO3FromVectors(q1, q) has 1 + c ~ 0.01 and loses u / (1 + c) (the reference's own formula), which would otherwise set every K.
ANGLE_CLASSES = ("to2.2", "near_pi")


def angle_class(theta):
    return "near_pi" if theta >= 3.0 else "to2.2"


# The numpy oracle's worst ratios as tests/test_lie_exact.py measures them (x86-64, glibc), to the last digit, and K = 4 x ratio with no
# rounding: a device figure between 4 x ratio and a rounded-up K would pass by the rounding alone.
ORACLE_STEP = {
    True: {  # discrete velocity lift
        "to2.2": {"A.R": 0.8509850592534548, "A.x": 0.3856152506649245, "w": 4.896051556624047, "Q.R": 11.180723056200556, "Q.a": 3.510240341976509, "est.R": 0.897884474958592, "est.x": 0.5690352612121031, "est.v": 4.734621433907131, "est.p": 22.68588146077722},
        "near_pi": {"A.R": 1.5727934100072998, "A.x": 0.3055867399283866, "w": 5.807985982641051, "Q.R": 35.31555174771253, "Q.a": 3.973290146432208, "est.R": 1.5802655683961373, "est.x": 0.5287423919979198, "est.v": 9.728843555170775, "est.p": 316.5464386661664},
    },
    False: {  # exponential of the lifted velocity
        "to2.2": {"A.R": 0.8509850592534548, "A.x": 0.3856152506649245, "w": 6.91935240481778, "Q.R": 4.702698944499128, "Q.a": 0.9823857624704284, "est.R": 0.897884474958592, "est.x": 0.5690352612121031, "est.v": 5.2737533981393865, "est.p": 12.132697101424013},
        "near_pi": {"A.R": 1.5727934100072998, "A.x": 0.3055867399283866, "w": 6.056110376654938, "Q.R": 5.968690548992942, "Q.a": 0.8654127509998002, "est.R": 1.5802655683961373, "est.x": 0.5287423919979198, "est.v": 12.258599908536908, "est.p": 16.83106390761604},
    },
}
ORACLE_INNOVATION = {"A.R": 2.7965320422490265, "A.x": 1.538723722592491, "w": 0.7786780998970408, "Q.R": 1.1335399593957327, "Q.a": 1.6831420837152693}
ORACLE_POLE = {"C0": 1.0705401808364519, "delta": 0.45372131516914854, "Bg": 0.506962644904864, "Avg": 1.9773596722957205, "G": 1.0}
# ORACLE-END
K_STEP = {lift: {c: {k: 4 * v for k, v in r.items()} for c, r in cl.items()} for lift, cl in ORACLE_STEP.items()}
K_INNOVATION = {k: 4 * v for k, v in ORACLE_INNOVATION.items()}  # one K per quantity for the three innovation modes (the worst of the three)
K_POLE = {k: 4 * v for k, v in ORACLE_POLE.items()}  # K (u / theta^2) scale; scale: C0 1/|p|, delta 1, Bg 1, Avg 2 g, G 2


def settings(discrete_velocity=True, **kw):
    d = synth.template_settings_dict()
    d["useDiscreteVelocityLift"] = bool(discrete_velocity)
    d.update(kw)
    return d


def _unit(v):
    v = np.asarray(v, dtype=float)
    return v / np.linalg.norm(v)


def _quat(axis, angle):
    a = _unit(axis)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * a])


def rotate(axis, angle, v):
    """v rotated by angle about axis (Rodrigues, fp64: only used to MAKE inputs)."""
    a, v = _unit(axis), np.asarray(v, dtype=float)
    return v * np.cos(angle) + np.cross(a, v) * np.sin(angle) + a * (a @ v) * (1 - np.cos(angle))


def _spd(n, rng, scale=1.0):
    L = 0.3 * rng.standard_normal((n, 6))
    return scale * (np.diag(rng.uniform(0.5, 2.0, n)) + L @ L.T)


def base_snapshot(N=21, seed=7, sigma_scale=1.0):
    """A state with non-trivial A and Q_i: 21 landmarks 2 .. 8 m in front of the camera; the N = 5 state is its first five landmarks
    (so one reference serves both sizes).  Velocities are small (0.2 m/s): over dt = 0.5 a landmark moves by < 0.05 rad on top of the
    rotation, so SO3FromVectors(q1, q) of the discrete lift stays > 0.09 rad away from antipodal at theta = 3.0 and 3.3."""
    rng = np.random.default_rng(seed)
    M = 21
    ang = np.deg2rad(30.0) * np.sqrt(rng.uniform(size=M))
    az = rng.uniform(0, 2 * np.pi, M)
    p = np.stack([np.sin(ang) * np.cos(az), np.sin(ang) * np.sin(az), np.cos(ang)], axis=1) * rng.uniform(2.0, 8.0, M)[:, None]
    origin = dict(q=_quat([0.3, 1.0, -0.2], 1.1), x=np.array([0.4, -0.7, 1.2]), v=0.2 * _unit([0.5, -0.3, 0.8]), p=p[:N].copy())
    Qq = np.array([_quat(rng.standard_normal(3), rng.uniform(0.1, 0.6)) for _ in range(M)])
    group = dict(Aq=_quat([-0.5, 0.2, 0.9], 2.4), Ax=np.array([0.3, 0.1, -0.2]), w=np.array([0.05, -0.08, 0.03]), Qq=Qq[:N].copy(),
                 Qa=rng.uniform(0.7, 1.4, M)[:N].copy())
    S = _spd(11 + 3 * M, rng, sigma_scale)[: 11 + 3 * N, : 11 + 3 * N].copy()
    return dict(ids=np.arange(10, 10 + N, dtype=np.int32), origin=origin, group=group, bias=np.zeros(6), sigma=S, time=T0,
                currentVelocity=np.zeros(6), accumulatedVelocity=np.zeros(6), accumulatedTime=0.0, initialised=1)


def propagate_cases():
    """[(name, theta, axis, dt)]: omega * dt = theta * axis."""
    return [(f"th{th}-{an}-dt{dt}", th, ax, dt) for dt in DTS for th in THETAS for an, ax in AXES.items()]


def propagate_snapshot(theta, axis, dt, N):
    """(snapshot, stamp): currentVelocity rotates by theta about axis over dt = stamp - T0 (dt is that difference, an exact double)."""
    snap = base_snapshot(N)
    stamp = T0 + dt
    snap["currentVelocity"] = np.concatenate([theta * _unit(axis) / (stamp - T0), case_accel(theta, axis, dt)])
    return snap, stamp


def case_accel(theta, axis, dt):
    """The accelerometer half of a case's currentVelocity: its own for every case (8.5 .. 11 m/s^2 in a seeded random direction), so that the
    yardstick of X.w -- w + R_A dt (-a + g eta), a cancellation that depends on a -- is the worst of 56 samples and not one sample's luck."""
    rng = np.random.default_rng([int(round(theta * 1e4)), int(round(1e3 * abs(axis[0]) + 1e2 * abs(axis[1]) + 10 * abs(axis[2]))), int(dt > 0.1)])
    return rng.uniform(8.5, 11.0) * _unit(rng.standard_normal(3))


def pole_directions(thetas=POLE_THETAS):
    """Unit vectors at angle theta from the optical axis e3 (where -y0 -> e3 is the half turn), at five azimuths: [(theta, azimuth, y)]."""
    return [(th, az, np.array([np.sin(th) * np.cos(az), np.sin(th) * np.sin(az), np.cos(th)])) for th in thetas for az in POLE_AZIMUTHS]


def pole_landmarks(thetas=POLE_THETAS):
    """[(theta, p0)] for every direction and both depths."""
    return [(th, d * y) for th, _, y in pole_directions(thetas) for d in POLE_DEPTHS]


def pole_snapshot(thetas=POLE_THETAS, extra=None):
    """A state whose origin landmarks are pole_landmarks(thetas) (+ `extra` benign ones in front); identity Q_i would make the residual test
    trivial, so Q_i are small rotations."""
    lm = [p for _, p in pole_landmarks(thetas)]
    if extra is not None:
        lm = list(extra) + lm
    N = len(lm)
    rng = np.random.default_rng(11)
    snap = base_snapshot(5)
    snap["ids"] = np.arange(10, 10 + N, dtype=np.int32)
    snap["origin"]["p"] = np.array(lm)
    snap["group"]["Qq"] = np.array([_quat(rng.standard_normal(3), rng.uniform(0.05, 0.2)) for _ in range(N)])
    snap["group"]["Qa"] = rng.uniform(0.8, 1.25, N)
    snap["sigma"] = _spd(11 + 3 * N, rng)
    return snap


def tilted_accel(theta, az):
    """A first accelerometer sample whose direction is theta away from level (+z), azimuth az."""
    return 9.81 * np.array([np.sin(theta) * np.cos(az), np.sin(theta) * np.sin(az), np.cos(theta)])


def numpy_settings(en, d):
    s = en.Settings(**{k: v for k, v in d.items() if not k.startswith("cameraOffset")})
    s.cameraOffset = en.SE3(d["cameraOffset_q"], d["cameraOffset_x"])
    return s


def numpy_filter(en, snap, d):
    """oracle/eqf_numpy.py's VIOFilter carrying a snapshot (en: the module)."""
    s = numpy_settings(en, d)
    f = en.VIOFilter(s)
    o, g = snap["origin"], snap["group"]
    N = len(snap["ids"])
    f.xi0 = en.VIOState(en.SE3(o["q"], o["x"]), o["v"], np.asarray(o["p"]).reshape(N, 3), snap["ids"], s.cameraOffset.copy())
    f.X = en.VIOGroup(en.SE3(g["Aq"], g["Ax"]), g["w"], [en.SOT3(q, a) for q, a in zip(np.asarray(g["Qq"]).reshape(N, 4), g["Qa"])], snap["ids"])
    f.Sigma = np.array(snap["sigma"], dtype=float)
    f.inputBias = np.array(snap["bias"], dtype=float)
    f.currentTime = float(snap["time"])
    cv, av = snap["currentVelocity"], snap["accumulatedVelocity"]
    f.currentVelocity = en.IMUVelocity(0.0, cv[0:3], cv[3:6])
    f.accumulatedVelocity = en.IMUVelocity(0.0, av[0:3], av[3:6])
    f.accumulatedTime = float(snap["accumulatedTime"])
    f.initialisedFlag = bool(snap["initialised"])
    return f


INNOVATION_MODES = {"discrete": dict(useInnovationLift=True, useDiscreteInnovationLift=True),
                    "continuous": dict(useInnovationLift=True, useDiscreteInnovationLift=False),
                    "nolift": dict(useInnovationLift=False, useDiscreteInnovationLift=False)}
# (N, scale of Sigma): chosen on the CPU with the numpy oracle so that its |dU_omega| is 1.2 .. 1.5 rad in all three modes (inside 0.6 .. 2)
# and its largest |gamma_q| / |q_i| is 0.64 (>= 0.5); nearest SO3FromVectors(q + gamma_q, q) of the discrete lift: 1 + c = 1.8
INNOVATION_STATES = ((5, 100.0), (21, 1.0))
INNOVATION_STAMP = T0 + 0.005


def innovation_case(en, N, sigma_scale, mode):
    """(settings, snapshot, bearings): the bearings the snapshot's estimate predicts, all rotated by 0.6 rad about (0.5, 0.5, 0.7)."""
    d = settings(True, **INNOVATION_MODES[mode])
    snap = base_snapshot(N, sigma_scale=sigma_scale)
    yhat = en.measure_system_state(numpy_filter(en, snap, d).stateEstimate())
    a, ang = _unit([0.5, 0.5, 0.7]), 0.6
    y = np.array([v * np.cos(ang) + np.cross(a, v) * np.sin(ang) + a * (a @ v) * (1 - np.cos(ang)) for v in yhat])
    return d, snap, y / np.linalg.norm(y, axis=1, keepdims=True)


def antipodal_innovation_case(en, alpha=3e4, s=3.0, i=2, var=1e5):
    """(settings, snapshot, bearings) whose discrete innovation lift meets SO3FromVectors(q_i + gamma_q, q_i) at the antipode, chosen on the
    CPU: landmark i has the variance `var` along r + t / alpha (r radial, t tangential; 1e-6 elsewhere) and the measurement variance is 1e-12,
    so a tangential residual of (1 + s) |C t| |q| / alpha gives gamma_q = -(1 + s)(q + |q| t / alpha), and q + gamma_q lies (1 + 1/s) / alpha
    rad from -q: the numpy oracle has 1 + c = 1.2e-9 there (a factor 8 inside the 1e-8 threshold) and throws.  The state rests
    (v = w = omega = 0, Q_i = 1), so the Riccati step before the update leaves the direction of the landmark's block alone."""
    d = settings(True, measurementVariance=1e-12, **INNOVATION_MODES["discrete"])
    snap = base_snapshot(5)
    N = 5
    snap["origin"]["v"] = np.zeros(3)
    snap["group"]["w"] = np.zeros(3)
    snap["group"]["Qq"] = np.tile([1.0, 0.0, 0.0, 0.0], (N, 1))
    snap["group"]["Qa"] = np.ones(N)
    snap["currentVelocity"] = np.concatenate([np.zeros(3), [0.0, -9.81, 0.0]])
    q = snap["origin"]["p"][i]
    r = _unit(q)
    t = _unit(np.cross(r, [0.3, -0.8, 0.5]))
    v = _unit(r + t / alpha)
    S = 1e-6 * np.eye(11 + 3 * N)
    S[11 + 3 * i:14 + 3 * i, 11 + 3 * i:14 + 3 * i] += var * np.outer(v, v)
    snap["sigma"] = S
    y = en.measure_system_state(numpy_filter(en, snap, d).stateEstimate())
    st = en.VIOState(p=[q], ids=[1])
    Ct = np.linalg.norm(en.eqf_output_matrix_C(st)[:, 5:8] @ t)
    y[i] = _unit(rotate(np.cross(r, t), -(1 + s) * Ct * np.linalg.norm(q) / alpha * 2.0, y[i]))
    return d, snap, y


def innovation_parts(last, mode, N):
    """(dU, gamma_g, gamma_v, gamma_q) of a last_update() dictionary: from Gamma in the lift modes, from gamma without the lift."""
    if mode == "nolift":
        g = np.asarray(last["gamma"])[6:]
        return None, g[0:2], g[2:5], g[5:5 + 3 * N].reshape(N, 3)
    G = np.asarray(last["Gamma"])
    return G[0:6], None, G[6:9], G[9:9 + 3 * N].reshape(N, 3)


def numpy_group(f):
    X = f.X
    return dict(Aq=X.A.q.copy(), Ax=X.A.x.copy(), w=X.w.copy(), Qq=np.array([Q.q for Q in X.Q]).reshape(-1, 4), Qa=np.array([Q.a for Q in X.Q]))


def numpy_estimate(f):
    e = f.stateEstimate()
    return dict(q=e.pose.q.copy(), x=e.pose.x.copy(), v=e.velocity.copy(), p=e.p.copy())
