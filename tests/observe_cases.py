"""TEST INFRASTRUCTURE ONLY -- the committed cases of the rows eqf_observe_landmarks forms (tests/observe_exact.py, test_observe_exact.py,
test_observe_host.py, test_gpu_observe.py): small snapshots of the part of a filter's state the rows depend on -- ids, the origin's
landmark positions p0, the group's Q_i = (q_i, a_i) -- with N = 5 and 22 landmarks, generated from a fixed seed.  The scales a_i run over
two decades (0.1 .. 10), the depths |p_hat| from 0.3 m to 300 m, and the measurements lie off the prediction by 1e-6 .. 1.2 rad (a
bearing), about 1 % (a range, a position).  Offsets: the identity, and a camera turned by 0.3 rad at a 0.1 m baseline.  One id of the
N = 22 cases is not in the state."""
import numpy as np

from eqf_vio_amd import consistency as cs

SIZES = (5, 22)
KINDS = (cs.OBS_BEARING, cs.OBS_RANGE, cs.OBS_POSITION)
ABSENT_ID = 5000
CASES = tuple((kind, cam, N) for kind in KINDS for cam in ("identity", "offset") for N in SIZES)


def _unit(v):
    return v / np.linalg.norm(v)


def camera(name):
    """None, or (q_c, t_c): 0.3 rad about a fixed axis, 0.1 m baseline"""
    if name == "identity":
        return None
    axis = _unit(np.array([0.3, -0.8, 0.5]))
    return np.concatenate([[np.cos(0.15)], np.sin(0.15) * axis]), 0.1 * _unit(np.array([0.9, 0.1, -0.4]))


def landmarks(N, seed=0):
    """dict(ids (N,), p (N, 3) = p0, Qq (N, 4), Qa (N,)) with p_hat = Q_i^-1 p0_i at depths 0.3 .. 300 m"""
    rng = np.random.default_rng(4100 + 17 * N + seed)
    Qq = np.array([_unit(rng.standard_normal(4)) for _ in range(N)])
    Qa = rng.permutation(np.logspace(-1.0, 1.0, N))
    depth = rng.permutation(np.logspace(np.log10(0.3), np.log10(300.0), N))
    p = np.zeros((N, 3))
    for i in range(N):
        p_hat = depth[i] * _unit(rng.standard_normal(3) + np.array([0.0, 0.0, 1.5]))
        p[i] = Qa[i] * cs.quat_to_matrix(Qq[i]) @ p_hat
    return dict(ids=np.arange(N, dtype=np.int32) * 3 + 100, p=p, Qq=Qq, Qa=Qa)


def state(N, seed=0):
    """what consistency.observe_rows_host and observe_exact.reference read of a dump_state dictionary"""
    lm = landmarks(N, seed)
    return dict(ids=lm["ids"], origin=dict(p=lm["p"]), group=dict(Qq=lm["Qq"], Qa=lm["Qa"]))


def entries(kind, st, cam, seed=0):
    """(ids (K,), meas (K, 3)): every landmark of the state (and ABSENT_ID when there are 22 of them), measured off the prediction"""
    N = len(st["ids"])
    rng = np.random.default_rng(977 + 31 * N + 7 * kind + seed)
    J = cs.landmark_jacobian_blocks(st["group"])
    Rc, tc = (np.eye(3), np.zeros(3)) if cam is None else (cs.quat_to_matrix(cam[0] / np.linalg.norm(cam[0])), cam[1])
    theta = rng.permutation(np.logspace(-6.0, np.log10(1.2), N))
    meas = np.zeros((N, 3))
    for i in range(N):
        pc = Rc.T @ (J[i] @ st["origin"]["p"][i] - tc)
        d = np.linalg.norm(pc)
        if kind == cs.OBS_BEARING:
            yh = pc / d
            ax = _unit(np.cross(yh, rng.standard_normal(3)))
            meas[i] = _unit(np.cos(theta[i]) * yh + np.sin(theta[i]) * np.cross(ax, yh))
        elif kind == cs.OBS_RANGE:
            meas[i, 0] = d * (1.0 + 0.01 * rng.standard_normal())
        else:
            meas[i] = pc + 0.01 * d * rng.standard_normal(3)
    ids = np.asarray(st["ids"], dtype=np.int32)
    if N == 22:
        ids, meas = np.append(ids, ABSENT_ID).astype(np.int32), np.vstack([meas, meas[0]])
    return ids, meas


def case(c, seed=0):
    """(kind, state, ids, meas, cam) of a member of CASES"""
    kind, camname, N = c
    st, cam = state(N, seed), camera(camname)
    ids, meas = entries(kind, st, cam, seed)
    return kind, st, ids, meas, cam
