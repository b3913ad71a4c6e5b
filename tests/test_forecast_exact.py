"""The yardstick of tests/test_gpu_forecast.py, checked on the CPU for the cases the device is held to (tests/forecast_cases.py):

(a) the two constants tests/forecast_exact.py adds are measured here from fp64 statements, never from the device, printed and asserted:
    FC_TAU_MEASURED   the fp64 oracle's linearisation blocks (oracle/eqf_numpy.py's A0t / Bt as they sit in F) against the 50-digit blocks at
                      EVERY integrating step of every case, 17 steps from the snapshot included, in units of u max|block|
    TAU_D_MEASURED    D = (I - y y^T) / |p| as consistency.bearing_cov_host forms it in fp64 against the 50-digit D, in units of u max|D|
(b) consistency.forecast_host on the numpy filter (the dense route: K processIMUData calls and integrateUpToTime on a copy) and a numpy
    model of the kernel's order of operations (base block, panels and diagonal blocks only, upper triangles mirrored, F_bb through its
    sparsity) lie inside every bound on every case, in both charts;
(c) each of eleven injected faults lies outside a bound on at least one case -- the bounds can tell a wrong forecast from a right one."""
import copy

import numpy as np
import pytest

import forecast_cases as fcs
import forecast_exact as fx
import lie_edge_cases as ec
import riccati_exact as rx
from eqf_vio_amd import consistency as cs
from oracle import eqf_numpy as en

NAMES = ("pose_R", "pose_x", "velocity", "p", "bearing", "base", "lm", "S", "ycov")
FAULTS = ("hold_not_replaced", "bias_not_subtracted", "t1_dropped", "nonpositive_dt_integrated", "first_dt_for_all", "neighbours_panel",
          "D_transposed", "point_noise_missing", "S_without_r", "norm_squared_in_D", "present_jacobian")
_REF = {}


def reference(name, local):
    if (name, local) not in _REF:
        c = fcs.cases()[name]
        _REF[(name, local)] = fx.Reference(c.snap, c.settings(), c.imu, c.t1, local)
    return _REF[(name, local)]


def oracle_blocks(f, dt):
    """oracle/eqf_numpy.py's blocks of the step the filter is about to take, as they sit in F (riccati_exact.scaled_from_oracle), and Bt, T."""
    T = f.accumulatedTime + dt
    mean = (f.accumulatedVelocity + f.currentVelocity * dt) * (1.0 / T)
    A0t, Bt = en.eqf_state_matrix_A(f.X, f.xi0, mean), en.eqf_input_matrix_B(f.X, f.xi0)
    return rx.scaled_from_oracle(A0t, Bt, T, len(f.xi0.ids)), Bt, T


def kernel_step(sc, Bt, T, d, Sbb, Pn, Sd, fault=None):
    """One Riccati step on (Sigma_bb, panels (N, 3, 11), diagonal blocks (N, 3, 3)) in the order of csrc/eqf_forecast.hpp."""
    N = len(Sd)
    sw2, sa2, ppv = d["velOmegaVariance"], d["velAccelVariance"], d["pointProcessVariance"]
    F = np.eye(11)
    F[6:8, 0:3], F[8:11, 0:3], F[8:11, 3:6], F[8:11, 6:8] = sc["TBg"], sc["TBvw"], sc["TRA"], sc["TAvg"]
    Nb = np.zeros((11, 3))
    Nb[6:11] = Bt[0:5, 0:3]
    RA = Bt[2:5, 3:6]
    nz = sw2 * Nb @ Nb.T
    nz[8:11, 8:11] += sa2 * RA @ RA.T
    nz += np.diag([d["biasOmegaProcessVariance"]] * 3 + [d["biasAccelProcessVariance"]] * 3 + [d["gravityProcessVariance"]] * 2 + [d["velocityProcessVariance"]] * 3)
    Sn = (F @ Sbb) @ F.T + T * nz
    Sn = np.triu(Sn) + np.triu(Sn, 1).T
    Pout, Sout = np.zeros_like(Pn), np.zeros_like(Sd)
    for i in range(N):
        D, Lw, Lv = sc["D"][i], sc["Lw"][i], sc["Lv"][i]
        if fault == "D_transposed":
            D = D.T
        P = Pn[(i + 1) % N] if fault == "neighbours_panel" else Pn[i]
        G = Lw @ Sbb[0:3] + Lv @ Sbb[8:11] + D @ P
        H = D @ Sd[i] + Lw @ P[:, 0:3].T + Lv @ P[:, 8:11].T
        S = H @ D.T + (G[:, 0:3] + (sw2 / T) * Lw) @ Lw.T + G[:, 8:11] @ Lv.T
        if fault != "point_noise_missing":
            S = S + T * ppv * np.eye(3)
        Sout[i] = np.triu(S) + np.triu(S, 1).T
        Pout[i] = G @ F.T - sw2 * Lw @ Nb.T
    return Sn, Pout, Sout


def model(case, local, fault=None):
    """The kernel's recursion beside the numpy filter's group (the filter's own dense Sigma is not looked at), with one fault injected."""
    d = case.settings()
    snap = dict(case.snap)
    S0 = np.asarray(snap["sigma"], dtype=float)
    N = case.N
    snap["sigma"] = np.eye(11 + 3 * N)
    f = ec.numpy_filter(en, snap, d)
    if fault == "bias_not_subtracted":
        f.inputBias = np.zeros(6)
    f0 = copy.deepcopy(f)
    Sbb = S0[:11, :11].copy()
    Pn = np.array([S0[11 + 3 * i:14 + 3 * i, :11] for i in range(N)]).reshape(N, 3, 11)
    Sd = fx.blocks_of(S0, N).astype(float)
    calls = [(r, True) for r in case.imu] + ([(np.array([case.t1] + [0.0] * 6), False)] if case.t1 is not None and fault != "t1_dropped" else [])
    steps, first_dt = 0, None
    for r, is_imu in calls:
        dt = r[0] - f.currentTime
        if fault == "nonpositive_dt_integrated" and dt < 0:
            f.currentTime = r[0] + dt
            dt = -dt
        if f.currentTime >= 0 and dt > 0:
            first_dt = dt if first_dt is None else first_dt
            if fault == "first_dt_for_all":
                dt = first_dt
                f.currentTime = r[0] - dt
            sc, Bt, T = oracle_blocks(f, dt)
            Sbb, Pn, Sd = kernel_step(sc, Bt, T, d, Sbb, Pn, Sd, fault)
            steps += 1
        held = f.currentVelocity
        if is_imu:
            f.processIMUData(en.IMUVelocity(r[0], r[1:4], r[4:7]))
            if fault == "hold_not_replaced":
                f.currentVelocity = held
        else:
            f.integrateUpToTime(r[0])
    est = f.stateEstimate()
    Jf = f0 if fault == "present_jacobian" else f
    origin = dict(q=Jf.xi0.pose.q, x=Jf.xi0.pose.x, v=Jf.xi0.velocity, p=Jf.xi0.p)
    group = dict(Aq=Jf.X.A.q, Ax=Jf.X.A.x, w=Jf.X.w, Qq=np.array([Q.q for Q in Jf.X.Q]).reshape(N, 4), Qa=np.array([Q.a for Q in Jf.X.Q]).reshape(N))
    J = cs.local_jacobian_blocks(origin, group)
    Jb = cs.jacobian_matrix(dict(G=J["G"], RAt=J["RAt"], lm=np.zeros((0, 3, 3))))
    lmloc = np.array([J["lm"][i] @ Sd[i] @ J["lm"][i].T for i in range(N)]).reshape(N, 3, 3)
    p = np.asarray(est.p, dtype=float).reshape(N, 3)
    C = cs.output_blocks(f.xi0.p)
    r = 0.0 if fault == "S_without_r" else d["measurementVariance"]
    ycov = np.zeros((N, 3, 3))
    for i in range(N):
        n = np.linalg.norm(p[i])
        y = p[i] / n
        D = (np.eye(3) - np.outer(y, y)) / (n * n if fault == "norm_squared_in_D" else n)
        ycov[i] = D @ lmloc[i] @ D.T
    return dict(time=f.getTime(), steps=steps, pose_q=est.pose.q, pose_x=est.pose.x, velocity=est.velocity, p=p,
                bearing=p / np.linalg.norm(p, axis=1, keepdims=True) if N else p, base=Jb @ Sbb @ Jb.T if local else Sbb,
                lm=lmloc if local else Sd, S=np.array([C[i] @ Sd[i] @ C[i].T + r * np.eye(2) for i in range(N)]).reshape(N, 2, 2), ycov=ycov)


# ---- (a) -----------------------------------------------------------------------------------------------------------------------------------
def test_constants_are_measured_from_fp64_statements():
    worst_tau, where_tau, worst_d = 0.0, None, 0.0
    for name, c in fcs.cases().items():
        d = c.settings()
        fe, steps, _ = fx.walk(c.snap, d, c.imu, c.t1)
        theta0 = fx.pole_angle(fe.xi0)
        f = ec.numpy_filter(en, dict(c.snap, sigma=np.eye(11 + 3 * c.N)), d)
        k = 0
        for r, is_imu in [(r, True) for r in c.imu] + ([(np.array([c.t1] + [0.0] * 6), False)] if c.t1 is not None else []):
            dt = r[0] - f.currentTime
            if f.currentTime >= 0 and dt > 0:
                sc, _, _ = oracle_blocks(f, dt)
                units = rx.block_units(steps[k], sc)
                if theta0 < 0.3:  # the blocks built from the gravity chart are held to the pole form there (forecast_exact.step_bound), not to tau
                    mp_ = steps[k].mp
                    assert units.pop("TBg") <= ec.K_POLE["Bg"] / theta0 ** 2 / fx._mx(mp_["Bg"]), (name, k)
                    assert units.pop("TAvg") <= ec.K_POLE["Avg"] * 2 * 9.81 / theta0 ** 2 / fx._mx(mp_["Avg"]), (name, k)
                if max(units.values()) > worst_tau:
                    worst_tau, where_tau = max(units.values()), (name, k, max(units, key=units.get))
                k += 1
            if is_imu:
                f.processIMUData(en.IMUVelocity(r[0], r[1:4], r[4:7]))
            else:
                f.integrateUpToTime(r[0])
        assert k == len(steps)
        R = reference(name, True)
        for i in range(c.N):
            p = np.array([float(x) for x in R.est.p[i]])
            n = np.linalg.norm(p)
            y = p / n
            D = (np.eye(3) - np.outer(y, y)) / n
            mx = max(abs(x) for row in R.D[i] for x in row)
            err = max(abs(fx.mpf(float(D[a, b])) - R.D[i][a][b]) for a in range(3) for b in range(3))
            worst_d = max(worst_d, float(err / (fx.mpf(fx.U) * mx)))
    print(f"FC_TAU measured {worst_tau!r} units at {where_tau} (riccati_exact.TAU_MEASURED {rx.TAU_MEASURED}); TAU_D measured {worst_d!r} units")
    assert worst_tau <= 1.25 * fx.FC_TAU_MEASURED and worst_tau > fx.FC_TAU_MEASURED / 4
    assert worst_d <= 1.25 * fx.TAU_D_MEASURED and worst_d > fx.TAU_D_MEASURED / 4
    assert fx.TAU == max(rx.TAU_BLK, 10 * fx.FC_TAU_MEASURED) and fx.TAU_D == max(1.0, 10 * fx.TAU_D_MEASURED)


# ---- (b) -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fcs.cases()))
def test_the_fp64_statements_lie_inside_every_bound(name):
    c = fcs.cases()[name]
    d = c.settings()
    flt = ec.numpy_filter(en, c.snap, d)
    worst = {}
    for local in (True, False):
        R = reference(name, local)
        for what, got in (("forecast_host", cs.forecast_host(flt, c.imu, c.t1, local=local, measurement_variance=d["measurementVariance"], sample=en.IMUVelocity)),
                          ("kernel model", model(c, local))):
            assert got["steps"] == R.steps and got["time"] == R.time, (name, what)
            r = fx.ratios(got, R)
            worst[what] = max(worst.get(what, 0.0), max(r.values()))
            assert max(r.values()) <= 1.0, (name, what, local, r)
    print(f"{name}: worst ratio to the bound " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ---- (c) -----------------------------------------------------------------------------------------------------------------------------------
# the cases on which each fault is looked for (N = 5: cheap); a fault must leave a bound on at least one of them
FAULT_CASES = ("k1t", "k17t", "back", "k1t-exp")


@pytest.mark.parametrize("fault", FAULTS)
def test_every_injected_fault_leaves_a_bound(fault):
    out = {}
    for name in FAULT_CASES:
        c = fcs.cases()[name]
        for local in (True, False):
            r = fx.ratios(model(c, local, fault), reference(name, local))
            out[(name, local)] = max(r.values())
    worst = max(out.values())
    print(f"{fault}: worst ratio to the bound {worst:.3g} at {max(out, key=out.get)}")
    assert worst > 1.0, (fault, out)
