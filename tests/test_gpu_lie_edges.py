"""The O(N) geometric state on the device -- X.A, X.w, X.Q_i, the chart constants C0i / R_s / cDiff / cInv, the residual -- where
synth.make_stream never takes it: rotations of 0.4999 .. 3.3 rad in ONE step (the closed-form half of expCoefficients, the seam at
theta^2 = 0.25, all four branches of m2q), innovations of more than a radian, origin landmarks and a first accelerometer sample down to
2e-4 rad from the chart pole, and the singularity bits of eqf_device_error by value.  Public API only: restore_state, one call, the getters.

The reference is tests/lie_exact.py (mpmath, 50 digits, from the definitions).  Bound forms K u (1 + magnitude) and K (u / theta^2) scale;
every K (tests/lie_edge_cases.py) is 4 x the worst ratio of the NUMPY ORACLE against the same reference on the same inputs, measured and
asserted by tests/test_lie_exact.py on the CPU -- never the device's own number.  Figures of one run on an MI355X, worst ratio of the device
(every launch path) next to the oracle's, are in DESIGN.md section 5; each test prints its own before it asserts.  That run, device | oracle,
theta <= 2.2 / theta >= 3.0:
    discrete lift     A.R 0.85/1.93|0.85/1.57  A.x 0.45/0.42|0.39/0.31  w 6.69/8.37|4.90/5.81  Q.R 11.3/37.6|11.2/35.3  Q.a 2.11/3.30|3.51/3.97
                      est.R 1.12/1.97|0.90/1.58  est.x 0.72/0.55|0.57/0.53  est.v 11.9/7.61|4.73/9.73  est.p 20.2/173|22.7/317
    exponential lift  A.R 0.85/1.93|0.85/1.57  A.x 0.45/0.42|0.39/0.31  w 5.64/5.00|6.92/6.06  Q.R 3.95/5.84|4.70/5.97  Q.a 1.00/0.84|0.98/0.87
                      est.R 1.12/1.97|0.90/1.58  est.x 0.72/0.55|0.57/0.53  est.v 7.88/6.89|5.27/12.3  est.p 13.8/16.8|12.1/16.8
    X <- Delta X                  A.R 5.69|2.80  A.x 2.78|1.54  w 1.50|0.78  Q.R 0.92|1.13  Q.a 1.35|1.68
    near the pole [u/theta^2]     C0 1.50|1.07  residual 0.60|0.45  Bg 1.71|0.51  Avg 3.37|1.98  G 1.25|1.00
    Sigma after the step against the dense oracle 3.2e-16, pose 3.3e-16, landmarks 2.3e-13; nothing outside 4 x the oracle.
    Run time: 3.7 .. 5.6 s per parametrisation of the group-step test, 18.5 s for the file.

Not reached through a host build (tests/test_lie_exact.py (c)) and therefore only here: se3ExpParts of the burst kernels, stepLandmark /
stepGlobal, landmarkConstants, the inlined exponential of the partitioned filter's per-rank step."""
import numpy as np
import pytest

import lie_edge_cases as ec
import lie_exact as lx
from helpers import rel_fro

pytestmark = pytest.mark.gpu

CAP = 21
# (name, environment at eqf_create, dense backend, filters in the handle); "burst": the family the existing tests hold bit for bit
PATHS = [
    ("default", {}, False, 1, "burst"),
    ("fused0", {"EQF_BURST_FUSED": "0"}, False, 1, "burst"),
    ("fused1", {"EQF_BURST_FUSED": "1"}, False, 1, "burst"),
    ("rows1", {"EQF_BURST_ROWS": "1"}, False, 1, "burst"),
    ("rows2", {"EQF_BURST_ROWS": "2"}, False, 1, "burst"),
    ("rows4", {"EQF_BURST_ROWS": "4"}, False, 1, "burst"),
    ("two", {}, False, 2, "burst"),
    ("noburst", {"EQF_IMU_BURST": "0"}, False, 1, "single"),
    ("noburst-fused", {"EQF_IMU_BURST": "0", "EQF_SPLIT_PROPAGATE": "0"}, False, 1, "single"),
    ("split", {"EQF_IMU_BURST": "0", "EQF_SPLIT_PROPAGATE": "1"}, False, 1, "single"),
    ("dense", {}, True, 1, "single"),
]
ENV_KEYS = ("EQF_BURST_FUSED", "EQF_BURST_ROWS", "EQF_IMU_BURST", "EQF_SPLIT_PROPAGATE")


@pytest.fixture(scope="module")
def hip():
    from eqf_vio_amd import binding

    return binding


def make_handle(hip, monkeypatch, d, env, dense=False, batch=1, capacity=CAP):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    f = hip.FilterBatch(d, capacity=capacity, batch=batch)
    if dense:
        f.set_dense_propagate(True)
    for k in env:
        monkeypatch.delenv(k)
    return f


_REF = {}


def step_reference(oracle_lib, name, th, ax, dt, discrete):
    """Per case and lift, once for the whole module: the mpmath reference of the N = 21 step (its first five landmarks are the N = 5 case) and
    the dense C++ oracle's Sigma / estimate after the same processIMUData, for both sizes."""
    key = (name, discrete)
    if key not in _REF:
        d = ec.settings(discrete)
        snap, stamp = ec.propagate_snapshot(th, ax, dt, 21)
        X, est = lx.reference_step(snap, stamp, d)
        ora = {}
        for N in ec.NS:
            sn, _ = ec.propagate_snapshot(th, ax, dt, N)
            fo = oracle_lib.OracleFilter(d)
            fo.set_state(sn)
            fo.processIMUData(stamp, IMU_W, IMU_A)
            ora[N] = (fo.stateCovariance(), fo.stateEstimate())
        _REF[key] = (X, est, ora)
    return _REF[key]


IMU_W, IMU_A = np.array([0.1, -0.2, 0.05]), np.array([0.3, -9.7, 0.9])  # the NEXT sample: it only becomes currentVelocity


@pytest.mark.parametrize("kind", ["imu", "vision"])
@pytest.mark.parametrize("discrete", [True, False])
def test_one_group_step_at_large_angles_on_every_launch_path(oracle_lib, hip, monkeypatch, discrete, kind):
    """omega dt = theta axis for theta in 0.4999 .. 3.3 about x, y, z and a general axis, dt = 0.005 and 0.5, N = 5 and 21 (ragged for the
    burst's 8-landmark builder), both velocity lifts; one process_imu, or the integrateUpToTime of one process_vision whose update is switched
    off by a measurement variance of 1e30 (gain 1e-30: Delta is the identity to the last bit but for crs(o, o) under FMA, <= u/2).
    A, w, Q_i and the estimate against the reference within K u (1 + magnitude) on every path; Sigma and the estimate against the dense oracle
    at the gates of test_single_propagate_and_single_update_from_an_injected_state (1e-12; 1e-13 pose, 1e-12 landmarks); the burst family
    bit for bit among itself, every path within 1e-9 of the default one -- what the existing tests claim on benign input."""
    d = ec.settings(discrete, **({"measurementVariance": 1e30} if kind == "vision" else {}))
    cases = ec.propagate_cases()
    out, worst, worst_gate, bad, shapes = {}, {}, {"S": 0.0, "pose": 0.0, "p": 0.0}, [], {}
    for pname, env, dense, B, family in PATHS:
        fg = make_handle(hip, monkeypatch, d, env, dense, B)
        res = out[pname] = {}
        for ci, (name, th, ax, dt) in enumerate(cases):
            X21, est21, ora = step_reference(oracle_lib, name, th, ax, dt, discrete)
            Kc = ec.K_STEP[discrete][ec.angle_class(th)]
            for N in ec.NS:
                snap, stamp = ec.propagate_snapshot(th, ax, dt, N)
                X, est = lx.prefix(X21, est21, N)
                fg.restore_state(snap, 0)
                if B == 2:  # the neighbour carries another case of the list
                    o_name, o_th, o_ax, o_dt = cases[(ci + 9) % len(cases)]
                    fg.restore_state(ec.propagate_snapshot(o_th, o_ax, dt, N)[0], 1)
                if kind == "imu":
                    fg.process_imu([stamp], IMU_W, IMU_A)
                else:
                    y = lx.to_np([lx.unit(p) for p in est.p])
                    st = fg.process_vision([stamp], snap["ids"], y)
                    assert np.all(st == 0), st
                g, e, S = fg.group(0), fg.state_estimate(0), fg.sigma(0)
                res[(name, N)] = (g, e, S)
                for k, v in lx.group_ratios(g, X, e, est).items():
                    if v > worst.get((ec.angle_class(th), k), (0.0,))[0]:
                        worst[(ec.angle_class(th), k)] = (v, pname, name, N)
                    if not v <= Kc[k]:
                        bad.append((pname, name, N, k, round(v, 2), Kc[k]))
                So, eo = ora[N]
                gate = {"S": rel_fro(S, So), "pose": max(np.abs(e["x"] - eo["x"]).max(), np.abs(e["q"] - eo["q"]).max()), "p": np.abs(e["p"] - eo["p"]).max()}
                for k, v in gate.items():
                    worst_gate[k] = max(worst_gate[k], float(v))
                if not (gate["S"] < 1e-12 and gate["pose"] < 1e-13 and gate["p"] < 1e-12):
                    bad.append((pname, name, N, "oracle gates", gate))
        assert fg.device_error() == 0, pname
        if family == "burst":  # the path ran the launch it is named after
            shape = fg.launch_shape()
            if pname.startswith("fused"):
                assert shape["fused"] == (pname == "fused1"), (pname, shape)
            if pname.startswith("rows"):
                assert shape["rows_per_wave"] == int(pname[4:]), (pname, shape)
            shapes[pname] = (shape["fused"], shape["rows_per_wave"], shape["builder_landmarks"])
    print(f"burst launch shapes (fused, rows per wave, builder landmarks): {shapes}")
    print(f"device, group step, {'discrete' if discrete else 'exponential'} lift, {kind}: worst ratio to u (1 + magnitude) over {len(PATHS)} paths")
    for (c, k), v in sorted(worst.items()):
        print(f"    {c:8s} {k:6s} {v[0]:8.2f}  (K {ec.K_STEP[discrete][c][k]:8.2f})  on {v[1]} at {v[2]} N = {v[3]}")
    print(f"    against the dense oracle: Sigma {worst_gate['S']:.2e}, pose {worst_gate['pose']:.2e}, landmarks {worst_gate['p']:.2e}")
    # the launch paths among themselves
    ref = out["default"]
    for pname, _, _, _, family in PATHS[1:]:
        for key, (g, e, S) in out[pname].items():
            g0, e0, S0 = ref[key]
            if family == "burst":
                same = np.array_equal(S, S0) and (pname.startswith("rows") or all(np.array_equal(g[k], g0[k]) for k in g0))
                if not same:
                    bad.append((pname, key, "not bit for bit with the default burst"))
            if not (rel_fro(S, S0) < 1e-9 and all(np.abs(e[k] - e0[k]).max() < 1e-9 for k in e0)):
                bad.append((pname, key, "more than 1e-9 from the default path"))
    assert not bad, bad[:20]


def test_one_group_step_at_large_angles_in_the_partitioned_filter(oracle_lib):
    """The same step through TiledFilter (1 x 1 grid, blocks of 8 landmarks: N = 21 is ragged), whose per-rank step carries its own copy
    of the exponential, by the snapshot-restart route: theta = 3.0 about the general axis and 0.5001 about y, both lifts."""
    from eqf_vio_amd import tiled

    worst, bad = {}, []
    for discrete in (True, False):
        d = ec.settings(discrete)
        for name, th, ax, dt in [c for c in ec.propagate_cases() if c[0] in ("th3.0-g-dt0.005", "th0.5001-y-dt0.5")]:
            X, est, ora = step_reference(oracle_lib, name, th, ax, dt, discrete)
            snap, stamp = ec.propagate_snapshot(th, ax, dt, 21)
            be = tiled.HipBackend(d, capacity=CAP)
            tf = tiled.TiledFilter(tiled.ProcessGrid(None, 1, 1, device=be.device), be, 8)
            tf.initialise_from(snap)
            tf.processIMUData(stamp, IMU_W, IMU_A)
            e = tf.stateEstimate()
            S = tf.stateCovariance()
            for k, v in lx.group_ratios(be.group(), X, e, est).items():
                worst[k] = max(worst.get(k, 0.0), v)
                if not v <= ec.K_STEP[discrete][ec.angle_class(th)][k]:
                    bad.append((name, discrete, k, v))
            relS = rel_fro(S, ora[21][0])
            print(f"partitioned filter {name} discrete={discrete}: Sigma against the dense oracle {relS:.2e}")
            if not relS < 1e-12:
                bad.append((name, discrete, "Sigma", relS))
            assert be.device_error() == 0
            tf.close()
    print("partitioned filter, worst ratios: " + "  ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert not bad, bad


@pytest.mark.parametrize("mode", ["discrete", "continuous", "nolift"])
def test_innovation_application_at_large_delta(hip, mode):
    """X <- Delta X with |dU_omega| of 1.2 .. 1.5 rad and |gamma_q| up to 0.65 |q_i| (wide Sigma, bearings 0.6 rad off the prediction): X
    after the update against the reference applied to the DEVICE'S OWN (dU, gamma_v, gamma_q), so the solver does not enter.  The
    precondition is asserted on the device's Gamma: the test fails, it does not skip, if the input misses the branch."""
    from oracle import eqf_numpy as en

    bad = []
    for N, scale in ec.INNOVATION_STATES:
        d, snap, y = ec.innovation_case(en, N, scale, mode)
        fg = hip.FilterBatch(d, capacity=CAP, batch=1)
        fg.restore_state(snap)
        assert np.all(fg.process_vision([ec.INNOVATION_STAMP], snap["ids"], y) == 0)
        g = fg.group()
        dU, gg, gv, gq = ec.innovation_parts(fg.last_update(), mode, N)
        xi0 = lx.State.from_dict(snap["origin"], d["cameraOffset_q"], d["cameraOffset_x"])
        if dU is None:
            eta0, _, ci = lx.pose_constants(xi0.R)
            g2 = lx.vec(gg)
            dUw = lx.to_np(lx.cross(eta0, [ci[i][0] * g2[0] + ci[i][1] * g2[1] for i in range(3)]))
        else:
            dUw = dU[0:3]
        rel = (np.linalg.norm(gq, axis=1) / np.linalg.norm(snap["origin"]["p"], axis=1)).max()
        assert 0.6 <= np.linalg.norm(dUw) <= 2.0 and rel >= 0.5, (np.linalg.norm(dUw), rel)
        Xpre, _ = lx.reference_step(snap, ec.INNOVATION_STAMP, d)
        r = lx.group_ratios(g, lx.apply_innovation(Xpre, xi0, dU, gv, gq, mode, gg))
        print(f"device, X <- Delta X, {mode}, N = {N}: |dU_omega| = {np.linalg.norm(dUw):.3f}, max |gamma_q|/|q| = {rel:.3f}, ratios "
              + "  ".join(f"{k} {v:.2f}" for k, v in r.items()))
        bad += [(N, k, v) for k, v in r.items() if not v <= ec.K_INNOVATION[k]]
        assert fg.device_error() == 0
    assert not bad, bad


def check_pole_landmarks(fg, snap, d, stamp, what, bad):
    """C0i of every landmark of the handle's filter 0 and the residual of one update whose bearings are 1e-3 rad off the prediction, against
    the reference from the snapshot (taken as exact doubles); theta per landmark from its origin."""
    p0 = np.asarray(snap["origin"]["p"])
    th = np.arccos(np.clip(p0[:, 2] / np.linalg.norm(p0, axis=1), -1, 1))
    th = np.array([min(ec.POLE_THETAS, key=lambda t: abs(np.log(t / max(x, 1e-300)))) for x in th])  # (the list's value, not its rounding)
    C0 = fg.debug_blocks()["C0"]
    Xpre, _ = lx.reference_step(snap, stamp, d)
    t = ec._unit([0.3, -0.8, 0.5])
    y = np.zeros_like(p0)
    for i, p in enumerate(p0):
        y0 = p / np.linalg.norm(p)
        off = ec._unit(y0 * np.cos(1e-3) + ec._unit(np.cross(y0, t)) * np.sin(1e-3))
        y[i] = ec._unit(lx.to_np(lx.mv(lx.tr(Xpre.Q[i][0]), lx.vec(off))))  # R_Q y is 1e-3 rad off y0
    assert np.all(fg.process_vision([stamp], snap["ids"], y) == 0)
    delta = fg.last_update()["delta"]
    worst = {"C0": {}, "delta": {}}
    for i, p in enumerate(p0):
        Cr, _ = lx.landmark_constants(p)
        rc = lx.pole_ratio(C0[i], Cr, th[i], 1.0 / np.linalg.norm(p))
        rd = lx.pole_ratio(delta[2 * i:2 * i + 2], lx.residual(y[i], Xpre.Q[i][0], p), th[i])
        assert 2e-4 < np.abs(delta[2 * i:2 * i + 2]).max() < 1e-3  # (the residual is the 1e-3 rad of the input, halved by the chart)
        worst["C0"][th[i]], worst["delta"][th[i]] = max(worst["C0"].get(th[i], 0.0), rc), max(worst["delta"].get(th[i], 0.0), rd)
        if not (rc <= ec.K_POLE["C0"] and rd <= ec.K_POLE["delta"]):
            bad.append((what, i, th[i], rc, rd))
    for k, v in worst.items():
        print(f"device near the pole, {what}, {k:5s} ratio to (u / theta^2) scale: " + "  ".join(f"{t:g}: {x:.3f}" for t, x in sorted(v.items(), reverse=True)))
    assert fg.device_error() == 0, what


def test_origin_landmarks_near_the_chart_pole(hip):
    """Origin landmarks 0.5 .. 2e-4 rad from the optical axis (1 + c = theta^2 / 2 in rotFromUnitVectors), five azimuths, depths 1 and 10,
    brought in by restore_state and as new landmarks through process_vision: C0i and the residual within K (u / theta^2) scale of the
    reference, and no flag (2e-4 is a factor 2 outside the 1e-8 threshold)."""
    bad = []
    d = ec.settings(True)
    snap = ec.pole_snapshot()
    N = len(snap["ids"])
    fg = hip.FilterBatch(d, capacity=N, batch=1)
    fg.restore_state(snap)
    assert fg.device_error() == 0
    check_pole_landmarks(fg, snap, d, ec.T0 + 0.005, "restored", bad)
    dirs = ec.pole_directions()
    for depth in ec.POLE_DEPTHS:
        d = ec.settings(True, initialSceneDepth=depth)
        fg = hip.FilterBatch(d, capacity=len(dirs), batch=1)
        fg.process_imu([0.0], [0.01, -0.02, 0.03], [9.0, 0.5, 3.0])
        fg.process_imu([0.005], [0.01, -0.02, 0.03], [9.0, 0.5, 3.0])
        ids = np.arange(1, len(dirs) + 1, dtype=np.int32)
        assert np.all(fg.process_vision([0.0075], ids, np.array([y for _, _, y in dirs])) == 0)
        assert fg.device_error() == 0 and fg.num_landmarks() == len(dirs)
        snap = fg.dump_state()
        assert np.abs(np.linalg.norm(snap["origin"]["p"], axis=1) - depth).max() < 1e-14 * depth  # the appended origins land where meant
        check_pole_landmarks(fg, snap, d, 0.0125, f"new, depth {depth:g}", bad)
    assert not bad, bad


def test_gravity_chart_near_the_pole(hip, monkeypatch):
    """A first accelerometer sample 0.5 .. 2e-4 rad from level, five azimuths (30 filters of one handle): cDiff / cInv through the blocks
    Bg = cDiff R_A eta^ and Avg = -g cInv of the next step (debug_blocks, split path) and the chart part G = cDiff R_A^T cInv of
    local_jacobian, against the reference taken from the device's own origin pose; nothing raises a flag."""
    dirs = ec.pole_directions()
    fg = make_handle(hip, monkeypatch, ec.settings(True), {"EQF_IMU_BURST": "0", "EQF_SPLIT_PROPAGATE": "1"}, batch=len(dirs), capacity=4)
    acc = np.array([ec.tilted_accel(th, az) for th, az, _ in dirs])
    fg.process_imu([0.0], np.zeros(3), acc)
    fg.process_imu([0.005], np.zeros(3), acc)
    assert fg.device_error() == 0
    worst, bad = {"Bg": {}, "Avg": {}, "G": {}}, []
    for b, (th, az, _) in enumerate(dirs):
        q0 = fg.origin(b)["q"]
        eta0, cd, ci = lx.pose_constants(lx.rot_of_quat(q0))
        assert abs(float(lx.mp.acos(eta0[2])) / th - 1) < 1e-6  # the start is theta from level
        blk, G = fg.debug_blocks(b), fg.local_jacobian(b)["G"]
        r = {"Bg": lx.pole_ratio(blk["Bg"], lx.mm(cd, lx.hat(eta0)), th), "Avg": lx.pole_ratio(blk["Avg"], lx.mscl(-lx.GRAVITY, ci), th, 2 * 9.81),
             "G": lx.pole_ratio(G, lx.mm(cd, ci), th, 2.0)}
        for k, v in r.items():
            worst[k][th] = max(worst[k].get(th, 0.0), v)
            if not v <= ec.K_POLE[k]:
                bad.append((th, az, k, v))
    for k, v in worst.items():
        print(f"device, gravity chart near the pole, {k:3s} ratio to (u / theta^2) scale: " + "  ".join(f"{t:g}: {x:.3f}" for t, x in v.items()))
    assert fg.device_error() == 0
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------------------------------
# the singularity bits of eqf_device_error, by value
# ------------------------------------------------------------------------------------------------------------------------------------------
def _benign_bearings():
    return np.array([ec._unit(v) for v in ([0.3, 0.1, 1.0], [-0.2, 0.25, 1.0], [0.1, -0.3, 1.0])])


def _start(fg, accel=(9.0, 0.5, 3.0)):
    fg.process_imu([0.0], [0.01, -0.02, 0.03], accel)
    fg.process_imu([0.005], [0.01, -0.02, 0.03], accel)


def _replays_bit_for_bit(hip, fg, dense=False, clean=True):
    """after eqf_reset the handle gives what a new handle gives on a benign stream (clean: and neither raises a flag)"""
    from eqf_vio_amd import synth

    st = synth.make_stream(3, duration=0.16)
    new = hip.FilterBatch(fg.settings, capacity=fg.cap, batch=fg.B)
    if dense:
        fg.set_dense_propagate(True)
        new.set_dense_propagate(True)
    for f in (fg, new):
        for kind, k in st.events():
            if kind == "imu":
                f.process_imu([st.imu[k, 0]], st.imu[k, 1:4], st.imu[k, 4:7])
            else:
                f.process_vision([st.vision_stamps[k]], st.ids, st.bearings[k])
    for b in range(fg.B):
        assert np.array_equal(fg.sigma(b), new.sigma(b)) and all(np.array_equal(fg.group(b)[k], new.group(b)[k]) for k in ("Aq", "Ax", "w", "Qq", "Qa"))
    assert fg.device_error() == new.device_error() and (fg.device_error() == 0 or not clean)


@pytest.mark.parametrize("theta", ec.FLAG_THETAS)
def test_new_landmark_on_the_pole_raises_bit_16(hip, theta):
    """theta <= 1e-4: 1 + c <= 5e-9, a factor 2 inside the threshold.  The bit by value (with bit 4 from the update of the same call when the
    landmark is exactly ON the pole, as include/eqf_vio_amd.h says), sticky, cleared by eqf_reset, and the handle replays a benign stream bit
    for bit afterwards."""
    fg = hip.FilterBatch(ec.settings(True), capacity=4, batch=1)
    for th, az, y in ec.pole_directions((theta,))[:3]:
        _start(fg)
        assert fg.device_error() == 0
        assert np.all(fg.process_vision([0.0075], [1, 2, 3, 4], np.vstack([_benign_bearings(), y])) == 0)
        want = 16 | (4 if theta == 0.0 else 0)  # exactly ON the pole 1 / (1 + c) is infinite: C0i is NaN and the call's update meets a NaN pivot
        assert fg.device_error() == want, (theta, az)
        fg.process_imu([0.010], [0.01, -0.02, 0.03], [9.0, 0.5, 3.0])
        assert fg.device_error() == want  # sticky
        fg.reset()
        assert fg.device_error() == 0
    _replays_bit_for_bit(hip, fg)


@pytest.mark.parametrize("theta", ec.FLAG_THETAS)
def test_restored_landmark_on_the_pole_raises_bit_32(hip, theta):
    fg = hip.FilterBatch(ec.settings(True), capacity=8, batch=1)
    for th, az, y in ec.pole_directions((theta,))[:3]:
        snap = ec.base_snapshot(5)
        snap["origin"]["p"][3] = 4.0 * y
        fg.restore_state(snap)
        assert fg.device_error() == 32, (theta, az)
        fg.process_imu([ec.T0 + 0.005], IMU_W, IMU_A)
        assert fg.device_error() == 32  # sticky
        fg.reset()
        assert fg.device_error() == 0
    fg.restore_state(ec.base_snapshot(5))  # the same state without the offending landmark
    assert fg.device_error() == 0
    fg.reset()
    _replays_bit_for_bit(hip, fg)


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("theta", ec.FLAG_THETAS)
def test_start_on_the_pole_raises_bit_1(hip, theta, dense):
    """A first accelerometer sample theta <= 1e-4 from level: bit 1 from the call that initialises the pose, under either Riccati backend (the
    next call steps with the cached constants, so the dense backend's builder has nothing to look at).  The local getters answer
    EQF_ERR_NUMERIC while the chart is singular; reset clears all of it."""
    fg = hip.FilterBatch(ec.settings(True), capacity=4, batch=1)
    if dense:
        fg.set_dense_propagate(True)
    for th, az, _ in ec.pole_directions((theta,))[:3]:
        _start(fg, ec.tilted_accel(theta, az))
        err = fg.device_error()
        print(f"start {theta:g} rad from level, azimuth {az:g}, dense = {dense}: eqf_device_error = {err}")
        assert err == 1, (theta, az, err)
        fg.process_imu([0.010], [0.01, -0.02, 0.03], [9.0, 0.5, 3.0])
        assert fg.device_error() == 1  # sticky
        with pytest.raises(hip.EqfError) as ei:
            fg.local_jacobian()
        assert ei.value.code == hip.ERR_NUMERIC
        fg.reset()
        assert fg.device_error() == 0
    if dense:
        fg.set_dense_propagate(True)
    _start(fg)
    assert fg.device_error() == 0 and fg.local_jacobian()["G"].shape == (2, 2)
    fg.reset()
    _replays_bit_for_bit(hip, fg, dense)


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("theta", ec.FLAG_THETAS)
def test_start_inside_a_stepping_call_raises_bit_64_under_the_dense_backend(hip, theta, dense):
    """The one input that reaches bit 64: a restored filter with a valid time and initialised = 0, so that the call that initialises the pose
    from a sample theta <= 1e-4 from level also steps and the Riccati builder computes the chart constants itself: 64 | 1 under the dense
    backend (1 from the group step beside it), 1 alone otherwise."""
    fg = hip.FilterBatch(ec.settings(True), capacity=8, batch=1)
    if dense:
        fg.set_dense_propagate(True)
    for th, az, _ in ec.pole_directions((theta,))[:3]:
        snap = ec.base_snapshot(5)
        snap["initialised"] = 0
        fg.restore_state(snap)
        assert fg.device_error() == 0
        fg.process_imu([ec.T0 + 0.005], IMU_W, ec.tilted_accel(theta, az))
        err = fg.device_error()
        print(f"initialising call that steps, {theta:g} rad from level, azimuth {az:g}, dense = {dense}: eqf_device_error = {err}")
        assert err == ((64 | 1) if dense else 1), (theta, az, err)
        fg.process_imu([ec.T0 + 0.010], IMU_W, IMU_A)
        assert fg.device_error() == err  # sticky
        with pytest.raises(hip.EqfError) as ei:
            fg.local_jacobian()
        assert ei.value.code == hip.ERR_NUMERIC
        fg.reset()
        assert fg.device_error() == 0
    # the same call with a tilted sample raises nothing
    snap = ec.base_snapshot(5)
    snap["initialised"] = 0
    if dense:
        fg.set_dense_propagate(True)
    fg.restore_state(snap)
    fg.process_imu([ec.T0 + 0.005], IMU_W, IMU_A)
    assert fg.device_error() == 0
    fg.reset()
    _replays_bit_for_bit(hip, fg, dense)


def test_antipodal_innovation_raises_bit_8_and_leaves_the_other_filter_alone(hip):
    """SO3FromVectors(q_i + gamma_q, q_i) of the discrete innovation lift at the antipode (input chosen on the CPU, where the numpy oracle
    throws: lie_edge_cases.antipodal_innovation_case, 1 + c = 1.2e-9): bit 8 by value, sticky, cleared by eqf_reset, the handle replays bit
    for bit afterwards; filter 1 of the handle, with the bearings its estimate predicts, is bit for bit what it is when filter 0 gets them too."""
    from oracle import eqf_numpy as en

    d, snap, y = ec.antipodal_innovation_case(en)
    benign = en.measure_system_state(ec.numpy_filter(en, snap, d).stateEstimate())
    runs = []
    for offending in (True, False):
        fg = hip.FilterBatch(d, capacity=5, batch=2)
        fg.restore_state(snap, 0)
        fg.restore_state(snap, 1)
        assert np.all(fg.process_vision([ec.INNOVATION_STAMP], snap["ids"], np.stack([y if offending else benign, benign])) == 0)
        err = fg.device_error()
        print(f"antipodal innovation in filter 0, offending = {offending}: eqf_device_error = {err}")
        assert err == (8 if offending else 0), err
        runs.append((fg.sigma(1), fg.group(1), fg.state_estimate(1), fg.bias(1)))
        if offending:
            fg.process_imu([ec.INNOVATION_STAMP + 0.005], IMU_W, IMU_A)
            assert fg.device_error() == 8  # sticky
            fg.reset()
            assert fg.device_error() == 0
            # (with this case's measurement variance of 1e-12 the synthetic stream is not benign: its third update meets the antipode in the
            # numpy oracle too -- so only "like a new handle, flags included" is asked here)
            _replays_bit_for_bit(hip, fg, clean=False)
    a, b = runs
    assert np.all(np.isfinite(a[0])) and np.array_equal(a[0], b[0]) and np.array_equal(a[3], b[3])
    assert all(np.array_equal(a[1][k], b[1][k]) for k in a[1]) and all(np.array_equal(a[2][k], b[2][k]) for k in a[2])


@pytest.mark.parametrize("how", ["new", "restored"])
@pytest.mark.parametrize("theta", ec.FLAG_THETAS)
def test_offending_landmark_leaves_the_other_filter_of_the_handle_alone(hip, theta, how):
    """Two filters in one handle: filter 0 gets a landmark on the pole -- a new one (bit 16) or a restored one (bit 32); its constants are
    garbage, exactly ON the pole NaN, so its own updates may add bit 4 and nothing else -- and filter 1 runs benign input: its state and Sigma
    are bit for bit what they are when filter 0's landmark is benign.  (The bits by value: the two tests above.)"""
    from eqf_vio_amd import synth
    from oracle import eqf_numpy as en

    pole = ec.pole_directions((theta,))[1][2]
    bit = 16 if how == "new" else 32
    runs = []
    for offending in (True, False):
        if how == "new":
            st = synth.make_stream(4, duration=0.16)
            fg = hip.FilterBatch(ec.settings(True), capacity=4, batch=2)
            for kind, k in st.events():
                if kind == "imu":
                    fg.process_imu([st.imu[k, 0]], st.imu[k, 1:4], st.imu[k, 4:7])
                else:
                    y = np.stack([st.bearings[k], st.bearings[k]])
                    if offending:
                        y[0, 3] = pole
                    fg.process_vision([st.vision_stamps[k]], st.ids, y)
        else:
            d, snap, y = ec.innovation_case(en, 5, 1.0, "discrete")
            fg = hip.FilterBatch(d, capacity=5, batch=2)
            fg.restore_state(snap, 1)
            if offending:
                snap["origin"]["p"][3] = 4.0 * pole
            fg.restore_state(snap, 0)
            for k in range(1, 4):
                fg.process_imu([ec.T0 + 0.001 * k], IMU_W, IMU_A)
            fg.process_vision([ec.INNOVATION_STAMP], snap["ids"], y)
        err = fg.device_error()
        print(f"{how} landmark {theta:g} rad from the pole in filter 0, offending = {offending}: eqf_device_error = {err}")
        assert (err & bit and not err & ~(bit | 4)) if offending else err == 0, err
        runs.append((fg.sigma(1), fg.group(1), fg.state_estimate(1), fg.bias(1)))
    a, b = runs
    assert np.all(np.isfinite(a[0])) and np.array_equal(a[0], b[0]) and np.array_equal(a[3], b[3])
    assert all(np.array_equal(a[1][k], b[1][k]) for k in a[1]) and all(np.array_equal(a[2][k], b[2][k]) for k in a[2])
