"""The mpmath reference of the geometric state (tests/lie_exact.py) against the numpy oracle and against the device's formulas compiled for
the host -- no GPU.

(a) benign input (states of a short synthetic run): reference and oracle/eqf_numpy.py agree to 1e-13, so the reference computes the
    operation the filter means.
(b) edge input (tests/lie_edge_cases.py: rotations of 0.4999 .. 3.3 rad per step, innovations of more than a radian, origin landmarks down to
    2e-4 rad from the chart pole): the numpy oracle's error against the reference as a ratio to the bound forms.  These ratios are the
    yardstick of tests/test_gpu_lie_edges.py: every K there is 4 x the worst ratio here, unrounded (lie_edge_cases.ORACLE_*), and this test asserts 4 x ratio <= K.
    Measured (x86-64, glibc libm), worst ratio per bound form (theta <= 2.2 / theta >= 3.0 for the group step; DESIGN.md section 5 has the
    device's figures beside them):
        group step, discrete lift    A.R 0.85/1.57  A.x 0.39/0.31  w 4.90/5.81  Q.R 11.2/35.3  Q.a 3.51/3.97  est.R 0.90/1.58  est.x 0.57/0.53
                                     est.v 4.73/9.73  est.p 22.7/317
        group step, exponential lift A.R 0.85/1.57  A.x 0.39/0.31  w 6.92/6.06  Q.R 4.70/5.97  Q.a 0.98/0.87  est.R 0.90/1.58  est.x 0.57/0.53
                                     est.v 5.27/12.3  est.p 12.1/16.8
        X <- Delta X, three modes    A.R 2.80  A.x 1.54  w 0.78  Q.R 1.13  Q.a 1.68
        near the pole [u/theta^2]    C0 1.07  residual 0.45  Bg 0.51  Avg 1.98  G 1.00
(c) tests/lie_host_main.cpp: eqf_math.hpp compiled by g++ for the host under ASan / UBSan -- the device's own formulas short of FMA
    contraction and of the device's sin / cos -- on the same edge inputs, against the reference, with the bounds of (b).  se3ExpParts
    (eqf_burst.hpp), stepLandmark / stepGlobal (eqf_propagate.hpp) and landmarkConstants (eqf_update.hpp) do not compile for the host (their
    headers hold kernels: threadIdx, LDS, wave intrinsics), so they are reached on the device only (tests/test_gpu_lie_edges.py).
(d) the reference must SEE a fault: a closed-form B cut to four series terms, a transposed R_s and m2q with two branch bodies swapped each
    fall outside the bound that the correct formula meets.  The faults live here, not in the library."""
import os
import subprocess

import numpy as np
import pytest

import lie_edge_cases as ec
import lie_exact as lx
from eqf_vio_amd import synth
from oracle import eqf_numpy as en

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = lx.U
# expCoefficients above the seam, bound form K u (1 + |value|), from the formulas' own first-order error where the division by t = th^2
# amplifies most (t = 0.25): err(A) <= 2.5 u (sqrt, sin, one division), err(B) <= (u |cos| + u/2 (1 - cos) + u/2 th sin th) / t + u/2 B
# <= 7 u, err(C) <= (err(A) + u/2) / t + u/2 C <= 12.1 u, i.e. 10.4 u (1 + C); K = 16 leaves a factor 1.5 for the terms of second order.
K_EXPC = 16.0
# m2q(q2m(q)) of a unit quaternion to rounding: q2m is 4 operations deep on values <= 2, m2q a sqrt, a division and a product; the worst
# branch divides by t >= 1 (the largest of four squares summing to 4 is >= 1): <= 8 u absolute in the matrix, <= 8 u in q
K_M2Q = 16.0
MEASURED = {}  # what the yardstick tests measured in this run (a script that renews ORACLE_* of lie_edge_cases.py reads it)


def numpy_snapshot(f):
    return dict(ids=f.X.ids.copy(), origin=dict(q=f.xi0.pose.q.copy(), x=f.xi0.pose.x.copy(), v=f.xi0.velocity.copy(), p=f.xi0.p.copy()),
                group=ec.numpy_group(f), bias=f.inputBias.copy(), sigma=f.Sigma.copy(), time=f.currentTime,
                currentVelocity=np.concatenate([f.currentVelocity.omega, f.currentVelocity.accel]), accumulatedVelocity=np.zeros(6),
                accumulatedTime=0.0, initialised=1)


def step_ratios(snap, stamp, d):
    """The numpy oracle's group step of a snapshot against the reference: ratios per quantity."""
    f = ec.numpy_filter(en, snap, d)
    f.integrateUpToTime(stamp)
    X, est = lx.reference_step(snap, stamp, d)
    return lx.group_ratios(ec.numpy_group(f), X, ec.numpy_estimate(f), est)


def innovation_ratios(d, snap, y, mode):
    """One processVisionData of the numpy oracle; X after it against the reference applied to the oracle's own (dU, gamma_v, gamma_q)."""
    N = len(snap["ids"])
    f = ec.numpy_filter(en, snap, d)
    f.processVisionData(ec.INNOVATION_STAMP, snap["ids"], y)
    dU, gg, gv, gq = ec.innovation_parts(f.last, mode, N)
    xi0 = lx.State.from_dict(snap["origin"], d["cameraOffset_q"], d["cameraOffset_x"])
    Xpre, _ = lx.reference_step(snap, ec.INNOVATION_STAMP, d)
    Xref = lx.apply_innovation(Xpre, xi0, dU, gv, gq, mode, gg)
    if dU is None:
        eta0, _, ci = lx.pose_constants(xi0.R)
        g2 = lx.vec(gg)
        dUw = lx.to_np(lx.cross(eta0, [ci[i][0] * g2[0] + ci[i][1] * g2[1] for i in range(3)]))
    else:
        dUw = dU[0:3]
    rel = np.linalg.norm(gq, axis=1) / np.linalg.norm(snap["origin"]["p"], axis=1)
    return lx.group_ratios(ec.numpy_group(f), Xref), float(np.linalg.norm(dUw)), float(rel.max())


# ------------------------------------------------------------------------------------------------------------------------------------------
# (a)
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["discrete", "continuous", "nolift"])
@pytest.mark.parametrize("discrete_velocity", [True, False])
def test_reference_agrees_with_the_oracle_on_benign_input(discrete_velocity, mode):
    """States of a 0.3 s synthetic run (N = 6): the group step of every 7th IMU call, every vision update's X <- Delta X, C0i, R_s, the
    residual and the pose constants; reference against oracle <= 1e-13 absolute (the values are O(1) .. O(10))."""
    N = 6
    st = synth.make_stream(N, duration=0.3)
    d = ec.settings(discrete_velocity, **ec.INNOVATION_MODES[mode])
    f = en.VIOFilter(ec.numpy_settings(en, d))
    worst, steps, updates = 0.0, 0, 0

    def close(got, want):
        nonlocal worst
        worst = max(worst, float(np.abs(np.asarray(got, dtype=float) - lx.to_np(want)).max()))

    def close_group(g, X):
        close(en.quat_to_matrix(g["Aq"]), X.AR), close(g["Ax"], X.Ax), close(g["w"], X.w)
        for i, Q in enumerate(X.Q):
            close(en.quat_to_matrix(g["Qq"][i]), Q[0]), close([g["Qa"][i]], [Q[1]])

    for n, (kind, k) in enumerate(st.events()):
        if kind == "imu":
            r = st.imu[k]
            snap = numpy_snapshot(f) if f.initialisedFlag and n % 7 == 0 and f.currentTime >= 0 else None
            f.processIMUData(en.IMUVelocity(r[0], r[1:4], r[4:7]))
            if snap is not None:
                X, est = lx.reference_step(snap, r[0], d)
                close_group(ec.numpy_group(f), X)
                e = ec.numpy_estimate(f)
                close(en.quat_to_matrix(e["q"]), est.R), close(e["x"], est.x), close(e["v"], est.v)
                for i, p in enumerate(est.p):
                    close(e["p"][i], p)
                steps += 1
        else:
            fpre = ec.numpy_filter(en, numpy_snapshot(f), d)
            fpre.integrateUpToTime(st.vision_stamps[k])
            f.processVisionData(st.vision_stamps[k], st.ids, st.bearings[k])
            if not f.last or len(fpre.X.Q) != N:
                continue  # (the first frame only adds the landmarks)
            snap = numpy_snapshot(fpre)
            xi0 = lx.State.from_dict(snap["origin"], d["cameraOffset_q"], d["cameraOffset_x"])
            dU, gg, gv, gq = ec.innovation_parts(f.last, mode, N)
            close_group(ec.numpy_group(f), lx.apply_innovation(lx.Group.from_dict(snap["group"]), xi0, dU, gv, gq, mode, gg))
            C0 = en.eqf_output_matrix_C(f.xi0)
            for i, p in enumerate(f.xi0.p):
                Cr, Rs = lx.landmark_constants(p)
                close(C0[2 * i:2 * i + 2, 5 + 3 * i:8 + 3 * i], Cr)
                close(en.quat_to_matrix(en._sphere_rot(p / np.linalg.norm(p))), Rs)
                close(f.last["delta"][2 * i:2 * i + 2], lx.residual(st.bearings[k][i], lx.rot_of_quat(fpre.X.Q[i].q), p))
            eta0, cd, ci = lx.pose_constants(xi0.R)
            e0 = en.project_to_manifold(f.xi0).gravityDir
            close(e0, eta0), close(en.stereo_sphere_chart_diff(e0, e0), cd), close(en.stereo_sphere_chart_inv_diff(np.zeros(2), e0), ci)
            updates += 1
    assert steps >= 6 and updates >= 4
    print(f"reference against the numpy oracle on benign input: worst absolute difference {worst:.2e}")
    assert worst <= 1e-13, worst


# ------------------------------------------------------------------------------------------------------------------------------------------
# (b)
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("discrete_velocity", [True, False])
def test_oracle_yardstick_of_the_group_step_at_large_angles(discrete_velocity):
    d = ec.settings(discrete_velocity)
    worst = {c: {} for c in ec.ANGLE_CLASSES}
    for name, th, ax, dt in ec.propagate_cases():
        snap, stamp = ec.propagate_snapshot(th, ax, dt, 21)
        w = worst[ec.angle_class(th)]
        for k, v in step_ratios(snap, stamp, d).items():
            if v > w.get(k, (0.0, ""))[0]:
                w[k] = (v, name)
    print(f"numpy oracle, group step, {'discrete' if discrete_velocity else 'exponential'} lift, ratio to u (1 + magnitude):")
    for c, w in worst.items():
        for k, (v, name) in w.items():
            print(f"    {c:8s} {k:6s} {v:8.2f}  at {name}")
    MEASURED[("step", discrete_velocity)] = {c: {k: v for k, (v, _) in w.items()} for c, w in worst.items()}
    bad = [(c, k, v, name) for c, w in worst.items() for k, (v, name) in w.items() if not 4 * v <= ec.K_STEP[discrete_velocity][c][k]]
    assert not bad, bad


@pytest.mark.parametrize("mode", ["discrete", "continuous", "nolift"])
def test_oracle_yardstick_of_the_innovation_at_large_delta(mode):
    bad = []
    for N, scale in ec.INNOVATION_STATES:
        d, snap, y = ec.innovation_case(en, N, scale, mode)
        r, dUw, rel = innovation_ratios(d, snap, y, mode)
        for k, v in r.items():
            MEASURED.setdefault("innovation", {})[k] = max(MEASURED.get("innovation", {}).get(k, 0.0), v)
        print(f"numpy oracle, X <- Delta X, {mode}, N = {N}: |dU_omega| = {dUw:.3f}, max |gamma_q|/|q| = {rel:.3f}, ratios "
              + "  ".join(f"{k} {v:.2f}" for k, v in r.items()))
        assert 0.6 <= dUw <= 2.0 and rel >= 0.5, (dUw, rel)  # the inputs reach the branch
        bad += [(mode, N, k, v) for k, v in r.items() if not 4 * v <= ec.K_INNOVATION[k]]
    assert not bad, bad


def oracle_pole_ratios():
    """The numpy oracle near the pole: {quantity: {theta: worst ratio to (u / theta^2) scale}}."""
    out = {k: {} for k in ec.K_POLE}

    def put(k, th, v):
        out[k][th] = max(out[k].get(th, 0.0), v)

    rng = np.random.default_rng(3)
    for th, p in ec.pole_landmarks():
        depth = np.linalg.norm(p)
        y0 = p / depth
        st = en.VIOState(p=[p], ids=[1])
        Cr, _ = lx.landmark_constants(p)
        put("C0", th, lx.pole_ratio(en.eqf_output_matrix_C(st)[:, 5:8], Cr, th, 1.0 / depth))
        q = ec._quat(rng.standard_normal(3), 0.1)
        t = np.cross(y0, [0.3, -0.8, 0.5])
        y = en.quat_rotate(en.quat_inverse(q), y0 * np.cos(1e-3) + t / np.linalg.norm(t) * np.sin(1e-3))  # R_Q y is 1e-3 rad off y0
        put("delta", th, lx.pole_ratio(en.stereo_sphere_chart(en.quat_rotate(q, y), y0), lx.residual(y, lx.rot_of_quat(q), p), th))
    for th, az, _ in ec.pole_directions():
        q0 = en.so3_from_vectors(ec.tilted_accel(th, az), en.E3)
        e0 = en.quat_rotate(en.quat_inverse(q0), en.E3)
        eta0, cd, ci = lx.pose_constants(lx.rot_of_quat(q0))
        cdn, cin = en.stereo_sphere_chart_diff(e0, e0), en.stereo_sphere_chart_inv_diff(np.zeros(2), e0)
        put("Bg", th, lx.pole_ratio(cdn @ en.skew(e0), lx.mm(cd, lx.hat(eta0)), th))
        put("Avg", th, lx.pole_ratio(-9.81 * cin, lx.mscl(-lx.GRAVITY, ci), th, 2 * 9.81))
        put("G", th, lx.pole_ratio(cdn @ cin, lx.mm(cd, ci), th, 2.0))
    return out


def test_oracle_yardstick_near_the_chart_pole():
    r = oracle_pole_ratios()
    print("numpy oracle near the chart pole, ratio to (u / theta^2) scale, per theta:")
    for k, v in r.items():
        print(f"    {k:6s} " + "  ".join(f"{th:g}: {x:.3f}" for th, x in v.items()))
    MEASURED["pole"] = {k: max(v.values()) for k, v in r.items()}
    bad = [(k, v) for k, v in r.items() if not 4 * max(v.values()) <= ec.K_POLE[k]]
    assert not bad, bad


def test_oracle_throws_on_the_antipodal_innovation_input():
    """The input of the GPU test of bit 8 (eqf_device_error) makes the reference's discrete innovation lift throw, a factor >= 2 inside the
    threshold; with the bearing left on the prediction it does not."""
    d, snap, y = ec.antipodal_innovation_case(en)
    f = ec.numpy_filter(en, snap, d)
    with pytest.raises(en.AntipodalError):
        f.processVisionData(ec.INNOVATION_STAMP, snap["ids"], y)
    f = ec.numpy_filter(en, snap, dict(d, useDiscreteInnovationLift=False))
    f.processVisionData(ec.INNOVATION_STAMP, snap["ids"], y)
    q, g = snap["origin"]["p"][2], f.last["Gamma"][9:].reshape(-1, 3)[2]
    one_plus_c = 1 + (q + g) @ q / np.linalg.norm(q + g) / np.linalg.norm(q)
    print(f"antipodal innovation input: 1 + c = {one_plus_c:.3e}")
    assert 0 <= one_plus_c <= 5e-9
    f = ec.numpy_filter(en, snap, d)
    f.processVisionData(ec.INNOVATION_STAMP, snap["ids"], en.measure_system_state(f.stateEstimate()))


# ------------------------------------------------------------------------------------------------------------------------------------------
# (c)
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lie_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lie_host") / "lie_host")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", os.path.join(ROOT, "eqf_vio_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "lie_host_main.cpp")], check=True)

    def run(cases):
        text = "\n".join(name + " " + " ".join(repr(float(x)) for x in np.concatenate([np.ravel(a) for a in args])) for name, *args in cases)
        r = subprocess.run([exe], input=text + "\n", capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        rows = [np.array([float(t) for t in ln.split()]) for ln in r.stdout.split("\n")[:-1]]
        assert len(rows) == len(cases)
        return rows

    return run


def test_host_expCoefficients_across_the_seam(lie_host):
    """Series below t = 0.25, closed forms above, to 16 u (1 + |value|) on both sides and at the seam itself."""
    ts = [0.0, 1e-12, 0.1, 0.2499999999, np.nextafter(0.25, 0), 0.25, np.nextafter(0.25, 1), 0.2500000001] + [th * th for th in ec.THETAS] + [9.0, 39.0]
    worst = 0.0
    for t, row in zip(ts, lie_host([("expc", [t]) for t in ts])):
        for got, want in zip(row, lx.exp_coefficients(t)):
            worst = max(worst, lx.ratio([got], [want]))
    print(f"host expCoefficients: worst ratio to u (1 + |value|) {worst:.2f}")
    assert worst <= K_EXPC, worst


def test_host_exponentials_at_large_angles(lie_host):
    """se3Exp / so3Exp of eqf_math.hpp at the propagate cases' rotations against the reference, bounds of the group step's A (discrete
    lift: A is the exponential itself there)."""
    v = np.array([0.11, -0.07, 0.16])
    cases = [("se3exp", th * ec._unit(ax), v) for th in ec.THETAS for ax in ec.AXES.values()]
    worst = {c: [0.0, 0.0] for c in ec.ANGLE_CLASSES}
    for (_, w, _), row, row3 in zip(cases, lie_host(cases), lie_host([("so3exp", c[1]) for c in cases])):
        R, x = lx.se3_exp(lx.vec(w), lx.vec(v))
        ws = worst[ec.angle_class(np.linalg.norm(w) + 1e-12)]
        ws[0] = max(ws[0], lx.ratio(lx.to_np(lx.rot_of_quat(row[0:4])), R), lx.ratio(lx.to_np(lx.rot_of_quat(row3)), R))
        ws[1] = max(ws[1], lx.ratio(row[4:7], x))
    print(f"host se3Exp / so3Exp: worst ratio (R, x) per angle class {worst}")
    for c, (wr, wx) in worst.items():
        assert wr <= ec.K_STEP[True][c]["A.R"] and wx <= ec.K_STEP[True][c]["A.x"], (c, wr, wx)


def m2q_branch(q):
    """Which of m2q's four branches the rotation of q takes (the conditions of eqf_math.hpp)."""
    M = en.quat_to_matrix(np.asarray(q, dtype=float))
    m00, m11, m22 = np.diag(M)
    if m00 + m11 + m22 > 0:
        return 0
    if m00 >= m11 and m00 >= m22:
        return 1
    return 2 if (m11 > m00 and m11 >= m22) else 3


def test_host_m2q_on_all_four_branches(lie_host):
    """m2q(q2m(q)) on rotations past 120 degrees about x, y, z and a general axis, and below: each of m2q's four branches is reached (asserted)
    and returns the rotation it was given."""
    qs = [ec._quat(ax, th) for th in (0.5, 2.2, 3.0, 3.3) for ax in ec.AXES.values()] + [ec._quat([1, 1, 0.0], 3.1), ec._quat([0.1, 1, 1], 3.1)]
    assert {m2q_branch(q) for q in qs} == {0, 1, 2, 3}
    worst = max(lx.ratio(lx.to_np(lx.rot_of_quat(row)), lx.rot_of_quat(q)) for q, row in zip(qs, lie_host([("m2q", q) for q in qs])))
    print(f"host m2q(q2m(q)): worst ratio {worst:.2f}")
    assert worst <= K_M2Q, worst


def test_host_chart_maps_near_the_pole(lie_host):
    """so3FromVectors / sphereRotQ / stereoChartDiff / stereoChartInvDiffAtZero / stereoChart at 0.5 .. 2e-4 rad from the pole against the
    reference in the bound form K (u / theta^2) scale with the oracle's K; `bad` stays 0.  sphereRotQ's axis lies in the xy-plane: only
    so3FromVectors on general pairs takes m2q's m22-largest branch, checked with them."""
    dirs = ec.pole_directions()
    worst = {"Rs": 0.0, "cdiff": 0.0, "cinv": 0.0, "chart": 0.0}
    t = ec._unit([0.3, -0.8, 0.5])
    for (th, _, y), rs, cd, ci, ch in zip(dirs, lie_host([("srot", y) for _, _, y in dirs]), lie_host([("cdiff", y, y) for _, _, y in dirs]),
                                          lie_host([("cinv", y) for _, _, y in dirs]),
                                          lie_host([("chart", ec._unit(y * np.cos(1e-3) + np.cross(y, t) * np.sin(1e-3)), y) for _, _, y in dirs])):
        assert rs[-1] == 0 and cd[-1] == 0 and ci[-1] == 0 and ch[-1] == 0, th
        pole = lx.vec(y)
        worst["Rs"] = max(worst["Rs"], lx.pole_ratio(lx.to_np(lx.rot_of_quat(rs[0:4])), lx.sphere_rot(pole), th))
        worst["cdiff"] = max(worst["cdiff"], lx.pole_ratio(cd[0:6], lx.chart_diff(pole, pole), th))
        worst["cinv"] = max(worst["cinv"], lx.pole_ratio(ci[0:6], lx.chart_inv_diff_at_zero(pole), th, 2.0))
        eta = lx.vec(ec._unit(y * np.cos(1e-3) + np.cross(y, t) * np.sin(1e-3)))
        worst["chart"] = max(worst["chart"], lx.pole_ratio(ch[0:2], lx.chart(eta, pole), th))
    print("host chart maps near the pole, ratio to (u / theta^2) scale: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    # R_s and its two differentials are the C0 / Bg / Avg of the yardstick without their outer factors
    assert worst["Rs"] <= ec.K_POLE["C0"] and worst["cdiff"] <= ec.K_POLE["Bg"] and worst["cinv"] <= ec.K_POLE["Avg"]
    assert worst["chart"] <= ec.K_POLE["delta"]
    # so3FromVectors between general directions, up to 3.0 rad apart
    rng = np.random.default_rng(5)
    pairs = [(rng.standard_normal(3), rng.standard_normal(3)) for _ in range(24)] + [(ec.rotate(ax, 3.0, o), o) for ax, o in
                                                                                      (([0, 0, 1.0], [1.0, 0.2, 0]), ([1.0, 0, 0], [0, 0.3, 1.0]), ([0, 1.0, 0], [0.2, 0, 1.0]))]
    br = set()
    for (o, dd), row in zip(pairs, lie_host([("so3fv", o, dd) for o, dd in pairs])):
        assert row[-1] == 0
        c = float(ec._unit(o) @ ec._unit(dd))
        r = lx.ratio(lx.to_np(lx.rot_of_quat(row[0:4])), lx.rot_a_to_b(lx.vec(o), lx.vec(dd)))
        assert r <= 8 + 8 / (1 + c), (o, dd, r)  # (the formula's own u / (1 + c), three products deep)
        br.add(m2q_branch(row[0:4]))
    assert br == {0, 1, 2, 3}, br


def test_host_bad_flag_threshold(lie_host):
    """|1 + c| <= 1e-8: on the host 1.4e-4 rad from the pole sets `bad` and 1.5e-4 does not; the flag cases of the GPU test (<= 1e-4) are a
    factor 2 inside, its pole cases (>= 2e-4) a factor 2 outside."""
    ths = [0.0, 1e-5, 1e-4, 1.4e-4, 1.5e-4, 2e-4]
    for th, want in zip(ths, [1, 1, 1, 1, 0, 0]):
        dirs = ec.pole_directions((th,))
        for row in lie_host([("srot", y) for _, _, y in dirs]) + lie_host([("cdiff", y, y) for _, _, y in dirs]) + lie_host([("cinv", y) for _, _, y in dirs]):
            assert row[-1] == want, (th, row)
        one_plus_c = 1 - np.cos(th)
        assert (one_plus_c <= 5e-9) if th <= 1e-4 else True
        assert (one_plus_c >= 2e-8 * 0.999) if th >= 2e-4 else True


# ------------------------------------------------------------------------------------------------------------------------------------------
# (d)
# ------------------------------------------------------------------------------------------------------------------------------------------
def test_reference_sees_a_wrong_closed_form_B():
    """so3Exp with B from four series terms above the seam (1e-9 off at t = 0.25, far off beyond): outside the A.R bound at every propagate
    angle above the seam, while the right closed form is inside."""
    for th in (0.5001, 1.0, 2.2, 3.0, 3.3):
        w = th * ec._unit(ec.AXES["g"])
        t = th * th
        wx = en.skew(w)
        Rref = lx.so3_exp(lx.vec(w))
        good = np.eye(3) + np.sin(th) / th * wx + (1 - np.cos(th)) / t * wx @ wx
        bad = np.eye(3) + np.sin(th) / th * wx + (0.5 - t / 24 + t * t / 720 - t ** 3 / 40320) * wx @ wx
        K = ec.K_STEP[True][ec.angle_class(th)]["A.R"]
        assert lx.ratio(good, Rref) <= K
        assert lx.ratio(bad, Rref) > 100 * K, th


def test_reference_sees_a_transposed_chart_rotation():
    for th, _, y in ec.pole_directions():
        Rs = en.so3_from_vectors_matrix(-y, en.E3)
        ref = lx.sphere_rot(lx.vec(y))
        assert lx.pole_ratio(Rs, ref, th) <= ec.K_POLE["C0"]
        assert lx.pole_ratio(Rs.T, ref, th) > 100 * ec.K_POLE["C0"], th


def m2q_swapped(m):
    """Eigen's matrix -> quaternion with the bodies of the m11-largest and the m22-largest branch exchanged."""
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0 or (m[0, 0] >= m[1, 1] and m[0, 0] >= m[2, 2]):
        return en.quat_from_matrix(m)
    i = 2 if m[1, 1] >= m[2, 2] else 1  # (swapped)
    j, k = (i + 1) % 3, (i + 2) % 3
    q = np.zeros(4)
    with np.errstate(all="ignore"):
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q[1 + i] = 0.5 * t
        t = 0.5 / t
        q[0], q[1 + j], q[1 + k] = (m[k, j] - m[j, k]) * t, (m[j, i] + m[i, j]) * t, (m[k, i] + m[i, k]) * t
    return q


def test_reference_sees_a_swapped_m2q_branch():
    """Every branch of m2q is algebraically valid wherever its pivot is not zero, so a swapped branch shows on rotations about (nearly) ONE
    axis: 3.0 and 3.3 rad about y and z, the propagate cases' axes, tilted by 3e-6 rad so that the exchanged branch divides by a pivot of
    ~1e-6 instead of 0 and returns a finite rotation -- which falls outside K_M2Q by value; exactly on the axis it returns NaN."""
    for th in (3.0, 3.3):
        for an, tilt in (("y", [3e-6, 0, 2e-6]), ("z", [2e-6, -3e-6, 0])):
            q = ec._quat(ec.AXES[an] + np.array(tilt), th)
            M = en.quat_to_matrix(q)
            ref = lx.rot_of_quat(q)
            assert m2q_branch(q) == {"y": 2, "z": 3}[an]
            assert lx.ratio(en.quat_to_matrix(en.quat_from_matrix(M)), ref) <= K_M2Q
            got = en.quat_to_matrix(m2q_swapped(M))
            r = lx.ratio(got, ref)
            print(f"m2q with swapped branches, {th} rad about {an} + 3e-6: ratio {r:.3g}")
            assert np.all(np.isfinite(got)) and r > 100 * K_M2Q, (th, an, r)
            exact = en.quat_to_matrix(m2q_swapped(en.quat_to_matrix(ec._quat(ec.AXES[an], th))))
            assert not np.all(np.isfinite(exact)) or lx.ratio(exact, ref) > 100 * K_M2Q
