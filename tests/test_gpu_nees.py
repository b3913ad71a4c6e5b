"""Joint NEES, log det and definiteness of the covariance on the device (csrc/eqf_nees.hpp: eqf_get_nees, FilterBatch.nees) against numpy's
Cholesky of the matrix the device factored, taken from the device's OWN getter (sigma(b) / sigma_local(b)), symmetrised from its lower
triangle and cut at `first`.

Tolerance: relative n u kappa_2(A) on nees and min_pivot, absolute n u kappa_2(A) on logdet, u = 2^-53, kappa_2 computed here -- the
first-order bound of a backward-stable Cholesky solve with its constant set to 1 (both sides carry such an error).  So that it cannot hide
a real error, every stream case asserts that the tolerance is <= 1e-5 and that scaling A by 1.001 moves the reference nees by more than
100 tolerances.  Every case prints its largest observed ratio |device - numpy| / bound."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIRSTS = (0, 6, 11)


@pytest.fixture(scope="module")
def hip():
    from eqf_vio_amd import binding

    return binding


def _run(fg, st, frames, meas=None, nb=None):
    """`frames` vision frames of the stream through the per-call interface."""
    seen = 0
    for kind, k in st.events():
        if kind == "imu":
            r = st.imu[k]
            fg.process_imu(r[0], r[1:4], r[4:7])
        else:
            if meas is not None:
                fg.process_vision(st.vision_stamps[k], *meas[k])
            else:
                fg.process_vision(st.vision_stamps[k], st.ids, st.bearings[k], nb=nb)
            seen += 1
            if seen == frames:
                break
    assert seen == frames


def _cut(S, first):
    A = np.tril(S[first:, first:])
    return A + np.tril(A, -1).T


def _reference(S, first, E):
    """numpy's factorisation of the cut matrix: nees per row of E, logdet, min_pivot, the order n and the tolerance n u kappa_2."""
    A = _cut(S, first)
    n = A.shape[0]
    if n == 0:
        return dict(nees=np.zeros(len(E)), logdet=0.0, min_pivot=np.inf, n=0, tol=0.0, A=A)
    L = np.linalg.cholesky(A)
    z = np.linalg.solve(L, E[:, first:].T)
    d = np.diag(L)
    return dict(nees=np.sum(z * z, axis=0), logdet=2.0 * float(np.log(d).sum()), min_pivot=float((d * d).min()), n=n,
                tol=n * U * float(np.linalg.cond(A)), A=A)


def _errors(S, nrhs, seed):
    """Seeded normal times sqrt(diag A)."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nrhs, S.shape[0])) * np.sqrt(np.abs(np.diag(S)))


def _compare(got, b, k, ref, what, stream=True):
    """Outputs of filter b (its first k error vectors) against the reference; returns the largest |diff| / bound."""
    tol = ref["tol"]
    assert got["info"][b] == 0 and got["dof"][b] == ref["n"], (what, got["info"][b], got["dof"][b])
    if ref["n"] == 0:
        assert np.all(got["nees"][b] == 0.0) and got["logdet"][b] == 0.0 and got["min_pivot"][b] == np.inf, what
        return 0.0
    if stream:
        assert tol <= 1e-5, (what, tol)
    ratios = [abs(got["logdet"][b] - ref["logdet"]) / tol, abs(got["min_pivot"][b] - ref["min_pivot"]) / (tol * ref["min_pivot"])]
    ratios += list(np.abs(got["nees"][b, :k] - ref["nees"][:k]) / (tol * ref["nees"][:k]))
    worst = float(max(ratios))
    assert worst <= 1.0, (what, worst, tol, got["logdet"][b], ref["logdet"], got["nees"][b, :k], ref["nees"][:k])
    return worst


def _check_handle(fg, what, seed=11):
    """Every filter of the handle, both charts, the three cuts, nrhs = 1 and 16.  Returns the largest ratio seen."""
    B = fg.B
    worst = 0.0
    for local in (0, 1):
        S = [fg.sigma_local(b) if local else fg.sigma(b) for b in range(B)]
        E = [_errors(S[b], 16, seed + b) for b in range(B)]
        for first in FIRSTS:
            ref = [_reference(S[b], first, E[b]) for b in range(B)]
            for b in range(B):  # the tolerance cannot hide a real error: A -> 1.001 A moves the reference by more than 100 tolerances
                if ref[b]["n"] > 0:
                    moved = _reference(1.001 * _cut(S[b], first), 0, E[b][:, first:])["nees"]
                    assert np.all(np.abs(moved - ref[b]["nees"]) > 100 * ref[b]["tol"] * ref[b]["nees"]), (what, local, first, b)
            for nrhs in (1, 16):
                got = fg.nees([e[:nrhs] for e in E], local=bool(local), first=first)
                assert got["nees"].shape == (B, nrhs)
                for b in range(B):
                    r = _compare(got, b, nrhs, ref[b], (what, local, first, nrhs, b))
                    worst = max(worst, r)
            print(f"{what} local={local} first={first}: n {[r['n'] for r in ref]}, bound {[float('%.2e' % r['tol']) for r in ref]}")
    print(f"{what}: largest |device - numpy| / bound {worst:.3e}")
    assert fg.device_error() == 0
    return worst


@pytest.mark.parametrize("N", [1, 17, 18, 39, 64, 200])
def test_nees_against_numpy_cholesky_of_the_devices_own_matrix(hip, N):
    """Internal orders 15, 63, 66, 129, 204 (192 with first = 11) and 612: below one block, either side of the first block boundary, just
    past the second, an exact multiple, ten block columns with a ragged last one."""
    from eqf_vio_amd import synth

    st = synth.make_stream(N, duration=0.4)
    fg = hip.FilterBatch(synth.template_settings_dict(), capacity=N + 7, batch=1)
    _run(fg, st, 5)
    assert fg.num_landmarks(0) == N
    _check_handle(fg, f"stream N={N}")


def _no_landmarks(hip, batch=1):
    from eqf_vio_amd import synth

    st = synth.make_stream(4, duration=0.4)
    fg = hip.FilterBatch(synth.template_settings_dict(), capacity=7, batch=batch)
    for r in st.imu[:60]:
        fg.process_imu(r[0], r[1:4], r[4:7])
    assert fg.num_landmarks(0) == 0
    return fg


def test_a_filter_without_landmarks_answers_for_its_base_part(hip):
    fg = _no_landmarks(hip)
    _check_handle(fg, "no landmarks")
    got = fg.nees(None, local=True, first=11)
    assert got["nees"].shape == (1, 0) and got["dof"][0] == 0 and got["logdet"][0] == 0.0 and got["info"][0] == 0


def test_a_batch_of_four_with_different_landmark_counts_in_one_call(hip):
    from eqf_vio_amd import synth

    st = synth.make_stream(70, duration=0.4)
    fg = hip.FilterBatch(synth.template_settings_dict(), capacity=77, batch=4)
    _run(fg, st, 5, nb=[0, 5, 18, 70])
    assert [fg.num_landmarks(b) for b in range(4)] == [0, 5, 18, 70]
    _check_handle(fg, "batch 0/5/18/70")


def _churned(hip):
    """Ten frames of the 0.6 s stream at capacity N, as tests/test_gpu_local.py runs its churn case (not the five frames at capacity N + 7 of
    the stream cases): long enough for landmarks to have entered AND left, and a filter that has run full is the harder state."""
    from eqf_vio_amd import synth

    N = 30
    st = synth.make_stream(N, duration=0.6)
    meas = synth.churn_measurements(st, seed=7)
    fg = hip.FilterBatch(synth.template_settings_dict(), capacity=N, batch=1)
    _run(fg, st, 10, meas=meas)
    assert not np.array_equal(fg.ids(0), st.ids)
    return fg


def test_a_filter_after_landmark_churn(hip):
    _check_handle(_churned(hip), "churn")


def _truth(st, f):
    """The stream's analytic truth at vision frame f as a state dict (body velocity, camera-frame landmarks); as in test_consistency.py."""
    from eqf_vio_amd import synth
    from oracle import eqf_numpy as O

    t = np.array([st.vision_stamps[f]])
    p, pd, _, R, _ = synth._trajectory(t)
    R, p, pd = R[0], p[0], pd[0]
    RIC = synth._quat_to_matrix(synth.CAM_OFFSET_Q)
    body = (R.T @ (st.landmarks_world - p).T).T
    cam = (RIC.T @ (body - synth.CAM_OFFSET_X).T).T
    return dict(q=O.quat_from_matrix(R), v=R.T @ pd, p=cam)


@pytest.fixture(scope="module")
def stream30(hip):
    from eqf_vio_amd import synth

    N = 30
    st = synth.make_stream(N, duration=0.4)
    fg = hip.FilterBatch(synth.template_settings_dict(), capacity=N + 7, batch=1)
    fg.set_option("innovation_stats", 1)
    _run(fg, st, 5)
    return st, fg


def test_the_real_error_of_the_streams_analytic_truth(hip, stream30):
    from eqf_vio_amd import consistency

    st, fg = stream30
    err = consistency.local_error(fg.state_estimate(0), _truth(st, 4), bias=fg.bias(0), true_bias=np.array([0.01] * 3 + [0.05] * 3))
    e = consistency.error_vector(err)
    assert e.shape == (11 + 3 * 30,)
    Sl = fg.sigma_local(0)
    for first in FIRSTS:
        ref = _reference(Sl, first, e[None, :])
        got = fg.nees(e[None, None, :], local=True, first=first)
        r = _compare(got, 0, 1, ref, ("truth", first))
        host = consistency.nees_joint(Sl, e, first=first)
        assert abs(host["nees"] - ref["nees"][0]) <= ref["tol"] * ref["nees"][0] and host["dof"] == got["dof"][0]
        print(f"truth first={first}: NEES / dof {got['nees'][0, 0] / got['dof'][0]:.3g}, ratio to bound {r:.3e}")


def test_chart_invariance(hip, stream30):
    """nees(local=1, J e) = nees(local=0, e) and logdet_local - logdet_origin = 2 sum log |det J_block| over the blocks from `first` on, each
    within the sum of the two tolerances."""
    from eqf_vio_amd import consistency

    _, fg = stream30
    S, Sl, blk = fg.sigma(0), fg.sigma_local(0), fg.local_jacobian(0)
    J = consistency.jacobian_matrix(blk)
    e = _errors(S, 4, 5)
    Je = e @ J.T
    for first in FIRSTS:
        t0, t1 = _reference(S, first, e)["tol"], _reference(Sl, first, Je)["tol"]
        g0, g1 = fg.nees(e[None], local=False, first=first), fg.nees(Je[None], local=True, first=first)
        assert g0["info"][0] == 0 and g1["info"][0] == 0
        assert np.all(np.abs(g1["nees"][0] - g0["nees"][0]) <= (t0 + t1) * g0["nees"][0]), (first, g0["nees"], g1["nees"])
        dets = [np.linalg.det(b) for b in blk["lm"]] + ([np.linalg.det(blk["G"]), np.linalg.det(blk["RAt"])] if first < 11 else [])
        want = 2.0 * float(np.sum(np.log(np.abs(dets))))
        assert abs((g1["logdet"][0] - g0["logdet"][0]) - want) <= t0 + t1, (first, g1["logdet"][0] - g0["logdet"][0], want)


def test_marginal_consistency_without_landmarks(hip):
    """With no landmarks the joint NEES is the navigation-state NEES of the marginals."""
    from eqf_vio_amd import consistency

    fg = _no_landmarks(hip)
    rng = np.random.default_rng(3)
    Sl = fg.sigma_local(0)
    v = rng.standard_normal(11) * np.sqrt(np.diag(Sl))
    err = dict(bias=v[0:6], gravity=v[6:8], velocity=v[8:11], lm=np.zeros((0, 3)))
    want = consistency.nees_marginal(fg.marginals(0, local=True), err)["nav"]
    got = fg.nees([consistency.error_vector(err)[None, :]], local=True, first=0)
    assert got["dof"][0] == 11 and abs(got["nees"][0, 0] - want) <= 1e-10 * want, (got["nees"], want)


def _same(a, b, rows=None):
    for key in ("nees", "logdet", "min_pivot", "dof", "info"):
        x, y = (a[key], b[key]) if rows is None else (a[key][rows[0]], b[key][rows[1]])
        assert np.array_equal(x, y, equal_nan=True), (key, x, y)


def test_bit_for_bit_from_run_to_run_and_wherever_the_filter_sits(hip):
    from eqf_vio_amd import synth

    fg = _churned(hip)
    d = synth.template_settings_dict()
    snap = fg.dump_state(0)
    n = 11 + 3 * fg.num_landmarks(0)
    E = _errors(fg.sigma_local(0), 16, 2)
    one, four = hip.FilterBatch(d, capacity=41, batch=1), hip.FilterBatch(d, capacity=33, batch=4)
    one.restore_state(snap, 0)
    four.restore_state(snap, 2)
    E4 = np.zeros((4, 16, n))
    E4[2] = E
    for local in (False, True):
        for first in FIRSTS:
            a = fg.nees(E[None], local=local, first=first)
            _same(a, fg.nees(E[None], local=local, first=first))
            _same(a, one.nees(E[None], local=local, first=first))
            _same(a, four.nees(E4, local=local, first=first), rows=(0, 2))
            assert a["info"][0] == 0


def _getters(fg):
    e = fg.state_estimate(0)
    s = fg.innovation_stats(0)
    return [fg.sigma(0), e["q"], e["x"], e["v"], e["p"], np.array([s["nis"], s["logdet_S"], s["loglik"], s["dof"], s["valid"]]), s["nis_lm"]]


def test_no_side_effects(hip):
    """sigma(b), state_estimate(b) and innovation_stats unchanged by the call; a twin handle that never calls nees stays bit for bit in Sigma
    over three further frames."""
    from eqf_vio_amd import synth

    N = 21
    st = synth.make_stream(N, duration=0.5)
    d = synth.template_settings_dict()
    fa, fb = hip.FilterBatch(d, capacity=N + 7, batch=1), hip.FilterBatch(d, capacity=N + 7, batch=1)
    seen = 0
    for f in (fa, fb):
        f.set_option("innovation_stats", 1)
    for kind, k in st.events():
        if kind == "imu":
            r = st.imu[k]
            fa.process_imu(r[0], r[1:4], r[4:7])
            fb.process_imu(r[0], r[1:4], r[4:7])
            continue
        fa.process_vision(st.vision_stamps[k], st.ids, st.bearings[k])
        fb.process_vision(st.vision_stamps[k], st.ids, st.bearings[k])
        seen += 1
        if seen >= 5:
            before = _getters(fa)
            assert before[5][4] == 1
            E = _errors(before[0], 3, k)
            for local in (False, True):
                for first in FIRSTS:
                    assert fa.nees(E[None], local=local, first=first)["info"][0] == 0
            for x, y in zip(before, _getters(fa)):
                assert np.array_equal(x, y), k
            assert np.array_equal(fa.sigma(0), fb.sigma(0)), k
        if seen == 8:
            break
    assert seen == 8 and fa.device_error() == 0 and fb.device_error() == 0


def _random_spd(n, kappa, seed):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (Q * np.logspace(0, -math.log10(kappa), n)) @ Q.T
    return 0.5 * (A + A.T)


def test_definiteness_is_reported_per_filter(hip):
    """Through set_sigma at N = 70 (order 221, internal 222: four block columns): diag(d) with one entry -1 at reference index 3, 100 and the
    last -> info = 1 and NaN outputs for that filter only, its batch neighbours bit for bit what they were, device_error() still 0; a
    random SPD matrix with kappa = 1e6 passes within the bound."""
    from eqf_vio_amd import synth

    N = 70
    n = 11 + 3 * N
    st = synth.make_stream(N, duration=0.4)
    fg = hip.FilterBatch(synth.template_settings_dict(), capacity=N + 7, batch=3)
    _run(fg, st, 2)
    rng = np.random.default_rng(9)
    E = rng.standard_normal((3, 2, n))
    good = fg.nees(E, local=False, first=0)
    assert np.all(good["info"] == 0)
    for idx in (3, 100, n - 1):
        d = 1.0 + rng.random(n)
        d[idx] = -1.0
        fg.set_sigma(np.diag(d), 1)
        got = fg.nees(E, local=False, first=0)
        assert list(got["info"]) == [0, 1, 0] and got["dof"][1] == n, (idx, got["info"])
        assert np.isnan(got["logdet"][1]) and np.isnan(got["min_pivot"][1]) and np.all(np.isnan(got["nees"][1])), idx
        _same(good, got, rows=(0, 0))
        _same(good, got, rows=(2, 2))
        assert fg.device_error() == 0
    A = _random_spd(n, 1e6, 4)
    fg.set_sigma(A, 1)
    E[1] = _errors(A, 2, 6)
    got = fg.nees(E, local=False, first=0)
    ref = _reference(fg.sigma(1), 0, E[1])
    r = _compare(got, 1, 2, ref, "random SPD", stream=False)
    print(f"random SPD n={n}: kappa_2 {np.linalg.cond(ref['A']):.3e}, bound {ref['tol']:.2e}, ratio {r:.3e}")
    _same(good, got, rows=(0, 0))
    assert fg.device_error() == 0


def test_an_uninitialised_filter_is_flagged_alone(hip):
    """local = 1 needs the gravity chart: a filter that was never initialised (level identity pose, SO3.cpp:160) answers info = -1."""
    from eqf_vio_amd import synth

    N = 5
    st = synth.make_stream(N, duration=0.4)
    d = synth.template_settings_dict()
    fg = hip.FilterBatch(d, capacity=N + 7, batch=2)
    _run(fg, st, 3)
    fg.restore_state(hip.FilterBatch(d, capacity=N + 7, batch=1).dump_state(0), 1)
    got = fg.nees(None, local=True, first=0)
    assert list(got["info"]) == [0, -1] and np.isnan(got["logdet"][1]) and np.isfinite(got["logdet"][0])
    got = fg.nees(None, local=False, first=0)
    assert list(got["info"]) == [0, 0]
    assert fg.device_error() == 0


def test_argument_errors_leave_the_outputs_untouched(hip):
    from eqf_vio_amd import synth

    N = 6
    n = 11 + 3 * N
    st = synth.make_stream(N, duration=0.3)
    d = synth.template_settings_dict()
    L = hip.lib()
    dp = C.POINTER(C.c_double)
    fg = hip.FilterBatch(d, capacity=N, batch=2)
    _run(fg, st, 3)
    f32 = hip.FilterBatch(d, capacity=N, batch=2, precision=hip.PRECISION_F32)
    _run(f32, st, 3)
    E = np.ones((2, 16, n))
    out = np.full((2, 17), -7.0)
    stats = (hip.SigmaStats * 2)()
    for s in stats:
        s.logdet, s.min_pivot, s.dof, s.info = -7.0, -7.0, -7, -7

    def call(h, local=1, first=0, nrhs=1, lde=n, st_=stats, e=E, o=out):
        return L.eqf_get_nees(h, local, first, nrhs, e.ctypes.data_as(dp) if e is not None else None, lde,
                              o.ctypes.data_as(dp) if o is not None else None, st_)

    S0 = fg.sigma(1)
    assert call(fg._h, first=5) == hip.ERR_INVALID
    assert call(fg._h, nrhs=17) == hip.ERR_INVALID
    assert call(fg._h, nrhs=-1) == hip.ERR_INVALID
    assert call(fg._h, lde=n - 1) == hip.ERR_INVALID
    assert call(fg._h, st_=None) == hip.ERR_INVALID
    assert call(fg._h, local=2) == hip.ERR_INVALID
    assert call(fg._h, e=None) == hip.ERR_INVALID
    assert call(fg._h, o=None) == hip.ERR_INVALID
    assert call(None) == hip.ERR_INVALID
    assert call(f32._h) == hip.ERR_UNSUPPORTED
    assert np.all(out == -7.0)
    assert all(s.logdet == -7.0 and s.min_pivot == -7.0 and s.dof == -7 and s.info == -7 for s in stats)
    assert np.array_equal(fg.sigma(1), S0) and fg.device_error() == 0 and f32.device_error() == 0
    assert call(fg._h) == 0 and stats[0].info == 0 and stats[1].dof == n and out[0, 0] > 0.0 and out[0, 2] == -7.0


def test_cpp_facade_against_the_python_binding_bit_for_bit(hip):
    """VIOFilter::stateNEES of cpp/VIOFilter.h through the example binary (argument `nees`, values printed as hexadecimal floats) against
    filter.VIOFilter.stateNEES on the same sequence."""
    from eqf_vio_amd import filter as vf

    N, frames = 20, 6
    exe = os.path.join(ROOT, "eqf_vio_amd", "cpp", "eqf_example")
    out = subprocess.run([exe, str(N), str(frames), "nees"], capture_output=True, text=True, check=True).stdout.splitlines()
    lines = [ln.split()[1:] for ln in out if ln.startswith("nees ")]
    assert len(lines) == 6
    st = hip.settings_from_dict(dict(initialPointVariance=5000.0, measurementVariance=0.003, velOmegaVariance=1e-4, velAccelVariance=1e-4,
                                    outlierThreshold=1e9))
    fg = vf.VIOFilter(st, capacity=N)
    lm = np.array([[2 * math.sin(1.3 * i), 2 * math.cos(0.7 * i), 5 + math.sin(0.37 * i)] for i in range(N)])
    y = np.array([[v[0] / n, v[1] / n, v[2] / n] for v, n in ((v, math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])) for v in lm)])
    k = 0
    for f in range(frames):
        stamp = 0.05 * f + 0.0025
        while 0.005 * k < stamp:
            fg.processIMUData(vf.IMUVelocity(0.005 * k, np.zeros(3), np.array([9.81, 0, 0])))
            k += 1
        fg.processVisionData(vf.VisionMeasurement(stamp, np.arange(N, dtype=np.int32), y))
        fg.stateEstimate()  # (the example reads the state after every vision call)
    e = np.array([0.01 * math.sin(0.9 * i + 0.3) for i in range(11 + 3 * N)])
    for ln in lines:
        local, first, dof, info = (int(x) for x in ln[0:4])
        s = fg.stateNEES(e, local=bool(local), first=first)
        assert (dof, info) == (s["dof"], s["info"]) == (11 + 3 * N - first, 0)
        assert [float.fromhex(x) for x in ln[4:7]] == [s["nees"], s["logdet"], s["min_pivot"]], (local, first)
