"""The covariance in the coordinates of the estimate on the device (csrc/eqf_local.hpp: eqf_get_sigma_local, eqf_get_marginals,
eqf_get_local_jacobian) against J Sigma J^T formed in numpy from the device's OWN sigma(), origin() and group() with the oracle's chart
functions; no side effects on the filter; error paths; the C++ facade's members against the Python binding bit for bit."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from consistency_helpers import chart_jacobian_blocks_oracle

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip():
    from eqf_vio_amd import binding

    return binding


def _run(fg, st, frames, meas=None, nb=None, ids=None):
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
                fg.process_vision(st.vision_stamps[k], st.ids if ids is None else ids, st.bearings[k], nb=nb)
            seen += 1
            if seen == frames:
                break
    assert seen == frames


def _check_filter(fg, b, what):
    """sigma_local / local_jacobian / marginals of filter b; returns the largest |diff| / (256 u (|J| |Sigma| |J|^T)) seen."""
    from eqf_vio_amd import consistency

    S, origin, group, ids = fg.sigma(b), fg.origin(b), fg.group(b), fg.ids(b)
    N = len(ids)
    J = chart_jacobian_blocks_oracle(origin, group, ids)
    want = J @ S @ J.T
    bound = 256 * U * (np.abs(J) @ np.abs(S) @ np.abs(J).T)
    Sl = fg.sigma_local(b)
    assert Sl.shape == want.shape == (11 + 3 * N, 11 + 3 * N)
    diff = np.abs(Sl - want)
    ratio = float((diff[bound > 0] / bound[bound > 0]).max())
    print(f"{what} b={b} N={N}: |J|max {np.abs(J).max():.3f}, max |diff| / bound {ratio:.4f} (i.e. {256 * ratio:.2f} u)")
    assert np.all(diff <= bound), (what, b, ratio)
    assert np.all(diff[bound == 0] == 0)
    # the J blocks as the device built them, against the host module: 64 u of the block's largest entry
    dj, hj = fg.local_jacobian(b), consistency.local_jacobian_blocks(origin, group)
    assert np.abs(dj["G"] - hj["G"]).max() <= 64 * U * np.abs(hj["G"]).max(), (what, b)
    assert np.abs(dj["RAt"] - hj["RAt"]).max() <= 64 * U * np.abs(hj["RAt"]).max(), (what, b)
    assert dj["lm"].shape == hj["lm"].shape == (N, 3, 3)
    for i in range(N):
        assert np.abs(dj["lm"][i] - hj["lm"][i]).max() <= 64 * U * np.abs(hj["lm"][i]).max(), (what, b, i)
    # marginals: bit for bit the blocks of sigma() / sigma_local()
    for local, M in ((0, S), (1, Sl)):
        mg = fg.marginals(b, local=bool(local))
        assert np.array_equal(mg["base"], M[:11, :11]), (what, b, local)
        assert mg["lm"].shape == (N, 3, 3)
        for i in range(N):
            assert np.array_equal(mg["lm"][i], M[11 + 3 * i: 14 + 3 * i, 11 + 3 * i: 14 + 3 * i]), (what, b, local, i)
    return ratio


@pytest.mark.parametrize("N", [1, 5, 16, 17, 64, 200])
def test_sigma_local_against_numpy_from_the_devices_own_state(hip, N):
    """|sigma_local - J Sigma J^T|_ij <= 256 * 2^-53 * (|J| |Sigma| |J|^T)_ij after five vision frames, capacity > N.  (Two three-term
    dot-product stages per entry and side ~12 u, the J entries from quaternion -> matrix and one division ~20 u, the gravity block's chart
    differentials ~60 flops: 256 u leaves a factor 2 - 4.)"""
    from eqf_vio_amd import synth

    st = synth.make_stream(N, duration=0.4)
    fg = hip.FilterBatch(synth.template_settings_dict(), capacity=N + 7, batch=1)
    _run(fg, st, 5)
    _check_filter(fg, 0, "stream")
    assert fg.device_error() == 0


def test_sigma_local_in_a_batch_with_different_landmark_counts(hip):
    from eqf_vio_amd import synth

    N = 40
    st = synth.make_stream(N, duration=0.4)
    fg = hip.FilterBatch(synth.template_settings_dict(), capacity=48, batch=3)
    _run(fg, st, 4, nb=[40, 17, 5])
    assert [fg.num_landmarks(b) for b in range(3)] == [40, 17, 5]
    for b in (2, 0, 1):
        _check_filter(fg, b, "batch")
    assert fg.device_error() == 0


def test_sigma_local_after_landmark_churn(hip):
    from eqf_vio_amd import synth

    N = 30
    st = synth.make_stream(N, duration=0.6)
    meas = synth.churn_measurements(st, seed=7)
    fg = hip.FilterBatch(synth.template_settings_dict(), capacity=N, batch=1)
    _run(fg, st, 10, meas=meas)
    assert not np.array_equal(fg.ids(0), st.ids)  # (landmarks have come and gone: the state is not the stream's full, ordered set)
    _check_filter(fg, 0, "churn")
    assert fg.device_error() == 0


def test_no_landmarks_gives_the_base_part_only(hip):
    from eqf_vio_amd import synth

    st = synth.make_stream(4, duration=0.1)
    fg = hip.FilterBatch(synth.template_settings_dict(), capacity=8, batch=1)
    for r in st.imu[:6]:
        fg.process_imu(r[0], r[1:4], r[4:7])
    assert fg.num_landmarks(0) == 0
    assert _check_filter(fg, 0, "no landmarks") >= 0.0
    assert fg.sigma_local(0).shape == (11, 11) and fg.marginals(0)["lm"].shape == (0, 3, 3)


def _all_getters(fg, b=0):
    d = fg.dump_state(b)
    out = [d["ids"], d["origin"]["q"], d["origin"]["x"], d["origin"]["v"], d["origin"]["p"], d["group"]["Aq"], d["group"]["Ax"], d["group"]["w"],
           d["group"]["Qq"], d["group"]["Qa"], d["bias"], d["sigma"], np.array([d["time"], d["accumulatedTime"], d["initialised"]]),
           d["currentVelocity"], d["accumulatedVelocity"]]
    e, lu = fg.state_estimate(b), fg.last_update(b)
    return out + [e["q"], e["x"], e["v"], e["p"], lu["delta"], lu["gamma"], lu["Gamma"]]


def test_the_new_getters_leave_the_filter_bit_for_bit_alone(hip):
    """sigma() and every other getter before and after sigma_local() / marginals() / local_jacobian(); and a handle on which they are
    called after every frame stays bit for bit on a handle that never saw them."""
    from eqf_vio_amd import synth

    N = 33
    st = synth.make_stream(N, duration=0.5)
    d = synth.template_settings_dict()
    fa, fb = hip.FilterBatch(d, capacity=N, batch=1), hip.FilterBatch(d, capacity=N, batch=1)
    for kind, k in st.events():
        if kind == "imu":
            r = st.imu[k]
            fa.process_imu(r[0], r[1:4], r[4:7])
            fb.process_imu(r[0], r[1:4], r[4:7])
        else:
            fa.process_vision(st.vision_stamps[k], st.ids, st.bearings[k])
            fb.process_vision(st.vision_stamps[k], st.ids, st.bearings[k])
            before = _all_getters(fa)
            fa.sigma_local(0)
            fa.marginals(0, local=True)
            fa.marginals(0, local=False)
            fa.local_jacobian(0)
            for x, y in zip(before, _all_getters(fa)):
                assert np.array_equal(x, y), k
    for x, y in zip(_all_getters(fa), _all_getters(fb)):
        assert np.array_equal(x, y)
    assert fa.device_error() == 0 and fb.device_error() == 0


def test_error_paths_leave_the_handle_usable(hip):
    from eqf_vio_amd import synth

    N = 6
    st = synth.make_stream(N, duration=0.3)
    d = synth.template_settings_dict()
    L = hip.lib()
    dp = C.POINTER(C.c_double)
    n = 11 + 3 * N
    buf, base, lm, G, R = np.zeros((n, n)), np.zeros((11, 11)), np.zeros((N, 3, 3)), np.zeros((2, 2)), np.zeros((3, 3))

    def p(a):
        return a.ctypes.data_as(dp)

    # an fp32 handle: EQF_ERR_UNSUPPORTED before any effect
    f32 = hip.FilterBatch(d, capacity=N, batch=1, precision=hip.PRECISION_F32)
    _run(f32, st, 3)
    S0 = f32.sigma(0)
    stats = hip.InnovationStats()
    assert L.eqf_get_sigma_local(f32._h, 0, p(buf), n) == hip.ERR_UNSUPPORTED
    assert L.eqf_get_marginals(f32._h, 0, 1, p(base), p(lm)) == hip.ERR_UNSUPPORTED
    assert L.eqf_get_local_jacobian(f32._h, 0, p(G), p(R), p(lm)) == hip.ERR_UNSUPPORTED
    assert L.eqf_set_option(f32._h, b"innovation_stats", 1) == hip.ERR_UNSUPPORTED
    assert L.eqf_get_innovation_stats(f32._h, 0, C.byref(stats), None) == hip.ERR_UNSUPPORTED
    assert np.array_equal(f32.sigma(0), S0) and f32.device_error() == 0
    _run_more = st.imu[-1]
    f32.process_imu(_run_more[0] + 1.0, _run_more[1:4], _run_more[4:7])
    assert f32.device_error() == 0
    # an fp64 handle: EQF_ERR_INVALID for a bad filter index, a NULL output, ld < n
    fg = hip.FilterBatch(d, capacity=N, batch=2)
    _run(fg, st, 3)
    S0 = fg.sigma(1)
    for b in (-1, 2):
        assert L.eqf_get_sigma_local(fg._h, b, p(buf), n) == hip.ERR_INVALID
        assert L.eqf_get_marginals(fg._h, b, 1, p(base), p(lm)) == hip.ERR_INVALID
        assert L.eqf_get_local_jacobian(fg._h, b, p(G), p(R), p(lm)) == hip.ERR_INVALID
        assert L.eqf_get_innovation_stats(fg._h, b, C.byref(stats), None) == hip.ERR_INVALID
    assert L.eqf_get_sigma_local(fg._h, 0, None, n) == hip.ERR_INVALID
    assert L.eqf_get_sigma_local(fg._h, 0, p(buf), n - 1) == hip.ERR_INVALID
    assert L.eqf_get_marginals(fg._h, 0, 1, None, p(lm)) == hip.ERR_INVALID
    assert L.eqf_get_marginals(fg._h, 0, 1, p(base), None) == hip.ERR_INVALID
    assert L.eqf_get_marginals(fg._h, 0, 2, p(base), p(lm)) == hip.ERR_INVALID
    assert L.eqf_get_local_jacobian(fg._h, 0, None, p(R), p(lm)) == hip.ERR_INVALID
    assert L.eqf_get_local_jacobian(fg._h, 0, p(G), None, p(lm)) == hip.ERR_INVALID
    assert L.eqf_get_local_jacobian(fg._h, 0, p(G), p(R), None) == hip.ERR_INVALID
    assert L.eqf_get_innovation_stats(fg._h, 0, None, None) == hip.ERR_INVALID
    assert L.eqf_set_option(fg._h, b"innovation_stats", 2) == hip.ERR_INVALID
    assert L.eqf_get_sigma_local(None, 0, p(buf), n) == hip.ERR_INVALID
    assert np.array_equal(fg.sigma(1), S0)
    _check_filter(fg, 1, "after the rejected calls")
    assert fg.device_error() == 0


def test_cpp_facade_members_against_the_python_binding_bit_for_bit(hip):
    """VIOFilter::stateCovarianceLocal / innovationStats of cpp/VIOFilter.h through the example binary (argument `local`, values printed as
    hexadecimal floats) against filter.VIOFilter on the same sequence."""
    from eqf_vio_amd import filter as vf

    N, frames = 12, 6
    exe = os.path.join(ROOT, "eqf_vio_amd", "cpp", "eqf_example")
    out = subprocess.run([exe, str(N), str(frames), "local"], capture_output=True, text=True, check=True).stdout.splitlines()
    inn = [ln for ln in out if ln.startswith("innovation ")][0].split()[1:]
    sl = [ln for ln in out if ln.startswith("sigma_local ")][0].split()[1:]
    st = hip.settings_from_dict(dict(initialPointVariance=5000.0, measurementVariance=0.003, velOmegaVariance=1e-4, velAccelVariance=1e-4,
                                    outlierThreshold=1e9))
    fg = vf.VIOFilter(st, capacity=N)
    fg.set_option("innovation_stats", 1)
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
    s = fg.innovationStats()
    assert s["valid"] and int(inn[3]) == s["dof"] == 2 * N
    assert [float.fromhex(x) for x in inn[0:3]] == [s["nis"], s["logdet_S"], s["loglik"]]
    assert np.array_equal(np.array([float.fromhex(x) for x in inn[4:]]), s["nis_lm"])
    Sl = fg.stateCovarianceLocal()
    assert int(sl[0]) == 11 + 3 * N
    assert np.array_equal(np.array([float.fromhex(x) for x in sl[1:]]).reshape(Sl.shape), Sl)
