"""The outlier gate of a handle (eqf_set_outlier_gate / eqf_get_gate_report, csrc/eqf_churn.hpp) against the numpy oracle with the same
gate in removeOutliers' place (tests/gate_helpers.py; tests/test_gate_oracle.py checks that expectation on the CPU and asserts that no
statistic of these histories lies near the threshold).  Tolerances are the project's own: SIGMA_TOL / POSE_TOL of test_gpu_parity.py for
the closed loop, and for a statistic the bound 4 kappa(S_ii) eps ref of test_gpu_innovation.py::_check_stats with its two eps."""
import functools
import os
import subprocess

import numpy as np
import pytest

import gate_helpers as G
from consistency_helpers import inject
from helpers import rel_fro

pytestmark = pytest.mark.gpu

SIGMA_TOL = 1e-7         # tests/test_gpu_parity.py
POSE_TOL = 1e-8
EPS_ONE_UPDATE = 2e-9    # tests/test_gpu_innovation.py
EPS_CLOSED_LOOP = 1e-7
CHORD, MAHA = 0, 1


@pytest.fixture(scope="module")
def hip():
    from eqf_vio_amd import binding

    return binding


def _check_report(rep, ref, eps, what):
    """n, ids and removed exactly; |stat - ref| <= 4 kappa(S_ii) eps ref per landmark."""
    assert len(rep["ids"]) == len(ref["ids"]), what
    assert np.array_equal(rep["ids"], ref["ids"]), what
    if len(ref["ids"]):
        tol = 4 * ref["kappa"] * eps * ref["stat"]
        print(f"{what}: n={len(ref['ids'])} removed={int(ref['removed'].sum())} stat worst diff/tol {np.max(np.abs(rep['stat'] - ref['stat']) / tol):.2e}")
        assert np.all(np.abs(rep["stat"] - ref["stat"]) <= tol), what
    assert np.array_equal(rep["removed"], ref["removed"]), what


# ---------------------------------------------------------------------------------------------------------------- 1. from an injected state
@functools.lru_cache(maxsize=None)
def _state_before_the_fourth_frame(N):
    """Three vision frames and the IMU calls up to the fourth on the device: (stream, settings, snapshot, index of the fourth frame)."""
    from eqf_vio_amd import binding, synth

    st = synth.make_stream(N, duration=0.3)
    d = synth.template_settings_dict()
    fg = binding.FilterBatch(d, capacity=N, batch=1)
    ev = list(st.events())
    vis = [i for i, (kind, _) in enumerate(ev) if kind == "vision"]
    for kind, j in ev[: vis[3]]:
        if kind == "imu":
            fg.process_imu(st.imu[j, 0], st.imu[j, 1:4], st.imu[j, 4:7])
        else:
            fg.process_vision(st.vision_stamps[j], st.ids, st.bearings[j])
    snap = fg.dump_state()
    assert fg.device_error() == 0
    return st, d, snap, ev[vis[3]][1]


@pytest.mark.parametrize("nrot", [0, 1, 3])
@pytest.mark.parametrize("N", [1, 7, 58, 59, 64, 65, 130, 300])
def test_report_against_numpy_from_an_injected_state(hip, N, nrot):
    """One vision frame with nrot bearings turned by 0.2 rad, on the device and in numpy from the same state.  N = 58 takes the separate
    launches (speculative probe), 59 on k_edit (with three removals: its deferral), 64 / 65 the ballot boundary, 300 a second trip."""
    st, d, snap, j = _state_before_the_fourth_frame(N)
    rot = sorted(set([0, N // 2, N - 1][:nrot]))
    y = st.bearings[j].copy()
    for i in rot:
        y[i] = G.rotated(y[i])
    fo = inject(G.mahalanobis_filter(d, G.TAU), snap)
    fo.processVisionData(st.vision_stamps[j], st.ids, y)
    ref = fo.report
    assert list(np.flatnonzero(ref["removed"])) == rot  # (the oracle removes what was turned ...)
    assert np.min(np.abs(ref["stat"] - G.TAU)) > 1e-3 * G.TAU  # (... and nothing is near the threshold)
    fg = hip.FilterBatch(d, capacity=N, batch=1)
    fg.restore_state(snap)
    fg.set_outlier_gate(MAHA, G.TAU)
    fg.process_vision(st.vision_stamps[j], st.ids, y)
    _check_report(fg.gate_report(0), ref, EPS_ONE_UPDATE, f"N={N} nrot={nrot}")
    assert np.array_equal(fg.ids(), fo.X.ids)
    if len(fo.X.ids):
        assert rel_fro(fg.sigma(), fo.stateCovariance()) < SIGMA_TOL
    assert fg.device_error() == 0


# ---------------------------------------------------------------------------------------------------------------- 2. closed loop
def _ragged_frame(k):
    """Frame k of the three histories as the arguments of process_vision."""
    hs = [G.history(h) for h in range(3)]
    stride = max(len(m[1][k][0]) for m in hs)
    ids, y, nb = np.zeros((3, stride), dtype=np.int32), np.zeros((3, stride, 3)), np.zeros(3, dtype=np.int32)
    for b, (_, meas, _) in enumerate(hs):
        mi, my = meas[k]
        nb[b] = len(mi)
        ids[b, : len(mi)] = mi
        y[b, : len(mi)] = my
    return [h[0].vision_stamps[k] for h in hs], ids, y, nb


def _drive_ragged(fg, on_frame=None):
    sts = [G.history(h)[0] for h in range(3)]
    for kind, k in sts[0].events():
        if kind == "imu":
            fg.process_imu([s.imu[k, 0] for s in sts], [s.imu[k, 1:4] for s in sts], [s.imu[k, 4:7] for s in sts])
        else:
            stamps, ids, y, nb = _ragged_frame(k)
            fg.process_vision(stamps, ids, y, nb=nb)
            if on_frame:
                on_frame(k)


def _check_against_oracle(fg, k, with_report):
    for b in range(3):
        rec = G.oracle_run(b)[k]
        assert np.array_equal(fg.ids(b), rec["ids"]), (k, b)
        if with_report:
            _check_report(fg.gate_report(b), rec["report"], EPS_CLOSED_LOOP, f"frame {k} filter {b}")
        if len(rec["ids"]):
            assert rel_fro(fg.sigma(b), rec["sigma"]) < SIGMA_TOL, (k, b)
        e = fg.state_estimate(b)
        assert np.abs(e["x"] - rec["x"]).max() < POSE_TOL and np.abs(e["q"] - rec["q"]).max() < POSE_TOL, (k, b)


@pytest.mark.parametrize("peek", [True, False])
def test_closed_loop_ragged_batch_against_the_subclassed_oracle(hip, peek):
    """Three filters in one handle with 12 / 90 / 110 landmarks in view, churn on every few frames, injected outliers (filter 1: frames 3, 7
    and 9, two at once on 7).  Against the oracle after every frame (peek) or only at the end, when the device's answer is picked up late."""
    from eqf_vio_amd import synth

    fg = hip.FilterBatch(synth.template_settings_dict(), capacity=150, batch=3)
    fg.set_outlier_gate(MAHA, G.TAU)
    last = []
    _drive_ragged(fg, lambda k: (last.append(k), _check_against_oracle(fg, k, True) if peek else None))
    _check_against_oracle(fg, last[-1], True)
    assert fg.device_error() == 0


# ---------------------------------------------------------------------------------------------------------------- 3. one decision, three paths
def test_the_three_gate_paths_are_one_decision(hip, monkeypatch):
    """k_edit, the speculative k_probe_maha (device_edit = 0) and the synchronous one (EQF_GATE_SPECULATIVE=0): ids, Sigma, position and the
    report bit for bit equal -- three filters with churn every frame and outliers (sizes of test_one_launch_bookkeeping_equals_the_separate_launches)."""
    from eqf_vio_amd import synth

    B, pools = 3, [240, 270, 300]
    sts = [synth.make_stream(pools[b], seed=277 + b, duration=0.8) for b in range(B)]
    meas = [synth.churn_measurements(sts[b], seed=25 + b, max_visible=[150, 200, 260][b], outlier_frames=(5, 9) if b % 2 else (7,), outlier_angle=0.2)
            for b in range(B)]
    d = synth.template_settings_dict()
    stride = max(pools)
    outs = []
    for path in ("edit", "speculative_probe", "synchronous_probe"):
        if path == "synchronous_probe":
            monkeypatch.setenv("EQF_GATE_SPECULATIVE", "0")
        fg = hip.FilterBatch(d, capacity=max(pools), batch=B)
        fg.debug_option("device_edit", 1 if path == "edit" else 0)
        fg.set_outlier_gate(MAHA, G.TAU)
        seq = []
        for kind, k in sts[0].events():
            if kind == "imu":
                fg.process_imu([s.imu[k, 0] for s in sts], [s.imu[k, 1:4] for s in sts], [s.imu[k, 4:7] for s in sts])
                continue
            ids, y, nb = np.zeros((B, stride), dtype=np.int32), np.zeros((B, stride, 3)), np.zeros(B, dtype=np.int32)
            for b in range(B):
                mi, my = meas[b][k]
                nb[b] = len(mi)
                ids[b, : len(mi)] = mi
                y[b, : len(mi)] = my
            fg.process_vision([s.vision_stamps[k] for s in sts], ids, y, nb=nb)
            for b in range(B):
                r = fg.gate_report(b)
                seq.append((fg.ids(b).copy(), fg.sigma(b).copy(), fg.state_estimate(b)["x"].copy(), r["ids"], r["stat"], r["removed"]))
        assert fg.device_error() == 0
        outs.append(seq)
    assert sum(int(s[5].sum()) for s in outs[0]) >= 3  # (the gate did remove landmarks)
    assert sum(len(s[3]) for s in outs[0]) > 1000
    for other in outs[1:]:
        for f, (a, b) in enumerate(zip(outs[0], other)):
            for u, v in zip(a, b):
                assert np.array_equal(u, v), f


# ---------------------------------------------------------------------------------------------------------------- 4. the deferral
def test_mahalanobis_gate_that_leaves_a_filter_too_small_for_the_queued_update(hip):
    """62 landmarks, five outliers in one frame -> 57: k_edit switches the queued update off (flag 2) and the host launches it, shaped for 57."""
    from eqf_vio_amd import synth

    N = 62
    st = synth.make_stream(N, seed=77, duration=0.4)
    d = synth.template_settings_dict()
    fo = G.mahalanobis_filter(d, G.TAU)
    fg = hip.FilterBatch(d, capacity=N, batch=1)
    fg.set_outlier_gate(MAHA, G.TAU)
    ids = st.ids
    for kind, k in st.events():
        if kind == "imu":
            G.np_imu(fo, st.imu[k])
            fg.process_imu([st.imu[k, 0]], st.imu[k, 1:4], st.imu[k, 4:7])
            continue
        y = st.bearings[k].copy()
        if k == 3:
            for i in (4, 9, 17, 33, 50):
                y[i] = G.rotated(y[i])
        if k == 4:
            ids = np.array(fo.X.ids, dtype=np.int32)  # (keep the set at 57)
        sel = np.searchsorted(st.ids, ids)
        fo.processVisionData(st.vision_stamps[k], ids, y[sel])
        fg.process_vision([st.vision_stamps[k]], ids, y[sel])
        if k == 3:
            assert len(fo.X.ids) == 57 and np.min(np.abs(fo.report["stat"] - G.TAU)) > 1e-3 * G.TAU
            ref = fo.report
            rep = fg.gate_report(0)
            assert len(rep["ids"]) == 62 and int(rep["removed"].sum()) == 5
            _check_report(rep, ref, EPS_CLOSED_LOOP, "deferral frame")
    assert fg.num_landmarks() == 57
    assert np.array_equal(fg.ids(), fo.X.ids)
    assert rel_fro(fg.sigma(), fo.stateCovariance()) < SIGMA_TOL
    eo, eg = fo.stateEstimate(), fg.state_estimate()
    assert np.abs(eo.pose.x - eg["x"]).max() < POSE_TOL and np.abs(eo.pose.q - eg["q"]).max() < POSE_TOL
    assert fg.device_error() == 0


# ---------------------------------------------------------------------------------------------------------------- 5. the default is untouched
def _run_history(fg, h, collect):
    st, meas, _ = G.history(h)
    out = []
    for kind, k in st.events():
        if kind == "imu":
            fg.process_imu([st.imu[k, 0]], st.imu[k, 1:4], st.imu[k, 4:7])
        else:
            fg.process_vision([st.vision_stamps[k]], *meas[k])
            out.append(collect(fg))
    assert fg.device_error() == 0
    return out


def _bits(fg):
    e = fg.state_estimate()
    return fg.ids().copy(), fg.sigma().copy(), e["x"].copy(), e["q"].copy(), e["p"].copy()


def test_setting_the_default_gate_changes_nothing(hip):
    """(EQF_GATE_CHORD, settings.outlierThreshold) set explicitly == never set, bit for bit, over a churn stream on which the chord gate trips."""
    from eqf_vio_amd import synth

    d = synth.template_settings_dict()
    d["outlierThreshold"] = 0.05
    a = hip.FilterBatch(d, capacity=120, batch=1)
    b = hip.FilterBatch(d, capacity=120, batch=1)
    assert a.outlier_gate() == (CHORD, 0.05)
    b.set_outlier_gate(CHORD, 0.05)
    ra, rb = _run_history(a, 1, _bits), _run_history(b, 1, _bits)
    sizes = [len(r[0]) for r in ra]
    for f, (u, v) in enumerate(zip(ra, rb)):
        for x, y in zip(u, v):
            assert np.array_equal(x, y), f
    # (the gate tripped: the measurement stream alone would give other landmark counts -- compare with a disarmed handle)
    d2 = dict(d)
    d2["outlierThreshold"] = 1e9
    c = hip.FilterBatch(d2, capacity=120, batch=1)
    assert sizes != [len(r[0]) for r in _run_history(c, 1, _bits)]


@pytest.mark.parametrize("N", [40, 70])
def test_chord_report_equals_numpy_chords(hip, N):
    """The chord gate gets its report too: one frame from an injected state (N = 40: the probe, N = 70: k_edit), chords to 1e-12."""
    st, d, snap, j = _state_before_the_fourth_frame(N)
    d = dict(d)
    d["outlierThreshold"] = 0.1
    y = st.bearings[j].copy()
    y[N // 2] = G.rotated(y[N // 2])
    fo = inject(G.chord_filter(d), snap)
    fo.processVisionData(st.vision_stamps[j], st.ids, y)
    ref = fo.report
    assert list(np.flatnonzero(ref["removed"])) == [N // 2] and np.min(np.abs(ref["stat"] - 0.1)) > 1e-3
    fg = hip.FilterBatch(d, capacity=N, batch=1)
    fg.restore_state(snap)
    fg.process_vision(st.vision_stamps[j], st.ids, y)
    rep = fg.gate_report(0)
    print(f"N={N}: chord worst difference {np.max(np.abs(rep['stat'] - ref['stat'])):.2e}")
    assert np.array_equal(rep["ids"], ref["ids"]) and np.array_equal(rep["removed"], ref["removed"])
    assert np.max(np.abs(rep["stat"] - ref["stat"])) <= 1e-12
    assert np.array_equal(fg.ids(), fo.X.ids)


def test_mahalanobis_gate_at_infinity_is_the_disarmed_handle(hip):
    from eqf_vio_amd import synth

    d = synth.template_settings_dict()
    assert d["outlierThreshold"] == 1e9
    a = hip.FilterBatch(d, capacity=120, batch=1)
    b = hip.FilterBatch(d, capacity=120, batch=1)
    b.set_outlier_gate(MAHA, np.inf)
    ra = _run_history(a, 1, _bits)
    rb = _run_history(b, 1, lambda f: _bits(f) + (len(f.gate_report(0)["ids"]),))
    for f, (u, v) in enumerate(zip(ra, rb)):
        assert v[5] == 0  # (disarmed: nothing examined)
        for x, y in zip(u, v):
            assert np.array_equal(x, y), f


# ---------------------------------------------------------------------------------------------------------------- 6. with "innovation_stats"
def test_kept_landmarks_have_the_statistic_as_their_nis(hip):
    """Closed loop on history 1 with the innovation statistics on: for every landmark that was in the report and kept, the gate's number is
    the nis_lm of the update that followed, and no such nis_lm exceeds tau -- both up to 4 kappa(S_ii) eps ref."""
    from eqf_vio_amd import synth

    fg = hip.FilterBatch(synth.template_settings_dict(), capacity=120, batch=1)
    fg.set_option("innovation_stats", 1)
    fg.set_outlier_gate(MAHA, G.TAU)
    run = G.oracle_run(1)
    frames = []

    def collect(f):
        k = len(frames)
        frames.append(k)
        rep, s, ids = f.gate_report(0), f.innovation_stats(0), [int(i) for i in f.ids()]
        assert s["valid"]
        checked = 0
        for i, st_, rem in zip(rep["ids"], rep["stat"], rep["removed"]):
            if rem:
                assert int(i) not in ids
                continue
            nis = s["nis_lm"][ids.index(int(i))]
            ref = run[k]["nis_lm"][int(i)]
            tol = 4 * run[k]["kappa_lm"][int(i)] * EPS_CLOSED_LOOP * ref
            assert abs(st_ - nis) <= tol, (k, int(i), st_, nis, tol)
            assert nis <= G.TAU + tol, (k, int(i))
            checked += 1
        return checked

    total = sum(_run_history(fg, 1, collect))
    assert total > 400


# ---------------------------------------------------------------------------------------------------------------- 7. arguments and ordering
def test_arguments(hip):
    import ctypes as C

    from eqf_vio_amd import synth

    L = hip.lib()
    d = synth.template_settings_dict()
    fg = hip.FilterBatch(d, capacity=8, batch=2)
    assert L.eqf_set_outlier_gate(None, CHORD, 0.1) == hip.ERR_INVALID
    for kind, thr in ((2, 0.1), (-1, 0.1), (CHORD, float("nan")), (MAHA, float("nan")), (MAHA, 0.0), (MAHA, -1.0), (MAHA, -np.inf)):
        assert L.eqf_set_outlier_gate(fg._h, kind, thr) == hip.ERR_INVALID, (kind, thr)
        assert fg.outlier_gate() == (CHORD, 1e9)  # (before any effect)
    n = C.c_int(-1)
    assert L.eqf_get_gate_report(fg._h, 2, C.byref(n), None, None, None) == hip.ERR_INVALID
    assert L.eqf_get_gate_report(fg._h, 0, None, None, None, None) == hip.ERR_INVALID
    assert L.eqf_get_gate_report(fg._h, 1, C.byref(n), None, None, None) == 0 and n.value == 0
    fg.set_outlier_gate(MAHA, 9.21)
    assert fg.outlier_gate() == (MAHA, 9.21)
    fg.set_outlier_gate(CHORD, 3.0)  # (disarmed, as outlierThreshold >= 2 is)
    assert fg.outlier_gate() == (CHORD, 3.0)
    f32 = hip.FilterBatch(d, capacity=8, batch=1, precision=hip.PRECISION_F32)
    assert L.eqf_set_outlier_gate(f32._h, MAHA, 1.0) == hip.ERR_UNSUPPORTED
    assert L.eqf_set_outlier_gate(f32._h, CHORD, 0.05) == 0 and f32.outlier_gate() == (CHORD, 0.05)


def test_setter_resolves_a_pending_answer_with_the_old_gate(hip):
    """A frame with an outlier under the chord gate, its answer not yet looked at; then the setter.  The frame is resolved as a chord frame:
    the outlier is gone and the report holds chords (the outlier's is 2 sin(0.1), its d2 would be around 2)."""
    st, d, snap, j = _state_before_the_fourth_frame(70)
    d = dict(d)
    d["outlierThreshold"] = 0.1
    y = st.bearings[j].copy()
    y[35] = G.rotated(y[35])
    fg = hip.FilterBatch(d, capacity=70, batch=1)
    fg.restore_state(snap)
    fg.process_vision(st.vision_stamps[j], st.ids, y)
    fg.set_outlier_gate(MAHA, 100.0)
    assert fg.outlier_gate() == (MAHA, 100.0)
    rep = fg.gate_report(0)
    assert len(rep["ids"]) == 70 and list(np.flatnonzero(rep["removed"])) == [35]
    assert abs(rep["stat"][35] - 2 * np.sin(0.1)) < 0.02 and np.delete(rep["stat"], 35).max() < 0.1
    assert 35 not in fg.ids() and fg.num_landmarks() == 69
    # ... and the next frame runs under the new gate: nothing above 100, d2 in the report
    fo = inject(G.mahalanobis_filter(d, 100.0), fg.dump_state())
    ids = fg.ids().copy()
    y2 = st.bearings[j + 1][ids].copy()
    y2[10] = G.rotated(y2[10])
    fo.processVisionData(st.vision_stamps[j + 1], ids, y2)
    fg.process_vision(st.vision_stamps[j + 1], ids, y2)
    _check_report(fg.gate_report(0), fo.report, EPS_ONE_UPDATE, "frame after the setter")
    assert fo.report["stat"][10] > 0.5 and fg.num_landmarks() == 69


def test_stream_mode_equals_per_call_mode_under_the_mahalanobis_gate(hip):
    from eqf_vio_amd import synth

    N = 70
    st = synth.make_stream(N, duration=0.6)
    y = st.bearings.copy()
    for f, i in ((3, 5), (6, 40), (6, 41), (9, 69)):
        y[f, i] = G.rotated(y[f, i])
    d = synth.template_settings_dict()
    a = hip.FilterBatch(d, capacity=N, batch=1)
    b = hip.FilterBatch(d, capacity=N, batch=1)
    a.set_outlier_gate(MAHA, G.TAU)
    b.set_outlier_gate(MAHA, G.TAU)
    b.stream_upload(st.imu, st.vision_stamps, st.ids, y)
    removed = 0
    for kind, k in st.events():
        if kind == "imu":
            a.process_imu([st.imu[k, 0]], st.imu[k, 1:4], st.imu[k, 4:7])
            b.stream_imu(k)
        else:
            a.process_vision([st.vision_stamps[k]], st.ids, y[k])
            b.stream_vision(k)
            ra, rb = a.gate_report(0), b.gate_report(0)
            assert all(np.array_equal(ra[key], rb[key]) for key in ra), k
            removed += int(ra["removed"].sum())
            assert np.array_equal(a.ids(), b.ids()), k
    assert removed >= 4
    assert np.array_equal(a.sigma(), b.sigma())
    ea, eb = a.state_estimate(), b.state_estimate()
    assert all(np.array_equal(ea[k], eb[k]) for k in ea)
    assert a.device_error() == 0 and b.device_error() == 0


def test_reset_empties_the_report_and_keeps_the_gate(hip):
    from eqf_vio_amd import synth

    N = 20
    st = synth.make_stream(N, duration=0.3)
    fg = hip.FilterBatch(synth.template_settings_dict(), capacity=N, batch=1)
    fg.set_outlier_gate(MAHA, G.TAU)

    def run():
        for kind, k in st.events():
            if kind == "imu":
                fg.process_imu([st.imu[k, 0]], st.imu[k, 1:4], st.imu[k, 4:7])
            else:
                fg.process_vision([st.vision_stamps[k]], st.ids, st.bearings[k])
        return fg.gate_report(0), fg.sigma().copy()

    r1, s1 = run()
    assert len(r1["ids"]) == N and not r1["removed"].any() and np.all(r1["stat"] > 0)
    fg.reset()
    assert len(fg.gate_report(0)["ids"]) == 0
    assert fg.outlier_gate() == (MAHA, G.TAU)
    r2, s2 = run()
    assert all(np.array_equal(r1[k], r2[k]) for k in r1) and np.array_equal(s1, s2)
    # set_state and copy_filters forget the report of the filter they overwrite; the gate is the handle's own
    other = hip.FilterBatch(synth.template_settings_dict(), capacity=N, batch=1)
    other.copy_filters(fg, [0], [0])
    assert other.outlier_gate() == (CHORD, 1e9) and len(other.gate_report(0)["ids"]) == 0
    fg.restore_state(fg.dump_state())
    assert len(fg.gate_report(0)["ids"]) == 0 and fg.outlier_gate() == (MAHA, G.TAU)


# ---------------------------------------------------------------------------------------------------------------- 8. the C++ facade
def test_cpp_facade_gate_report_matches_the_oracle():
    """eqf_example ... gate: VIOFilter::setOutlierGate(EQF_GATE_MAHALANOBIS, 0.5) and gateReport() after every frame, the bearing of landmark
    3 turned by 0.2 rad about x on frame frames - 3, every bearing disturbed by 1e-3 (an exact one leaves residuals of rounding size, which
    no relative bound fits); the same inputs through the subclassed numpy oracle."""
    from oracle import eqf_numpy as O

    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eqf_vio_amd", "cpp", "eqf_example")
    assert os.path.exists(exe), "build it with __graft_entry__.build()"
    N, frames = 20, 10
    out = subprocess.run([exe, str(N), str(frames), "gate"], capture_output=True, text=True, check=True).stdout
    lines = [l.split() for l in out.splitlines() if l.startswith("gate ")]
    assert len(lines) == frames
    i = np.arange(N)
    lm = np.stack([2 * np.sin(1.3 * i), 2 * np.cos(0.7 * i), 5 + np.sin(0.37 * i)], axis=1)
    y = lm / np.linalg.norm(lm, axis=1, keepdims=True)
    fo = G.MahalanobisGateFilter(O.Settings(initialPointVariance=5000.0, measurementVariance=0.003, velOmegaVariance=1e-4, velAccelVariance=1e-4,
                                            outlierThreshold=1e9), G.TAU)
    k = 0
    removed = 0
    for f in range(frames):
        stamp = 0.05 * f + 0.0025
        while 0.005 * k < stamp:
            fo.processIMUData(O.IMUVelocity(0.005 * k, np.zeros(3), np.array([9.81, 0.0, 0.0])))
            k += 1
        yy = y.copy()
        yy[:, 0] += 1e-3 * np.sin(7.0 * i + 3.0 * f)
        yy[:, 1] += 1e-3 * np.cos(5.0 * i + 2.0 * f)
        yy /= np.sqrt(yy[:, 0] * yy[:, 0] + yy[:, 1] * yy[:, 1] + yy[:, 2] * yy[:, 2])[:, None]
        if f == frames - 3:
            c, s = np.cos(0.2), np.sin(0.2)
            yy[3] = [yy[3, 0], c * yy[3, 1] - s * yy[3, 2], s * yy[3, 1] + c * yy[3, 2]]
        fo.processVisionData(stamp, i.astype(np.int32), yy)
        tok = lines[f]
        assert int(tok[1]) == f
        n = int(tok[2])
        rep = dict(ids=np.array([int(t) for t in tok[3::3]]), stat=np.array([float.fromhex(t) for t in tok[4::3]]),
                   removed=np.array([bool(int(t)) for t in tok[5::3]]))
        assert n == len(rep["ids"])
        ref = fo.report
        if len(ref["stat"]):
            assert np.min(np.abs(ref["stat"] - G.TAU)) > 1e-3 * G.TAU
        _check_report(rep, ref, EPS_CLOSED_LOOP, f"facade frame {f}")
        removed += int(ref["removed"].sum())
    assert removed == 1
