"""The Mahalanobis outlier gate in the numpy oracle (tests/gate_helpers.py), without a GPU: the expectation the device tests of
tests/test_gpu_gate.py compare against is itself checked here -- it degenerates to the base oracle when disarmed, its statistic is the
per-landmark NIS of the update that follows, and on the histories of the device tests it removes exactly the injected bearings with no
statistic anywhere near the threshold (so that a device / oracle comparison cannot hide behind a tie)."""
import numpy as np
import pytest

import gate_helpers as G
from consistency_helpers import innovation_reference, np_imu, numpy_filter


def test_disarmed_gate_is_the_base_oracle_exactly():
    from eqf_vio_amd import synth

    st = synth.make_stream(30, seed=610, duration=0.6)
    meas = synth.churn_measurements(st, seed=31, max_visible=12, outlier_frames=(4, 7, 9), outlier_angle=0.2)
    d = synth.template_settings_dict()
    assert d["outlierThreshold"] == 1e9
    fa, fb = G.mahalanobis_filter(d, np.inf), numpy_filter(d)
    changed = 0
    for kind, k in st.events():
        if kind == "imu":
            np_imu(fa, st.imu[k])
            np_imu(fb, st.imu[k])
            continue
        before = list(fa.X.ids)
        fa.processVisionData(st.vision_stamps[k], *meas[k])
        fb.processVisionData(st.vision_stamps[k], *meas[k])
        changed += before != list(fa.X.ids)
        assert not fa.report["removed"].any()
        assert np.array_equal(fa.X.ids, fb.X.ids), k
        assert np.array_equal(fa.Sigma, fb.Sigma), k
        ea, eb = fa.stateEstimate(), fb.stateEstimate()
        assert np.array_equal(ea.pose.x, eb.pose.x) and np.array_equal(ea.pose.q, eb.pose.q) and np.array_equal(ea.p, eb.p), k
    assert changed >= 5  # (a churn stream: the landmark set did change)


@pytest.mark.parametrize("h", [0, 1, 2])
def test_statistic_of_a_kept_landmark_is_its_nis_of_the_update(h):
    """nis_lm of innovation_reference is computed from the assembled S and delta of the update, AFTER the outliers left and the new
    landmarks came; the gate's number from the landmark's own blocks before.  For a kept landmark they are the same quantity."""
    worst, count = 0.0, 0
    for rec in G.oracle_run(h):
        r = rec["report"]
        for i, s, rem in zip(r["ids"], r["stat"], r["removed"]):
            if rem:
                continue
            ref = rec["nis_lm"][int(i)]
            worst = max(worst, abs(s - ref) / ref)
            count += 1
            assert abs(s - ref) <= 1e-8 * ref, (h, int(i), s, ref)
    print(f"history {h}: {count} kept landmarks, worst relative difference {worst:.1e}")
    assert count > 50


def test_chi2_gate_threshold_is_the_two_dof_quantile():
    from eqf_vio_amd.consistency import chi2_gate_threshold

    for p, q in ((0.95, 5.991), (0.99, 9.210), (0.999, 13.816)):
        assert abs(chi2_gate_threshold(p) - q) < 5e-4
        assert abs(1.0 - np.exp(-chi2_gate_threshold(p) / 2) - p) < 1e-15  # (the CDF of chi-square with 2 dof)
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            chi2_gate_threshold(bad)


@pytest.mark.parametrize("h", [0, 1, 2])
def test_oracle_removes_exactly_the_injected_bearings_and_nothing_is_near_the_threshold(h):
    _, _, injected = G.history(h)
    removals, margin = 0, np.inf
    for f, rec in enumerate(G.oracle_run(h)):
        r = rec["report"]
        examined = set(int(i) for i in r["ids"])
        removed = set(int(i) for i in r["ids"][r["removed"]])
        assert removed == injected[f] & examined, (h, f)
        assert injected[f] <= examined, (h, f)  # (every injected bearing belongs to a landmark the gate examines: none is wasted on a new one)
        removals += len(removed)
        if len(r["stat"]):
            margin = min(margin, float(np.min(np.abs(r["stat"] - G.TAU)) / G.TAU))
    print(f"history {h}: {removals} removals, closest statistic {margin:.3f} (relative) from tau = {G.TAU}")
    assert removals == (4 if h == 1 else 3)
    assert margin > 1e-3


def test_chord_report_is_what_the_reference_gate_compares():
    """The sibling that records the chords changes nothing, and flags what removeOutliers removes."""
    from eqf_vio_amd import synth

    st, meas, injected = G.history(0)
    d = synth.template_settings_dict()
    d["outlierThreshold"] = 0.12
    fa, fb = G.chord_filter(d), numpy_filter(d)
    removed = 0
    for kind, k in st.events():
        if kind == "imu":
            np_imu(fa, st.imu[k])
            np_imu(fb, st.imu[k])
            continue
        before = set(int(i) for i in fa.X.ids) & set(int(i) for i in meas[k][0])
        fa.processVisionData(st.vision_stamps[k], *meas[k])
        fb.processVisionData(st.vision_stamps[k], *meas[k])
        assert np.array_equal(fa.X.ids, fb.X.ids) and np.array_equal(fa.Sigma, fb.Sigma), k
        r = fa.report
        assert set(int(i) for i in r["ids"]) == before
        gone = set(int(i) for i in r["ids"][r["removed"]])
        assert gone == before - set(int(i) for i in fa.X.ids), k
        removed += len(gone)
    assert removed >= 3
