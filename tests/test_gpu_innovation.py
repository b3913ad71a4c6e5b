"""Innovation statistics of the vision update (csrc/eqf_innov.hpp; eqf_set_option "innovation_stats", eqf_get_innovation_stats) against the
numpy oracle's S and delta: one update from an injected state, the closed loop, independence of the factorisation's launch shape, and no
side effect on the filter.  Reference values come from a Cholesky factor of the LOWER triangle of the oracle's S (the device's chain
reads the lower triangle; the oracle's Sigma is not exactly symmetric because the reference's gain form is not symmetrised)."""
import math

import numpy as np
import pytest

from consistency_helpers import inject, innovation_reference, np_imu, numpy_filter

pytestmark = pytest.mark.gpu

EPS_ONE_UPDATE = 2e-9   # the one-update Sigma bound of tests/test_gpu_configs.py::test_single_propagate_and_single_update_from_an_injected_state
EPS_CLOSED_LOOP = 1e-7  # SIGMA_TOL of tests/test_gpu_parity.py: what the closed-loop Sigma is held to


@pytest.fixture(scope="module")
def hip():
    from eqf_vio_amd import binding

    return binding


def _check_stats(s, ref, eps, what):
    """|nis - ref| <= 4 kappa eps ref, |logdet_S - ref| <= 4 m kappa eps, nis_lm likewise with the block's own kappa."""
    k, m = ref["kappa"], ref["m"]
    tol_nis, tol_ld = 4 * k * eps * ref["nis"], 4 * m * k * eps
    print(f"{what}: m={m} cond(S)={k:.2f} nis={s['nis']:.6e} (ref diff {abs(s['nis'] - ref['nis']):.2e}, tol {tol_nis:.2e}) "
          f"logdet={s['logdet_S']:.6f} (ref diff {abs(s['logdet_S'] - ref['logdet_S']):.2e}, tol {tol_ld:.2e}) "
          f"nis_lm worst diff/tol {np.max(np.abs(s['nis_lm'] - ref['nis_lm']) / (4 * ref['kappa_lm'] * eps * ref['nis_lm'])):.2e}")
    assert s["valid"] and s["dof"] == m
    assert abs(s["nis"] - ref["nis"]) <= tol_nis, what
    assert abs(s["logdet_S"] - ref["logdet_S"]) <= tol_ld, what
    assert np.all(np.abs(s["nis_lm"] - ref["nis_lm"]) <= 4 * ref["kappa_lm"] * eps * ref["nis_lm"]), what
    terms = np.array([s["nis"], s["logdet_S"], m * math.log(2 * math.pi)])
    assert abs(s["loglik"] + 0.5 * terms.sum()) <= 4 * 2.0 ** -53 * np.abs(terms).sum(), what
    return tol_nis, tol_ld


def _events_until_vision(ev, start):
    """Indices [start, i] of the IMU events from `start` and the one vision event that follows them."""
    i = start
    while ev[i][0] == "imu":
        i += 1
    return i


@pytest.mark.parametrize("N", [5, 40, 200])
@pytest.mark.parametrize("k", [1, 3, 6])
def test_one_update_from_an_injected_state(hip, N, k):
    """The device state after k vision frames goes into a numpy VIOFilter; the IMU calls and ONE vision call run on both.  Also: the same
    update with measurementVariance raised by 1 % moves nis and logdet_S by more than 100 x the tolerance (the test can see a wrong S)."""
    from eqf_vio_amd import synth

    st = synth.make_stream(N, duration=0.5)
    d = synth.template_settings_dict()
    fg = hip.FilterBatch(d, capacity=N, batch=1)
    fg.set_option("innovation_stats", 1)
    ev = list(st.events())
    vis = [i for i, (kind, _) in enumerate(ev) if kind == "vision"]
    stop = vis[k - 1] + 1
    for kind, j in ev[:stop]:
        if kind == "imu":
            fg.process_imu(st.imu[j, 0], st.imu[j, 1:4], st.imu[j, 4:7])
        else:
            fg.process_vision(st.vision_stamps[j], st.ids, st.bearings[j])
    snap = fg.dump_state()
    fo = inject(numpy_filter(d), snap)
    d2 = dict(d)
    d2["measurementVariance"] = d["measurementVariance"] * 1.01
    f2 = hip.FilterBatch(d2, capacity=N, batch=1)
    f2.set_option("innovation_stats", 1)
    f2.restore_state(snap)
    last = _events_until_vision(ev, stop)
    for kind, j in ev[stop:last + 1]:
        if kind == "imu":
            np_imu(fo, st.imu[j])
            fg.process_imu(st.imu[j, 0], st.imu[j, 1:4], st.imu[j, 4:7])
            f2.process_imu(st.imu[j, 0], st.imu[j, 1:4], st.imu[j, 4:7])
        else:
            fo.processVisionData(st.vision_stamps[j], st.ids, st.bearings[j])
            assert fg.process_vision(st.vision_stamps[j], st.ids, st.bearings[j])[0] == 0
            assert f2.process_vision(st.vision_stamps[j], st.ids, st.bearings[j])[0] == 0
    ref = innovation_reference(fo.last["S"], fo.last["delta"])
    assert 4 * ref["kappa"] * EPS_ONE_UPDATE < 1e-6, ref["kappa"]  # (keeps the bounds from being vacuous)
    s, s2 = fg.innovation_stats(0), f2.innovation_stats(0)
    tol_nis, tol_ld = _check_stats(s, ref, EPS_ONE_UPDATE, f"N={N} k={k}")
    print(f"  measurementVariance + 1 %: nis moves {abs(s2['nis'] - s['nis']) / tol_nis:.0f} x tol, logdet_S {abs(s2['logdet_S'] - s['logdet_S']) / tol_ld:.0f} x tol")
    assert abs(s2["nis"] - s["nis"]) > 100 * tol_nis and abs(s2["logdet_S"] - s["logdet_S"]) > 100 * tol_ld
    assert fg.device_error() == 0 and f2.device_error() == 0


def test_one_update_in_a_batch_of_four_against_four_oracles(hip):
    from eqf_vio_amd import synth

    N, B, k = 40, 4, 3
    sts = [synth.make_stream(N, seed=1234 + 7 * b, duration=0.4) for b in range(B)]
    d = synth.template_settings_dict()
    fg = hip.FilterBatch(d, capacity=N, batch=B)
    fg.set_option("innovation_stats", 1)
    ev = list(sts[0].events())  # (same stamps in every stream)
    vis = [i for i, (kind, _) in enumerate(ev) if kind == "vision"]
    stop = vis[k - 1] + 1

    def dev(kind, j):
        if kind == "imu":
            fg.process_imu([s.imu[j, 0] for s in sts], np.array([s.imu[j, 1:4] for s in sts]), np.array([s.imu[j, 4:7] for s in sts]))
        else:
            st = fg.process_vision([s.vision_stamps[j] for s in sts], sts[0].ids, np.array([s.bearings[j] for s in sts]))
            assert np.all(st == 0)

    for kind, j in ev[:stop]:
        dev(kind, j)
    fos = [inject(numpy_filter(d), fg.dump_state(b)) for b in range(B)]
    last = _events_until_vision(ev, stop)
    for kind, j in ev[stop:last + 1]:
        dev(kind, j)
        for b in range(B):
            if kind == "imu":
                np_imu(fos[b], sts[b].imu[j])
            else:
                fos[b].processVisionData(sts[b].vision_stamps[j], sts[b].ids, sts[b].bearings[j])
    for b in range(B):
        ref = innovation_reference(fos[b].last["S"], fos[b].last["delta"])
        assert 4 * ref["kappa"] * EPS_ONE_UPDATE < 1e-6
        _check_stats(fg.innovation_stats(b), ref, EPS_ONE_UPDATE, f"batch b={b}")
    assert fg.device_error() == 0


def test_closed_loop_against_the_numpy_oracle_every_frame(hip):
    """2 s of the N = 50 stream side by side.  The stream's first vision frame, in which every landmark is new, has delta = 0 by
    construction: nis < 1e-20 there instead of the relative bound; no other frame is exempt."""
    from eqf_vio_amd import synth

    N = 50
    st = synth.make_stream(N, duration=2.0)
    d = synth.template_settings_dict()
    fg = hip.FilterBatch(d, capacity=N, batch=1)
    fg.set_option("innovation_stats", 1)
    fo = numpy_filter(d)
    # before the first IMU sample: the vision call is skipped, valid = 0
    assert fg.process_vision(st.vision_stamps[0] - 1.0, st.ids, st.bearings[0])[0] == hip.SKIPPED_BEFORE_FIRST_IMU
    assert not fg.innovation_stats(0)["valid"]
    frames = 0
    for kind, j in st.events():
        if kind == "imu":
            np_imu(fo, st.imu[j])
            fg.process_imu(st.imu[j, 0], st.imu[j, 1:4], st.imu[j, 4:7])
            continue
        fo.processVisionData(st.vision_stamps[j], st.ids, st.bearings[j])
        assert fg.process_vision(st.vision_stamps[j], st.ids, st.bearings[j])[0] == 0
        s = fg.innovation_stats(0)
        ref = innovation_reference(fo.last["S"], fo.last["delta"])
        assert s["valid"] and s["dof"] == 2 * N and math.isfinite(s["loglik"]), j
        if j == 0:
            print(f"frame 0: nis {s['nis']:.3e} (oracle {ref['nis']:.3e})")
            assert s["nis"] < 1e-20 and np.all(s["nis_lm"] < 1e-20)
            assert abs(s["logdet_S"] - ref["logdet_S"]) <= 4 * ref["m"] * ref["kappa"] * EPS_CLOSED_LOOP
        else:
            assert 4 * ref["kappa"] * EPS_CLOSED_LOOP < 1e-4, (j, ref["kappa"])
            _check_stats(s, ref, EPS_CLOSED_LOOP, f"frame {j}")
        frames += 1
        if j == 5:
            # the same stamp again: dt <= 0, the call is skipped and the statistics are not valid any more
            assert fg.process_vision(st.vision_stamps[j], st.ids, st.bearings[j])[0] == hip.SKIPPED_NONPOSITIVE_DT
            assert not fg.innovation_stats(0)["valid"]
    assert frames >= 39
    assert fg.innovation_stats(0)["valid"]
    fg.set_option("innovation_stats", 0)
    s = fg.innovation_stats(0)
    assert not s["valid"] and s["nis"] == 0.0 and s["dof"] == 0
    assert fg.device_error() == 0


def _stats_bits(fg, B):
    out = []
    for b in range(B):
        s = fg.innovation_stats(b)
        assert s["valid"]
        out.append(np.concatenate([[s["nis"], s["logdet_S"], s["loglik"], s["dof"]], s["nis_lm"]]))
    return out


@pytest.mark.parametrize("N", [21, 70, 200])
def test_statistics_do_not_depend_on_the_launch_shape(hip, monkeypatch, N):
    """nis, logdet_S and nis_lm of the first update from a common restored state, 8 filters: bit for bit equal between the default launch,
    the per-column launches (EQF_CHOL_RESIDENT=0), the prep launch in front (EQF_RES_FOLD_PREP=0), arrival tickets (res_tickets = 2) and the
    int8 downdate (downdate_slices = 6); and between two runs."""
    from eqf_vio_amd import synth

    B = 8
    sts = [synth.make_stream(N, seed=99 + b, duration=0.3) for b in range(B)]
    d = synth.template_settings_dict()
    ev = list(sts[0].events())
    vis = [i for i, (kind, _) in enumerate(ev) if kind == "vision"]
    stop = vis[2] + 1
    last = _events_until_vision(ev, stop)

    def feed(fg, events):
        for kind, j in events:
            if kind == "imu":
                fg.process_imu([s.imu[j, 0] for s in sts], np.array([s.imu[j, 1:4] for s in sts]), np.array([s.imu[j, 4:7] for s in sts]))
            else:
                assert np.all(fg.process_vision([s.vision_stamps[j] for s in sts], sts[0].ids, np.array([s.bearings[j] for s in sts])) == 0)

    f0 = hip.FilterBatch(d, capacity=N, batch=B)
    feed(f0, ev[:stop])
    snaps = [f0.dump_state(b) for b in range(B)]

    def variant(env=None, option=None):
        for k_, v_ in (env or {}).items():
            monkeypatch.setenv(k_, v_)
        fg = hip.FilterBatch(d, capacity=N, batch=B)
        for k_ in (env or {}):
            monkeypatch.delenv(k_)
        for b in range(B):
            fg.restore_state(snaps[b], b)
        fg.set_option("innovation_stats", 1)
        if option:
            fg.set_option(*option)
        feed(fg, ev[stop:last + 1])
        assert fg.device_error() == 0
        return _stats_bits(fg, B)

    base = variant()
    for what, kw in (("second run", {}), ("EQF_CHOL_RESIDENT=0", dict(env={"EQF_CHOL_RESIDENT": "0"})),
                     ("EQF_RES_FOLD_PREP=0", dict(env={"EQF_RES_FOLD_PREP": "0"})), ("res_tickets=2", dict(option=("res_tickets", 2))),
                     ("downdate_slices=6", dict(option=("downdate_slices", 6)))):
        got = variant(**kw)
        for b in range(B):
            assert np.array_equal(got[b], base[b]), (what, N, b)


@pytest.mark.parametrize("stream_mode", [False, True])
def test_the_option_has_no_side_effect(hip, stream_mode):
    """Two handles on the same stream, option on and off: sigma(), the state and last_update() bit for bit equal after 20 frames; the launch
    shape of the handle with the option switched off is that of a handle that never saw the option."""
    from eqf_vio_amd import synth

    N = 40
    st = synth.make_stream(N, duration=1.05)
    d = synth.template_settings_dict()
    fs = [hip.FilterBatch(d, capacity=N, batch=1) for _ in range(3)]
    fs[0].set_option("innovation_stats", 1)
    fs[1].set_option("innovation_stats", 1)
    fs[1].set_option("innovation_stats", 0)
    if stream_mode:
        for f in fs:
            f.stream_upload(st.imu, st.vision_stamps, st.ids, st.bearings)
    frames = 0
    for kind, j in st.events():
        for f in fs:
            if stream_mode:
                (f.stream_imu if kind == "imu" else f.stream_vision)(j)
            elif kind == "imu":
                f.process_imu(st.imu[j, 0], st.imu[j, 1:4], st.imu[j, 4:7])
            else:
                f.process_vision(st.vision_stamps[j], st.ids, st.bearings[j])
        frames += kind == "vision"
    assert frames >= 20
    assert fs[0].innovation_stats(0)["valid"] and not fs[1].innovation_stats(0)["valid"] and not fs[2].innovation_stats(0)["valid"]
    assert fs[1].launch_shape() == fs[2].launch_shape() == fs[0].launch_shape()
    ref = fs[2]
    for f in fs[:2]:
        a, b = f.dump_state(), ref.dump_state()
        assert np.array_equal(a["sigma"], b["sigma"]) and np.array_equal(a["bias"], b["bias"]) and a["time"] == b["time"]
        for grp in ("origin", "group"):
            for key in a[grp]:
                assert np.array_equal(a[grp][key], b[grp][key]), (grp, key)
        la, lb = f.last_update(), ref.last_update()
        for key in la:
            assert np.array_equal(la[key], lb[key]), key
        ea, eb = f.state_estimate(), ref.state_estimate()
        for key in ea:
            assert np.array_equal(ea[key], eb[key]), key
        assert f.device_error() == 0


def test_reset_forgets_the_statistics(hip):
    from eqf_vio_amd import synth

    N = 10
    st = synth.make_stream(N, duration=0.2)
    fg = hip.FilterBatch(synth.template_settings_dict(), capacity=N, batch=2)
    fg.set_option("innovation_stats", 1)
    for kind, j in st.events():
        if kind == "imu":
            fg.process_imu(st.imu[j, 0], st.imu[j, 1:4], st.imu[j, 4:7])
        else:
            fg.process_vision(st.vision_stamps[j], st.ids, st.bearings[j])
    assert fg.innovation_stats(0)["valid"] and fg.innovation_stats(1)["valid"]
    fg.reset()
    assert not fg.innovation_stats(0)["valid"] and not fg.innovation_stats(1)["valid"]
    assert fg.device_error() == 0
