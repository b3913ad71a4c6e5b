"""The innovation lift of eqf_update_linear / eqf_update_landmarks / eqf_apply_increment / eqf_perturb_filters on the device
(csrc/eqf_lift.hpp; eqf_set_option "innovation_lift", eqf_get_lift_report) against the 50-digit reference and the measured bound of
tests/lift_exact.py, on the cases of tests/lift_cases.py that tests/test_lift_exact.py holds the fp64 restatements to.  Every reference
starts from the device's own state before the call and takes the gamma the device itself formed.  Everything that is not arithmetic is bit
for bit: Sigma against the call with the option off, the default, an untouched filter, a filter alone against the same filter in a batch,
run to run.  Nothing here provokes a fault: an indefinite Sigma_e is an ordinary numeric verdict of the factorisation.
Each test prints its worst device / bound ratios."""
import numpy as np
import pytest

import blocks_exact as bx
import lift_cases as lc
import lift_exact as le
import update_exact as ux

pytestmark = pytest.mark.gpu
CALLS = ("apply_increment", "update_linear", "update_landmarks")


@pytest.fixture(scope="module")
def hip():
    from eqf_vio_amd import binding

    return binding


def _bits(x):
    if isinstance(x, dict):
        return {k: _bits(v) for k, v in x.items()}
    return np.ascontiguousarray(x).tobytes() + str(np.asarray(x).shape).encode()


def _handle(hip, snaps, d, option, cap=None):
    cap = cap or max(len(s["ids"]) for s in snaps) + lc.CAP_EXTRA
    fg = hip.FilterBatch(d, capacity=cap, batch=len(snaps))
    for b, s in enumerate(snaps):
        fg.restore_state(s, b)
    if option is not None:
        fg.set_option("innovation_lift", option)
    return fg


def _call(fg, call, snaps, mask=None, drop_last=False):
    """one of the three calls with the increments of lift_cases.py, every filter its own; returns (gamma (B, n_max) or None, report dict or None)"""
    Ns = [len(s["ids"]) for s in snaps]
    if call == "apply_increment":
        G = [lc.raw(N, lc.own_sigma(N)) for N in Ns]
        fg.apply_increment(G, mask=mask)
        return G, None
    if call == "update_linear":
        ops = [lc.zupt(N) for N in Ns]
        out = fg.update_linear([o[0] for o in ops], [o[1] for o in ops], ops[0][2], local=False, mask=mask, want_gamma=True)
        return [out["gamma"][b, :11 + 3 * N] for b, N in enumerate(Ns)], out
    ops = [lc.stereo(N, s["ids"]) for N, s in zip(Ns, snaps)]
    k = [len(o[0]) - (1 if drop_last and N > 1 else 0) for o, N in zip(ops, Ns)]
    out = fg.update_landmarks([o[0][:kk] for o, kk in zip(ops, k)], [o[2][:kk] for o, kk in zip(ops, k)], [o[3][:kk] for o, kk in zip(ops, k)],
                              [o[4][:kk] for o, kk in zip(ops, k)], rows=2, local=False, mask=mask)
    return [out["gamma"][b, :11 + 3 * N] for b, N in enumerate(Ns)], out


def _state(fg, b):
    return dict(group=fg.group(b), bias=fg.bias(b), sigma=fg.sigma(b), origin=fg.origin(b))


def _check_against_reference(fg, b, pre, gamma, d, disc, worst, what):
    rep = fg.lift_report(b)
    assert rep["kind"] == (2 if disc else 1) and rep["info"] == 0, (what, rep)
    ref = le.reference(gamma, pre, pre["sigma"], d["cameraOffset_q"], d["cameraOffset_x"], disc)
    r = {"DeltaU": le.ratio_dU(rep["DeltaU"], ref) / lc.K_LIFT}
    r.update({k: v / lc.K_STEP for k, v in le.ratios_X(fg.group(b), fg.bias(b), ref, lc.K_LIFT).items()})
    for k, v in r.items():
        worst[k] = max(worst.get(k, 0.0), v)
    assert max(r.values()) <= 1.0, (what, r)
    L = np.linalg.cholesky(pre["sigma"][6:, 6:])
    assert abs(rep["min_pivot"] - np.min(np.diag(L)) ** 2) <= 1e-6 * np.min(np.diag(L)) ** 2, what
    assert 0.0 < rep["pivot_ratio"] <= 1.0
    return ref


# ---- 1. fails without the feature
def test_option_and_getter_exist(hip):
    assert hasattr(hip.lib(), "eqf_get_lift_report")
    fg = _handle(hip, [lc.snapshot(3)], lc.settings(1), None)
    assert hip.lib().eqf_set_option(fg._h, b"innovation_lift", 1) == 0
    assert hip.lib().eqf_get_lift_report(fg._h, 0, hip.LiftReport()) == hip.ERR_INVALID   # (no such call yet)
    fg.apply_increment([lc.raw(3, lc.own_sigma(3))])
    assert fg.lift_report(0)["kind"] == 2 and fg.device_error() == 0
    fg.close()


# ---- 2. against the exact reference
@pytest.mark.parametrize("N,disc", lc.CASES)
def test_against_the_exact_reference(hip, N, disc):
    d = lc.settings(disc)
    snap = lc.snapshot(N)
    worst = {}
    for call in CALLS:
        on, off = _handle(hip, [snap], d, 1), _handle(hip, [snap], d, 0)
        pre = on.dump_state(0)
        assert _bits(pre["sigma"]) == _bits(off.sigma(0))
        G, out = _call(on, call, [snap])
        _call(off, call, [snap])
        if out is not None:
            assert out["info"][0] == 0, (call, out["info"])
        _check_against_reference(on, 0, pre, G[0], d, disc, worst, (N, disc, call))
        # the lift does not touch Sigma
        assert _bits(on.sigma(0)) == _bits(off.sigma(0)), (N, disc, call)
        assert off.lift_report(0)["kind"] == 0 and on.device_error() == 0 and off.device_error() == 0
        # ... and it has the translation and yaw part that the plain lift's (dUw; 0) lacks
        assert not np.any(off.lift_report(0)["DeltaU"][3:6]) and np.all(on.lift_report(0)["DeltaU"][3:6] != 0.0)
        on.close()
        off.close()
    print("lift / bound", (N, disc), {k: "%.3g" % v for k, v in worst.items()})


# ---- 3. against the vision update
@pytest.mark.parametrize("disc", (1, 0))
def test_against_the_vision_update(hip, disc):
    from eqf_vio_amd import synth

    N = 20
    d = lc.settings(disc)
    st = synth.make_stream(N, duration=0.6)
    A = hip.FilterBatch(d, capacity=N + lc.CAP_EXTRA, batch=1)
    seen, last_imu, frame = 0, None, None
    for kind, k in st.events():
        if kind == "imu":
            r = st.imu[k]
            A.process_imu(r[0], r[1:4], r[4:7])
            last_imu = r
        elif seen < 5:
            A.process_vision(st.vision_stamps[k], st.ids, st.bearings[k])
            seen += 1
        else:
            frame = k
            break
    assert frame is not None and A.num_landmarks(0) == N and st.vision_stamps[frame] > last_imu[0]
    B = hip.FilterBatch(d, capacity=N + lc.CAP_EXTRA, batch=1)
    B.copy_filters(A, [0], [0])
    B.set_option("innovation_lift", 1)
    start = A.dump_state(0)
    assert _bits(B.dump_state(0)) == _bits(start)
    # A frame whose stamp EQUALS the last IMU stamp is not an update at all: integrateUpToTime answers false for dt <= 0 and
    # processVisionData returns (VIOFilter.cpp:146-152, :234-236).  So the frame keeps its own stamp, 2.5 ms behind the last IMU sample, and
    # twin B takes the same integration step -- the last sample held up to that stamp, Riccati included -- through an IMU call that repeats
    # the sample at the frame's stamp.  Its state then is the state the frame's update starts from.
    stamp, y = st.vision_stamps[frame], st.bearings[frame]
    B.process_imu(stamp, last_imu[1:4], last_imu[4:7])
    pre = B.dump_state(0)
    # twin A: the frame names exactly the state's landmarks; the gate is wide (outlierThreshold 1e9)
    A.process_vision(stamp, st.ids, y)
    lu = A.last_update(0)
    assert A.num_landmarks(0) == N and np.array_equal(A.origin(0)["p"], pre["origin"]["p"])
    # twin B: the same rows through the block update
    C0 = lc.oracle_output_blocks(pre, d)
    R = np.broadcast_to(d["measurementVariance"] * np.eye(2), (N, 2, 2)).copy()
    out = B.update_landmarks(pre["ids"], C0, lu["delta"].reshape(N, 2), R, rows=2, local=False)
    assert out["info"][0] == 0 and out["dof"][0] == 2 * N
    rep = B.lift_report(0)
    assert rep["kind"] == (2 if disc else 1) and rep["info"] == 0
    # Each route has a reference and a bound of its own: the vision call update_exact.Case from the state both twins started from (the
    # propagate's bound included), the block update blocks_exact from twin B's state behind its IMU call.  |A - B| <= bound_A + bound_B +
    # |reference_A - reference_B|, the last a known number (the two references start a propagate's rounding apart).
    vref, vb = ux.Case(start, d, stamp, y).reference(start["sigma"])
    ops = dict(rows=2, idx=np.arange(N), H=C0, resid=lu["delta"].reshape(N, 2), R=R, local=0, lm_gate=np.inf)
    uref = bx.reference(pre["sigma"], ops, None)
    bb = bx.bounds(uref)
    gA, gB = lu["gamma"], out["gamma"][0, :11 + 3 * N]
    f64 = ux.f64
    worst = {}

    def within(what, a, b_, tol, refgap):
        r = float(np.max(np.abs(a - b_) / (tol + refgap + 1e-300)))
        worst[what] = r
        assert r <= 1.0, (what, disc, r)

    within("gamma", gA, gB, vb["gamma"] + bb["gamma"], np.abs(f64(vref["gamma"]) - f64(uref["gamma"])))
    within("Sigma", A.sigma(0), B.sigma(0), vb["Sp"] + bb["Sp"], np.abs(f64(vref["Sp"]) - f64(uref["Sp"])))
    within("bias", A.bias(0), B.bias(0), vb["gamma"][0:6] + bb["gamma"][0:6] + 2 * le.U * np.abs(A.bias(0)),
           np.abs(f64(vref["gamma"]) - f64(uref["gamma"]))[0:6])
    # the lift: the block route against the 50-digit reference with its own gamma, the vision route's Gamma[0:6] within its own bound of
    # its own reference -- and DeltaU of the one agrees with Gamma[0:6] of the other within the sum
    refB = _check_against_reference(B, 0, pre, gB, d, disc, worst, ("blocks", disc))
    dUA, dUB = lu["Gamma"][0:6], rep["DeltaU"]
    assert np.all(np.abs(dUA - f64(vref["Gamma6"])) <= vb["Gamma6"])
    refgap = np.abs(f64(vref["Gamma6"]) - np.array([float(v) for v in refB["DeltaU"]]))
    within("DeltaU", dUA, dUB, vb["Gamma6"] + lc.K_LIFT * le.form_dU(refB), refgap)
    # X.A, X.w, every Q_i and the bias: twin B against the 50-digit group step above; twin A against the same step taken with ITS gamma
    # from the same starting state, with the vision route's own DeltaU budget (its bound plus the gap of its reference to this one) in
    # lift_exact's bound_X
    refA = le.reference(gA, pre, pre["sigma"], d["cameraOffset_q"], d["cameraOffset_x"], disc)
    gapA = np.abs(f64(vref["Gamma6"]) - np.array([float(v) for v in refA["DeltaU"]]))
    budget = float(np.max(vb["Gamma6"] + gapA)) / le.form_dU(refA)
    rA = {k: v / lc.K_STEP for k, v in le.ratios_X(A.group(0), A.bias(0), refA, budget).items()}
    worst.update({"A:" + k: v for k, v in rA.items()})
    print("vision twin", disc, {k: "%.3g" % v for k, v in worst.items()})
    assert max(rA.values()) <= 1.0, rA
    assert A.device_error() == 0 and B.device_error() == 0
    A.close()
    B.close()


# ---- 4. the default is unchanged
def test_default_is_unchanged_and_one_landmark_takes_the_plain_lift(hip):
    snaps = [lc.snapshot(N) for N in lc.RAGGED]
    for call in CALLS:
        got = []
        for d, option in ((lc.settings(1), 0), (lc.settings(1), None), (lc.settings(1, lift=0), 1)):
            fg = _handle(hip, snaps, d, option)
            _, out = _call(fg, call, snaps)
            got.append(dict(state=[_bits(_state(fg, b)) for b in range(3)], rep=[_bits(fg.lift_report(b)) for b in range(3)],
                            out=None if out is None else _bits({k: out[k] for k in ("nis", "logdet_S", "loglik", "dof", "info", "gamma")})))
            assert all(fg.lift_report(b)["kind"] == 0 and fg.lift_report(b)["info"] == 0 for b in range(3))
            fg.close()
        assert got[0] == got[1] == got[2], call
        # option on: the filter with one landmark reports kind 0 and equals the plain result bit for bit; its neighbours take the bundleLift
        fg = _handle(hip, snaps, lc.settings(1), 1)
        _call(fg, call, snaps)
        reps = [fg.lift_report(b) for b in range(3)]
        assert [r["kind"] for r in reps] == [0, 2, 2] and all(r["info"] == 0 for r in reps), (call, reps)
        assert _bits(_state(fg, 0)) == got[0]["state"][0] and _bits(reps[0]) == got[0]["rep"][0], call
        assert _bits(_state(fg, 1)["sigma"]) == got[0]["state"][1]["sigma"] and _bits(_state(fg, 1)["group"]) != got[0]["state"][1]["group"]
        fg.close()


# ---- 5. untouched on failure
def test_failed_lift_leaves_the_filter_untouched(hip):
    N = 20
    d = lc.settings(1)
    good = lc.snapshot(N)
    bad = lc.snapshot(N)
    n = 11 + 3 * N
    S = bad["sigma"].copy()
    S[n - 1, n - 1] = -abs(S[n - 1, n - 1])     # Sigma_e indefinite in the last landmark; S = H Sigma H^T + R of the calls below stays definite
    bad["sigma"] = S
    snaps = [good, bad, good]
    for call in CALLS:
        fg = _handle(hip, snaps, d, 1)
        err0 = fg.device_error()
        before = _bits(fg.dump_state(1))
        _, out = _call(fg, call, snaps, drop_last=True)
        reps = [fg.lift_report(b) for b in range(3)]
        assert [r["info"] for r in reps] == [0, 4, 0] and reps[1]["kind"] == 2, (call, reps)
        assert _bits(fg.dump_state(1)) == before, call
        if out is not None:
            assert list(out["info"]) == [0, 4, 0] and not np.any(out["gamma"][1]), (call, out["info"])
        assert fg.device_error() == err0
        # the neighbours: what a call without the failing filter leaves
        ref = _handle(hip, snaps, d, 1)
        _, out2 = _call(ref, call, snaps, mask=[1, 0, 1], drop_last=True)
        for b in (0, 2):
            assert _bits(fg.dump_state(b)) == _bits(ref.dump_state(b)) and _bits(fg.lift_report(b)) == _bits(ref.lift_report(b)), (call, b)
            if out is not None:
                assert all(_bits(out[k][b]) == _bits(out2[k][b]) for k in ("nis", "logdet_S", "loglik", "dof", "info", "gamma")), (call, b)
        assert ref.lift_report(1)["info"] == 3 and _bits(ref.dump_state(1)) == before
        fg.close()
        ref.close()


# ---- 6. reproducibility
def test_run_to_run_alone_and_in_a_batch_and_perturb(hip):
    d = lc.settings(1)
    s20, s41, s3 = lc.snapshot(20), lc.snapshot(41), lc.snapshot(3)
    for call in CALLS:
        runs = []
        for snaps in ([s20, s41, s3], [s20, s41, s3], [s3, s41, s20]):
            fg = _handle(hip, snaps, d, 1, cap=41 + lc.CAP_EXTRA)
            _call(fg, call, snaps)
            runs.append({len(s["ids"]): (_bits(_state(fg, b)), _bits(fg.lift_report(b))) for b, s in enumerate(snaps)})
            fg.close()
        fg = _handle(hip, [s20], d, 1, cap=41 + lc.CAP_EXTRA)
        _call(fg, call, [s20])
        alone = (_bits(_state(fg, 0)), _bits(fg.lift_report(0)))
        fg.close()
        assert runs[0] == runs[1], (call, "run to run")
        assert runs[0][20] == runs[2][20] == alone, (call, "position 0, position 2, alone")
    # eqf_perturb_filters == eqf_sample_sigma + eqf_apply_increment with the option on
    snaps = [s20, s3]
    z = np.random.default_rng(2600).standard_normal((2, 1, 11 + 3 * 20))
    for first in (0, 6):
        one, two = _handle(hip, snaps, d, 1), _handle(hip, snaps, d, 1)
        one.perturb(z, first=first, scale=[0.01, 0.02])
        eps = two.sample_sigma(z, local=False, first=first, scale=[0.01, 0.02])["eps"]
        two.apply_increment(eps[:, 0, :])
        for b in range(2):
            assert _bits(_state(one, b)) == _bits(_state(two, b)) and _bits(one.lift_report(b)) == _bits(two.lift_report(b)), (first, b)
            assert one.lift_report(b)["kind"] == 2 and one.lift_report(b)["info"] == 0
        one.close()
        two.close()


# ---- 7. errors before any effect
def test_option_errors(hip):
    fg = _handle(hip, [lc.snapshot(3)], lc.settings(1), None)
    for v in (-1, 2, 7):
        assert hip.lib().eqf_set_option(fg._h, b"innovation_lift", v) == hip.ERR_INVALID
    fg.apply_increment([lc.raw(3, lc.own_sigma(3))])
    assert fg.lift_report(0)["kind"] == 0     # (the refused values left the option off)
    assert hip.lib().eqf_get_lift_report(fg._h, 1, hip.LiftReport()) == hip.ERR_INVALID
    fg.close()
    f32 = hip.FilterBatch(lc.settings(1), capacity=8, batch=1, precision=hip.PRECISION_F32)
    for v in (0, 1):
        assert hip.lib().eqf_set_option(f32._h, b"innovation_lift", v) == hip.ERR_UNSUPPORTED
    f32.close()
