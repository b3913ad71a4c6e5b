"""The low-rank linear measurement update on the device (csrc/eqf_linear.hpp: eqf_update_linear; FilterBatch.update_linear) entry by entry
against the reference and the a-priori bound of tests/linear_exact.py, on the cases of tests/linear_cases.py that tests/test_linear_exact.py
holds the CPU restatements to.  Every reference starts from the device's own sigma(), origin() and group() before the call; R goes in with its
upper triangle negated (only the lower triangle may be read).  Everything that is not arithmetic is bit for bit: the group step against
set_sigma + apply_increment on a second handle, untouched filters, a filter alone against the same filter inside a batch, a twin restored from
a dump, the C++ facade.  Nothing here provokes a fault: the indefinite S is an ordinary numeric verdict of the solve kernel.
Worst device / bound ratios on an MI355X: NOTES.md R18.1 (each test prints its own)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import consistency_cases as cc
import consistency_exact as cx
import linear_cases as lc
import linear_exact as le
from eqf_vio_amd import consistency as cs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip():
    from eqf_vio_amd import binding

    return binding


@pytest.fixture(scope="module")
def master_J():
    s = cc.local_state(max(lc.SIZES + lc.RAGGED), lc.THETA)
    return cx.jacobian_mp(s["origin"], s["group"])


@pytest.fixture(scope="module")
def own_sigma(hip):
    """{N: a filter's own Sigma after five vision frames}"""
    from eqf_vio_amd import synth

    out = {}
    for N in sorted({n for n in lc.SIZES + lc.RAGGED if n}):
        st = synth.make_stream(N, duration=0.4)
        fg = hip.FilterBatch(cc.settings(), capacity=N + lc.CAP_EXTRA, batch=1)
        seen = 0
        for kind, k in st.events():
            if kind == "imu":
                r = st.imu[k]
                fg.process_imu(r[0], r[1:4], r[4:7])
            else:
                fg.process_vision(st.vision_stamps[k], st.ids, st.bearings[k])
                seen += 1
                if seen == 5:
                    break
        assert fg.num_landmarks(0) == N and fg.device_error() == 0
        out[N] = fg.sigma(0)
        fg.close()
    return out


def _poison(R):
    return np.tril(R) - np.triu(R, 1)


def _bits(x):
    if isinstance(x, dict):
        return {k: _bits(v) for k, v in x.items()}
    return np.ascontiguousarray(x).tobytes() + str(np.asarray(x).shape).encode()


def _assert_same(a, b, what):
    a, b = _bits(a), _bits(b)
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k], f"{what}: {k} differs"


def _getters(fg, b, last=True):
    """everything a caller can read of filter b (last = False: without the records of the last vision update, which a handle that has
    never run one does not have -- for comparisons ACROSS handles)"""
    g = dict(n=fg.num_landmarks(b), est=fg.state_estimate(b), innov=fg.innovation_stats(b), gate=fg.gate_report(b),
             og=np.array(fg.outlier_gate(), dtype=float))
    if last:
        g["last"] = fg.last_update(b)
    g.update(fg.dump_state(b))  # ids, origin, group, bias, sigma, time, integrator
    return g


def _same_state(fg, b, snap):
    o, g = fg.origin(b), fg.group(b)
    for k in ("q", "x", "v", "p"):
        assert np.array_equal(o[k], snap["origin"][k]), k
    for k in ("Aq", "Ax", "w", "Qq", "Qa"):
        assert np.array_equal(g[k], snap["group"][k]), k


def _operands(snap, S0, N, local, m, hfam, rkind, seed=0):
    H = lc.rows(N, m, hfam, seed)
    Ht64 = H @ cs.jacobian_matrix(cs.local_jacobian_blocks(snap["origin"], snap["group"])) if local else H
    R = lc.noise(S0, Ht64, H.shape[0], rkind, seed)
    return H, R, lc.residual(S0, Ht64, R, seed)


def _reference(S0, H, r, R, local, master_J):
    Ht, dHt = le.rows(H, local, master_J)
    ref = le.reference(S0, Ht, r, R)
    bnd = le.bounds(ref, dHt)
    assert bnd["validity"] <= le.VALIDITY
    return ref, bnd


def _got(out, b, Sp, n):
    return dict(Sigma=Sp, gamma=out["gamma"][b, :n], nis=out["nis"][b], logdet_S=out["logdet_S"][b], loglik=out["loglik"][b])


# ---- 1. entry by entry, and the group step
@pytest.mark.parametrize("N", lc.SIZES)
def test_update_entry_by_entry_and_the_group_step(hip, master_J, own_sigma, N):
    n = 11 + 3 * N
    worst = {}
    for fam, local, m, hfam, rkind in lc.plan(N):
        what = (N, fam, local, m, hfam, rkind)
        snap = lc.snapshot(N, fam, own_sigma.get(N))
        fg = hip.FilterBatch(cc.settings(), capacity=N + lc.CAP_EXTRA, batch=1)
        fg.restore_state(snap, 0)
        _same_state(fg, 0, snap)
        pre = fg.dump_state(0)
        pre_last = fg.last_update(0)
        S0 = fg.sigma(0)
        assert np.array_equal(S0, S0.T), what
        H, R, r = _operands(snap, S0, N, local, m, hfam, rkind)
        ref, bnd = _reference(S0, H, r, R, local, master_J)
        out = fg.update_linear(H, r, _poison(R), local=bool(local), want_gamma=True)
        assert out["info"][0] == 0 and out["dof"][0] == H.shape[0], what
        Sp = fg.sigma(0)
        assert Sp.tobytes() == np.ascontiguousarray(Sp.T).tobytes(), (what, "Sigma+ is not bit-for-bit symmetric")
        for k, v in le.ratios(_got(out, 0, Sp, n), ref, bnd).items():
            worst[k] = max(worst.get(k, 0.0), v)
            assert v <= 1.0, (what, k, v)
        # what stays: origin, clock, integrator, ids
        post = fg.dump_state(0)
        for k in ("ids", "origin", "time", "currentVelocity", "accumulatedVelocity", "accumulatedTime", "initialised"):
            assert _bits(post[k]) == _bits(pre[k]), (what, k)
        _assert_same(fg.last_update(0), pre_last, what)
        # the group step is eqf_apply_increment's with the gamma the call returned
        fb = hip.FilterBatch(cc.settings(), capacity=N + lc.CAP_EXTRA, batch=1)
        fb.restore_state(pre, 0)
        fb.set_sigma(Sp, 0)
        fb.apply_increment(out["gamma"][:, :n])
        _assert_same(_getters(fg, 0, last=False), _getters(fb, 0, last=False), what)
        assert _bits(post["group"]) != _bits(pre["group"]) and fg.device_error() == 0, what
        fg.close(), fb.close()
    print(f"N={N}: worst device / bound  " + "  ".join(f"{k} {worst[k]:.3f}" for k in ("Sp", "gamma", "nis", "logdet_S", "loglik")))


# ---- 2. the ragged handle: mask, gate, and a filter alone against the same filter in a batch
def test_ragged_handle_mask_and_gate(hip, master_J, own_sigma):
    counts, mask = lc.RAGGED, lc.RAGGED_MASK
    fams = ("graded", "own", "coupled", "one_small")
    fg = hip.FilterBatch(cc.settings(), capacity=max(counts) + lc.CAP_EXTRA, batch=len(counts))
    snaps = [lc.snapshot(N, fams[b], own_sigma.get(N)) for b, N in enumerate(counts)]
    for b, s in enumerate(snaps):
        fg.restore_state(s, b)
    S0 = [fg.sigma(b) for b in range(4)]
    ops = [_operands(snaps[b], S0[b], N, 1, 3, "dense", "dense", seed=b) for b, N in enumerate(counts)]
    refs = [_reference(S0[b], ops[b][0], ops[b][2], ops[b][1], 1, master_J) for b in range(4)]
    nis = sorted((float(refs[b][0]["nis"]), b) for b in range(4) if mask[b])
    gate = math.sqrt(nis[-1][0] * nis[-2][0])  # between the two largest reference values of the filters that take part
    assert (nis[-1][0] - gate) / gate >= 1e-3 and (gate - nis[-2][0]) / gate >= 1e-3, nis
    gated = nis[-1][1]
    before = [_getters(fg, b) for b in range(4)]
    out = fg.update_linear([o[0] for o in ops], [o[2] for o in ops], [_poison(o[1]) for o in ops], local=True, gate=gate, mask=mask,
                           want_gamma=True)
    want = [3 if not mask[b] else (2 if b == gated else 0) for b in range(4)]
    assert list(out["info"]) == want, (list(out["info"]), want)
    for b, N in enumerate(counts):
        n = 11 + 3 * N
        if want[b]:
            _assert_same(_getters(fg, b), before[b], f"untouched filter {b} (info {want[b]})")
            assert not out["gamma"][b].any()
            if want[b] == 2:  # (a gated filter still reports what the gate looked at)
                rt = le.ratios(dict(Sigma=S0[b], gamma=np.zeros(n), nis=out["nis"][b], logdet_S=out["logdet_S"][b], loglik=out["loglik"][b]),
                               dict(refs[b][0], Sp=S0[b], gamma=np.zeros(n)), refs[b][1])
                assert max(rt.values()) <= 1.0, rt
            else:
                assert np.isnan(out["nis"][b])
        else:
            Sp = fg.sigma(b)
            assert Sp.tobytes() == np.ascontiguousarray(Sp.T).tobytes()
            rt = le.ratios(_got(out, b, Sp, n), *refs[b])
            print(f"ragged, filter {b} (N={N}): device / bound", {k: round(v, 3) for k, v in rt.items()})
            assert max(rt.values()) <= 1.0, (b, rt)
            assert not out["gamma"][b, n:].any()
    assert fg.device_error() == 0


def test_alone_and_at_index_2_of_3_and_from_run_to_run(hip, own_sigma):
    N = 43
    n = 11 + 3 * N
    snap = lc.snapshot(N, "own", own_sigma[N])
    H, R, r = _operands(snap, snap["sigma"], N, 1, 15, "dense", "dense")
    res = []
    for batch, b, cap in ((1, 0, N + 7), (1, 0, N + 7), (3, 2, N + 2)):
        fg = hip.FilterBatch(cc.settings(), capacity=cap, batch=batch)
        fg.restore_state(snap, b)
        Hs = [np.zeros((15, 11))] * b + [H]
        out = fg.update_linear(Hs, [np.zeros(15)] * b + [r], [np.eye(15)] * b + [_poison(R)], local=True, mask=[0] * b + [1], want_gamma=True)
        assert out["info"][b] == 0 and all(out["info"][:b] == 3)
        res.append((fg.dump_state(b), dict(gamma=out["gamma"][b, :n], nis=out["nis"][b], logdet_S=out["logdet_S"][b], loglik=out["loglik"][b])))
        fg.close()
    for k in (1, 2):
        _assert_same(res[0][0], res[k][0], f"state, run {k}")
        _assert_same(res[0][1], res[k][1], f"report, run {k}")
    assert _bits(res[0][0]) != _bits(snap)


# ---- 3. failure paths
def test_indefinite_S_and_singular_chart_are_verdicts_per_filter(hip, own_sigma):
    N = 18
    snap = lc.snapshot(N, "own", own_sigma[N])
    fg = hip.FilterBatch(cc.settings(), capacity=N + 7, batch=2)
    fg.restore_state(snap, 0)
    fg.restore_state(snap, 1)
    H = lc.rows(N, 3, "dense")
    J = cs.jacobian_matrix(fg.local_jacobian(0) if False else cs.local_jacobian_blocks(snap["origin"], snap["group"]))
    c = 2.0 * float(np.linalg.eigvalsh(H @ J @ snap["sigma"] @ J.T @ H.T).max())
    before = [_getters(fg, b) for b in range(2)]
    out = fg.update_linear([H, H], np.full((2, 3), 0.01), [-c * np.eye(3), c * np.eye(3)], local=True, want_gamma=True)
    assert list(out["info"]) == [1, 0] and np.isnan(out["nis"][0]) and np.isfinite(out["nis"][1])
    _assert_same(_getters(fg, 0), before[0], "the filter whose S is not positive definite")
    assert _bits(fg.dump_state(1)) != _bits({k: before[1][k] for k in fg.dump_state(1)})
    assert fg.device_error() == 0
    # a filter that has not been initialised: the origin's gravity direction is the pole of its own chart
    f0 = hip.FilterBatch(cc.settings(), capacity=4, batch=1)
    pre = f0.dump_state(0)
    o = f0.update_linear(cs.velocity_rows(0), np.zeros(3), np.eye(3), local=True, want_gamma=True)
    assert o["info"][0] == -1 and not o["gamma"].any()
    _assert_same(f0.dump_state(0), pre, "uninitialised filter, local rows")
    assert f0.update_linear(cs.velocity_rows(0), np.zeros(3), np.eye(3), local=False)["info"][0] == 0  # (the origin chart needs no J)
    assert f0.device_error() == 0


def test_argument_errors_come_before_any_effect(hip, own_sigma):
    from eqf_vio_amd import synth

    N = 5
    n = 11 + 3 * N
    snap = lc.snapshot(N, "own", own_sigma[N])
    fg = hip.FilterBatch(cc.settings(), capacity=N + 2, batch=2)
    for b in range(2):
        fg.restore_state(snap, b)
    f32 = hip.FilterBatch(cc.settings(), capacity=N, batch=2, precision=hip.PRECISION_F32)
    st = synth.make_stream(N, duration=0.4)
    for kind, k in list(st.events())[:30]:
        if kind == "imu":
            f32.process_imu(st.imu[k][0], st.imu[k][1:4], st.imu[k][4:7])
    L = hip.lib()
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_ubyte)
    P = lambda a: a.ctypes.data_as(dp) if a is not None else None  # noqa: E731
    m = 3
    H = np.ascontiguousarray(np.broadcast_to(lc.rows(N, m, "dense"), (2, m, n)))
    r, R = np.full((2, m), 0.01), np.ascontiguousarray(np.broadcast_to(np.eye(m), (2, m, m)))
    G = np.full((2, n), -7.0)
    rep = (hip.LinearReport * 2)()
    for s in rep:
        s.nis, s.dof, s.info = -7.0, -7, -7
    mask01 = np.array([1, 0], dtype=np.uint8)

    def call(h, local=1, mm=m, Hh=H, ldh=n, rr=r, RR=R, gate=np.inf, mask=None, g=G, ldg=n, rp=rep):
        return L.eqf_update_linear(h, local, mm, P(Hh), ldh, P(rr), P(RR), gate, None if mask is None else mask.ctypes.data_as(up), P(g), ldg, rp)

    def poisoned(a, idx, v):
        a = a.copy()
        a[idx] = v
        return a

    before = [_getters(fg, b) for b in range(2)]
    before32 = [f32.dump_state(b) for b in range(2)]
    bad = [dict(local=2), dict(local=-1), dict(mm=0), dict(mm=17), dict(Hh=None), dict(rr=None), dict(RR=None), dict(ldh=n - 1), dict(ldg=n - 1),
           dict(gate=np.nan), dict(gate=0.0), dict(gate=-1.0), dict(Hh=poisoned(H, (1, 2, n - 1), np.nan)), dict(Hh=poisoned(H, (0, 0, 0), np.inf)),
           dict(rr=poisoned(r, (1, 1), np.nan)), dict(RR=poisoned(R, (0, 2, 1), np.inf)), dict(RR=poisoned(R, (1, 0, 0), np.nan)),
           dict(Hh=poisoned(H, (0, 1, 3), np.nan), mask=mask01)]
    for kw in bad:
        assert call(fg._h, **kw) == hip.ERR_INVALID, {k: (v if not isinstance(v, np.ndarray) else "array") for k, v in kw.items()}
    assert call(None) == hip.ERR_INVALID
    assert call(f32._h) == hip.ERR_UNSUPPORTED
    assert np.all(G == -7.0) and all(s.nis == -7.0 and s.dof == -7 and s.info == -7 for s in rep)
    for b in range(2):
        _assert_same(_getters(fg, b), before[b], f"after the refused calls, slot {b}")
        _assert_same(f32.dump_state(b), before32[b], f"after the refused calls, fp32 slot {b}")
    assert fg.device_error() == 0 and f32.device_error() == 0
    # good arguments work; what is wrong with a masked-out filter's operands or with R's upper triangle is nobody's business
    assert call(fg._h, Hh=poisoned(H, (1, 1, 3), np.nan), RR=poisoned(R, (0, 0, 2), np.nan), mask=mask01, ldg=n) == 0
    assert [s.info for s in rep] == [0, 3] and rep[0].dof == m and np.all(G[1] == 0.0) and G[0].any()
    _assert_same(_getters(fg, 1), before[1], "masked-out slot")
    assert call(fg._h, g=None, ldg=0, rp=None) == 0  # (enqueues and returns)
    assert fg.device_error() == 0


# ---- 4. the twin: host caches
@pytest.mark.parametrize("mode", ["per call", "per call, churn and gate", "stream mode, gate"])
def test_twin_restored_after_the_update_runs_bit_for_bit(hip, mode):
    """Three IMU calls are queued when the update arrives (it settles them: the burst has left C Sigma and S behind).  A stale cache on the
    host or the device, or a pad row that is not zero, would show as a difference between the updated handle and a fresh handle restored
    from its dump: ten IMU calls and a vision frame, twice, every getter after each frame."""
    from eqf_vio_amd import synth

    N = 30
    st = synth.make_stream(N, duration=0.4)
    stream, churn = mode.startswith("stream"), "churn" in mode
    meas = synth.churn_measurements(st, seed=7, outlier_frames=(3, 4), outlier_angle=0.2) if churn else None
    cap = N if churn else N + 5
    d = synth.template_settings_dict()
    fa, fb = hip.FilterBatch(d, capacity=cap, batch=2), hip.FilterBatch(d, capacity=cap, batch=2)
    for h in (fa, fb):
        h.set_option("innovation_stats", 1)
        if "gate" in mode:
            h.set_outlier_gate(hip.GATE_MAHALANOBIS, 9.21)
        if stream:
            h.stream_upload(st.imu, st.vision_stamps, st.ids, st.bearings)

    def events(f0, f1):
        out, f = [], 0
        for kind, k in st.events():
            if f >= f1:
                break
            if f >= f0:
                out.append((kind, k))
            if kind == "vision":
                f += 1
        return out

    def rest(h, ev):
        for kind, k in ev:
            if stream:
                h.stream_imu(k) if kind == "imu" else h.stream_vision(k)
            elif kind == "imu":
                h.process_imu(st.imu[k][0], st.imu[k][1:4], st.imu[k][4:7])
            elif meas is not None:
                h.process_vision(st.vision_stamps[k], *meas[k])
            else:
                h.process_vision(st.vision_stamps[k], st.ids, st.bearings[k])

    rest(fa, events(0, 3))
    nxt = events(3, 4)
    rest(fa, nxt[:3])
    # a speed measurement that agrees with the estimate to a centimetre per second, and a gentle one of the gravity direction
    Ns = [fa.num_landmarks(b) for b in range(2)]
    Hs = [np.vstack([cs.velocity_rows(Nb), cs.gravity_rows(Nb)]) for Nb in Ns]
    out = fa.update_linear(Hs, np.array([[0.01, -0.005, 0.008, 1e-3, -2e-3], [-0.004, 0.006, 0.002, 5e-4, 1e-3]]), np.diag([1e-3] * 3 + [1e-4] * 2),
                           local=True, gate=cs.chi2_gate_threshold(0.9999, dof=5))
    assert np.all(out["info"] == 0), out
    for b in range(2):
        fb.restore_state(fa.dump_state(b), b)
        _assert_same(fb.dump_state(b), fa.dump_state(b), f"{mode}: restored slot {b}")
    for f, ev in ((3, nxt[3:]), (4, events(4, 5))):
        assert sum(kind == "imu" for kind, _ in events(f, f + 1)) == 10
        rest(fa, ev), rest(fb, ev)
        for b in range(2):
            ga, gb = _getters(fa, b), _getters(fb, b)
            _assert_same(ga, gb, f"{mode}: slot {b} after frame {f}")
            assert fa.innovation_stats(b)["valid"]
    assert fa.device_error() == 0 and fb.device_error() == 0


# ---- 5. sign and chart on the device
@pytest.mark.parametrize("what", ["velocity", "landmark"])
def test_sign_and_chart_on_the_device(hip, what):
    for N in (5, 18):
        snap, H, resid, R, truth, est, sl, J = lc.sign_and_chart_case(N, what, 0)
        fg = hip.FilterBatch(cc.settings(), capacity=N + 7, batch=1)
        fg.restore_state(snap, 0)
        e0 = fg.state_estimate(0)
        before = lc.measured_error(e0, truth, fg.bias(0), truth["bias"], sl)
        assert fg.update_linear(H, resid, R, local=True)["info"][0] == 0
        after = lc.measured_error(fg.state_estimate(0), truth, fg.bias(0), truth["bias"], sl)
        ratio = float(np.linalg.norm(after) / np.linalg.norm(before))
        print(f"{what} N={N}: measured error after / before {ratio:.2e}")
        assert ratio < 0.1, (what, N, ratio)
        assert fg.device_error() == 0
        fg.close()


# ---- 6. the C++ facade
def test_cpp_facade_against_the_python_binding_bit_for_bit(hip):
    """VIOFilter::processLinearMeasurement of cpp/VIOFilter.h through the example binary (argument `linear`, hexadecimal floats) against
    filter.VIOFilter.process_linear_measurement on the same sequence."""
    from eqf_vio_amd import filter as vf

    N, frames = 20, 6
    exe = os.path.join(ROOT, "eqf_vio_amd", "cpp", "eqf_example")
    out = subprocess.run([exe, str(N), str(frames), "linear"], capture_output=True, text=True, check=True).stdout.splitlines()
    reps = [ln.split()[1:] for ln in out if ln.startswith("linear ")]
    states = [ln.split()[1:] for ln in out if ln.startswith("updated ")]
    assert len(reps) == 2 and len(states) == 2
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
        est = fg.stateEstimate()
    n = 11 + 3 * N
    H2 = np.array([[math.sin(0.3 * i + kk) for i in range(n)] for kk in range(2)])
    calls = [(cs.velocity_rows(N), -np.asarray(est.velocity), 1e-4 * np.eye(3), True, np.inf),
             (H2, np.array([0.01, -0.02]), np.array([[0.02, 7.0], [0.005, 0.03]]), False, 50.0)]
    for (H, r, R, local, gate), rep, state in zip(calls, reps, states):
        got = fg.process_linear_measurement(H, r, R, local=local, gate=gate)
        assert (int(rep[0]), int(rep[1])) == (got["dof"], got["info"]) == (len(r), 0)
        assert np.array([float.fromhex(x) for x in rep[2:5]]).tobytes() == np.array([got["nis"], got["logdet_S"], got["loglik"]]).tobytes()
        e, S = fg.stateEstimate(), fg.stateCovariance()
        want = np.concatenate([e.pose_q, e.pose_x, e.velocity, S.reshape(-1)])
        assert int(state[0]) == N
        assert np.array([float.fromhex(x) for x in state[1:]]).tobytes() == want.tobytes()


# ---- 7. the route
def test_route_four_launches_and_nothing_of_the_vision_update(hip, own_sigma):
    N = 43
    snap = lc.snapshot(N, "own", own_sigma[N])
    fg = hip.FilterBatch(cc.settings(), capacity=N + 7, batch=1)
    fg.restore_state(snap, 0)
    fg.profile_enable(True)
    H, R, r = _operands(snap, snap["sigma"], N, 1, 3, "velocity", "diag")
    calls = 3
    for _ in range(calls):
        assert fg.update_linear(H, r, R, local=True)["info"][0] == 0
    prof = fg.profile()
    for k in ("k_lin_rows", "k_lin_gain", "k_lin_solve", "k_lin_downdate"):
        assert prof[k][0] == calls, (k, prof[k])
    for k in ("k_update_prep", "k_chol_step", "k_update_reduce", "k_update_finish", "k_downdate", "k_chol_step_dd", "k_chol_resident",
              "k_propagate", "k_imu_burst", "k_dense_riccati"):
        assert prof[k][0] == 0, (k, prof[k])
    fg.profile_enable(False)
    assert fg.device_error() == 0
