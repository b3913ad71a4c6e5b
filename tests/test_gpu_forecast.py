"""The non-mutating forecast (include/eqf_vio_amd.h: eqf_forecast; csrc/eqf_forecast.hpp) on the device, public API only.

Every output against the exact reference of tests/forecast_exact.py within its a-priori bound, ratio <= 1 entry by entry, over the cases of
tests/forecast_cases.py (the CPU holds the fp64 statements to the same bounds on the same cases: tests/test_forecast_exact.py); batches,
reproducibility, the zero horizon bit for bit against the getters, non-mutation bit for bit, the route the call replaces (copy, propagate,
getters), and every argument error.  No bound here comes from the device."""
import ctypes as C

import numpy as np
import pytest

import forecast_cases as fcs
import forecast_exact as fx

pytestmark = pytest.mark.gpu

_REF = {}


@pytest.fixture(scope="module")
def hip():
    from eqf_vio_amd import binding

    return binding


def reference(name, local):
    if (name, local) not in _REF:
        c = fcs.cases()[name]
        _REF[(name, local)] = fx.Reference(c.snap, c.settings(), c.imu, c.t1, local)
    return _REF[(name, local)]


def part(res, b):
    return {k: (v[b] if k != "status" else int(v[b])) for k, v in res.items()}


def handle(hip, case, batch=1, capacity=None, **kw):
    f = hip.FilterBatch(case.settings(), capacity=capacity or max(case.N, 1) + 3, batch=batch, **kw)
    return f


def check(got, R, what, bad, worst):
    r = fx.ratios(got, R)
    for k, v in r.items():
        worst[k] = max(worst.get(k, 0.0), v)
        if not v <= 1.0:
            bad.append((what, k, v))
    for k in ("lm", "S", "ycov"):  # exactly symmetric where the header says so
        A = np.asarray(got[k])
        if k != "lm" or what[-1] == 0:
            if not np.array_equal(A, np.swapaxes(A, -1, -2)):
                bad.append((what, k, "not symmetric"))
    if what[-1] == 0 and not np.array_equal(got["base"], got["base"].T):
        bad.append((what, "base", "not symmetric"))
    if got["steps"] != R.steps or got["time"] != R.time:
        bad.append((what, "steps/time", got["steps"], R.steps, got["time"], R.time))


def run_case(hip, name, bad, worst):
    c = fcs.cases()[name]
    f = handle(hip, c)
    try:
        f.restore_state(c.snap)
        for local in (1, 0):
            res = f.forecast(c.imu if len(c.imu) else None, c.t1, local=bool(local))
            assert res["status"][0] == 0, (name, res["status"])
            check(part(res, 0), reference(name, local), (name, local), bad, worst)
        assert f.device_error() == 0
    finally:
        f.close()


@pytest.mark.parametrize("name", fcs.GPU_SIZES)
def test_sizes_across_lane_wave_and_workgroup_edges(hip, name):
    """N = 0, 1, 63, 64, 65, 257: one sample and the closing step, both charts."""
    bad, worst = [], {}
    run_case(hip, name, bad, worst)
    print(f"{name}: worst ratio to the bound " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert not bad, bad[:10]


@pytest.mark.parametrize("name", ["k0t", "k1", "k1t", "k16", "k16t", "k17", "k17t", "k1t-exp", "k17t-exp", "back", "turn", "pole", "graded"])
def test_horizons_lifts_and_edge_states(hip, name):
    """K = 0 with t1, 1, 16, 17 with and without t1, both velocity lifts, stamps that do not advance in the middle of the samples, a 0.5 rad
    step, a gravity chart 1e-2 rad from its pole, scales over two decades (N = 5)."""
    bad, worst = [], {}
    run_case(hip, name, bad, worst)
    print(f"{name}: worst ratio to the bound " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert not bad, bad[:10]


def bits(res, b=None):
    """every output of a forecast as one tuple of byte strings (of filter b)"""
    keys = [k for k in res if k != "status"]
    return tuple(np.ascontiguousarray(x).tobytes() for k in keys for x in (res[k] if b is None else [res[k][b]])) + (
        () if b is not None else (res["status"].tobytes(),))


def test_batch_of_three_one_not_initialised_alone_and_twice(hip):
    """N = {0, 5, 65} and a fourth filter that was never initialised: each against its own reference; the fourth answers
    EQF_SKIPPED_NOT_INITIALISED with every output zero; a filter alone gives the bits it gives inside the batch; two calls give the same bits."""
    names = ("n0", "k1t", "n65")
    cs = [fcs.cases()[n] for n in names]
    # (one sample and t1 each: the samples are per filter)
    K = 1
    imu = np.zeros((K, 4, 7))
    t1 = np.zeros(4)
    for b, c in enumerate(cs):
        imu[:, b], t1[b] = c.imu, c.t1
    imu[:, 3], t1[3] = cs[1].imu, cs[1].t1
    f = hip.FilterBatch(cs[0].settings(), capacity=68, batch=4)
    bad, worst = [], {}
    try:
        for b, c in enumerate(cs):
            f.restore_state(c.snap, b)
        res = f.forecast(imu, t1, local=True)
        assert list(res["status"]) == [0, 0, 0, hip.SKIPPED_NOT_INITIALISED]
        for b, n in enumerate(names):
            check(part(res, b), reference(n, 1), (n, "batch", 1), bad, worst)
        for k in res:
            if k != "status":
                assert not np.any(res[k][3]), k
        again = f.forecast(imu, t1, local=True)
        assert bits(res) == bits(again)
        assert f.device_error() == 0
    finally:
        f.close()
    for b, c in enumerate(cs):
        g = hip.FilterBatch(c.settings(), capacity=68, batch=1)
        try:
            g.restore_state(c.snap)
            alone = g.forecast(c.imu, c.t1, local=True)
            assert bits(alone, 0) == bits(res, b), names[b]
        finally:
            g.close()
    assert not bad, bad[:10]


@pytest.mark.parametrize("name", ["n0", "k1", "n65"])
def test_zero_horizon_is_the_getters_bit_for_bit(hip, name):
    """K = 0 without t1, and samples none of which integrates: pose, velocity, p, base and lm are eqf_get_state_estimate's and
    eqf_get_marginals' bits in both charts; S against the exact reference."""
    c = fcs.cases()[name]
    f = handle(hip, c)
    try:
        f.restore_state(c.snap)
        est = f.state_estimate()
        stale = fcs.samples(2)
        stale[:, 0] = [c.snap["time"], c.snap["time"] - 0.001]  # neither advances: no step integrates
        for local in (True, False):
            m = f.marginals(local=local)
            for imu, t1, status in ((None, None, 0), (stale, c.snap["time"] - 0.002, hip.SKIPPED_NONPOSITIVE_DT)):
                res = f.forecast(imu, t1, local=local)
                assert res["status"][0] == status and res["steps"][0] == 0
                for k, want in (("pose_q", est["q"]), ("pose_x", est["x"]), ("velocity", est["v"]), ("p", est["p"]), ("base", m["base"]), ("lm", m["lm"])):
                    assert np.array_equal(res[k][0], want), (name, local, k)
        res = f.forecast(local=True)
        R = fx.Reference(c.snap, c.settings(), np.zeros((0, 7)), None, True)
        r = fx.ratios(part(res, 0), R, names=("S", "ycov", "bearing"))
        assert max(r.values()) <= 1.0, r
        assert res["time"][0] == c.snap["time"]
    finally:
        f.close()


def snapshot_bits(f, b=0):
    d = f.dump_state(b)
    flat = []
    for v in (d["ids"], d["bias"], d["sigma"], d["currentVelocity"], d["accumulatedVelocity"], d["origin"]["q"], d["origin"]["x"], d["origin"]["v"],
              d["origin"]["p"], d["group"]["Aq"], d["group"]["Ax"], d["group"]["w"], d["group"]["Qq"], d["group"]["Qa"]):
        flat.append(np.ascontiguousarray(v).tobytes())
    lu = f.last_update(b)
    gr = f.gate_report(b)
    st = f.innovation_stats(b)  # (valid = 0 and zeros while the option is off)
    return (tuple(flat), d["time"], d["accumulatedTime"], d["initialised"], tuple(np.ascontiguousarray(lu[k]).tobytes() for k in sorted(lu)),
            tuple(np.ascontiguousarray(gr[k]).tobytes() for k in sorted(gr)),
            (np.float64(st["nis"]).tobytes(), np.float64(st["logdet_S"]).tobytes(), st["dof"], st["valid"], st["nis_lm"].tobytes()), f.device_error())


def drive(hip, N=12, frames=3, gate=False, burst=0):
    """A handle driven over a short synthetic stream to a few IMU calls behind its third frame; returns (handle, stream, next imu index, next frame)."""
    from eqf_vio_amd import synth

    st = synth.make_stream(N, duration=0.4)
    f = hip.FilterBatch(synth.template_settings_dict(), capacity=N + 4, batch=1)
    f.set_option("innovation_stats", 1)
    if gate:
        from eqf_vio_amd import consistency as cs

        f.set_outlier_gate(hip.GATE_MAHALANOBIS, cs.chi2_gate_threshold(0.999))
    f.set_imu_burst(burst)
    ev = list(st.events())
    cut = [i for i, (kind, _) in enumerate(ev) if kind == "vision"][frames - 1] + 1
    for kind, k in ev[:cut]:
        if kind == "imu":
            f.process_imu([st.imu[k, 0]], st.imu[k, 1:4], st.imu[k, 4:7])
        else:
            f.process_vision([st.vision_stamps[k]], st.ids, st.bearings[k])
    return f, st, ev[cut:]


@pytest.mark.parametrize("burst,gate", [(0, False), (15, False), (15, True)])
def test_forecast_changes_nothing(hip, burst, gate):
    """Every getter answers with the same bits after a forecast as before it; two IMU calls and a vision frame afterwards give the bits of a
    twin that never forecast -- also with three IMU calls queued (burst 15) and with the speculative Mahalanobis gate pending, where the
    forecast's own outputs equal those after an explicit synchronize."""
    f, st, rest = drive(hip, burst=burst, gate=gate)
    twin, _, _ = drive(hip, burst=burst, gate=gate)
    try:
        imus = [k for kind, k in rest if kind == "imu"]
        queued = imus[:3]
        for g in (f, twin):
            for k in queued:  # (burst 15: these stay queued, behind the frame whose gate answer is still pending)
                g.process_imu([st.imu[k, 0]], st.imu[k, 1:4], st.imu[k, 4:7])
        ahead = st.imu[imus[3]:imus[3] + 4].copy()
        t1 = ahead[-1, 0] + 0.002
        res = f.forecast(ahead, t1, local=True)
        assert res["status"][0] == 0 and res["steps"][0] == 5
        twin.synchronize()
        before = snapshot_bits(twin)
        assert snapshot_bits(f) == before
        res2 = f.forecast(ahead, t1, local=True)
        assert bits(res) == bits(res2)       # (the second call found nothing deferred: the same outputs as with the queue and the gate pending)
        assert snapshot_bits(f) == before
        nxt = [e for e in rest if not (e[0] == "imu" and e[1] in queued)]
        n_imu = 0
        for kind, k in nxt:
            for g in (f, twin):
                if kind == "imu":
                    g.process_imu([st.imu[k, 0]], st.imu[k, 1:4], st.imu[k, 4:7])
                else:
                    g.process_vision([st.vision_stamps[k]], st.ids, st.bearings[k])
            n_imu += kind == "imu"
            if kind == "vision" and n_imu >= 2:
                break
        assert snapshot_bits(f) == snapshot_bits(twin)
    finally:
        f.close()
        twin.close()


@pytest.mark.parametrize("burst", [0, 15])
def test_against_copy_propagate_and_getters(hip, burst):
    """The route the call replaces: eqf_copy_filters into a second handle, the same samples through eqf_process_imu there, the getters.  Both
    results lie within the bound of the same reference, so they differ by at most twice the bound, entry by entry.  Then a Mahalanobis-gated
    frame on the propagated copy: the d2 its gate reports is gate_distance(S, delta) of the forecast's S with the copy's own residual, to
    the bound of S pushed through d2 = delta^T S^-1 delta."""
    from eqf_vio_amd import consistency as cs

    c = fcs.cases()["k16"]
    f = handle(hip, c)
    g = handle(hip, c)
    try:
        f.restore_state(c.snap)
        g.set_imu_burst(burst)
        g.set_outlier_gate(hip.GATE_MAHALANOBIS, 1e300)
        res = part(f.forecast(c.imu, None, local=True), 0)
        res0 = part(f.forecast(c.imu, None, local=False, want=("lm", "base")), 0)
        g.copy_filters(f, [0], [0])
        for r in c.imu:
            g.process_imu([r[0]], r[1:4], r[4:7])
        est, m1, m0 = g.state_estimate(), g.marginals(local=True), g.marginals(local=False)
        R1, R0 = reference("k16", 1), reference("k16", 0)
        for k, a, b, bound in (("p", res["p"], est["p"], R1.bound["p"]), ("velocity", res["velocity"], est["v"], R1.bound["velocity"]),
                               ("pose_x", res["pose_x"], est["x"], R1.bound["pose_x"]), ("base", res["base"], m1["base"], R1.bound["base"]),
                               ("lm", res["lm"], m1["lm"], R1.bound["lm"]), ("base0", res0["base"], m0["base"], R0.bound["base"]),
                               ("lm0", res0["lm"], m0["lm"], R0.bound["lm"])):
            assert np.all(np.abs(np.asarray(a) - np.asarray(b)) <= 2 * np.asarray(bound, dtype=float)), k
        assert np.abs(fx.rotation_of(res["pose_q"]) - fx.rotation_of(est["q"])).max() <= 2 * R1.bound["pose_R"].max()
        # a frame on the copy at the time reached + 3 ms: the forecast WITH that stamp gives the S its gate divides by
        t1 = c.after()
        fr = part(f.forecast(c.imu, t1, local=True, want=("S", "bearing")), 0)
        y = fr["bearing"] + 1e-3 * np.random.default_rng(4).standard_normal(fr["bearing"].shape)
        y /= np.linalg.norm(y, axis=1, keepdims=True)
        assert g.process_vision([t1], c.snap["ids"], y)[0] == 0
        rep = g.gate_report()
        delta = g.last_update()["delta"].reshape(-1, 2)
        d2 = cs.gate_distance(fr["S"], delta)
        Rt = fx.Reference(c.snap, c.settings(), c.imu, t1, True)
        # |d(d2)| <= |w|^T dS |w| with w = S^-1 delta, twice (both sides carry a dS), plus 16 u d2 for the two 2 x 2 solves
        for i in range(c.N):
            w = np.linalg.solve(fr["S"][i], delta[i])
            tol = 2 * np.abs(w) @ Rt.bound["S"][i] @ np.abs(w) + 16 * fx.U * d2[i]
            assert abs(rep["stat"][i] - d2[i]) <= tol, (i, rep["stat"][i], d2[i], tol)
        assert g.device_error() == 0 and f.device_error() == 0
    finally:
        f.close()
        g.close()


def test_argument_errors_leave_the_handle_alone(hip):
    c = fcs.cases()["k1t"]
    L = hip.lib()
    d = c.settings()
    for kw, sett in ((dict(precision=hip.PRECISION_F32), d), ({}, dict(d, fastRiccati=1))):
        f = hip.FilterBatch(sett, capacity=8, batch=1, **kw)
        try:
            with pytest.raises(hip.EqfError) as ei:
                f.forecast(c.imu, c.t1)
            assert ei.value.code == hip.ERR_UNSUPPORTED
        finally:
            f.close()
    f = handle(hip, c)
    try:
        f.restore_state(c.snap)
        before = snapshot_bits(f)
        out = hip.ForecastOut()
        pbuf = np.zeros((c.N, 3))
        tbuf = np.zeros(1)
        imu = np.ascontiguousarray(c.imu)
        dp = C.POINTER(C.c_double)
        P = lambda a: a.ctypes.data_as(dp)  # noqa: E731
        t1 = np.array([c.t1])
        call = lambda K, im, t, local, stride, o: L.eqf_forecast(f._h, K, im, t, local, stride, o, None)  # noqa: E731
        assert call(1, P(imu), P(t1), 1, 0, None) == hip.ERR_INVALID              # NULL out
        assert L.eqf_forecast(None, 1, P(imu), P(t1), 1, 0, C.byref(out), None) == hip.ERR_INVALID
        assert call(-1, P(imu), P(t1), 1, 0, C.byref(out)) == hip.ERR_INVALID
        assert call(257, P(imu), P(t1), 1, 0, C.byref(out)) == hip.ERR_INVALID
        assert call(1, None, P(t1), 1, 0, C.byref(out)) == hip.ERR_INVALID         # imu NULL with K > 0
        assert call(0, P(imu), P(t1), 1, 0, C.byref(out)) == hip.ERR_INVALID       # imu given with K = 0
        assert call(1, P(imu), P(t1), 2, 0, C.byref(out)) == hip.ERR_INVALID       # local
        out.p = P(pbuf)
        assert call(1, P(imu), P(t1), 1, c.N - 1, C.byref(out)) == hip.ERR_INVALID  # stride below N with a per-landmark output
        assert call(1, P(imu), P(t1), 1, c.N, C.byref(out)) == hip.EQF_OK
        out.p = None
        out.time = P(tbuf)
        assert call(1, P(imu), P(t1), 1, 0, C.byref(out)) == hip.EQF_OK             # ... and without one the stride is not looked at
        for bad in (np.nan, np.inf):
            im = imu.copy()
            im[0, 0] = bad
            assert call(1, P(im), P(t1), 1, 0, C.byref(out)) == hip.ERR_INVALID
            assert call(1, P(imu), P(np.array([bad])), 1, 0, C.byref(out)) == hip.ERR_INVALID
        assert snapshot_bits(f) == before
        # a NaN rate is the caller's: that filter's status is EQF_ERR_NUMERIC, its outputs NaN, and nothing is raised in the handle
        im = imu.copy()
        im[0, 2] = np.nan
        res = f.forecast(np.concatenate([im, fcs.samples(2)[1:]]), None)
        assert res["status"][0] == hip.ERR_NUMERIC and np.all(np.isnan(res["base"][0])) and np.all(np.isnan(res["p"][0]))
        assert snapshot_bits(f) == before
    finally:
        f.close()
