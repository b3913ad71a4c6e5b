"""The moment-matched mixture on the device (eqf_get_mixture_moments / eqf_merge_filters, csrc/eqf_mixture.hpp) against the exact reference of
tests/mixture_exact.py built from the device's own getters, entry by entry and inside the a-priori bound; the bitwise facts the header
promises; the merge's write-back (a twin restored through eqf_set_state runs on bit for bit); sign and chart; verdicts and errors; the
route.  Sizes run over the edges of k_mix_reduce's blocking: kMixRows = 4 row landmarks and kMixLanes = 64 column landmarks per tile
(one below, at, one above), the 16-landmark tile of the propagate kernels, the 256-lane chunk of every other k_mix_* kernel (N = 255, 256,
257: second strips of k_mix_estimate / k_mix_error, several blocks of k_mix_mean / k_mix_store / k_mix_commit / k_mix_restore, the stride
loop of k_mix_report, five column chunks and 65 row blocks of k_mix_reduce), N = 0 and N = 1."""
import numpy as np
import pytest

import mixture_cases as mc
import mixture_exact as mx
from eqf_vio_amd import consistency as cs

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257)
COUNTS = (1, 2, 3, 5, 17)
POOL = 5          # distinct filters of a handle of cases
CAP_EXTRA = 3


@pytest.fixture(scope="module")
def hip():
    from eqf_vio_amd import binding

    return binding


def _bits(x):
    if isinstance(x, dict):
        return {k: _bits(v) for k, v in x.items()}
    return np.ascontiguousarray(x).tobytes() + str(np.asarray(x).shape).encode()


def _same(a, b, what):
    a, b = _bits(a), _bits(b)
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k], f"{what}: {k} differs"


def _getters(fg, b):
    g = dict(n=fg.num_landmarks(b), est=fg.state_estimate(b), gate=fg.gate_report(b), last=fg.last_update(b))
    g.update(fg.dump_state(b))
    return g


def _member(fg, b):
    m = fg.dump_state(b)
    m["estimate"] = fg.state_estimate(b)
    return m


def _handle(hip, N, batch=POOL, order=None):
    """a handle whose filters are the committed case members of size N (order: which member goes to which slot)"""
    fg = hip.FilterBatch(mc.cc.settings(), capacity=N + CAP_EXTRA, batch=batch)
    for b, k in enumerate(order if order is not None else range(batch)):
        if k is not None:
            fg.restore_state(mc.member(N, k), b)
    return fg


def _plan(n):
    """(idx, w, ref) over POOL filters: n = 3 has a weight that is exactly 0, n >= 5 repeated members"""
    idx = [k % POOL for k in range(n)] if n != 5 else [0, 1, 2, 3, 1]
    w = np.random.default_rng(900 + n).uniform(0.2, 1.5, n)
    if n == 3:
        w[1] = 0.0
    return idx, w, idx[(n - 1) // 2]


# ---- 1. entry by entry
@pytest.mark.parametrize("N", SIZES)
def test_moments_entry_by_entry(hip, N):
    fg = _handle(hip, N)
    pool = [_member(fg, b) for b in range(POOL)]
    worst = {}
    for n in COUNTS:
        idx, w, ref = _plan(n)
        ms = [pool[b] for b in idx]
        for centred in (True, False):
            got = fg.mixture_moments(idx, w, ref, centred)
            R = mx.reference(ms, w, idx.index(ref), centred, mc.K_E)
            assert R["bound"]["validity"] <= mx.VALIDITY
            assert got["info"] == 0 and got["n"] == n
            r = mx.ratios(got, R)
            for k, v in r.items():
                worst[k] = max(worst.get(k, 0.0), v)
            print(f"N={N} n={n} centred={centred}: " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
            assert max(r.values()) <= 1.0, (N, n, centred, r)
            assert got["P"].tobytes() == np.ascontiguousarray(got["P"].T).tobytes(), "P is not bit-for-bit symmetric"
            assert fg.debug_sigma_pad(ref, image=1) == 0.0, "pad row / column 11 of P is not exactly zero"
    print(f"N={N} worst ratios {worst}")
    assert fg.device_error() == 0
    fg.close()


# ---- 2. bitwise facts
def test_bitwise_facts(hip):
    N = 17
    fg = _handle(hip, N)
    for b in (0, 3):
        got = fg.mixture_moments([b], [0.7], b)
        S = fg.sigma_local(b)
        # (the lower triangle is computed with k_sigma_local's roundings, the upper is its mirror)
        assert np.tril(got["P"]).tobytes() == np.tril(S).tobytes(), "n = 1 is not sigma_local, bit for bit"
        assert got["mean"].tobytes() == np.zeros(11 + 3 * N).tobytes() and got["n_eff"] == 1.0 and got["spread_trace"] == 0.0
    idx, w, ref = [0, 1, 2, 3], np.array([0.5, 0.25, 1.0, 0.75]), 2
    a = fg.mixture_moments(idx, w, ref)
    b = fg.mixture_moments(idx, w, ref)
    _same(a, b, "run to run")
    z = fg.mixture_moments([0, 4, 1, 2, 4, 3], [0.5, 0.0, 0.25, 1.0, 0.0, 0.75], ref)
    for k in ("mean", "P", "spread_trace", "total_trace"):
        assert _bits(z[k]) == _bits(a[k]), f"a member of weight 0 changed {k}"
    # the same members at other positions of a larger, ragged handle
    fr = hip.FilterBatch(mc.cc.settings(), capacity=N + 40, batch=8)
    place = {0: 6, 1: 2, 2: 7, 3: 0}
    for k, b in place.items():
        fr.restore_state(mc.member(N, k), b)
    fr.restore_state(mc.member(33, 1), 1)
    fr.restore_state(mc.member(5, 2), 4)
    c = fr.mixture_moments([place[k] for k in idx], w, place[ref])
    for k in ("mean", "P", "spread_trace", "total_trace", "n_eff"):
        assert _bits(c[k]) == _bits(a[k]), f"{k} depends on where the members are"
    m1, m2 = fg.merge(idx, w, ref, 4), fr.merge([place[k] for k in idx], w, place[ref], 5)
    _same(m1, m2, "merge report")
    ga, gb = _getters(fg, 4), _getters(fr, 5)
    for k in ("est", "origin", "group", "bias", "sigma", "ids"):
        assert _bits(ga[k]) == _bits(gb[k]), f"merged {k} depends on where the members are"
    assert fg.device_error() == 0 and fr.device_error() == 0
    fg.close(), fr.close()


# ---- 3. the merge
@pytest.mark.parametrize("N,where", [(5, "free"), (17, "member"), (65, "ref"), (0, "member"), (257, "member")])
def test_merge_against_the_reference(hip, N, where):
    fg = _handle(hip, N, batch=POOL + 1)
    idx, w, ref = [0, 1, 2, 3, 1], np.array([0.4, 0.3, 0.0, 1.1, 0.6]), 3
    dst = dict(free=POOL, member=1, ref=ref)[where]
    ms = [_member(fg, b) for b in idx]
    before = [_getters(fg, b) for b in range(POOL + 1)]
    R = mx.merge_reference(ms, w, idx.index(ref), mc.K_E)
    assert R["bound"]["validity"] <= mx.VALIDITY
    rep = fg.merge(idx, w, ref, dst)
    assert rep["info"] == 0 and rep["n"] == len(idx)
    r = mx.merge_ratios(fg.state_estimate(dst), fg.bias(dst), fg.sigma_local(dst), R)
    r.update({k: abs(rep[k] - float(R[k])) / R["bound"][k] for k in ("n_eff", "spread_trace", "total_trace")})
    print(f"N={N} dst {where}: " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, r
    g = fg.group(dst)
    assert np.array_equal(g["Aq"], [1, 0, 0, 0]) and not g["Ax"].any() and not g["w"].any()
    assert np.array_equal(g["Qq"], np.tile([1.0, 0, 0, 0], (N, 1))) and np.array_equal(g["Qa"], np.ones(N))
    S = fg.sigma(dst)
    assert S.tobytes() == np.ascontiguousarray(S.T).tobytes()
    assert fg.debug_sigma_pad(dst, image=0) == 0.0, "pad row / column 11 of the merged Sigma is not exactly zero"
    after = _getters(fg, dst)
    for k in ("ids", "time", "currentVelocity", "accumulatedVelocity", "accumulatedTime", "initialised", "last"):
        assert _bits(after[k]) == _bits(before[ref][k]), k
    for b in range(POOL + 1):
        if b != dst:
            _same(_getters(fg, b), before[b], f"filter {b}, not the destination")
    assert fg.device_error() == 0
    fg.close()


def _run(h, st, events):
    for kind, k in events:
        if kind == "imu":
            h.process_imu(st.imu[k][0], st.imu[k][1:4], st.imu[k][4:7])
        else:
            h.process_vision(st.vision_stamps[k], st.ids, st.bearings[k])


def _frames(st, f0, f1):
    out, f = [], 0
    for kind, k in st.events():
        if f >= f1:
            break
        if f >= f0:
            out.append((kind, k))
        if kind == "vision":
            f += 1
    return out


def test_stream_members_merge_and_the_twin_runs_on_bit_for_bit(hip):
    """Members from one short synthetic stream: every filter resampled from one parent, perturbed with its own z and scale, run one more
    frame (the ids stay identical); the moments against the reference; then the merge into a member, and a twin handle restored through
    eqf_set_state from the destination's getters runs two more frames bit for bit like it -- a stale cache, a pad row that is not zero or
    constants that were not recomputed would show."""
    from eqf_vio_amd import synth

    N, B = 20, 4
    st = synth.make_stream(N, duration=0.4)
    d = synth.template_settings_dict()
    fa, fb = hip.FilterBatch(d, capacity=N + 4, batch=B), hip.FilterBatch(d, capacity=N + 4, batch=B)
    _run(fa, st, _frames(st, 0, 3))
    fa.resample(np.zeros(B, dtype=np.int32))
    fa.perturb(np.random.default_rng(5), scale=[0.0, 0.02, 0.05, 0.03])
    _run(fa, st, _frames(st, 3, 4))
    nxt = _frames(st, 4, 5)
    _run(fa, st, nxt[:3])  # (three IMU calls are queued when the merge arrives: it settles them)
    idx, w, ref = [0, 1, 2, 3], cs.mixture_weights([-1.0, -0.5, -2.0, -0.8]), 1
    ms = [_member(fa, b) for b in idx]
    assert all(np.array_equal(m["ids"], ms[0]["ids"]) for m in ms) and fa.device_error() == 0
    assert all(np.isfinite(m["sigma"]).all() and np.isfinite(m["estimate"]["p"]).all() and np.isfinite(m["bias"]).all() for m in ms)
    assert len({m["group"]["Aq"].tobytes() for m in ms}) == len(ms), "the perturbation did not pull the members apart"
    asym = max(float(np.abs(m["sigma"] - m["sigma"].T).max() / np.abs(m["sigma"]).max()) for m in ms)
    print(f"a filter's own Sigma is symmetric to {asym:.1e} of its largest entry (the kernels read its lower triangle)")
    got = fa.mixture_moments(idx, w, ref)
    Rm = mx.reference(ms, w, ref, True, mc.K_E)
    assert Rm["bound"]["validity"] <= mx.VALIDITY
    r = mx.ratios(got, Rm)
    print("stream members: " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert got["info"] == 0 and max(r.values()) <= 1.0, r
    R = mx.merge_reference(ms, w, ref, mc.K_E)
    assert fa.merge(idx, w, ref, 2, report=False) is None
    r = mx.merge_ratios(fa.state_estimate(2), fa.bias(2), fa.sigma_local(2), R)
    print("stream merge: " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, r
    for b in range(B):
        fb.restore_state(fa.dump_state(b), b)
        _same(fb.dump_state(b), fa.dump_state(b), f"restored slot {b}")
    for f, ev in ((4, nxt[3:]), (5, _frames(st, 5, 6))):
        _run(fa, st, ev), _run(fb, st, ev)
        for b in range(B):
            _same(_getters(fa, b), _getters(fb, b), f"slot {b} after frame {f}")
    assert fa.device_error() == 0 and fb.device_error() == 0
    fa.close(), fb.close()


# ---- 4. sign and chart
def test_sign_and_chart_on_the_device(hip):
    """Two copies of one filter moved by apply_increment by +-gamma in velocity, seen from the unmoved one (weight 0): eBar_velocity = 0 and
    the velocity block of P is Sigma_loc's plus R_A^T gamma gamma^T R_A.  The sign and the chart are told by hand tolerances of second
    order in |gamma| (apply_increment moves by a group exponential, linear in gamma only to first order); the values are held to the
    bound against the reference built from the moved filters' own getters, as everywhere else."""
    N = 5
    fg = _handle(hip, N, batch=3, order=[1, 1, 1])
    gam = np.array([2e-3, -1e-3, 1.5e-3])
    inc = np.zeros((3, 11 + 3 * N))
    inc[1, 8:11], inc[2, 8:11] = gam, -gam
    fg.apply_increment(inc)
    v = [fg.state_estimate(b)["v"] for b in range(3)]
    RAt = fg.local_jacobian(0)["RAt"]
    dv = RAt @ gam
    assert np.abs((v[1] - v[0]) - dv).max() < float(gam @ gam) and np.abs((v[2] - v[0]) + dv).max() < float(gam @ gam)
    got = fg.mixture_moments([0, 1, 2], [0.0, 1.0, 1.0], 0)
    assert got["info"] == 0
    g2 = float(gam @ gam)
    assert np.abs(got["mean"][8:11]).max() < g2
    want = 0.5 * (fg.sigma_local(1) + fg.sigma_local(2))[8:11, 8:11] + np.outer(dv, dv)
    assert np.abs(got["P"][8:11, 8:11] - want).max() < 1e-3 * g2, np.abs(got["P"][8:11, 8:11] - want).max() / g2
    R = mx.reference([_member(fg, b) for b in range(3)], [0.0, 1.0, 1.0], 0, True, mc.K_E)
    r = mx.ratios(got, R)
    print("sign and chart: " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert R["bound"]["validity"] <= mx.VALIDITY and max(r.values()) <= 1.0, r
    # ... and the reference itself says what the test is about: eBar_velocity = 0 and the extra velocity block, to second order
    assert np.abs(np.asarray(R["mean"][8:11], dtype=float)).max() < g2
    assert np.abs(np.asarray(R["spread"][8:11, 8:11], dtype=float) - np.outer(dv, dv)).max() < 1e-3 * g2
    fg.close()


# ---- 5. verdicts and errors
def test_a_singular_chart_is_a_verdict_and_the_destination_keeps_every_bit(hip):
    N = 5
    fg = _handle(hip, N, batch=4, order=[0, 1, None, 2])
    level = mc.member(N, 3)
    level["group"]["Aq"] = level["origin"]["q"] * np.array([1.0, -1.0, -1.0, -1.0])  # R_P0 R_A = I, eta = e3: the pole of the estimate's chart
    fg.restore_state(level, 2)
    before = [_getters(fg, b) for b in range(4)]
    got = fg.mixture_moments([0, 2], [1.0, 1.0], 0)
    assert got["info"] == -1 and np.isnan(got["mean"]).all() and np.isnan(got["P"]).all() and np.isnan(got["total_trace"])
    for dst in (3, 0):
        assert fg.merge([0, 1, 2], [1.0, 1.0, 1.0], 0, dst)["info"] == -1
    for b in range(4):
        _same(_getters(fg, b), before[b], f"filter {b} after a refused merge")
    # a fresh, uninitialised filter is level too: a verdict for the getter, an invalid argument for the merge
    fu = hip.FilterBatch(mc.cc.settings(), capacity=4, batch=2)
    assert fu.mixture_moments([0, 1], [1.0, 1.0], 0)["info"] == -1
    with pytest.raises(hip.EqfError) as ei:
        fu.merge([0, 1], [1.0, 1.0], 0, 0)
    assert ei.value.code == hip.ERR_INVALID
    assert fg.device_error() == 0 and fu.device_error() == 0
    fg.close(), fu.close()


def test_argument_errors_come_before_any_effect(hip):
    import ctypes as C

    N = 5
    fg = _handle(hip, N, batch=4, order=[0, 1, 2, 3])
    other = mc.member(N, 1)
    other["ids"] = other["ids"] + 1
    fg.restore_state(other, 3)            # other ids
    late = mc.member(N, 2)
    late["time"] = 2.0
    fg.restore_state(late, 2)             # another clock
    before = [_getters(fg, b) for b in range(4)]
    L, h = hip.lib(), fg._h
    n = 11 + 3 * N
    P, mean = np.zeros((n, n)), np.zeros(n)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)

    def moments(idx, w, ref, centred=1, ld=n, Pp=P, handle=h):
        i, ww = np.asarray(idx, dtype=np.int32), np.asarray(w, dtype=np.float64)
        return L.eqf_get_mixture_moments(handle, len(i), i.ctypes.data_as(ip) if idx is not None else None,
                                         ww.ctypes.data_as(dp) if w is not None else None, ref, centred, mean.ctypes.data_as(dp),
                                         Pp.ctypes.data_as(dp) if Pp is not None else None, ld, None)

    def merge(idx, w, ref, dst, handle=h):
        i, ww = np.asarray(idx, dtype=np.int32), np.asarray(w, dtype=np.float64)
        return L.eqf_merge_filters(handle, len(i), i.ctypes.data_as(ip), ww.ctypes.data_as(dp), ref, dst, None)

    inv = hip.ERR_INVALID
    assert moments([0, 1], [1.0, 1.0], 0) == 0
    assert moments([0, 1], [1.0, 1.0], 0, handle=None) == inv and merge([0, 1], [1.0, 1.0], 0, 0, handle=None) == inv
    assert moments([0, 1], [1.0, 1.0], 0, Pp=None) == inv
    assert L.eqf_get_mixture_moments(h, 2, None, mean.ctypes.data_as(dp), 0, 1, None, P.ctypes.data_as(dp), n, None) == inv
    assert L.eqf_get_mixture_moments(h, 0, mean.ctypes.data_as(ip), mean.ctypes.data_as(dp), 0, 1, None, P.ctypes.data_as(dp), n, None) == inv
    for idx, w, ref in (([0, 4], [1.0, 1.0], 0), ([0, -1], [1.0, 1.0], 0), ([0, 1], [1.0, 1.0], 4), ([0, 1], [1.0, 1.0], -1),
                        ([0, 1], [1.0, 1.0], 2),                       # ref not among idx
                        ([0, 1], [1.0, -0.5], 0), ([0, 1], [1.0, np.nan], 0), ([0, 1], [1.0, np.inf], 0), ([0, 1], [0.0, 0.0], 0),
                        ([0, 3], [1.0, 1.0], 0)):                      # other ids
        assert moments(idx, w, ref) == inv, (idx, w, ref)
        assert merge(idx, w, ref, 0) == inv, (idx, w, ref)
    assert moments([0, 1], [1.0, 1.0], 0, centred=2) == inv and moments([0, 1], [1.0, 1.0], 0, ld=n - 1) == inv
    assert merge([0, 1], [1.0, 1.0], 0, 4) == inv and merge([0, 1], [1.0, 1.0], 0, -1) == inv
    assert moments([0, 2], [1.0, 1.0], 0) == 0 and merge([0, 2], [1.0, 1.0], 0, 1) == inv   # another clock: the merge only
    for b in range(4):
        _same(_getters(fg, b), before[b], f"filter {b} after the refused calls")
    f32 = hip.FilterBatch(mc.cc.settings(), capacity=8, batch=2, precision=hip.PRECISION_F32)
    assert moments([0, 1], [1.0, 1.0], 0, handle=f32._h) == hip.ERR_UNSUPPORTED
    assert merge([0, 1], [1.0, 1.0], 0, 0, handle=f32._h) == hip.ERR_UNSUPPORTED
    assert fg.device_error() == 0
    fg.close(), f32.close()


# ---- 6. the route
def test_route_a_fixed_number_of_launches_and_nothing_of_the_vision_update(hip):
    N = 17
    fg = _handle(hip, N)
    fg.profile_enable(True)
    counts = []
    for n in (2, 17):
        idx, w, ref = _plan(n)
        assert fg.merge(idx, w, ref, idx[0])["info"] == 0
        counts.append(fg.debug_mixture_launches())
    assert counts[0] == counts[1] == 11, counts
    prof = fg.profile()
    for k in ("k_update_prep", "k_chol_step", "k_update_reduce", "k_update_finish", "k_downdate", "k_chol_step_dd", "k_chol_resident",
              "k_propagate", "k_imu_burst", "k_dense_riccati"):
        assert prof[k][0] == 0, (k, prof[k])
    fg.profile_enable(False)
    assert fg.device_error() == 0
    fg.close()
