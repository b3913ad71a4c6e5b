"""Draws from a handle's covariance and the group step that moves a filter by one (csrc/eqf_sample.hpp: eqf_sample_sigma,
eqf_apply_increment, eqf_perturb_filters; FilterBatch.sample_sigma / apply_increment / perturb).

The draw eps = s L z is compared with numpy's Cholesky of the matrix the device factored, taken from the device's OWN getter (sigma(b) /
sigma_local(b)), symmetrised from its lower triangle and cut at `first` (tests/test_gpu_nees.py's reference):
    |eps - s L z|_2 <= n u kappa_2(A) |L|_2 |z|_2,   u = 2^-53,
the first-order bound of two backward-stable factorisations of A that differ by n u |A| (constant 1).  So that it cannot hide a real error
the relative bound n u kappa_2 is asserted <= 1e-5, and the same z through chol(1.001 A) must move the reference by more than 100 bounds.
The covariance identity |E E^T - A|_F <= (2 n + 1) u trace(A) is free of conditioning: (n + 1) u |L|_F^2 for the factorisation, n u |L|_F^2
for numpy's product, |L|_F^2 = trace(A).
The group step is compared with the numpy oracle's VIOExp(liftInnovation(.)) * X; its tolerance is ten times the oracle's own error against
the 50-digit definitions of tests/lie_exact.py on the same input, both in units of u (1 + magnitude) and the oracle's error taken as at least
one such unit (a result that is rounded to double at all is off by up to half of one; the factor ten is for the other evaluation order).
Everything else is bit for bit: the bytes of every getter."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import lie_exact as lx
from consistency_helpers import inject, numpy_filter, origin_group_of

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIRSTS = (0, 6, 11)
NSAMP = (1, 16, 17, 64)


@pytest.fixture(scope="module")
def hip():
    from eqf_vio_amd import binding

    return binding


def _settings(**kw):
    from eqf_vio_amd import synth

    d = synth.template_settings_dict()
    d.update(kw)
    return d


def _events(st, f0, f1):
    out, f = [], 0
    for kind, k in st.events():
        if f >= f1:
            break
        if f >= f0:
            out.append((kind, k))
        if kind == "vision":
            f += 1
    return out


def _run(fg, st, f0, f1, meas=None, nb=None, stream=False):
    for kind, k in _events(st, f0, f1):
        if stream:
            fg.stream_imu(k) if kind == "imu" else fg.stream_vision(k)
        elif kind == "imu":
            r = st.imu[k]
            fg.process_imu(r[0], r[1:4], r[4:7])
        elif meas is not None:
            fg.process_vision(st.vision_stamps[k], *meas[k])
        else:
            fg.process_vision(st.vision_stamps[k], st.ids, st.bearings[k], nb=nb)


def _handle(hip, N, batch=1, nb=None, capacity=None, **kw):
    """Three vision frames of the 0.4 s stream."""
    from eqf_vio_amd import synth

    st = synth.make_stream(max(N, 1), duration=0.4)
    fg = hip.FilterBatch(_settings(**kw), capacity=(capacity or N + 7), batch=batch)
    fg.set_option("innovation_stats", 1)
    _run(fg, st, 0, 3, nb=nb)
    return st, fg


@pytest.fixture(scope="module")
def handles(hip):
    """One handle per landmark count, shared and never moved (the tests that move a filter build their own)."""
    out = {}
    for N in (5, 17, 18, 43):
        out[N] = _handle(hip, N)[1]
        assert out[N].num_landmarks(0) == N
    return out


def _cut(S, first):
    A = np.tril(S[first:, first:])
    return A + np.tril(A, -1).T


def _matrix(fg, b, local, first):
    return _cut(fg.sigma_local(b) if local else fg.sigma(b), first)


def _draw_ratio(A, z, eps, s, first, what):
    """Rows of eps (k, n_ref) against s L z for the cut matrix A; returns the largest |diff| / bound."""
    n = A.shape[0]
    assert np.all(eps[:, :first] == 0.0), what
    if n == 0:
        return 0.0
    L = np.linalg.cholesky(A)
    kappa = float(np.linalg.cond(A))
    assert n * U * kappa <= 1e-5, (what, n * U * kappa)
    L2 = np.linalg.cholesky(1.001 * A)
    nL = float(np.linalg.norm(L, 2))
    worst = 0.0
    for k in range(z.shape[0]):
        zz = z[k, first:first + n]
        want = s * (L @ zz)
        bound = n * U * kappa * nL * float(np.linalg.norm(zz)) * abs(s)
        assert np.linalg.norm(s * (L2 @ zz) - want) > 100 * bound, (what, k)
        worst = max(worst, float(np.linalg.norm(eps[k, first:first + n] - want)) / bound)
    assert worst <= 1.0, (what, worst)
    return worst


def _bits(x):
    if isinstance(x, dict):
        return {k: _bits(v) for k, v in x.items()}
    return np.ascontiguousarray(x).tobytes() + str(np.asarray(x).shape).encode()


def _assert_same(a, b, what):
    a, b = _bits(a), _bits(b)
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k], f"{what}: {k} differs"


def _getters(fg, b):
    g = dict(n=fg.num_landmarks(b), est=fg.state_estimate(b), innov=fg.innovation_stats(b))
    g.update(fg.dump_state(b))  # ids, origin, group, bias, sigma, time, integrator
    return g


# ---- 1. the draw against numpy
@pytest.mark.parametrize("N", [5, 17, 18, 43])
def test_draw_against_numpy_cholesky_of_the_devices_own_matrix(hip, handles, N):
    """Reference orders 26 / 62 / 65 / 140: internal orders 63 and 66 on either side of a block boundary, three block columns with a ragged
    last one; nsamp 1 / 16 / 17 / 64: one row, a full tile, a tile and one row, four tiles."""
    fg = handles[N]
    n = 11 + 3 * N
    rng = np.random.default_rng(N)
    worst = 0.0
    for local in (False, True):
        for first in FIRSTS:
            A = _matrix(fg, 0, local, first)
            for nsamp in NSAMP:
                z = rng.standard_normal((1, nsamp, n))
                got = fg.sample_sigma(z, local=local, first=first)
                assert got["info"][0] == 0 and got["dof"][0] == n - first and got["eps"].shape == (1, nsamp, n)
                worst = max(worst, _draw_ratio(A, z[0], got["eps"][0], 1.0, first, (N, local, first, nsamp)))
            s = fg.sample_sigma(z[:, :3], local=local, first=first, scale=0.5)
            worst = max(worst, _draw_ratio(A, z[0, :3], s["eps"][0], 0.5, first, (N, local, first, "scale 0.5")))
            assert np.array_equal(s["eps"][0], 0.5 * got["eps"][0, :3])  # (a power of two: the very same bits, halved)
    print(f"N={N}: largest |eps - s L z| / bound {worst:.3e}")
    assert fg.device_error() == 0


def test_draw_of_a_filter_without_landmarks(hip):
    from eqf_vio_amd import synth

    st = synth.make_stream(4, duration=0.4)
    fg = hip.FilterBatch(_settings(), capacity=7, batch=1)
    for r in st.imu[:60]:
        fg.process_imu(r[0], r[1:4], r[4:7])
    assert fg.num_landmarks(0) == 0
    z = np.random.default_rng(1).standard_normal((1, 17, 11))
    worst = 0.0
    for local in (False, True):
        for first in FIRSTS:
            got = fg.sample_sigma(z, local=local, first=first)
            assert got["info"][0] == 0 and got["dof"][0] == 11 - first
            worst = max(worst, _draw_ratio(_matrix(fg, 0, local, first), z[0], got["eps"][0], 1.0, first, ("no landmarks", local, first)))
    print(f"no landmarks: largest ratio {worst:.3e}")
    before = fg.dump_state(0)
    assert fg.perturb(z[:, :1], first=11, stats=True)["dof"][0] == 0  # (an empty submatrix: nothing to draw, nothing moves)
    _assert_same(fg.dump_state(0), before, "perturbation by an empty draw")
    assert fg.device_error() == 0


def test_draw_in_a_batch_of_four_with_different_landmark_counts(hip):
    counts = [0, 5, 18, 43]
    _, fg = _handle(hip, 43, batch=4, nb=counts)
    assert [fg.num_landmarks(b) for b in range(4)] == counts
    rng = np.random.default_rng(4)
    z = rng.standard_normal((4, 17, 11 + 3 * 43))
    scale = np.array([1.0, 0.5, 2.0, 0.25])
    worst = 0.0
    for local in (False, True):
        for first in FIRSTS:
            got = fg.sample_sigma(z, local=local, first=first, scale=scale)
            for b, N in enumerate(counts):
                n = 11 + 3 * N
                assert got["info"][b] == 0 and got["dof"][b] == n - first
                assert np.all(got["eps"][b, :, n:] == 0.0)  # (beyond a filter's own order the output is left alone)
                worst = max(worst, _draw_ratio(_matrix(fg, b, local, first), z[b, :, :n], got["eps"][b, :, :n], scale[b], first, (b, local, first)))
    print(f"batch 0/5/18/43: largest ratio {worst:.3e}")
    assert fg.device_error() == 0


# ---- 2. the covariance identity
@pytest.mark.parametrize("N", [5, 17, 18, 43])
def test_covariance_identity(hip, handles, N):
    """Z = identity columns, 64 at a time: the rows of eps are the columns of L."""
    fg = handles[N]
    n = 11 + 3 * N
    worst = 0.0
    for local in (False, True):
        for first in FIRSTS:
            A = _matrix(fg, 0, local, first)
            m = n - first
            Lt = np.zeros((m, n))
            for k0 in range(0, m, 64):
                k1 = min(k0 + 64, m)
                z = np.zeros((1, k1 - k0, n))
                z[0, np.arange(k1 - k0), first + np.arange(k0, k1)] = 1.0
                got = fg.sample_sigma(z, local=local, first=first)
                assert got["info"][0] == 0
                Lt[k0:k1] = got["eps"][0]
            E = Lt[:, first:].T
            assert np.all(np.triu(E, 1) == 0.0), (N, local, first)  # (L is lower triangular: exact zeros above the diagonal)
            bound = (2 * m + 1) * U * float(np.trace(A))
            r = float(np.linalg.norm(E @ E.T - A)) / bound
            L2 = np.linalg.cholesky(1.001 * A)
            assert np.linalg.norm(L2 @ L2.T - A) > 100 * bound
            print(f"N={N} local={int(local)} first={first}: |E E^T - A|_F / ((2n+1) u tr A) = {r:.3e}")
            worst = max(worst, r)
            assert r <= 1.0, (N, local, first, r)
    print(f"N={N}: largest ratio {worst:.3e}")


# ---- 3. round trip with the NEES
@pytest.mark.parametrize("N", [5, 18, 43])
def test_round_trip_with_the_nees(hip, handles, N):
    fg = handles[N]
    n = 11 + 3 * N
    z = np.random.default_rng(30 + N).standard_normal((1, 16, n))
    worst = 0.0
    for local in (False, True):
        for first in FIRSTS:
            eps = fg.sample_sigma(z, local=local, first=first)["eps"]
            got = fg.nees(eps, local=local, first=first)
            want = np.sum(z[0, :, first:] ** 2, axis=1)
            tol = (n - first) * U * float(np.linalg.cond(_matrix(fg, 0, local, first)))
            r = float(np.max(np.abs(got["nees"][0] - want) / (tol * want)))
            worst = max(worst, r)
            assert got["info"][0] == 0 and r <= 1.0, (N, local, first, r)
    print(f"N={N}: largest |nees - z^T z| / (n u kappa z^T z) {worst:.3e}")


# ---- 4. the increment against the oracle
def _exact_group(snap, gamma, d):
    xi0 = lx.State.from_dict(snap["origin"], d["cameraOffset_q"], d["cameraOffset_x"])
    return lx.apply_innovation(lx.Group.from_dict(snap["group"]), xi0, None, gamma[8:11], gamma[11:], "nolift", gg=gamma[6:8])


@pytest.mark.parametrize("N", [0, 5, 43])
def test_increment_against_the_oracle(hip, N):
    from oracle import eqf_numpy as O

    d = _settings()
    if N:
        _, fg = _handle(hip, N)
    else:
        fg = _handle(hip, 4, nb=[0])[1]
    assert fg.num_landmarks(0) == N
    before = _getters(fg, 0)
    last = fg.last_update(0)
    report = fg.gate_report(0)
    n = 11 + 3 * N
    gamma = np.random.default_rng(40 + N).standard_normal(n) * np.sqrt(np.diag(before["sigma"]))
    fg.apply_increment(gamma[None, :])
    after = _getters(fg, 0)
    # what must keep its bits
    for key in ("sigma", "origin", "time", "ids", "currentVelocity", "accumulatedVelocity", "accumulatedTime", "initialised", "innov", "n"):
        _assert_same({key: after[key]}, {key: before[key]}, "apply_increment")
    _assert_same(fg.last_update(0), last, "apply_increment: last_update")
    _assert_same(fg.gate_report(0), report, "apply_increment: gate report")
    # the oracle
    fo = inject(numpy_filter(d), before)
    X = O.vio_exp(O.lift_innovation(gamma[6:], fo.xi0)) * fo.X
    fo.X = X
    want = origin_group_of(fo)[1]
    assert np.array_equal(after["bias"], before["bias"] + gamma[0:6])
    exact = _exact_group(before, gamma, d)
    r_oracle = lx.group_ratios(want, exact)
    r_device = lx.group_ratios(after["group"], exact)
    print(f"N={N}: oracle against the 50-digit definitions {r_oracle}")
    print(f"N={N}: device against the 50-digit definitions {r_device}")
    tol = 10.0 * max(1.0, max(r_oracle.values()))
    assert max(r_device.values()) <= tol, (r_device, r_oracle)
    moved = max(np.abs(after["group"]["Aq"] - before["group"]["Aq"]).max(), np.abs(after["group"]["w"] - before["group"]["w"]).max())
    assert moved > 1e6 * U  # (the comparison is about a step that is there)
    assert fg.device_error() == 0


def test_increment_on_an_f32_handle(hip):
    """The state is fp64 in both precisions: the same snapshot moves to the same bits."""
    N = 17
    _, f64 = _handle(hip, N)
    snap = f64.dump_state(0)
    f32 = hip.FilterBatch(_settings(), capacity=N + 7, batch=1, precision=hip.PRECISION_F32)
    f32.restore_state(snap, 0)
    gamma = np.random.default_rng(2).standard_normal((1, 11 + 3 * N)) * 0.01
    f64.apply_increment(gamma)
    f32.apply_increment(gamma)
    a, b = f64.dump_state(0), f32.dump_state(0)
    _assert_same({k: a[k] for k in ("group", "bias", "origin")}, {k: b[k] for k in ("group", "bias", "origin")}, "fp32 handle")
    assert not np.array_equal(a["group"]["Aq"], snap["group"]["Aq"])


# ---- 5. the twin
@pytest.mark.parametrize("mode", ["per call", "per call, churn and gate", "stream mode, gate"])
def test_twin_restored_from_a_perturbed_filter_runs_bit_for_bit(hip, mode):
    """A stale cache on the host or the device would show as a difference between the perturbed handle and a fresh handle restored from its
    dump: ten IMU calls and a vision frame, twice, every getter after each frame."""
    from eqf_vio_amd import synth

    N = 30
    st = synth.make_stream(N, duration=0.4)
    stream, churn = mode.startswith("stream"), "churn" in mode
    meas = synth.churn_measurements(st, seed=7, outlier_frames=(3, 4), outlier_angle=0.2) if churn else None
    cap = N if churn else N + 5
    fa, fb = hip.FilterBatch(_settings(), capacity=cap, batch=2), hip.FilterBatch(_settings(), capacity=cap, batch=2)
    for h in (fa, fb):
        h.set_option("innovation_stats", 1)
        if "gate" in mode:
            h.set_outlier_gate(hip.GATE_MAHALANOBIS, 9.21)
        if stream:
            h.stream_upload(st.imu, st.vision_stamps, st.ids, st.bearings)
    _run(fa, st, 0, 3, meas=meas, stream=stream)
    # (IMU calls of the next frame are queued when the perturbation arrives: it has to settle them first)
    nxt = _events(st, 3, 4)
    for kind, k in nxt[:4]:
        fa.stream_imu(k) if stream else fa.process_imu(st.imu[k][0], st.imu[k][1:4], st.imu[k][4:7])
    z = np.random.default_rng(5).standard_normal((2, 1, 11 + 3 * max(fa.num_landmarks(0), fa.num_landmarks(1))))
    # (a small move: landmarks that came in a frame ago still carry initialPointVariance, and a filter thrown tens of metres is no test of a cache)
    stats = fa.perturb(z, first=0, scale=[0.05, 0.02], stats=True)
    assert np.all(stats["info"] == 0)
    for b in range(2):
        fb.restore_state(fa.dump_state(b), b)
        _assert_same(fb.dump_state(b), fa.dump_state(b), f"{mode}: restored slot {b}")

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

    for f, ev in ((3, nxt[4:]), (4, _events(st, 4, 5))):
        assert sum(kind == "imu" for kind, _ in _events(st, f, f + 1)) == 10
        rest(fa, ev), rest(fb, ev)
        for b in range(2):
            _assert_same(_getters(fa, b), _getters(fb, b), f"{mode}: slot {b} after frame {f}")
            assert fa.innovation_stats(b)["valid"]
    assert fa.device_error() == 0 and fb.device_error() == 0


# ---- 6. the fused call
def test_fused_call_equals_the_two_calls(hip):
    counts = [5, 18, 43, 18]
    st, fa = _handle(hip, 43, batch=4, nb=counts)
    _, fb = _handle(hip, 43, batch=4, nb=counts)
    rng = np.random.default_rng(6)
    z = rng.standard_normal((4, 1, 11 + 3 * 43))
    # (small moves, so that the filters can run on afterwards: after three frames a landmark still has a standard deviation of metres)
    for first, scale in ((0, [0.01, 0.02, 0.005, 0.01]), (6, [0.005, 0.0, 0.015, 0.0025]), (11, [0.0, 0.01, 0.0, 0.02])):
        before = [fa.dump_state(b) for b in range(4)]
        for b in range(4):
            _assert_same(fb.dump_state(b), before[b], "the two handles start equal")
        assert fa.perturb(z, first=first, scale=scale) is None
        got = fb.sample_sigma(z, local=False, first=first, scale=scale)
        assert np.all(got["info"] == 0)
        mask = None if all(scale) else np.asarray(scale) != 0.0
        fb.apply_increment(got["eps"][:, 0, :], mask=mask)
        for b in range(4):
            _assert_same(fa.dump_state(b), fb.dump_state(b), f"first={first} slot {b}")
            still = scale[b] == 0.0
            assert (_bits(fa.dump_state(b)) == _bits(before[b])) == still, (first, b)
    # a resampled batch no longer collapses onto its parent
    fa.resample([0, 0, 0, 0])
    for b in range(1, 4):
        _assert_same(fa.dump_state(b), fa.dump_state(0), "resample")
    fa.perturb(np.random.default_rng(7), first=0, scale=[0.0, 0.01, 0.01, 0.01])
    groups = [fa.group(b)["Aq"].tobytes() + fa.bias(b).tobytes() for b in range(4)]
    assert len(set(groups)) == 4
    for b in range(1, 4):
        assert np.array_equal(fa.sigma(b), fa.sigma(0))
    # ... and runs on
    _run(fa, st, 3, 4, nb=[5, 5, 5, 5])
    assert fa.device_error() == 0 and fb.device_error() == 0


# ---- 7. reproducibility
def test_bit_for_bit_from_run_to_run_and_wherever_the_filter_sits(hip, handles):
    fg = handles[43]
    snap = fg.dump_state(0)
    n = 11 + 3 * 43
    one, three = hip.FilterBatch(_settings(), capacity=51, batch=1), hip.FilterBatch(_settings(), capacity=45, batch=3)
    one.restore_state(snap, 0)
    three.restore_state(snap, 2)
    z = np.random.default_rng(8).standard_normal((1, 17, n))
    z3 = np.zeros((3, 17, n))
    z3[2] = z[0]
    for local in (False, True):
        for first in FIRSTS:
            a = fg.sample_sigma(z, local=local, first=first)
            b = fg.sample_sigma(z, local=local, first=first)
            c = one.sample_sigma(z, local=local, first=first)
            d = three.sample_sigma(z3, local=local, first=first)
            assert a["info"][0] == 0
            for key in ("eps", "logdet", "min_pivot", "dof", "info"):
                assert _bits(a[key][0]) == _bits(b[key][0]) == _bits(c[key][0]) == _bits(d[key][2]), (local, first, key)
    one.perturb(z[:, :1], first=0, scale=0.5)
    three.perturb(z3[:, :1], first=0, scale=0.5)
    _assert_same(one.dump_state(0), three.dump_state(2), "perturb: alone and at index 2 of 3")
    assert _bits(one.dump_state(0)) != _bits(snap)


# ---- 8. errors
def test_argument_errors_leave_outputs_and_state_untouched(hip):
    N = 6
    n = 11 + 3 * N
    _, fg = _handle(hip, N, batch=2, capacity=N)
    from eqf_vio_amd import synth

    st = synth.make_stream(N, duration=0.4)
    f32 = hip.FilterBatch(_settings(), capacity=N, batch=2, precision=hip.PRECISION_F32)
    _run(f32, st, 0, 3)
    L = hip.lib()
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_ubyte)
    Z = np.ones((2, 65, n))
    eps = np.full((2, 65, n), -7.0)
    stats = (hip.SigmaStats * 2)()
    for s in stats:
        s.logdet, s.min_pivot, s.dof, s.info = -7.0, -7.0, -7, -7
    P = lambda a: a.ctypes.data_as(dp) if a is not None else None  # noqa: E731

    def draw(h, local=1, first=0, nsamp=1, z=Z, ldz=n, scale=None, e=eps, lde=n, st_=stats):
        return L.eqf_sample_sigma(h, local, first, nsamp, P(z), ldz, P(scale), P(e), lde, st_)

    before = [_getters(fg, b) for b in range(2)]
    before32 = [f32.dump_state(b) for b in range(2)]
    for kw in (dict(local=2), dict(local=-1), dict(first=5), dict(first=12), dict(nsamp=65), dict(nsamp=-1), dict(ldz=n - 1), dict(lde=n - 1),
               dict(z=None), dict(e=None), dict(nsamp=0, st_=None)):
        assert draw(fg._h, **kw) == hip.ERR_INVALID, kw
    assert draw(None) == hip.ERR_INVALID
    assert draw(f32._h) == hip.ERR_UNSUPPORTED
    G = np.full((2, n), 1e-3)
    bad = G.copy()
    bad[1, n - 1] = np.nan
    inf = G.copy()
    inf[0, 3] = np.inf
    m = np.array([1, 0], dtype=np.uint8)
    assert L.eqf_apply_increment(fg._h, None, n, None) == hip.ERR_INVALID
    assert L.eqf_apply_increment(None, P(G), n, None) == hip.ERR_INVALID
    assert L.eqf_apply_increment(fg._h, P(G), n - 1, None) == hip.ERR_INVALID
    assert L.eqf_apply_increment(fg._h, P(bad), n, None) == hip.ERR_INVALID
    assert L.eqf_apply_increment(fg._h, P(inf), n, m.ctypes.data_as(up)) == hip.ERR_INVALID
    assert L.eqf_perturb_filters(fg._h, 5, P(Z), n, None, None) == hip.ERR_INVALID
    assert L.eqf_perturb_filters(fg._h, 0, None, n, None, None) == hip.ERR_INVALID
    assert L.eqf_perturb_filters(fg._h, 0, P(Z), n - 1, None, None) == hip.ERR_INVALID
    assert L.eqf_perturb_filters(fg._h, 0, P(Z), n, P(np.array([1.0, np.nan])), None) == hip.ERR_INVALID
    assert L.eqf_perturb_filters(None, 0, P(Z), n, None, None) == hip.ERR_INVALID
    assert L.eqf_perturb_filters(f32._h, 0, P(Z), n, None, None) == hip.ERR_UNSUPPORTED
    assert np.all(eps == -7.0)
    assert all(s.logdet == -7.0 and s.min_pivot == -7.0 and s.dof == -7 and s.info == -7 for s in stats)
    for b in range(2):
        _assert_same(_getters(fg, b), before[b], f"after the refused calls, slot {b}")
        _assert_same(f32.dump_state(b), before32[b], f"after the refused calls, fp32 slot {b}")
    assert fg.device_error() == 0 and f32.device_error() == 0
    # the same calls with good arguments work; a NaN in a masked-out filter's increment is nobody's business
    assert draw(fg._h, nsamp=2) == 0 and stats[0].info == 0 and stats[1].dof == n and eps[0, 1, 0] != -7.0 and eps[0, 4, 0] == -7.0
    assert draw(fg._h, nsamp=0) == 0 and stats[0].dof == n
    assert L.eqf_apply_increment(fg._h, P(bad), n, m.ctypes.data_as(up)) == 0
    _assert_same(fg.dump_state(1), {k: before[1][k] for k in fg.dump_state(1)}, "masked-out slot")
    assert not np.array_equal(fg.bias(0), before[0]["bias"])
    assert fg.device_error() == 0


def test_a_failed_factorisation_is_reported_per_filter_and_moves_nothing(hip):
    N = 18
    n = 11 + 3 * N
    _, fg = _handle(hip, N, batch=3)
    rng = np.random.default_rng(9)
    d = 1.0 + rng.random(n)
    d[40] = -1.0
    fg.set_sigma(np.diag(d), 1)
    z = rng.standard_normal((3, 3, n))
    before = [fg.dump_state(b) for b in range(3)]
    got = fg.sample_sigma(z, local=False, first=0)
    assert list(got["info"]) == [0, 1, 0] and np.all(np.isnan(got["eps"][1])) and np.isnan(got["logdet"][1])
    for b in (0, 2):
        r = _draw_ratio(_matrix(fg, b, False, 0), z[b], got["eps"][b], 1.0, 0, ("neighbour", b))
        print(f"neighbour {b} of the indefinite filter: ratio {r:.3e}")
    stats = fg.perturb(z[:, :1], first=0, stats=True)
    assert list(stats["info"]) == [0, 1, 0]
    _assert_same(fg.dump_state(1), before[1], "the filter whose factorisation failed")
    ref = hip.FilterBatch(_settings(), capacity=N + 7, batch=3)
    for b in (0, 2):
        ref.restore_state(before[b], b)
    ref.apply_increment(got["eps"][:, 0, :], mask=[1, 0, 1])
    for b in (0, 2):
        _assert_same(fg.dump_state(b), ref.dump_state(b), f"neighbour {b}")
        assert _bits(fg.dump_state(b)) != _bits(before[b])
    assert fg.device_error() == 0


# ---- 9. the C++ facade
def test_cpp_facade_against_the_python_binding_bit_for_bit(hip):
    """VIOFilter::sampleStateError / perturbState of cpp/VIOFilter.h through the example binary (argument `sample`, hexadecimal floats)
    against filter.VIOFilter on the same sequence."""
    from eqf_vio_amd import filter as vf

    N, frames = 20, 6
    exe = os.path.join(ROOT, "eqf_vio_amd", "cpp", "eqf_example")
    out = subprocess.run([exe, str(N), str(frames), "sample"], capture_output=True, text=True, check=True).stdout.splitlines()
    lines = [ln.split()[1:] for ln in out if ln.startswith("sample ")]
    moved = [ln.split()[1:] for ln in out if ln.startswith("perturbed ")]
    assert len(lines) == 6 and len(moved) == 1
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
    z = np.array([math.sin(1.7 * i + 0.2) for i in range(11 + 3 * N)])
    for ln in lines:
        local, first, dof, info = (int(x) for x in ln[0:4])
        s = fg.sampleStateError(z, local=bool(local), first=first, scale=0.5)
        assert (dof, info) == (s["dof"], s["info"]) == (11 + 3 * N - first, 0)
        got = np.array([float.fromhex(x) for x in ln[4:]])
        assert got.tobytes() == s["eps"].tobytes(), (local, first)
        assert np.all(got[:first] == 0.0) and np.all(got[first:] != 0.0)
    assert fg.perturbState(z, first=6, scale=0.25)["info"] == 0
    e, S = fg.stateEstimate(), fg.stateCovariance()
    want = np.concatenate([e.pose_q, e.pose_x, e.velocity, S.reshape(-1)])
    assert int(moved[0][0]) == N
    assert np.array([float.fromhex(x) for x in moved[0][1:]]).tobytes() == want.tobytes()
