"""Every device implementation of the covariance step  Sigma' = F Sigma F^T + T (P + Bt R Bt^T)  entry by entry against the longdouble
reference of tests/riccati_exact.py, within its a-priori bound: ratio <= 1 at EVERY entry, Sigma' symmetric to the bound, the burst kernels'
off-diagonal landmark blocks exact transposes of each other, and no device error.  Public API only: restore_state, the IMU calls, sigma().

Routes: the fused single step (k_propagate), the split pair (k_build_blocks + k_riccati_stream; there also debug_blocks() against the 50-digit
blocks within tau_blk units), the burst kernels (1 / 2 / 4 rows per wavefront, two launches or the fused launch, the 4- / 8- / 16-landmark
builders reached through the shape heuristics of eqf_capi.hip and proven by launch_shape()), the dense MFMA backend, the float instantiations,
and the partitioned filter's k_tl_* kernels on a 1 x 1 grid.  States, Sigma families, sizes and calls: tests/riccati_cases.py; the same cases
hold two fp64 numpy restatements inside the bound on the CPU (tests/test_riccati_exact.py), where tau_blk is measured from the fp64 oracle.
No constant here comes from the device: k = 32 is counted from the structure, tau_blk = 10 x the oracle's 6.61 units.

Worst ratio to the bound per route on an MI355X (each test prints its own): NOTES.md R14.1 -- fp64 routes 0.02 .. 0.10, fp32 0.14 .. 0.35, the
device's own blocks (debug_blocks) 6.4 units against the oracle's 6.6."""
import numpy as np
import pytest

import riccati_cases as rc
import riccati_exact as rx

pytestmark = pytest.mark.gpu

ENV_KEYS = ("EQF_BURST_FUSED", "EQF_BURST_ROWS", "EQF_IMU_BURST", "EQF_SPLIT_PROPAGATE")
_SNAP, _STEPS, _REF = {}, {}, {}


@pytest.fixture(scope="module")
def hip():
    from eqf_vio_amd import binding

    return binding


def snapshot(hip, N):
    if N not in _SNAP:
        _SNAP[N] = rc.device_snapshot(hip, N)
    return _SNAP[N]


def reference(hip, N, fam, four=False, fp32=False):
    """(Sigma the step starts from, the calls, Sigma_ref, bound, Steps): computed once per case for the whole module."""
    key = (N, fam, four, fp32)
    if key not in _REF:
        snap = snapshot(hip, N)
        calls = rc.four_calls(snap) if four else rc.one_call(snap, fam)
        sk = (N, "four" if four else ("gap" if fam == "d" else "one"))
        if sk not in _STEPS:
            _STEPS[sk] = rx.exact_steps(snap, rc.settings(), calls)
        S0 = rc.sigma_family(snap, fam)
        assert np.array_equal(S0, S0.T)
        _REF[key] = (S0, calls) + rx.reference_run(_STEPS[sk], S0, fp32) + (_STEPS[sk],)
    return _REF[key]


def make_handle(hip, monkeypatch, env, capacity, batch=1, dense=False, precision=None, burst=False):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    f = hip.FilterBatch(rc.settings(), capacity=capacity, batch=batch, **({} if precision is None else {"precision": precision}))
    for k in env:
        monkeypatch.delenv(k)
    if dense:
        f.set_dense_propagate(True)
    if burst:
        f.set_imu_burst(15)
    return f


def step(fg, snaps, S0s, calls):
    """restore every filter of the handle (identical bits for every route), run the calls, return the covariances"""
    for b, (snap, S0) in enumerate(zip(snaps, S0s)):
        fg.restore_state(dict(snap, sigma=S0), b)
    for c in zip(*calls):  # (call k of every filter)
        fg.process_imu([x[0] for x in c], np.array([x[1] for x in c]), np.array([x[2] for x in c]))
    return [fg.sigma(b) for b in range(len(snaps))]


def check(S, Sref, E, what, worst, bad, transposes=False):
    r, ij = rx.worst_ratio(S, Sref, E)
    s = rx.symmetry_ratio(S, E)
    assert np.all(np.isfinite(S)), what
    worst[what[-1]] = max(worst.get(what[-1], (0.0,)), (r, ij, what[:-1]))
    if not (r <= 1.0 and s <= 1.0):
        bad.append((what, "ratio", r, ij, "symmetry", s))
    if transposes:
        LL = S[11:, 11:]
        N = LL.shape[0] // 3
        off = np.kron(1 - np.eye(N), np.ones((3, 3))).astype(bool)
        if not np.array_equal(LL[off], LL.T[off]):
            bad.append((what, "off-diagonal landmark blocks are not exact transposes"))


def report(route, worst):
    print(f"{route}: worst ratio to the bound per Sigma family  " + "   ".join(f"{k}: {v[0]:.3f} at {v[1]} {v[2]}" for k, v in sorted(worst.items())))


SINGLE = {"fused": {"EQF_IMU_BURST": "0", "EQF_SPLIT_PROPAGATE": "0"}, "split": {"EQF_IMU_BURST": "0", "EQF_SPLIT_PROPAGATE": "1"}, "dense": {}}
BURST = {f"burst-rows{r}-fused{f}": {"EQF_BURST_ROWS": str(r), "EQF_BURST_FUSED": str(f)} for r in (1, 2, 4) for f in (0, 1)}


def run_route(hip, monkeypatch, route, env, N, fams, worst, bad, four=False, precision=None):
    """One handle of capacity N + 5 (the tiles carry inactive landmarks), one filter, every family of one size.  Returns launch_shape() of a
    burst route.  The library records the shape of an IMU-only burst only for the FIRST burst of a handle (launchBurst: lastBurstShape[6] == 0),
    so it is read and asserted right behind the first family's burst; the later bursts of the handle have the same batch, N and environment,
    which is all the shape heuristic looks at."""
    burst = route.startswith("burst")
    fg = make_handle(hip, monkeypatch, env, N + 5, dense=route == "dense", precision=precision, burst=burst)
    shape = None
    try:
        snap = snapshot(hip, N)
        for fam in fams:
            S0, calls, Sref, E, steps = reference(hip, N, fam, four, precision is not None)
            (S,) = step(fg, [snap], [S0], [calls])
            check(S, Sref, E, (route, N, fam), worst, bad, transposes=burst)
            if burst and shape is None:
                shape = fg.launch_shape()
                rows, fused = int(env.get("EQF_BURST_ROWS", 0)), env.get("EQF_BURST_FUSED")
                if rows:
                    assert shape["rows_per_wave"] == rows, (route, N, shape)
                if fused is not None:  # (the fused launch exists for the 4-landmark builder with one row per wavefront, fp64)
                    assert shape["fused"] == (fused == "1" and shape["rows_per_wave"] == 1 and shape["builder_landmarks"] == 4 and precision is None), (route, N, shape)
                assert shape["steps"] == len(calls), (route, N, shape)
            if route == "split" and not four and precision is None:  # (the fp32 handle does not keep the blocks in a readable form)
                units = rx.block_units(steps[0], rx.scaled_from_debug_blocks(fg.debug_blocks()))
                worst["blocks"] = max(worst.get("blocks", (0.0,)), (max(units.values()), max(units, key=units.get), (route, N)))
                if not max(units.values()) <= rx.TAU_BLK:
                    bad.append((route, N, fam, "debug_blocks", units))
        assert fg.device_error() == 0, (route, N)
    finally:
        fg.close()
    return shape


@pytest.mark.parametrize("route", list(SINGLE) + list(BURST))
def test_one_step_on_every_single_gpu_route(hip, monkeypatch, route):
    """N = 1, 15, 16, 17, 33, 49, 70, all four Sigma families, one IMU call, one filter in a handle of capacity N + 5."""
    env = SINGLE.get(route, BURST.get(route))
    worst, bad, shapes = {}, [], set()
    for N in rc.SIZES:
        shape = run_route(hip, monkeypatch, route, env, N, rc.FAMILIES, worst, bad)
        if shape:
            shapes.add((shape["builder_landmarks"], shape["rows_per_wave"], shape["fused"]))
    report(route, worst)
    if shapes:
        print(f"{route}: launch shapes (builder landmarks, rows per wavefront, fused) {sorted(shapes)}")
        assert {s[0] for s in shapes} == {4}  # (one small filter: the 4-landmark builder)
    assert not bad, bad[:10]


def test_four_rows_per_wavefront_at_130(hip, monkeypatch):
    """N = 130: three 64-column ring tiles and 33 four-row groups, the last one ragged."""
    worst, bad = {}, []
    shape = run_route(hip, monkeypatch, "burst-rows4", {"EQF_BURST_ROWS": "4"}, rc.BIG, rc.FAMILIES, worst, bad)
    report("burst, four rows per wavefront, N = 130", worst)
    assert shape["rows_per_wave"] == 4 and not shape["fused"], shape
    assert not bad, bad[:10]


def builder_batch(cus, N, lm):
    """The smallest batch that the heuristic of launchBurst sends to the `lm`-landmark builder: 4 while ceil(N / 4) B <= CUs (or the fused launch
    fits: ceil(N / 4) + ring tiles <= 1.25 CUs / B), 8 while ceil(N / 8) B <= CUs, 16 beyond."""
    per = -(-N // (4 if lm == 8 else 8))
    return cus // per + 1


@pytest.mark.parametrize("lm", [8, 16])
def test_eight_and_sixteen_landmark_builders(hip, monkeypatch, lm):
    """N = 17 (ragged for both builders: 2 x 8 + 1, 16 + 1) in the smallest batch the heuristics send there (52 / 86 filters on 256 CUs): every
    filter from the same bits, every filter inside the bound on all four families, and launch_shape() proves the builder."""
    import torch

    N = 17
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = builder_batch(cus, N, lm)
    fg = make_handle(hip, monkeypatch, {}, N + 5, batch=B, burst=True)
    try:
        snap = snapshot(hip, N)
        worst, bad, shape = {}, [], None
        for fam in rc.FAMILIES:
            S0, calls, Sref, E, _ = reference(hip, N, fam)
            for b, S in enumerate(step(fg, [snap] * B, [S0] * B, [calls] * B)):
                check(S, Sref, E, (f"builder{lm}", N, b, fam), worst, bad, transposes=True)
            if shape is None:  # (recorded for the first burst of a handle only; the later ones have the same batch, N and environment)
                shape = fg.launch_shape()
                assert shape["builder_landmarks"] == lm and not shape["fused"] and shape["steps"] == 1, (B, cus, shape)
        report(f"burst, {lm}-landmark builder, {B} filters of N = {N}, shape {shape}", worst)
        assert fg.device_error() == 0
    finally:
        fg.close()
    assert not bad, bad[:10]


@pytest.mark.parametrize("route", ["fused", "split", "burst"])
def test_ragged_batch_of_three(hip, monkeypatch, route):
    """N = 5, 17, 33 in one handle of capacity 38: each filter against its own reference."""
    env = SINGLE.get(route, {})
    fg = make_handle(hip, monkeypatch, env, max(rc.RAGGED) + 5, batch=3, burst=route == "burst")
    worst, bad = {}, []
    try:
        for fam in rc.FAMILIES:
            refs = [reference(hip, N, fam) for N in rc.RAGGED]
            Ss = step(fg, [snapshot(hip, N) for N in rc.RAGGED], [r[0] for r in refs], [r[1] for r in refs])
            for N, S, r in zip(rc.RAGGED, Ss, refs):
                check(S, r[2], r[3], (route, N, fam), worst, bad, transposes=route == "burst")
        report(f"ragged batch, {route}", worst)
        assert fg.device_error() == 0
    finally:
        fg.close()
    assert not bad, bad[:10]


@pytest.mark.parametrize("N", rc.KSTEP)
def test_burst_of_four_calls(hip, monkeypatch, N):
    """Four queued calls in one burst, the second repeating the first's stamp (it must change nothing but the sample): against the K-step
    reference and the bound pushed through |F| e |F|^T step by step.  Default shape and the two-launch shape."""
    worst, bad = {}, []
    for route, env in (("burst-default", {}), ("burst-rows2-fused0", BURST["burst-rows2-fused0"])):
        shape = run_route(hip, monkeypatch, route, env, N, rc.FAMILIES_FOUR, worst, bad, four=True)
        assert shape["steps"] == 4, shape
    report(f"burst of four, N = {N}", worst)
    assert not bad, bad[:10]


@pytest.mark.parametrize("route", ["fused", "split", "burst"])
def test_fp32_handles(hip, monkeypatch, route):
    """precision = PRECISION_F32 at N = 17 and 70 with the fp32 bound: u = 2^-24 in gamma_k, and one storage rounding each of the input Sigma,
    of every block entry and of the output."""
    env = SINGLE.get(route, {})
    worst, bad = {}, []
    for N in rc.F32:
        run_route(hip, monkeypatch, route, env, N, rc.FAMILIES, worst, bad, precision=hip.PRECISION_F32)
    report(f"fp32, {route}", worst)
    assert not bad, bad[:10]


@pytest.mark.parametrize("N,bl", rc.TILED + rc.TILED_BIG[:1])
def test_partitioned_filter(hip, N, bl):
    """(200, 64 -- rc.TILED_BIG: four block rows, the last one ragged, 13 landmark tiles of 16 per row -- as well as rc.TILED.)
    tiled.TiledFilter on a 1 x 1 grid through initialise_from(snapshot), stateCovariance() against the same reference.  The filter queues IMU
    calls by default (TiledFilter.burst) and a getter flushes them through k_tl_build / k_tl_base / k_tl_riccati_burst, also when one call is
    queued; k_tl_riccati runs only with burst = False.  So: one processIMUData with burst off (k_tl_riccati) and with burst on
    (k_tl_riccati_burst, one step) on all four families, and one burst of four (the second call on the first's stamp) on families a, b, c."""
    from eqf_vio_amd import tiled

    snap = snapshot(hip, N)
    worst, bad = {}, []
    cases = [(fam, False, burst) for burst in (False, True) for fam in rc.FAMILIES] + [(fam, True, True) for fam in rc.FAMILIES_FOUR]
    for fam, four, burst in cases:
        S0, calls, Sref, E, _ = reference(hip, N, fam, four)
        be = tiled.HipBackend(rc.settings(), capacity=N + 5)
        tf = tiled.TiledFilter(tiled.ProcessGrid(None, 1, 1, device=be.device), be, bl)
        try:
            tf.burst = burst
            tf.initialise_from(dict(snap, sigma=S0))
            for stamp, w, a in calls:
                tf.processIMUData(stamp, w, a)
            S = tf.stateCovariance()
            kernel = "k_tl_riccati_burst x 4 calls" if four else ("k_tl_riccati_burst" if burst else "k_tl_riccati")
            check(S, Sref, E, (kernel, N, bl, fam + ("4" if four else "") + ("" if burst else "-single")), worst, bad)
            assert be.device_error() == 0 and tf.device_error() == 0
        finally:
            tf.close()
    report(f"partitioned filter, N = {N}, blocks of {bl}", worst)
    assert not bad, bad[:10]
