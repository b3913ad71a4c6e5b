"""Every device route of the vision update entry by entry against the reference of tests/update_exact.py, within its a-priori bound: after
restore_state and ONE vision call (integrate to the stamp, then update)
    Sigma+ inside its bound at EVERY entry and symmetric to the bound        gamma and delta inside their bounds at every entry
    Gamma[0:6] inside its bound at every entry (N >= 2, families a, c, e)    Gamma[6:] bit for bit gamma[8:] (the kernel copies it)
    bias_after - bias_before within one rounding of gamma[0:6]               device_error() == 0
Public API only.  States, Sigma families, sizes and the call: tests/update_cases.py; the same cases hold two fp64 numpy restatements and a
model of the blocked kernels inside the bound on the CPU (tests/test_update_exact.py), where K_delta is measured from the fp64 oracle and
eleven injected faults leave the bound.  No constant here comes from the device.

Routes: the default launch shape at every size (per-column launches below N = 20, the one-launch k_chol_resident from there), the prep work
as a launch of its own (EQF_RES_FOLD_PREP=0), the per-column launches fused and split (EQF_CHOL_RESIDENT=0, EQF_CHOL_SPLIT=0 / 1), the
int8-slice downdate, fp32 handles, the operands C Sigma' and S left by a burst, a ragged handle, an oversubscribed grid with and without
arrival tickets, and the partitioned filter on a 1 x 1 grid.

Worst ratio to the bound per route on an MI355X (each test prints its own): NOTES.md R15.1 -- fp64 routes Sigma+ 0.001 .. 0.10, gamma <= 0.15,
delta <= 0.26, Gamma[0:6] <= 0.016; the int8-slice downdate 0.09 of its slice bound; fp32 handles Sigma+ <= 0.20, gamma <= 0.31."""
import numpy as np
import pytest

import riccati_cases as rc
import update_cases as uc
import update_exact as ux

pytestmark = pytest.mark.gpu

ENV_KEYS = ("EQF_RES_FOLD_PREP", "EQF_CHOL_RESIDENT", "EQF_CHOL_SPLIT", "EQF_BURST_FUSED", "EQF_BURST_ROWS", "EQF_IMU_BURST", "EQF_SPLIT_PROPAGATE")
_SNAP, _CASE, _REF = {}, {}, {}


@pytest.fixture(scope="module")
def hip():
    from eqf_vio_amd import binding

    return binding


def snapshot(hip, N):
    if N not in _SNAP:
        _SNAP[N] = rc.device_snapshot(hip, N)
    return _SNAP[N]


def reference(hip, N, fam, fp32=False, burst=False, slices=0):
    """(Sigma the call starts from, (stamp, ids, bearings), ref, bounds): computed once per case for the whole module.  burst: three IMU calls
    are queued in front of the vision call, the reference steps through all four."""
    key = (N, fam, fp32, burst, slices)
    if key not in _REF:
        snap = snapshot(hip, N)
        call = uc.vision_call(N, fam)
        ck = (N, "e" if fam == "e" else "a", burst)
        if ck not in _CASE:
            _CASE[ck] = ux.Case(snap, uc.settings(), call[0], call[2], uc.imu_calls_before(N) if burst else ())
        S0 = uc.sigma_family(snap, fam)
        assert np.array_equal(S0, S0.T)
        _REF[key] = (S0, call) + _CASE[ck].reference(S0, fp32, slices)
    return _REF[key]


def make_handle(hip, monkeypatch, env, capacity, batch=1, precision=None):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    f = hip.FilterBatch(uc.settings(), capacity=capacity, batch=batch, **({} if precision is None else {"precision": precision}))
    for k in env:
        monkeypatch.delenv(k)
    return f


def check(out, N, fam, ref, bd, what, worst, bad):
    """out: dict(Sp, delta, gamma, Gamma, bias_before, bias_after) of one filter"""
    r = {k: ux.worst_ratio(out[k], ref[k], bd[k]) for k in ("Sp", "gamma", "delta")}
    r["symmetry"] = (ux.symmetry_ratio(out["Sp"], bd["Sp"]), None)
    if uc.gamma6_asserted(N, fam):
        r["Gamma6"] = ux.worst_ratio(out["Gamma"][0:6], ref["Gamma6"], bd["Gamma6"])
    else:
        print(f"{what}: Gamma[0:6] reported only: device {out['Gamma'][0:6]}, reference {ux.f64(ref['Gamma6'])}, "
              f"ratio {ux.worst_ratio(out['Gamma'][0:6], ref['Gamma6'], bd['Gamma6'])[0]:.3g}")
    q = worst.setdefault(fam, {})
    for k, (v, at) in r.items():
        q[k] = max(q.get(k, (0.0,)), (v, at, what))
        if not v <= 1.0:
            bad.append((what, fam, k, v, at))
    if not all(np.all(np.isfinite(out[k])) for k in ("Sp", "gamma", "delta", "Gamma")):
        bad.append((what, fam, "not finite"))
    if not np.array_equal(out["Gamma"][6:], out["gamma"][8:]):
        bad.append((what, fam, "Gamma[6:] is not a copy of gamma[8:]"))
    # bias <- fl(bias + gamma[0:6]): one rounding of the sum, u |bias_after| <= 2 u max(|bias_before|, |gamma|); the difference is formed in
    # longdouble here, where it is exact
    step = out["bias_after"].astype(ux.LD) - out["bias_before"].astype(ux.LD)
    if not np.all(np.abs(step - out["gamma"][0:6].astype(ux.LD)) <= ux.U64 * np.abs(out["bias_after"])):
        bad.append((what, fam, "bias step", ux.f64(step), out["gamma"][0:6]))


def report(route, worst):
    print(f"{route}: worst ratio to the bound  " + "   ".join(
        f"{fam}: " + " ".join(f"{k} {v[0]:.3g}" for k, v in sorted(q.items())) for fam, q in sorted(worst.items())))


def read(fg, b, bias_before):
    lu = fg.last_update(b)
    return dict(Sp=fg.sigma(b), delta=lu["delta"], gamma=lu["gamma"], Gamma=lu["Gamma"], bias_before=bias_before, bias_after=fg.bias(b))


def one_call(fg, snaps, S0s, calls, imu=None):
    """restore every filter of the handle, (queue the IMU calls,) one vision call, read every filter"""
    B = len(snaps)
    for b, (snap, S0) in enumerate(zip(snaps, S0s)):
        fg.restore_state(dict(snap, sigma=S0), b)
    before = [fg.bias(b) for b in range(B)]
    for k in range(len(imu[0]) if imu else 0):
        fg.process_imu([c[k][0] for c in imu], np.array([c[k][1] for c in imu]), np.array([c[k][2] for c in imu]))
    stride = max(len(c[1]) for c in calls)
    ids, y = np.zeros((B, stride), dtype=np.int32), np.zeros((B, stride, 3))
    for b, (_, i, yy) in enumerate(calls):
        ids[b, :len(i)], y[b, :len(i)] = i, yy
    st = fg.process_vision([c[0] for c in calls], ids, y, nb=[len(c[1]) for c in calls])
    assert np.all(st == 0), st
    return [read(fg, b, before[b]) for b in range(B)]


def run_route(hip, monkeypatch, route, env, sizes, fams, precision=None, option=None):
    worst, bad = {}, []
    for N in sizes:
        fg = make_handle(hip, monkeypatch, env, N + 5, precision=precision)
        try:
            if option:
                fg.set_option(*option)
            snap = snapshot(hip, N)
            for fam in fams:
                S0, call, ref, bd = reference(hip, N, fam, precision is not None, slices=option[1] if option and option[0] == "downdate_slices" else 0)
                (out,) = one_call(fg, [snap], [S0], [call])
                check(out, N, fam, ref, bd, (route, N), worst, bad)
            assert fg.device_error() == 0, (route, N)
        finally:
            fg.close()
    report(route, worst)
    assert not bad, bad[:10]


@pytest.mark.parametrize("N", uc.SIZES)
def test_default_route(hip, monkeypatch, N):
    """All four families at one size.  The one-launch kernel runs where the E-chain has more block columns than the S-chain (updateShape in
    csrc/eqf_capi.hip: N = 20, 21, 32, 42, 64, 65, 70, with the prep roles folded in), the per-column launches (k_update_prep64,
    k_chol_step64) where they have equally many (N = 1, 2, 5, 19, 33, 41); 19 / 20 / 21, 32 / 33, 41 / 42, 64 / 65 straddle a 64-column edge
    of the E- or the S-chain."""
    run_route(hip, monkeypatch, "default", {}, (N,), uc.FAMILIES)


def test_prep_as_its_own_launch(hip, monkeypatch):
    run_route(hip, monkeypatch, "EQF_RES_FOLD_PREP=0", {"EQF_RES_FOLD_PREP": "0"}, uc.FOLD_PREP0, uc.FAMILIES)


@pytest.mark.parametrize("split", ["0", "1"])
def test_per_column_launches(hip, monkeypatch, split):
    run_route(hip, monkeypatch, f"EQF_CHOL_RESIDENT=0 EQF_CHOL_SPLIT={split}", {"EQF_CHOL_RESIDENT": "0", "EQF_CHOL_SPLIT": split}, uc.PER_COLUMN, uc.FAMILIES)


def test_int8_slice_downdate(hip, monkeypatch):
    """set_option("downdate_slices", 6): Y cut into six 7-bit slices, the downdate on the integer matrix pipe.  E3 of the bound is the
    rigorous bound of that construction (tests/i8_emulator.py: bound) from the exponent words of the reference's Y; every other term is the
    fp64 one -- gamma, delta and Gamma do not go through the slices."""
    run_route(hip, monkeypatch, "downdate_slices=6", {}, uc.SLICES, uc.FAMILIES, option=("downdate_slices", 6))


def test_fp32_handles(hip, monkeypatch):
    """PRECISION_F32: Sigma stored as float, the downdate on Y rounded to float, factorisations fp64 -- the fp32 bound (u = 2^-24 in E3 and the
    storage terms, riccati_exact's fp32 E_ric)."""
    run_route(hip, monkeypatch, "fp32", {}, uc.F32, uc.F32_FAMILIES, precision=hip.PRECISION_F32)


@pytest.mark.parametrize("N", uc.BURST)
def test_operands_left_by_the_burst(hip, monkeypatch, N):
    """set_imu_burst(15), three IMU calls, then the vision call closes the burst, which leaves C Sigma' and S from the blocks its workgroups
    hold (debug_option "cs_in_burst" = 2: with every rows-per-wavefront build; launch_shape()["cs_out"] proves it).  One small filter would
    take the fused burst launch, which never leaves the operands (launchBurst: !fused), so the handle is made with EQF_BURST_FUSED=0: the
    two-launch burst.  The reference steps the group and Sigma through all four calls."""
    worst, bad = {}, []
    fg = make_handle(hip, monkeypatch, {"EQF_BURST_FUSED": "0"}, N + 5)
    try:
        fg.set_imu_burst(15)
        fg.debug_option("cs_in_burst", 2)
        snap = snapshot(hip, N)
        for fam in uc.FAMILIES:
            S0, call, ref, bd = reference(hip, N, fam, burst=True)
            (out,) = one_call(fg, [snap], [S0], [call], imu=[uc.imu_calls_before(N)])
            shape = fg.launch_shape()
            assert shape["cs_out"] and not shape["fused"] and shape["steps"] == 4, shape
            check(out, N, fam, ref, bd, ("burst operands", N), worst, bad)
        assert fg.device_error() == 0
    finally:
        fg.close()
    report(f"operands left by the burst, N = {N}", worst)
    assert not bad, bad[:10]


def test_ragged_handle(hip, monkeypatch):
    """N = 5, 21, 33 in one handle of capacity 38: each filter against its own reference."""
    worst, bad = {}, []
    fg = make_handle(hip, monkeypatch, {}, max(uc.RAGGED) + 5, batch=3)
    try:
        for fam in uc.FAMILIES:
            refs = [reference(hip, N, fam) for N in uc.RAGGED]
            outs = one_call(fg, [snapshot(hip, N) for N in uc.RAGGED], [r[0] for r in refs], [r[1] for r in refs])
            for N, out, r in zip(uc.RAGGED, outs, refs):
                check(out, N, fam, r[2], r[3], ("ragged", N), worst, bad)
        assert fg.device_error() == 0
    finally:
        fg.close()
    report("ragged handle", worst)
    assert not bad, bad[:10]


def test_oversubscribed_grid(hip, monkeypatch):
    """N = 200 (S-chain 7 block columns, E-chain 10: 146 chain roles per filter), the same restored state in every filter of a handle of 3 and
    of a handle of 16, family e; one reference serves both.  By the heuristics of csrc/eqf_capi.hip (updateShape) on a 256-CU part: 3 filters
    are 438 roles, more than the chip holds, and prep + chain roles stay under six per CU -- k_chol_resident<double, PIPEH, FOLD> with the
    prep roles in front; 16 filters are 9.1 roles per CU -- the two-workgroups-per-CU build <double, PIPEH, OCC2> behind the prep launch,
    and with debug_option "res_tickets" = 2 its TICKET build.  (The handle does not expose which build ran.)  Every filter is inside the bound
    and the filters of a handle are bit for bit equal to each other."""
    N, fam = uc.BATCH_N, "e"
    worst, bad = {}, []
    S0, call, ref, bd = reference(hip, N, fam)
    snap = snapshot(hip, N)
    for B, tickets in ((3, 0), (16, 0), (16, 2)):
        fg = make_handle(hip, monkeypatch, {}, N + 5, batch=B)
        try:
            fg.debug_option("res_tickets", tickets)
            outs = one_call(fg, [snap] * B, [S0] * B, [call] * B)
            assert fg.device_error() == 0
        finally:
            fg.close()
        check(outs[0], N, fam, ref, bd, (f"batch {B} tickets {tickets}", N), worst, bad)
        for b in range(1, B):
            for k in ("Sp", "delta", "gamma", "Gamma", "bias_after"):
                if not np.array_equal(outs[b][k], outs[0][k]):
                    bad.append((B, tickets, b, k, "differs from filter 0"))
    report("oversubscribed grid, N = 200", worst)
    assert not bad, bad[:10]


@pytest.mark.parametrize("N,bl", uc.TILED)
def test_partitioned_filter(hip, N, bl):
    """tiled.TiledFilter on a 1 x 1 grid through initialise_from(snapshot), the IMU queue off (burst = False): one processVisionData, then
    stateCovariance(), lastUpdate() and bias() against the same reference."""
    from eqf_vio_amd import tiled

    snap = snapshot(hip, N)
    worst, bad = {}, []
    for fam in uc.FAMILIES:
        S0, (stamp, ids, y), ref, bd = reference(hip, N, fam)
        be = tiled.HipBackend(uc.settings(), capacity=N + 5)
        tf = tiled.TiledFilter(tiled.ProcessGrid(None, 1, 1, device=be.device), be, bl)
        try:
            tf.burst = False
            tf.initialise_from(dict(snap, sigma=S0))
            before = tf.bias()
            assert tf.processVisionData(stamp, ids, y) == 0
            lu = tf.lastUpdate()
            out = dict(Sp=tf.stateCovariance(), delta=lu["delta"], gamma=lu["gamma"], Gamma=lu["Gamma"], bias_before=before, bias_after=tf.bias())
            check(out, N, fam, ref, bd, ("partitioned", N, bl), worst, bad)
            assert be.device_error() == 0 and tf.device_error() == 0
        finally:
            tf.close()
    report(f"partitioned filter, N = {N}, blocks of {bl}", worst)
    assert not bad, bad[:10]


def test_gamma6_at_one_landmark_is_recorded(oracle_lib, hip, monkeypatch):
    """N = 1: bundleLift's 4 x 4 normal equations are singular (coeffMat is 3 x 4, cond(M) ~ 3e16) and Gamma[0:6] is decided by rounding in
    each implementation's own formula.  Recorded, not gated: what the device, the numpy oracle and the C++ oracle return on the same restored
    state and the same call, beside the longdouble reference (DESIGN.md section 5 keeps the figures).  Gamma[6:] is well defined and is held."""
    import lie_edge_cases as ec
    from oracle import eqf_numpy as en

    N, fam = 1, "e"
    S0, (stamp, ids, y), ref, bd = reference(hip, N, fam)
    snap = dict(snapshot(hip, N), sigma=S0)
    fg = make_handle(hip, monkeypatch, {}, N + 5)
    try:
        (out,) = one_call(fg, [snap], [S0], [(stamp, ids, y)])
        assert fg.device_error() == 0
    finally:
        fg.close()
    fn = ec.numpy_filter(en, snap, uc.settings())
    fn.processVisionData(stamp, ids, y)
    fo = oracle_lib.OracleFilter(uc.settings())
    fo.set_state(snap)
    fo.processVisionData(stamp, ids, y)
    rows = {"device": out["Gamma"], "numpy oracle": fn.last["Gamma"], "C++ oracle": fo.last_update()["Gamma"]}
    print(f"N = 1, family e: reference Gamma[0:6] {ux.f64(ref['Gamma6'])}, bound / max|Gamma[0:6]| {bd['Gamma6'].max() / np.abs(ux.f64(ref['Gamma6'])).max():.3g}")
    for name, G in rows.items():
        print(f"    {name:13s} Gamma[0:6] {np.asarray(G)[0:6]}")
        assert ux.worst_ratio(np.asarray(G)[6:], ref["gamma"][8:], bd["gamma"][8:])[0] <= 1.0, name
