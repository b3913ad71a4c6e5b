"""The deterministic split on the device (csrc/eqf_split.hpp: eqf_split_filters; FilterBatch.split_filters).

Two yardsticks.  (1) Entry by entry: every Sigma_k and gamma_k against the 50-digit reference of split_exact.py computed from the source's own
sigma(), inside its a-priori bound (K_SPLIT measured on the host, never here); the worst ratio is printed.  (2) Bit for bit, the fork
pattern of test_gpu_schmidt.py: a twin handle is a full copy of the handle before the call and gets eqf_copy_filters with the same
(dst, src) and eqf_apply_increment with the gamma rows the split returned; every child's state then has the twin's bits, a child without
shrink the source's Sigma bits, a (0, 0) child is the copy itself, and filters that are not named keep every bit.

The sources come from ONE batch of six filters after five frames of a synthetic stream, holding N = 85, 21, 5, 1, 0 landmarks and a spare
slot (capacity 87), each Sigma's lower triangle mirrored; the shapes N = 1 (order 15), 5 (27: one tile), 21 (75: across a 64 edge) and 85
(267: past the 256-lane and the 16-row chunks) are also run alone in handles of capacity N + 2, whose leading dimension is ragged against
the order.  At N = 85 the K = 3 call checks every entry of every child against the bound; the second call there (the edge children) and
the moment identity with local = 0 leave the 50-digit part out, for its run time alone -- their bitwise checks stay.  Nothing here
provokes a fault: the zero row and the indefinite Sigma are ordinary numeric verdicts."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lift_cases as lc  # noqa: E402
import split_exact as sx  # noqa: E402

pytestmark = pytest.mark.gpu
COUNTS = [85, 21, 5, 1, 0, 0]
SLOT = {85: 0, 21: 1, 5: 2, 1: 3, 0: 4}
SPARE = 5
CAP = 87
FRAMES = 5


@pytest.fixture(scope="module")
def hip():
    from eqf_vio_amd import binding

    return binding


@pytest.fixture(scope="module")
def stream():
    from eqf_vio_amd import synth

    return synth.make_stream(85, duration=0.45)


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


def _run(fg, st, f0, f1, nb):
    for kind, k in _events(st, f0, f1):
        if kind == "imu":
            r = st.imu[k]
            fg.process_imu(r[0], r[1:4], r[4:7])
        else:
            fg.process_vision(st.vision_stamps[k], st.ids, st.bearings[k], nb=nb)


@pytest.fixture(scope="module")
def base(hip, stream):
    """the batch of six after five frames, every Sigma's lower triangle mirrored; the tests fork it and never change it"""
    fg = hip.FilterBatch(lc.settings(1), capacity=CAP, batch=6)
    _run(fg, stream, 0, FRAMES, COUNTS)
    assert [fg.num_landmarks(b) for b in range(6)] == COUNTS and fg.device_error() == 0
    for b in range(6):
        S = fg.sigma(b)
        fg.set_sigma(np.tril(S) + np.tril(S, -1).T, b)
        S = fg.sigma(b)
        assert S.tobytes() == np.ascontiguousarray(S.T).tobytes()
    yield fg
    fg.close()


def _fork(hip, src, batch=None, capacity=None, pairs=None):
    """a handle that holds copies of src's filters: all of them, or pairs = (dst list, src list)"""
    fg = hip.FilterBatch(lc.settings(1), capacity=capacity or src.cap, batch=batch or src.B)
    d, s = pairs if pairs else (list(range(src.B)), list(range(src.B)))
    fg.copy_filters(src, d, s)
    return fg


def _bits(x):
    if isinstance(x, dict):
        return {k: _bits(v) for k, v in x.items()}
    return np.ascontiguousarray(x).tobytes() + str(np.asarray(x).shape).encode()


def _getters(fg, b):
    g = dict(n=fg.num_landmarks(b), est=fg.state_estimate(b), last=fg.last_update(b))
    g.update(fg.dump_state(b))  # ids, origin, group, bias, sigma, time, integrator
    return g


def _same(a, b, what, skip=()):
    a, b = _bits(a), _bits(b)
    assert a.keys() == b.keys()
    for k in a:
        if k not in skip:
            assert a[k] == b[k], f"{what}: getter {k} differs"


def _dense_row(n, seed):
    return np.random.default_rng([411, seed, n]).standard_normal(n)


def _depth_row(fg, b, i):
    from eqf_vio_amd import consistency as cs

    return cs.depth_axis_row(fg.state_estimate(b)["p"][i], i, 11 + 3 * fg.num_landmarks(b))


_REF = {}


def _reference(key, Sigma, a, J, shift, shrink):
    """(the 50-digit reference, the bounds, Sbar) of one source, computed once per key"""
    if key not in _REF:
        Ht, Hbar = sx.row_mp(a, J)
        _REF[key] = (sx.exact(Sigma, Ht, shift, shrink), sx.bound(Sigma, Hbar, shift, shrink), float(Hbar @ (np.abs(Sigma) @ Hbar)))
    return _REF[key]


def _split_and_check(hip, fg, rows, children, local, key, lift=False, exact=True):
    """Splits on fg (rows: {src: a}; children: (dst, src, shift, shrink)) and checks everything that holds for a call whose sources all
    succeed: the twin's bits, the exactness rules, symmetry, the untouched filters and the bound.  Returns (out, getters after)."""
    from eqf_vio_amd import consistency as cs

    B = fg.B
    twin = _fork(hip, fg)
    before = [_getters(fg, b) for b in range(B)]
    for b in range(B):
        _same(_getters(twin, b), before[b], f"twin of filter {b}")
    dst, src = [c[0] for c in children], [c[1] for c in children]
    shift, shrink = np.array([c[2] for c in children], dtype=float), np.array([c[3] for c in children], dtype=float)
    J = {s: cs.jacobian_matrix(fg.local_jacobian(s)) for s in rows} if local else {s: None for s in rows}
    if lift:
        fg.set_option("innovation_lift", 1)
    out = fg.split_filters([rows.get(b) for b in range(B)], dst, src, shift, shrink, local=local, want_gamma=True, report=True)
    assert fg.device_error() == 0 and out["info"].tolist() == [0] * len(children)
    # the twin: the copy, then the increments the split returned
    twin.copy_filters(twin, dst, src)
    G = [np.zeros(11 + 3 * twin.num_landmarks(b)) for b in range(B)]
    mask = np.zeros(B, dtype=np.uint8)
    for k, (d, s, sh, sk) in enumerate(children):
        n = 11 + 3 * before[s]["n"]
        assert not out["gamma"][k][n:].any()
        if sh != 0.0:
            G[d], mask[d] = out["gamma"][k][:n], 1
        else:
            assert not out["gamma"][k].any()
    if mask.any():
        twin.apply_increment(G, mask)
    after = [_getters(fg, b) for b in range(B)]
    for k, (d, s, sh, sk) in enumerate(children):
        what = f"{key} child {k} ({d} <- {s}, shift {sh}, shrink {sk})"
        _same(after[d], _getters(twin, d), what, skip=() if sk == 0.0 else ("sigma",))     # checks 3, 5, 6: the state is the twin's
        Sd = after[d]["sigma"]
        assert Sd.tobytes() == np.ascontiguousarray(Sd.T).tobytes(), what + ": Sigma is not bitwise symmetric"  # check 2
        if sk == 0.0:
            assert _bits(Sd) == _bits(before[s]["sigma"]), what + ": Sigma differs from the source's"      # check 4
        if sh == 0.0:
            _same(after[d], before[s], what + " (the source's state)", skip=("sigma",))               # check 5
    for b in range(B):
        if b not in dst:
            _same(after[b], before[b], f"{key}: filter {b} is not named")
    if exact:
        worst = {"Sigma": 0.0, "gamma": 0.0}
        for s, a in rows.items():
            ks = [k for k in range(len(children)) if src[k] == s]
            ref, (bS, bG), Sbar = _reference((key, s), before[s]["sigma"], a, J[s], shift[ks], shrink[ks])
            n = 11 + 3 * before[s]["n"]
            r = sx.ratios([after[dst[k]]["sigma"] for k in ks], [out["gamma"][k][:n] for k in ks], ref, bS, bG)
            worst = {q: max(worst[q], r[q]) for q in worst}
            assert abs(out["S"][ks[0]] - float(ref["S"])) <= sx.K_SPLIT * sx.EPS * Sbar and all(out["S"][k] == out["S"][ks[0]] for k in ks)
        print(f"{key}: worst ratio against the exact reference, in units of the bound (K_SPLIT = {sx.K_SPLIT:g}): {worst}")
        assert worst["Sigma"] <= 1.0 and worst["gamma"] <= 1.0, (key, worst)
    twin.close()
    return out, after


KIDS3 = [(0.0, 0.0), (0.9, 0.0), (0.0, 0.6)]


@pytest.mark.parametrize("N", [1, 5, 21, 85])
@pytest.mark.parametrize("local", [0, 1])
def test_shapes_alone_in_ragged_handles(hip, base, N, local):
    """Checks 1-6 at every shape: a handle of capacity N + 2 with three filters, all copies of the source; filter 0 splits into the K = 3
    components of split_components (one in place, shift and shrink both set) and, in a second call, into the edge children (0, 0),
    (shift, 0) and (0, shrink)."""
    from eqf_vio_amd import consistency as cs

    fg = _fork(hip, base, batch=3, capacity=N + 2, pairs=([0, 1, 2], [SLOT[N]] * 3))
    a = _depth_row(fg, 0, N // 2) if local else _dense_row(11 + 3 * N, N)
    w, sh, sk = cs.split_components(3, 1.1, outer_weight=0.2)
    kids = [(b, 0, sh[b], sk[b]) for b in range(3)]
    out, after = _split_and_check(hip, fg, {0: a}, kids, local, f"alone N={N} local={local} K=3")
    # check 10: the moment identity from the children's own sigma() and gamma, in the origin chart
    if N < 85 or local:  # (the largest order once: the sum is taken at 50 digits)
        ref, (bS, bG), _ = _REF[(f"alone N={N} local={local} K=3", 0)]
        S0 = base.sigma(SLOT[N])
        r = sx.moment_ratio(w, [after[b]["sigma"] for b in range(3)], [out["gamma"][b][:11 + 3 * N] for b in range(3)], S0, bS, bG)
        print(f"alone N={N} local={local}: moment identity, worst ratio {r}")
        assert r <= 1.0
    fg.close()
    fg = _fork(hip, base, batch=3, capacity=N + 2, pairs=([0, 1, 2], [SLOT[N]] * 3))
    kids = [(b, 0, KIDS3[b][0], KIDS3[b][1]) for b in range(3)]
    _split_and_check(hip, fg, {0: a}, kids, local, f"alone N={N} local={local} edges", exact=N < 85)
    fg.close()


def test_increment_step_is_the_plain_one_whatever_the_option(hip, base):
    """Check 6, second half: with "innovation_lift" = 1 on the split handle the children still have the bits of eqf_apply_increment on a
    twin WITHOUT the option."""
    fg = _fork(hip, base, batch=3, capacity=23, pairs=([0, 1, 2], [SLOT[21]] * 3))
    kids = [(0, 0, -0.8, 0.3), (1, 0, 0.8, 0.3), (2, 0, 0.4, 0.0)]
    _split_and_check(hip, fg, {0: _dense_row(74, 7)}, kids, 0, "lift option", lift=True, exact=False)
    fg.close()


def test_fan_out_two_sources_and_a_source_alone_against_the_batch(hip, base):
    """Check 7: K = 5 children of the N = 21 filter with one in place, the N = 5 filter split in the same call into the N = 0 slot and in
    place -- the N = 85 filter is not named and keeps every bit; then the N = 21 filter alone in a one-filter handle against the same child
    in place inside the batch, bit for bit."""
    B21, B5 = SLOT[21], SLOT[5]
    big = hip.FilterBatch(lc.settings(1), capacity=CAP, batch=9)
    big.copy_filters(base, list(range(6)), list(range(6)))
    rows = {B21: _dense_row(74, 21), B5: _depth_row(big, B5, 3)}
    kids = [(B21, B21, 0.5, 0.2), (SPARE, B21, -0.5, 0.2), (6, B21, 0.0, 0.0), (7, B21, 1.2, 0.0), (8, B21, 0.0, 0.7),
            (SLOT[0], B5, -1.0, 1.0), (B5, B5, 1.0, 1.0)]
    out, after = _split_and_check(hip, big, rows, kids, 1, "fan-out")
    assert [big.num_landmarks(b) for b in range(9)] == [85, 21, 5, 1, 5, 21, 21, 21, 21]
    alone = _fork(hip, base, batch=1, capacity=23, pairs=([0], [B21]))
    o1 = alone.split_filters([rows[B21]], [0], [0], [0.5], [0.2], local=True, want_gamma=True)
    _same(_getters(alone, 0), after[B21], "a source alone in a handle against the batch")
    assert _bits(o1["gamma"][0][:74]) == _bits(out["gamma"][0][:74]) and _bits(o1["S"][0]) == _bits(out["S"][0])
    # ... and from run to run
    again = _fork(hip, base, batch=1, capacity=23, pairs=([0], [B21]))
    again.split_filters([rows[B21]], [0], [0], [0.5], [0.2], local=True, report=False)
    _same(_getters(again, 0), _getters(alone, 0), "run to run")
    for h in (big, alone, again):
        assert h.device_error() == 0
        h.close()


@pytest.mark.parametrize("report", [True, False])
@pytest.mark.parametrize("why", ["zero_row", "indefinite"])
def test_a_failed_source_writes_nothing_and_the_other_is_applied(hip, base, why, report):
    """Check 8: source N = 5 fails (an all-zero row: S = 0; or an indefinite Sigma put there with set_sigma: S < 0), source N = 21 of the same
    call succeeds."""
    B21, B5, B1 = SLOT[21], SLOT[5], SLOT[1]
    fg = _fork(hip, base)
    a5 = np.zeros(26)
    if why == "indefinite":
        S = fg.sigma(B5)
        S[12, 12] = -S[12, 12]
        fg.set_sigma(S, B5)
        a5[12] = 1.0
    rows = {B5: a5, B21: _dense_row(74, 3)}
    kids = [(B5, B5, 0.5, 0.5), (B1, B5, -0.5, 0.5), (B21, B21, 0.7, 0.4), (SPARE, B21, -0.7, 0.4)]
    dst, src = [k[0] for k in kids], [k[1] for k in kids]
    before = [_getters(fg, b) for b in range(6)]
    out = fg.split_filters([rows.get(b) for b in range(6)], dst, src, [k[2] for k in kids], [k[3] for k in kids], local=False,
                           want_gamma=report, report=report)
    after = [_getters(fg, b) for b in range(6)]
    assert fg.device_error() == 0
    if report:
        assert out["info"].tolist() == [1, 1, 0, 0] and np.isnan(out["S"][:2]).all() and (out["S"][2:] > 0).all()
        assert not out["gamma"][:2].any() and out["gamma"][2:].any()
    else:
        assert out is None
    for b in (B5, B1, SLOT[85], SLOT[0]):
        _same(after[b], before[b], f"{why}: filter {b} of the failed source (or not named)")
    # the other source of the same call: what the call gives without the failing one
    ok = _fork(hip, base)
    ok.split_filters([rows.get(b) if b == B21 else None for b in range(6)], dst[2:], src[2:], [k[2] for k in kids[2:]], [k[3] for k in kids[2:]],
                     local=False)
    for b in (B21, SPARE):
        _same(after[b], _getters(ok, b), f"{why}: filter {b} of the source that succeeds")
    assert after[SPARE]["n"] == 21 and _bits(after[B21]["sigma"]) != _bits(before[B21]["sigma"])
    fg.close(), ok.close()


def test_local_rows_against_origin_rows_fed_a_J(hip, base):
    """Check 9: local = 1 with a against local = 0 with a J, J from eqf_get_local_jacobian -- both inside the bound about the same exact
    reference (a J at 50 digits)."""
    from eqf_vio_amd import consistency as cs

    b = SLOT[21]
    a = _dense_row(74, 99)
    a[:6] = 0.0
    J = cs.jacobian_matrix(base.local_jacobian(b))
    S0 = base.sigma(b)
    shift, shrink = np.array([0.9, -0.9]), np.array([0.5, 0.5])
    Ht, Hbar = sx.row_mp(a, J)
    ref, (bS, bG) = sx.exact(S0, Ht, shift, shrink), sx.bound(S0, Hbar, shift, shrink)
    for local, row in ((1, a), (0, a @ J)):
        fg = _fork(hip, base)
        out = fg.split_filters([row if q == b else None for q in range(6)], [b, SPARE], [b, b], shift, shrink, local=bool(local), want_gamma=True)
        assert out["info"].tolist() == [0, 0]
        r = sx.ratios([fg.sigma(b), fg.sigma(SPARE)], [out["gamma"][k][:74] for k in range(2)], ref, bS, bG)
        print(f"local={local}: worst ratio {r}")
        assert r["Sigma"] <= 1.0 and r["gamma"] <= 1.0
        fg.close()


def test_argument_errors_leave_the_handle_untouched(hip, base):
    """Check 11."""
    fg = _fork(hip, base)
    before = [_getters(fg, b) for b in range(6)]
    B21, B5 = SLOT[21], SLOT[5]
    A = np.zeros((6, 11 + 3 * 85))
    A[:, 8] = 1.0
    nan_row, short = A.copy(), A[:, :73].copy()
    nan_row[B21, 73] = np.nan
    bad = [
        dict(a=A, dst=[B21, 6], src=[B21, B21]), dict(a=A, dst=[B21, -1], src=[B21, B21]), dict(a=A, dst=[SPARE, B5], src=[B21, 6]),
        dict(a=A, dst=[SPARE, SPARE], src=[B21, B5]),                      # a repeated dst
        dict(a=A, dst=[B5, B21], src=[B21, B5]),                           # a swap
        dict(a=A, dst=[B5, SPARE], src=[B21, B5]),                         # a shift through another source
        dict(a=A, dst=[SPARE], src=[B21], shift=[np.inf]), dict(a=A, dst=[SPARE], src=[B21], shift=[np.nan]),
        dict(a=A, dst=[SPARE], src=[B21], shrink=[-1e-9]), dict(a=A, dst=[SPARE], src=[B21], shrink=[1.0 + 1e-9]),
        dict(a=A, dst=[SPARE], src=[B21], shrink=[np.nan]),
        dict(a=nan_row, dst=[SPARE], src=[B21]),                           # a non-finite entry in the read part of a named source's row
        dict(a=short, dst=[SPARE], src=[B21]),                             # lda below the source's order
    ]
    for kw in bad:
        n = len(kw["dst"])
        with pytest.raises(hip.EqfError) as e:
            fg.split_filters(kw["a"], kw["dst"], kw["src"], kw.get("shift", [0.5] * n), kw.get("shrink", [0.5] * n), local=False)
        assert e.value.code == hip.ERR_INVALID, kw
    L = hip.lib()
    import ctypes as C

    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    d1, s1, one = np.array([SPARE], dtype=np.int32), np.array([B21], dtype=np.int32), np.array([0.5])
    args = lambda **k: [k.get("f", fg._h), k.get("local", 0), k.get("a", A.ctypes.data_as(dp)), A.shape[1], k.get("n", 1),  # noqa: E731
                        k.get("dst", d1.ctypes.data_as(ip)), s1.ctypes.data_as(ip), one.ctypes.data_as(dp), one.ctypes.data_as(dp),
                        k.get("gamma", None), k.get("ldg", 0), None]
    for k in (dict(local=2), dict(local=-1), dict(n=-1), dict(a=None), dict(dst=None), dict(f=None),
              dict(gamma=np.zeros(73).ctypes.data_as(dp), ldg=73)):        # ldg below the source's order
        assert L.eqf_split_filters(*args(**k)) == hip.ERR_INVALID, k
    assert L.eqf_split_filters(*args(n=0)) == 0 and L.eqf_split_filters(*args(n=0, a=None, dst=None)) == 0
    # a row with a NaN beyond the read part, or in the row of a filter that is no child's source, is fine -- checked last: it splits
    for b in range(6):
        _same(_getters(fg, b), before[b], f"filter {b} after the refused calls")
    ok = A.copy()
    ok[B5, 3] = np.nan
    ok[B21, 74:] = np.nan
    assert fg.split_filters(ok, [SPARE], [B21], [0.5], [0.5], local=False)["info"].tolist() == [0]
    assert fg.device_error() == 0
    fg.close()
    f32 = hip.FilterBatch(lc.settings(1), capacity=8, batch=2, precision=hip.PRECISION_F32)
    with pytest.raises(hip.EqfError) as e:
        f32.split_filters(np.ones((2, 11)), [1], [0], [0.5], [0.5], local=False)
    assert e.value.code == hip.ERR_UNSUPPORTED
    f32.close()


def test_children_run_on_like_restored_filters(hip, base, stream):
    """Check 12: a follow-up frame (IMU calls and a vision call) on the children gives the bits it gives on a twin restored through
    eqf_set_state from the children's getters -- eqf_copy_filters' contract."""
    fg = _fork(hip, base)
    B21 = SLOT[21]
    fg.split_filters([_depth_row(fg, B21, 4) if b == B21 else None for b in range(6)], [B21, SPARE, SLOT[0]], [B21] * 3, [0.0, 1.1, -1.1],
                     [0.5, 0.5, 0.5], local=True, report=False)
    tw = hip.FilterBatch(lc.settings(1), capacity=CAP, batch=6)
    for b in range(6):
        tw.restore_state(fg.dump_state(b), b)
    nb = [fg.num_landmarks(b) for b in range(6)]
    assert nb == [85, 21, 5, 1, 21, 21]
    for h in (fg, tw):
        _run(h, stream, FRAMES, FRAMES + 1, nb)
    for b in range(6):
        _same(_getters(fg, b), _getters(tw, b), f"filter {b} one frame on", skip=("last",))
    assert fg.device_error() == 0 and tw.device_error() == 0
    assert fg.get_time()[0] > base.get_time()[0]
    fg.close(), tw.close()
