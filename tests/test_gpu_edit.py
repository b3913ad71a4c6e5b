"""Every device route of a vision frame's landmark bookkeeping (csrc/eqf_churn.hpp: k_edit, k_compact, k_append, k_probe, k_probe_maha,
k_median_depth; csrc/eqf_capi.hip: visionOneLaunch, visionSeparate, addNewAndUpdate, resolveGate) against the exact reference of
tests/edit_exact.py: after restore_state and ONE vision call
    status 0, device_error() == 0, num_landmarks and ids equal to the reference's, in order
    origin(): pose, velocity and the kept landmarks' p bit for bit the snapshot's; ONE double depth within K_DEPTH u of the exact depth with
    every new landmark's p bit for bit fl(y depth) (initialSceneDepth itself where nothing is left)
    gate_report(): ids = the kept list, the verdicts the reference's, chords within K_CHORD u (1 + chord); empty when the gate is disarmed
    full-comparison sizes: Sigma+, gamma, delta, Gamma[0:6] inside EditCase's bound at every entry, symmetry, Gamma[6:], the bias step
    (test_gpu_update.check)
Public API only.  Frames, states and the per-route case lists: tests/edit_cases.py; the CPU file tests/test_edit_exact.py asserts the
decision margins of the same cases, measures K_DEPTH / K_CHORD from the fp64 oracle and shows eleven injected faults outside these checks.
The margins are asserted here again, on the device's own snapshot.  No constant here comes from the device.

The route is proven by the launches of profile()'s "churn" class around the call: k_edit is ONE launch; the separate launches are more
wherever the frame loses a landmark or the gate looks at one (a frame that only appends is one k_append launch: there the forcing option
debug_option("device_edit", 0) is what is relied on)."""
import numpy as np
import pytest

import edit_cases as C
import edit_exact as ex
import lie_exact as lx
import riccati_cases as rc
import update_exact as ux
from test_gpu_update import check, make_handle, read, report

pytestmark = pytest.mark.gpu

_SNAP, _REF, _BOOK = {}, {}, {}
EDIT, SEPARATE = "k_edit", "separate"


@pytest.fixture(scope="module")
def hip():
    from eqf_vio_amd import binding

    return binding


def snapshot(hip, N):
    if N not in _SNAP:
        _SNAP[N] = rc.device_snapshot(hip, max(N, 1))
    return _SNAP[N]


def reference(hip, s, fp32=False):
    """(case, S0, frame, ref, bounds) of a full-comparison spec, once per module"""
    k = C.key(s) + (fp32,)
    if k not in _REF:
        c = C.case_of(s, snapshot(hip, s["N"]))
        S0 = C.sigma_of(c, s["fam"])
        assert np.array_equal(S0, S0.T)
        e = ex.EditCase(c["snap"], C.settings(), c["stamp"], c["ids"], c["y"], c["kind"], c["thr"])
        _REF[k] = (c, S0) + e.reference(S0, fp32)
    return _REF[k]


def book_reference(s):
    """(case, S0, frame, None, None) of a bookkeeping-only spec: the group stepped at 50 digits, no Riccati blocks, no update reference"""
    k = C.key(s)
    if k not in _BOOK:
        snap, stamp, y = C.big_call(s["N"])
        c = C.make_case(snap, stamp, y, frame=s["frame"], pattern=s["pattern"], kind=s["kind"], out_at=s["out_at"])
        c = c if s["armed"] else C.disarmed(c)
        d = C.settings()
        X, _ = lx.reference_step(c["snap"], c["stamp"], d)
        xi0 = lx.State.from_dict(c["snap"]["origin"], d["cameraOffset_q"], d["cameraOffset_x"])
        _BOOK[k] = (c, c["snap"]["sigma"], ex.edit_frame(X, xi0, c["snap"]["ids"], c["ids"], c["y"], c["kind"], c["thr"], d), None, None)
    return _BOOK[k]


def label(s):
    return f"N={s['N']} {s['frame']}{'/' + s['pattern'] if s['pattern'] else ''} {'maha' if s['kind'] else 'chord'}{'' if s['armed'] else ' off'} {s['fam']}"


def churn_launches(fg):
    return fg.profile()["churn"][0]


def call(fg, cases, S0s):
    """restore every filter, set the gate, ONE vision call, read every filter (test_gpu_update.read, plus status, ids, origin and the gate
    report) and count the churn launches around the call.  (test_gpu_update.one_call asserts status 0 for every filter and has no place for
    the gate; the ragged handle's filter with the empty measurement reports EQF_SKIPPED_NO_BEARINGS.)"""
    B = len(cases)
    for b, (c, S0) in enumerate(zip(cases, S0s)):
        fg.restore_state(dict(c["snap"], sigma=S0), b)
    fg.set_outlier_gate(cases[0]["kind"], cases[0]["thr"])
    before = [fg.bias(b) for b in range(B)]
    stride = max(1, max(len(c["ids"]) for c in cases))
    ids, y = np.zeros((B, stride), dtype=np.int32), np.zeros((B, stride, 3))
    for b, c in enumerate(cases):
        ids[b, :len(c["ids"])], y[b, :len(c["ids"])] = c["ids"], c["y"]
    n0 = churn_launches(fg)
    st = fg.process_vision([c["stamp"] for c in cases], ids, y, nb=[len(c["ids"]) for c in cases])
    out = [dict(read(fg, b, before[b]), status=int(st[b]), ids=fg.ids(b), origin=fg.origin(b), report=fg.gate_report(b)) for b in range(B)]
    return out, churn_launches(fg) - n0


def judge(out, c, S0, fr, ref, bd, fam, what, worst, bad, stats):
    """every assertion of the module docstring for one filter"""
    assert fr.margin_stat >= ex.MARGIN_STAT and fr.margin_depth >= ex.MARGIN_DEPTH, (what, fr.margin_stat, fr.margin_depth)
    if out["status"] != 0:
        bad.append((what, "status", out["status"]))
    o0 = c["snap"]["origin"]
    for k in ("q", "x", "v"):
        if not np.array_equal(out["origin"][k], np.asarray(o0[k], dtype=float)):
            bad.append((what, f"origin {k} moved"))
    armed = ex.gate_armed(c["kind"], c["thr"]) and c["N"] > 0
    fails, depth = ex.bookkeeping_failures(fr, o0["p"], out["ids"], out["origin"]["p"], C.settings(), out["report"] if armed else None, c["kind"])
    bad += [(what, f) for f in fails]
    if not armed and len(out["report"]["ids"]):
        bad.append((what, "a disarmed gate reported", len(out["report"]["ids"])))
    if fails:
        return
    if depth is not None and fr.depth2 is not None:
        stats["depth"] = max(stats.get("depth", 0.0), ex.depth_ratio(depth, fr.depth))
    if armed and c["kind"] == C.CHORD:
        stats["chord"] = max(stats.get("chord", 0.0), ex.chord_ratio(out["report"]["stat"], fr.stat))
    if ref is not None:
        check(out, len(fr.ids), fam, ref, bd, what, worst, bad)


def run(hip, monkeypatch, route, specs, env=None, precision=None, book=False, expect=None, option=True):
    """Each spec in a handle of its own capacity.  expect: EDIT (one churn launch) or SEPARATE (at least one; more than one proves it)."""
    worst, bad, stats, launches = {}, [], {}, {}
    handles = {}
    try:
        for s in specs:
            c, S0, fr, ref, bd = book_reference(s) if book else reference(hip, s, precision is not None)
            if c["capacity"] not in handles:
                fg = handles[c["capacity"]] = make_handle(hip, monkeypatch, env or {}, c["capacity"], precision=precision)
                if option:
                    fg.debug_option("device_edit", 1 if expect == EDIT else 0)
                fg.profile_enable(True)
            fg = handles[c["capacity"]]
            (out,), n = call(fg, [c], [S0])
            launches[label(s)] = n
            if (expect == EDIT and n != 1) or (expect == SEPARATE and n < 1):
                bad.append((label(s), f"{n} churn launches on the route {expect}"))
            judge(out, c, S0, fr, ref, bd, s["fam"], (route, label(s)), worst, bad, stats)
            if fg.device_error() != 0:
                bad.append((label(s), "device_error", fg.device_error()))
    finally:
        for fg in handles.values():
            fg.close()
    report(route, worst)
    print(f"{route}: churn launches {launches}")
    print(f"{route}: depth worst {stats.get('depth', 0.0):.3g} u (K_DEPTH {ex.K_DEPTH:.3g}), chord worst {stats.get('chord', 0.0):.3g} u (K_CHORD {ex.K_CHORD:.3g})")
    assert not bad, bad[:10]
    return launches


def _chunks(specs, n):
    return [specs[i:i + n] for i in range(0, len(specs), n)]


# ---- k_edit ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("specs", _chunks(C.EDIT_DISARMED, 5), ids=lambda v: label(v[0]))
def test_one_launch_gate_disarmed(hip, monkeypatch, specs):
    """lose / add / all_lost+add / full at N = 5, 21, 70, every depth pattern, the empty filter"""
    run(hip, monkeypatch, "k_edit, gate disarmed", specs, expect=EDIT)


@pytest.mark.parametrize("specs", _chunks(C.EDIT_CHORD, 4), ids=lambda v: label(v[0]))
def test_one_launch_chord_gate(hip, monkeypatch, specs):
    """k_edit<double, 0>: every frame at N = 70, the deferred update (flag 2) at 59 .. 61, the ballot-word and prefix-sum edges at 63, 64, 65
    and 129 with outliers at kept index 0, 63, 64 and the last, and the median that changes when the outlier leaves"""
    run(hip, monkeypatch, "k_edit, chord gate", specs, expect=EDIT)


@pytest.mark.parametrize("specs", _chunks(C.EDIT_MAHA, 3), ids=lambda v: label(v[0]))
def test_one_launch_mahalanobis_gate(hip, monkeypatch, specs):
    run(hip, monkeypatch, "k_edit, Mahalanobis gate", specs, expect=EDIT)


@pytest.mark.parametrize("s", C.BOOK_EDIT, ids=label)
def test_one_launch_bookkeeping_at_large_sizes(hip, monkeypatch, s):
    """256 / 257: the second 256-landmark trip of k_edit's probe and of its in-place record passes (landmark 0 leaves: every record crosses
    a pass boundary); 1024 kept landmarks fill kEditMax and the LDS arrays.  ids, origin and the gate report only."""
    run(hip, monkeypatch, "k_edit, bookkeeping only", [s], book=True, expect=EDIT)


# ---- the separate launches -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("speculative", ["1", "0"])
@pytest.mark.parametrize("specs", _chunks(C.SEPARATE + C.SEPARATE_MAHA, 5), ids=lambda v: label(v[0]))
def test_separate_launches(hip, monkeypatch, specs, speculative):
    """debug_option("device_edit", 0): k_compact, k_probe / k_probe_maha, k_append, with the speculative gate (a frame with an outlier is
    redone by resolveGate when the handle is next touched) and with EQF_GATE_SPECULATIVE=0 (the host waits for the gate's answer)"""
    n = run(hip, monkeypatch, f"separate launches, EQF_GATE_SPECULATIVE={speculative}", specs, env={"EQF_GATE_SPECULATIVE": speculative}, expect=SEPARATE)
    assert all(v > 1 for k, v in n.items() if "lose" in k or "all " in k or "outlier" in k), n


def test_host_chooses_the_separate_launches_below_59_entries(hip, monkeypatch):
    """Gate armed and fewer than kEditSafeN measurement entries: no option set, the host keeps the separate launches by itself"""
    n = run(hip, monkeypatch, "gate armed at 58", C.HOST_CHOICE_58, expect=SEPARATE, option=False)
    assert all(v > 1 for v in n.values()), n


@pytest.mark.parametrize("s", C.BOOK_SEPARATE, ids=label)
def test_separate_launches_beyond_the_one_launch_limit(hip, monkeypatch, s):
    """1025 and 1040 landmarks: beyond kEditMax both settings of device_edit take k_probe + k_median_depth + k_append with depthSel; no
    option set.  Left are 1025, 1037 and 1035 landmarks, and 1040 and 1036: even counts, where the upper median differs from the lower one.
    ids, origin and the gate report only."""
    assert book_reference(s)[2].depth2 is not None   # (the frame adds landmarks behind landmarks that are left: a median is selected)
    n = run(hip, monkeypatch, "beyond kEditMax", [s], book=True, expect=SEPARATE, option=False)
    assert all(v >= 2 for v in n.values()), n   # (k_append alone is one launch: k_median_depth, and the probe in front of it, did run)


# ---- fp32 handles, a ragged handle, the partitioned filter -----------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [EDIT, SEPARATE])
def test_fp32_handles(hip, monkeypatch, route):
    """PRECISION_F32 (bounds with fp32=True; origins and depths are fp64 either way).  `all` runs under the armed chord gate wherever the route
    takes an armed frame: at N = 70 on both, at N = 17 on the separate launches only (k_edit needs 59 measurement entries)."""
    run(hip, monkeypatch, f"fp32, {route}", C.F32_EDIT if route == EDIT else C.F32_SEPARATE, precision=hip.PRECISION_F32, expect=route)


@pytest.mark.parametrize("route", [EDIT, SEPARATE])
def test_ragged_handle(hip, monkeypatch, route):
    """Four filters in one handle, chord gate armed, each against its own reference: one loses landmarks (the batch-wide hostFlip), one has
    only an outlier, one only gains landmarks.  On the separate launches the fourth gets an EMPTY measurement: by the reference's order
    (integrate, then removeOldLandmarks) it loses every landmark and reports EQF_SKIPPED_NO_BEARINGS -- pose, velocity and bias bit for bit
    the snapshot's, the 11 x 11 block that is left inside the propagate's bound.  k_edit takes an armed frame only if every filter has at
    least 59 measurement entries, so there the fourth filter is armed, quiet and gains two landmarks."""
    specs = C.RAGGED_EDIT if route == EDIT else C.RAGGED
    full = [s for s in specs if s["frame"] != "none"]
    refs = [reference(hip, s) for s in full]
    cases, S0s = [r[0] for r in refs], [r[1] for r in refs]
    if len(full) < len(specs):
        idle = C.case_of(specs[3], snapshot(hip, specs[3]["N"]))
        cases, S0s = cases + [idle], S0s + [C.sigma_of(idle, "a")]
    worst, bad, stats = {}, [], {}
    fg = make_handle(hip, monkeypatch, {}, max(c["capacity"] for c in cases), batch=4)
    try:
        fg.debug_option("device_edit", 1 if route == EDIT else 0)
        fg.profile_enable(True)
        outs, n = call(fg, cases, S0s)
        for s, out, (c, S0, fr, ref, bd) in zip(full, outs, refs):
            judge(out, c, S0, fr, ref, bd, s["fam"], (f"ragged {route}", label(s)), worst, bad, stats)
        if len(full) < len(specs):
            q, o0 = outs[3], idle["snap"]["origin"]
            e = ex.EditCase(idle["snap"], C.settings(), idle["stamp"], [], np.zeros((0, 3)), idle["kind"], idle["thr"])
            S1, E = e.propagate(S0s[3])
            r = ux.worst_ratio(q["Sp"], S1[:11, :11], ux.f64(E)[:11, :11])[0] if q["Sp"].shape == (11, 11) else np.inf
            print(f"ragged {route}: the filter with the empty measurement: status {q['status']}, base block ratio {r:.3g}")
            if (q["status"] != hip.SKIPPED_NO_BEARINGS or len(q["ids"]) or not r <= 1.0 or not np.array_equal(q["bias_after"], q["bias_before"])
                    or not all(np.array_equal(q["origin"][k], np.asarray(o0[k], dtype=float)) for k in ("q", "x", "v"))):
                bad.append(("the filter with the empty measurement", q["status"], len(q["ids"]), r))
        assert fg.device_error() == 0
        assert (n == 1) if route == EDIT else (n > 1), n
    finally:
        fg.close()
    report(f"ragged handle, {route}", worst)
    assert not bad, bad[:10]


@pytest.mark.parametrize("k", range(len(C.TILED_SPECS)), ids=lambda k: label(C.TILED_SPECS[k]))
def test_partitioned_filter(hip, k):
    """tiled.TiledFilter on a 1 x 1 grid, the IMU queue off: csrc/eqf_tiledf.hip takes the median and the gate on the host, k_tl_edit_state /
    k_tl_edit_local move the data.  The same assertions, the origin through the backend's getter and the filter's slot map."""
    from eqf_vio_amd import tiled

    s = C.TILED_SPECS[k]
    bl = dict(C.TILED)[s["N"]]
    c, S0, fr, ref, bd = reference(hip, s)
    worst, bad, stats = {}, [], {}
    be = tiled.HipBackend(dict(C.settings(), outlierThreshold=c["thr"]), capacity=c["capacity"])
    tf = tiled.TiledFilter(tiled.ProcessGrid(None, 1, 1, device=be.device), be, bl)
    try:
        tf.burst = False
        tf.initialise_from(dict(c["snap"], sigma=S0))
        before = tf.bias()
        status = tf.processVisionData(c["stamp"], c["ids"], c["y"])
        lu = tf.lastUpdate()
        o = be.origin()
        slots = tf.slot_of
        origin = dict(o, p=np.asarray(o["p"]).reshape(-1, 3)[slots] if len(slots) and slots.max() < len(o["p"]) else np.zeros((0, 3)))
        out = dict(status=int(status), ids=tf.ids, origin=origin, report=dict(ids=[]), Sp=tf.stateCovariance(), delta=lu["delta"], gamma=lu["gamma"],
                   Gamma=lu["Gamma"], bias_before=before, bias_after=tf.bias())
        # (the partitioned filter has no gate report: the verdicts show in the ids)
        judge(out, dict(c, kind=C.CHORD, thr=1e9), S0, fr, ref, bd, s["fam"], ("partitioned", label(s), bl), worst, bad, stats)
        assert be.device_error() == 0 and tf.device_error() == 0
    finally:
        tf.close()
    report(f"partitioned filter, {label(s)}, blocks of {bl}", worst)
    assert not bad, bad[:10]
