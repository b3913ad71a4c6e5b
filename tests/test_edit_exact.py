"""The frame's landmark bookkeeping of tests/edit_exact.py on the CPU, for exactly the frames tests/test_gpu_edit.py holds the device to
(tests/edit_cases.py) -- no GPU.

(a) reference consistency: the fp64 numpy oracle (oracle/eqf_numpy.py; with gate_helpers' Mahalanobis gate where the case asks for it) and,
    under the chord gate, the C++ oracle run every full-comparison case from the same restored state: final ids equal, kept p0 bit for bit
    the snapshot's, new p0 = fl(y depth) for one depth within K_DEPTH, gate report (ids, verdicts, chords within K_CHORD), and Sigma+, gamma,
    delta and Gamma[0:6] (where asserted) inside EditCase's bound at every entry.  Two exemptions, for Sigma+ of the dense gain forms only: family b
    (printed, the factor form asserted: NOTES R15.1) and the tie3 / tie_all patterns (asserted inside bound + dense_form_allowance, a derived
    term for the explicit inverse; the factor form inside the bound itself).  The lists' coverage of the named sizes, frames and patterns is
    asserted too.
(b) the decision margins of EVERY committed case, the bookkeeping-only sizes included: statistics >= 1e-3 (relative) from the threshold, the
    selected squared depth >= 1e-9 from every neighbour that is not bitwise the same landmark.
(c) K_DEPTH and K_CHORD re-measured from the numpy oracle over the committed cases: 4 x worst <= K, and the literal is not stale.
(d) the longdouble reference against the whole call at 50 digits for N <= 17.
(e) eleven injected faults in a numpy restatement of the frame at N = 21 and 70: each leaves the new checks; the table printed beside it says
    what the gates in use before (rel_fro(Sigma+) < 1e-7 against the unfaulted run, equal ids, Gamma[0:6] to 1e-8 as a stand-in for the pose)
    would have said."""
import numpy as np
import pytest

import edit_cases as C
import edit_exact as ex
import gate_helpers as G
import lie_edge_cases as ec
import lie_exact as lx
import riccati_cases as rc
import update_cases as uc
import update_exact as ux
from consistency_helpers import inject
from oracle import eqf_numpy as en
from test_update_exact import factor_form

_SNAP, _REF = {}, {}
SIGMA_TOL, POSE_TOL = 1e-7, 1e-8     # tests/test_gpu_parity.py


def snapshot(oracle_lib, N):
    if N not in _SNAP:
        _SNAP[N] = rc.oracle_snapshot(oracle_lib, max(N, 1))
    return _SNAP[N]


def reference(oracle_lib, s):
    """(case, S0, EditCase, frame, ref, bounds) of a spec, once per module"""
    k = C.key(s)
    if k not in _REF:
        c = C.case_of(s, snapshot(oracle_lib, s["N"]))
        S0 = C.sigma_of(c, s["fam"])
        assert np.array_equal(S0, S0.T)
        e = ex.EditCase(c["snap"], C.settings(), c["stamp"], c["ids"], c["y"], c["kind"], c["thr"])
        _REF[k] = (c, S0, e) + e.reference(S0)
    return _REF[k]


def numpy_run(c, S0):
    d = dict(C.settings(), outlierThreshold=c["thr"] if c["kind"] == C.CHORD else 1e9)
    fo = G.chord_filter(d) if c["kind"] == C.CHORD else G.mahalanobis_filter(d, c["thr"])
    inject(fo, dict(c["snap"], sigma=S0))
    fo.processVisionData(c["stamp"], c["ids"], c["y"])
    return fo


def _label(s):
    return f"N={s['N']} {s['frame']}{'/' + s['pattern'] if s['pattern'] else ''} {'maha' if s['kind'] else 'chord'}{'' if s['armed'] else ' off'} {s['fam']}"


FULL = C.unique([s for s in C.FULL_SPECS if s["frame"] != "none"])


# ---- (a) ------------------------------------------------------------------------------------------------------------------------------------
def dense_form_allowance(ref):
    """What an explicit inverse adds to the error of Sigma+ = Sigma' - (Sigma' C^T) inv(S) (C Sigma'), the form of both oracles, entrywise and
    first order: the inverse X from a factorisation has |dX| <= gamma_3m |X| |L||L^T| |X| [Higham, Accuracy and Stability, section 14.1], the
    two products add gamma_{2m+1} |B^T||X||B|.  Unlike the bound of update_exact.py it does not shrink where Sigma+ cancels."""
    L = ref["L"]
    m = len(L)
    X = ux.f64(ux.solve_upper_t(L, ux.solve_lower(L, np.eye(m, dtype=ux.LD))))
    aX, aB, aL = np.abs(X), np.abs(ux.f64(ref["B"])), np.abs(ux.f64(L))
    return ux.gamma(3 * m) * (aB.T @ (aX @ (aL @ aL.T) @ aX) @ aB) + ux.gamma(2 * m + 1) * (aB.T @ aX @ aB)


@pytest.mark.parametrize("s", FULL, ids=_label)
def test_oracles_agree_with_the_reference(oracle_lib, s):
    """Both oracles on every full-comparison case.  Bookkeeping: always.  The update: inside the bound of update_exact.py, but
      family b           the dense gain form is printed, the factor form asserted (test_update_exact.py does the same: NOTES R15.1)
      tie3 / tie_all     tied landmarks leave cross terms of Sigma+ that cancel from O(10) to O(1e-4), where the explicit inverse's error does not
                         shrink with them: the dense Sigma+ of either oracle goes from 0.15 to 3 times the bound with LAPACK's blocking and thread
                         count (N = 50: 0.59 on one thread, 3.07 on eight; the C++ oracle 1.69).  There Sigma+ of the dense forms is asserted
                         inside bound + dense_form_allowance, everything else inside the bound, and the factor form inside the bound itself."""
    c, S0, e, fr, ref, bd = reference(oracle_lib, s)
    armed = ex.gate_armed(c["kind"], c["thr"])
    tied, graded = s["pattern"] in ("tie3", "tie_all"), s["fam"] == "b"
    bd_dense = dict(bd, Sp=bd["Sp"] + dense_form_allowance(ref)) if tied else bd
    asserted = uc.gamma6_asserted(len(fr.ids), s["fam"])
    fo = numpy_run(c, S0)
    bad, depth = ex.bookkeeping_failures(fr, c["snap"]["origin"]["p"], fo.X.ids, fo.xi0.p, C.settings(), fo.report if armed and s["N"] else None, c["kind"])
    got = dict(Sp=fo.Sigma, gamma=fo.last["gamma"], delta=fo.last["delta"], Gamma6=fo.last["Gamma"][0:6])
    plain = {k: ux.worst_ratio(got[k], ref[k], bd[k])[0] for k in got}
    r = {k: ux.worst_ratio(got[k], ref[k], bd_dense[k])[0] for k in got}
    r["symmetry"] = ux.symmetry_ratio(got["Sp"], bd_dense["Sp"])
    if not asserted:
        r.pop("Gamma6")
    print(f"{_label(s)}: numpy oracle, ratio to the bound " + " ".join(f"{k} {v:.3g}" for k, v in r.items())
          + (f"  (Sp to the plain bound {plain['Sp']:.3g})" if tied else "")
          + (f"  depth {ex.depth_ratio(depth, fr.depth):.3g} u" if depth is not None and fr.depth2 is not None else "")
          + (f"  chord {ex.chord_ratio(fo.report['stat'], fr.stat):.3g} u" if armed and c["kind"] == C.CHORD and s["N"] else ""))
    assert not bad, bad
    if not graded:
        assert all(v <= 1.0 for v in r.values()), r
    if tied or graded:
        ff = numpy_frame(c, S0)
        rf = {k: ux.worst_ratio(ff[k], ref[k], bd[k])[0] for k in ("Sp", "gamma", "delta") + (("Gamma6",) if asserted else ())}
        print("    factor form " + " ".join(f"{k} {v:.3g}" for k, v in rf.items()))
        assert all(v <= 1.0 for v in rf.values()), rf
    if c["kind"] == C.CHORD:   # the C++ oracle has the chord gate only
        f = oracle_lib.OracleFilter(dict(C.settings(), outlierThreshold=c["thr"]))
        f.set_state(dict(c["snap"], sigma=S0))
        f.processVisionData(c["stamp"], c["ids"], c["y"])
        badc, _ = ex.bookkeeping_failures(fr, c["snap"]["origin"]["p"], f.ids(), f.xi0()["p"], C.settings())
        assert not badc, badc
        rc_ = ux.worst_ratio(f.stateCovariance(), ref["Sp"], bd_dense["Sp"])[0]
        print(f"    C++ oracle Sp {rc_:.3g}" + (f"  (to the plain bound {ux.worst_ratio(f.stateCovariance(), ref['Sp'], bd['Sp'])[0]:.3g})" if tied else ""))
        assert graded or rc_ <= 1.0


def test_every_size_frame_and_pattern_is_in_a_route():
    """The coverage the case lists claim, asserted: every full-comparison and bookkeeping-only size, every frame on k_edit (armed, but the two
    frames an armed k_edit cannot take) and on the separate launches, every depth pattern, the Mahalanobis product, and beyond kEditMax an
    even and an odd number of landmarks left in front of k_median_depth."""
    assert set(C.FULL_SIZES) <= {s["N"] for s in C.FULL_SPECS}
    assert set(C.BOOK_SIZES) == {s["N"] for s in C.BOOK_EDIT + C.BOOK_SEPARATE}
    frames = lambda specs: {s["frame"] for s in specs if s["pattern"] is None}   # noqa: E731
    assert frames(C.EDIT_CHORD) | {"all_lost+add", "empty+add"} == set(C.FRAMES)
    assert {"lose", "add", "all_lost+add", "full", "empty+add"} <= frames(C.EDIT_DISARMED)
    assert frames(C.SEPARATE) | {"outlier"} >= set(C.FRAMES) and "outlier" in frames(C.HOST_CHOICE_58)
    assert {s["pattern"] for s in C.EDIT_DISARMED + C.EDIT_CHORD} >= set(C.PATTERNS)
    assert {(s["N"], s["frame"]) for s in C.EDIT_MAHA} == {(N, fr) for N in (64, 65, 70) for fr in ("outlier", "outlier+add", "all")}
    even = [book_frame(s)[1] for s in C.BOOK_SEPARATE[-2:]]
    assert all(s["N"] > 1024 for s in C.BOOK_SEPARATE) and all(fr.depth2 is not None and len(fr.d2_left) % 2 == 0 for fr in even)
    assert [len(fr.d2_left) for fr in even] == [1040, 1036]


# ---- (b) ------------------------------------------------------------------------------------------------------------------------------------
def _margins(fr, what, low):
    print(f"{what}: margins  statistic {fr.margin_stat:.3g}  depth {fr.margin_depth:.3g}")
    if not fr.margin_stat >= ex.MARGIN_STAT or not fr.margin_depth >= ex.MARGIN_DEPTH:
        low.append((what, fr.margin_stat, fr.margin_depth))


def test_decision_margins_of_the_full_cases(oracle_lib):
    low = []
    for s in FULL:
        _margins(reference(oracle_lib, s)[3], _label(s), low)
    assert not low, low


def book_frame(s):
    """(case, Frame) of a bookkeeping-only spec: the group stepped at 50 digits, no Riccati blocks, no update"""
    snap, stamp, y = C.big_call(s["N"])
    c = C.make_case(snap, stamp, y, frame=s["frame"], pattern=s["pattern"], kind=s["kind"], out_at=s["out_at"])
    c = c if s["armed"] else C.disarmed(c)
    d = C.settings()
    X, _ = lx.reference_step(c["snap"], c["stamp"], d)
    xi0 = lx.State.from_dict(c["snap"]["origin"], d["cameraOffset_q"], d["cameraOffset_x"])
    return c, ex.edit_frame(X, xi0, c["snap"]["ids"], c["ids"], c["y"], c["kind"], c["thr"], d)


@pytest.mark.parametrize("s", C.unique(C.BOOK_EDIT + C.BOOK_SEPARATE), ids=_label)
def test_decision_margins_of_the_bookkeeping_only_cases(s):
    c, fr = book_frame(s)
    low = []
    _margins(fr, _label(s), low)
    assert not low, low
    if s["N"] > 300:   # (the dense numpy oracle needs 15 s for a 3131 x 3131 frame; the 50-digit step above takes one)
        return
    fo = numpy_run(c, c["snap"]["sigma"])
    bad, depth = ex.bookkeeping_failures(fr, c["snap"]["origin"]["p"], fo.X.ids, fo.xi0.p, C.settings(), fo.report if s["armed"] else None, c["kind"])
    assert not bad, bad


# ---- (c) ------------------------------------------------------------------------------------------------------------------------------------
def test_k_depth_and_k_chord_are_four_times_the_oracles_measured_ratios(oracle_lib):
    wd, wc = (0.0, None), (0.0, None)
    for s in FULL:
        c, S0, e, fr, ref, bd = reference(oracle_lib, s)
        fo = numpy_run(c, S0)
        nn = sum(1 for o in fr.src if o < 0)
        if nn and fr.depth2 is not None:
            depth = ex.find_depth(fo.xi0.p[-nn:], fr.y[-nn:], fr.depth, 64.0)
            assert depth is not None, _label(s)
            wd = max(wd, (ex.depth_ratio(depth, fr.depth), _label(s)))
        if c["kind"] == C.CHORD and ex.gate_armed(c["kind"], c["thr"]) and s["N"]:
            wc = max(wc, (ex.chord_ratio(fo.report["stat"], fr.stat), _label(s)))
    print(f"numpy oracle against 50 digits: depth worst {wd[0]!r} u at {wd[1]}, K_DEPTH = {ex.K_DEPTH!r}; chord worst {wc[0]!r} u (1 + chord) at {wc[1]}, "
          f"K_CHORD = {ex.K_CHORD!r}")
    assert 4.0 * wd[0] <= ex.K_DEPTH and ex.K_DEPTH == 4.0 * ex.K_DEPTH_MEASURED
    assert 4.0 * wc[0] <= ex.K_CHORD and ex.K_CHORD == 4.0 * ex.K_CHORD_MEASURED
    assert wd[0] >= 0.5 * ex.K_DEPTH_MEASURED and wc[0] >= 0.5 * ex.K_CHORD_MEASURED, "a measured K is stale: renew it from the figures above"


# ---- (d) ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [s for s in FULL if s["N"] <= ux.MP_MAX_N - 2 and s["fam"] != "b"], ids=_label)
def test_longdouble_reference_against_fifty_digits(oracle_lib, s):
    c, S0, e, fr, ref, bd = reference(oracle_lib, s)
    fr2, mp_ref = e.reference_mp(S0)
    assert fr2.ids == fr.ids
    worst = {}
    for k in ("Sp", "gamma", "delta", "Gamma6"):
        if k == "Gamma6" and not uc.gamma6_asserted(len(fr.ids), s["fam"]):
            continue
        worst[k] = ux.worst_ratio(ref[k], mp_ref[k], bd[k])[0]
    print(f"{_label(s)}: longdouble against 50 digits, ratio to the bound " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert all(v <= 0.01 for v in worst.values()), worst


# ---- (e) ------------------------------------------------------------------------------------------------------------------------------------
def inputs_from_filter(f, y, r):
    """What an fp64 implementation holds in front of its update (Sigma' and the geometry), from a numpy oracle filter whose landmark set is
    final; the form test_update_exact.factor_form takes"""
    N = len(f.xi0.ids)
    delta = en.output_coordinate_chart(en.output_group_action(f.X.inverse(), y), en.measure_system_state(f.xi0))
    C0 = en.eqf_output_matrix_C(f.xi0)
    xiHat = en.state_group_action(f.X, f.xi0)
    eta0 = en.project_to_manifold(f.xi0).gravityDir
    eta0 = eta0 / np.linalg.norm(eta0)
    RCt = en.quat_to_matrix(en.quat_inverse(en.quat_mul(xiHat.pose.q, xiHat.cameraOffset.q)))
    AdP0 = f.xi0.pose.adjoint()
    PC = xiHat.pose * xiHat.cameraOffset
    ZP = np.zeros((5 + 3 * N, 6))
    for i in range(N):
        pm = np.zeros((3, 6))
        pm[:, 0:3], pm[:, 3:6] = -en.skew(PC.apply(xiHat.p[i])), np.eye(3)
        ZP[5 + 3 * i:8 + 3 * i] = f.X.Q[i].as_matrix3() @ RCt @ pm @ AdP0
    Kpar = np.zeros((6, 4))
    Kpar[0:3, 0], Kpar[3:6, 1:4] = eta0, np.eye(3)
    Pd = -(np.eye(3) - np.outer(eta0, eta0)) @ en.skew(eta0) @ en.stereo_sphere_chart_inv_diff(np.zeros(2), eta0)
    return dict(N=N, S1=f.Sigma.copy(), delta=np.asarray(delta).reshape(-1), C0=np.array([C0[2 * i:2 * i + 2, 5 + 3 * i:8 + 3 * i] for i in range(N)]),
                ZP=ZP, Kpar=Kpar, Pd=Pd, r=r)


FAULTS = {  # name: the frame it is injected into (it needs an even nF, a tie, an outlier next to the median ...)
    "median_lower_for_even_nF": dict(frame="all", even=True), "median_before_the_gate": dict(pattern="tie_after_gate"),
    "median_of_the_old_estimate": dict(frame="all"), "tie_break_dropped": dict(pattern="tie3", armed=False),
    "bearing_at_state_index": dict(frame="all"), "outlier_re_added": dict(frame="outlier+add"), "record_from_next_index": dict(frame="lose"),
    "sigma_rows_only": dict(frame="lose"), "point_variance_missing": dict(frame="add"), "cross_term_1e-9": dict(frame="add"),
    "lmc_at_old_slot": dict(frame="lose")}


def numpy_frame(c, S0, fault=None):
    """The frame restated in plain numpy on the numpy oracle's stepped state, with one of FAULTS; then the update in the factor form.
    Returns dict(ids, p, Sp, gamma, delta, Gamma6) (the update's entries None where the fault leaves nothing to factor)."""
    d = C.settings()
    f = ec.numpy_filter(en, dict(c["snap"], sigma=S0), d)
    old_p = f.stateEstimate().p.reshape(-1, 3).copy()
    assert f.integrateUpToTime(c["stamp"])
    sid = [int(i) for i in f.X.ids]
    mid = [int(i) for i in c["ids"]]
    where = {i: k for k, i in enumerate(mid)}
    est = f.stateEstimate().p.reshape(-1, 3)
    yhat = est / np.linalg.norm(est, axis=1, keepdims=True)
    kept = [o for o, i in enumerate(sid) if i in where]
    armed = ex.gate_armed(c["kind"], c["thr"])
    out = [o for o in kept if armed and np.linalg.norm(c["y"][where[sid[o]]] - yhat[o]) > c["thr"]]
    left = [o for o in kept if o not in out]
    gone = set() if fault == "outlier_re_added" else {sid[o] for o in out}
    new = [k for k, i in enumerate(mid) if i not in {sid[o] for o in left} and i not in gone]
    pool = {"median_before_the_gate": kept}.get(fault, left)
    d2 = np.sort(np.sum((old_p if fault == "median_of_the_old_estimate" else est)[pool] ** 2, axis=1))
    nF = len(pool)
    depth = d["initialSceneDepth"] if nF == 0 else np.sqrt(d2[(nF - 1) // 2 if fault == "median_lower_for_even_nF" else nF // 2])
    if fault == "tie_break_dropped":   # with equal depths at the selected rank no thread selects: the depth stays what the memory held
        depth = 0.0
    meas = [where[sid[o]] for o in left] + new
    src = list(left)
    if fault == "record_from_next_index":
        src[len(src) // 2] = left[len(src) // 2] + 1
    ynew = np.array([c["y"][len(left) + j] if fault == "bearing_at_state_index" else c["y"][k] for j, k in enumerate(new)]).reshape(-1, 3)
    p = np.vstack([f.xi0.p.reshape(-1, 3)[src], ynew * depth])
    ids = [sid[o] for o in left] + [mid[k] for k in new]
    idx = np.array(list(range(11)) + [11 + 3 * o + k for o in left for k in range(3)])
    n_old, n = len(idx), len(idx) + 3 * len(new)
    S = np.zeros((n, n))
    S[:n_old, :n_old] = f.Sigma[np.ix_(idx, idx)]
    if fault == "sigma_rows_only":      # the columns of one moved landmark still hold what was there before the compaction
        j = 11 + 3 * (len(left) // 2)
        S[:n_old, j:j + 3] = f.Sigma[idx, j:j + 3]
    S[range(n_old, n), range(n_old, n)] = d["initialPointVariance"]
    if fault == "point_variance_missing":
        S[n_old + 1, n_old + 1] = 0.0
    if fault == "cross_term_1e-9":
        S[n_old, 12] = S[12, n_old] = 1e-9
    res = dict(ids=ids, p=p, depth=depth, Sp=None)
    if not np.all(np.isfinite(p)) or np.any(np.sum(p * p, axis=1) == 0):
        return res
    g = f
    g.xi0.p, g.xi0.ids, g.X.ids = p.copy(), np.array(ids), np.array(ids)
    g.X.Q = [f.X.Q[o] for o in left] + [en.SOT3() for _ in new]
    g.Sigma = S
    inp = inputs_from_filter(g, c["y"][meas], d["measurementVariance"])
    if fault == "lmc_at_old_slot":      # the constants of a moved landmark were not moved with it: C0 from the neighbour's p0
        j = len(left) // 2
        inp["C0"][j] = inp["C0"][j - 1]
    try:
        res.update(factor_form(inp))
    except np.linalg.LinAlgError:
        pass
    return res


@pytest.mark.parametrize("N", [21, 70])
def test_injected_faults_leave_the_new_checks(oracle_lib, N):
    missed, lines = [], []
    for name, how in FAULTS.items():
        out_at = None
        if how.get("even") and (N - 3 - 2) % 2:
            out_at = [1, N // 3, N - 3]
        s = C.spec(N, how.get("frame", "add"), how.get("pattern"), armed=how.get("armed", True), fam="a", out_at=out_at)
        c, S0, e, fr, ref, bd = reference(oracle_lib, s)
        assert fr.margin_stat >= ex.MARGIN_STAT and fr.margin_depth >= ex.MARGIN_DEPTH
        ok, got = numpy_frame(c, S0), numpy_frame(c, S0, name)
        verdicts = []
        for run in (ok, got):
            bad, _ = ex.bookkeeping_failures(fr, c["snap"]["origin"]["p"], run["ids"], run["p"], C.settings())
            r = {}
            if not bad and run["Sp"] is not None:
                r = {k: ux.worst_ratio(run[k], ref[k], bd[k])[0] for k in ("Sp", "gamma", "delta", "Gamma6")}
                r["symmetry"] = ux.symmetry_ratio(run["Sp"], bd["Sp"])
            elif not bad:
                bad = ["the update cannot be factored"]
            verdicts.append((bad, r))
        assert not verdicts[0][0] and all(v <= 1.0 for v in verdicts[0][1].values()), (name, verdicts[0])
        bad, r = verdicts[1]
        caught = bool(bad) or any(not v <= 1.0 for v in r.values())
        # what the gates in use before this file would have said: equal ids, rel_fro(Sigma+), Gamma[0:6] (the pose moves by it)
        same_ids = got["ids"] == ok["ids"]
        if same_ids and got["Sp"] is not None:
            fro = float(np.linalg.norm(got["Sp"] - ok["Sp"]) / np.linalg.norm(ok["Sp"]))
            dG = float(np.abs(got["Gamma6"] - ok["Gamma6"]).max())
            old = "PASSES the old gates" if fro < SIGMA_TOL and dG < POSE_TOL else "caught by the old gates"
            old = f"rel_fro {fro:.2e} Gamma6 {dG:.2e} -> {old}"
        else:
            old = "caught by the old gates (ids)" if not same_ids else "no finite update: caught by the old gates"
        lines.append(f"N = {N} {name:28s} new checks: {(bad[0][:60] if bad else ' '.join(f'{k} {v:.3g}' for k, v in r.items()))} | before: {old}")
        if not caught:
            missed.append((name, r))
    print("\n".join(lines))
    assert not missed, missed
