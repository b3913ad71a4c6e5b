"""TEST INFRASTRUCTURE ONLY -- the landmark bookkeeping of one vision frame, exactly, and the vision call that contains it.

After integrateUpToTime a frame (ref: src/VIOFilter.cpp:345-443, the order of processVisionData) does
    removeOldLandmarks   state ids that are absent from the measurement leave
    removeOutliers       for every landmark left, with qHat_i = Q_i^-1 p0_i from lie_exact.state_group_action at 50 digits,
                           kind 0 (chord)        |y_i - qHat_i / |qHat_i||  >  threshold
                           kind 1 (Mahalanobis)  d2_i = delta_i^T (C_i Sigma'_ii C_i^T + r I)^-1 delta_i  >  threshold, from the longdouble Sigma'
                                                 and update_exact's delta_i and C0_i (lie_exact.residual / landmark_constants)
                         the landmark leaves TOGETHER WITH its measurement entry: it does not come back as a new landmark of this frame
    addNewLandmarks      the measurement entries without a landmark are appended in measurement order at
                           depth = sqrt(the order statistic nF // 2 (zero based, ascending) of |qHat_i|^2 over WHAT IS LEFT), nF their number,
                           depth = initialSceneDepth when nothing is left,
                         p0 = y depth, Q = identity, Sigma: zero cross terms, initialPointVariance on the new diagonal
All of it is discrete decisions, data movement, one order statistic and one product, so the reference is exact but for the two places a
rounding can decide: a statistic next to its threshold and two squared depths next to each other.  edit_frame returns the case's two
DECISION MARGINS for that reason -- the smallest relative distance of a statistic from the threshold, and the relative gap between the
selected squared depth and its nearest neighbour that is not bitwise the same landmark -- and tests/test_edit_exact.py asserts them
(>= 1e-3 and >= 1e-9) for every committed case.

EditCase is update_exact.Case with this step between the propagate and update_exact.Geometry: Sigma' and the propagate's bound E_ric are
taken through the index list (deleted rows and columns leave; a new landmark's block is initialPointVariance I with error 0), and
update_reference / update_bounds run on the result as they are.  No formula of update_exact.py changes.

The two constants follow the project's convention (K = 4 x what the fp64 numpy oracle shows against the 50-digit value over the committed
cases; tests/test_edit_exact.py re-measures both and asserts 4 x ratio <= K; neither comes from the device):
    K_DEPTH   |depth_fp64 - depth_exact| <= K_DEPTH u depth_exact
    K_CHORD   |chord_fp64 - chord_exact| <= K_CHORD u (1 + chord)"""
import numpy as np
from mpmath import mp, mpf

import lie_exact as lx
import riccati_exact as rx
import update_exact as ux

LD = rx.LD
U64 = rx.U64
CHORD, MAHA = 0, 1
K_DEPTH_MEASURED = 2.5715684902808325   # the numpy oracle's worst |depth - depth_exact| / (u depth_exact)        (test_edit_exact.py re-measures both;
K_CHORD_MEASURED = 2.34730751411376     # the numpy oracle's worst |chord - chord_exact| / (u (1 + chord_exact))     worst at N = 58 and N = 63)
K_DEPTH = 4.0 * K_DEPTH_MEASURED
K_CHORD = 4.0 * K_CHORD_MEASURED
MARGIN_STAT = 1e-3
MARGIN_DEPTH = 1e-9


def gate_armed(kind, thr):
    """A chord between unit vectors never exceeds 2: such a chord gate cannot trip and examines nothing; neither does an infinite d2 gate."""
    return thr is not None and np.isfinite(thr) and (kind == MAHA or thr < 2.0)


class Frame:
    """What edit_frame returns.
    ids        final ids in state order                      kept_ids   the ids the gate looked at (after removeOldLandmarks), state order
    stat       the gate's number per kept landmark (mpf)      removed    its verdict per kept landmark (bool array)
    src        per final landmark its index in the state BEFORE the frame, -1 for a new landmark
    meas       per final landmark its index in the measurement (the permutation)
    y          the bearings in final state order (N_final, 3)
    depth      the exact depth of the new landmarks (mpf; None when the frame adds nothing)      depth2, depth_rank: the selected |qHat|^2
    d2_left    |qHat_i|^2 of what is left (mpf), in state order
    X, xi0     the edited lie_exact.Group / State           index      rows of the edited Sigma' in the old one, -1 for new rows
    margin_stat, margin_depth   the decision margins (inf where there is no decision)"""


def edit_frame(X, xi0, state_ids, meas_ids, y, kind, thr, d, S1=None):
    """X, xi0: the stepped lie_exact.Group / State; S1: the longdouble Sigma' (kind 1 only)."""
    state_ids = [int(i) for i in state_ids]
    meas_ids = [int(i) for i in meas_ids]
    assert all(a < b for a, b in zip(meas_ids, meas_ids[1:])), "ids strictly ascending"
    y = np.asarray(y, dtype=float).reshape(len(meas_ids), 3)
    where = {i: k for k, i in enumerate(meas_ids)}
    est = lx.state_group_action(X, xi0)
    # removeOldLandmarks
    kept = [o for o, i in enumerate(state_ids) if i in where]
    fr = Frame()
    fr.kept_ids = [state_ids[o] for o in kept]
    # removeOutliers
    fr.stat, removed = [], []
    if gate_armed(kind, thr):
        t = mpf(float(thr))
        for o in kept:
            yi = lx.vec(y[where[state_ids[o]]])
            if kind == CHORD:
                s = lx.norm(lx.sub(yi, lx.unit(est.p[o])))
            else:
                delta = lx.residual(y[where[state_ids[o]]], X.Q[o][0], xi0.p[o])
                C = lx.landmark_constants([float(v) for v in xi0.p[o]])[0]
                Sii = [[mpf(float(v)) + mpf(float(v - LD(float(v)))) for v in row] for row in S1[11 + 3 * o:14 + 3 * o, 11 + 3 * o:14 + 3 * o]]
                M = lx.mm(lx.mm(C, Sii), lx.tr(C))
                r = mpf(float(d["measurementVariance"]))
                a, b, c, e = M[0][0] + r, M[0][1], M[1][0], M[1][1] + r
                det = a * e - b * c
                s = (delta[0] * (e * delta[0] - b * delta[1]) + delta[1] * (a * delta[1] - c * delta[0])) / det
            fr.stat.append(s)
            removed.append(bool(s > t))
        fr.margin_stat = min([float(abs(s - t) / t) for s in fr.stat], default=np.inf)
    else:
        removed = [False] * len(kept)
        fr.margin_stat = np.inf
    fr.removed = np.array(removed if fr.stat else [], dtype=bool)
    left = [o for o, rm in zip(kept, removed) if not rm]
    gone = {state_ids[o] for o, rm in zip(kept, removed) if rm}
    # addNewLandmarks
    have = {state_ids[o] for o in left}
    new = [k for k, i in enumerate(meas_ids) if i not in have and i not in gone]
    fr.d2_left = [lx.dot(est.p[o], est.p[o]) for o in left]
    fr.depth = fr.depth2 = fr.depth_rank = None
    fr.margin_depth = np.inf
    if new:
        if left:
            order = sorted(range(len(left)), key=lambda j: fr.d2_left[j])
            sel = order[len(left) // 2]
            fr.depth_rank, fr.depth2 = sel, fr.d2_left[sel]
            fr.depth = mp.sqrt(fr.depth2)
            same = _record(X, xi0, left[sel])
            gaps = [abs(fr.d2_left[j] - fr.depth2) / fr.depth2 for j in range(len(left)) if _record(X, xi0, left[j]) != same]
            fr.margin_depth = float(min(gaps)) if gaps else np.inf
        else:
            fr.depth = mpf(float(d["initialSceneDepth"]))
    fr.src = left + [-1] * len(new)
    fr.meas = [where[state_ids[o]] for o in left] + new
    fr.ids = [state_ids[o] for o in left] + [meas_ids[k] for k in new]
    fr.y = y[fr.meas].reshape(len(fr.meas), 3)
    newp = [[mpf(float(v)) * fr.depth for v in y[k]] for k in new]
    fr.xi0 = lx.State(xi0.R, xi0.x, xi0.v, [xi0.p[o] for o in left] + newp, xi0.camR, xi0.camx)
    fr.X = lx.Group(X.AR, X.Ax, X.w, [X.Q[o] for o in left] + [(lx.eye(), mpf(1)) for _ in new])
    fr.index = list(range(11)) + [11 + 3 * o + c if o >= 0 else -1 for o in fr.src for c in range(3)]
    return fr


def _record(X, xi0, o):
    """The landmark's record as the filter holds it: p0 and Q (two landmarks with the same record have the same depth in every arithmetic)."""
    return (tuple(xi0.p[o]), tuple(tuple(r) for r in X.Q[o][0]), X.Q[o][1])


def edit_matrix(S, index, diag):
    """S taken through the index list: rows / columns of index -1 are new -- zero off the diagonal, `diag` on it."""
    idx = np.asarray(index)
    old = idx >= 0
    out = np.zeros((len(idx), len(idx)), dtype=S.dtype)
    out[np.ix_(old, old)] = S[np.ix_(idx[old], idx[old])]
    out[~old, ~old] = diag
    return out


class EditCase:
    """The reference of one vision call from a snapshot: integrate to `stamp`, the frame's bookkeeping under the gate (kind, thr), the update."""

    def __init__(self, snap, d, stamp, meas_ids, y, kind=CHORD, thr=None):
        f = rx.ExactFilter(snap, d)
        step = f.process_imu(stamp, np.zeros(3), np.zeros(3))
        assert step is not None or len(snap["ids"]) == 0, "the vision call must integrate"
        self.steps = [step] if step is not None else []
        self.d, self.kind, self.thr = d, kind, thr
        self.X1, self.xi01 = f.X, f.xi0
        self.state_ids, self.meas_ids, self.y_meas = list(snap["ids"]), list(meas_ids), np.asarray(y, dtype=float)
        self.r = float(d["measurementVariance"])
        self._frame = None
        if kind == CHORD or not gate_armed(kind, thr):
            self._frame = edit_frame(f.X, f.xi0, self.state_ids, self.meas_ids, self.y_meas, kind, thr, d)

    def frame(self, S1=None):
        """The Frame; under the Mahalanobis gate it depends on Sigma' (longdouble)."""
        if self._frame is not None:
            return self._frame
        return edit_frame(self.X1, self.xi01, self.state_ids, self.meas_ids, self.y_meas, self.kind, self.thr, self.d, S1)

    def propagate(self, S0, fp32=False):
        return rx.reference_run(self.steps, S0, fp32)

    def reference(self, S0, fp32=False):
        """(frame, ref, bounds): update_reference / update_bounds on the edited Sigma' and the edited E_ric"""
        S1, E = self.propagate(S0, fp32)
        fr = self.frame(S1)
        S1e = edit_matrix(S1, fr.index, LD(float(self.d["initialPointVariance"])))
        Ee = edit_matrix(np.asarray(E).astype(LD), fr.index, LD(0))
        geo = ux.Geometry(fr.X, fr.xi0, fr.y)
        ref = ux.update_reference(S1e, geo, self.r)
        return fr, ref, ux.update_bounds(ref, Ee, fp32)

    def reference_mp(self, S0):
        """The same in mpmath at 50 digits (N <= update_exact.MP_MAX_N before and after the frame)"""
        assert len(self.state_ids) <= ux.MP_MAX_N
        S1 = ux.propagate_mp(self.steps, S0)
        fr = self.frame(ux.to_ld(S1))
        assert len(fr.ids) <= ux.MP_MAX_N
        idx = np.asarray(fr.index)
        S1e = np.array([[mpf(0)] * len(idx) for _ in idx], dtype=object)
        for a, ia in enumerate(idx):
            for b, ib in enumerate(idx):
                if ia >= 0 and ib >= 0:
                    S1e[a, b] = S1[ia, ib]
                elif a == b:
                    S1e[a, b] = mpf(float(self.d["initialPointVariance"]))
        return fr, ux.update_reference(S1e, ux.Geometry(fr.X, fr.xi0, fr.y), self.r, use_mp=True)


def depth_candidates(depth_exact, k=None):
    """The doubles within K_DEPTH u (relative) of the exact depth, nearest first"""
    k = K_DEPTH if k is None else k
    c = float(depth_exact)
    tol = mpf(k) * mpf(U64) * depth_exact
    out, lo, hi = [c], c, c
    while True:
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        grew = False
        for v in (lo, hi):
            if abs(mpf(float(v)) - depth_exact) <= tol:
                out.append(float(v))
                grew = True
        if not grew:
            break
    return [v for v in out if abs(mpf(v) - depth_exact) <= tol]


def find_depth(p_new, y_new, depth_exact, k=None):
    """The ONE double depth within k u (relative) of the exact depth with p_new bit for bit fl(y depth) for every new landmark, or None"""
    p_new, y_new = np.asarray(p_new, dtype=float).reshape(-1, 3), np.asarray(y_new, dtype=float).reshape(-1, 3)
    for c in depth_candidates(depth_exact, k):
        if np.array_equal(y_new * c, p_new):
            return c
    return None


def bookkeeping_failures(fr, p_before, ids, p, d, report=None, kind=CHORD, k_depth=None, k_chord=None):
    """What of the frame's bookkeeping a filter got wrong (a list of strings, empty when all is right), and the depth it used.
    ids, p: the filter's ids and origin landmarks after the call; p_before: the snapshot's origin landmarks; report: its gate report
    (dict ids / stat / removed) where the gate was armed."""
    bad = []
    p, p_before = np.asarray(p, dtype=float).reshape(-1, 3), np.asarray(p_before, dtype=float).reshape(-1, 3)
    if [int(i) for i in ids] != fr.ids or len(p) != len(fr.ids):
        return [f"ids {[int(i) for i in ids][:8]} .. against {fr.ids[:8]} .. ({len(ids)} / {len(fr.ids)})"], None
    old = [f for f, o in enumerate(fr.src) if o >= 0]
    new = [f for f, o in enumerate(fr.src) if o < 0]
    moved = [f for f in old if not np.array_equal(p[f], p_before[fr.src[f]])]
    if moved:
        bad.append(f"kept landmarks {moved[:8]} are not bit for bit the snapshot's")
    depth = None
    if new:
        exact = fr.depth
        if fr.depth2 is None:   # nothing was left: initialSceneDepth itself, exactly
            depth = float(d["initialSceneDepth"])
            if not np.array_equal(fr.y[new] * depth, p[new]):
                bad.append(f"new landmarks are not fl(y initialSceneDepth): {p[new][:2]}")
        else:
            depth = find_depth(p[new], fr.y[new], exact, k_depth)
            if depth is None:
                with np.errstate(all="ignore"):
                    guess = np.linalg.norm(p[new], axis=1)
                bad.append(f"no one depth within K_DEPTH u of {float(exact)!r} gives the new landmarks bit for bit; |p_new| = {guess[:4]}")
    if report is not None:
        if [int(i) for i in report["ids"]] != fr.kept_ids:
            bad.append(f"gate report ids {list(report['ids'])[:8]} against {fr.kept_ids[:8]}")
        elif not np.array_equal(np.asarray(report["removed"], dtype=bool), fr.removed):
            bad.append(f"gate verdicts {np.flatnonzero(report['removed'])} against {np.flatnonzero(fr.removed)}")
        elif kind == CHORD:
            r = chord_ratio(report["stat"], fr.stat)
            if not r <= (K_CHORD if k_chord is None else k_chord):
                bad.append(f"chord {r:.3g} u (1 + chord) from the exact one")
    return bad, depth


def chord_ratio(stat, exact):
    """max |stat - exact| / (u (1 + exact))"""
    return max([float(abs(mpf(float(s)) - e) / (mpf(U64) * (1 + e))) for s, e in zip(stat, exact)], default=0.0)


def depth_ratio(depth, exact):
    return float(abs(mpf(float(depth)) - exact) / (mpf(U64) * exact))
