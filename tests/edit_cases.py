"""TEST INFRASTRUCTURE ONLY -- the states and frames that tests/test_edit_exact.py (CPU) and tests/test_gpu_edit.py (MI355X) share, so that
the decision margins and the bound are checked on the CPU for exactly the frames the device is held to.

State: riccati_cases.device_snapshot / oracle_snapshot with the ids moved up by ID0 (so that a new id can lie BELOW every state id), the
Sigma families a, c, e of update_cases (b where Gamma[0:6] is not asserted).  The call is the stream's fifth vision frame, as in
update_cases.  Gate: chord at 0.05 or Mahalanobis at 0.5, an outlier is a bearing turned by 0.2 rad (gate_helpers.rotated).

FRAMES (make_case(frame=...)); o = the kept indices whose bearing is turned
    lose             landmark 0, the middle one and the last are absent: every record moves
    add              new ids below AND above every state id: the low id is appended at the end, the permutation is not the identity
    outlier          nothing but outliers                          outlier+add, lose+outlier, all (lose + outliers + add)
    armed_quiet+add  the gate armed and nothing trips              all_lost+add   nothing is left: depth = initialSceneDepth
    empty+add        the filter restored with N = 0                full           `add` in a handle whose capacity is the final N
    returning        the last landmark is the outlier and its id the largest of the measurement; one new id below: the gated id is in the
                     measurement and must not be in the final ids
DEPTH PATTERNS (make_case(pattern=...)), all with two new landmarks
    nF1 .. nF4       all but the first 1 .. 4 landmarks are lost (the upper median for even nF)
    tie3             the landmarks of rank m - 1 and m + 1 (m = nF // 2) become bitwise copies (p0, Q, bearing) of the one of rank m
    tie_all          every landmark is a copy of landmark 0
    tie_after_gate   the outlier is the landmark next to the median in rank whose removal makes ANOTHER landmark the median
BOOKKEEPING-ONLY sizes (256 .. 1040) use big_snapshot: a deterministic synthetic state (no stream behind it, Sigma diagonal), the same on both
machines, because neither oracle can be driven to a 3131 x 3131 covariance in test time; only ids, origin and the gate report are compared
there."""
import numpy as np

import gate_helpers as G
import lie_edge_cases as ec
import riccati_cases as rc
import update_cases as uc
from oracle import eqf_numpy as en

ID0 = 100
LOW_ID, HIGH_ID = 7, 50000
CHORD, MAHA = 0, 1
CHORD_THR, MAHA_THR = 0.05, G.TAU
ANGLE = 0.2
NEW_Y = np.array([[0.12, -0.09, 1.0], [-0.2, 0.15, 1.0]])
NEW_Y = NEW_Y / np.linalg.norm(NEW_Y, axis=1, keepdims=True)

FRAMES = ("lose", "add", "outlier", "outlier+add", "lose+outlier", "all", "armed_quiet+add", "all_lost+add", "empty+add", "full", "returning")
PATTERNS = ("nF1", "nF2", "nF3", "nF4", "tie3", "tie_all", "tie_after_gate")
FULL_SIZES = (5, 21, 58, 59, 60, 61, 63, 64, 65, 70, 129)
BOOK_SIZES = (256, 257, 1024, 1025, 1040)
TILED = rc.TILED


def settings():
    return uc.settings()


def shifted(snap):
    """The snapshot with its ids moved up by ID0"""
    return dict(snap, ids=np.asarray(snap["ids"], dtype=np.int32) + ID0)


def big_snapshot(N, seed=5):
    """A synthetic state of N landmarks 2 .. 8 m in front of the camera with non-trivial Q_i, ids ID0 .. ID0 + N - 1, Sigma diagonal"""
    rng = np.random.default_rng(seed + N)
    base = ec.base_snapshot(5)
    ang = np.deg2rad(30.0) * np.sqrt(rng.uniform(size=N))
    az = rng.uniform(0, 2 * np.pi, N)
    p = np.stack([np.sin(ang) * np.cos(az), np.sin(ang) * np.sin(az), np.cos(ang)], axis=1) * rng.uniform(2.0, 8.0, N)[:, None]
    base["origin"]["p"] = p
    axis = rng.standard_normal((N, 3))
    half = 0.5 * rng.uniform(0.01, 0.05, N)
    base["group"]["Qq"] = np.concatenate([np.cos(half)[:, None], np.sin(half)[:, None] * axis / np.linalg.norm(axis, axis=1, keepdims=True)], axis=1)
    base["group"]["Qa"] = rng.uniform(0.9, 1.1, N)
    base["ids"] = np.arange(ID0, ID0 + N, dtype=np.int32)
    base["sigma"] = np.diag(rng.uniform(0.5, 2.0, 11 + 3 * N))
    base["currentVelocity"] = np.array([0.02, -0.01, 0.03, 0.3, -9.7, 0.4])
    return base


def stepped(snap, stamp):
    """(predicted bearings, squared depths) of the numpy oracle's state at the stamp: only used to CHOOSE landmarks and to make bearings"""
    f = ec.numpy_filter(en, snap, settings())
    f.integrateUpToTime(stamp, False)
    p = f.stateEstimate().p.reshape(-1, 3)
    d2 = np.sum(p * p, axis=1)
    return p / np.sqrt(d2)[:, None], d2


def big_call(N):
    """(snapshot, stamp, bearings): the predicted bearings with a deterministic disturbance of about 2e-3 rad"""
    snap = big_snapshot(N)
    stamp = ec.T0 + 0.025
    yhat, _ = stepped(snap, stamp)
    rng = np.random.default_rng(N)
    y = yhat + 2e-3 * rng.standard_normal(yhat.shape)
    return snap, stamp, y / np.linalg.norm(y, axis=1, keepdims=True)


def _copy_record(snap, dst, src, y):
    snap["origin"]["p"][dst] = snap["origin"]["p"][src]
    snap["group"]["Qq"][dst] = snap["group"]["Qq"][src]
    snap["group"]["Qa"][dst] = snap["group"]["Qa"][src]
    y[dst] = y[src]


def default_outliers(N):
    return sorted({0, N // 2, N - 1})[:2] if N > 2 else [0]


def make_case(snap, stamp, y, frame="add", pattern=None, kind=CHORD, thr=None, out_at=None, capacity=None, name=None):
    """snap: a snapshot with shifted ids; y: the frame's bearings of the snapshot's landmarks.  Returns a dict with the (possibly patterned)
    snapshot, the measurement (ids ascending, bearings), the gate and the handle capacity to use."""
    N = len(snap["ids"])
    snap = dict(snap, origin=dict(snap["origin"], p=np.array(snap["origin"]["p"], dtype=float).reshape(N, 3)),
                group=dict(snap["group"], Qq=np.array(snap["group"]["Qq"], dtype=float).reshape(N, 4), Qa=np.array(snap["group"]["Qa"], dtype=float).reshape(N)))
    y = np.array(y, dtype=float).reshape(N, 3)
    ids = [int(i) for i in snap["ids"]]
    lost, outl, add = set(), [], False
    if frame in ("lose", "lose+outlier", "all"):
        lost = {0, N // 2, N - 1}
    if frame in ("add", "outlier+add", "all", "armed_quiet+add", "all_lost+add", "empty+add", "full") or pattern:
        add = True
    if frame == "all_lost+add":
        lost = set(range(N))
    if frame == "empty+add":
        assert N == 0
    if pattern and pattern.startswith("nF"):
        lost = set(range(int(pattern[2:]), N))
    if pattern in ("tie3", "tie_all", "tie_after_gate"):
        _, d2 = stepped(snap, stamp)
        live = [o for o in range(N) if o not in lost]
        order = sorted(live, key=lambda o: d2[o])
        m = len(order) // 2
        if pattern == "tie3":
            _copy_record(snap, order[m - 1], order[m], y)
            _copy_record(snap, order[m + 1], order[m], y)
        elif pattern == "tie_all":
            for o in range(1, N):
                _copy_record(snap, o, 0, y)
        else:
            out_at = [order[m + 1] if len(order) % 2 == 0 else order[m - 1]]
            frame = "outlier+add"
    if frame in ("outlier", "outlier+add", "lose+outlier", "all", "returning"):
        kept = [o for o in range(N) if o not in lost]
        if frame == "returning":
            outl = [N - 1]
        elif out_at is not None:
            outl = [o for o in out_at if o in kept]
        else:
            outl = [kept[j] for j in default_outliers(len(kept))]
            if frame == "outlier+add":
                outl = outl[:1]
        for o in outl:
            y[o] = G.rotated(y[o], ANGLE)
    meas = [(ids[o], y[o]) for o in range(N) if o not in lost]
    if frame == "returning":
        meas.append((LOW_ID, NEW_Y[0]))
    elif add:
        meas += [(LOW_ID, NEW_Y[0]), (HIGH_ID, NEW_Y[1])]
    meas.sort(key=lambda t: t[0])
    n_new = sum(1 for i, _ in meas if i not in ids)
    if thr is None:
        thr = CHORD_THR if kind == CHORD else MAHA_THR
    cap = capacity if capacity is not None else (N + n_new if frame == "full" else N + 5)
    return dict(name=name or f"{frame}{'/' + pattern if pattern else ''}", snap=snap, stamp=float(stamp), ids=np.array([i for i, _ in meas], dtype=np.int32),
                y=np.array([v for _, v in meas], dtype=float).reshape(len(meas), 3), kind=kind, thr=thr, capacity=cap, outliers=[ids[o] for o in outl],
                N=N)


def disarmed(case):
    """The same frame under a gate that cannot trip (chord threshold >= 2)"""
    return dict(case, kind=CHORD, thr=1e9)


def empty_snapshot(snap):
    """The snapshot's base state with no landmark"""
    return dict(snap, ids=np.zeros(0, dtype=np.int32), origin=dict(snap["origin"], p=np.zeros((0, 3))),
                group=dict(snap["group"], Qq=np.zeros((0, 4)), Qa=np.zeros(0)), sigma=np.array(snap["sigma"], dtype=float)[:11, :11].copy())


def sigma_of(case, fam):
    """Sigma of the family for the case's (patterned) snapshot: the family's matrix at the snapshot's size"""
    snap = case["snap"]
    if len(snap["ids"]) == 0:
        S = np.array(snap["sigma"], dtype=float)
        return np.triu(S) + np.triu(S, 1).T
    return uc.sigma_family(snap, fam)


# ---- the committed cases, per device route ----------------------------------------------------------------------------------------------------
def spec(N, frame="add", pattern=None, kind=CHORD, armed=True, fam="a", out_at=None):
    return dict(N=N, frame=frame, pattern=pattern, kind=kind, armed=armed, fam=fam, out_at=out_at)


def _edge_outliers(N):
    return sorted({0, 63, 64, N - 1} & set(range(N)))


# k_edit, gate disarmed: frames x sizes, every depth pattern (nF* from the N = 5 state, the ties at 21)
EDIT_DISARMED = ([spec(N, fr, armed=False, fam=fam) for N, fam in ((5, "e"), (21, "c"), (70, "a")) for fr in ("lose", "add", "all_lost+add", "full")]
                 + [spec(5, pattern=p, armed=False, fam="a") for p in ("nF1", "nF2", "nF3", "nF4")]
                 + [spec(21, pattern="tie3", armed=False, fam="e"), spec(21, pattern="tie_all", armed=False, fam="b")]
                 + [spec(0, "empty+add", armed=False, fam="a")])
# k_edit<double, 0>, chord gate armed, at least 59 measurement entries: every frame at 70 (but all_lost+add, whose two measurement
# entries send an armed frame to the separate launches: it is in SEPARATE, armed; an empty filter arms no gate); 59 .. 61 lose outliers down to 57 / 58 / 58
# landmarks (the update deferred, flag 2); 63, 64, 65, 129 with outliers at kept index 0, 63, 64 and the last
EDIT_CHORD = ([spec(70, fr, fam="c" if k % 2 else "a") for k, fr in enumerate(f for f in FRAMES if f not in ("empty+add", "all_lost+add"))]
              + [spec(70, pattern="tie_after_gate"), spec(70, pattern="tie3", fam="c")]
              + [spec(59, "outlier"), spec(60, "outlier", fam="c"), spec(61, "outlier", out_at=[0, 30, 60])]
              + [spec(N, "outlier+add" if N % 2 else "outlier", out_at=_edge_outliers(N), fam="c" if N == 64 else "a") for N in (63, 64, 65, 129)])
EDIT_MAHA = [spec(N, fr, kind=MAHA) for N in (64, 65, 70) for fr in ("outlier", "outlier+add", "all")]
# the separate launches (device_edit = 0, or chosen by the host below 59 measurement entries with the gate armed)
SEPARATE = ([spec(21, fr, fam=fam) for fr, fam in (("lose", "c"), ("add", "a"), ("outlier+add", "a"), ("all", "c"), ("armed_quiet+add", "a"), ("returning", "a"))]
            + [spec(58, "all"), spec(58, "outlier+add", fam="c"), spec(70, "all"), spec(70, "lose+outlier", fam="c")]
            + [spec(21, pattern="tie_after_gate"), spec(21, "all_lost+add", armed=False, fam="e"), spec(21, pattern="tie3", armed=False, fam="e"),
               spec(70, "all_lost+add", fam="c"), spec(0, "empty+add", armed=False), spec(21, "full")])
SEPARATE_MAHA = [spec(21, "all", kind=MAHA), spec(58, "outlier+add", kind=MAHA)]
HOST_CHOICE_58 = [spec(58, "all"), spec(58, "outlier", fam="c")]   # 57 and 58 measurement entries (58 landmarks + 2 new ones would be k_edit's)
# fp32 handles: `all` runs armed wherever the route can take it armed -- k_edit from 59 measurement entries on, the separate launches always
F32_EDIT = [spec(N, fr, armed=(fr == "all" and N >= 59), fam=fam) for N in (17, 70) for fr, fam in (("lose", "c"), ("all", "a"))]
F32_SEPARATE = [spec(N, fr, armed=(fr == "all"), fam=fam) for N in (17, 70) for fr, fam in (("lose", "c"), ("all", "a"))]
F32 = F32_EDIT + [s for s in F32_SEPARATE if s not in F32_EDIT]
TILED_SPECS = [spec(N, "all") for N, _ in TILED] + [spec(N, pattern="tie3", armed=False) for N, _ in TILED]
# one handle of four filters.  With the gate armed k_edit takes a frame only if EVERY filter has at least 59 measurement entries, so the ragged
# handle of the one-launch route has four such filters and the one with the empty measurement is on the separate launches only
RAGGED = [spec(21, "lose", fam="c"), spec(33, "outlier"), spec(5, "add"), spec(17, "none")]
RAGGED_EDIT = [spec(63, "lose", fam="c"), spec(70, "outlier"), spec(61, "add"), spec(65, "armed_quiet+add")]
FULL_SPECS = EDIT_DISARMED + EDIT_CHORD + EDIT_MAHA + SEPARATE + SEPARATE_MAHA + HOST_CHOICE_58 + F32 + TILED_SPECS + RAGGED[:3] + RAGGED_EDIT
# bookkeeping only: (N, frame, pattern, armed)
BOOK_EDIT = [spec(256, "lose", armed=False), spec(257, "all", armed=False), spec(1024, pattern="tie3", armed=False), spec(257, "all")]
# (k_median_depth has a rank expression of its own: 1040 `add` and 1040 `all` with one outlier leave 1040 and 1036 landmarks, EVEN
# counts, so that a lower median is seen there too; the other three leave 1025, 1037 and 1035)
BOOK_SEPARATE = [spec(1025, pattern="tie3", armed=False), spec(1040, "all", armed=False), spec(1040, "all"), spec(1040, "add", armed=False),
                 spec(1040, "all", out_at=[500])]


def key(s):
    return (s["N"], s["frame"], s["pattern"], s["kind"], s["armed"], s["fam"], tuple(s["out_at"]) if s["out_at"] else None)


def unique(specs, with_family=True):
    seen, out = set(), []
    for s in specs:
        k = key(s) if with_family else key(dict(s, fam=None))
        if k not in seen:
            seen.add(k)
            out.append(s)
    return out


def case_of(s, snap, stamp=None, y=None):
    """make_case for a spec from the size's base snapshot (ids not yet shifted); stamp / y default to the stream's fifth vision frame"""
    N = s["N"]
    if stamp is None:
        stamp, _, y = uc.vision_call(max(N, 1), "e" if s["fam"] == "e" else "a")
    snap = shifted(snap)
    if N == 0:
        snap, y = empty_snapshot(snap), np.zeros((0, 3))
    if s["frame"] == "none":
        c = make_case(snap, stamp, y, frame="add", kind=s["kind"])
        return dict(c, ids=np.zeros(0, dtype=np.int32), y=np.zeros((0, 3)), name="empty measurement")
    c = make_case(snap, stamp, y, frame=s["frame"], pattern=s["pattern"], kind=s["kind"],
                  out_at=s["out_at"])
    return c if s["armed"] else disarmed(c)
