"""Scoring candidate vision frames on the device (eqf_score_vision, csrc/eqf_score.hpp) against the exact reference and the a-priori bound of
tests/score_exact.py built from the device's own getters, record by record; the bitwise facts the header promises; non-mutation; the
joint-compatibility monotonicity; the update the score predicts; local trouble; argument errors; edges.  States and candidates:
tests/score_cases.py -- one ragged handle of capacity 100 with N = 100, 33 (ids not ascending, produced by churn) and 7, five candidates
per filter, matched counts 1, 2, 31, 32, 33, 64, 65, 97 (orders 2 .. 194).  The same cases hold the numpy statement and a model of the
blocking inside the bound on the CPU (tests/test_score_exact.py).  No constant here comes from the device.

Worst ratio to the bound on an MI355X (test 1 prints its own per matched count): NOTES.md R24.1 -- nis <= 0.0019, logdet_S <= 0.0016,
loglik <= 0.0016, nis_lm <= 0.080."""
import ctypes as C

import numpy as np
import pytest

import consistency_cases as cc
import consistency_exact as cx
import riccati_cases as rc
import score_cases as sc
import score_exact as sx
import update_exact as ux

pytestmark = pytest.mark.gpu

B = len(sc.STATE_N)
_SNAP, _REF = {}, {}


@pytest.fixture(scope="module")
def hip():
    from eqf_vio_amd import binding

    return binding


def snapshots(hip):
    if not _SNAP:
        for b in range(B):
            _SNAP[b] = sc.device_state(hip, b)
    return [_SNAP[b] for b in range(B)]


def handle(hip, capacity=sc.CAPACITY, batch=B, place=None):
    """the ragged handle: filter b of the cases in slot place[b] (default b)"""
    fg = hip.FilterBatch(sc.settings(), capacity=capacity, batch=batch)
    for b, snap in enumerate(snapshots(hip)):
        fg.restore_state(snap, b if place is None else place[b])
    return fg


def cands(hip):
    return [sc.candidates(b, snapshots(hip)[b]["ids"]) for b in range(B)]


def geometry(hip, b):
    key = ("geo", b)
    if key not in _REF:
        snap = snapshots(hip)[b]
        _REF[key] = sx.geometry(snap, sc.settings(), sc.state_bearings(b, snap["ids"]))
    return _REF[key]


def reference(hip, b, slots):
    """(ref, bounds) of the candidate of filter b that matches `slots`, once per module; Sigma is the device's own sigma()"""
    key = (b, tuple(slots))
    if key not in _REF:
        ref = sx.reference(snapshots(hip)[b]["sigma"], geometry(hip, b), float(sc.settings()["measurementVariance"]), slots)
        _REF[key] = (ref, sx.bounds(ref))
    return _REF[key]


def score(fg, per_filter, **kw):
    """per_filter[b]: list of (ids, bearings, ...) -> FrameScores with nis_lm and used"""
    return fg.score_vision([[c[0] for c in row] for row in per_filter], [[c[1] for c in row] for row in per_filter], want_lm=True, **kw)


def record(r, b, c, ids):
    """the record of candidate (b, c) of a result, nis_lm and used cut to the candidate's own entries"""
    n = len(ids)
    return dict(nis=r.nis[b, c], logdet_S=r.logdet_S[b, c], loglik=r.loglik[b, c], dof=r.dof[b, c], info=r.info[b, c],
                nis_lm=r.nis_lm[b, c, :n].copy(), used=r.used[b, c, :n].copy())


def _bits(x):
    if isinstance(x, dict):
        return {k: _bits(v) for k, v in x.items()}
    return np.ascontiguousarray(x).tobytes() + str(np.asarray(x).shape).encode()


def same(a, b, what):
    a, b = _bits(a), _bits(b)
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k], f"{what}: {k} differs"


def getters(fg, b):
    """every getter of filter b"""
    g = dict(n=fg.num_landmarks(b), est=fg.state_estimate(b), gate=fg.gate_report(b), last=fg.last_update(b), innov=fg.innovation_stats(b),
             err=fg.device_error(), sigma_local=fg.sigma_local(b), marg0=fg.marginals(b, local=False), marg1=fg.marginals(b, local=True),
             time=fg.get_time())
    g.update(fg.dump_state(b))
    return g


def digest(fg):
    return [getters(fg, b) for b in range(fg.B)]


def same_handle(a, b, what):
    for k, (x, y) in enumerate(zip(a, b)):
        same(x, y, f"{what}, filter {k}")


# ---- 1. entry by entry
def test_records_entry_by_entry(hip):
    fg = handle(hip)
    cs_ = cands(hip)
    for b in range(B):
        assert [int(i) for i in fg.ids(b)] == [int(i) for i in sc.labels(b)]
        assert np.array_equal(fg.sigma(b), snapshots(hip)[b]["sigma"])
    assert list(fg.ids(1)) != sorted(fg.ids(1))
    r = score(fg, cs_)
    assert fg.device_error() == 0
    seen, worst = set(), {}
    for b in range(B):
        state_ids = [int(i) for i in fg.ids(b)]
        for c, (ids, y, slots) in enumerate(cs_[b]):
            got = record(r, b, c, ids)
            M = len(slots)
            seen.add(M)
            assert got["info"] == 0 and got["dof"] == 2 * M, (b, c, got["info"], got["dof"])
            pos = [list(ids).index(state_ids[s]) for s in slots]
            used = np.zeros(len(ids), dtype=np.uint8)
            used[pos] = 1
            assert np.array_equal(got["used"], used), (b, c)
            assert np.all(got["nis_lm"][used == 0] == 0.0) and np.all(r.nis_lm[b, c, len(ids):] == 0.0) and np.all(r.used[b, c, len(ids):] == 0)
            ref, bnd = reference(hip, b, slots)
            if M:
                assert sx.condition(ref, bnd) <= 1.0, (b, c, "the bound is not licensed on this state")
            q = sx.ratios(dict(got, nis_lm=got["nis_lm"][pos]), ref, bnd)
            for k, v in q.items():
                worst[(M, k)] = max(worst.get((M, k), 0.0), v)
            assert max(q.values()) <= 1.0, (b, c, M, q)
    assert set(sc.MATCHED) <= seen and 0 in seen
    for M in sorted(seen):
        print(f"|M| = {M:3d} (order {2 * M:3d}): device / bound  " + "  ".join(f"{k} {worst[(M, k)]:.3g}" for k in ("nis", "logdet_S", "loglik", "nis_lm")))
    fg.close()


# ---- 2. bitwise facts
def test_bitwise_facts(hip):
    fg = handle(hip)
    cs_ = cands(hip)
    empty = (np.zeros(0, dtype=np.int32), np.zeros((0, 3)), [])
    full = score(fg, cs_)
    want = {(b, c): record(full, b, c, cs_[b][c][0]) for b in range(B) for c in range(sc.NCAND)}
    same({str(k): v for k, v in want.items()},
         {str(k): record(score(fg, cs_), k[0], k[1], cs_[k[0]][k[1]][0]) for k in want}, "run to run")
    # alone in a call
    for b, c in ((0, 0), (0, 1), (1, 0), (1, 3), (2, 1), (0, 4)):
        alone = score(fg, [[cs_[b][c]] if bb == b else [empty] for bb in range(B)])
        same(record(alone, b, 0, cs_[b][c][0]), want[(b, c)], f"alone {(b, c)}")
    # other orders, a candidate twice, another stride
    order = [4, 2, 0, 3, 1, 0]
    mixed = score(fg, [[cs_[b][c] for c in order] for b in range(B)], stride=107)
    for b in range(B):
        for k, c in enumerate(order):
            same(record(mixed, b, k, cs_[b][c][0]), want[(b, c)], f"reordered {(b, c)}")
        same(record(mixed, b, 2, cs_[b][0][0]), record(mixed, b, 5, cs_[b][0][0]), "a candidate twice in one call")
    # the chunking
    for chunk in (1, 2, 0):
        fg.set_option("score_chunk", chunk)
        got = score(fg, cs_)
        same({str(k): record(got, k[0], k[1], cs_[k[0]][k[1]][0]) for k in want}, {str(k): v for k, v in want.items()}, f"chunk {chunk}")
    with pytest.raises(Exception):
        fg.set_option("score_chunk", 4097)
    # another slot of a larger batch, through eqf_copy_filters
    big = hip.FilterBatch(sc.settings(), capacity=sc.CAPACITY + 21, batch=5)
    place = [4, 0, 2]
    big.copy_filters(fg, place, [0, 1, 2])
    rows = [[empty] * sc.NCAND for _ in range(5)]
    for b in range(B):
        rows[place[b]] = cs_[b]
    got = score(big, rows)
    for (b, c), w in want.items():
        same(record(got, place[b], c, cs_[b][c][0]), w, f"larger batch {(b, c)}")
    for k in (1, 3):   # the filters of the larger handle that were never initialised
        assert np.all(got.info[k] == 0) and np.all(got.dof[k] == 0) and np.all(got.nis[k] == 0.0)
    big.close()
    fg.close()


# ---- 3. the call only reads
def _run_on(hip, fg, score_between=None):
    """four IMU calls and the next vision frame of every filter's stream"""
    recs = rc.plan(sc.STATE_N[0])[2]
    for k, r in enumerate(recs):
        fg.process_imu(r[0], r[1:4], r[4:7])
        if score_between is not None and k == 1:
            score_between()
    stride = max(sc.STATE_N)
    ids, y, nb, stamps = np.zeros((B, stride), dtype=np.int32), np.zeros((B, stride, 3)), [], []
    for b in range(B):
        st, head, _ = rc.plan(sc.STATE_N[b])
        nxt = 1 + max(k for kind, k in head if kind == "vision")
        lab = sc.labels(b)
        order = np.argsort(lab, kind="stable")
        ids[b, :len(lab)], y[b, :len(lab)] = lab[order], st.bearings[nxt][order]
        nb.append(len(lab))
        stamps.append(st.vision_stamps[nxt])
    assert np.all(fg.process_vision(stamps, ids, y, nb=nb) == 0)


def test_the_call_only_reads(hip):
    fg, twin = handle(hip), handle(hip)
    for h in (fg, twin):
        h.set_option("innovation_stats", 1)
    cs_ = cands(hip)
    before = digest(fg)
    n0 = fg.nees()
    r = score(fg, cs_)
    assert np.all(r.info == 0)
    same(n0, fg.nees(), "eqf_get_nees around a score")
    same_handle(before, digest(fg), "getters around a score")
    # (the twin is compared once both have updated: eqf_get_last_update of a handle that never updated is whatever its allocation held)
    # a handle that scored, also with IMU calls queued, goes on like one that never did
    _run_on(hip, fg, score_between=lambda: score(fg, cs_))
    _run_on(hip, twin)
    assert fg.device_error() == 0
    same_handle(digest(fg), digest(twin), "after four IMU calls and a vision frame")
    fg.close()
    twin.close()


# ---- 4. joint compatibility: monotone in the candidate
def test_nested_candidates_are_monotone(hip):
    from eqf_vio_amd import consistency as cs

    fg = handle(hip)
    ids0 = [int(i) for i in fg.ids(0)]
    y0 = sc.state_bearings(0, ids0)
    sizes = (1, 2, 20, 66, 100)
    row = []
    for k in sizes[:sc.NCAND]:
        sl = list(range(k))
        entries = sorted((ids0[s], tuple(y0[s])) for s in sl)
        row.append((np.array([e[0] for e in entries], dtype=np.int32), np.array([e[1] for e in entries]), sl))
    empty = (np.zeros(0, dtype=np.int32), np.zeros((0, 3)), [])
    r = score(fg, [row, [empty] * len(row), [empty] * len(row)])
    assert np.all(r.info == 0)
    refs = [reference(hip, 0, c[2]) for c in row]
    for k in range(len(row) - 1):
        assert r.nis[0, k] <= r.nis[0, k + 1] + refs[k][1]["nis"] + refs[k + 1][1]["nis"], (sizes[k], r.nis[0, k], r.nis[0, k + 1])
    assert abs(r.nis[0, 0] - r.nis_lm[0, 0, 0]) <= refs[0][1]["nis"] + refs[0][1]["nis_lm"][0]
    ok = cs.joint_compatible(r, 0.999)
    assert ok.shape == r.nis.shape and np.all(ok[1:])   # (empty candidates are compatible)
    fg.close()


# ---- 5. against the update it predicts (plumbing: r, dof, the index maps, the residual's signs)
def test_against_the_update_it_predicts(hip):
    A = handle(hip)
    Bh = hip.FilterBatch(sc.settings(), capacity=sc.CAPACITY, batch=B)
    Bh.copy_filters(A, list(range(B)), list(range(B)))
    Bh.set_option("innovation_stats", 1)
    Bh.set_outlier_gate(hip.GATE_CHORD, 10.0)   # (a chord never exceeds 2: disarmed)
    snaps = snapshots(hip)
    t1 = float(snaps[0]["time"]) + 0.002
    held = rc.plan(sc.STATE_N[0])[2][0]
    stride = max(sc.STATE_N)
    ids, y, nb, frame = np.zeros((B, stride), dtype=np.int32), np.zeros((B, stride, 3)), [], []
    for b in range(B):
        sid = [int(i) for i in snaps[b]["ids"]]
        yb = sc.state_bearings(b, sid)
        order = np.argsort(sid, kind="stable")
        ids[b, :len(sid)], y[b, :len(sid)] = np.array(sid)[order], yb[order]
        nb.append(len(sid))
        frame.append((np.array(sid, dtype=np.int32)[order], yb[order], list(range(len(sid))), order))
    assert np.all(Bh.process_vision([t1] * B, ids, y, nb=nb) == 0)
    assert np.all(A.process_imu([t1] * B, held[1:4], held[4:7]) == 0)
    r = score(A, [[frame[b][:3]] for b in range(B)])
    assert A.device_error() == 0 and Bh.device_error() == 0
    d = sc.settings()
    for b in range(B):
        st = Bh.innovation_stats(b)
        N = sc.STATE_N[b]
        assert st["valid"] and st["dof"] == 2 * N == r.dof[b, 0] and r.info[b, 0] == 0
        # the two bounds: this route's at A's state (its Sigma after the IMU call) and the innovation statistics' of the same vision call
        snapA = A.dump_state(b)
        ref = sx.reference(snapA["sigma"], sx.geometry(snapA, d, sc.state_bearings(b, snapA["ids"])), float(d["measurementVariance"]), list(range(N)))
        mine = sx.bounds(ref)
        case = ux.Case(snaps[b], d, t1, sc.state_bearings(b, snaps[b]["ids"]))
        uref, ubnd = case.reference(snaps[b]["sigma"])
        _, theirs = cx.innovation_stats_reference(uref, ubnd, cc.C_LOG)
        lm_state = np.empty(N)
        lm_state[frame[b][3]] = r.nis_lm[b, 0, :N]   # entry k of the frame is the landmark in state slot order[k]
        assert abs(r.nis[b, 0] - st["nis"]) <= mine["nis"] + theirs["nis"], (b, r.nis[b, 0], st["nis"])
        assert abs(r.logdet_S[b, 0] - st["logdet_S"]) <= mine["logdet_S"] + theirs["logdet_S"], (b, r.logdet_S[b, 0], st["logdet_S"])
        assert np.all(np.abs(lm_state - st["nis_lm"]) <= mine["nis_lm"] + theirs["nis_lm"]), b
        print(f"filter {b}: nis {r.nis[b, 0]!r} vs update {st['nis']!r}; logdet_S {r.logdet_S[b, 0]!r} vs {st['logdet_S']!r}; "
              f"dof {r.dof[b, 0]}; nis_lm bit for bit: {np.array_equal(lm_state, st['nis_lm'])}, nis: {r.nis[b, 0] == st['nis']}, "
              f"logdet_S: {r.logdet_S[b, 0] == st['logdet_S']}")
    A.close()
    Bh.close()


# ---- 6. trouble stays local
def test_trouble_stays_local(hip):
    fg = handle(hip)
    cs_ = cands(hip)
    clean = score(fg, cs_)
    S = fg.sigma(1)
    k = slice(11 + 3 * 5, 14 + 3 * 5)
    S[k, k] = -np.eye(3)     # landmark slot 5 of filter 1: S_ii = C (-I) C^T + r I is not positive definite
    fg.set_sigma(S, 1)
    got = score(fg, cs_)
    assert fg.device_error() == 0
    for b in range(B):
        for c in range(sc.NCAND):
            rec = record(got, b, c, cs_[b][c][0])
            if b == 1 and 5 in cs_[b][c][2]:
                assert rec["info"] == 1 and rec["dof"] == 2 * len(cs_[b][c][2])
                assert np.isnan(rec["nis"]) and np.isnan(rec["logdet_S"]) and np.isnan(rec["loglik"])
            else:
                same(rec, record(clean, b, c, cs_[b][c][0]), f"untouched {(b, c)}")
    assert sum(1 for c in range(sc.NCAND) if 5 in cs_[1][c][2]) >= 2 and sum(1 for c in range(sc.NCAND) if 5 not in cs_[1][c][2]) >= 2
    masked = score(fg, cs_, mask=[1, 0, 1])
    assert np.all(masked.info[1] == 3) and np.all(np.isnan(masked.nis[1])) and np.all(np.isnan(masked.loglik[1])) and np.all(masked.dof[1] == 0)
    assert np.all(masked.nis_lm[1] == 0.0) and np.all(masked.used[1] == 0)
    for b in (0, 2):
        for c in range(sc.NCAND):
            same(record(masked, b, c, cs_[b][c][0]), record(clean, b, c, cs_[b][c][0]), f"beside a masked filter {(b, c)}")
    assert fg.device_error() == 0
    fg.close()


# ---- 7. argument errors come before any effect
def test_argument_errors_come_before_any_effect(hip):
    fg = handle(hip)
    L = hip.lib()
    ip, dp, up = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_ubyte)
    before = digest(fg)
    stride, ncand = 4, 2

    def call(h=None, ncand_=ncand, nb=None, ids=None, y=None, stride_=stride, mask=None, null=()):
        nbv = np.ascontiguousarray(np.full((B, ncand), 3) if nb is None else nb, dtype=np.int32)
        idv = np.ascontiguousarray(np.tile(np.array([0, 1, 2, 3]), (B, ncand, 1)) if ids is None else ids, dtype=np.int32)
        yv = np.ascontiguousarray(np.tile(np.array([0.0, 0.0, 1.0]), (B, ncand, stride, 1)) if y is None else y, dtype=np.float64)
        out = (hip.FrameScore * (B * ncand))()
        mk = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        return L.eqf_score_vision((fg if h is None else h)._h if "f" not in null else None, ncand_,
                                  None if "nb" in null else nbv.ctypes.data_as(ip), None if "ids" in null else idv.ctypes.data_as(ip),
                                  None if "y" in null else yv.ctypes.data_as(dp), stride_, None if mk is None else mk.ctypes.data_as(up),
                                  None if "out" in null else out, None, None)

    assert call() == 0
    bad_nb_hi, bad_nb_lo, cap_nb = np.full((B, ncand), 3), np.full((B, ncand), 3), np.full((B, ncand), 3)
    bad_nb_hi[1, 1], bad_nb_lo[2, 0] = 5, -1
    unsorted = np.tile(np.array([0, 1, 2, 3]), (B, ncand, 1))
    unsorted[2, 1] = [0, 2, 2, 3]
    nan_y = np.tile(np.array([0.0, 0.0, 1.0]), (B, ncand, stride, 1))
    nan_y[0, 1, 2, 1] = np.nan
    inf_y = nan_y.copy()
    inf_y[0, 1, 2, 1] = np.inf
    refusals = [(dict(null=("f",)), hip.ERR_INVALID), (dict(null=("nb",)), hip.ERR_INVALID), (dict(null=("ids",)), hip.ERR_INVALID),
                (dict(null=("y",)), hip.ERR_INVALID), (dict(null=("out",)), hip.ERR_INVALID), (dict(ncand_=0), hip.ERR_INVALID),
                (dict(stride_=0), hip.ERR_INVALID), (dict(nb=bad_nb_hi), hip.ERR_INVALID), (dict(nb=bad_nb_lo), hip.ERR_INVALID),
                (dict(y=nan_y), hip.ERR_INVALID), (dict(y=inf_y), hip.ERR_INVALID), (dict(ids=unsorted), hip.ERR_UNSORTED)]
    for kw, code in refusals:
        assert call(**kw) == code, (kw.keys(), code)
        same_handle(before, digest(fg), f"after a refused call {list(kw)}")
    # what a masked filter's lists hold is not looked at; behind nb nothing is
    assert call(ids=unsorted, mask=[1, 1, 0]) == 0 and call(y=nan_y, mask=[0, 1, 1]) == 0
    nb2 = np.full((B, ncand), 3)
    nb2[0, 1] = 2
    assert call(y=nan_y, nb=nb2) == 0
    # capacity: a handle smaller than the lists
    small = hip.FilterBatch(sc.settings(), capacity=2, batch=B)
    plain = lambda h: [dict(h.dump_state(b), err=h.device_error()) for b in range(B)]  # noqa: E731  (its filters are not initialised: no chart)
    s0 = plain(small)
    assert call(h=small) == hip.ERR_CAPACITY
    same_handle(s0, plain(small), "after EQF_ERR_CAPACITY")
    small.close()
    f32 = hip.FilterBatch(sc.settings(), capacity=8, batch=B, precision=hip.PRECISION_F32)
    assert call(h=f32) == hip.ERR_UNSUPPORTED
    f32.close()
    same_handle(before, digest(fg), "at the end")
    fg.close()


# ---- 8. edges
def test_edges_and_the_python_facade(hip):
    from eqf_vio_amd import filter as vf

    fg = hip.FilterBatch(sc.settings(), capacity=sc.CAPACITY, batch=B)
    fg.restore_state(snapshots(hip)[2], 0)   # filters 1 and 2 stay uninitialised
    c2 = sc.candidates(2, snapshots(hip)[2]["ids"])
    r = score(fg, [[c2[4], c2[3], c2[0]], [c2[0], c2[1], c2[4]], [c2[0], c2[0], c2[0]]])
    for b, c in ((0, 0), (0, 1), (1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2)):   # nb = 0; no match; an uninitialised filter
        assert r.info[b, c] == 0 and r.dof[b, c] == 0, (b, c)
        for v in (r.nis[b, c], r.logdet_S[b, c], r.loglik[b, c]):
            assert v == 0.0 and not np.signbit(v), (b, c, v)
        assert np.all(r.nis_lm[b, c] == 0.0) and np.all(r.used[b, c] == 0)
    assert r.info[0, 2] == 0 and r.dof[0, 2] == 14 and r.nis[0, 2] > 0.0
    fg.close()
    # the Python facade with ragged lists
    f = vf.VIOFilter(hip.settings_from_dict(sc.settings()), capacity=sc.CAPACITY)
    f.batch.restore_state(snapshots(hip)[2], 0)
    ids, y, slots = c2[0]
    got = f.score(vf.VisionMeasurement(0.0, ids, y), want_lm=True)
    assert got["info"] == 0 and got["dof"] == 14 and got["nis"] == r.nis[0, 2] and got["loglik"] == r.loglik[0, 2]
    assert got["used"].sum() == 7 and len(got["nis_lm"]) == len(ids)
    assert f.scoreVisionData(vf.VisionMeasurement(0.0, np.zeros(0, dtype=np.int32), np.zeros((0, 3))))["dof"] == 0
