"""Explicit landmark removal and insertion with priors on the device (csrc/eqf_mapedit.hpp: eqf_edit_landmarks, FilterBatch.edit_landmarks /
remove_landmarks / insert_landmarks).

The reference of every claim is the HOST ROUTE on a twin handle: dump_state before the call, the edit applied in numpy
(consistency.edit_landmarks_host), restore_state -- which tests/test_replay.py pins as a bitwise resume and which shares no code with the
device path.  "Same" is bit for bit (the bytes of every array) on every getter; there are no tolerances.

Shapes: capacity 96, landmark counts 0 / 1 / 2 / 21 / 85 / 86 (85 landmarks: n = 12 + 3 * 85 = 267, just past one 256-thread row chunk), a
single filter and ragged batches of three, after five frames of a synthetic stream in which every fourth landmark leaves and comes back: Sigma
is dense, the group elements are not the identity and the state's order is not ascending.

Whether an insert-only call leaves Sigma in its buffer, and the kept entries unwritten, cannot be seen through debug_sigma_pad (it reports
the pad row of the CURRENT image only): that was checked by reading k_mapedit_append and eqf_edit_landmarks, which flips pS only when
something is removed."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAP = 96
NAN = float("nan")


@pytest.fixture(scope="module")
def hip():
    from eqf_vio_amd import binding

    return binding


@pytest.fixture(scope="module")
def cons():
    from eqf_vio_amd import consistency

    return consistency


@pytest.fixture(scope="module")
def stream():
    from eqf_vio_amd import synth

    return synth.make_stream(86, duration=0.6)  # 11 vision frames


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


def _frame(st, k, counts, thin):
    """Frame k for filters that track the first counts[b] landmarks; `thin`: every fourth of them (from the second) is not seen."""
    stride = max(max(counts), 1)
    ids, y, nb = np.zeros((len(counts), stride), dtype=np.int32), np.zeros((len(counts), stride, 3)), []
    y[:, :, 2] = 1.0
    for b, n in enumerate(counts):
        sel = [i for i in range(n) if not (thin and i % 4 == 1)]
        ids[b, :len(sel)], y[b, :len(sel)] = st.ids[sel], st.bearings[k][sel]
        nb.append(len(sel))
    return ids, y, nb


_SOURCES = {}


def _source(hip, st, counts, precision=None):
    """A handle whose filters hold counts[b] landmarks after five frames, the third without every fourth landmark (they come back at the
    END of the state).  Built once per shape; the tests work on copies (eqf_copy_filters: bitwise)."""
    key = (tuple(counts), precision)
    if key not in _SOURCES:
        kw = {} if precision is None else dict(precision=precision)
        fg = hip.FilterBatch(_settings(), capacity=CAP, batch=len(counts), **kw)
        for kind, k in _events(st, 0, 5):
            if kind == "imu":
                r = st.imu[k]
                fg.process_imu(r[0], r[1:4], r[4:7])
            else:
                ids, y, nb = _frame(st, k, counts, thin=(k == 2))
                fg.process_vision(st.vision_stamps[k], ids, y, nb=nb)
        assert [fg.num_landmarks(b) for b in range(len(counts))] == list(counts)
        assert fg.device_error() == 0
        if max(counts) >= 21:
            big = int(np.argmax(counts))
            assert np.any(np.diff(fg.ids(big)) < 0), "the state's order should not be ascending"
        _SOURCES[key] = fg
    return _SOURCES[key]


def _copy(hip, src, precision=None, **settings):
    kw = {} if precision is None else dict(precision=precision)
    fg = hip.FilterBatch(_settings(**settings), capacity=src.cap, batch=src.B, **kw)
    fg.copy_filters(src, list(range(src.B)), list(range(src.B)))
    return fg


def _sweep(fg, b, f64=True):
    g = dict(n=fg.num_landmarks(b), ids=fg.ids(b), est=fg.state_estimate(b), origin=fg.origin(b), group=fg.group(b), bias=fg.bias(b),
             sigma=fg.sigma(b), time=fg.get_time()[b])
    if f64:
        g.update(marg_origin=fg.marginals(b, local=False), marg_local=fg.marginals(b, local=True), jac=fg.local_jacobian(b))
    return g


def _bits(x):
    if isinstance(x, dict):
        return {k: _bits(v) for k, v in x.items()}
    return np.ascontiguousarray(x).tobytes() + str(np.asarray(x).shape).encode()


def _assert_same(a, b, what):
    a, b = _bits(a), _bits(b)
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k], f"{what}: {k} differs"


def _prior(seed, n):
    """n positions in front of the camera and n full covariances (only their lower triangles count)."""
    r = np.random.default_rng(seed)
    p = np.column_stack([r.uniform(-1.5, 1.5, n), r.uniform(-1.0, 1.0, n), r.uniform(2.0, 9.0, n)])
    a = r.standard_normal((n, 3, 3)) * 0.2
    P = a @ np.transpose(a, (0, 2, 1)) + 0.01 * np.eye(3)
    P[:, 0, 1], P[:, 0, 2], P[:, 1, 2] = 7.0, -3.0, NAN  # (the upper triangle is never read)
    return p, P


NONE = (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros((0, 3)), np.zeros((0, 3, 3)))


def _edit_and_twin(hip, cons, src, edits, precision=None, **settings):
    """The device call on a copy of src and the host route on another: (handle, twin, removed, inserted, snapshots before)."""
    fg, tw = _copy(hip, src, precision, **settings), _copy(hip, src, precision, **settings)
    before = [fg.dump_state(b) for b in range(fg.B)]
    removed, inserted = fg.edit_landmarks(remove=[e[0] for e in edits], insert=[(e[1], e[2], e[3]) for e in edits])
    for b, e in enumerate(edits):
        new, r, i = cons.edit_landmarks_host(before[b], *e)
        assert removed[b].tobytes() == r.tobytes() and inserted[b].tobytes() == i.tobytes(), f"verdicts of filter {b}"
        if len(e[0]) or len(e[1]):
            tw.restore_state(new, b)
    return fg, tw, removed, inserted, before


def _compare(fg, tw, what, f64=True):
    for b in range(fg.B):
        _assert_same(_sweep(fg, b, f64), _sweep(tw, b, f64), f"{what}, filter {b}")
    assert fg.device_error() == 0 and tw.device_error() == 0


# ---- 1. remove only
def _remove_sets(ids):
    s = sorted(int(x) for x in ids)
    n = len(s)
    out = {"first in the state": [int(ids[0])] if n else [], "last in the state": [int(ids[-1])] if n else [],
           "an interior run": sorted(int(x) for x in ids[n // 3:n // 3 + max(1, n // 4)]), "every second": s[::2], "all": s,
           "none present": [1000, 1001, 1005], "present and absent": sorted(s[1::3] + [2000, 2001])}
    return out


@pytest.mark.parametrize("n", [0, 1, 2, 21, 85, 86])
def test_remove_only(hip, cons, stream, n):
    src = _source(hip, stream, [n])
    ids = src.ids(0)
    for what, rem in _remove_sets(ids).items():
        fg, tw, removed, _, before = _edit_and_twin(hip, cons, src, [(np.array(rem, dtype=np.int32),) + NONE[1:]])
        _compare(fg, tw, f"N = {n}, remove {what}")
        assert removed[0].tolist() == [int(r in set(ids.tolist())) for r in rem]
        assert fg.ids(0).tolist() == [int(x) for x in ids if int(x) not in set(rem)]
        if what == "none present":
            _assert_same(_sweep(fg, 0), _sweep(src, 0), "nothing named is there: nothing changes")
        assert fg.remove_landmarks([rem])[0].tolist() == [0] * len(rem)  # (they are gone now; the thin form of the call)


# ---- 2. insert only
@pytest.mark.parametrize("n,k", [(0, 1), (0, 7), (1, 1), (2, 7), (21, 1), (21, 7), (85, 7), (86, 1), (86, 10), (0, 96)],
                         ids=lambda v: str(v))
def test_insert_only(hip, cons, stream, n, k):
    src = _source(hip, stream, [n])
    p, P = _prior(100 + k, k)
    new_ids = np.arange(500, 500 + k, dtype=np.int32)
    fg, tw, _, inserted, before = _edit_and_twin(hip, cons, src, [(NONE[0], new_ids, p, P)])
    assert inserted[0].tolist() == [1] * k and fg.num_landmarks(0) == n + k
    _compare(fg, tw, f"N = {n}, insert {k}")
    low = np.tril(P) + np.transpose(np.tril(P, -1), (0, 2, 1))
    assert fg.marginals(0, local=False)["lm"][n:].tobytes() == low.tobytes()   # P's mirrored lower triangle, exactly
    assert fg.origin(0)["p"][n:].tobytes() == p.tobytes()
    assert fg.state_estimate(0)["p"][n:].tobytes() == p.tobytes()
    g = fg.group(0)
    assert g["Qq"][n:].tobytes() == np.tile([1.0, 0.0, 0.0, 0.0], (k, 1)).tobytes() and g["Qa"][n:].tobytes() == np.ones(k).tobytes()
    S, S0 = fg.sigma(0), before[0]["sigma"]
    m = 11 + 3 * n
    assert S[:m, :m].tobytes() == np.ascontiguousarray(S0).tobytes()  # the kept part, every bit
    assert not S[m:, :m].any() and not S[:m, m:].any()
    assert S[m:, :].tobytes() == S[:, m:].T.copy().tobytes()  # the new rows are the new columns, bit for bit
    assert fg.debug_sigma_pad(0) == 0.0
    assert fg.insert_landmarks([(new_ids, p, P)])[0].tolist() == [0] * k  # (they are there now; the thin form of the call)


# ---- 3. both, with a replace, rejected entries and an id that is already there
@pytest.mark.parametrize("n", [2, 21, 85, 86])
def test_remove_and_insert_in_one_call(hip, cons, stream, n):
    src = _source(hip, stream, [n])
    ids = src.ids(0)
    s = sorted(int(x) for x in ids)
    rem = sorted(set(s[::3]) | {3000})
    replaced, present = s[0], s[1]  # s[0] is removed and comes back; s[1] stays, so naming it is verdict 0
    ins = sorted([replaced, present, 600, 601, 602, 603])
    p, P = _prior(7, len(ins))
    p[ins.index(601)] = [0.5, NAN, 3.0]
    P[ins.index(602)] = np.array([[1.0, 0, 0], [0, 1.0, 0], [2.0, 0, 3.0]])  # third pivot 3 - 4 < 0
    want = [1 if i in (replaced, 600, 603) else (0 if i == present else 2) for i in ins]
    fg, tw, removed, inserted, _ = _edit_and_twin(hip, cons, src, [(np.array(rem, dtype=np.int32), np.array(ins, dtype=np.int32), p, P)])
    assert inserted[0].tolist() == want and removed[0].tolist() == [int(r in set(s)) for r in rem]
    _compare(fg, tw, f"N = {n}, remove and insert")
    got = fg.ids(0).tolist()
    assert got[-3:] == [replaced, 600, 603] and 601 not in got and 602 not in got and got.count(present) == 1
    S = fg.sigma(0)
    m = S.shape[0] - 9
    assert np.all(np.isfinite(S)) and S[m:, :].tobytes() == S[:, m:].T.copy().tobytes()  # nothing of the rejected entries shows
    assert np.all(np.isfinite(fg.origin(0)["p"]))


# ---- 4. a batch: idle, remove everything, remove and fill to capacity
@pytest.mark.parametrize("counts", [[21, 85, 86], [86, 2, 0], [1, 21, 85]], ids=lambda c: "-".join(map(str, c)))
def test_batch_of_three(hip, cons, stream, counts):
    src = _source(hip, stream, counts)
    ids = [src.ids(b) for b in range(3)]
    rem2 = sorted(int(x) for x in ids[2][1::2])
    k2 = CAP - (counts[2] - len(rem2))
    p, P = _prior(21, k2)
    edits = [NONE, (np.array(sorted(int(x) for x in ids[1]), dtype=np.int32),) + NONE[1:],
             (np.array(rem2, dtype=np.int32), np.arange(700, 700 + k2, dtype=np.int32), p, P)]
    fg, tw, removed, inserted, before = _edit_and_twin(hip, cons, src, edits)
    _compare(fg, tw, f"batch {counts}")
    assert [fg.num_landmarks(b) for b in range(3)] == [counts[0], 0, CAP]
    _assert_same(_sweep(fg, 0), _sweep(src, 0), "the idle filter keeps every bit although Sigma changed buffers")
    # the same filters alone in a handle: the same bits (nothing depends on the position in the batch)
    for b in (1, 2):
        alone = hip.FilterBatch(_settings(), capacity=CAP, batch=1)
        alone.copy_filters(src, [0], [b])
        _assert_same(_sweep(alone, 0), _sweep(src, b), f"filter {b} copied into a handle of its own")
        r1, i1 = alone.edit_landmarks(remove=[edits[b][0]], insert=[edits[b][1:]])
        assert r1[0].tobytes() == removed[b].tobytes() and i1[0].tobytes() == inserted[b].tobytes()
        _assert_same(_sweep(alone, 0), _sweep(fg, b), f"filter {b} alone")


# ---- 5. going on after the edit
def _continue(cons, fg, st, new_id, stereo_ids):
    """15 IMU samples, stereo rows on a subset, one vision frame naming every id plus a new one, then forecast, scores and NEES."""
    out = {}
    imu = [k for kind, k in _events(st, 5, 8) if kind == "imu"]
    for k in imu[:15]:
        r = st.imu[k]
        fg.process_imu(r[0], r[1:4], r[4:7])
    q21, t21 = np.array([0.9998, 0.01, -0.015, 0.005]), np.array([0.12, 0.002, -0.004])
    q21 = q21 / np.linalg.norm(q21)
    R21 = cons.quat_to_matrix(q21)
    lists = []
    for b in range(fg.B):
        ids_b = fg.ids(b).tolist()
        est = fg.state_estimate(b)["p"]
        sel = sorted(i for i in stereo_ids[b] if i in ids_b)
        H, res = [], []
        for i in sel:
            ph = est[ids_b.index(i)]
            truth = ph * (1.0 + 0.01 * ((i % 5) - 2))  # where the second camera "saw" it: a few percent along the ray
            p2 = R21.T @ (truth - t21)
            h, r = cons.stereo_rows(ph, q21, t21, p2 / np.linalg.norm(p2))
            H.append(h), res.append(r)
        lists.append((np.array(sel, dtype=np.int32), np.array(H).reshape(-1, 2, 3), np.array(res).reshape(-1, 2)))
    out["stereo"] = fg.update_landmarks([l[0] for l in lists], [l[1] for l in lists], [l[2] for l in lists],
                                        [1e-4 * np.eye(2)] * fg.B, rows=2, local=True)
    out["after_stereo"] = [_sweep(fg, b) for b in range(fg.B)]
    stamp = st.imu[imu[14]][0] + 0.001
    stride = max(fg.num_landmarks(b) for b in range(fg.B)) + 1
    vid, vy, nb = np.zeros((fg.B, stride), dtype=np.int32), np.zeros((fg.B, stride, 3)), []
    vy[:, :, 2] = 1.0
    for b in range(fg.B):
        ids_b = fg.ids(b).tolist()
        est = fg.state_estimate(b)["p"]
        named = sorted(ids_b + [new_id])
        for j, i in enumerate(named):
            ph = est[ids_b.index(i)] if i in ids_b else np.array([0.3, -0.2, 4.0])
            ph = ph + 1e-3 * np.array([((i * 7) % 5) - 2, ((i * 3) % 7) - 3, 0.0])
            vid[b, j], vy[b, j] = i, ph / np.linalg.norm(ph)
        nb.append(len(named))
    out["vision_status"] = fg.process_vision(stamp, vid, vy, nb=nb)
    out["after_vision"] = [_sweep(fg, b) for b in range(fg.B)]
    out["last"] = [fg.last_update(b) for b in range(fg.B)]
    fc = fg.forecast(imu=st.imu[imu[15]:imu[15] + 3], t1=st.imu[imu[15] + 2][0] + 0.002)
    out["forecast"] = {k: (v if k == "status" else [np.array(x) for x in v]) for k, v in fc.items()}
    sc = fg.score_vision(vid[:, None, :], vy[:, None, :, :], nb=np.array(nb).reshape(-1, 1))
    out["score"] = {k: getattr(sc, k) for k in ("nis", "logdet_S", "loglik", "dof", "info")}
    out["nees"] = fg.nees(None, local=True)
    out["err"] = fg.device_error()
    return out


def _flat(x, pre=""):
    if isinstance(x, dict):
        for k, v in x.items():
            yield from _flat(v, f"{pre}.{k}")
    elif isinstance(x, (list, tuple)):
        for j, v in enumerate(x):
            yield from _flat(v, f"{pre}[{j}]")
    else:
        yield pre, np.ascontiguousarray(x).tobytes() + str(np.asarray(x).shape).encode()


@pytest.mark.parametrize("lift", [0, 1], ids=["plain lift", "innovation_lift"])
def test_every_later_call_gives_the_twins_bits(hip, cons, stream, lift):
    counts = [21, 85, 2]
    src = _source(hip, stream, counts)
    edits, stereo = [], []
    for b in range(3):
        s = sorted(int(x) for x in src.ids(b))
        rem = s[::4] if b != 2 else []
        k = 5 if b != 1 else CAP - 1 - (counts[b] - len(rem))  # (filter 1 up to one below the capacity: the frame brings one more)
        p, P = _prior(31 + b, k)
        edits.append((np.array(rem, dtype=np.int32), np.arange(800, 800 + k, dtype=np.int32), p, P))
        stereo.append([800, 802, 804] + s[1:9:2])
    fg, tw, _, _, _ = _edit_and_twin(hip, cons, src, edits)
    for h in (fg, tw):
        h.set_option("innovation_lift", lift)
    _compare(fg, tw, "before going on")
    a, t = _continue(cons, fg, stream, 900, stereo), _continue(cons, tw, stream, 900, stereo)
    fa, ft = dict(_flat(a)), dict(_flat(t))
    assert fa.keys() == ft.keys()
    for k in fa:
        assert fa[k] == ft[k], f"{k} differs from the twin's"
    assert a["err"] == 0 and np.all(a["vision_status"] == 0)
    if lift == 0:
        assert np.all(a["stereo"]["info"] == 0), a["stereo"]["info"]
        assert np.all(a["stereo"]["used"][0, :7] == 1)  # three inserted landmarks and four old ones were measured
    assert [fg.num_landmarks(b) for b in range(3)][1] == CAP and 900 in fg.ids(0).tolist()


# ---- 6. an EQF_PRECISION_F32 handle
def test_f32_handle(hip, cons, stream):
    src = _source(hip, stream, [85, 21], precision=hip.PRECISION_F32)
    edits = []
    for b in range(2):
        s = sorted(int(x) for x in src.ids(b))
        p, P = _prior(41 + b, 6)
        edits.append((np.array(s[1::3], dtype=np.int32), np.array([s[1], 810, 811, 812, 813, 814], dtype=np.int32), p, P))
    fg, tw, _, inserted, _ = _edit_and_twin(hip, cons, src, edits, precision=hip.PRECISION_F32)
    assert inserted[0].tolist() == [1] * 6
    _compare(fg, tw, "fp32 handle", f64=False)
    low = np.tril(P) + np.transpose(np.tril(P, -1), (0, 2, 1))
    S = fg.sigma(1)
    assert S[-3:, -3:].tobytes() == low[-1].astype(np.float32).astype(np.float64).tobytes()  # P rounded to the handle's precision
    # insert only, in place
    p, P = _prior(43, 3)
    e2 = [(NONE[0], np.array([820, 821, 822], dtype=np.int32), p, P), NONE]
    fg2, tw2, _, _, _ = _edit_and_twin(hip, cons, fg, e2, precision=hip.PRECISION_F32)
    _compare(fg2, tw2, "fp32 handle, insert only", f64=False)


# ---- 7. past any bound a list in LDS would have
def test_large_state(hip, cons):
    N = 1030
    r = np.random.default_rng(5)
    fg = hip.FilterBatch(_settings(), capacity=N + 4, batch=1)
    snap = fg.dump_state(0)
    ids = r.permutation(np.arange(10, 10 + N)).astype(np.int32)
    a = r.standard_normal((11 + 3 * N, 24))
    snap.update(ids=ids, sigma=a @ a.T * 1e-3 + np.diag(r.uniform(0.5, 1.5, 11 + 3 * N)), initialised=1)
    half = 0.55  # (a pose away from the identity, whose gravity direction sits on the pole of its own chart)
    snap["origin"]["q"] = np.concatenate([[np.cos(half)], np.sin(half) * np.array([0.3, 1.0, -0.2]) / np.linalg.norm([0.3, 1.0, -0.2])])
    snap["origin"]["p"] = np.column_stack([r.uniform(-2, 2, N), r.uniform(-2, 2, N), r.uniform(2, 9, N)])
    snap["group"]["Qq"] = np.tile([1.0, 0.0, 0.0, 0.0], (N, 1))
    snap["group"]["Qa"] = r.uniform(0.8, 1.25, N)
    fg.restore_state(snap, 0)
    assert fg.device_error() == 0
    before = fg.dump_state(0)
    rem = np.array(sorted(int(x) for x in ids[::3]), dtype=np.int32)
    p, P = _prior(51, 5)
    new_ids = np.arange(5000, 5005, dtype=np.int32)
    removed, inserted = fg.edit_landmarks(remove=[rem], insert=[(new_ids, p, P)])
    assert removed[0].all() and inserted[0].tolist() == [1] * 5
    want, _, _ = cons.edit_landmarks_host(before, rem, new_ids, p, P)
    assert fg.ids(0).tobytes() == want["ids"].tobytes()
    assert fg.sigma(0).tobytes() == np.ascontiguousarray(want["sigma"]).tobytes()
    assert fg.origin(0)["p"].tobytes() == np.ascontiguousarray(want["origin"]["p"]).tobytes()
    assert fg.device_error() == 0


# ---- 8. argument errors leave the handle untouched
def test_argument_errors_change_nothing(hip, stream):
    import ctypes as C

    src = _source(hip, stream, [21, 85, 86])
    fg = _copy(hip, src)
    before = [_sweep(fg, b) for b in range(3)]
    p, P = _prior(61, 12)
    ok_ins = (np.arange(900, 905, dtype=np.int32), p[:5], P[:5])
    none_ins = (np.zeros(0, dtype=np.int32), p[:0], P[:0])
    s = sorted(int(x) for x in fg.ids(0))
    cases = {
        "unsorted removals": (dict(remove=[[s[3], s[2]], [], []], insert=[ok_ins, none_ins, none_ins]), "UNSORTED"),
        "duplicate insertions": (dict(remove=[[s[2]], [], []], insert=[none_ins, (np.array([900, 900], dtype=np.int32), p[:2], P[:2]), none_ins]),
                                 "UNSORTED"),
        "over capacity": (dict(remove=[[s[2]], [], []], insert=[ok_ins, none_ins, (np.arange(900, 911, dtype=np.int32), p[:11], P[:11])]),
                          "CAPACITY"),
    }
    for what, (kw, name) in cases.items():
        with pytest.raises(hip.EqfError) as e:
            fg.edit_landmarks(**kw)
        assert e.value.code == dict(UNSORTED=hip.ERR_UNSORTED, CAPACITY=hip.ERR_CAPACITY)[name], what
        for b in range(3):
            _assert_same(_sweep(fg, b), before[b], f"{what}: filter {b}")
    # a NULL list with a count, and a count beyond the stride: only the C ABI can say that
    L = hip.lib()
    ip, up = C.POINTER(C.c_int), C.POINTER(C.c_ubyte)
    nr = np.array([1, 0, 0], dtype=np.int32)
    rid = np.array([[s[0]], [0], [0]], dtype=np.int32)
    assert L.eqf_edit_landmarks(fg._h, nr.ctypes.data_as(ip), None, 1, None, None, 0, None, None, None, None) == -1
    nr2 = np.array([2, 0, 0], dtype=np.int32)
    assert L.eqf_edit_landmarks(fg._h, nr2.ctypes.data_as(ip), rid.ctypes.data_as(ip), 1, None, None, 0, None, None, None, None) == -1
    assert L.eqf_edit_landmarks(None, nr.ctypes.data_as(ip), rid.ctypes.data_as(ip), 1, None, None, 0, None, None, None, None) == -1
    for b in range(3):
        _assert_same(_sweep(fg, b), before[b], f"NULL list / count beyond the stride: filter {b}")
    # ... and the same arrays with the right count do remove the landmark
    out = np.zeros((3, 1), dtype=np.uint8)
    assert L.eqf_edit_landmarks(fg._h, nr.ctypes.data_as(ip), rid.ctypes.data_as(ip), 1, None, None, 0, None, None, out.ctypes.data_as(up), None) == 0
    assert out[0, 0] == 1 and s[0] not in fg.ids(0).tolist() and fg.num_landmarks(0) == 20


# ---- 9. the device's own flag
def test_landmark_on_the_chart_pole_raises_bit_16(hip, cons, stream):
    """landmarkConstants rotates -p0 / |p0| onto e3 (sphereRotQ = SO3FromVectors(-pole, e3)): the half turn, where that rotation is not
    defined, is p0 along +e3, the optical axis -- tests/lie_edge_cases.pole_directions at theta = 0.  Such a landmark is finite, not zero
    and has a fine prior: the host accepts it, the device raises bit 16, as for a new landmark of a vision frame.  The other filters of
    the handle are not touched."""
    import lie_edge_cases as ec

    pole = ec.pole_directions((0.0,))[0][2]
    assert pole.tolist() == [0.0, 0.0, 1.0]
    src = _source(hip, stream, [21, 85, 86])
    fg = _copy(hip, src)
    before = [_sweep(fg, b) for b in range(3)]
    p, P = _prior(71, 2)
    p[1] = 4.0 * pole
    verdict = fg.insert_landmarks([None, (np.array([950, 951], dtype=np.int32), p, P), None])
    assert verdict[1].tolist() == [1, 1]
    assert fg.device_error() == 16
    for b in (0, 2):
        _assert_same(_sweep(fg, b), before[b], f"filter {b} beside the flagged one")
    assert fg.origin(1)["p"][-1].tolist() == [0.0, 0.0, 4.0] and fg.num_landmarks(1) == 87


# ---- the call settles what the handle has deferred before it decides anything
def test_deferred_work_is_settled_first(hip, stream):
    """The call directly behind six queued IMU calls, and directly behind a vision call whose gate answer is pending (an outlier frame:
    the gate changes the id lists the verdicts are decided on), no getter in between -- against the same sequence with synchronize()
    in front of every edit."""
    from eqf_vio_amd import synth

    st = stream
    meas = synth.churn_measurements(st, seed=7, outlier_frames=(6, 8), outlier_angle=0.05)
    p, P = _prior(81, 4)
    rem = np.array(sorted(int(x) for x in st.ids[::5]), dtype=np.int32)
    got = []
    for sync in (False, True):
        fg = hip.FilterBatch(_settings(outlierThreshold=0.01), capacity=CAP, batch=2)
        for kind, k in _events(st, 0, 5):
            if kind == "imu":
                fg.process_imu(st.imu[k][0], st.imu[k][1:4], st.imu[k][4:7])
            else:
                fg.process_vision(st.vision_stamps[k], *meas[k])
        ev = _events(st, 5, 7)
        nv = [i for i, e in enumerate(ev) if e[0] == "vision"]
        assert nv[0] >= 6 and nv[1] - nv[0] > 6
        res = []
        for i, (kind, k) in enumerate(ev[: nv[0]]):  # frame 5 without its vision call: the last six IMU calls are queued, not launched
            if i == nv[0] - 6:
                fg.synchronize()
            fg.process_imu(st.imu[k][0], st.imu[k][1:4], st.imu[k][4:7])
        if sync:
            fg.synchronize()
        res.append(fg.edit_landmarks(remove=[rem, rem[:3]], insert=[(np.arange(900, 904, dtype=np.int32), p, P), None]))
        res.append([_sweep(fg, b) for b in range(2)])
        fg.process_vision(st.vision_stamps[5], *meas[5])
        for kind, k in ev[nv[0] + 1: nv[1]]:
            fg.process_imu(st.imu[k][0], st.imu[k][1:4], st.imu[k][4:7])
        fg.process_vision(st.vision_stamps[6], *meas[6])  # an outlier frame, its gate answer pending
        if sync:
            fg.synchronize()
        everything = np.arange(0, 1000, dtype=np.int32)
        res.append(fg.edit_landmarks(remove=[everything[1::2], None], insert=[None, (np.arange(900, 904, dtype=np.int32), p, P)]))
        res.append([_sweep(fg, b) for b in range(2)])
        assert fg.device_error() == 0
        got.append(res)
    fa, ft = dict(_flat(got[0])), dict(_flat(got[1]))
    assert fa.keys() == ft.keys()
    for k in fa:
        assert fa[k] == ft[k], f"{k}: deferred against synchronised"
    assert got[0][0][0][0].any() and got[0][2][0][0].any()  # both edits did remove something
