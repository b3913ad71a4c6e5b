"""The Schmidt (consider) updates on the device (csrc/eqf_schmidt.hpp: eqf_update_linear_schmidt / eqf_update_landmarks_schmidt;
FilterBatch.update_linear / update_landmarks with consider=...).  The yardstick is the library's own FULL update on a fork of the same
filter, bit for bit: from a handle H0 with a filter's own Sigma (five frames of a synthetic stream) three forks are made with
eqf_copy_filters -- A gets the Schmidt call, F the full call with identical arguments, G eqf_apply_increment with the gamma A returned.
Then Sigma(A) has F's bits at every entry outside c x c and H0's inside, is bitwise symmetric, gamma(A) is F's off c and +0.0 on c, report
and `used` are F's, and the state of A has G's bits.  The shapes are the gathered downdate's edges: N = 22 (two column tiles, one ragged
active row tile of 18), N = 43 (three column tiles, 78 active rows: two row tiles, the second ragged, active triples across a tile edge),
m = 80 (two 64-chunks of k), m = 1 and 16 for the linear call.  Nothing here provokes a fault: the indefinite S and the indefinite
Sigma_e are ordinary numeric verdicts."""
import ctypes as C

import numpy as np
import pytest

import lift_cases as lc

pytestmark = pytest.mark.gpu
SIZES = (5, 22, 43)
ABSENT = 5000


@pytest.fixture(scope="module")
def hip():
    from eqf_vio_amd import binding

    return binding


@pytest.fixture(scope="module")
def h0(hip):
    """{N: a one-filter handle after five vision frames of a synthetic stream}"""
    from eqf_vio_amd import synth

    out = {}
    for N in SIZES:
        st = synth.make_stream(N, duration=0.4)
        fg = hip.FilterBatch(lc.settings(1), capacity=N + 2, batch=1)
        seen = 0
        for kind, k in st.events():
            if kind == "imu":
                r = st.imu[k]
                fg.process_imu(r[0], r[1:4], r[4:7])
            else:
                fg.process_vision(st.vision_stamps[k], st.ids, st.bearings[k])
                seen += 1
                if seen == 5:
                    break
        assert fg.num_landmarks(0) == N and fg.device_error() == 0
        # (a vision frame leaves Sigma symmetric to rounding only, and the Schmidt call keeps every bit of Sigma_cc, both triangles: H0 gets
        # its own lower triangle mirrored, as the snapshots of the other GPU tests do, so that "bitwise symmetric" can be asked of the result)
        S = fg.sigma(0)
        fg.set_sigma(np.tril(S) + np.tril(S, -1).T, 0)
        S = fg.sigma(0)
        assert S.tobytes() == np.ascontiguousarray(S.T).tobytes()
        out[N] = fg
    yield out
    for fg in out.values():
        fg.close()


def _bits(x):
    if isinstance(x, dict):
        return {k: _bits(v) for k, v in x.items()}
    return np.ascontiguousarray(x).tobytes() + str(np.asarray(x).shape).encode()


def _state(fg, b=0):
    """state estimate, origin, group, bias and time"""
    return _bits(dict(est=fg.state_estimate(b), origin=fg.origin(b), group=fg.group(b), bias=fg.bias(b), time=fg.get_time()[b]))


def _all(fg, b=0):
    return _bits(dict(est=fg.state_estimate(b), n=fg.num_landmarks(b), **fg.dump_state(b)))


def _fork(hip, srcs, lift=0, cap=None):
    """a handle whose filter b is a copy of the one-filter handle srcs[b]"""
    cap = cap or max(s.num_landmarks(0) for s in srcs) + 2
    fg = hip.FilterBatch(lc.settings(1), capacity=cap, batch=len(srcs))
    for b, s in enumerate(srcs):
        fg.copy_filters(s, [b], [0])
    if lift:
        fg.set_option("innovation_lift", 1)
    return fg


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _cidx(ids, consider):
    """reference-map state indices of the consider ids the state holds"""
    cs_ = set(int(i) for i in consider)
    return np.array([11 + 3 * i + k for i, lid in enumerate(ids) if int(lid) in cs_ for k in range(3)], dtype=np.int64)


def _lm_ops(fg, b, lms, seed, gated=(), absent=False, rows=2):
    """entries on the landmarks lms (indices) of filter b: ids ascending, H random, R a multiple of the identity, resid inside its own sigma
    (a gated entry a thousand times that); the origin chart's sizes (local = 0 gates by them)"""
    ids_all = fg.ids(b)
    S = fg.sigma(b)
    rng = np.random.default_rng([2702, seed, len(lms)])
    order = np.argsort(ids_all[list(lms)]) if len(lms) else []
    lms = [lms[i] for i in order]
    ids = [int(ids_all[i]) for i in lms]
    K = len(lms)
    H = rng.standard_normal((K, rows, 3))
    R = np.zeros((K, rows, rows))
    r = np.zeros((K, rows))
    for k, i in enumerate(lms):
        P = H[k] @ S[11 + 3 * i:14 + 3 * i, 11 + 3 * i:14 + 3 * i] @ H[k].T
        R[k] = float(np.mean(np.diag(P))) * np.eye(rows)
        r[k] = 0.3 * np.sqrt(np.diag(P + R[k])) * rng.standard_normal(rows) * (1000.0 if k in gated else 1.0)
    if absent:
        ids, H, R, r = ids + [ABSENT], np.concatenate([H, H[:1]]), np.concatenate([R, R[:1]]), np.concatenate([r, r[:1]])
    return dict(ids=np.array(ids, dtype=np.int32), H=H, resid=r, R=R, rows=rows)


def _lin_ops(fg, b, m, lms, seed):
    """m dense rows on the velocity and the landmarks lms"""
    N = fg.num_landmarks(b)
    S = fg.sigma(b)
    rng = np.random.default_rng([2703, seed, m])
    H = np.zeros((m, 11 + 3 * N))
    cols = [8, 9, 10] + [11 + 3 * i + k for i in lms for k in range(3)]
    H[:, cols] = rng.standard_normal((m, len(cols)))
    P = H @ S @ H.T
    R = float(np.mean(np.diag(P))) * np.eye(m)
    return dict(H=H, resid=0.3 * np.sqrt(np.diag(P + R)) * rng.standard_normal(m), R=R)


def _call(fg, kind, ops, local, consider, **kw):
    """ops, consider: one per filter"""
    if kind == "linear":
        return fg.update_linear([o["H"] for o in ops], [o["resid"] for o in ops], [o["R"] for o in ops], local=bool(local), want_gamma=True,
                                consider=consider, **kw)
    return fg.update_landmarks([o["ids"] for o in ops], [o["H"] for o in ops], [o["resid"] for o in ops], [o["R"] for o in ops],
                               rows=ops[0]["rows"], local=bool(local), consider=consider, **kw)


REPORT = ("nis", "logdet_S", "loglik", "dof", "info")


def _same_report(a, f, b=0):
    for k in REPORT:
        assert _bits(a[k][b]) == _bits(f[k][b]), k
    if "used" in f:
        assert _bits(a["used"][b]) == _bits(f["used"][b])


def _protocol(hip, src, kind, ops, local, consider, lift=0, expect_move=True, **kw):
    """the three forks and every assertion on them; returns (A's output, Sigma of A, Sigma of H0)"""
    N = src.num_landmarks(0)
    n = 11 + 3 * N
    A, F, G = (_fork(hip, [src], lift) for _ in range(3))
    S0 = src.sigma(0)
    assert _bits(A.sigma(0)) == _bits(S0)
    oa = _call(A, kind, [ops], local, [consider], **kw)
    of = _call(F, kind, [ops], local, None, **kw)
    assert oa["info"][0] == 0 and of["info"][0] == 0, (oa["info"], of["info"])
    G.apply_increment(oa["gamma"][:, :n])
    c = _cidx(src.ids(0), consider)
    SA, SF = A.sigma(0), F.sigma(0)
    inside = np.zeros((n, n), dtype=bool)
    inside[np.ix_(c, c)] = True
    assert np.array_equal(_u64(SA)[~inside], _u64(SF)[~inside]), "outside c x c: not the full call's bits"
    assert np.array_equal(_u64(SA)[inside], _u64(S0)[inside]), "c x c: not H0's bits"
    assert SA.tobytes() == np.ascontiguousarray(SA.T).tobytes(), "Sigma+ is not bit-for-bit symmetric"
    ga, gf = oa["gamma"][0, :n], of["gamma"][0, :n]
    a = np.setdiff1d(np.arange(n), c)
    assert np.array_equal(_u64(ga[a]), _u64(gf[a])) and not _u64(ga[c]).any(), "gamma"
    _same_report(oa, of)
    assert _state(A) == _state(G), "the state of A is not the one eqf_apply_increment with A's gamma leaves"
    if lift:
        ra, rg = A.lift_report(0), G.lift_report(0)
        assert ra["kind"] == rg["kind"] != 0 and ra["info"] == rg["info"] == 0 and _bits(ra["DeltaU"]) == _bits(rg["DeltaU"])
    if expect_move:
        assert not np.array_equal(_u64(SA)[~inside], _u64(S0)[~inside]) and _state(A) != _state(src)
        if len(c):
            assert gf[c].all() and not np.array_equal(_u64(SF)[inside], _u64(S0)[inside]), "the full call does move c"
    for h in (A, F, G):
        assert h.device_error() == 0
        h.close()
    return oa, SA, S0


def _sets(src):
    """the two consider sets of the issue for the handle's size"""
    ids = src.ids(0)
    if len(ids) == 22:
        return [int(i) for k, i in enumerate(ids) if k not in (3, 20)]
    return [int(i) for i in sorted(ids)[1::2]]


# ---- 1. both calls, both charts, the two partitions
@pytest.mark.parametrize("local", (0, 1))
@pytest.mark.parametrize("N", (22, 43))
@pytest.mark.parametrize("kind", ("linear", "landmarks"))
def test_against_the_full_call_bit_for_bit(hip, h0, kind, N, local):
    src = h0[N]
    consider = sorted(_sets(src))
    assert 12 + 3 * (N - len(consider)) == (18 if N == 22 else 78)
    lms = [1, 3, 7, 20] if N == 22 else [0, 1, 2, 20, 21, 41, 42]   # consider and active landmarks
    ops = _lin_ops(src, 0, 3, lms[:3], N) if kind == "linear" else _lm_ops(src, 0, lms, N)
    _protocol(hip, src, kind, ops, local, consider)


# ---- 2. two chunks of k: 40 entries of 2 rows take part, one entry is absent, one over lm_gate
def test_landmarks_two_k_chunks_with_an_absent_and_a_gated_entry(hip, h0):
    src = h0[43]
    consider = sorted(_sets(src))
    ops = _lm_ops(src, 0, list(range(41)), 80, gated=(17,), absent=True)
    oa, _, _ = _protocol(hip, src, "landmarks", ops, 0, consider, lm_gate=60.0)
    used = list(oa["used"][0])
    assert oa["dof"][0] == 80 and used.count(1) == 40 and used[17] == 2 and used[41] == 0, (oa["dof"], used)


# ---- 3. the linear call at m = 1 and m = 16
@pytest.mark.parametrize("m", (1, 16))
def test_linear_m_1_and_16(hip, h0, m):
    src = h0[43]
    oa, _, _ = _protocol(hip, src, "linear", _lin_ops(src, 0, m, [0, 1, 20, 42], m), 1, sorted(_sets(src)))
    assert oa["dof"][0] == m


# ---- 4. the empty set and n_consider = NULL: the full call, every getter
@pytest.mark.parametrize("kind", ("linear", "landmarks"))
def test_empty_set_and_null_are_the_full_call(hip, h0, kind):
    src = h0[22]
    ops = _lin_ops(src, 0, 3, [1, 3], 4) if kind == "linear" else _lm_ops(src, 0, [1, 3, 7, 20], 4)
    A, F, Z = (_fork(hip, [src]) for _ in range(3))
    oa, of = _call(A, kind, [ops], 1, [[]]), _call(F, kind, [ops], 1, None)
    assert _all(A) == _all(F) and _bits(oa["gamma"]) == _bits(of["gamma"]) and _all(A) != _all(src)
    _same_report(oa, of)
    # n_consider == NULL through the C ABI
    L = hip.lib()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    n = 11 + 3 * 22
    rep = (hip.LinearReport * 1)()
    if kind == "linear":
        H, r, R = (np.ascontiguousarray(ops[k]) for k in ("H", "resid", "R"))
        rc = L.eqf_update_linear_schmidt(Z._h, 1, 3, H.ctypes.data_as(dp), n, r.ctypes.data_as(dp), R.ctypes.data_as(dp), float("inf"), None, None,
                                         None, 0, None, 0, rep)
    else:
        K = len(ops["ids"])
        nk = np.array([K], dtype=np.int32)
        H, r, R = (np.ascontiguousarray(ops[k]) for k in ("H", "resid", "R"))
        rc = L.eqf_update_landmarks_schmidt(Z._h, 1, 2, nk.ctypes.data_as(ip), ops["ids"].ctypes.data_as(ip), K, H.ctypes.data_as(dp),
                                            r.ctypes.data_as(dp), R.ctypes.data_as(dp), float("inf"), float("inf"), None, None, None, 0, None, None,
                                            0, rep)
    assert rc == 0 and rep[0].info == 0 and _all(Z) == _all(F) and rep[0].nis == of["nis"][0]
    for h in (A, F, Z):
        assert h.device_error() == 0
        h.close()


# ---- 5. every landmark considered: only the base rows and columns move, no landmark moves
@pytest.mark.parametrize("kind", ("linear", "landmarks"))
def test_every_landmark_considered(hip, h0, kind):
    src = h0[22]
    ops = _lin_ops(src, 0, 3, [1, 3], 5) if kind == "linear" else _lm_ops(src, 0, [1, 3, 7, 20], 5)
    consider = sorted(int(i) for i in src.ids(0))
    A = _fork(hip, [src])
    _call(A, kind, [ops], 0, [consider])
    assert _bits(A.state_estimate(0)["p"]) == _bits(src.state_estimate(0)["p"]), "a consider landmark moved"
    A.close()
    _, SA, S0 = _protocol(hip, src, kind, ops, 0, consider)
    d = _u64(SA) != _u64(S0)
    assert not d[11:, 11:].any() and d[:11, :].any() and d[:11, 11:].any()


# ---- 6. ids the state does not hold are ignored
def test_ids_the_state_does_not_hold_are_ignored(hip, h0):
    src = h0[22]
    consider = sorted(_sets(src))
    more = sorted(consider + [ABSENT, ABSENT + 7, -3])
    ops = _lm_ops(src, 0, [1, 3, 7, 20], 6)
    A, B = _fork(hip, [src]), _fork(hip, [src])
    oa, ob = _call(A, "landmarks", [ops], 1, [consider]), _call(B, "landmarks", [ops], 1, [more])
    assert _all(A) == _all(B) and _bits(oa["gamma"]) == _bits(ob["gamma"]) and oa["info"][0] == 0
    A.close(), B.close()
    _protocol(hip, src, "landmarks", ops, 1, more)


# ---- 7. a ragged batch: alone against its place in the batch, run to run
@pytest.mark.parametrize("kind", ("linear", "landmarks"))
def test_ragged_batch_alone_and_from_run_to_run(hip, h0, kind):
    srcs = [h0[N] for N in SIZES]
    sets = [sorted(int(i) for i in srcs[0].ids(0))[1:3], sorted(_sets(srcs[1])), []]
    lms = [[0, 1, 4], [1, 3, 7, 20], [0, 1, 2, 20, 21, 41, 42]]
    if kind == "linear":
        ops = [_lin_ops(s, 0, 3, l[:3], 7) for s, l in zip(srcs, lms)]
    else:
        ops = [_lm_ops(s, 0, l, 7) for s, l in zip(srcs, lms)]
    kw = dict(stride=7) if kind == "landmarks" else {}
    runs = []
    for _ in range(2):
        fg = _fork(hip, srcs)
        out = _call(fg, kind, ops, 1, sets, **kw)
        assert list(out["info"]) == [0, 0, 0] and fg.device_error() == 0
        runs.append(([_all(fg, b) for b in range(3)], _bits({k: out[k] for k in REPORT + ("gamma",)})))
        fg.close()
    assert runs[0] == runs[1], "second run"
    for b in range(3):
        fa = _fork(hip, [srcs[b]])
        oa = _call(fa, kind, [ops[b]], 1, [sets[b]], **kw)
        n = 11 + 3 * SIZES[b]
        assert _all(fa) == runs[0][0][b], f"filter {b} alone"
        assert _bits(oa["gamma"][0, :n]) == _bits(out["gamma"][b, :n]) and not out["gamma"][b, n:].any()
        _same_report(oa, {k: out[k][b:] for k in REPORT})
        # ... and it is the Schmidt result: the consider block kept H0's bits, the rest moved
        c = _cidx(srcs[b].ids(0), sets[b])
        SA, S0 = fa.sigma(0), srcs[b].sigma(0)
        assert np.array_equal(_u64(SA)[np.ix_(c, c)], _u64(S0)[np.ix_(c, c)]) and not np.array_equal(_u64(SA), _u64(S0))
        assert fa.device_error() == 0
        fa.close()


# ---- 8. filters that must keep every bit
@pytest.mark.parametrize("kind", ("linear", "landmarks"))
def test_masked_gated_indefinite_and_singular_chart_keep_every_bit(hip, h0, kind):
    src = h0[22]
    consider = sorted(_sets(src))
    ops = _lin_ops(src, 0, 3, [1, 3], 8) if kind == "linear" else _lm_ops(src, 0, [1, 3, 7, 20], 8)
    neg = dict(ops, R=-1e6 * np.abs(ops["R"]) - np.eye(ops["R"].shape[-1]))   # S = Ht Sigma Ht^T + R is negative definite
    F = _fork(hip, [src])
    nis = float(_call(F, kind, [ops], 1, None)["nis"][0])
    F.close()
    fg = _fork(hip, [src] * 4)
    before = [_all(fg, b) for b in range(4)]
    # filter 0 masked out, 1 gated by the joint nis, 2 with an indefinite S, 3 applied
    out = _call(fg, kind, [ops, ops, neg, ops], 1, [consider] * 4, gate=0.5 * nis, mask=[0, 1, 1, 0])
    assert list(out["info"]) == [3, 2, 1, 3], out["info"]
    out2 = _call(fg, kind, [ops, ops, neg, ops], 1, [consider] * 4, mask=[0, 0, 0, 1])
    assert list(out2["info"]) == [3, 3, 3, 0]
    for b in range(3):
        assert _all(fg, b) == before[b], f"filter {b}"
        assert not out["gamma"][b].any()
    assert _all(fg, 3) != before[3] and _bits(out["nis"][1]) == _bits(np.float64(nis)) and fg.device_error() == 0
    fg.close()
    # a filter that has not been initialised: the origin's gravity direction is the pole of its own chart (local = 1: info -1)
    f0 = hip.FilterBatch(lc.settings(1), capacity=4, batch=1)
    pre = _all(f0)
    if kind == "linear":
        o = f0.update_linear(np.ones((1, 11)), [0.0], np.eye(1), local=True, want_gamma=True, consider=[[3]])
    else:
        o = f0.update_landmarks([[3]], [np.ones((1, 1, 3))], [np.zeros((1, 1))], [np.eye(1)[None]], rows=1, local=True, consider=[[3]])
    assert o["info"][0] == -1 and not o["gamma"].any() and _all(f0) == pre and f0.device_error() == 0
    f0.close()


# ---- 9. with the handle's innovation lift: the protocol, and a refusal
@pytest.mark.parametrize("kind", ("linear", "landmarks"))
def test_with_the_innovation_lift_and_a_refusal(hip, h0, kind):
    src = h0[22]
    consider = sorted(_sets(src))
    ops = _lin_ops(src, 0, 3, [1, 3], 9) if kind == "linear" else _lm_ops(src, 0, [1, 3, 7, 20], 9)
    _protocol(hip, src, kind, ops, 0, consider, lift=1)
    # Sigma_e indefinite in the last landmark (a consider one); S of the call stays definite: the lift refuses, info 4
    bad = src.dump_state(0)
    S = bad["sigma"].copy()
    S[-1, -1] = -abs(S[-1, -1])
    bad["sigma"] = S
    fg = hip.FilterBatch(lc.settings(1), capacity=24, batch=1)
    fg.restore_state(bad, 0)
    fg.set_option("innovation_lift", 1)
    before = _all(fg)
    out = _call(fg, kind, [ops], 0, [consider])
    assert out["info"][0] == 4 and fg.lift_report(0)["info"] == 4 and not out["gamma"].any()
    assert _all(fg) == before and fg.device_error() == 0
    fg.close()


# ---- 10. argument errors come before any effect
def test_argument_errors_come_before_any_effect(hip, h0):
    src = h0[5]
    fg = _fork(hip, [src, src], cap=6)
    f32 = hip.FilterBatch(lc.settings(1), capacity=6, batch=2, precision=hip.PRECISION_F32)
    L = hip.lib()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    P = lambda a, t=dp: a.ctypes.data_as(t) if a is not None else None  # noqa: E731
    ids = sorted(int(i) for i in src.ids(0))
    n = 11 + 3 * 5
    lin = _lin_ops(src, 0, 2, [0, 1], 10)
    H = np.ascontiguousarray(np.stack([lin["H"]] * 2))
    r = np.ascontiguousarray(np.stack([lin["resid"]] * 2))
    R = np.ascontiguousarray(np.stack([lin["R"]] * 2))
    lm = _lm_ops(src, 0, [0, 1, 4], 10)
    nk = np.array([3, 3], dtype=np.int32)
    lid = np.ascontiguousarray(np.stack([lm["ids"]] * 2))
    Hb, rb, Rb = (np.ascontiguousarray(np.stack([lm[k]] * 2)) for k in ("H", "resid", "R"))
    G = np.full((2, n), -7.0)
    rep = (hip.LinearReport * 2)()
    for s in rep:
        s.nis, s.dof, s.info = -7.0, -7, -7

    def lin_call(h, nc, cid, cstride):
        return L.eqf_update_linear_schmidt(h, 1, 2, P(H), n, P(r), P(R), float("inf"), None, P(nc, ip), P(cid, ip), cstride, P(G), n, rep)

    def lm_call(h, nc, cid, cstride):
        return L.eqf_update_landmarks_schmidt(h, 1, 2, P(nk, ip), P(lid, ip), 3, P(Hb), P(rb), P(Rb), float("inf"), float("inf"), None, P(nc, ip),
                                              P(cid, ip), cstride, None, P(G), n, rep)

    i32 = lambda *v: np.array(v, dtype=np.int32)  # noqa: E731
    good = (i32(2, 1), i32(ids[0], ids[2], 0, ids[1], 0, 0, 0, 0), 4)
    bad = [((i32(2, 2), i32(ids[0], ids[2], 0, 0, ids[3], ids[1], 0, 0), 4), hip.ERR_UNSORTED),
           ((i32(2, 2), i32(ids[0], ids[2], 0, 0, ids[3], ids[3], 0, 0), 4), hip.ERR_UNSORTED),
           ((i32(7, 1), np.arange(14, dtype=np.int32), 7), hip.ERR_CAPACITY),          # beyond the handle's capacity of 6
           ((i32(2, 3), i32(ids[0], ids[2], ids[0], ids[1]), 2), hip.ERR_CAPACITY),    # cstride < n_consider[1]
           ((i32(2, -1), good[1], 4), hip.ERR_INVALID),
           ((i32(2, 1), None, 4), hip.ERR_INVALID)]
    before = [_all(fg, b) for b in range(2)]
    before32 = [_bits(f32.dump_state(b)) for b in range(2)]
    for call in (lin_call, lm_call):
        for args, code in bad:
            assert call(fg._h, *args) == code, (call.__name__, code)
        assert call(None, *good) == hip.ERR_INVALID
        assert call(f32._h, *good) == hip.ERR_UNSUPPORTED
    assert np.all(G == -7.0) and all(s.nis == -7.0 and s.dof == -7 and s.info == -7 for s in rep)
    for b in range(2):
        assert _all(fg, b) == before[b] and _bits(f32.dump_state(b)) == before32[b], b
    assert fg.device_error() == 0 and f32.device_error() == 0
    # good arguments work
    for call in (lin_call, lm_call):
        assert call(fg._h, *good) == 0 and [s.info for s in rep] == [0, 0]
        c = _cidx(src.ids(0), [ids[0], ids[2]])
        assert not G[0, c].any() and G[0, np.setdiff1d(np.arange(n), c)][:11].all()
    assert fg.device_error() == 0
    fg.close(), f32.close()
