"""eqf_observe_landmarks_iterated on the device (csrc/eqf_iterate.hpp; FilterBatch.observe_landmarks(max_lin=...)).  The library's own
calls are the yardsticks, bit for bit: max_lin = 1 against eqf_observe_landmarks on a fork; the commit against
eqf_update_landmarks(local = 0) on a fork fed the returned rows; the linearisation point against eqf_apply_increment with the last plane
of g_trace followed by eqf_observe_landmarks there.  Each step g_trace[k] -> g_trace[k + 1] is held to the 50-digit one-step reference
of tests/iterate_exact.py inside K_ITER's bound, taken on its own so that errors do not compound.  The handles and helpers are
test_gpu_observe.py's.  Nothing here provokes a fault: the indefinite Sigma and the trial point that is not finite are ordinary numeric
verdicts."""
import numpy as np
import pytest

import iterate_exact as ix
import lift_cases as lc
import observe_cases as oc
from eqf_vio_amd import consistency as cs
from test_gpu_observe import REPORT, _all, _bits, _fork, _ops, _restored, h0, hip  # noqa: F401  (h0, hip: fixtures)

pytestmark = pytest.mark.gpu
KINDS = (cs.OBS_BEARING, cs.OBS_RANGE, cs.OBS_POSITION)
ITER = ("n_lin", "status", "last_step")
INF = float("inf")


def _far_ops(fg, kind, lms, cam=None, seed=0, absent=False):
    """_ops with every measurement well off the prediction, so that one linearisation is a poor one: a range and a position 40 % out"""
    ops = _ops(fg, kind, lms, cam=cam, seed=seed, absent=absent)
    if kind != cs.OBS_BEARING:
        ops["meas"] = 1.4 * ops["meas"]
        ops["R"] = 0.01 * ops["R"]
    return ops


def _iterated(fg, ops, max_lin, tol=0.0, **kw):
    cams = [o["cam"] for o in ops]
    cam = cams[0] if all(c is cams[0] for c in cams) else cams
    return fg.observe_landmarks(ops[0]["kind"], [o["ids"] for o in ops], [o["meas"] for o in ops], [o["R"] for o in ops], cam=cam, want_rows=True,
                                max_lin=max_lin, tol=tol, want_trace=True, **kw)


def _commit_replay(fg, ops, out, **kw):
    """eqf_update_landmarks(local = 0) on fg with the committed rows, the entries whose used is 1 only, nothing gated, at the same stride"""
    rows = cs.OBS_ROWS[ops[0]["kind"]]
    ids, H, r, R = [], [], [], []
    for b, o in enumerate(ops):
        keep = [k for k in range(len(o["ids"])) if out["used"][b, k] == 1]
        ids.append(o["ids"][keep])
        H.append(out["Ht"][b, keep].reshape(len(keep), rows, 3))
        r.append(out["resid"][b, keep].reshape(len(keep), rows))
        R.append(o["R"][keep].reshape(len(keep), rows, rows))
    return fg.update_landmarks(ids, H, r, R, rows=rows, local=False, stride=out["used"].shape[1], lm_gate=INF, **kw)


def _last_plane(out, b=0):
    tr = out["g_trace"][:, b]
    nz = [k for k in range(len(tr)) if tr[k].any()]
    return tr[nz[-1]] if nz else tr[0]


def _check_commit_and_point(hip, src, ops, max_lin, tol=0.0, lift=0, consider=None, cap=None, **kw):
    """the iterated call on one fork; the commit replayed on a second; the linearisation point rebuilt on a third"""
    A, F, P = (_fork(hip, [src], lift, cap) for _ in range(3))
    ckw = dict(kw, consider=None if consider is None else [consider])
    out = _iterated(A, [ops], max_lin, tol, **ckw)
    assert A.debug_iterate_launches() == _extra_launches(out["used"].shape[1], cs.OBS_ROWS[ops["kind"]], max_lin)
    rep = _commit_replay(F, [ops], out, **{k: v for k, v in ckw.items() if k != "lm_gate"})
    assert _all(A) == _all(F), "the commit is not eqf_update_landmarks(local = 0) with the committed rows"
    for k in REPORT + ("gamma",):
        assert _bits(out[k]) == _bits(rep[k]), k
    # the linearisation point: the last plane of g_trace as an increment on the prior, the one-shot rows there
    K, rows = len(ops["ids"]), cs.OBS_ROWS[ops["kind"]]
    sid = [int(i) for i in src.ids(0)]
    g = _last_plane(out)
    gam = np.zeros(11 + 3 * len(sid))
    for k in range(K):
        if out["used"][0, k] == 1:
            i = sid.index(int(ops["ids"][k]))
            gam[11 + 3 * i:14 + 3 * i] = g[k]
    P.set_option("innovation_lift", 0)
    P.apply_increment(gam[None, :])
    at = P.observe_landmarks(ops["kind"], ops["ids"], ops["meas"], ops["R"], cam=ops["cam"], want_rows=True, stride=out["used"].shape[1])
    on = [k for k in range(K) if out["used"][0, k] == 1]
    assert _bits(at["Ht"][0, on]) == _bits(out["Ht"][0, on]), "Ht_out is not the one-shot call's at the traced point"
    for k in on:
        terms = np.abs(at["resid"][0, k]) + np.abs(at["Ht"][0, k]) @ np.abs(g[k])
        want = at["resid"][0, k] + at["Ht"][0, k] @ g[k]
        assert np.all(np.abs(out["resid"][0, k] - want) <= 2 * np.finfo(float).eps * terms), k
    _check_steps(src, ops, out, consider)
    assert A.device_error() == 0 and F.device_error() == 0 and P.device_error() == 0
    A.close(), F.close(), P.close()
    return out


def _check_steps(src, ops, out, consider):
    """every traced step on its own against the 50-digit one-step reference"""
    st = src.dump_state(0)
    K = len(ops["ids"])
    on = [k for k in range(K) if out["used"][0, k] == 1]
    taken = int(out["n_lin"][0])
    worst = 0.0
    for k in range(taken - 1):
        gk, gn = out["g_trace"][k, 0, :K], out["g_trace"][k + 1, 0, :K]
        assert gn.any(), f"plane {k + 1} of g_trace is empty below n_lin = {taken}"
        ref = ix.one_step(ops["kind"], st["sigma"], st, ops["ids"], ops["meas"], ops["R"], gk, on, ops["cam"], consider)
        worst = max(worst, ix.step_ratio(gn, ref))
    print(f"kind {ops['kind']} K={K}: device step / K_ITER bound: {worst:.3f}")
    assert worst <= 1.0


def _extra_launches(stride, rows, max_lin):
    nb = (rows * stride + 63) // 64
    return 0 if max_lin <= 1 else (max_lin - 1) * (3 + 3 * nb - 1) + 1


# ---- 1. one linearisation is the one-shot call
@pytest.mark.parametrize("kind", KINDS)
def test_one_linearisation_is_observe_landmarks_bit_for_bit(hip, h0, kind):
    src = h0[22]
    ops = _ops(src, kind, list(range(0, 22, 2)), cam=oc.camera("offset"), seed=2, far=(3,), absent=True)
    A, F = _fork(hip, [src]), _fork(hip, [src])
    out = _iterated(A, [ops], 1, lm_gate=60.0)
    one = F.observe_landmarks(kind, ops["ids"], ops["meas"], ops["R"], cam=ops["cam"], want_rows=True, lm_gate=60.0)
    assert _all(A) == _all(F)
    for k in REPORT + ("gamma", "used", "Ht", "resid"):
        assert _bits(out[k]) == _bits(one[k]), k
    assert list(out["n_lin"]) == [1] and list(out["status"]) == [1] and out["last_step"][0] == 0.0 and not out["g_trace"].any()
    assert out["g_trace"].shape == (1, 1, len(ops["ids"]), 3) and A.debug_iterate_launches() == 0
    A.close(), F.close()


# ---- 2. the commit, the linearisation point and each step, at the shapes where a piece can go wrong
@pytest.mark.parametrize("N", (5, 22))
@pytest.mark.parametrize("kind", KINDS)
def test_commit_point_and_steps(hip, h0, kind, N):
    src = h0[N]
    ops = _far_ops(src, kind, list(range(N)), cam=oc.camera("offset"), seed=11, absent=(N == 22))
    out = _check_commit_and_point(hip, src, ops, 4)
    assert out["status"][0] == 1 and out["n_lin"][0] == 4 and out["info"][0] == 0 and out["g_trace"][1].any()
    assert not out["g_trace"][0].any()


def test_two_block_columns_of_s_and_a_second_pair_tile(hip, h0):
    out = _check_commit_and_point(hip, h0[43], _far_ops(h0[43], cs.OBS_BEARING, list(range(33)), seed=3), 3)   # order of S 66
    assert out["dof"][0] == 66
    out = _check_commit_and_point(hip, h0[22], _far_ops(h0[22], cs.OBS_POSITION, list(range(22)), seed=3), 3)  # order of S 66, 2 x 2 pair tiles
    assert out["dof"][0] == 66


def test_the_256_thread_loops(hip, h0):
    """260 range entries on a capacity-264 handle: past the rows kernels' 256-thread loop, and with the order of S at 260 and 780 rows of
    T the step kernel's strided loops go round again -- the back substitution's from column 257 on, the product's from entry 85 on.  The
    landmarks share a common-mode error, so that L is dense and what those tails compute reaches every g; each step is held to the
    one-step reference like everywhere else."""
    N = 260
    st = h0[5].dump_state(0)
    lm = oc.landmarks(N)
    S = np.zeros((11 + 3 * N, 11 + 3 * N))
    S[:11, :11] = st["sigma"][:11, :11]
    v = np.zeros(3 * N)
    for i in range(N):
        S[11 + 3 * i:14 + 3 * i, 11 + 3 * i:14 + 3 * i] = (0.3 * np.linalg.norm(lm["p"][i])) ** 2 * np.eye(3)
        v[3 * i:3 * i + 3] = 0.2 * lm["p"][i]
    S[11:, 11:] += np.outer(v, v)
    st.update(ids=np.arange(N, dtype=np.int32) + 10, sigma=S)
    st["origin"]["p"], st["group"]["Qq"], st["group"]["Qa"] = lm["p"], lm["Qq"], lm["Qa"]
    src = _restored(hip, st, cap=264)
    out = _check_commit_and_point(hip, src, _far_ops(src, cs.OBS_RANGE, list(range(N)), cam=oc.camera("offset"), seed=4), 2, cap=264)
    assert out["dof"][0] == N and out["info"][0] == 0 and out["n_lin"][0] == 2 and out["g_trace"][1].any()
    src.close()


@pytest.mark.parametrize("kind", (cs.OBS_BEARING, cs.OBS_RANGE))
def test_considered_entries_keep_g_zero_and_their_covariance(hip, h0, kind):
    src = h0[22]
    consider = [int(i) for i in sorted(src.ids(0))[1::2]] + [oc.ABSENT_ID + 1]
    lms = [1, 3, 6, 7, 20]
    ops = _far_ops(src, kind, lms, cam=oc.camera("offset"), seed=7)
    S0 = src.sigma(0)
    A = _fork(hip, [src])
    out = _iterated(A, [ops], 4, consider=[consider])
    for k, lid in enumerate(ops["ids"]):
        if int(lid) in consider:
            assert not out["g_trace"][:, 0, k].any() and not np.signbit(out["g_trace"][:, 0, k]).any()
        else:
            assert out["g_trace"][1, 0, k].any()
    c = [11 + 3 * i + k for i, lid in enumerate(src.ids(0)) if int(lid) in consider for k in range(3)]
    assert _bits(A.sigma(0)[np.ix_(c, c)]) == _bits(S0[np.ix_(c, c)]) and not out["gamma"][0, c].any()
    A.close()
    _check_commit_and_point(hip, src, ops, 4, consider=consider)


def test_with_the_innovation_lift_on(hip, h0):
    src = h0[22]
    _check_commit_and_point(hip, src, _far_ops(src, cs.OBS_RANGE, [1, 3, 7, 20], cam=oc.camera("offset"), seed=8), 3, lift=1)


# ---- 3. batches: ragged, masked, one camera per filter, filters that stop at different n_lin
def test_ragged_batch_each_filter_alone(hip, h0):
    kind = cs.OBS_RANGE
    s5, s22 = h0[5], h0[22]
    o5 = _far_ops(s5, kind, [0, 1, 2, 4], seed=5)
    o22 = _far_ops(s22, kind, list(range(0, 22, 3)), seed=5, absent=True)
    o22b = _ops(s22, kind, [2, 9], seed=6)   # a fraction of a sigma off: settles early
    q, t = oc.camera("offset")
    cams = [(q, t), (np.array([1.0, 0, 0, 0]), np.zeros(3)), (3.0 * q * [1, -1, 1, 1], -2.0 * t)]
    ops = [dict(o, cam=c) for o, c in zip((o5, o22, o22b), cams)]
    srcs = [s5, s22, s22]
    # a tolerance between the filters' fourth steps (from a run that never stops early): they stop at different linearisations
    fp = _fork(hip, srcs)
    tr = _iterated(fp, ops, 8)["g_trace"]
    fp.close()
    s3 = [float(np.max(np.abs(tr[4, b] - tr[3, b]))) for b in range(3)]
    tol = float(np.sqrt(min(s3) * max(s3)))
    fg = _fork(hip, srcs)
    out = _iterated(fg, ops, 8, tol)
    print(f"fourth steps {s3}, tol {tol:.3g}: n_lin {list(out['n_lin'])}, status {list(out['status'])}, last_step {list(out['last_step'])}")
    assert list(out["info"]) == [0, 0, 0] and len(set(int(n) for n in out["n_lin"])) > 1, out["n_lin"]
    assert all(s in (0, 1) for s in out["status"]) and 0 in out["status"]
    stride = out["used"].shape[1]
    for b in range(3):
        fa = _fork(hip, [srcs[b]], cap=24)
        oa = _iterated(fa, [ops[b]], 8, tol, stride=stride)
        assert _all(fa) == _all(fg, b), f"filter {b} alone"
        n = 11 + 3 * srcs[b].num_landmarks(0)
        assert _bits(oa["gamma"][0, :n]) == _bits(out["gamma"][b, :n])
        for k in REPORT + ITER + ("Ht", "resid", "used"):
            assert _bits(oa[k][0]) == _bits(out[k][b]), k
        assert _bits(oa["g_trace"][:, 0]) == _bits(out["g_trace"][:, b])
        fa.close()
    # planes behind a filter's last linearisation are zeros
    for b in range(3):
        assert not out["g_trace"][int(out["n_lin"][b]):, b].any()
    # one filter masked: it keeps every bit and reports status 4; the others are what they were
    fm = _fork(hip, srcs)
    before = _all(fm, 0)
    om = _iterated(fm, ops, 8, tol, mask=[0, 1, 1])
    assert list(om["info"]) == [3, 0, 0] and _all(fm, 0) == before and _all(fm, 1) == _all(fg, 1) and _all(fm, 2) == _all(fg, 2)
    assert om["status"][0] == 4 and om["n_lin"][0] == 0 and not om["g_trace"][:, 0].any() and not om["Ht"][0].any()
    fg.close(), fm.close()


# ---- 4. trouble on the way
def test_a_trial_point_that_is_not_finite_stalls_and_commits_the_previous_rows(hip, h0):
    """a range 1000 times the predicted one under a depth prior wide enough to follow it: exp(-p0 . g / |p0|^2) underflows"""
    st, ids, meas, R = ix.stall_case(h0[5].dump_state(0))
    host = cs.observe_iterated_host(cs.OBS_RANGE, st["sigma"], st, ids, meas, R, max_lin=4)
    assert host["status"] == cs.ITER_STALLED and host["n_lin"] == 1
    src = _restored(hip, st)
    ops = dict(kind=cs.OBS_RANGE, ids=ids, meas=meas, R=R, cam=None)
    A, F = _fork(hip, [src]), _fork(hip, [src])
    out = _iterated(A, [ops], 4)
    one = F.observe_landmarks(cs.OBS_RANGE, ids, meas, R, want_rows=True)
    assert out["status"][0] == 2 and out["n_lin"][0] == 1 and out["last_step"][0] > 0 and not out["g_trace"].any()
    assert _all(A) == _all(F), "the previous rows -- linearisation 0's -- are the ones committed"
    for k in REPORT + ("gamma", "used", "Ht", "resid"):
        assert _bits(out[k]) == _bits(one[k]), k
    A.close(), F.close(), src.close()


def test_an_indefinite_sigma_fails_the_solve_and_the_filter_keeps_every_bit(hip, h0):
    src = h0[22]
    bad = src.dump_state(0)
    S = bad["sigma"].copy()
    i = 3
    S[11 + 3 * i:14 + 3 * i, 11 + 3 * i:14 + 3 * i] = -1e3 * np.eye(3) * np.abs(S[11 + 3 * i, 11 + 3 * i])
    bad["sigma"] = S
    fb = _restored(hip, bad)
    ops = _ops(h0[22], cs.OBS_POSITION, [1, 3, 7], seed=9)
    ops["R"] = 1e-9 * ops["R"]
    A = _fork(hip, [fb])
    before = _all(A)
    out = _iterated(A, [ops], 4)
    assert out["status"][0] == 3 and out["n_lin"][0] == 1 and np.isnan(out["last_step"][0]) and out["info"][0] == 1
    assert _all(A) == before and not out["gamma"].any() and A.device_error() == 0
    A.close(), fb.close()


# ---- 5. the call's own contract
def test_without_outputs_it_enqueues_and_a_twin_with_outputs_has_the_same_bits(hip, h0):
    src = h0[22]
    ops = _far_ops(src, cs.OBS_BEARING, [0, 4, 5, 13], seed=12)
    A, F = _fork(hip, [src]), _fork(hip, [src])
    assert A.observe_landmarks(ops["kind"], ops["ids"], ops["meas"], ops["R"], max_lin=3, wait=False) is None
    out = _iterated(F, [ops], 3)
    A.synchronize()
    assert _all(A) == _all(F) and out["info"][0] == 0
    A.close(), F.close()


def test_argument_errors_arrive_before_any_effect(hip, h0):
    src = h0[5]
    ops = _far_ops(src, cs.OBS_RANGE, [0, 1], seed=13)
    A = _fork(hip, [src])
    before = _all(A)
    for kw in (dict(max_lin=17), dict(max_lin=2, tol=-1.0), dict(max_lin=2, tol=float("nan")), dict(max_lin=2, tol=INF),
               dict(max_lin=0, want_trace=True), dict(max_lin=2, gate=0.0)):
        with pytest.raises(Exception):
            A.observe_landmarks(ops["kind"], ops["ids"], ops["meas"], ops["R"], **kw)
    with pytest.raises(Exception):
        A.observe_landmarks(ops["kind"], ops["ids"][::-1].copy(), ops["meas"], ops["R"], max_lin=2)
    assert _all(A) == before and A.device_error() == 0
    A.close()


def test_the_iteration_lowers_the_map_cost(hip, h0):
    """what the feature is for: at a poor first linearisation the committed increment has a lower MAP cost than the one-shot call's"""
    src = h0[22]
    ops = _far_ops(src, cs.OBS_RANGE, [1, 3, 7, 20], seed=14)
    st = src.dump_state(0)
    A, F = _fork(hip, [src]), _fork(hip, [src])
    it = _iterated(A, [ops], 8, 1e-9)
    one = F.observe_landmarks(ops["kind"], ops["ids"], ops["meas"], ops["R"], want_rows=True)
    n = 11 + 3 * 22
    c_it = cs.map_cost(ops["kind"], st["sigma"], st, ops["ids"], ops["meas"], ops["R"], it["gamma"][0, :n], it["used"][0])
    c_one = cs.map_cost(ops["kind"], st["sigma"], st, ops["ids"], ops["meas"], ops["R"], one["gamma"][0, :n], one["used"][0])
    print(f"MAP cost: iterated {c_it:.6g} (n_lin {it['n_lin'][0]}), one-shot {c_one:.6g}")
    assert c_it <= c_one
    A.close(), F.close()
