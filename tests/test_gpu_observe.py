"""eqf_observe_landmarks on the device (csrc/eqf_observe.hpp; FilterBatch.observe_landmarks): the rows the kernel forms against the
50-digit reference of tests/observe_exact.py, taken from the handle's own dumped origin and group, inside K_OBS's bound; and everything
behind the rows against the library's own eqf_update_landmarks(local = 0) on a fork made by eqf_copy_filters, fed the returned rows, bit
for bit -- Sigma, state, bias, group, used, report and gamma.  The handles are those of test_gpu_schmidt.py: one filter after five vision
frames of a small synthetic stream.  Nothing here provokes a fault: the indefinite S and the indefinite Sigma_e are ordinary numeric
verdicts."""
import ctypes as C

import numpy as np
import pytest

import lift_cases as lc
import observe_cases as oc
import observe_exact as ox
from eqf_vio_amd import consistency as cs

pytestmark = pytest.mark.gpu
SIZES = (5, 22, 43)
KINDS = (cs.OBS_BEARING, cs.OBS_RANGE, cs.OBS_POSITION)
REPORT = ("nis", "logdet_S", "loglik", "dof", "info")


@pytest.fixture(scope="module")
def hip():
    from eqf_vio_amd import binding

    return binding


@pytest.fixture(scope="module")
def h0(hip):
    """{N: a one-filter handle after five vision frames of a synthetic stream, its Sigma mirrored from the lower triangle}"""
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
        S = fg.sigma(0)
        fg.set_sigma(np.tril(S) + np.tril(S, -1).T, 0)
        out[N] = fg
    yield out
    for fg in out.values():
        fg.close()


def _bits(x):
    if isinstance(x, dict):
        return {k: _bits(v) for k, v in x.items()}
    return np.ascontiguousarray(x).tobytes() + str(np.asarray(x).shape).encode()


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


def _restored(hip, st, cap=None):
    fg = hip.FilterBatch(lc.settings(1), capacity=cap or len(st["ids"]) + 2, batch=1)
    fg.restore_state(st, 0)
    return fg


def _ops(fg, kind, lms, cam=None, seed=0, far=(), absent=False, b=0):
    """entries on the landmarks lms (indices) of filter b, ids ascending: the measurement a fraction of its own sigma off the prediction
    (an entry of `far` a thousand times that), R the mean predicted variance times the identity"""
    st = fg.dump_state(b)
    S = st["sigma"]
    rows = cs.OBS_ROWS[kind]
    rng = np.random.default_rng([4107, seed, kind, len(lms)])
    lms = sorted(lms, key=lambda i: int(st["ids"][i]))
    ids = np.array([int(st["ids"][i]) for i in lms], dtype=np.int32)
    K = len(lms)
    Ht, _, _ = cs.observe_rows_host(kind, st, ids, np.tile([0.0, 0.0, 1.0], (K, 1)) if kind != cs.OBS_RANGE else np.ones((K, 3)), cam)
    J = cs.landmark_jacobian_blocks(st["group"])
    q_c, t_c = (np.array([1.0, 0, 0, 0]), np.zeros(3)) if cam is None else (np.asarray(cam[0]) / np.linalg.norm(cam[0]), np.asarray(cam[1]))
    Rc = cs.quat_to_matrix(q_c)
    meas, R = np.zeros((K, 3)), np.zeros((K, rows, rows))
    for k, i in enumerate(lms):
        P = Ht[k] @ S[11 + 3 * i:14 + 3 * i, 11 + 3 * i:14 + 3 * i] @ Ht[k].T
        R[k] = float(np.mean(np.diag(P))) * np.eye(rows)
        r = 0.3 * np.sqrt(np.diag(P + R[k])) * rng.standard_normal(rows) * (1000.0 if k in far else 1.0)
        pc = Rc.T @ (J[i] @ st["origin"]["p"][i] - t_c)
        d = np.linalg.norm(pc)
        if kind == cs.OBS_BEARING:
            meas[k] = cs.stereo_sphere_chart_inv(np.clip(r, -0.9, 0.9), pc / d)
        elif kind == cs.OBS_RANGE:
            meas[k, 0] = d + r[0]
        else:
            meas[k] = pc + r
    if absent:
        ids, meas, R = np.append(ids, oc.ABSENT_ID).astype(np.int32), np.vstack([meas, meas[:1]]), np.concatenate([R, R[:1]])
    return dict(kind=kind, ids=ids, meas=meas, R=R, cam=cam)


def _observe(fg, ops, **kw):
    """ops: one per filter"""
    cams = [o["cam"] for o in ops]
    cam = cams[0] if all(c is cams[0] for c in cams) else cams
    return fg.observe_landmarks(ops[0]["kind"], [o["ids"] for o in ops], [o["meas"] for o in ops], [o["R"] for o in ops], cam=cam, want_rows=True, **kw)


def _replay(fg, ops, out, b_out=None, **kw):
    """eqf_update_landmarks(local = 0) on fg with the rows `out` returned, the not-observable entries left out, at the same stride"""
    rows = cs.OBS_ROWS[ops[0]["kind"]]
    ids, H, r, R = [], [], [], []
    for b, o in enumerate(ops):
        bo = b if b_out is None else b_out[b]
        K = len(o["ids"])
        keep = [k for k in range(K) if out["used"][bo, k] != 3]
        ids.append(o["ids"][keep])
        H.append(out["Ht"][bo, keep].reshape(len(keep), rows, 3))
        r.append(out["resid"][bo, keep].reshape(len(keep), rows))
        R.append(o["R"][keep].reshape(len(keep), rows, rows))
    return fg.update_landmarks(ids, H, r, R, rows=rows, local=False, stride=out["used"].shape[1], **kw)


def _same_as_replay(hip, src, ops, lift=0, consider=None, expect_info=0, cap=None, **kw):
    """the observing call on one fork of src, the replay on another: every bit equal; returns the call's output"""
    A, F = _fork(hip, [src], lift, cap), _fork(hip, [src], lift, cap)
    before = _all(A)
    out = _observe(A, [ops], consider=None if consider is None else [consider], **kw)
    rep = _replay(F, [ops], out, consider=None if consider is None else [consider], **kw)
    assert out["info"][0] == expect_info == rep["info"][0], (out["info"], rep["info"])
    assert _all(A) == _all(F), "not the bits of eqf_update_landmarks(local = 0) with the returned rows"
    for k in REPORT + ("gamma",):
        assert _bits(out[k]) == _bits(rep[k]), k
    K = len(ops["ids"])
    u = out["used"][0, :K]
    assert list(u[u != 3]) == list(rep["used"][0, :int(np.sum(u != 3))])
    S = A.sigma(0)
    assert S.tobytes() == np.ascontiguousarray(S.T).tobytes(), "Sigma+ is not bit-for-bit symmetric"
    if expect_info == 0 and out["dof"][0] > 0:
        assert _all(A) != before
    else:
        assert _all(A) == before and not out["gamma"].any()
    assert A.device_error() == 0 and F.device_error() == 0
    A.close(), F.close()
    return out


# ---- 1. the rows against the reference
@pytest.mark.parametrize("N", oc.SIZES)
@pytest.mark.parametrize("camname", ("identity", "offset"))
@pytest.mark.parametrize("kind", KINDS)
def test_rows_against_the_exact_reference(hip, h0, kind, camname, N):
    """the committed case's landmarks put into the handle's state; the reference reads them back from the handle's own dump"""
    st = h0[N].dump_state(0)
    lm = oc.landmarks(N)
    st["origin"]["p"], st["group"]["Qq"], st["group"]["Qa"] = lm["p"], lm["Qq"], lm["Qa"]
    fg = _restored(hip, st)
    dumped = fg.dump_state(0)
    cam = oc.camera(camname)
    ids, meas = oc.entries(kind, dict(ids=dumped["ids"], origin=dumped["origin"], group=dumped["group"]), cam)
    order = np.argsort(ids)
    ids, meas = ids[order], meas[order]
    ref = ox.reference(kind, dumped, ids, meas, cam)
    out = fg.observe_landmarks(kind, ids, meas, 1.0, cam=cam, want_rows=True)
    K = len(ids)
    used = np.where(out["used"][0, :K] == 2, 1, out["used"][0, :K])
    rh, rr = ox.ratios(out["Ht"][0, :K], out["resid"][0, :K], used, ref)
    print(f"kind {kind} {camname} N={N}: device / bound: Ht {rh:.3f}, resid {rr:.3f}")
    assert rh <= 1.0 and rr <= 1.0
    assert fg.device_error() == 0
    fg.close()


# ---- 2. everything behind the rows, bit for bit
@pytest.mark.parametrize("N", (22, 43))
@pytest.mark.parametrize("kind", KINDS)
def test_downstream_is_update_landmarks_with_the_returned_rows(hip, h0, kind, N):
    src = h0[N]
    ops = _ops(src, kind, list(range(0, N, 2)), cam=oc.camera("offset"), seed=2, far=(3,), absent=True)
    out = _same_as_replay(hip, src, ops, lm_gate=60.0)
    K = len(ops["ids"])
    assert out["used"][0, K - 1] == 0 and out["used"][0, 3] == 2 and out["dof"][0] == cs.OBS_ROWS[kind] * (K - 2)


# ---- 3. chunk edges
def test_two_block_columns_of_s_and_a_second_pair_tile(hip, h0):
    out = _same_as_replay(hip, h0[43], _ops(h0[43], cs.OBS_BEARING, list(range(33)), seed=3))   # order of S 66: two block columns of 64
    assert out["dof"][0] == 66
    out = _same_as_replay(hip, h0[22], _ops(h0[22], cs.OBS_POSITION, list(range(17)), seed=3))  # 17 entries: a second 16-entry pair tile
    assert out["dof"][0] == 51


def test_the_rows_kernels_256_thread_loop(hip, h0):
    """257 entries on a capacity-260 handle: one filter, ranges (the smallest S)"""
    N = 257
    st = h0[5].dump_state(0)
    lm = oc.landmarks(N)
    S = np.zeros((11 + 3 * N, 11 + 3 * N))
    S[:11, :11] = st["sigma"][:11, :11]
    for i in range(N):
        S[11 + 3 * i:14 + 3 * i, 11 + 3 * i:14 + 3 * i] = (0.05 * lm["Qa"][i] * np.linalg.norm(lm["p"][i]) / lm["Qa"][i]) ** 2 * np.eye(3)
    st.update(ids=np.arange(N, dtype=np.int32) + 10, sigma=S)
    st["origin"]["p"], st["group"]["Qq"], st["group"]["Qa"] = lm["p"], lm["Qq"], lm["Qa"]
    src = _restored(hip, st, cap=260)
    out = _same_as_replay(hip, src, _ops(src, cs.OBS_RANGE, list(range(N)), cam=oc.camera("offset"), seed=4), cap=260)
    assert out["dof"][0] == N and list(out["used"][0]) == [1] * N
    src.close()


# ---- 4. a ragged batch
def _axis_landmark(hip, src, i):
    """src with landmark i on the chart's axis: p_hat = -2 e3 exactly, so that the bearing e3 is its antipode (not observable)"""
    st = src.dump_state(0)
    st["origin"]["p"][i], st["group"]["Qq"][i], st["group"]["Qa"][i] = [0.0, 0.0, -2.0], [1.0, 0.0, 0.0, 0.0], 1.0
    return _restored(hip, st)


def test_ragged_batch_alone_and_from_run_to_run(hip, h0):
    kind = cs.OBS_BEARING
    s5, s22 = _axis_landmark(hip, h0[5], 1), h0[22]
    empty = hip.FilterBatch(lc.settings(1), capacity=4, batch=1)
    o5 = _ops(s5, kind, [0, 1, 2, 4], seed=5)
    k1 = list(o5["ids"]).index(int(s5.ids(0)[1]))
    o5["meas"][k1], o5["R"][k1] = [0.0, 0.0, 1.0], 1e-4 * np.eye(2)            # the antipode of landmark 1's direction
    o22 = _ops(s22, kind, list(range(0, 22, 3)), seed=5, far=(2,), absent=True)
    none = dict(kind=kind, ids=np.zeros(0, dtype=np.int32), meas=np.zeros((0, 3)), R=np.zeros((0, 2, 2)), cam=None)
    ops, srcs = [o5, o22, none], [s5, s22, empty]
    runs = []
    for _ in range(2):
        fg = _fork(hip, srcs)
        out = _observe(fg, ops, lm_gate=60.0)
        runs.append(([_all(fg, b) for b in range(3)], _bits({k: out[k] for k in REPORT + ("gamma", "used", "Ht", "resid")})))
        assert fg.device_error() == 0
        fg.close()
    assert runs[0] == runs[1], "second run"
    assert list(out["info"]) == [0, 0, 0] and list(out["dof"]) == [6, 2 * (len(o22["ids"]) - 2), 0]
    assert list(out["used"][0, :4]) == [3 if k == k1 else 1 for k in range(4)] and not out["Ht"][0, k1].any() and not out["resid"][0, k1].any()
    assert out["used"][1, 2] == 2 and out["used"][1, len(o22["ids"]) - 1] == 0 and not out["used"][2].any()
    assert out["nis"][2] == 0 and out["loglik"][2] == 0 and not out["gamma"][2].any()
    for b in range(2):
        fa = _fork(hip, [srcs[b]], cap=24)
        oa = _observe(fa, [ops[b]], lm_gate=60.0, stride=out["used"].shape[1])
        assert _all(fa) == runs[0][0][b], f"filter {b} alone"
        n = 11 + 3 * srcs[b].num_landmarks(0)
        assert _bits(oa["gamma"][0, :n]) == _bits(out["gamma"][b, :n]) and _bits(oa["Ht"][0]) == _bits(out["Ht"][b])
        for k in REPORT:
            assert _bits(oa[k][0]) == _bits(out[k][b]), k
        # ... and without the entry that is not observable: the same bits
        if b == 0:
            fw = _fork(hip, [srcs[b]], cap=24)
            keep = [k for k in range(4) if k != k1]
            _observe(fw, [dict(o5, ids=o5["ids"][keep], meas=o5["meas"][keep], R=o5["R"][keep])], lm_gate=60.0, stride=out["used"].shape[1])
            assert _all(fw) == runs[0][0][0]
            fw.close()
        fa.close()
    # one filter masked: it keeps every bit, the others are what they were
    fg = _fork(hip, srcs)
    before = _all(fg, 0)
    om = _observe(fg, ops, lm_gate=60.0, mask=[0, 1, 1])
    assert list(om["info"]) == [3, 0, 0] and _all(fg, 0) == before and _all(fg, 1) == runs[0][0][1]
    assert not om["used"][0].any() and not om["Ht"][0].any() and not om["gamma"][0].any()
    fg.close(), s5.close(), empty.close()


# ---- 5. one camera per filter
def test_a_camera_per_filter_is_the_single_offset_call_of_each(hip, h0):
    src = h0[22]
    q, t = oc.camera("offset")
    cams = [(q, t), (np.array([1.0, 0, 0, 0]), np.zeros(3)), (3.0 * q * [1, -1, 1, 1], -2.0 * t)]
    ops = [_ops(src, cs.OBS_BEARING, [1, 4, 9, 20], cam=c, seed=6) for c in cams]
    fg = _fork(hip, [src] * 3)
    out = _observe(fg, ops)
    assert list(out["info"]) == [0, 0, 0]
    for b in range(3):
        fa = _fork(hip, [src])
        oa = _observe(fa, [ops[b]])
        assert _all(fa) == _all(fg, b), b
        for k in REPORT + ("gamma", "Ht", "resid", "used"):
            assert _bits(oa[k][0]) == _bits(out[k][b]), k
        fa.close()
    # the identity offset has the bits of no offset at all
    fn = _fork(hip, [src])
    _observe(fn, [dict(ops[1], cam=None)])
    assert _all(fn) == _all(fg, 1)
    fn.close(), fg.close()


# ---- 6. consider lists
@pytest.mark.parametrize("kind", (cs.OBS_BEARING, cs.OBS_RANGE))
def test_with_consider_lists_it_is_the_schmidt_call(hip, h0, kind):
    src = h0[22]
    consider = [int(i) for i in sorted(src.ids(0))[1::2]] + [oc.ABSENT_ID + 1]
    out = _same_as_replay(hip, src, _ops(src, kind, [1, 3, 7, 20], cam=oc.camera("offset"), seed=7), consider=consider)
    c = [11 + 3 * i + k for i, lid in enumerate(src.ids(0)) if int(lid) in consider for k in range(3)]
    assert not out["gamma"][0, c].any() and out["gamma"][0, :11].all()


# ---- 7. filters that must keep every bit
def test_masked_gated_indefinite_and_refused_filters_keep_every_bit(hip, h0):
    src = h0[22]
    kind = cs.OBS_POSITION
    ops = _ops(src, kind, [1, 3, 7, 20], cam=oc.camera("offset"), seed=8)
    neg = dict(ops, R=-1e6 * np.abs(ops["R"]) - np.eye(3))   # S = Ht Sigma Ht^T + R is negative definite
    F = _fork(hip, [src])
    nis = float(_observe(F, [ops])["nis"][0])
    F.close()
    fg = _fork(hip, [src] * 4)
    before = [_all(fg, b) for b in range(4)]
    out = _observe(fg, [ops, ops, neg, ops], gate=0.5 * nis, mask=[0, 1, 1, 0])
    assert list(out["info"]) == [3, 2, 1, 3], out["info"]
    for b in range(4):
        assert _all(fg, b) == before[b], f"filter {b}"
        assert not out["gamma"][b].any()
    assert _bits(out["nis"][1]) == _bits(np.float64(nis)) and fg.device_error() == 0
    fg.close()
    # Sigma_e indefinite in the last landmark; S of the call stays definite: the lift refuses, info 4
    bad = src.dump_state(0)
    S = bad["sigma"].copy()
    S[-1, -1] = -abs(S[-1, -1])
    bad["sigma"] = S
    fb = _restored(hip, bad)
    _same_as_replay(hip, fb, ops, lift=1, expect_info=4)
    fb.close()
    # ... and with the lift on a healthy filter the call is still the replay's
    _same_as_replay(hip, src, ops, lift=1)


# ---- 8. the gravity chart plays no part
def test_a_singular_gravity_chart_does_not_stop_the_call(hip, h0):
    """a filter that has not been initialised has its gravity direction at the pole of its own chart (test_gpu_schmidt.py: local = 1 gives
    info -1); with the landmarks and the covariance of a running filter it takes the observing call like any other"""
    f0 = hip.FilterBatch(lc.settings(1), capacity=7, batch=1)
    st, run = f0.dump_state(0), h0[5].dump_state(0)
    f0.close()
    st.update(ids=run["ids"], sigma=run["sigma"])
    st["origin"]["p"], st["group"]["Qq"], st["group"]["Qa"] = run["origin"]["p"], run["group"]["Qq"], run["group"]["Qa"]
    src = _restored(hip, st)
    ops = _ops(src, cs.OBS_BEARING, [0, 2, 3], cam=oc.camera("offset"), seed=9)
    probe = _fork(hip, [src])
    Ht0 = np.zeros((3, 2, 3))
    Ht0[:, 0, 0] = Ht0[:, 1, 1] = 1.0
    o = probe.update_landmarks([ops["ids"]], [Ht0], [np.zeros((3, 2))], [ops["R"]], rows=2, local=True)
    assert o["info"][0] == -1, "the gravity chart of this state is meant to be singular"
    probe.close()
    out = _same_as_replay(hip, src, ops)
    assert out["info"][0] == 0 and out["dof"][0] == 6
    src.close()


# ---- 9. the call that does not wait, and argument errors
def test_non_blocking_form_has_the_same_bits(hip, h0):
    src = h0[22]
    ops = _ops(src, cs.OBS_BEARING, [0, 5, 6, 11, 21], cam=oc.camera("offset"), seed=10)
    A, B = _fork(hip, [src]), _fork(hip, [src])
    _observe(A, [ops])
    assert B.observe_landmarks(ops["kind"], ops["ids"], ops["meas"], ops["R"], cam=ops["cam"], wait=False) is None
    B.synchronize()
    assert _all(A) == _all(B) and _all(A) != _all(src) and B.device_error() == 0
    A.close(), B.close()


def test_argument_errors_come_before_any_effect(hip, h0):
    src = h0[5]
    fg = _fork(hip, [src, src], cap=6)
    f32 = hip.FilterBatch(lc.settings(1), capacity=6, batch=2, precision=hip.PRECISION_F32)
    L = hip.lib()
    dp, ip, up = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_ubyte)
    P = lambda a, t=dp: a.ctypes.data_as(t) if a is not None else None  # noqa: E731
    o = _ops(src, cs.OBS_BEARING, [0, 1, 4], seed=11)
    nk = np.array([3, 3], dtype=np.int32)
    lid = np.ascontiguousarray(np.stack([o["ids"]] * 2))
    meas, Rb = (np.ascontiguousarray(np.stack([o[k]] * 2)) for k in ("meas", "R"))
    n = 11 + 3 * 5
    G, Ht, rs, used = np.full((2, n), -7.0), np.full((2, 3, 2, 3), -7.0), np.full((2, 3, 2), -7.0), np.full((2, 3), 7, dtype=np.uint8)
    rep = (hip.LinearReport * 2)()
    for s in rep:
        s.nis, s.dof, s.info = -7.0, -7, -7
    inf = float("inf")

    def call(h, kind=0, cam=None, per=0, nk_=nk, lid_=lid, meas_=meas, Rb_=Rb, gate=inf, lm=inf, nc=None, cid=None, cstride=0, ldg=n):
        return L.eqf_observe_landmarks(h, kind, P(cam), per, P(nk_, ip), P(lid_, ip), 3, P(meas_), P(Rb_), gate, lm, None, P(nc, ip), P(cid, ip),
                                       cstride, P(used, up), P(Ht), P(rs), P(G), ldg, rep)

    nanm, infm = meas.copy(), meas.copy()
    nanm[1, 2, 1], infm[0, 0, 0] = np.nan, np.inf
    nanR = Rb.copy()
    nanR[0, 1, 1, 0] = np.nan
    unsorted = lid.copy()
    unsorted[1, 1], unsorted[1, 2] = lid[1, 2], lid[1, 1]
    cam0, camn = np.zeros(7), np.array([1.0, 0, 0, 0, 0, np.nan, 0])
    cam2 = np.array([[1.0, 0, 0, 0, 0, 0, 0], [0.0, 0, 0, 0, 0, 0, 0]])
    i32 = lambda *v: np.array(v, dtype=np.int32)  # noqa: E731
    bad = [(dict(kind=3), hip.ERR_INVALID), (dict(kind=-1), hip.ERR_INVALID), (dict(per=2), hip.ERR_INVALID), (dict(cam=cam0), hip.ERR_INVALID),
           (dict(cam=camn), hip.ERR_INVALID), (dict(cam=cam2, per=1), hip.ERR_INVALID), (dict(meas_=nanm), hip.ERR_INVALID),
           (dict(meas_=infm), hip.ERR_INVALID), (dict(Rb_=nanR), hip.ERR_INVALID), (dict(nk_=i32(3, 4)), hip.ERR_INVALID),
           (dict(gate=0.0), hip.ERR_INVALID), (dict(lm=float("nan")), hip.ERR_INVALID), (dict(ldg=n - 1), hip.ERR_INVALID),
           (dict(meas_=None), hip.ERR_INVALID), (dict(lid_=unsorted), hip.ERR_UNSORTED),
           (dict(nc=i32(2, 2), cid=i32(int(lid[0, 1]), int(lid[0, 0]), 0, 0), cstride=2), hip.ERR_UNSORTED),
           (dict(nc=i32(7, 0), cid=np.arange(14, dtype=np.int32), cstride=7), hip.ERR_CAPACITY)]
    before = [_all(fg, b) for b in range(2)]
    before32 = [_bits(f32.dump_state(b)) for b in range(2)]
    for kw, code in bad:
        assert call(fg._h, **kw) == code, (kw.keys(), code)
    assert call(None) == hip.ERR_INVALID and call(f32._h) == hip.ERR_UNSUPPORTED
    assert np.all(G == -7.0) and np.all(Ht == -7.0) and np.all(rs == -7.0) and np.all(used == 7)
    assert all(s.nis == -7.0 and s.dof == -7 and s.info == -7 for s in rep)
    for b in range(2):
        assert _all(fg, b) == before[b] and _bits(f32.dump_state(b)) == before32[b], b
    assert fg.device_error() == 0 and f32.device_error() == 0
    # good arguments work, also with a NaN where nothing is read (a range's meas[1], meas[2])
    assert call(fg._h) == 0 and [s.info for s in rep] == [0, 0] and list(used[0]) == [1, 1, 1]
    rngm = np.ascontiguousarray(np.stack([_ops(src, cs.OBS_RANGE, [0, 1, 4], seed=11)["meas"]] * 2))
    rngm[:, :, 1:] = np.nan
    R1, Ht1, rs1 = np.ones((2, 3, 1, 1)) * 1e-2, np.zeros((2, 3, 1, 3)), np.zeros((2, 3, 1))
    assert L.eqf_observe_landmarks(fg._h, 1, None, 0, P(nk, ip), P(lid, ip), 3, P(rngm), P(R1), inf, inf, None, None, None, 0, P(used, up),
                                   P(Ht1), P(rs1), None, 0, rep) == 0
    assert [s.info for s in rep] == [0, 0] and np.all(np.isfinite(Ht1)) and Ht1.any() and fg.device_error() == 0
    fg.close(), f32.close()
