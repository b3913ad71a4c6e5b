"""The per-landmark block measurement update on the device (csrc/eqf_blocks.hpp: eqf_update_landmarks; FilterBatch.update_landmarks) entry by
entry against the reference and the a-priori bound of tests/blocks_exact.py, on the cases of tests/blocks_cases.py that
tests/test_blocks_exact.py holds the CPU statement to.  The shapes are the kernels' edges: the order of S at 1, 63, 64, 66 and 129 (64-wide
block columns), the state order at N = 4, 43, 86 (64-row tiles of Sigma past 64, 128 and 256), batch 1; and a batch of three with ragged N
and ragged entry counts, one of them 0.  Every reference starts from the device's own sigma(), origin() and group() before the call; every
R_k goes in with its upper triangle negated (only the lower triangles may be read).  Everything that is not arithmetic is bit for bit.
Nothing here provokes a fault: the indefinite S is an ordinary numeric verdict of the tail kernel.
Worst device / bound ratios on an MI355X: NOTES.md R20.1 (each test prints its own).

A deviation from the statement "a decoupled block is carried through the launches": the kernels pack the entries that take part to the front
and never form the decoupled blocks, so "the same bits as the call without that entry at the same stride" holds by construction; it is
tested below all the same."""
import ctypes as C

import numpy as np
import pytest

import blocks_cases as bc
import blocks_exact as bx
import consistency_cases as cc
import consistency_exact as cx
import linear_exact as le
from eqf_vio_amd import consistency as cs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from eqf_vio_amd import binding

    return binding


@pytest.fixture(scope="module")
def own_sigma(hip):
    """{N: a filter's own Sigma after five vision frames}"""
    from eqf_vio_amd import synth

    out = {}
    for N in sorted({c[0] for c in bc.CASES.values() if c[5] == "own"}):
        st = synth.make_stream(N, duration=0.4)
        fg = hip.FilterBatch(cc.settings(), capacity=N + bc.CAP_EXTRA, batch=1)
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
        out[N] = fg.sigma(0)
        fg.close()
    return out


@pytest.fixture(scope="module")
def master_J():
    """{N: 50-digit J of the committed state}"""
    out = {}
    for N in bc.SIZES:
        s = cc.local_state(N, bc.THETA)
        out[N] = cx.jacobian_mp(s["origin"], s["group"])
    return out


def _bits(x):
    if isinstance(x, dict):
        return {k: _bits(v) for k, v in x.items()}
    return np.ascontiguousarray(x).tobytes() + str(np.asarray(x).shape).encode()


def _assert_same(a, b, what):
    a, b = _bits(a), _bits(b)
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k], f"{what}: {k} differs"


def _getters(fg, b, last=True):
    """everything a caller can read of filter b (last = False: without the records of the last vision update, which a handle that has never
    run one does not have -- for comparisons ACROSS handles)"""
    g = dict(n=fg.num_landmarks(b), est=fg.state_estimate(b), innov=fg.innovation_stats(b), gate=fg.gate_report(b),
             og=np.array(fg.outlier_gate(), dtype=float))
    if last:
        g["last"] = fg.last_update(b)
    g.update(fg.dump_state(b))  # ids, origin, group, bias, sigma, time, integrator
    return g


def _call(fg, opsl, local, **kw):
    """FilterBatch.update_landmarks with one operand dict per filter (None: no entries)"""
    rows = next(o["rows"] for o in opsl if o is not None)
    e = [np.zeros(0, dtype=np.int32), np.zeros((0, rows, 3)), np.zeros((0, rows)), np.zeros((0, rows, rows))]
    lists = [[(o["ids"], o["H"], o["resid"], bc.poison(o["R"]))[j] if o is not None else e[j] for o in opsl] for j in range(4)]
    return fg.update_landmarks(*lists, rows=rows, local=bool(local), **kw)


def _got(out, b, Sp, n):
    K = out["used"].shape[1]
    return dict(Sigma=Sp, gamma=out["gamma"][b, :n], nis=out["nis"][b], logdet_S=out["logdet_S"][b], loglik=out["loglik"][b], dof=out["dof"][b],
                used=out["used"][b, :K])


def _ratios(out, b, Sp, n, ref, bnd, K):
    got = _got(out, b, Sp, n)
    got["used"] = got["used"][:K]
    assert not out["used"][b, K:].any()
    return bx.ratios(got, ref, bnd)


def _subset(ops, keep):
    o = dict(ops)
    for k in ("ids", "idx", "H", "resid", "R"):
        o[k] = ops[k][keep]
    o["gated"], o["absent"] = (), None
    return o


# ---- 1. entry by entry against the reference, the group step, and what stays
@pytest.mark.parametrize("name", list(bc.CASES))
def test_update_entry_by_entry_and_the_group_step(hip, master_J, own_sigma, name):
    N = bc.CASES[name][0]
    n = 11 + 3 * N
    snap = bc.snapshot(name, own_sigma.get(N))
    fg = hip.FilterBatch(cc.settings(), capacity=N + bc.CAP_EXTRA, batch=1)
    fg.restore_state(snap, 0)
    pre, pre_all = fg.dump_state(0), _getters(fg, 0)
    S0 = fg.sigma(0)
    ops = bc.operands(name, snap, S0)
    ref = bx.reference(S0, ops, master_J[N])
    bnd = bx.bounds(ref)
    assert bnd["validity"] <= bx.VALIDITY
    out = _call(fg, [ops], ops["local"], lm_gate=ops["lm_gate"])
    assert out["info"][0] == 0
    Sp = fg.sigma(0)
    assert Sp.tobytes() == np.ascontiguousarray(Sp.T).tobytes(), "Sigma+ is not bit-for-bit symmetric"
    rt = _ratios(out, 0, Sp, n, ref, bnd, len(ops["idx"]))
    print(f"{name}: device / bound  " + "  ".join(f"{k} {v:.3f}" for k, v in rt.items()))
    for k, v in rt.items():
        assert v <= 1.0, (name, k, v)
    # what stays: origin, clock, integrator, ids, the records of the last vision update, the innovation statistics, the gate report
    post = _getters(fg, 0)
    for k in ("ids", "origin", "time", "currentVelocity", "accumulatedVelocity", "accumulatedTime", "initialised", "last", "innov", "gate", "og", "n"):
        assert _bits(post[k]) == _bits(pre_all[k]), (name, k)
    # the state after the step: eqf_apply_increment's step with the gamma the call returned (which sits inside its bound), bit for bit
    fb = hip.FilterBatch(cc.settings(), capacity=N + bc.CAP_EXTRA, batch=1)
    fb.restore_state(pre, 0)
    fb.set_sigma(Sp, 0)
    fb.apply_increment(out["gamma"][:, :n])
    _assert_same(_getters(fg, 0, last=False), _getters(fb, 0, last=False), name)
    assert _bits(post["group"]) != _bits(pre["group"]) and fg.device_error() == 0
    # an entry that does not take part leaves the bits of the call without it at the same stride
    if ops["gated"] or ops["absent"] is not None:
        keep = [k for k in range(len(ops["idx"])) if ref["used"][k] == 1]
        fc = hip.FilterBatch(cc.settings(), capacity=N + bc.CAP_EXTRA, batch=1)
        fc.restore_state(pre, 0)
        o2 = _call(fc, [_subset(ops, keep)], ops["local"], stride=len(ops["idx"]))
        assert o2["info"][0] == 0 and o2["dof"][0] == out["dof"][0]
        _assert_same(_getters(fc, 0, last=False), _getters(fg, 0, last=False), f"{name}: without the entries that do not take part")
        _assert_same({k: o2[k] for k in ("gamma", "nis", "logdet_S", "loglik")}, {k: out[k] for k in ("gamma", "nis", "logdet_S", "loglik")}, name)
        fc.close()
    fg.close(), fb.close()


# ---- 2. a batch of three: ragged N, ragged entry counts (one of them 0); alone against position 2 of 3; run to run
def test_ragged_batch_alone_and_from_run_to_run(hip, master_J, own_sigma):
    names = ("small8", None, "stereo66")
    Ns = (4, 86, 43)
    snaps = [bc.snapshot("small8"), bc.snapshot("mixed129", own_sigma[86]), bc.snapshot("stereo66")]
    res = []
    for run in range(2):
        fg = hip.FilterBatch(cc.settings(), capacity=max(Ns) + bc.CAP_EXTRA, batch=3)
        for b in range(3):
            fg.restore_state(snaps[b], b)
        S0 = [fg.sigma(b) for b in range(3)]
        opsl = [dict(bc.operands(nm, snaps[b], S0[b]), local=1) if nm else None for b, nm in enumerate(names)]
        before = _getters(fg, 1)
        out = _call(fg, opsl, 1)
        assert list(out["info"]) == [0, 0, 0] and list(out["dof"]) == [8, 0, 66], (out["info"], out["dof"])
        _assert_same(_getters(fg, 1), before, "the filter without entries")
        assert out["nis"][1] == 0.0 and out["logdet_S"][1] == 0.0 and not out["gamma"][1].any() and not out["used"][1].any()
        if run == 0:
            for b in (0, 2):
                n = 11 + 3 * Ns[b]
                ref = bx.reference(S0[b], opsl[b], master_J[Ns[b]])
                Sp = fg.sigma(b)
                assert Sp.tobytes() == np.ascontiguousarray(Sp.T).tobytes()
                rt = _ratios(out, b, Sp, n, ref, bx.bounds(ref), len(opsl[b]["idx"]))
                print(f"ragged batch, filter {b} (N={Ns[b]}): device / bound", {k: round(v, 3) for k, v in rt.items()})
                assert max(rt.values()) <= 1.0, (b, rt)
                assert not out["gamma"][b, n:].any()
        res.append((fg.dump_state(2), {k: out[k][2] for k in ("nis", "logdet_S", "loglik", "dof")}, out["gamma"][2, :11 + 3 * 43].copy(), opsl[2]))
        assert fg.device_error() == 0
        fg.close()
    _assert_same(res[0][0], res[1][0], "state, second run")
    _assert_same(res[0][1], res[1][1], "report, second run")
    # the same filter alone in a handle of another capacity
    fa = hip.FilterBatch(cc.settings(), capacity=43 + 2, batch=1)
    fa.restore_state(snaps[2], 0)
    oa = _call(fa, [res[0][3]], 1)
    _assert_same(fa.dump_state(0), res[0][0], "alone against position 2 of 3")
    _assert_same({k: oa[k][0] for k in ("nis", "logdet_S", "loglik", "dof")}, res[0][1], "alone: report")
    assert oa["gamma"][0].tobytes() == res[0][2].tobytes()
    fa.close()


# ---- 3. against eqf_update_linear: the same measurement as dense rows (m = 8 <= 16); both inside the same reference bound
def test_against_update_linear_with_dense_rows(hip, master_J):
    name, N = "small8", 4
    n = 11 + 3 * N
    snap = bc.snapshot(name)
    fa = hip.FilterBatch(cc.settings(), capacity=N + bc.CAP_EXTRA, batch=1)
    fb = hip.FilterBatch(cc.settings(), capacity=N + bc.CAP_EXTRA, batch=1)
    for local in (0, 1):
        fa.restore_state(snap, 0), fb.restore_state(snap, 0)
        S0 = fa.sigma(0)
        assert np.array_equal(S0, S0.T) and fb.sigma(0).tobytes() == S0.tobytes()
        ops = dict(bc.operands(name, snap, S0), local=local)
        ref = bx.reference(S0, ops, master_J[N])
        bnd = bx.bounds(ref)
        oa = _call(fa, [ops], local)
        Hd = cs.landmark_blocks_matrix(N, ops["idx"], ops["H"])
        Rd = np.zeros((8, 8))
        for k in range(4):
            Rd[2 * k:2 * k + 2, 2 * k:2 * k + 2] = bc.poison(ops["R"][k])
        ob = fb.update_linear(Hd, ops["resid"].reshape(-1), Rd, local=bool(local), want_gamma=True)
        assert oa["info"][0] == 0 and ob["info"][0] == 0 and oa["dof"][0] == ob["dof"][0] == 8
        ra = _ratios(oa, 0, fa.sigma(0), n, ref, bnd, 4)
        rb = le.ratios(dict(Sigma=fb.sigma(0), gamma=ob["gamma"][0, :n], nis=ob["nis"][0], logdet_S=ob["logdet_S"][0], loglik=ob["loglik"][0]), ref, bnd)
        print(f"local={local}: update_landmarks / bound {max(ra.values()):.3f}, update_linear / bound {max(rb.values()):.3f}")
        assert max(ra.values()) <= 1.0 and max(rb.values()) <= 1.0, (ra, rb)
    fa.close(), fb.close()


# ---- 4. filters that do not take part keep every bit
def test_masked_gated_indefinite_and_singular_chart_keep_every_bit(hip, master_J, own_sigma):
    name, N = "position63", 43
    snap = bc.snapshot(name, own_sigma[N])
    fg = hip.FilterBatch(cc.settings(), capacity=N + bc.CAP_EXTRA, batch=4)
    for b in range(4):
        fg.restore_state(snap, b)
    S0 = fg.sigma(0)
    ops = bc.operands(name, snap, S0)
    ref = bx.reference(S0, ops, master_J[N])
    neg = dict(ops, R=-1e6 * np.abs(ops["R"]) - np.eye(3)[None])  # S = Ht Sigma Ht^T + R is negative definite
    before = [_getters(fg, b) for b in range(4)]
    # filter 0 masked out, 1 gated by the joint nis, 2 with an indefinite S, 3 applied
    rows = ops["rows"]
    lists = [[o[k] for o in (ops, ops, neg, ops)] for k in ("ids", "H", "resid")] + [[bc.poison(o["R"]) for o in (ops, ops, neg, ops)]]
    gate = 0.5 * float(ref["nis"])
    out1 = fg.update_landmarks(*lists, rows=rows, local=True, gate=gate, mask=[0, 1, 1, 0])
    assert list(out1["info"]) == [3, 2, 1, 3], out1["info"]
    out2 = fg.update_landmarks(*lists, rows=rows, local=True, mask=[0, 0, 0, 1])
    assert list(out2["info"]) == [3, 3, 3, 0]
    for b in range(3):
        _assert_same(_getters(fg, b), before[b], f"filter {b}")
        assert not out1["gamma"][b].any()
    assert np.isnan(out1["nis"][0]) and np.isnan(out1["nis"][2]) and not out1["used"][0].any()
    bnd = bx.bounds(ref)
    assert abs(out1["nis"][1] - float(ref["nis"])) <= bnd["nis"] and abs(out1["logdet_S"][1] - float(ref["logdet_S"])) <= bnd["logdet_S"]
    assert out1["dof"][1] == 63 and _bits(fg.dump_state(3)) != _bits({k: before[3][k] for k in fg.dump_state(3)})
    assert fg.device_error() == 0
    fg.close()
    # a filter that has not been initialised: the origin's gravity direction is the pole of its own chart (local = 1: info -1)
    f0 = hip.FilterBatch(cc.settings(), capacity=4, batch=1)
    pre = f0.dump_state(0)
    o = f0.update_landmarks([[3]], [np.ones((1, 1, 3))], [np.zeros((1, 1))], [np.eye(1)[None]], rows=1, local=True)
    assert o["info"][0] == -1 and not o["gamma"].any()
    _assert_same(f0.dump_state(0), pre, "uninitialised filter, local rows")
    assert f0.device_error() == 0
    f0.close()


# ---- 5. through the stack: a stereo rig on a synth stream
def test_stereo_rig_on_a_stream_and_the_facade(hip):
    from eqf_vio_amd import filter as vf
    from eqf_vio_amd import synth

    N, frames = 20, 10
    st = synth.make_stream(N, duration=0.05 * frames + 0.01)
    d = synth.template_settings_dict()
    Rn = (2e-3) ** 2 * np.eye(2)

    def run(middle, facade):
        fg = vf.VIOFilter(hip.settings_from_dict(d), capacity=N + 2) if facade else hip.FilterBatch(d, capacity=N + 2, batch=1)
        seen, rep, ld = 0, None, []
        for kind, k in st.events():
            if kind == "imu":
                r = st.imu[k]
                if facade:
                    fg.processIMUData(vf.IMUVelocity(r[0], r[1:4], r[4:7]))
                else:
                    fg.process_imu(r[0], r[1:4], r[4:7])
                continue
            if facade:
                fg.processVisionData(vf.VisionMeasurement(st.vision_stamps[k], st.ids, st.bearings[k]))
            else:
                fg.process_vision(st.vision_stamps[k], st.ids, st.bearings[k])
            seen += 1
            fb = fg._fb if facade else fg
            if seen == frames - 1 and middle:
                # the second camera sees every landmark where the first camera's bearing and the synthetic scene put it
                est = fb.state_estimate(0)
                ids = fb.dump_state(0)["ids"]
                H, r = [], []
                for i, lid in enumerate(ids):
                    j = list(st.ids).index(lid)
                    p_true = st.bearings[k][j] * float(np.linalg.norm(est["p"][i]))  # (the first camera's ray at the estimated range)
                    y2 = cs.quat_to_matrix(bc.Q_21).T @ (p_true - bc.T_21)
                    Hk, rk = cs.stereo_rows(est["p"][i], bc.Q_21, bc.T_21, y2 / np.linalg.norm(y2))
                    H.append(Hk), r.append(rk)
                if facade:
                    rep = fg.processLandmarkMeasurements(ids, np.array(H), np.array(r), Rn, local=True)
                else:
                    o = fg.update_landmarks([ids], [np.array(H)], [np.array(r)], [Rn], local=True)
                    rep = dict(nis=float(o["nis"][0]), logdet_S=float(o["logdet_S"][0]), loglik=float(o["loglik"][0]), dof=int(o["dof"][0]),
                               info=int(o["info"][0]), used=o["used"][0, :len(ids)], gamma=o["gamma"][0])
            if seen >= frames - 1:
                ld.append(fb.nees(None, local=True))
            if seen == frames:
                break
        assert fb.device_error() == 0 and fb.num_landmarks(0) == N and len(ld) == 2 and (rep is not None or not middle)
        return fb.dump_state(0), rep, ld

    s_with, rep, ld_with = run(True, False)
    s_without, _, ld_without = run(False, False)
    assert rep["info"] == 0 and rep["dof"] == 2 * N and np.all(rep["used"] == 1)
    for a, b in zip(ld_with, ld_without):   # after the stereo update and after the frame that follows it
        assert a["info"][0] == 0 and b["info"][0] == 0 and a["logdet"][0] < b["logdet"][0], (a["logdet"], b["logdet"])
    print(f"log det Sigma_loc, with / without the second camera: {ld_with[0]['logdet'][0]:.2f} / {ld_without[0]['logdet'][0]:.2f} after the update, "
          f"{ld_with[1]['logdet'][0]:.2f} / {ld_without[1]['logdet'][0]:.2f} after the next frame")
    s_fac, rep_fac, _ = run(True, True)
    _assert_same(s_fac, s_with, "VIOFilter.processLandmarkMeasurements against FilterBatch.update_landmarks")
    _assert_same({k: rep_fac[k] for k in rep}, rep, "the reports")


# ---- 6. argument errors come before any effect
def test_argument_errors_come_before_any_effect(hip):
    from eqf_vio_amd import synth

    N = 4
    snap = bc.snapshot("small8")
    fg = hip.FilterBatch(cc.settings(), capacity=N + 1, batch=2)
    for b in range(2):
        fg.restore_state(snap, b)
    f32 = hip.FilterBatch(cc.settings(), capacity=N, batch=2, precision=hip.PRECISION_F32)
    st = synth.make_stream(N, duration=0.4)
    for kind, k in list(st.events())[:30]:
        if kind == "imu":
            f32.process_imu(st.imu[k][0], st.imu[k][1:4], st.imu[k][4:7])
    L = hip.lib()
    dp, ip, up = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_ubyte)
    P = lambda a, t=dp: a.ctypes.data_as(t) if a is not None else None  # noqa: E731
    n, rows, stride = 11 + 3 * N, 2, 3
    nk = np.array([3, 2], dtype=np.int32)
    ids = np.array([[10, 11, 13], [10, 12, 0]], dtype=np.int32)
    H = np.ones((2, stride, rows, 3))
    r = np.full((2, stride, rows), 0.01)
    R = np.ascontiguousarray(np.broadcast_to(np.eye(rows), (2, stride, rows, rows)))
    G = np.full((2, n), -7.0)
    U = np.full((2, stride), 9, dtype=np.uint8)
    rep = (hip.LinearReport * 2)()
    for s in rep:
        s.nis, s.dof, s.info = -7.0, -7, -7
    mask01 = np.array([1, 0], dtype=np.uint8)

    def call(h, local=1, rw=rows, nn=nk, ii=ids, sd=stride, Hh=H, rr=r, RR=R, gate=np.inf, lm=np.inf, mask=None, u=U, g=G, ldg=n, rp=rep):
        return L.eqf_update_landmarks(h, local, rw, P(nn, ip), P(ii, ip), sd, P(Hh), P(rr), P(RR), gate, lm, P(mask, up), P(u, up), P(g), ldg, rp)

    def poisoned(a, idx, v):
        a = a.copy()
        a[idx] = v
        return a

    before = [_getters(fg, b) for b in range(2)]
    before32 = [f32.dump_state(b) for b in range(2)]
    bad = [dict(local=2), dict(local=-1), dict(rw=0), dict(rw=4), dict(nn=None), dict(ii=None), dict(Hh=None), dict(rr=None), dict(RR=None),
           dict(sd=0), dict(nn=np.array([4, 2], dtype=np.int32)), dict(nn=np.array([3, -1], dtype=np.int32)), dict(ldg=n - 1), dict(gate=np.nan),
           dict(gate=0.0), dict(gate=-1.0), dict(lm=np.nan), dict(lm=0.0), dict(Hh=poisoned(H, (1, 1, 1, 2), np.nan)),
           dict(Hh=poisoned(H, (0, 0, 0, 0), np.inf)), dict(rr=poisoned(r, (1, 1, 0), np.nan)), dict(RR=poisoned(R, (0, 2, 1, 0), np.inf)),
           dict(RR=poisoned(R, (1, 0, 0, 0), np.nan)), dict(Hh=poisoned(H, (0, 1, 0, 1), np.nan), mask=mask01)]
    for kw in bad:
        assert call(fg._h, **kw) == hip.ERR_INVALID, {k: (v if not isinstance(v, np.ndarray) else "array") for k, v in kw.items()}
    assert call(None) == hip.ERR_INVALID
    assert call(f32._h) == hip.ERR_UNSUPPORTED
    assert call(fg._h, ii=np.array([[10, 13, 11], [10, 12, 0]], dtype=np.int32)) == hip.ERR_UNSORTED
    assert call(fg._h, ii=np.array([[10, 11, 11], [10, 12, 0]], dtype=np.int32)) == hip.ERR_UNSORTED
    # more entries than the handle's capacity (and more than the state can hold): stride 6 > capacity 5
    big = np.array([6, 1], dtype=np.int32)
    assert call(fg._h, nn=big, sd=6, ii=np.arange(12, dtype=np.int32).reshape(2, 6) + 10, Hh=np.ones((2, 6, rows, 3)), rr=np.zeros((2, 6, rows)),
                RR=np.ascontiguousarray(np.broadcast_to(np.eye(rows), (2, 6, rows, rows))), u=None) == hip.ERR_CAPACITY
    assert np.all(G == -7.0) and np.all(U == 9) and all(s.nis == -7.0 and s.dof == -7 and s.info == -7 for s in rep)
    for b in range(2):
        _assert_same(_getters(fg, b), before[b], f"after the refused calls, slot {b}")
        _assert_same(f32.dump_state(b), before32[b], f"after the refused calls, fp32 slot {b}")
    assert fg.device_error() == 0 and f32.device_error() == 0
    # good arguments work; what is wrong with a masked-out filter's operands, beyond nk[b] or with an upper triangle is nobody's business
    assert call(fg._h, Hh=poisoned(poisoned(H, (1, 1, 0, 1), np.nan), (0, 2, 0, 0), 2.0), RR=poisoned(R, (0, 0, 0, 1), np.nan), mask=mask01) == 0
    assert [s.info for s in rep] == [0, 3] and rep[0].dof == 3 * rows and np.all(G[1] == 0.0) and G[0].any()
    assert list(U[0]) == [1, 1, 1] and list(U[1]) == [0, 0, 0]
    _assert_same(_getters(fg, 1), before[1], "masked-out slot")
    assert call(fg._h, u=None, g=None, ldg=0, rp=None) == 0  # (enqueues and returns)
    assert call(fg._h, mask=mask01, rr=poisoned(r, (1, 2, 1), np.nan)) == 0
    assert fg.device_error() == 0
    fg.close(), f32.close()
