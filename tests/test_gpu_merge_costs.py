"""The pairwise merge costs and the greedy mixture reduction on the device (eqf_get_merge_costs, csrc/eqf_mergecost.hpp;
FilterBatch.reduce_mixture) against the exact reference of tests/mergecost_exact.py built from the device's own getters, record by record
and inside the a-priori bound; the bitwise facts the header promises; non-mutation; verdicts and errors; the reduction's merge log against
the numpy statement's on the committed cluster cases.  Sizes: mergecost_cases.SIZES -- with first = 0 internal orders 12, 15, 63, 66, 129
and 258, each side of the 64-wide block column edges."""
import ctypes as C

import numpy as np
import pytest

import mergecost_cases as gc
import mergecost_exact as gx
import mixture_cases as mc
import mixture_exact as mx
from eqf_vio_amd import consistency as cs

pytestmark = pytest.mark.gpu

SOME = [(0, 1), (5, 1), (2, 4), (3, 5), (3, 0), (1, 2)]  # a repeated index, the weight of 0, the centre, pairs named both ways round
CAP_EXTRA = 3


@pytest.fixture(scope="module")
def hip():
    from eqf_vio_amd import binding

    return binding


def _bits(x):
    if isinstance(x, dict):
        return {k: _bits(v) for k, v in x.items()}
    return np.ascontiguousarray(x).tobytes() + str(np.asarray(x).shape).encode()


def _same(a, b, what):
    a, b = _bits(a), _bits(b)
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k], f"{what}: {k} differs"


def _getters(fg, b):
    g = dict(n=fg.num_landmarks(b), est=fg.state_estimate(b), gate=fg.gate_report(b), last=fg.last_update(b), innov=fg.innovation_stats(b),
             err=fg.device_error())
    g.update(fg.dump_state(b))
    return g


def _member(fg, b):
    m = fg.dump_state(b)
    m["estimate"] = fg.state_estimate(b)
    return m


def _handle(hip, N, batch=gc.POOL, order=None, cap=None):
    fg = hip.FilterBatch(mc.cc.settings(), capacity=(N + CAP_EXTRA) if cap is None else cap, batch=batch)
    for b, k in enumerate(order if order is not None else range(batch)):
        if k is not None:
            fg.restore_state(mc.member(N, k), b)
    return fg


RECORD = ("cost", "logdet_pair", "maha", "info", "member_logdet", "member_min_pivot", "member_dof", "member_info")


def _records(r, keys=RECORD):
    return {k: r[k] for k in keys}


# ---- 1. entry by entry
@pytest.mark.parametrize("N", gc.SIZES)
def test_records_entry_by_entry(hip, N):
    fg = _handle(hip, N)
    pool = [_member(fg, b) for b in range(gc.POOL)]
    ms, w, ref = gc.case(N, pool)
    idx = list(gc.IDX)
    imgs, cache = gx.member_images(ms, ref, mc.K_E), {}
    worst = {}
    for kind in gx.KINDS:
        for first in gc.FIRSTS:
            pairs = None if (N < 39 and first == 0) else SOME
            got = fg.merge_costs(idx, w, ref=idx[ref], kind=kind, first=first, pairs=pairs)
            R = gx.reference(ms, w, ref, kind, first, pairs, mc.K_E, gc.K_LOG1P, imgs, cache)
            assert R["bound"]["validity"] <= gx.VALIDITY
            assert not got["info"].any() and not got["member_info"].any()
            assert np.all(got["member_dof"] == 11 + 3 * N - first)
            if pairs is None:
                M = got["matrix"]
                assert np.array_equal(M, M.T) and not np.diag(M).any() and M[0, 1] == got["cost"][0]
            r = gx.ratios(got, R)
            for k, v in r.items():
                worst[k] = max(worst.get(k, 0.0), v)
            print(f"N={N} {kind} first={first}: " + " ".join(f"{k} {v:.4f}" for k, v in r.items()))
            assert max(r.values()) <= 1.0, (N, kind, first, r)
    print(f"N={N} worst device/bound ratios {worst}")
    assert fg.device_error() == 0
    fg.close()


# ---- 2. bitwise facts
@pytest.mark.parametrize("N", (17, 18))
def test_bitwise_facts(hip, N):
    fg = _handle(hip, N, batch=6)
    fg.copy_filters(fg, [5], [1])
    idx, w, ref = [0, 1, 2, 3, 4, 1, 5], np.array([0.5, 0.3, 0.0, 1.0, 0.7, 0.2, 0.4]), 3
    for kind, first in (("runnalls", 0), ("bhattacharyya", 6), ("runnalls", 11)):
        a = fg.merge_costs(idx, w, ref=ref, kind=kind, first=first)
        _same(_records(a), _records(fg.merge_costs(idx, w, ref=ref, kind=kind, first=first)), "run to run")
        pp = a["pairs"]
        # each pair alone; the pairs reversed and permuted
        for k in (0, 7, len(pp) - 1):
            one = fg.merge_costs(idx, w, ref=ref, kind=kind, first=first, pairs=[pp[k]])
            for q in ("cost", "logdet_pair", "maha", "info"):
                assert _bits(one[q][0]) == _bits(a[q][k]), f"pair {k} alone: {q}"
        perm = np.random.default_rng(N).permutation(len(pp))
        b = fg.merge_costs(idx, w, ref=ref, kind=kind, first=first, pairs=pp[perm][:, ::-1])
        for q in ("cost", "logdet_pair", "maha", "info"):
            assert _bits(b[q]) == _bits(a[q][perm]), f"reversed and permuted: {q}"
        _same(_records(b, RECORD[4:]), _records(a, RECORD[4:]), "member records with other pairs")
        # the chunking
        for chunk in (1, 3):
            fg.set_option("merge_cost_chunk", chunk)
            _same(_records(fg.merge_costs(idx, w, ref=ref, kind=kind, first=first)), _records(a), f"chunk {chunk}")
        fg.set_option("merge_cost_chunk", 0)
        # identical members cost exactly 0: the same filter twice (positions 1, 5) and its copy made by eqf_copy_filters (position 6)
        for i, j in ((1, 5), (1, 6), (5, 6)):
            k = [q for q in range(len(pp)) if tuple(pp[q]) == (i, j)][0]
            assert a["cost"][k] == 0.0 and a["maha"][k] == 0.0 and a["logdet_pair"][k] == a["member_logdet"][i], (kind, first, i, j)
        # the member that IS ref against eqf_get_nees(local = 1)
        nees = fg.nees(local=True, first=first)
        k = idx.index(ref)
        for q, v in (("logdet", "member_logdet"), ("min_pivot", "member_min_pivot"), ("dof", "member_dof"), ("info", "member_info")):
            assert _bits(nees[q][ref]) == _bits(a[v][k]), q
    # the same members restored into a handle of 7 at other slots (ragged: other sizes around them)
    a = fg.merge_costs([0, 1, 2, 3, 4], w[:5], ref=3)
    fr = hip.FilterBatch(mc.cc.settings(), capacity=N + 40, batch=7)
    place = {0: 6, 1: 2, 2: 5, 3: 0, 4: 3}
    for k, b in place.items():
        fr.restore_state(mc.member(N, k), b)
    fr.restore_state(mc.member(33, 1), 1)
    fr.restore_state(mc.member(5, 2), 4)
    c = fr.merge_costs([place[k] for k in range(5)], w[:5], ref=place[3])
    _same(_records(c), _records(a), "where the members are")
    with pytest.raises(hip.EqfError):
        fg.set_option("merge_cost_chunk", 4097)
    assert fg.device_error() == 0 and fr.device_error() == 0
    fg.close(), fr.close()


# ---- 3. non-mutation
def _run(h, st, events):
    for kind, k in events:
        if kind == "imu":
            h.process_imu(st.imu[k][0], st.imu[k][1:4], st.imu[k][4:7])
        else:
            h.process_vision(st.vision_stamps[k], st.ids, st.bearings[k])


def _frames(st, f0, f1):
    out, f = [], 0
    for kind, k in st.events():
        if f >= f1:
            break
        if f >= f0:
            out.append((kind, k))
        if kind == "vision":
            f += 1
    return out


def test_the_call_only_reads_and_a_twin_that_never_asked_runs_on_bit_for_bit(hip):
    from eqf_vio_amd import synth

    N, B = 20, 4
    st = synth.make_stream(N, duration=0.4)
    d = synth.template_settings_dict()
    fa, fb = hip.FilterBatch(d, capacity=N + 4, batch=B), hip.FilterBatch(d, capacity=N + 4, batch=B)
    for f in (fa, fb):
        f.set_option("innovation_stats", 1)
        _run(f, st, _frames(st, 0, 3))
        f.resample(np.zeros(B, dtype=np.int32))
        f.perturb(np.random.default_rng(5), scale=[0.0, 0.02, 0.05, 0.03])
        _run(f, st, _frames(st, 3, 4))
    nxt = _frames(st, 4, 5)
    _run(fa, st, nxt[:3]), _run(fb, st, nxt[:3])  # (three IMU calls are queued when the question arrives: it settles them)
    w = cs.mixture_weights([-1.0, -0.5, -2.0, -0.8])
    first = fa.merge_costs([0, 1, 2, 3], w, ref=1)
    assert not first["info"].any() and np.all(first["cost"] > 0.0)
    before = [_getters(fa, b) for b in range(B)]
    sl = [fa.sigma_local(b) for b in range(B)]
    for kind in gx.KINDS:
        for fst in gc.FIRSTS:
            fa.merge_costs([0, 1, 2, 3], w, ref=1, kind=kind, first=fst)
    for b in range(B):
        _same(_getters(fa, b), before[b], f"filter {b} after the calls")
        _same(_getters(fa, b), _getters(fb, b), f"filter {b} against the twin that never asked")
        assert _bits(fa.sigma_local(b)) == _bits(sl[b])
    for f, ev in ((4, nxt[3:]), (5, _frames(st, 5, 6))):
        _run(fa, st, ev), _run(fb, st, ev)
        fa.merge_costs([0, 1, 2, 3], w, ref=1, pairs=[(0, 1)])
        for b in range(B):
            _same(_getters(fa, b), _getters(fb, b), f"slot {b} after frame {f}")
    assert fa.device_error() == 0 and fb.device_error() == 0
    fa.close(), fb.close()


# ---- 4. verdicts
def test_trouble_of_one_member_stays_in_its_pairs(hip):
    N = 17
    fg = _handle(hip, N, batch=5)
    idx, w = [0, 1, 2, 3, 4], np.array([0.5, 0.3, 0.6, 1.0, 0.7])
    clean = fg.merge_costs(idx, w, ref=3)
    S = fg.sigma(2)
    S[20, 20] = -S[20, 20]  # indefinite
    fg.set_sigma(S, 2)
    got = fg.merge_costs(idx, w, ref=3)
    hit = np.array([2 in p for p in got["pairs"]])
    assert np.all(got["info"][hit] == 1) and not got["info"][~hit].any()
    assert np.all(got["member_info"] == [0, 0, 1, 0, 0]) and np.isnan(got["member_logdet"][2])
    for q in ("cost", "logdet_pair", "maha"):
        assert np.isnan(got[q][hit]).all(), q
        assert _bits(got[q][~hit]) == _bits(clean[q][~hit]), f"{q}: another pair's record moved"
    S[20, 20] = np.nan
    fg.set_sigma(S, 2)
    got = fg.merge_costs(idx, w, ref=3, kind="bhattacharyya", first=6)
    cb = fg.merge_costs([0, 1, 3, 4], w[[0, 1, 3, 4]], ref=3, kind="bhattacharyya", first=6)
    assert np.all(got["info"][hit] == 1) and not got["info"][~hit].any()
    assert _bits(got["cost"][~hit]) == _bits(cb["cost"]), "a NaN reached another pair's record"
    # a level member: the gravity chart of its estimate is singular
    level = mc.member(N, 3)
    level["group"]["Aq"] = level["origin"]["q"] * np.array([1.0, -1.0, -1.0, -1.0])
    fg.restore_state(level, 2)
    got = fg.merge_costs(idx, w, ref=3)
    assert np.all(got["info"][hit] == -1) and not got["info"][~hit].any() and np.all(got["member_info"] == [0, 0, -1, 0, 0])
    assert np.isnan(got["cost"][hit]).all() and _bits(got["cost"][~hit]) == _bits(clean["cost"][~hit])
    fu = hip.FilterBatch(mc.cc.settings(), capacity=4, batch=2)  # fresh, uninitialised filters are level too
    u = fu.merge_costs([0, 1], [1.0, 1.0], ref=0)
    assert u["info"][0] == -1 and np.all(u["member_info"] == -1)
    assert fg.device_error() == 0 and fu.device_error() == 0
    fg.close(), fu.close()


# ---- 5. errors
def test_argument_errors_come_before_any_effect(hip):
    N = 5
    fg = _handle(hip, N, batch=4, order=[0, 1, 2, 3])
    other = mc.member(N, 1)
    other["ids"] = other["ids"] + 1
    fg.restore_state(other, 3)  # other ids
    before = [_getters(fg, b) for b in range(4)]
    L, h = hip.lib(), fg._h
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    out, mem = (hip.PairCost * 8)(), (hip.SigmaStats * 8)()

    def costs(idx, w, ref, kind=0, first=0, npairs=None, pairs=None, handle=h, o=out, m=mem):
        i, ww = np.asarray(idx, dtype=np.int32), np.asarray(w, dtype=np.float64)
        n = len(i)
        pp = None if pairs is None else np.asarray(pairs, dtype=np.int32)
        npairs = (n * (n - 1) // 2 if pairs is None else len(pp)) if npairs is None else npairs
        return L.eqf_get_merge_costs(handle, n, i.ctypes.data_as(ip), ww.ctypes.data_as(dp), ref, kind, first, npairs,
                                     None if pp is None else pp.ctypes.data_as(ip), o, m)

    inv = hip.ERR_INVALID
    assert costs([0, 1, 2], [1.0, 1.0, 1.0], 0) == 0
    assert costs([0, 1, 2], [1.0, 1.0, 1.0], 0, npairs=0) == 0 and costs([0], [1.0], 0) == 0   # the member records alone; n = 1
    assert costs([0, 1, 2], [1.0, 1.0, 1.0], 0, m=None) == 0
    assert costs([0, 1], [1.0, 1.0], 0, handle=None) == inv
    for idx, w, ref in (([0, 4], [1.0, 1.0], 0), ([0, -1], [1.0, 1.0], 0), ([0, 1], [1.0, 1.0], 4), ([0, 1], [1.0, 1.0], 2),
                        ([0, 1], [1.0, -0.5], 0), ([0, 1], [1.0, np.nan], 0), ([0, 1], [0.0, 0.0], 0), ([0, 3], [1.0, 1.0], 0)):
        assert costs(idx, w, ref) == inv, (idx, w, ref)
    assert costs([0, 1], [1.0, 1.0], 0, kind=2) == inv and costs([0, 1], [1.0, 1.0], 0, kind=-1) == inv
    assert costs([0, 1], [1.0, 1.0], 0, first=5) == inv and costs([0, 1], [1.0, 1.0], 0, first=12) == inv
    assert costs([0, 1], [1.0, 1.0], 0, npairs=-1) == inv and costs([0, 1], [1.0, 1.0], 0, npairs=2) == inv
    assert costs([0, 1], [1.0, 1.0], 0, pairs=[(0, 2)]) == inv and costs([0, 1], [1.0, 1.0], 0, pairs=[(-1, 0)]) == inv
    assert costs([0, 1], [1.0, 1.0], 0, o=None) == inv
    for b in range(4):
        _same(_getters(fg, b), before[b], f"filter {b} after the refused calls")
    f32 = hip.FilterBatch(mc.cc.settings(), capacity=8, batch=2, precision=hip.PRECISION_F32)
    assert costs([0, 1], [1.0, 1.0], 0, handle=f32._h) == hip.ERR_UNSUPPORTED
    assert fg.device_error() == 0
    fg.close(), f32.close()


# ---- 6. the greedy reduction
@pytest.mark.parametrize("N", gc.CLUSTER_SIZES)
@pytest.mark.parametrize("kind", gx.KINDS)
def test_reduce_mixture_follows_the_numpy_statement(hip, N, kind):
    ms, w, lab = gc.cluster_case(N)
    n = len(ms)
    fg = hip.FilterBatch(mc.cc.settings(), capacity=N + CAP_EXTRA, batch=n + 1)
    slots = [k + 1 for k in range(n)]  # (slot 0 stays empty: indices are not positions)
    for m, b in zip(ms, slots):
        fg.restore_state(m, b)
    dev = [_member(fg, b) for b in slots]
    alive_h, wk_h, left_h, log_h = cs.reduce_mixture_host(dev, w, gc.CLUSTER_TARGET, kind=kind)
    idx_d, wk_d, log_d = fg.reduce_mixture(slots, w, gc.CLUSTER_TARGET, kind=kind)
    assert [p for p, _ in log_d] == [p for p, _ in log_h], (log_d, log_h)
    assert list(idx_d) == [slots[k] for k in alive_h] and _bits(wk_d) == _bits(wk_h)
    for (p, cd), (_, ch) in zip(log_d, log_h):
        print(f"N={N} {kind}: merged {p} device cost {cd:.6e} host {ch:.6e}")
        assert abs(cd - ch) <= 1e-3 * abs(ch)   # (near-copies: costs of 1e-6, bounds of 1e-12; the decisions carry the margin)
    # the survivors' moments against the reference of the numpy statement's survivors
    ref_pos = int(np.argmax(wk_h))
    got = fg.mixture_moments(list(idx_d), wk_d, int(idx_d[ref_pos]))
    R = mx.reference(left_h, wk_h, ref_pos, True, mc.K_E)
    r = mx.ratios(got, R)
    print(f"N={N} {kind}: survivors' moments, device against the statement's survivors: " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert got["info"] == 0 and max(r[k] for k in ("mean", "P")) <= 1.0, r
    assert fg.device_error() == 0
    fg.close()
