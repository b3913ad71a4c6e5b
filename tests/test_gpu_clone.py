"""Copy, fork and resample filters on the device (csrc/eqf_clone.hpp: eqf_copy_filters, FilterBatch.copy_filters / resample,
VIOFilter.copyStateFrom).

The reference of every claim is the HOST ROUTE on a twin handle, restore_state(dump_state(...)), which tests/test_replay.py pins as a
bitwise resume and which shares no code with the device path.  "Same" is bit for bit (the bytes of every array) on every getter of the
public header: ids, time, state estimate, origin, group, bias, Sigma, integrator, last update and -- fp64 handles -- innovation statistics.

(Written without a GPU at hand: DESIGN.md section 4.5d records that these cases had not run on a device when they were added.)"""
import math
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = [0, 5, 18, 70]


@pytest.fixture(scope="module")
def hip():
    from eqf_vio_amd import binding

    return binding


@pytest.fixture(scope="module")
def stream70():
    from eqf_vio_amd import synth

    st = synth.make_stream(70, duration=0.6)  # 11 vision frames
    return st, synth.churn_measurements(st, seed=7, outlier_frames=(6, 8), outlier_angle=0.05)


def _settings(**kw):
    from eqf_vio_amd import synth

    d = synth.template_settings_dict()
    d.update(kw)
    return d


def _events(st, f0, f1):
    """The events of vision frames [f0, f1) with the IMU records in front of each, in the runner's order."""
    out, f = [], 0
    for kind, k in st.events():
        if f >= f1:
            break
        if f >= f0:
            out.append((kind, k))
        if kind == "vision":
            f += 1
    return out


def _run(fg, st, f0, f1, meas=None, nb=None, after_frame=None):
    for kind, k in _events(st, f0, f1):
        if kind == "imu":
            r = st.imu[k]
            fg.process_imu(r[0], r[1:4], r[4:7])
        else:
            if meas is not None:
                fg.process_vision(st.vision_stamps[k], *meas[k])
            else:
                fg.process_vision(st.vision_stamps[k], st.ids, st.bearings[k], nb=nb)
            if after_frame:
                after_frame(k)


def _getters(fg, b, f64=True, local=False):
    g = dict(n=fg.num_landmarks(b), est=fg.state_estimate(b), last=fg.last_update(b))
    g.update(fg.dump_state(b))  # ids, origin, group, bias, sigma, time, integrator
    if f64:
        g["innov"] = fg.innovation_stats(b)
    if local:
        g["sigma_local"] = fg.sigma_local(b)
    return g


def _bits(x):
    if isinstance(x, dict):
        return {k: _bits(v) for k, v in x.items()}
    return np.ascontiguousarray(x).tobytes() + str(np.asarray(x).shape).encode()


def _assert_same(a, b, what):
    a, b = _bits(a), _bits(b)
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k], f"{what}: getter {k} differs"


def _all(fg, **kw):
    return [_getters(fg, b, **kw) for b in range(fg.B)]


def _source(hip, st, **kw):
    """Batch 4, capacity 77, landmark counts 0 / 5 / 18 / 70 after five frames: internal orders 12, 27, 66, 222."""
    fg = hip.FilterBatch(_settings(**kw), capacity=77, batch=4)
    fg.set_option("innovation_stats", 1)
    _run(fg, st, 0, 5, nb=COUNTS)
    assert [fg.num_landmarks(b) for b in range(4)] == COUNTS
    return fg


def _twin(hip, settings, capacity, snaps):
    tw = hip.FilterBatch(settings, capacity=capacity, batch=len(snaps))
    tw.set_option("innovation_stats", 1)
    for b, s in enumerate(snaps):
        tw.restore_state(s, b)
    return tw


def _state_keys(g):
    """What every later frame is compared on: ids, Sigma, state, innovation statistics (and the rest of the dump)."""
    return {k: v for k, v in g.items() if k != "last"}


def test_across_handles_with_other_layouts_and_continuation_with_churn(hip, stream70):
    """Cases 1 and 2 of the issue: capacity 77 -> capacity 70 (ld 224, exact fit) and -> batch 6 of capacity 200 (ld 624) in a permuted slot
    order, then five more frames with churn and the default outlier gate against host-route twins.  Slot 1 of the batch-6 handle held 70
    landmarks and receives the filter of 5: stale rows beyond N that later appends grow into.  The source runs its five frames with the
    template's settings (gate off: with it on, the first frames of a fresh filter already drop landmarks and the counts are not 0 / 5 /
    18 / 70); the gate is a setting of the destinations and of their twins, and settings are not copied."""
    st, meas = stream70
    gate = dict(outlierThreshold=0.01)
    src = _source(hip, st)
    before = _all(src, local=True)
    # capacity 70: only an exact fit for the largest
    d70 = hip.FilterBatch(_settings(**gate), capacity=70, batch=4)
    d70.set_option("innovation_stats", 1)
    d70.copy_filters(src, [0, 1, 2, 3], [0, 1, 2, 3])
    # batch 6, capacity 200, with a history of its own: slots 1 and 4 held 70 landmarks
    d200 = hip.FilterBatch(_settings(**gate), capacity=200, batch=6)
    d200.set_option("innovation_stats", 1)
    _run(d200, st, 0, 3, nb=[3, 70, 7, 0, 70, 12])
    own = _all(d200, local=True)
    assert own[1]["n"] > 5 and own[4]["n"] > 0  # (more landmarks than their new occupants bring)
    dst_idx, src_idx = [4, 1, 5, 0], [0, 1, 2, 3]  # 70 -> 5 in slot 1, 70 -> 0 in slot 4; slots 2 and 3 are not named
    d200.copy_filters(src, dst_idx, src_idx)
    assert src.device_error() == 0 and d70.device_error() == 0 and d200.device_error() == 0
    for b in range(4):
        _assert_same(_getters(d70, b, local=True), before[b], f"capacity 70 filter {b}")
        _assert_same(_getters(src, b, local=True), before[b], f"source filter {b} after the copies")
    for d, s in zip(dst_idx, src_idx):
        _assert_same(_getters(d200, d, local=True), before[s], f"capacity 200 slot {d} <- {s}")
    for b in (2, 3):
        _assert_same(_getters(d200, b, local=True), own[b], f"capacity 200 slot {b} (not named)")
    # eqf_get_nees follows: the copies against the source, every filter in one call
    ns, n70 = src.nees(None, local=True), d70.nees(None, local=True)
    assert all(ns[k].tobytes() == n70[k].tobytes() for k in ("logdet", "min_pivot", "dof", "info"))
    # ---- continuation against twins restored through the host
    plain = lambda gs: [{k: v for k, v in g.items() if k != "sigma_local"} for g in gs]
    t70 = _twin(hip, _settings(**gate), 70, plain(before))
    snaps200 = plain(own)
    for d, s in zip(dst_idx, src_idx):
        snaps200[d] = plain(before)[s]
    t200 = _twin(hip, _settings(**gate), 200, snaps200)
    frames = []

    def compare(k):
        frames.append(k)
        for a, t, what in ((d70, t70, "capacity 70"), (d200, t200, "capacity 200")):
            for b in range(a.B):
                _assert_same(_state_keys(_getters(a, b)), _state_keys(_getters(t, b)), f"{what} filter {b} after frame {k}")

    for k in range(5, 10):
        for fg in (d70, t70, d200, t200):
            _run(fg, st, k, k + 1, meas=meas)
        compare(k)
    assert frames == [5, 6, 7, 8, 9]
    assert d200.num_landmarks(1) > 5  # (the filter of 5 grew into the rows its slot's earlier occupant left behind)
    assert all(fg.device_error() == 0 for fg in (d70, t70, d200, t200))


@pytest.mark.parametrize("parents", [[1, 0, 2, 3], [1, 2, 0, 3], [1, 2, 3, 3], [3, 3, 3, 3], [0, 1, 2, 3]],
                         ids=["swap", "cycle", "shift", "fanout", "identity"])
def test_in_place(hip, stream70, parents):
    """A gather inside one handle: every source is read as it was before the call."""
    st, meas = stream70
    fg = _source(hip, st)
    snaps = _all(fg)
    fg.resample(parents)
    for b in range(4):
        _assert_same(_getters(fg, b), snaps[parents[b]], f"filter {b} <- {parents[b]}")
    tw = _twin(hip, _settings(), 77, [snaps[p] for p in parents])
    for h in (fg, tw):
        _run(h, st, 5, 6, meas=meas)
    for b in range(4):
        _assert_same(_state_keys(_getters(fg, b)), _state_keys(_getters(tw, b)), f"filter {b} one frame on")
    assert fg.device_error() == 0 and tw.device_error() == 0


def test_deferred_work_is_settled_first(hip, stream70):
    """The call directly behind six queued IMU calls and directly behind a vision call whose gate answer is pending, no getter in between,
    against the same sequence with synchronize() on both handles first."""
    st, meas = stream70
    got = []
    for sync in (False, True):
        src = hip.FilterBatch(_settings(outlierThreshold=0.01), capacity=77, batch=4)
        dst = hip.FilterBatch(_settings(outlierThreshold=0.01), capacity=77, batch=4)
        _run(src, st, 0, 5, nb=COUNTS)
        _run(dst, st, 0, 2, nb=[7, 7, 7, 7])
        ev = _events(st, 5, 7)
        nv = [i for i, e in enumerate(ev) if e[0] == "vision"]
        assert nv[0] >= 6 and nv[1] - nv[0] > 6
        res = []
        # frame 5 without its vision call: the last six IMU calls are a burst that is queued, not launched
        for i, (kind, k) in enumerate(ev[: nv[0]]):
            if i == nv[0] - 6:
                src.synchronize()
            src.process_imu(st.imu[k][0], st.imu[k][1:4], st.imu[k][4:7])
        if sync:
            src.synchronize(), dst.synchronize()
        dst.copy_filters(src, [3, 2, 1, 0], [0, 1, 2, 3])
        res.append(_all(dst))
        # the vision call with an outlier frame's churn (frame 6 is an outlier frame; 5 first), its gate pending
        src.process_vision(st.vision_stamps[5], *meas[5])
        for kind, k in ev[nv[0] + 1 : nv[1]]:
            src.process_imu(st.imu[k][0], st.imu[k][1:4], st.imu[k][4:7])
        src.process_vision(st.vision_stamps[6], *meas[6])
        if sync:
            src.synchronize(), dst.synchronize()
        dst.copy_filters(src, [0, 1, 2, 3], [0, 1, 2, 3])
        res.append(_all(dst))
        res.append(_all(src))
        assert src.device_error() == 0 and dst.device_error() == 0
        got.append(res)
    _assert_same({str(i): {str(b): g for b, g in enumerate(r)} for i, r in enumerate(got[0])},
                 {str(i): {str(b): g for b, g in enumerate(r)} for i, r in enumerate(got[1])}, "deferred against synchronised")
    for b in range(4):  # (and the last copy is a copy)
        _assert_same(got[0][1][b], got[0][2][b], f"filter {b} behind a pending gate")


def test_other_settings_stay_the_destinations(hip, stream70):
    """The state is copied, the settings are not: a destination with another measurementVariance and camera offset equals a twin of THOSE
    settings restored through the host, over three further frames."""
    st, meas = stream70
    src = _source(hip, st)
    q = np.array([0.98, 0.1, -0.1, math.sqrt(1 - 0.98 * 0.98 - 0.02)])
    other = _settings(measurementVariance=0.01, cameraOffset_q=q, cameraOffset_x=np.array([0.1, -0.05, 0.02]))
    dst = hip.FilterBatch(other, capacity=80, batch=4)
    dst.set_option("innovation_stats", 1)
    dst.copy_filters(src, [0, 1, 2, 3], [0, 1, 2, 3])
    snaps = _all(src)
    tw = _twin(hip, other, 80, snaps)
    ref = hip.FilterBatch(_settings(), capacity=80, batch=4)  # (the source's settings: must come out different)
    for b in range(4):
        ref.restore_state(snaps[b], b)
    for k in range(5, 8):
        for h in (dst, tw, ref):
            _run(h, st, k, k + 1, meas=meas)
        for b in range(4):
            _assert_same(_state_keys(_getters(dst, b)), _state_keys(_getters(tw, b)), f"filter {b} after frame {k}")
    assert not np.array_equal(dst.sigma(3), ref.sigma(3))
    assert dst.device_error() == 0 and tw.device_error() == 0


def test_stream_mode(hip):
    """Between two stream-mode handles after stream_vision(2); frames 3-5 bitwise against a twin."""
    from eqf_vio_amd import synth

    N = 18
    st = synth.make_stream(N, duration=0.4)
    hs = [hip.FilterBatch(_settings(), capacity=N + 3, batch=2) for _ in range(3)]
    for h in hs:
        h.stream_upload(st.imu, st.vision_stamps, st.ids, st.bearings)
    a, b, t = hs

    def run(h, f0, f1):
        for kind, k in _events(st, f0, f1):
            h.stream_imu(k) if kind == "imu" else h.stream_vision(k)

    run(a, 0, 3)
    b.copy_filters(a, [1, 0], [0, 1])
    for d, s in ((1, 0), (0, 1)):
        t.restore_state(a.dump_state(s), d)
        _assert_same(_getters(b, d), _getters(a, s), f"stream handle slot {d}")
    for f in range(3, 6):
        run(b, f, f + 1), run(t, f, f + 1)
        for d in range(2):
            _assert_same(_state_keys(_getters(b, d)), _state_keys(_getters(t, d)), f"slot {d} after frame {f}")
    assert all(h.device_error() == 0 for h in hs)


def test_f32_to_f32(hip):
    from eqf_vio_amd import synth

    N = 18
    st = synth.make_stream(N, duration=0.4)
    a = hip.FilterBatch(_settings(), capacity=N, batch=1, precision=hip.PRECISION_F32)
    b = hip.FilterBatch(_settings(), capacity=N + 9, batch=2, precision=hip.PRECISION_F32)
    _run(a, st, 0, 4)
    assert a.num_landmarks(0) == N
    b.copy_filters(a, [1], [0])
    _assert_same(_getters(b, 1, f64=False), _getters(a, 0, f64=False), "fp32 copy")
    fresh = _getters(b, 0, f64=False)
    b.resample([1, 0])  # (a swap: both go through the staging image)
    _assert_same(_getters(b, 0, f64=False), _getters(a, 0, f64=False), "fp32 swap in place, slot 0")
    _assert_same(_getters(b, 1, f64=False), fresh, "fp32 swap in place, slot 1")
    assert a.device_error() == 0 and b.device_error() == 0


def test_errors_come_before_any_effect(hip, stream70):
    st, _ = stream70
    src = _source(hip, st)
    dst = hip.FilterBatch(_settings(), capacity=77, batch=4)
    small = hip.FilterBatch(_settings(), capacity=20, batch=4)
    f32 = hip.FilterBatch(_settings(), capacity=77, batch=4, precision=hip.PRECISION_F32)
    for h in (dst, small):
        h.set_option("innovation_stats", 1)
        _run(h, st, 0, 2, nb=[4, 9, 0, 6])
    _run(f32, st, 0, 2, nb=[4, 9, 0, 6])
    snap = {id(h): _all(h, f64=h is not f32) for h in (src, dst, small, f32)}
    cases = [
        (dst, src, [0, 1, 0], [1, 2, 3], hip.ERR_INVALID),     # a destination named twice
        (dst, src, [0, 4], [1, 2], hip.ERR_INVALID),           # destination index out of range
        (dst, src, [0, 1], [1, -1], hip.ERR_INVALID),          # source index out of range
        (dst, dst, [0, 1, 1], [1, 0, 2], hip.ERR_INVALID),     # in place, named twice
        (small, src, [0, 1, 2], [0, 1, 3], hip.ERR_CAPACITY),  # 70 landmarks into capacity 20 (the pairs in front of it included)
        (f32, src, [0], [1], hip.ERR_UNSUPPORTED),             # F64 -> F32
        (src, f32, [0], [1], hip.ERR_UNSUPPORTED),             # F32 -> F64
    ]
    for d, s, di, si, code in cases:
        with pytest.raises(hip.EqfError) as e:
            d.copy_filters(s, di, si)
        assert e.value.code == code, (di, si)
        for h in (src, dst, small, f32):
            for b in range(4):
                _assert_same(_getters(h, b, f64=h is not f32), snap[id(h)][b], f"after the refused call {di} <- {si}")
            assert h.device_error() == 0
    dst.copy_filters(src, [], [])  # n = 0 is fine, and moves nothing
    for b in range(4):
        _assert_same(_getters(dst, b), snap[id(dst)][b], "n = 0")
    small.copy_filters(src, [3, 0], [1, 2])  # (what fits is copied)
    _assert_same(_getters(small, 3), snap[id(src)][1], "5 landmarks into capacity 20")
    _assert_same(_getters(small, 0), snap[id(src)][2], "18 landmarks into capacity 20")


def test_cpp_facade_against_the_python_binding_bit_for_bit(hip):
    """VIOFilter::copyStateFrom of cpp/VIOFilter.h through the example binary (argument `clone`: a fork with twice the measurement variance
    after frames / 2 frames, both run on; hexadecimal floats) against filter.VIOFilter.copyStateFrom on the same sequence."""
    from eqf_vio_amd import filter as vf

    N, frames = 20, 6
    exe = os.path.join(ROOT, "eqf_vio_amd", "cpp", "eqf_example")
    out = subprocess.run([exe, str(N), str(frames), "clone"], capture_output=True, text=True, check=True).stdout.splitlines()
    lines = {ln.split()[0]: ln.split()[1:] for ln in out if ln.startswith("clone_")}
    assert sorted(lines) == ["clone_a", "clone_b"]
    base = dict(initialPointVariance=5000.0, measurementVariance=0.003, velOmegaVariance=1e-4, velAccelVariance=1e-4, outlierThreshold=1e9)
    fa = vf.VIOFilter(hip.settings_from_dict(base), capacity=N)
    fb = None
    lm = np.array([[2 * math.sin(1.3 * i), 2 * math.cos(0.7 * i), 5 + math.sin(0.37 * i)] for i in range(N)])
    y = np.array([[v[0] / n, v[1] / n, v[2] / n] for v, n in ((v, math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])) for v in lm)])
    k = 0
    for f in range(frames):
        stamp = 0.05 * f + 0.0025
        while 0.005 * k < stamp:
            for h in (fa, fb):
                if h is not None:
                    h.processIMUData(vf.IMUVelocity(0.005 * k, np.zeros(3), np.array([9.81, 0, 0])))
            k += 1
        for h in (fa, fb):
            if h is not None:
                h.processVisionData(vf.VisionMeasurement(stamp, np.arange(N, dtype=np.int32), y))
        fa.stateEstimate()  # (the example reads the state after every vision call)
        if f + 1 == frames // 2:
            fb = vf.VIOFilter(hip.settings_from_dict(dict(base, measurementVariance=2 * 0.003)), capacity=N)
            fb.copyStateFrom(fa)
    for tag, h in (("clone_a", fa), ("clone_b", fb)):
        e, S = h.stateEstimate(), h.stateCovariance()
        want = np.concatenate([e.pose_q, e.pose_x, e.velocity, S.reshape(-1)])
        ln = lines[tag]
        assert int(ln[0]) == N == len(e.ids)
        got = np.array([float.fromhex(x) for x in ln[1:]])
        assert got.tobytes() == want.tobytes(), tag
    assert lines["clone_a"] != lines["clone_b"]  # (the fork has its own measurement variance)


def test_resample_end_to_end(hip):
    """loglik (innovation_stats) -> systematic_resample -> resample: eight filters of N = 21, two of them fed bearings with 0.05 rad of
    added noise.  Both are replaced, and every filter equals its parent's snapshot.  No accuracy number is asserted."""
    from eqf_vio_amd import consistency, synth

    N, B, bad = 21, 8, (2, 5)
    st = synth.make_stream(N, duration=0.4)
    rng = np.random.default_rng(5)
    fg = hip.FilterBatch(_settings(), capacity=N, batch=B)
    fg.set_option("innovation_stats", 1)
    for kind, k in _events(st, 0, 6):
        if kind == "imu":
            r = st.imu[k]
            fg.process_imu(r[0], r[1:4], r[4:7])
        else:
            y = np.broadcast_to(st.bearings[k], (B, N, 3)).copy()
            for b in bad:
                nz = 0.05 * rng.standard_normal((N, 3))
                nz -= np.sum(nz * y[b], axis=1, keepdims=True) * y[b]
                y[b] = (y[b] + nz) / np.linalg.norm(y[b] + nz, axis=1, keepdims=True)
            fg.process_vision(st.vision_stamps[k], st.ids, y)
    stats = [fg.innovation_stats(b) for b in range(B)]
    assert all(s["valid"] for s in stats)
    loglik = np.array([s["loglik"] for s in stats])
    print("loglik", loglik)
    parents = consistency.systematic_resample(loglik, 0.5)
    print("parents", parents)
    assert not set(bad) & set(int(p) for p in parents)
    snaps = _all(fg)
    fg.resample(parents)
    for b in range(B):
        _assert_same(_getters(fg, b), snaps[parents[b]], f"filter {b} <- {parents[b]}")
    assert fg.device_error() == 0
