"""A handle's on-demand buffers grow under a larger call and are kept by a smaller one (csrc/eqf_workspace_host.hpp's reserve() over the
HIP backend of eqf_capi.hip): every route that sizes a buffer by the call makes a small call, a larger call and the small call again on ONE
handle.

Shapes: one fp64 handle of 4 filters, capacity 24, holding 5, 22, 0 and 13 landmarks; the master state is restored with copy_filters before
every mutating call.  Reference: a FRESH handle holding the same state that makes only the large call of the case -- its buffers are
allocated at that size at once, nothing is replaced.  Pass condition: outputs and the state afterwards (Sigma, ids, the getters) are
equal bit for bit -- growing a buffer changes where the operands lie, never what the kernels compute, so this is a derived condition and
not a tolerance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUNTS = [5, 22, 0, 13]
CAP = 24
ALL = [0, 1, 2, 3]


@pytest.fixture(scope="module")
def hip():
    from eqf_vio_amd import binding

    return binding


@pytest.fixture(scope="module")
def world(hip):
    """(settings, stream, master handle): five frames of a 22-landmark stream, filter b seeing the first COUNTS[b] landmarks"""
    from eqf_vio_amd import synth

    st = synth.make_stream(22, duration=0.6)
    settings = synth.template_settings_dict()
    master = hip.FilterBatch(settings, capacity=CAP, batch=4)
    f = 0
    for kind, k in st.events():
        if f >= 5:
            break
        if kind == "imu":
            r = st.imu[k]
            master.process_imu(r[0], r[1:4], r[4:7])
        else:
            master.process_vision(st.vision_stamps[k], st.ids, st.bearings[k], nb=COUNTS)
            f += 1
    assert [master.num_landmarks(b) for b in range(4)] == COUNTS
    return settings, st, master


def _handle(hip, world, restore=True):
    settings, _, master = world
    fg = hip.FilterBatch(settings, capacity=CAP, batch=4)
    if restore:
        fg.copy_filters(master, ALL, ALL)
    return fg


def _bits(x):
    if isinstance(x, dict):
        return {k: _bits(v) for k, v in x.items()}
    if hasattr(x, "keys"):
        return {k: _bits(x[k]) for k in x.keys()}
    if isinstance(x, (list, tuple)):
        return {k: _bits(v) for k, v in enumerate(x)}
    if x is None:
        return b"None"
    assert np.asarray(x).dtype != object, type(x)
    return np.ascontiguousarray(x).tobytes() + str(np.asarray(x).shape).encode()


def _state(fg):
    """ids, origin, group, bias, Sigma, time, integrator (dump_state) and the estimate, the covariance in the estimate's coordinates and
    its marginals, of every filter"""
    out = {}
    for b in range(fg.B):
        g = dict(fg.dump_state(b))
        g["est"] = fg.state_estimate(b)
        g["sigma_local"] = fg.sigma_local(b)
        g["marginals"] = fg.marginals(b)
        out[b] = g
    return out


def _same(a, b, what):
    a, b = _bits(a), _bits(b)

    def walk(x, y, path):
        if isinstance(x, dict):
            assert x.keys() == y.keys(), path
            for k in x:
                walk(x[k], y[k], f"{path}/{k}")
        else:
            assert x == y, f"{what}: {path} differs"

    walk(a, b, "")


def _three_calls(hip, world, small, large, mutating):
    """small, large, small on one handle against the large call alone on a fresh one; the second small call against the first"""
    _, _, master = world
    work, fresh = _handle(hip, world), _handle(hip, world)
    res = []
    for call in (small, large, small):
        if mutating:
            work.copy_filters(master, ALL, ALL)
        res.append((call(work), _state(work) if mutating else None))
    ref = (large(fresh), _state(fresh) if mutating else None)
    _same(res[1], ref, "the large call behind a small one")
    _same(res[2], res[0], "the small call behind a large one")
    if not mutating:
        _same(_state(work), _state(fresh), "the state behind calls that only read")
    return work, fresh


def _blocks(st, stride, rows, seed):
    """per filter: up to `stride` of its landmarks (every second one), blocks H (K, rows, 3), residuals and R"""
    rng = np.random.default_rng([2301, stride, rows, seed])
    ids, H, r, R = [], [], [], []
    for n in COUNTS:
        pick = np.asarray(st.ids[:n][::2][:stride], dtype=np.int32)
        k = len(pick)
        ids.append(pick)
        H.append(rng.standard_normal((k, rows, 3)))
        r.append(0.01 * rng.standard_normal((k, rows)))
        A = rng.standard_normal((k, rows, rows))
        R.append(0.05 * (A @ np.transpose(A, (0, 2, 1)) / rows + np.eye(rows)))
    return ids, H, r, R


def test_update_landmarks_grows_small_image_and_both_workspaces(hip, world):
    st = world[1]
    s, l = _blocks(st, 2, 1, 0), _blocks(st, 8, 3, 1)
    _three_calls(hip, world, lambda fg: fg.update_landmarks(*s, rows=1, stride=2), lambda fg: fg.update_landmarks(*l, rows=3, stride=8), True)


def test_update_landmarks_in_flight(hip, world):
    """without used / gamma / report the call does not wait: the large call replaces buffers the small one may still be using"""
    st = world[1]
    s, l = _blocks(st, 2, 1, 0), _blocks(st, 8, 3, 1)
    work, fresh = _handle(hip, world), _handle(hip, world)
    work.update_landmarks(*s, rows=1, stride=2, wait=False)
    work.update_landmarks(*l, rows=3, stride=8, wait=False)
    fresh.update_landmarks(*s, rows=1, stride=2, wait=False)
    fresh.synchronize()
    fresh.update_landmarks(*l, rows=3, stride=8, wait=False)
    _same(_state(work), _state(fresh), "two calls that do not wait")
    _same([work.last_update(b) for b in ALL], [fresh.last_update(b) for b in ALL], "two calls that do not wait")


def test_sample_sigma_grows_sample_rows(hip, world):
    n = 11 + 3 * max(COUNTS)
    rng = np.random.default_rng(2302)
    z1, z5 = rng.standard_normal((4, 1, n)), rng.standard_normal((4, 5, n))
    _three_calls(hip, world, lambda fg: fg.sample_sigma(z1, scale=[1.0, 0.5, 2.0, 1.5]), lambda fg: fg.sample_sigma(z5, scale=[1.0, 0.5, 2.0, 1.5]), False)


def test_mixture_moments_grows_member_table(hip, world):
    small = lambda fg: fg.mixture_moments([1, 1], [0.25, 0.75], ref=1)
    large = lambda fg: fg.mixture_moments([1, 1, 1, 1, 1, 1], [0.1, 0.2, 0.05, 0.3, 0.15, 0.2], ref=1)  # (members of one id set: repeats)
    _three_calls(hip, world, small, large, False)


def test_merge_costs_grow_chunk_workspace_and_item_block(hip, world):
    def small(fg):
        fg.set_option("merge_cost_chunk", 1)
        return fg.merge_costs([1, 1], [0.4, 0.6], ref=1, pairs=[(0, 1)])

    def large(fg):
        fg.set_option("merge_cost_chunk", 3)
        return fg.merge_costs([1, 1, 1, 1], [0.1, 0.2, 0.3, 0.4], ref=1)

    _three_calls(hip, world, small, large, False)


def _candidates(st, ncand):
    """candidate c of filter b: its first COUNTS[b] - c landmarks with the bearings of frame 5 + c"""
    ids = [[np.asarray(st.ids[:max(n - c, 0)], dtype=np.int32) for c in range(ncand)] for n in COUNTS]
    ys = [[np.asarray(st.bearings[5 + c])[:max(n - c, 0)] for c in range(ncand)] for n in COUNTS]
    return ids, ys


def test_score_vision_grows_chunk_workspace_and_table(hip, world):
    st = world[1]

    def small(fg):
        fg.set_option("score_chunk", 1)
        return fg.score_vision(*_candidates(st, 1), want_lm=True)

    def large(fg):
        fg.set_option("score_chunk", 4)
        return fg.score_vision(*_candidates(st, 4), want_lm=True)

    _three_calls(hip, world, small, large, False)


def test_copy_filters_grows_pair_table_then_small_image(hip, world):
    _, _, master = world
    work = _handle(hip, world, restore=False)
    for b in ALL:
        work.copy_filters(master, [b], [b])                   # (the master state, one pair at a time: the table stays at one pair)
    work.copy_filters(master, [0], [1])                       # one pair
    one = _state(work)
    work.copy_filters(master, ALL, [3, 2, 1, 0])              # four pairs: the pair table grows
    fresh = _handle(hip, world, restore=False)
    fresh.copy_filters(master, ALL, [3, 2, 1, 0])
    _same(_state(work), _state(fresh), "four pairs behind one")
    work.copy_filters(work, [0, 1], [1, 0])                   # in place, each a source and a destination: the small image is needed
    fresh.copy_filters(fresh, [0, 1], [1, 0])
    _same(_state(work), _state(fresh), "an in-place pair")
    assert [work.num_landmarks(b) for b in ALL] == [COUNTS[2], COUNTS[3], COUNTS[1], COUNTS[0]]
    work.copy_filters(master, [0], [1])                       # the small call again
    fresh.copy_filters(master, [0], [1])
    _same(_state(work), _state(fresh), "one pair behind four")
    _same(_state(work)[0], one[0], "one pair behind four: filter 0")
