"""Measurements behind DESIGN.md section 4.5o (rows formed on the device, eqf_observe_landmarks).  Needs the GPU.

  time [reps]    For the shapes 1 x 200 (40 bearing entries), 64 x 200 (the same) and 1 x 1000 (200 entries) -- filters x landmarks, three
                 frames of a synthetic stream -- a second camera's bearings of every fifth landmark, two routes, each followed by a
                 synchronise:
                     observe   FilterBatch.observe_landmarks(OBS_BEARING, ..., wait=False)
                     host      INTEGRATION.md's recipe: per filter state_estimate and dump_state, consistency.stereo_rows per entry, then
                               one update_landmarks(local=True, wait=False)
                 Every timed call starts from the same state (eqf_copy_filters from a master handle, then a synchronise) and is taken with
                 the host clock; both are warmed up once and alternated over `reps` repetitions (default 9), taking turns going first.  One
                 JSON line per shape: medians with min / max and the ratio host / observe.  A library that predates the call (loaded
                 through EQF_VIO_AMD_LIB: the parent commit's host route is the yardstick) is timed on the host route alone.
  kernels B N K [route]   The route (observe | host, default observe) five times on B filters of N landmarks with K entries, nothing
                 timed: the body of a kernel-trace run (rocprofv3 --kernel-trace --stats -- python scripts/observe_route.py kernels ...),
                 which gives k_obs_rows against k_blk_rows + k_local_jacobian and the number of launches of a call."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(1, 200, 40), (64, 200, 40), (1, 1000, 200)]
Q_21 = (0.9887710779360422, 0.0, 0.14943813247359922, 0.0)  # 0.3 rad about y
T_21 = (0.1, 0.0, 0.0)
VAR = 1e-4


def _setup(B, N):
    from eqf_vio_amd import binding, synth

    st = synth.make_stream(N, duration=0.05 * 3 + 0.02)
    d = synth.template_settings_dict()
    cap = N + 10
    master = binding.FilterBatch(d, capacity=cap, batch=B)
    for kind, k in st.events():
        if kind == "imu":
            master.process_imu(st.imu[k, 0], st.imu[k, 1:4], st.imu[k, 4:7])
        else:
            master.process_vision(st.vision_stamps[k], st.ids, st.bearings[k])
    master.synchronize()
    assert master.num_landmarks(0) == N and master.device_error() == 0
    return d, cap, master


def _bearings(master, B, N, K):
    """per filter: K ids spread over the landmarks and the second camera's unit bearings of the estimate, a little off"""
    import numpy as np

    from eqf_vio_amd import consistency as cs

    rng = np.random.default_rng(31)
    R21 = cs.quat_to_matrix(np.array(Q_21))
    ids, ys = [], []
    for b in range(B):
        sid = master.ids(b)
        order = np.argsort(sid)
        pick = order[np.linspace(0, N - 1, K).astype(int)]
        p = master.state_estimate(b)["p"][pick]
        y = (p - np.array(T_21)) @ R21 + 1e-3 * rng.standard_normal((K, 3))
        ids.append(sid[pick].astype(np.int32))
        ys.append(y / np.linalg.norm(y, axis=1, keepdims=True))
    return ids, ys


def _observe(fg, ids, ys):
    from eqf_vio_amd import binding

    fg.observe_landmarks(binding.OBS_BEARING, ids, ys, VAR, cam=(Q_21, T_21), wait=False)
    fg.synchronize()


def _host(fg, ids, ys):
    import numpy as np

    from eqf_vio_amd import consistency as cs

    H, r = [], []
    for b in range(fg.B):
        p_hat = dict(zip(fg.dump_state(b)["ids"], fg.state_estimate(b)["p"]))
        rows = [cs.stereo_rows(p_hat[i], Q_21, T_21, y) for i, y in zip(ids[b], ys[b])]
        H.append(np.array([h for h, _ in rows]))
        r.append(np.array([x for _, x in rows]))
    fg.update_landmarks(ids, H, r, [VAR * np.eye(2)] * fg.B, local=True, wait=False)
    fg.synchronize()


def timing(reps=9):
    import numpy as np

    from eqf_vio_amd import binding

    have = hasattr(binding.lib(), "eqf_observe_landmarks")
    q = lambda v: dict(median=round(float(np.median(v)), 4), min=round(float(min(v)), 4), max=round(float(max(v)), 4))  # noqa: E731
    for B, N, K in SHAPES:
        d, cap, master = _setup(B, N)
        idx = np.arange(B, dtype=np.int32)
        fg = binding.FilterBatch(d, capacity=cap, batch=B)
        ids, ys = _bearings(master, B, N, K)
        routes = [("observe_ms", _observe), ("host_ms", _host)] if have else [("host_ms", _host)]
        t = {name: [] for name, _ in routes}
        for rep in range(reps + 1):  # (the first round warms everything up: allocations, code objects)
            for name, fn in (routes if rep % 2 else routes[::-1]):
                fg.copy_filters(master, idx, idx)
                fg.synchronize()
                t0 = time.perf_counter()
                fn(fg, ids, ys)
                dt = 1e3 * (time.perf_counter() - t0)
                if rep:
                    t[name].append(dt)
        assert fg.device_error() == 0
        out = dict(B=B, N=N, entries=K, reps=reps, lib=os.environ.get("EQF_VIO_AMD_LIB", "this tree"), **{k: q(v) for k, v in t.items()})
        if have:
            out["host_over_observe"] = round(float(np.median(t["host_ms"]) / np.median(t["observe_ms"])), 2)
        print(json.dumps(out), flush=True)
        fg.close(), master.close()


def kernels(B, N, K, route="observe"):
    import numpy as np

    from eqf_vio_amd import binding

    d, cap, master = _setup(B, N)
    idx = np.arange(B, dtype=np.int32)
    fg = binding.FilterBatch(d, capacity=cap, batch=B)
    ids, ys = _bearings(master, B, N, K)
    for _ in range(5):
        fg.copy_filters(master, idx, idx)
        (_observe if route == "observe" else _host)(fg, ids, ys)
    assert fg.device_error() == 0
    print(json.dumps(dict(B=B, N=N, entries=K, route=route, calls=5)))


if __name__ == "__main__":
    if len(sys.argv) >= 5 and sys.argv[1] == "kernels":
        kernels(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), *sys.argv[5:6])
    elif len(sys.argv) >= 2 and sys.argv[1] == "time":
        timing(*(int(v) for v in sys.argv[2:3]))
    else:
        sys.exit(__doc__)
