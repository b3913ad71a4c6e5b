"""Measurements behind DESIGN.md section 4.5p (the deterministic split, eqf_split_filters).  Needs the GPU.

  time [reps]    For the shapes 1 x 200, 64 x 200 and 1 x 1000 (source filters x landmarks, three frames of a synthetic stream) every source
                 is split into K = 3 along the depth axis of one landmark (a local row), one child in place and two in other slots (a
                 handle of 3 filters for one source; at 64 x 200 the first 21 filters are the sources and 42 others take the children),
                 two routes, each followed by a synchronise:
                     split   FilterBatch.split_filters(..., local=True, report=False)
                     host    what a caller had before: u from the source's sigma() and local_jacobian(), copy_filters, then per child
                             sigma(), the rank-one edit in numpy and set_sigma(), then one apply_increment
                 Every timed call starts from the same state (eqf_copy_filters from a master handle, then a synchronise) and is taken with
                 the host clock; both are warmed up once and alternated over `reps` repetitions (default 9), taking turns going first.  One
                 JSON line per shape: medians with min / max, the ratio host / split and the split's rate against its counted bytes
                 (1 + K) n^2 8 per source.  A library that predates the call (loaded through EQF_VIO_AMD_LIB: the parent commit's host
                 route is the yardstick) is timed on the host route alone.
  kernels S N    S sources of N landmarks, five times, nothing timed: the split into three children in OTHER slots, then copy_filters onto
                 the same destinations -- the body of a kernel-trace run (rocprofv3 --kernel-trace --stats -- python scripts/split_route.py
                 kernels ...), which gives k_split_sigma against k_clone_sigma on the same destination bytes and the launches of a call."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(1, 200), (64, 200), (1, 1000)]
K = 3


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


def _plan(S, in_place):
    """(batch, dst, src): S sources in front, K children each -- the first in place, or all K in other slots"""
    import numpy as np

    extra = K - 1 if in_place else K
    dst, src = [], []
    for s in range(S):
        kids = ([s] if in_place else []) + [S + extra * s + j for j in range(extra)]
        dst += kids
        src += [s] * K
    return S + extra * S, np.array(dst, dtype=np.int32), np.array(src, dtype=np.int32)


def _rows(master, B, N):
    import numpy as np

    from eqf_vio_amd import consistency as cs

    A = np.zeros((B, 11 + 3 * N))
    for b in range(B):
        n = master.num_landmarks(b)
        if n:
            A[b, :11 + 3 * n] = cs.depth_axis_row(master.state_estimate(b)["p"][n // 2], n // 2, 11 + 3 * n)
    return A


def _split(fg, A, dst, src, shift, shrink):
    fg.split_filters(A, dst, src, shift, shrink, local=True, report=False)
    fg.synchronize()


def _host(fg, A, dst, src, shift, shrink):
    import numpy as np

    u = {}
    for s in sorted(set(int(v) for v in src)):
        n = 11 + 3 * fg.num_landmarks(s)
        J = fg.local_jacobian(s)
        h = A[s, :n].copy()
        h[6:8] = A[s, 6:8] @ J["G"]
        h[8:11] = A[s, 8:11] @ J["RAt"]
        h[11:] = np.einsum("ik,ikl->il", A[s, 11:n].reshape(-1, 3), J["lm"]).ravel()
        Bv = fg.sigma(s) @ h
        u[s] = Bv / np.sqrt(h @ Bv)
    move = dst != src
    fg.copy_filters(fg, dst[move], src[move])
    G = np.zeros((fg.B, A.shape[1]))
    mask = np.zeros(fg.B, dtype=np.uint8)
    for d, s, sh, sk in sorted(zip(dst, src, shift, shrink), key=lambda c: c[0] == c[1]):  # (the child in place last: it edits the source)
        fg.set_sigma(fg.sigma(int(d)) - sk * np.outer(u[int(s)], u[int(s)]), int(d))
        G[d, :len(u[int(s)])] = sh * u[int(s)]
        mask[d] = sh != 0.0
    fg.apply_increment(G if fg.B > 1 else [G[0]], mask)
    fg.synchronize()


def timing(reps=9):
    import numpy as np

    from eqf_vio_amd import binding, consistency as cs

    have = hasattr(binding.lib(), "eqf_split_filters")
    q = lambda v: dict(median=round(float(np.median(v)), 4), min=round(float(min(v)), 4), max=round(float(max(v)), 4))  # noqa: E731
    _, sh3, sk3 = cs.split_components(K, 1.0)
    for B, N in SHAPES:
        S = 1 if B == 1 else B // K
        batch, dst, src = _plan(S, True)
        batch = max(batch, B)
        d, cap, master = _setup(batch, N)
        idx = np.arange(batch, dtype=np.int32)
        fg = binding.FilterBatch(d, capacity=cap, batch=batch)
        A = _rows(master, batch, N)
        shift, shrink = np.tile(sh3, S), np.tile(sk3, S)
        routes = [("split_ms", _split), ("host_ms", _host)] if have else [("host_ms", _host)]
        t = {name: [] for name, _ in routes}
        for rep in range(reps + 1):  # (the first round warms everything up: allocations, code objects)
            for name, fn in (routes if rep % 2 else routes[::-1]):
                fg.copy_filters(master, idx, idx)
                fg.synchronize()
                t0 = time.perf_counter()
                fn(fg, A, dst, src, shift, shrink)
                dt = 1e3 * (time.perf_counter() - t0)
                if rep:
                    t[name].append(dt)
        assert fg.device_error() == 0
        out = dict(filters=batch, sources=S, N=N, K=K, reps=reps, lib=os.environ.get("EQF_VIO_AMD_LIB", "this tree"), **{k: q(v) for k, v in t.items()})
        if have:
            nbytes = S * (1 + K) * (12 + 3 * N) ** 2 * 8
            out["host_over_split"] = round(float(np.median(t["host_ms"]) / np.median(t["split_ms"])), 2)
            out["counted_MB"] = round(nbytes / 1e6, 2)
            out["counted_GBps_of_call"] = round(nbytes / 1e9 / (float(np.median(t["split_ms"])) * 1e-3), 1)
        print(json.dumps(out), flush=True)
        fg.close(), master.close()


def kernels(S, N):
    import numpy as np

    from eqf_vio_amd import binding, consistency as cs

    batch, dst, src = _plan(S, False)
    d, cap, master = _setup(batch, N)
    idx = np.arange(batch, dtype=np.int32)
    fg = binding.FilterBatch(d, capacity=cap, batch=batch)
    A = _rows(master, batch, N)
    _, sh3, sk3 = cs.split_components(K, 1.0)
    for _ in range(5):
        fg.copy_filters(master, idx, idx)
        fg.synchronize()
        _split(fg, A, dst, src, np.tile(sh3, S), np.tile(sk3, S))
        fg.copy_filters(fg, dst, src)
        fg.synchronize()
    assert fg.device_error() == 0
    print(json.dumps(dict(sources=S, filters=batch, N=N, K=K, calls=5, dst_bytes_per_call=S * K * (12 + 3 * N) ** 2 * 8)))


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "kernels":
        kernels(int(sys.argv[2]), int(sys.argv[3]))
    elif len(sys.argv) >= 2 and sys.argv[1] == "time":
        timing(*(int(v) for v in sys.argv[2:3]))
    else:
        sys.exit(__doc__)
