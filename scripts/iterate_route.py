"""Measurements behind DESIGN.md section 4.5q (the iterated landmark observation update, eqf_observe_landmarks_iterated).  Needs the GPU.

  time [reps]    For the shapes 1 x 200 (40 range entries), 64 x 200 (the same) and 1 x 1000 (200 entries) -- filters x landmarks, three
                 frames of a synthetic stream -- ranges of every fifth landmark 30 % beyond the prediction, each route followed by a
                 synchronise:
                     one_shot          FilterBatch.observe_landmarks(OBS_RANGE, ..., wait=False)
                     iterated_1/2/4    the same with max_lin = 1, 2, 4 and tol = 0 (every linearisation is taken)
                     host_2/4          the route the call replaces: per filter sigma() and dump_state(), consistency.observe_iterated_host
                                       with max_lin = 2, 4, then set_sigma and apply_increment
                 Every timed call starts from the same state (eqf_copy_filters from a master handle, then a synchronise) and is taken with
                 the host clock; all are warmed up once and alternated over `reps` repetitions (default 9), in rotating order.  One JSON
                 line per shape: medians with min / max.  A library that predates the call (loaded through EQF_VIO_AMD_LIB: the parent
                 commit's host route is the yardstick) is timed on one_shot and the host routes alone; at 64 x 200 the host route is timed
                 with reps // 3 repetitions (it takes seconds).
  kernels B N K MAXLIN   The call five times on B filters of N landmarks with K entries, nothing timed: the body of a kernel-trace run
                 (rocprofv3 --kernel-trace --stats -- python scripts/iterate_route.py kernels ...), which gives the kernels of one
                 intermediate linearisation (k_iter_form, the factorisation's, k_iter_step, k_iter_rows) against those of the one-shot call
                 (MAXLIN = 1), and k_iter_form's time for its counted bytes: per pair of entries nine values of Sigma read, 3 x rows of T
                 and, for q <= p, rows x rows of S written -- formBytes()."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from observe_route import SHAPES, _setup  # noqa: E402

VAR_REL = 0.02


def form_bytes(K, rows=1):
    """counted bytes of one k_iter_form launch per filter: K^2 pairs x (9 reads + 3 rows writes of T) + K (K + 1) / 2 x rows^2 of S"""
    return 8 * (K * K * (9 + 3 * rows) + K * (K + 1) // 2 * rows * rows)


def _ranges(master, B, N, K):
    import numpy as np

    ids, rho, R = [], [], []
    for b in range(B):
        sid = master.ids(b)
        order = np.argsort(sid)
        pick = order[np.linspace(0, N - 1, K).astype(int)]
        d = np.linalg.norm(master.state_estimate(b)["p"][pick], axis=1)
        ids.append(sid[pick].astype(np.int32))
        rho.append(1.3 * d)
        R.append(((VAR_REL * d) ** 2).reshape(K, 1, 1))
    return ids, rho, R


def _device(max_lin):
    def run(fg, ids, rho, R):
        from eqf_vio_amd import binding

        if max_lin is None:
            fg.observe_landmarks(binding.OBS_RANGE, ids, rho, R, wait=False)
        elif max_lin == 1:
            # (the binding takes the NEW entry point at one linearisation only when a trace is asked for: this route waits for its outputs)
            fg.observe_landmarks(binding.OBS_RANGE, ids, rho, R, max_lin=1, want_trace=True)
        else:
            fg.observe_landmarks(binding.OBS_RANGE, ids, rho, R, wait=False, max_lin=max_lin, tol=0.0)
        fg.synchronize()

    return run


def _host(max_lin):
    def run(fg, ids, rho, R):
        import numpy as np

        from eqf_vio_amd import binding
        from eqf_vio_amd import consistency as cs

        n = 11 + 3 * max(fg.num_landmarks(b) for b in range(fg.B))
        G = np.zeros((fg.B, n))
        for b in range(fg.B):
            st = fg.dump_state(b)
            r = cs.observe_iterated_host(binding.OBS_RANGE, fg.sigma(b), st, ids[b], np.asarray(rho[b]).reshape(-1, 1) * [1.0, 0, 0], R[b],
                                         max_lin=max_lin, tol=0.0)
            fg.set_sigma(r["Sigma"], b)
            G[b, :len(r["gamma"])] = r["gamma"]
        fg.apply_increment(G)
        fg.synchronize()

    return run


def timing(reps=9):
    import numpy as np

    from eqf_vio_amd import binding

    have = hasattr(binding.lib(), "eqf_observe_landmarks_iterated")
    q = lambda v: dict(median=round(float(np.median(v)), 4), min=round(float(min(v)), 4), max=round(float(max(v)), 4))  # noqa: E731
    for B, N, K in SHAPES:
        d, cap, master = _setup(B, N)
        idx = np.arange(B, dtype=np.int32)
        fg = binding.FilterBatch(d, capacity=cap, batch=B)
        ids, rho, R = _ranges(master, B, N, K)
        routes = [("one_shot_ms", _device(None))]
        if have:
            routes += [(f"iterated_{m}_ms", _device(m)) for m in (1, 2, 4)]
        routes += [(f"host_{m}_ms", _host(m)) for m in (2, 4)]
        t = {name: [] for name, _ in routes}
        for rep in range(reps + 1):  # (the first round warms everything up: allocations, code objects)
            k = rep % len(routes)
            for name, fn in routes[k:] + routes[:k]:
                if name.startswith("host") and B > 1 and rep > max(reps // 3, 1):
                    continue
                fg.copy_filters(master, idx, idx)
                fg.synchronize()
                t0 = time.perf_counter()
                fn(fg, ids, rho, R)
                dt = 1e3 * (time.perf_counter() - t0)
                if rep:
                    t[name].append(dt)
        assert fg.device_error() == 0
        out = dict(B=B, N=N, entries=K, reps=reps, lib=os.environ.get("EQF_VIO_AMD_LIB", "this tree"), **{k: q(v) for k, v in t.items()})
        if have:  # (counted by the library as they are made)
            out["extra_launches"] = {}
            for m in (1, 2, 4):
                fg.copy_filters(master, idx, idx)
                _device(m)(fg, ids, rho, R)
                out["extra_launches"][m] = fg.debug_iterate_launches()
        print(json.dumps(out), flush=True)
        fg.close(), master.close()


def kernels(B, N, K, max_lin):
    import numpy as np

    from eqf_vio_amd import binding

    d, cap, master = _setup(B, N)
    idx = np.arange(B, dtype=np.int32)
    fg = binding.FilterBatch(d, capacity=cap, batch=B)
    ids, rho, R = _ranges(master, B, N, K)
    for _ in range(5):
        fg.copy_filters(master, idx, idx)
        _device(max_lin if max_lin > 1 else None)(fg, ids, rho, R)
    assert fg.device_error() == 0
    print(json.dumps(dict(B=B, N=N, entries=K, max_lin=max_lin, calls=5, form_bytes_per_filter=form_bytes(K))))


if __name__ == "__main__":
    if len(sys.argv) >= 6 and sys.argv[1] == "kernels":
        kernels(*(int(v) for v in sys.argv[2:6]))
    elif len(sys.argv) >= 2 and sys.argv[1] == "time":
        timing(*(int(v) for v in sys.argv[2:3]))
    else:
        sys.exit(__doc__)
