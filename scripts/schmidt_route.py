"""Measurements behind DESIGN.md section 4.5n (Schmidt updates, eqf_update_linear_schmidt / eqf_update_landmarks_schmidt).  Needs the GPU.

  time [reps]    For the shapes 1 x 200 (150 considered, 40 stereo entries), 64 x 200 (the same) and 1 x 1000 (950 considered, 200 entries)
                 -- filters x landmarks, three frames of a synthetic stream -- and the two calls
                     landmarks  FilterBatch.update_landmarks with 2-row entries on every fifth landmark (considered and active ones)
                     linear     FilterBatch.update_linear with a 3-row zero-velocity update
                 three routes, each followed by a synchronise:
                     schmidt    the call with consider=...
                     full       the same call without it (every landmark moves: what the Schmidt call is asked to beat)
                     host       per filter eqf_get_sigma, consistency.schmidt_update_host, eqf_set_state
                 Every timed call starts from the same state (eqf_copy_filters from a master handle, then a synchronise) and is taken with
                 the host clock; all are warmed up once and alternated over `reps` repetitions (default 9; the two device routes take turns
                 going first, behind one untimed call: the host route's numpy leaves cold caches to whoever follows it).  One JSON line per shape and
                 call: medians with min / max, the measured ratio of the calls beside the counted one 1 - (|c| / n)^2 of the downdate, and
                 the counted bytes 16 (n^2 - |c|^2) B (divide by the kernel's time from the trace below).
  kernels B N C K   Both calls, Schmidt and full, five times each on B filters of N landmarks with C considered and K entries, nothing
                 timed: the body of a kernel-trace run (rocprofv3 --kernel-trace --stats -- python scripts/schmidt_route.py kernels ...),
                 which gives k_schmidt_downdate against k_blk_downdate / k_lin_downdate from the same build."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(1, 200, 150, 40), (64, 200, 150, 40), (1, 1000, 950, 200)]


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


def _operands(master, B, N, C, K):
    """per filter: the consider ids (the C oldest landmarks), K stereo-like entries spread over all landmarks, a zero-velocity update"""
    import numpy as np

    rng = np.random.default_rng(27)
    ids = np.sort(master.ids(0))
    consider = np.ascontiguousarray(np.broadcast_to(ids[:C].astype(np.int32), (B, C)))
    pick = ids[np.linspace(0, N - 1, K).astype(int)]
    lm = dict(ids=[pick.astype(np.int32)] * B, H=[rng.standard_normal((K, 2, 3))] * B, resid=[1e-3 * rng.standard_normal((K, 2))] * B,
              R=[1e-4 * np.eye(2)] * B)
    H = np.zeros((3, 11 + 3 * N))
    H[0, 8] = H[1, 9] = H[2, 10] = 1.0
    lin = dict(H=[H] * B, resid=[1e-3 * rng.standard_normal(3)] * B, R=1e-4 * np.eye(3))
    return consider, lm, lin


def _run(fg, call, ops, consider, wait=False):
    if call == "landmarks":
        return fg.update_landmarks(ops["ids"], ops["H"], ops["resid"], ops["R"], rows=2, local=False, wait=wait, consider=consider)
    return fg.update_linear(ops["H"], ops["resid"], ops["R"], local=False, stats=wait, consider=consider)


def _host_route(fg, call, ops, consider):
    import numpy as np

    from eqf_vio_amd import consistency as cs

    for b in range(fg.B):
        snap = fg.dump_state(b)  # eqf_get_sigma and the state getters
        N = len(snap["ids"])
        pos = {int(v): i for i, v in enumerate(snap["ids"])}
        if call == "landmarks":
            idx = [pos[int(i)] for i in ops["ids"][b]]
            Ht = cs.landmark_blocks_matrix(N, idx, ops["H"][b])
            R = np.kron(np.eye(len(idx)), ops["R"][b])
            r = ops["resid"][b].reshape(-1)
        else:
            Ht, R, r = ops["H"][b], ops["R"], ops["resid"][b]
        out = cs.schmidt_update_host(snap["sigma"], Ht, R, r, cs.consider_indices([pos[int(i)] for i in consider[b]]))
        snap["sigma"] = out["Sigma"]
        fg.restore_state(snap, b)  # eqf_set_state
    fg.synchronize()


def timing(reps=9):
    import numpy as np

    from eqf_vio_amd import binding

    q = lambda v: dict(median=round(float(np.median(v)), 4), min=round(float(min(v)), 4), max=round(float(max(v)), 4))  # noqa: E731
    for B, N, C, K in SHAPES:
        d, cap, master = _setup(B, N)
        idx = np.arange(B, dtype=np.int32)
        dev, host = (binding.FilterBatch(d, capacity=cap, batch=B) for _ in range(2))
        n, nc = 12 + 3 * N, 3 * C
        consider, lm, lin = _operands(master, B, N, C, K)

        def fresh(fg):
            fg.copy_filters(master, idx, idx)
            fg.synchronize()

        for call, ops in (("landmarks", lm), ("linear", lin)):
            t = dict(schmidt_ms=[], full_ms=[], host_ms=[])
            for rep in range(reps + 1):  # (the first round warms everything up: allocations, code objects)
                row = [0.0, 0.0]
                # (the host route leaves the caches to numpy: one untimed call first, and the two device routes take turns going first)
                fresh(dev)
                rp = _run(dev, call, ops, None, wait=True)
                assert not rp["info"].any(), rp["info"]
                for which in ((0, 1) if rep % 2 else (1, 0)):
                    cons = (consider, None)[which]
                    fresh(dev)
                    t0 = time.perf_counter()
                    _run(dev, call, ops, cons)
                    dev.synchronize()
                    row[which] = (time.perf_counter() - t0) * 1e3
                    if rep == 0:
                        rp = _run(dev, call, ops, cons, wait=True)
                        assert not rp["info"].any(), rp["info"]
                fresh(host)
                t0 = time.perf_counter()
                _host_route(host, call, ops, consider)
                row.append((time.perf_counter() - t0) * 1e3)
                if rep:
                    for k, v in zip(t, row):
                        t[k].append(v)
            med = {k: float(np.median(v)) for k, v in t.items()}
            counted = 1.0 - (nc / n) ** 2
            rec = dict(case="schmidt_route", call=call, B=B, N=N, considered=C, entries=K if call == "landmarks" else 3, n=n, reps=reps,
                       **{k: q(v) for k, v in t.items()}, counted_ratio=round(counted, 3),
                       schmidt_over_full=round(med["schmidt_ms"] / med["full_ms"], 3), schmidt_ahead_of_full=bool(med["schmidt_ms"] < med["full_ms"]),
                       host_over_schmidt=round(med["host_ms"] / med["schmidt_ms"], 1), counted_bytes=int(16.0 * (n * n - nc * nc) * B),
                       full_counted_bytes=int(16.0 * n * n * B))
            print(json.dumps(rec), flush=True)
        assert dev.device_error() == 0 and host.device_error() == 0
        del dev, host, master


def kernels(B, N, C, K):
    import numpy as np

    from eqf_vio_amd import binding

    d, cap, master = _setup(B, N)
    idx = np.arange(B, dtype=np.int32)
    fg = binding.FilterBatch(d, capacity=cap, batch=B)
    consider, lm, lin = _operands(master, B, N, C, K)
    for call, ops in (("landmarks", lm), ("linear", lin)):
        for cons in (consider, None):
            for _ in range(5):
                fg.copy_filters(master, idx, idx)
                fg.synchronize()
                _run(fg, call, ops, cons)
                fg.synchronize()
    assert fg.device_error() == 0


if __name__ == "__main__":
    if len(sys.argv) > 5 and sys.argv[1] == "kernels":
        kernels(*(int(v) for v in sys.argv[2:6]))
    elif len(sys.argv) > 1 and sys.argv[1] == "time":
        timing(int(sys.argv[2]) if len(sys.argv) > 2 else 9)
    else:
        raise SystemExit(__doc__)
