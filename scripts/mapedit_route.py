"""Measurements behind DESIGN.md section 4.5m (explicit landmark removal and insertion, eqf_edit_landmarks).  Needs the GPU.

  time [reps]    For the shapes 1 x 200, 64 x 200 and 1 x 1000 (filters x landmarks, three frames of a synthetic stream) and the two edits
                     swap    remove 10 % of every filter's landmarks and insert as many (the removing launch: Sigma changes buffers)
                     add10   insert 10 landmarks and remove none (the in-place launch)
                 the call against the host route it replaces:
                     device  FilterBatch.edit_landmarks, then a synchronise (`enqueue`: the call alone, it does not wait for the device)
                     host    per filter dump_state, consistency.edit_landmarks_host, restore_state; then a synchronise
                 Every timed call starts from the same state (eqf_copy_filters from a master handle, then a synchronise: the stream is idle)
                 and is taken with the host clock around it; both are warmed up once and alternated over `reps` repetitions (default 9).
                 The launch itself is timed by the handle's own event brackets on its stream (eqf_profile_enable, class "churn") in runs
                 of their own, profiling off for the end-to-end numbers.  For the removing launch the counted bytes are 2 * 8 * n^2 * B
                 (n = 12 + 3 N: every entry of the output read once and written once) over that time, set against a device-to-device copy
                 of 8 * n^2 * B bytes -- the same bytes read and written -- between two buffers of this process, timed with events on its
                 stream in the same run, alternating with the launch.  One JSON line per shape and edit: medians with min / max.
  kernels B N    Both edits five times each on B filters of N landmarks, nothing timed: the body of a kernel-trace run
                 (rocprofv3 --kernel-trace --stats -- python scripts/mapedit_route.py kernels B N), which gives the time of
                 k_mapedit_move / k_mapedit_append without the event brackets' share of the upload in front of them."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(1, 200), (64, 200), (1, 1000)]


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


def _edits(master, B, N):
    import numpy as np

    rng = np.random.default_rng(3)

    def prior(k):
        p = np.column_stack([rng.uniform(-1.5, 1.5, k), rng.uniform(-1.0, 1.0, k), rng.uniform(2.0, 9.0, k)])
        a = rng.standard_normal((k, 3, 3)) * 0.2
        return p, a @ np.transpose(a, (0, 2, 1)) + 0.01 * np.eye(3)

    ids = [master.ids(b) for b in range(B)]
    top = int(max(i.max() for i in ids)) + 1
    k = N // 10
    swap = dict(remove=[np.sort(i[::10][:k]) for i in ids], insert=[(np.arange(top, top + k, dtype=np.int32),) + prior(k) for _ in range(B)])
    add10 = dict(remove=None, insert=[(np.arange(top, top + 10, dtype=np.int32),) + prior(10) for _ in range(B)])
    return dict(swap=swap, add10=add10)


def _host_route(fg, edit):
    import numpy as np

    from eqf_vio_amd import consistency as cs

    none = np.zeros(0, dtype=np.int32)
    for b in range(fg.B):
        snap = fg.dump_state(b)  # eqf_get_sigma and the state getters
        i, p, P = edit["insert"][b]
        new, _, _ = cs.edit_landmarks_host(snap, none if edit["remove"] is None else edit["remove"][b], i, p, P)
        fg.restore_state(new, b)  # eqf_set_state
    fg.synchronize()


def _copy_roof(nbytes):
    """[ms] of device-to-device copies of nbytes, events on torch's current stream."""
    import torch

    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    src.zero_()

    def once():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src, non_blocking=True)
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    once()
    return once


def timing(reps=9):
    import numpy as np

    from eqf_vio_amd import binding

    q = lambda v: dict(median=round(float(np.median(v)), 4), min=round(float(min(v)), 4), max=round(float(max(v)), 4))  # noqa: E731
    for B, N in SHAPES:
        d, cap, master = _setup(B, N)
        idx = np.arange(B, dtype=np.int32)
        dev, host, prof = (binding.FilterBatch(d, capacity=cap, batch=B) for _ in range(3))
        prof.profile_enable(True)
        n = 12 + 3 * N
        copy_once = _copy_roof(8 * n * n * B)

        def fresh(fg):
            fg.copy_filters(master, idx, idx)
            fg.synchronize()

        for name, edit in _edits(master, B, N).items():
            t = dict(device_ms=[], enqueue_ms=[], host_ms=[], launch_ms=[], copy_ms=[])
            for rep in range(reps + 1):  # (the first round warms everything up: allocations, code objects)
                fresh(dev)
                t0 = time.perf_counter()
                dev.edit_landmarks(**edit)
                t1 = time.perf_counter()
                dev.synchronize()
                t2 = time.perf_counter()
                fresh(host)
                t3 = time.perf_counter()
                _host_route(host, edit)
                t4 = time.perf_counter()
                if rep == 0:  # the two routes agree, bit for bit
                    for b in range(B):
                        assert dev.ids(b).tobytes() == host.ids(b).tobytes() and dev.sigma(b).tobytes() == host.sigma(b).tobytes()
                fresh(prof)
                before = {k: v for k, v in prof.profile().items() if "churn" in k.lower()}
                prof.edit_landmarks(**edit)
                prof.synchronize()
                after = {k: v for k, v in prof.profile().items() if "churn" in k.lower()}
                (key,) = after.keys()
                assert after[key][0] - before[key][0] == 1, "one launch per call"
                launch = after[key][1] - before[key][1]
                cp = copy_once()
                if rep:
                    for k, v in zip(t, ((t2 - t0) * 1e3, (t1 - t0) * 1e3, (t4 - t3) * 1e3, launch, cp)):
                        t[k].append(v)
            med = {k: float(np.median(v)) for k, v in t.items()}
            rec = dict(case="mapedit_route", edit=name, B=B, N=N, n=n, reps=reps, **{k: q(v) for k, v in t.items()},
                       host_over_device=round(med["host_ms"] / med["device_ms"], 1), device_ahead_of_host=bool(med["device_ms"] < med["host_ms"]))
            if name == "swap":
                counted = 2.0 * 8 * n * n * B
                rec.update(counted_bytes=int(counted), launch_GBps=round(counted / med["launch_ms"] / 1e6, 1),
                           copy_GBps=round(counted / med["copy_ms"] / 1e6, 1), launch_over_copy=round(med["copy_ms"] / med["launch_ms"], 3))
            else:
                rec.pop("copy_ms")
            print(json.dumps(rec), flush=True)
        assert dev.device_error() == 0 and prof.device_error() == 0
        del dev, host, prof, master


def kernels(B, N):
    import numpy as np

    from eqf_vio_amd import binding

    d, cap, master = _setup(B, N)
    idx = np.arange(B, dtype=np.int32)
    fg = binding.FilterBatch(d, capacity=cap, batch=B)
    for edit in _edits(master, B, N).values():
        for _ in range(5):
            fg.copy_filters(master, idx, idx)
            fg.synchronize()
            fg.edit_landmarks(**edit)
            fg.synchronize()
    assert fg.device_error() == 0


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "kernels":
        kernels(int(sys.argv[2]), int(sys.argv[3]))
    elif len(sys.argv) > 1 and sys.argv[1] == "time":
        timing(int(sys.argv[2]) if len(sys.argv) > 2 else 9)
    else:
        raise SystemExit(__doc__)
