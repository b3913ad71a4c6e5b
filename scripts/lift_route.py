"""Measurements behind DESIGN.md section 4.5l (the innovation lift of the non-vision updates, option "innovation_lift").  Needs the GPU.

  time B N [reps]    On B filters of N landmarks each (three frames of a synthetic stream), for eqf_update_landmarks with 40 stereo entries
                     (2 rows each) and for eqf_update_linear with a 3-row zero-velocity update:
                         off    the call with the option off (the plain lift)
                         on     the call with the option on (bundleLift from the pre-update Sigma_e on the device)
                         host   the route the option replaces, per filter: eqf_get_sigma, the state getters, consistency.bundle_lift_host,
                                eqf_set_state -- timed on its own, it would run beside the `off` call
                         nees   eqf_get_nees(local = 0, first = 6, no error vectors): one copy of Sigma, one factorisation of Sigma_e and a
                                tail, the yardstick for what `on` should cost more than `off`
                     Every timed call starts from the same state (eqf_copy_filters from a master handle, then a synchronise: the stream is
                     idle), ends in a synchronise and is taken with the host clock around it; all four are warmed up once and alternated over
                     `reps` repetitions (default 7).  Prints one JSON line per update with medians, min / max, on - off, (on - off) / nees
                     and the share of on - off in `on`, and how far the device's DeltaU is from the host statement's."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEREO = 40


def _setup(B, N):
    from eqf_vio_amd import binding, synth

    st = synth.make_stream(N, duration=0.05 * 3 + 0.02)
    d = synth.template_settings_dict()
    master = binding.FilterBatch(d, capacity=N, batch=B)
    for kind, k in st.events():
        if kind == "imu":
            master.process_imu(st.imu[k, 0], st.imu[k, 1:4], st.imu[k, 4:7])
        else:
            master.process_vision(st.vision_stamps[k], st.ids, st.bearings[k])
    master.synchronize()
    assert master.num_landmarks(0) == N and master.device_error() == 0
    work = {}
    for opt in (0, 1):
        work[opt] = binding.FilterBatch(d, capacity=N, batch=B)
        work[opt].set_option("innovation_lift", opt)
    return d, master, work, st.ids


def _operands(kind, B, N, ids):
    import numpy as np

    rng = np.random.default_rng(7)
    if kind == "landmarks":
        K = min(STEREO, N)
        return dict(ids=[ids[:K]] * B, H=[rng.standard_normal((K, 2, 3))] * B, resid=[1e-3 * rng.standard_normal((K, 2))] * B,
                    R=[1e-4 * np.eye(2)] * B)
    H = np.zeros((3, 11 + 3 * N))
    H[0, 8] = H[1, 9] = H[2, 10] = 1.0
    return dict(H=np.broadcast_to(H, (B, 3, 11 + 3 * N)).copy(), resid=np.broadcast_to([0.03, -0.02, 0.015], (B, 3)).copy(), R=1e-4 * np.eye(3))


def _call(fg, kind, ops):
    if kind == "landmarks":
        return fg.update_landmarks(ops["ids"], ops["H"], ops["resid"], ops["R"], rows=2, local=False)
    return fg.update_linear(ops["H"], ops["resid"], ops["R"], local=False, want_gamma=True)


def _host_route(fg, d, gammas):
    from eqf_vio_amd import consistency as cs

    out = []
    for b in range(fg.B):
        snap = fg.dump_state(b)   # eqf_get_sigma and the state getters
        n = 11 + 3 * len(snap["ids"])
        lift = cs.bundle_lift_host(gammas[b][:n], dict(origin=snap["origin"], group=snap["group"], bias=snap["bias"], discrete=True,
                                                       camera=dict(q=d["cameraOffset_q"], x=d["cameraOffset_x"])), snap["sigma"])
        snap["group"], snap["bias"] = lift["group"], lift["bias"]
        fg.restore_state(snap, b)  # eqf_set_state
        out.append(lift["DeltaU"])
    fg.synchronize()
    return out


def timing(B, N, reps=7):
    import numpy as np

    d, master, work, ids = _setup(B, N)
    idx = np.arange(B, dtype=np.int32)

    def fresh(fg):
        fg.copy_filters(master, idx, idx)
        fg.synchronize()

    def timed(fn):
        t0 = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t0) * 1e3, r

    for kind in ("landmarks", "linear"):
        ops = _operands(kind, B, N, ids)
        t = dict(off=[], on=[], host=[], nees=[])
        apart = 0.0
        for rep in range(reps + 1):  # (the first round warms everything up: allocations, code objects)
            fresh(work[0])
            a, out0 = timed(lambda: (_call(work[0], kind, ops), work[0].synchronize())[0])
            fresh(work[1])
            b_, out1 = timed(lambda: (_call(work[1], kind, ops), work[1].synchronize())[0])
            assert not out0["info"].any() and not out1["info"].any() and work[1].device_error() == 0
            dU = np.array([work[1].lift_report(b)["DeltaU"] for b in range(B)])
            fresh(work[0])
            c, dUh = timed(lambda: _host_route(work[0], d, out0["gamma"]))
            fresh(work[0])
            e, _ = timed(lambda: work[0].nees(None, local=False, first=6))
            apart = max(apart, float(np.max(np.abs(dU - np.array(dUh))) / np.max(np.abs(dU))))
            if rep:
                for k, v in zip(("off", "on", "host", "nees"), (a, b_, c, e)):
                    t[k].append(v)
        med = {k: float(np.median(v)) for k, v in t.items()}
        q = lambda v: dict(median_ms=round(float(np.median(v)), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3))  # noqa: E731
        print(json.dumps(dict(case="lift_route", update=kind, B=B, N=N, order_Sigma_e=6 + 3 * N, reps=reps, **{k: q(v) for k, v in t.items()},
                              on_minus_off_ms=round(med["on"] - med["off"], 3), on_minus_off_over_nees=round((med["on"] - med["off"]) / med["nees"], 2),
                              lift_share_of_on=round((med["on"] - med["off"]) / med["on"], 3),
                              device_ahead_of_host=bool(med["on"] - med["off"] < med["host"]),
                              host_over_device_lift=round(med["host"] / max(med["on"] - med["off"], 1e-9), 1), DeltaU_rel_apart=apart)), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "time":
        timing(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]) if len(sys.argv) > 4 else 7)
    else:
        raise SystemExit(__doc__)
