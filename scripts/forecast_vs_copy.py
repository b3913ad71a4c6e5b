"""Measurements behind DESIGN.md section 4.5i (the non-mutating forecast, eqf_forecast).  Every leg needs the GPU.

  time B N     FilterBatch.forecast at K = 10 samples and t1 (eleven steps, every output, ends in a synchronise) against the route it
               replaces on the same states after three frames: copy_filters into a second handle of full capacity, the same ten samples and
               one more stamped t1 through process_imu there (burst 15: one launch pair for the lot), then state_estimate(b) and
               marginals(b) for every filter.  The route is timed in its favour: it does not form bearings, S or ycov.  Both warmed up,
               alternated over 20 repetitions; prints one JSON line with medians, min / max, the ratio, and how far the two results are apart.
  kern B N     a workload for `rocprofv3 --kernel-trace --stats -- python scripts/forecast_vs_copy.py kern B N`: thirty of each.
  sum DIR      kernel-trace stats CSVs under DIR/fckern_B_N -> the two k_forecast_* kernels against the kernels of the route, launches per
               call, and k_forecast_lm's bytes -- per filter the base block, N panels and N diagonal blocks of Sigma (8 (121 + 42 N)), Q, p0
               and the landmark constants (8 x 23 N), the step records (8 x 144 per step) and the output record (8 (144 + 32 N)) -- over its
               average time, against the measured 6.29 TB/s."""
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K = 10


def _setup(B, N):
    import numpy as np
    from eqf_vio_amd import binding, synth

    st = synth.make_stream(N, duration=0.05 * 3 + 0.06)
    fg = binding.FilterBatch(synth.template_settings_dict(), capacity=N, batch=B)
    fg.stream_upload(st.imu, st.vision_stamps, st.ids, st.bearings)
    seen = 0
    for kind, k in st.events():
        (fg.stream_imu if kind == "imu" else fg.stream_vision)(k)
        seen += kind == "vision"
        if seen == 3:
            break
    fg.synchronize()
    assert fg.num_landmarks(0) == N and fg.device_error() == 0
    other = binding.FilterBatch(synth.template_settings_dict(), capacity=N, batch=B)
    other.set_imu_burst(15)
    t = float(fg.get_time()[0])
    rng = np.random.default_rng(1)
    imu = np.zeros((K, 7))
    imu[:, 0] = t + 0.005 * (1 + np.arange(K))
    imu[:, 1:4] = [0.01, 0.02, -0.01] + 0.01 * rng.standard_normal((K, 3))
    imu[:, 4:7] = [0.3, 0.2, 9.7] + 0.05 * rng.standard_normal((K, 3))
    return fg, other, imu, float(imu[-1, 0] + 0.003)


def _route(fg, other, imu, t1, B):
    import numpy as np

    idx = np.arange(B, dtype=np.int32)
    other.copy_filters(fg, idx, idx)
    for r in imu:
        other.process_imu(r[0], r[1:4], r[4:7])
    other.process_imu(t1, imu[-1, 1:4], imu[-1, 4:7])  # (the step to t1 integrates with the last sample held, as the closing step does)
    return [(other.state_estimate(b), other.marginals(b, local=True)) for b in range(B)]


def timing(B, N, reps=20):
    import numpy as np

    fg, other, imu, t1 = _setup(B, N)
    dev = lambda: fg.forecast(imu, t1, local=True)      # noqa: E731
    host = lambda: _route(fg, other, imu, t1, B)        # noqa: E731
    a, h = dev(), host()  # (first calls: allocations)
    apart = max(float(np.max(np.abs(a["base"][b] - h[b][1]["base"]) / np.max(np.abs(h[b][1]["base"])))) for b in range(B))
    apart_lm = max(float(np.max(np.abs(a["lm"][b] - h[b][1]["lm"]) / np.max(np.abs(h[b][1]["lm"])))) for b in range(B))
    apart_p = max(float(np.max(np.abs(a["p"][b] - h[b][0]["p"]))) for b in range(B))
    dev(), host()
    td, th = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        dev()
        t1_ = time.perf_counter()
        host()
        t2 = time.perf_counter()
        td.append((t1_ - t0) * 1e3)
        th.append((t2 - t1_) * 1e3)
    assert fg.device_error() == 0 and other.device_error() == 0
    q = lambda v: dict(median_ms=round(float(np.median(v)), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3))  # noqa: E731
    print(json.dumps(dict(case="forecast", B=B, N=N, K=K, steps=K + 1, reps=reps, forecast=q(td), copy_route=q(th),
                          speedup_of_medians=round(float(np.median(th) / np.median(td)), 1), spreads_overlap=bool(max(td) >= min(th)),
                          base_rel_apart=apart, lm_rel_apart=apart_lm, p_abs_apart=apart_p)), flush=True)


def kern(B, N):
    fg, other, imu, t1 = _setup(B, N)
    for _ in range(30):
        fg.forecast(imu, t1, local=True)
        _route(fg, other, imu, t1, B)
    assert fg.device_error() == 0 and other.device_error() == 0
    print(f"fckern B={B} N={N}: done")


def summarize(d):
    for path in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
        tag = [t for t in os.path.relpath(path, d).split(os.sep) if t.startswith("fckern_")]
        if not tag:
            continue
        _, B, N = tag[0].split("_")
        B, N = int(B), int(N)
        rows = []
        for r in csv.DictReader(open(path)):
            name = (r.get("Name") or r.get("KernelName") or "").split("(")[0].split("::")[-1]
            rows.append((name, float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3, int(r["Calls"]), float(r["TotalDurationNs"]) / 1e3))
        fc = [x for x in rows if x[0].startswith("k_forecast")]
        # (the route's own kernels: the frames of the set-up launch others, and both legs share the copy engine's launches)
        route = ("k_clone", "k_burst", "k_propagate", "k_build_blocks", "k_riccati", "k_state_estimate", "k_local_jacobian", "k_marginals")
        rest = [x for x in rows if x[0].startswith(route)]
        by = 8.0 * B * ((121 + 42 * N) + 23 * N + (144 + 32 * N)) + 8.0 * B * 144 * (K + 1)
        print(f"{B} x {N}: forecast kernels per call {sum(x[5] for x in fc) / 30:.1f} us in {sum(x[4] for x in fc) / 30:.0f} launches; "
              f"route kernels per call {sum(x[5] for x in rest) / 30:.1f} us in {sum(x[4] for x in rest) / 30:.0f} launches")
        for x in fc:
            tail = f"   {by / 1e6:.3f} MB -> {by / x[1] / 1e6:.4f} TB/s = {100 * by / x[1] / 1e6 / 6.29:.2f} % of 6.29" if "lm" in x[0] else ""
            print(f"    {x[0]:20s} {x[1]:9.1f} / {x[2]:8.1f} / {x[3]:8.1f} us ({x[4]} calls){tail}")
        for x in sorted(rest, key=lambda v: -v[5])[:6]:
            print(f"    {x[0][:40]:40s} {x[1]:9.1f} us avg x {x[4]} calls")


if __name__ == "__main__":
    cmd = sys.argv[1] if len(sys.argv) > 1 else ""
    if cmd == "time":
        timing(int(sys.argv[2]), int(sys.argv[3]))
    elif cmd == "kern":
        kern(int(sys.argv[2]), int(sys.argv[3]))
    elif cmd == "sum":
        summarize(sys.argv[2])
    else:
        raise SystemExit(__doc__)
