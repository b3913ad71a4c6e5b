"""Measurements behind DESIGN.md section 4.5j (pairwise merge costs, eqf_get_merge_costs).  Every leg needs the GPU.

  time B N [reps]  FilterBatch.merge_costs over all B (B - 1) / 2 pairs of the B filters of a handle (Runnalls, first = 0; ends in a
                   synchronise) against the host route it replaces on the same states -- three frames of a synthetic stream, every filter
                   resampled from one parent and perturbed with its own draw --: sigma_local(b) for every member (an (11 + 3N)^2 matrix over
                   the bus each), then consistency.merge_costs_host (numpy slogdet and solve per pair).  Both warmed up on a small handle's
                   worth of pairs, alternated over `reps` repetitions (default: 5, 2 and 1 at 8 x 200, 64 x 200 and 16 x 1000: the host
                   route takes minutes there); prints one JSON line with medians, min / max, the ratio and how far the two are apart.
  kern B N         a workload for `rocprofv3 --kernel-trace --stats --output-format csv -d DIR/mckern_B_N -- python scripts/merge_cost_route.py kern
                   B N`: five calls.
  sum DIR          kernel-trace stats CSVs under DIR/mckern_B_N -> k_pair_form's bytes -- per pair two lower triangles read and one
                   written, per member one read and one written, 8 bytes an entry -- over its time against the measured 6.29 TB/s, and
                   the flops of the factorisation kernels -- m^3 / 3 per image, m = 12 + 3 N -- over theirs against the 63.5 TFLOP/s a plain
                   fp64 product on the matrix cores reaches alone (scripts/gemm_concurrency.py)."""
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from consistency_bench import FACTOR, kernel_name  # noqa: E402  (scripts/: the directory of this file)
CALLS = 5


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
    fg.resample(np.zeros(B, dtype=np.int32))
    fg.perturb(np.random.default_rng(3), scale=np.linspace(0.0, 0.05, B))
    w = np.random.default_rng(4).uniform(0.5, 1.5, B)
    return fg, np.arange(B, dtype=np.int32), w


def _route(fg, idx, w, ref):
    from eqf_vio_amd import consistency as cs

    pulled = [fg.sigma_local(int(b)) for b in idx]  # what the host route moves over the bus
    ms = []
    for b in idx:
        m = fg.dump_state(int(b))
        m["estimate"] = fg.state_estimate(int(b))
        ms.append(m)
    return cs.merge_costs_host(ms, w, ref), pulled


def timing(B, N, reps=None):
    import numpy as np

    if reps is None:
        reps = 5 if B * N <= 1600 else (2 if N <= 200 else 1)
    fg, idx, w = _setup(B, N)
    ref = int(np.argmax(w))
    dev = lambda: fg.merge_costs(idx, w, ref=int(idx[ref]))  # noqa: E731
    a = dev()  # (first call: allocations)
    _route(fg, idx[:2], w[:2], 0)
    assert not a["info"].any() and fg.device_error() == 0
    td, th, apart = [], [], 0.0
    for _ in range(reps):
        t0 = time.perf_counter()
        a = dev()
        t1 = time.perf_counter()
        h, _ = _route(fg, idx, w, ref)
        t2 = time.perf_counter()
        td.append((t1 - t0) * 1e3)
        th.append((t2 - t1) * 1e3)
        apart = max(apart, float(np.max(np.abs(a["cost"] - h["cost"]))))
    q = lambda v: dict(median_ms=round(float(np.median(v)), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3))  # noqa: E731
    print(json.dumps(dict(case="merge_costs", B=B, N=N, pairs=len(a["cost"]), order=12 + 3 * N, reps=reps, device=q(td), host_route=q(th),
                          speedup_of_medians=round(float(np.median(th) / np.median(td)), 1), spreads_overlap=bool(max(td) >= min(th)),
                          cost_abs_apart=apart, cost_max=float(np.max(a["cost"])))), flush=True)


def kern(B, N):
    fg, idx, w = _setup(B, N)
    for _ in range(CALLS):
        fg.merge_costs(idx, w, ref=0)
    assert fg.device_error() == 0
    print(f"mckern B={B} N={N}: done")


def summarize(d):
    for path in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
        tag = [t for t in os.path.relpath(path, d).split(os.sep) if t.startswith("mckern_")]
        if not tag:
            continue
        _, B, N = tag[0].split("_")
        B, N = int(B), int(N)
        rows = {}
        for r in csv.DictReader(open(path)):
            name = kernel_name(r.get("Name") or r.get("KernelName") or "")
            rows[name] = (float(r["TotalDurationNs"]) / 1e3, int(r["Calls"]))
        m, pairs = 12 + 3 * N, B * (B - 1) // 2
        tri = 8.0 * m * (m + 1) / 2
        by = CALLS * (pairs * 3 * tri + B * 2 * tri)
        fl = CALLS * (pairs + B) * m ** 3 / 3.0
        form = rows.get("k_pair_form", (0.0, 0))
        fac = [(k, v) for k, v in rows.items() if k in FACTOR["NeesArgs"]]
        tf = sum(v[0] for _, v in fac)
        print(f"{B} x {N} ({pairs} pairs, order {m}, {CALLS} calls):")
        if form[1]:
            print(f"    k_pair_form   {form[0] / CALLS:10.1f} us per call in {form[1] // CALLS} launches; {by / CALLS / 1e9:.3f} GB -> "
                  f"{by / form[0] / 1e6:.3f} TB/s = {100 * by / form[0] / 1e6 / 6.29:.1f} % of 6.29")
        if tf:
            print(f"    factorisation {tf / CALLS:10.1f} us per call in {sum(v[1] for _, v in fac) // CALLS} launches; {fl / CALLS / 1e9:.2f} Gflop -> "
                  f"{fl / tf / 1e6:.2f} TFLOP/s = {100 * fl / tf / 1e6 / 63.5:.1f} % of 63.5")
            for k, v in sorted(fac, key=lambda kv: -kv[1][0]):
                print(f"        {k:24s} {v[0] / CALLS:10.1f} us per call, {v[1] // CALLS} launches")
        for k in ("k_nees_tail", "k_pair_tail", "k_sigma_local", "k_mix_error", "k_mix_estimate", "k_local_jacobian"):
            if k in rows:
                print(f"    {k:14s}{rows[k][0] / CALLS:10.1f} us per call, {rows[k][1] / CALLS:.0f} launches")


if __name__ == "__main__":
    cmd = sys.argv[1] if len(sys.argv) > 1 else ""
    if cmd == "time":
        timing(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]) if len(sys.argv) > 4 else None)
    elif cmd == "kern":
        kern(int(sys.argv[2]), int(sys.argv[3]))
    elif cmd == "sum":
        summarize(sys.argv[2])
    else:
        raise SystemExit(__doc__)
