"""Measurements behind DESIGN.md section 4.5k (scoring candidate vision frames, eqf_score_vision).  Every leg needs the GPU.

  time B N C [reps [chunk]]
                     FilterBatch.score_vision of C candidates per filter, every candidate naming every landmark (its own small turn of the
                     next frame's bearings), against the route it replaces on the same states -- three frames of a synthetic stream --: per
                     candidate eqf_copy_filters into a scratch handle, eqf_process_vision there with "innovation_stats" on, and
                     eqf_get_innovation_stats for every filter.  The caller has brought the IMU up to the frame's stamp; the fork's vision call
                     is stamped 1 us later (a vision call must integrate), so the two routes differ by Q dt of 1 us.  Both end in a
                     synchronise, both warmed up once, alternated over `reps` repetitions (default 5); prints one JSON line with medians,
                     min / max, the ratio, whether the spreads overlap and how far the two routes' numbers are apart.  chunk: the option
                     "score_chunk" (default 0: as many images per round of launches as the handle has filters).
  kern B N C         a workload for `rocprofv3 --kernel-trace --stats --output-format csv -d DIR/sckern_B_N_C -- python scripts/score_route.py kern
                     B N C`: five calls.
  sum DIR            kernel-trace stats CSVs under DIR/sckern_B_N_C -> k_score_form's bytes -- per block pair of the lower block triangle 72
                     read and 32 written, N (N + 1) / 2 pairs per candidate -- over its time against the measured 6.29 TB/s, the flops of the
                     factorisation kernels -- m^3 / 3 per candidate, m = 2 N -- over theirs against the 63.5 TFLOP/s a plain fp64 product on
                     the matrix cores reaches alone (scripts/gemm_concurrency.py), and every kernel's share of the call."""
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from consistency_bench import kernel_name  # noqa: E402  (scripts/: the directory of this file)
CALLS = 5
SCORE_FACTOR = ("k_factor_diag<ScoreArgs>", "k_factor_panel<ScoreArgs>", "k_factor_trail<ScoreArgs>")


def _setup(B, N, ncand):
    import numpy as np
    from eqf_vio_amd import binding, synth

    st = synth.make_stream(N, duration=0.05 * 4 + 0.06)
    d = synth.template_settings_dict()
    fg = binding.FilterBatch(d, capacity=N, batch=B)
    seen, last = 0, 0
    for kind, k in st.events():
        if kind == "imu":
            last = k
            fg.process_imu(st.imu[k, 0], st.imu[k, 1:4], st.imu[k, 4:7])
        else:
            fg.process_vision(st.vision_stamps[k], st.ids, st.bearings[k])
            seen += 1
            if seen == 3:
                break
    stamp = float(st.vision_stamps[3])
    fg.process_imu(stamp, st.imu[last, 1:4], st.imu[last, 4:7])   # the caller brings the IMU up to the frame it is about to score
    fg.synchronize()
    assert fg.num_landmarks(0) == N and fg.device_error() == 0
    rng = np.random.default_rng(5)
    frames = []
    for c in range(ncand):
        y = st.bearings[3] + 2e-3 * rng.standard_normal((N, 3))
        frames.append(y / np.linalg.norm(y, axis=1, keepdims=True))
    scratch = binding.FilterBatch(d, capacity=N, batch=B)
    scratch.set_option("innovation_stats", 1)
    scratch.set_outlier_gate(binding.GATE_CHORD, 10.0)
    return fg, scratch, st.ids, frames, stamp


def _device(fg, ids, frames):
    B = fg.B
    return fg.score_vision([[ids] * len(frames)] * B, [frames] * B)


def _fork_route(fg, scratch, ids, frames, stamp):
    import numpy as np

    B = fg.B
    idx = np.arange(B, dtype=np.int32)
    nis, ld = np.zeros((B, len(frames))), np.zeros((B, len(frames)))
    for c, y in enumerate(frames):
        scratch.copy_filters(fg, idx, idx)
        scratch.process_vision(stamp + 1e-6, ids, y)
        for b in range(B):
            s = scratch.innovation_stats(b)
            nis[b, c], ld[b, c] = s["nis"], s["logdet_S"]
    scratch.synchronize()
    return nis, ld


def timing(B, N, ncand, reps=5, chunk=0):
    import numpy as np

    fg, scratch, ids, frames, stamp = _setup(B, N, ncand)
    fg.set_option("score_chunk", chunk)
    a = _device(fg, ids, frames)  # (first call: allocations)
    _fork_route(fg, scratch, ids, frames[:1], stamp)
    assert not a.info.any() and fg.device_error() == 0
    td, th, apart_nis, apart_ld = [], [], 0.0, 0.0
    for _ in range(reps):
        t0 = time.perf_counter()
        a = _device(fg, ids, frames)
        t1 = time.perf_counter()
        nis, ld = _fork_route(fg, scratch, ids, frames, stamp)
        t2 = time.perf_counter()
        td.append((t1 - t0) * 1e3)
        th.append((t2 - t1) * 1e3)
        apart_nis = max(apart_nis, float(np.max(np.abs(a.nis - nis) / np.abs(nis))))
        apart_ld = max(apart_ld, float(np.max(np.abs(a.logdet_S - ld))))
    q = lambda v: dict(median_ms=round(float(np.median(v)), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3))  # noqa: E731
    print(json.dumps(dict(case="score_vision", B=B, N=N, candidates=ncand, order=2 * N, reps=reps, score_chunk=chunk, device=q(td), fork_route=q(th),
                          speedup_of_medians=round(float(np.median(th) / np.median(td)), 2), spreads_overlap=bool(max(td) >= min(th)),
                          nis_rel_apart=apart_nis, logdet_abs_apart=apart_ld, nis_max=float(np.max(a.nis)))), flush=True)


def kern(B, N, ncand):
    fg, _, ids, frames, _ = _setup(B, N, ncand)
    for _ in range(CALLS):
        _device(fg, ids, frames)
    assert fg.device_error() == 0
    print(f"sckern B={B} N={N} C={ncand}: done")


def summarize(d):
    for path in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
        tag = [t for t in os.path.relpath(path, d).split(os.sep) if t.startswith("sckern_")]
        if not tag:
            continue
        _, B, N, ncand = tag[0].split("_")
        B, N, ncand = int(B), int(N), int(ncand)
        rows = {}
        for r in csv.DictReader(open(path)):
            name = kernel_name(r.get("Name") or r.get("KernelName") or "")
            rows[name] = (float(r["TotalDurationNs"]) / 1e3, int(r["Calls"]))
        mine = {k: v for k, v in rows.items() if k in SCORE_FACTOR + ("k_score_form", "k_score_tail")}
        m, items = 2 * N, B * ncand
        by = CALLS * items * (N * (N + 1) // 2) * (72 + 32)
        fl = CALLS * items * m ** 3 / 3.0
        form = rows.get("k_score_form", (0.0, 0))
        fac = [(k, v) for k, v in rows.items() if k in SCORE_FACTOR]
        tf = sum(v[0] for _, v in fac)
        total = sum(v[0] for v in mine.values())
        print(f"{B} x {N} x {ncand} candidates (order {m}, {CALLS} calls): the route's kernels take {total / CALLS:.1f} us per call")
        if form[1]:
            print(f"    k_score_form  {form[0] / CALLS:10.1f} us per call in {form[1] // CALLS} launches ({100 * form[0] / total:.1f} %); "
                  f"{by / CALLS / 1e6:.3f} MB -> {by / form[0] / 1e6:.3f} TB/s = {100 * by / form[0] / 1e6 / 6.29:.1f} % of 6.29")
        if tf:
            print(f"    factorisation {tf / CALLS:10.1f} us per call in {sum(v[1] for _, v in fac) // CALLS} launches ({100 * tf / total:.1f} %); "
                  f"{fl / CALLS / 1e9:.3f} Gflop -> {fl / tf / 1e6:.3f} TFLOP/s = {100 * fl / tf / 1e6 / 63.5:.2f} % of 63.5")
            for k, v in sorted(fac, key=lambda kv: -kv[1][0]):
                print(f"        {k:28s} {v[0] / CALLS:10.1f} us per call, {v[1] // CALLS} launches")
        if "k_score_tail" in rows:
            print(f"    k_score_tail  {rows['k_score_tail'][0] / CALLS:10.1f} us per call, {rows['k_score_tail'][1] // CALLS} launches "
                  f"({100 * rows['k_score_tail'][0] / total:.1f} %)")


if __name__ == "__main__":
    cmd = sys.argv[1] if len(sys.argv) > 1 else ""
    if cmd == "time":
        timing(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]) if len(sys.argv) > 5 else 5,
               int(sys.argv[6]) if len(sys.argv) > 6 else 0)
    elif cmd == "kern":
        kern(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
    elif cmd == "sum":
        summarize(sys.argv[2])
    else:
        raise SystemExit(__doc__)
