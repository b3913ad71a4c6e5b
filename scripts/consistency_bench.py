"""Measurements behind DESIGN.md section 4.5c (estimate-frame covariance, innovation statistics).  Every leg needs the GPU.

  kernels B N      a workload for `rocprofv3 --kernel-trace --stats -- python scripts/consistency_bench.py kernels B N`: k_sigma_local (batched
                   over the handle's B filters, eqf_debug_sigma_local_all) next to k_riccati_stream (single-step split propagate,
                   EQF_SPLIT_PROPAGATE=1 + imu burst 0) on the same Sigma, 30 launches each.  Algorithmic bytes of either: 2 n^2 * 8 * B,
                   n = 12 + 3 N (read Sigma once, write it once).
  wall N           wall time of marginals() / sigma_local() / sigma() through the binding.
  ab B N MODE      stream-mode timing, MODE = off | on ("innovation_stats"); EQF_VIO_AMD_LIB selects another build of the library (the
                   parent commit's, for off-against-parent).  Prints one JSON line: events/s (IMU + vision calls), us per vision frame.
  frames N F MODE  F vision frames in stream mode and nothing else (for a kernel-trace table of what an update launches).
  nees B N         the joint NEES of every filter of a handle, two routes in one process on the same states after three frames, nrhs = 1:
                   (a) FilterBatch.nees (one call, ends in a synchronise), (b) the host route it replaces, sigma_local(b) for every b +
                   consistency.nees_joint.  Both warmed up, alternated over 20 repetitions; prints one JSON line with medians, min / max.
  neeskern B N     a workload for `rocprofv3 --kernel-trace --stats -- python scripts/consistency_bench.py neeskern B N`: ten nees calls.
  neessum DIR      kernel-trace stats CSVs under DIR/neeskern_B_N -> summed time of the factorisation's kernels (k_factor_*<NeesArgs>) and
                   k_nees_tail per call against B n^3 / 3 flops at the fp64 matrix peak (78.6 Tflop/s).
  summarize DIR    kernel-trace stats CSVs under DIR -> the table of the `kernels` legs (achieved bytes/s, ratio).
  copy B N         DESIGN.md section 4.5d: FilterBatch.copy_filters (ends in a synchronise of both handles here) against the host route it
                   replaces, dump_state + restore_state for every filter, on the same states after three frames; once for a whole-handle copy
                   into a second handle and once for an in-place fan-out (every filter continues from filter 0).  Both warmed up, alternated
                   over 20 repetitions; prints one JSON line per case with medians, min / max and the ratio.
  copykern B N     a workload for `rocprofv3 --kernel-trace --stats -- python scripts/consistency_bench.py copykern B N`: k_clone_sigma (a
                   whole-handle copy into a second handle) next to k_sigma_local (eqf_debug_sigma_local_all) on the same Sigma, 30 each.
  copysum DIR      kernel-trace stats CSVs under DIR/copykern_B_N -> k_clone_sigma against k_sigma_local (both 2 n^2 * 8 * B bytes).
  sample B N       DESIGN.md section 4.5e: FilterBatch.perturb (stats=True: ends in a synchronise) against the host route it replaces, for
                   every filter dump_state (the covariance over the bus) + numpy Cholesky + L z + restore_state -- WITHOUT the group
                   arithmetic the host would also have to redo, so the host route is timed in its favour -- on the same states after three
                   frames, scale 1e-3 so that forty moves leave the filters where they were to first order.  Both warmed up, alternated over
                   20 repetitions; prints one JSON line with medians, min / max and the ratio.  No threshold is asserted.
  linear B N m     DESIGN.md section 4.5f: FilterBatch.update_linear(stats=True: ends in a synchronise) against the host route it replaces,
                   for every filter dump_state (the covariance over the bus) + consistency.linear_update_host + restore_state -- WITHOUT
                   the group arithmetic the host would also have to redo, so the host route is timed in its favour -- on the same states
                   after three frames.  m = 3: the velocity rows; otherwise dense rows; R is a hundred times H Sigma H^T's mean diagonal
                   and the residual a thousandth of a standard deviation, so that forty updates leave the filters where they were to
                   first order.  Both warmed up, alternated over 20 repetitions; prints one JSON line with medians, min / max, the ratio
                   and whether the spreads overlap.  No threshold is asserted.
  linearkern B N m a workload for `rocprofv3 --kernel-trace --stats -- python scripts/consistency_bench.py linearkern B N m`: thirty updates.
  linearsum DIR    kernel-trace stats CSVs under DIR/linearkern_B_N_m -> the four k_lin_* kernels; k_lin_gain as n^2 * 8 * B bytes (one read
                   of Sigma) and k_lin_downdate as (2 T_lower + T_mirror) * 64^2 * 8 * B bytes (read and write of the lower-triangle tiles,
                   write of the mirror tiles) over their average times, against the measured 6.29 TB/s.
  blocks B N K     DESIGN.md section 4.5h: FilterBatch.update_landmarks with K stereo entries per filter (2 rows each, the rig of
                   consistency.stereo_rows; wait=True: ends in a synchronise) against the host route it replaces, for every filter
                   dump_state (the covariance over the bus) + consistency.update_landmarks_host + restore_state -- WITHOUT the group
                   arithmetic the host would also have to redo, so the host route is timed in its favour -- on the same states after three
                   frames.  The second camera's bearings agree with the estimate (residual 0) and R is a hundred times H Sigma H^T's
                   mean diagonal, so that forty updates leave the filters where they were to first order.  Both warmed up, alternated
                   over 20 repetitions; prints one JSON line with medians, min / max, the ratio and whether the spreads overlap.  No
                   threshold is asserted.
  blockskern B N K a workload for `rocprofv3 --kernel-trace --stats -- python scripts/consistency_bench.py blockskern B N K`: thirty updates.
  blockssum DIR    kernel-trace stats CSVs under DIR/blockskern_B_N_K -> the k_blk_* kernels and the factorisation's (k_factor_*<BlkArgs>);
                   k_blk_downdate as (2 T_lower + T_mirror) * 64^2 * 8 * B bytes of Sigma (read and write of the lower-triangle tiles, write
                   of the mirror tiles) plus 2 * 64 * m * 8 bytes of Y per tile, over its average time, against the measured 6.29 TB/s.
  mixture B N      DESIGN.md section 4.5g: FilterBatch.merge of all B filters into filter 0 (report=True: ends in a synchronise) against
                   the host route it replaces -- sigma_local(b), state_estimate(b) and bias(b) for every member (n^2 doubles over the bus
                   each), the numpy sums of consistency.merge_host's second pass WITHOUT its Jacobians and chart transitions, so the host
                   route is timed in its favour, then restore_state (Sigma over the bus again) -- on the same states: B copies of one
                   filter after three frames, pulled apart by perturb(scale 1e-3), equal weights.  Both warmed up, alternated over 20
                   repetitions; prints one JSON line with medians, min / max and the ratio.  No threshold is asserted.
  mixturekern B N  a workload for `rocprofv3 --kernel-trace --stats -- python scripts/consistency_bench.py mixturekern B N`: thirty merges.
  mixturesum DIR   kernel-trace stats CSVs under DIR/mixturekern_B_N -> the k_mix_* kernels; k_mix_reduce as (B T_lower + T_all) n^2-sized
                   bytes -- it reads the lower triangle of every member's Sigma once, (n^2 + n) / 2 * 8 * B bytes, and writes P once,
                   n^2 * 8 bytes -- over its average time, against the measured 6.29 TB/s.
"""
import csv
import glob
import json
import os
import re
import sys
import time


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _filled(B, N, frames=3, burst=None, stats=None, duration=None):
    from eqf_vio_amd import binding, synth

    st = synth.make_stream(N, duration=duration or (0.05 * frames + 0.06))
    fg = binding.FilterBatch(synth.template_settings_dict(), capacity=N, batch=B)
    if burst is not None:
        fg.set_imu_burst(burst)
    if stats is not None:
        fg.set_option("innovation_stats", stats)
    fg.stream_upload(st.imu, st.vision_stamps, st.ids, st.bearings)
    return fg, st


def kernels(B, N):
    os.environ["EQF_SPLIT_PROPAGATE"] = "1"
    fg, st = _filled(B, N, frames=3, burst=0)
    ev = list(st.events())
    seen = 0
    for i, (kind, k) in enumerate(ev):
        (fg.stream_imu if kind == "imu" else fg.stream_vision)(k)
        seen += kind == "vision"
        if seen == 3:
            break
    fg.synchronize()
    assert fg.num_landmarks(0) == N and fg.device_error() == 0
    t = float(fg.get_time()[0])
    for j in range(30):
        t += 0.005
        fg.process_imu(t, [0.01, 0.02, -0.01], [9.7, 0.3, 0.2])  # one Riccati step: k_build_blocks + k_riccati_stream
        fg.debug_sigma_local_all()                               # k_local_jacobian + k_sigma_local over all B filters
    fg.synchronize()
    assert fg.device_error() == 0
    print(f"kernels B={B} N={N}: done")


def wall(N):
    fg, st = _filled(1, N, frames=2)
    for kind, k in st.events():
        (fg.stream_imu if kind == "imu" else fg.stream_vision)(k)
    fg.synchronize()
    out = {}
    for name, fn in (("marginals(local=True)", lambda: fg.marginals(0, local=True)), ("sigma_local()", lambda: fg.sigma_local(0)),
                     ("sigma()", lambda: fg.sigma(0))):
        fn()  # (first call: allocations)
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        out[name] = min(ts) * 1e3
    n = 11 + 3 * N
    print(f"wall N={N}: " + ", ".join(f"{k} {v:.2f} ms" for k, v in out.items()) +
          f"  (bytes to the host: {(121 + 9 * N) * 8 / 1e3:.0f} KB against {n * n * 8 / 1e6:.0f} MB)")


def ab(B, N, mode, reps=3):
    dur = 2.2 if N <= 200 else 0.6
    fg, st = _filled(B, N, duration=dur, stats=None)
    if mode == "on":
        fg.set_option("innovation_stats", 1)
    elif mode != "off":
        raise SystemExit("MODE is off or on")
    ev = list(st.events())
    nvis = sum(1 for kind, _ in ev if kind == "vision")
    warm = [i for i, (kind, _) in enumerate(ev) if kind == "vision"][max(1, nvis // 5)] + 1
    best = None
    for _ in range(reps):
        fg.reset()
        for kind, k in ev[:warm]:
            (fg.stream_imu if kind == "imu" else fg.stream_vision)(k)
        fg.synchronize()
        t0 = time.perf_counter()
        for kind, k in ev[warm:]:
            (fg.stream_imu if kind == "imu" else fg.stream_vision)(k)
        fg.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    assert fg.device_error() == 0
    nev = len(ev) - warm
    nfr = sum(1 for kind, _ in ev[warm:] if kind == "vision")
    print(json.dumps(dict(B=B, N=N, mode=mode, lib=os.environ.get("EQF_VIO_AMD_LIB", "this tree"), events_per_s=round(nev * B / best, 1),
                          us_per_frame=round(best / nfr * 1e6, 2), frames=nfr)))


def frames(N, F, mode):
    fg, st = _filled(1, N, frames=F)
    if mode == "on":
        fg.set_option("innovation_stats", 1)
    seen = 0
    for kind, k in st.events():
        (fg.stream_imu if kind == "imu" else fg.stream_vision)(k)
        seen += kind == "vision"
        if seen == F:
            break
    fg.synchronize()
    assert fg.device_error() == 0
    print(f"frames N={N} F={seen} mode={mode}: done")


def _nees_setup(B, N):
    import numpy as np

    fg, st = _filled(B, N, frames=3)
    seen = 0
    for kind, k in st.events():
        (fg.stream_imu if kind == "imu" else fg.stream_vision)(k)
        seen += kind == "vision"
        if seen == 3:
            break
    fg.synchronize()
    assert fg.num_landmarks(0) == N and fg.device_error() == 0
    rng = np.random.default_rng(1)
    E = 1e-2 * rng.standard_normal((B, 1, 11 + 3 * N))
    return fg, E


def nees(B, N, reps=20):
    import numpy as np
    from eqf_vio_amd import consistency

    fg, E = _nees_setup(B, N)

    def device():
        return fg.nees(E, local=True, first=0)["nees"][:, 0]

    def host():
        return np.array([consistency.nees_joint(fg.sigma_local(b), E[b, 0])["nees"] for b in range(B)])

    a, h = device(), host()  # (first calls: allocations)
    rel = float(np.max(np.abs(a - h) / h))
    device(), host()
    ta, th = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        device()
        t1 = time.perf_counter()
        host()
        t2 = time.perf_counter()
        ta.append((t1 - t0) * 1e3)
        th.append((t2 - t1) * 1e3)
    q = lambda v: dict(median_ms=round(float(np.median(v)), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3))
    print(json.dumps(dict(B=B, N=N, reps=reps, device=q(ta), host=q(th), speedup_of_medians=round(float(np.median(th) / np.median(ta)), 1),
                          device_vs_host_rel=rel)))


def sample(B, N, reps=20):
    import numpy as np

    fg, _ = _nees_setup(B, N)
    n = 11 + 3 * N
    z = np.random.default_rng(2).standard_normal((B, 1, n))
    scale = np.full(B, 1e-3)

    def device():
        return fg.perturb(z, first=0, scale=scale, stats=True)["info"]

    def host():
        for b in range(B):
            snap = fg.dump_state(b)
            S = np.tril(snap["sigma"])
            gamma = scale[b] * (np.linalg.cholesky(S + np.tril(S, -1).T) @ z[b, 0])
            snap["bias"] = snap["bias"] + gamma[0:6]  # (the group step is left out: see the module docstring)
            fg.restore_state(snap, b)

    assert not np.any(device())  # (first calls: allocations)
    host()
    device(), host()
    ta, th = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        device()
        t1 = time.perf_counter()
        host()
        t2 = time.perf_counter()
        ta.append((t1 - t0) * 1e3)
        th.append((t2 - t1) * 1e3)
    assert fg.device_error() == 0
    q = lambda v: dict(median_ms=round(float(np.median(v)), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3))
    print(json.dumps(dict(case="perturb", B=B, N=N, reps=reps, device=q(ta), host=q(th),
                          speedup_of_medians=round(float(np.median(th) / np.median(ta)), 1))))


def _linear_setup(B, N, m):
    import numpy as np
    from eqf_vio_amd import consistency

    fg, _ = _nees_setup(B, N)
    n = 11 + 3 * N
    H = consistency.velocity_rows(N) if m == 3 else np.random.default_rng(3).standard_normal((m, n))
    Hs = np.ascontiguousarray(np.broadcast_to(H, (B, m, n)))
    Sl = fg.sigma_local(0)
    d = float(np.mean(np.diag(H @ Sl @ H.T)))
    R = 100.0 * d * np.eye(m)
    r = 1e-3 * np.sqrt(d) * np.random.default_rng(4).standard_normal((B, m))
    return fg, H, Hs, r, R


def linear(B, N, m, reps=20):
    import numpy as np
    from eqf_vio_amd import consistency

    fg, H, Hs, r, R = _linear_setup(B, N, m)

    def device():
        return fg.update_linear(Hs, r, R, local=True, stats=True)["info"]

    def host():
        for b in range(B):
            snap = fg.dump_state(b)
            J = consistency.jacobian_matrix(consistency.local_jacobian_blocks(snap["origin"], snap["group"]))
            up = consistency.linear_update_host(snap["sigma"], H @ J, r[b], R)
            snap["sigma"] = up["Sigma"]
            snap["bias"] = snap["bias"] + up["gamma"][0:6]  # (the group step is left out: see the module docstring)
            fg.restore_state(snap, b)

    assert not np.any(device())  # (first calls: allocations)
    host()
    device(), host()
    ta, th = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        device()
        t1 = time.perf_counter()
        host()
        t2 = time.perf_counter()
        ta.append((t1 - t0) * 1e3)
        th.append((t2 - t1) * 1e3)
    assert fg.device_error() == 0
    q = lambda v: dict(median_ms=round(float(np.median(v)), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3))
    print(json.dumps(dict(case="update_linear", B=B, N=N, m=m, reps=reps, device=q(ta), host=q(th),
                          speedup_of_medians=round(float(np.median(th) / np.median(ta)), 1), spreads_overlap=bool(max(ta) >= min(th)))), flush=True)


def linearkern(B, N, m):
    import numpy as np

    fg, H, Hs, r, R = _linear_setup(B, N, m)
    for _ in range(30):
        assert not np.any(fg.update_linear(Hs, r, R, local=True, stats=True)["info"])
    assert fg.device_error() == 0
    print(f"linearkern B={B} N={N} m={m}: done")


def linearsum(d):
    print("B x N x m      kernel            avg / min / max us (calls)      bytes        TB/s (avg)   of 6.29")
    for path in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
        tag = [t for t in os.path.relpath(path, d).split(os.sep) if t.startswith("linearkern_")]
        if not tag:
            continue
        _, B, N, m = tag[0].split("_")
        B, N, m = int(B), int(N), int(m)
        n = 12 + 3 * N
        nt = -(-n // 64)
        by = {"k_lin_gain": 8.0 * n * n * B, "k_lin_downdate": 8.0 * 64 * 64 * B * (2 * nt * (nt + 1) // 2 + nt * (nt - 1) // 2)}
        for r in csv.DictReader(open(path)):
            name = r.get("Name") or r.get("KernelName") or ""
            for key in ("k_lin_rows", "k_lin_gain", "k_lin_solve", "k_lin_downdate", "k_apply_increment", "k_local_jacobian"):
                if key in name:
                    a, lo, hi = float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3
                    tail = f"{by[key] / 1e6:10.2f} MB   {by[key] / a / 1e6:6.3f}   {100 * by[key] / a / 1e6 / 6.29:5.1f} %" if key in by else ""
                    print(f"{B:3d} x {N:<5d} x {m:<2d} {key:24s} {a:9.1f} / {lo:8.1f} / {hi:8.1f} ({r['Calls']:>3s})   {tail}")


def _blocks_setup(B, N, K):
    import numpy as np
    from eqf_vio_amd import consistency

    fg, _ = _nees_setup(B, N)
    q21, t21 = np.array([0.9987502603949663, 0.0, 0.04997916927067833, 0.0]), np.array([0.12, 0.0, 0.005])
    R21 = consistency.quat_to_matrix(q21)
    lm = np.linspace(0, N - 1, K).astype(int)
    ids, Hs, rs, Rs, idx = [], [], [], [], []
    for b in range(B):
        est, snap = fg.state_estimate(b), fg.dump_state(b)
        J = np.asarray(consistency.local_jacobian_blocks(snap["origin"], snap["group"])["lm"]).reshape(-1, 3, 3)
        H = np.array([consistency.stereo_rows(est["p"][i], q21, t21, R21.T @ (est["p"][i] - t21) / np.linalg.norm(est["p"][i] - t21))[0] for i in lm])
        d = float(np.mean([np.diag(H[k] @ J[i] @ snap["sigma"][11 + 3 * i:14 + 3 * i, 11 + 3 * i:14 + 3 * i] @ J[i].T @ H[k].T) for k, i in enumerate(lm)]))
        ids.append(snap["ids"][lm]), Hs.append(H), rs.append(np.zeros((K, 2))), Rs.append(100.0 * d * np.eye(2)), idx.append(lm)
    return fg, ids, Hs, rs, Rs, idx


def blocks(B, N, K, reps=20):
    import numpy as np
    from eqf_vio_amd import consistency

    fg, ids, Hs, rs, Rs, idx = _blocks_setup(B, N, K)

    def device():
        return fg.update_landmarks(ids, Hs, rs, Rs, rows=2, local=True)["info"]

    def host():
        for b in range(B):
            snap = fg.dump_state(b)
            J = consistency.local_jacobian_blocks(snap["origin"], snap["group"])["lm"]
            up = consistency.update_landmarks_host(snap["sigma"], idx[b], Hs[b], rs[b], np.broadcast_to(Rs[b], (K, 2, 2)), J)
            snap["sigma"] = up["Sigma"]
            snap["bias"] = snap["bias"] + up["gamma"][0:6]  # (the group step is left out: see the module docstring)
            fg.restore_state(snap, b)

    assert not np.any(device())  # (first calls: allocations)
    host()
    device(), host()
    ta, th = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        device()
        t1 = time.perf_counter()
        host()
        t2 = time.perf_counter()
        ta.append((t1 - t0) * 1e3)
        th.append((t2 - t1) * 1e3)
    assert fg.device_error() == 0
    q = lambda v: dict(median_ms=round(float(np.median(v)), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3))
    print(json.dumps(dict(case="update_landmarks", B=B, N=N, entries=K, rows=2, reps=reps, device=q(ta), host=q(th),
                          speedup_of_medians=round(float(np.median(th) / np.median(ta)), 1), spreads_overlap=bool(max(ta) >= min(th)))), flush=True)


def blockskern(B, N, K):
    import numpy as np

    fg, ids, Hs, rs, Rs, idx = _blocks_setup(B, N, K)
    for _ in range(30):
        assert not np.any(fg.update_landmarks(ids, Hs, rs, Rs, rows=2, local=True)["info"])
    assert fg.device_error() == 0
    print(f"blockskern B={B} N={N} K={K}: done")


def kernel_name(raw):
    """A traced kernel's name without return type, namespaces and argument list; an instantiation keeps its argument type, which tells the
    routes of the shared factorisation apart: 'void eqf::k_factor_trail<eqf::BlkArgs>(eqf::BlkArgs, int, int)' -> 'k_factor_trail<BlkArgs>'"""
    head = re.sub(r"\b\w+::", "", raw.split("(")[0]).split()
    return head[-1] if head else ""


# the three kernels of the blocked factorisation by route (csrc/eqf_factor.hpp; a library from before it: the per-route names)
FACTOR = {"NeesArgs": ("k_factor_diag<NeesArgs>", "k_factor_panel<NeesArgs>", "k_factor_trail<NeesArgs>", "k_nees_diag", "k_nees_panel", "k_nees_trail"),
          "BlkArgs": ("k_factor_diag<BlkArgs>", "k_factor_panel<BlkArgs>", "k_factor_trail<BlkArgs>", "k_blk_diag", "k_blk_panel", "k_blk_trail")}


def blockssum(d):
    print("B x N x K      kernel            avg / min / max us (calls)      bytes        TB/s (avg)   of 6.29")
    for path in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
        tag = [t for t in os.path.relpath(path, d).split(os.sep) if t.startswith("blockskern_")]
        if not tag:
            continue
        _, B, N, K = tag[0].split("_")
        B, N, K = int(B), int(N), int(K)
        n, m = 12 + 3 * N, 2 * K
        nt = -(-n // 64)
        tl = nt * (nt + 1) // 2
        by = {"k_blk_downdate": 8.0 * B * (64 * 64 * (2 * tl + nt * (nt - 1) // 2) + 2 * 64 * m * tl)}
        for r in csv.DictReader(open(path)):
            name = kernel_name(r.get("Name") or r.get("KernelName") or "")
            for key in ("k_blk_rows", "k_blk_gain") + FACTOR["BlkArgs"] + ("k_blk_gamma", "k_blk_tail", "k_blk_downdate", "k_apply_increment",
                                                                         "k_local_jacobian"):
                if key == name:
                    a, lo, hi = float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3
                    tail = f"{by[key] / 1e6:10.2f} MB   {by[key] / a / 1e6:6.3f}   {100 * by[key] / a / 1e6 / 6.29:5.1f} %" if key in by else ""
                    print(f"{B:3d} x {N:<5d} x {K:<3d} {key:24s} {a:9.1f} / {lo:8.1f} / {hi:8.1f} ({r['Calls']:>3s})   {tail}")


def neeskern(B, N):
    fg, E = _nees_setup(B, N)
    for _ in range(10):
        fg.nees(E, local=True, first=0)
    print(f"neeskern B={B} N={N}: done")


def neessum(d):
    for path in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
        tag = [t for t in os.path.relpath(path, d).split(os.sep) if t.startswith("neeskern_")]
        if not tag:
            continue
        _, B, N = tag[0].split("_")
        B, N = int(B), int(N)
        tot, calls, parts = 0.0, 0, []
        for r in csv.DictReader(open(path)):
            name = kernel_name(r.get("Name") or r.get("KernelName") or "")
            if name in FACTOR["NeesArgs"] or name == "k_nees_tail":
                tot += float(r["TotalDurationNs"])
                parts.append(f"{name} {float(r['TotalDurationNs']) / 1e3:.0f} us / {r['Calls']}")
                if name == "k_nees_tail":
                    calls = int(r["Calls"])
        if not calls:
            continue
        n = 11 + 3 * N
        us = tot / calls / 1e3
        fl = B * n ** 3 / 3.0
        print(f"{B:3d} x {N:<5d} factorisation + k_nees_tail {us:10.1f} us per call, {fl / 1e9:8.2f} Gflop -> {fl / us / 1e6:7.2f} Tflop/s = {100 * fl / us / 1e6 / 78.6:5.2f} % of 78.6"
              f"   [{'; '.join(parts)}]")


def _copy_setup(B, N):
    fg, st = _filled(B, N, frames=3)
    seen = 0
    for kind, k in st.events():
        (fg.stream_imu if kind == "imu" else fg.stream_vision)(k)
        seen += kind == "vision"
        if seen == 3:
            break
    fg.synchronize()
    assert fg.num_landmarks(0) == N and fg.device_error() == 0
    from eqf_vio_amd import binding, synth

    other = binding.FilterBatch(synth.template_settings_dict(), capacity=N, batch=B)
    return fg, other


def copy(B, N, reps=20):
    import numpy as np

    fg, other = _copy_setup(B, N)
    idx = np.arange(B, dtype=np.int32)
    zero = np.zeros(B, dtype=np.int32)

    def dev_across():
        other.copy_filters(fg, idx, idx)
        other.synchronize()
        fg.synchronize()

    def host_across():
        for b in range(B):
            other.restore_state(fg.dump_state(b), b)

    def dev_fan():
        other.copy_filters(other, idx, zero)
        other.synchronize()

    def host_fan():
        snap = other.dump_state(0)
        for b in range(1, B):
            other.restore_state(snap, b)

    for name, dev, host in (("across", dev_across, host_across), ("fanout", dev_fan, host_fan)):
        if name == "fanout" and B == 1:
            # (one filter: an in-place fan-out is the identity and moves nothing; the snapshot / roll-back pair across handles is the row above)
            print(json.dumps(dict(case=name, B=B, N=N, note="identity: nothing moves")))
            continue
        dev(), host(), dev(), host()  # (first calls: allocations)
        td, th = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            dev()
            t1 = time.perf_counter()
            host()
            t2 = time.perf_counter()
            td.append((t1 - t0) * 1e3)
            th.append((t2 - t1) * 1e3)
        q = lambda v: dict(median_ms=round(float(np.median(v)), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3))
        same = all(np.array_equal(other.sigma(b), fg.sigma(0 if name == "fanout" else b)) for b in {0, B - 1})
        print(json.dumps(dict(case=name, B=B, N=N, reps=reps, device=q(td), host=q(th),
                              speedup_of_medians=round(float(np.median(th) / np.median(td)), 1),
                              device_slower_than_fastest_host=bool(max(td) >= min(th)), sigma_equal=bool(same))), flush=True)
    assert fg.device_error() == 0 and other.device_error() == 0


def copykern(B, N):
    import numpy as np

    fg, other = _copy_setup(B, N)
    idx = np.arange(B, dtype=np.int32)
    for _ in range(30):
        fg.debug_sigma_local_all()
        other.copy_filters(fg, idx, idx)
    fg.synchronize()
    other.synchronize()
    assert fg.device_error() == 0 and other.device_error() == 0
    print(f"copykern B={B} N={N}: done")


def copysum(d):
    print("B x N      bytes (2 n^2 8 B)   k_clone_sigma avg / min / max us   TB/s (avg)   k_sigma_local avg / min / max us   TB/s (avg)   clone / local (avg)")
    for path in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
        tag = [t for t in os.path.relpath(path, d).split(os.sep) if t.startswith("copykern_")]
        if not tag:
            continue
        _, B, N = tag[0].split("_")
        B, N = int(B), int(N)
        got = {}
        for r in csv.DictReader(open(path)):
            name = r.get("Name") or r.get("KernelName") or ""
            for key in ("k_clone_sigma", "k_sigma_local", "k_clone_small", "k_clone_restore"):
                if key in name:
                    got[key] = (float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3, int(r["Calls"]))
        if "k_clone_sigma" not in got or "k_sigma_local" not in got:
            print(B, N, "incomplete", got)
            continue
        n = 12 + 3 * N
        by = 2.0 * n * n * 8 * B
        c, l = got["k_clone_sigma"], got["k_sigma_local"]
        print(f"{B:3d} x {N:<5d} {by / 1e6:10.1f} MB   {c[0]:9.1f} / {c[1]:8.1f} / {c[2]:8.1f}   {by / c[0] / 1e6:6.2f}   {l[0]:9.1f} / {l[1]:8.1f} / {l[2]:8.1f}   "
              f"{by / l[0] / 1e6:6.2f}   {c[0] / l[0]:.2f}   (k_clone_small {got.get('k_clone_small', (0,))[0]:.1f} us, k_clone_restore "
              f"{got.get('k_clone_restore', (0,))[0]:.1f} us; {c[3]} / {l[3]} calls)")


def _mixture_setup(B, N):
    import numpy as np

    fg, _ = _copy_setup(B, N)
    fg.resample(np.zeros(B, dtype=np.int32))
    fg.perturb(np.random.default_rng(3), scale=1e-3)
    fg.synchronize()
    return fg


def mixture(B, N, reps=20):
    import numpy as np

    from eqf_vio_amd import consistency as cs

    fg = _mixture_setup(B, N)
    idx, w = np.arange(B, dtype=np.int32), np.ones(B)

    def dev():
        assert fg.merge(idx, w, 0, 0)["info"] == 0

    def host():
        est = [fg.state_estimate(b) for b in range(B)]
        bias = [fg.bias(b) for b in range(B)]
        S = [fg.sigma_local(b) for b in range(B)]
        E = np.array([cs.error_vector(cs.local_error(est[0], est[b], bias=bias[0], true_bias=bias[b])) for b in range(B)])
        mean = E.mean(axis=0)
        xbar = cs.local_retract(est[0], mean, bias=bias[0])
        D = E - mean
        P = sum(S) / B + D.T @ D / B
        snap = fg.dump_state(0)
        N0 = len(snap["ids"])
        snap["origin"] = dict(q=xbar["q"], x=np.mean([e["x"] for e in est], axis=0), v=xbar["v"], p=xbar["p"])
        snap["group"] = dict(Aq=np.array([1.0, 0, 0, 0]), Ax=np.zeros(3), w=np.zeros(3), Qq=np.tile([1.0, 0, 0, 0], (N0, 1)), Qa=np.ones(N0))
        snap["bias"], snap["sigma"] = xbar["bias"], P
        fg.restore_state(snap, 0)

    dev(), host(), dev(), host()  # (first calls: allocations)
    td, th = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        dev()
        t1 = time.perf_counter()
        host()
        t2 = time.perf_counter()
        td.append((t1 - t0) * 1e3)
        th.append((t2 - t1) * 1e3)
    q = lambda v: dict(median_ms=round(float(np.median(v)), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3))
    print(json.dumps(dict(case="merge", B=B, N=N, reps=reps, launches=fg.debug_mixture_launches(), device=q(td), host=q(th),
                          speedup_of_medians=round(float(np.median(th) / np.median(td)), 1),
                          device_slower_than_fastest_host=bool(max(td) >= min(th)))), flush=True)
    assert fg.device_error() == 0


def mixturekern(B, N):
    import numpy as np

    fg = _mixture_setup(B, N)
    idx, w = np.arange(B, dtype=np.int32), np.ones(B)
    for _ in range(30):
        fg.merge(idx, w, 0, 0, report=False)
    fg.synchronize()
    assert fg.device_error() == 0
    print(f"mixturekern B={B} N={N}: done")


def mixturesum(d):
    print("B x N      bytes read + written   k_mix_reduce avg / min / max us   TB/s (avg)   of 6.29 TB/s   the other k_mix_* (avg us)")
    for path in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
        tag = [t for t in os.path.relpath(path, d).split(os.sep) if t.startswith("mixturekern_")]
        if not tag:
            continue
        _, B, N = tag[0].split("_")
        B, N = int(B), int(N)
        got = {}
        for r in csv.DictReader(open(path)):
            name = r.get("Name") or r.get("KernelName") or ""
            for key in ("k_mix_reduce", "k_mix_estimate", "k_mix_error", "k_mix_mean", "k_mix_retract", "k_mix_report", "k_mix_store",
                        "k_mix_commit", "k_mix_restore", "k_local_jacobian"):
                if key in name:
                    got[key] = (float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3, int(r["Calls"]))
        if "k_mix_reduce" not in got:
            print(B, N, "incomplete", got)
            continue
        n = 12 + 3 * N
        by = 8.0 * (B * (n * n + n) / 2 + n * n)
        c = got["k_mix_reduce"]
        rest = ", ".join(f"{k[6:] if k.startswith('k_mix_') else k} {v[0]:.1f}" for k, v in sorted(got.items()) if k != "k_mix_reduce")
        print(f"{B:3d} x {N:<5d} {by / 1e6:10.1f} MB   {c[0]:9.1f} / {c[1]:8.1f} / {c[2]:8.1f}   {by / c[0] / 1e6:6.2f}   {by / c[0] / 1e6 / 6.29:6.1%}   {rest}")


def summarize(d):
    rows = []
    for path in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
        tag = os.path.relpath(path, d).split(os.sep)[0]  # kernels_B_N
        try:
            _, B, N = tag.split("_")
            B, N = int(B), int(N)
        except ValueError:
            continue
        avg = {}
        for r in csv.DictReader(open(path)):
            name = r.get("Name") or r.get("KernelName") or ""
            for key in ("k_sigma_local", "k_riccati_stream", "k_local_jacobian", "k_build_blocks"):
                if key in name:
                    avg[key] = (float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, int(r["Calls"]))
        rows.append((B, N, avg))
    print("B x N      bytes (2 n^2 8 B)   k_sigma_local avg / min us   TB/s (avg)   k_riccati_stream avg / min us   TB/s (avg)   sigma_local / riccati time")
    for B, N, avg in rows:
        n = 12 + 3 * N
        by = 2.0 * n * n * 8 * B
        if "k_sigma_local" not in avg or "k_riccati_stream" not in avg:
            print(B, N, "incomplete", avg)
            continue
        a, r = avg["k_sigma_local"], avg["k_riccati_stream"]
        print(f"{B:3d} x {N:<5d} {by / 1e6:10.1f} MB   {a[0]:10.1f} / {a[1]:8.1f}   {by / a[0] / 1e6:6.2f}   {r[0]:10.1f} / {r[1]:8.1f}   {by / r[0] / 1e6:6.2f}   {a[0] / r[0]:.2f}"
              f"   (k_local_jacobian {avg.get('k_local_jacobian', (0, 0, 0))[0]:.1f} us)")


if __name__ == "__main__":
    cmd = sys.argv[1]
    if cmd == "kernels":
        kernels(int(sys.argv[2]), int(sys.argv[3]))
    elif cmd == "wall":
        wall(int(sys.argv[2]))
    elif cmd == "ab":
        ab(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
    elif cmd == "frames":
        frames(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
    elif cmd == "nees":
        nees(int(sys.argv[2]), int(sys.argv[3]))
    elif cmd == "neeskern":
        neeskern(int(sys.argv[2]), int(sys.argv[3]))
    elif cmd == "neessum":
        neessum(sys.argv[2])
    elif cmd == "copy":
        copy(int(sys.argv[2]), int(sys.argv[3]))
    elif cmd == "copykern":
        copykern(int(sys.argv[2]), int(sys.argv[3]))
    elif cmd == "copysum":
        copysum(sys.argv[2])
    elif cmd == "sample":
        sample(int(sys.argv[2]), int(sys.argv[3]))
    elif cmd == "linear":
        linear(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
    elif cmd == "linearkern":
        linearkern(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
    elif cmd == "linearsum":
        linearsum(sys.argv[2])
    elif cmd == "blocks":
        blocks(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
    elif cmd == "blockskern":
        blockskern(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
    elif cmd == "blockssum":
        blockssum(sys.argv[2])
    elif cmd == "mixture":
        mixture(int(sys.argv[2]), int(sys.argv[3]))
    elif cmd == "mixturekern":
        mixturekern(int(sys.argv[2]), int(sys.argv[3]))
    elif cmd == "mixturesum":
        mixturesum(sys.argv[2])
    elif cmd == "summarize":
        summarize(sys.argv[2])
    else:
        raise SystemExit(__doc__)
