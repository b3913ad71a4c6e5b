"""A/B of the covariance downdate on the integer matrix pipe (eqf_set_option "downdate_slices", csrc/eqf_i8.hpp) against the fp64 downdate,
in ONE process, stream mode, the two legs alternating round by round: 1, 8 and 64 filters of N = 200, one filter of N = 1000 and of N = 4000.
Per leg: steps/s (IMU + vision events per second over the timed rounds, best round) and the update's kernel time per vision frame from the
handle's profile (EQF_PROF_CHOL_RESIDENT + EQF_PROF_DOWNDATE, the event-bracket times of eqf_profile_get; one profiled round of its own).
    python scripts/i8_downdate_ab.py [slices=6] [rounds=3] [shapes=all | 64x200,...]"""
import os
import sys
import time

for _v in ("OPENBLAS_NUM_THREADS", "OMP_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ.setdefault(_v, "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from eqf_vio_amd import binding, synth

slices = int(sys.argv[1]) if len(sys.argv) > 1 else 6
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
SHAPES = [(1, 200, 2.0), (8, 200, 2.0), (64, 200, 1.0), (1, 1000, 0.6), (1, 4000, 0.36)]
if len(sys.argv) > 3 and sys.argv[3] != "all":
    want = {tuple(int(x) for x in s.split("x")) for s in sys.argv[3].split(",")}
    SHAPES = [s for s in SHAPES if (s[0], s[1]) in want]
d = synth.template_settings_dict()


def make(B, N, st, S):
    fb = binding.FilterBatch(d, capacity=N, batch=B)
    fb.set_option("downdate_slices", S)
    fb.stream_upload(st.imu, st.vision_stamps, st.ids, st.bearings)
    return fb


def run(fb, st):
    ev = list(st.events())
    fb.synchronize()
    t0 = time.perf_counter()
    for kind, k in ev:
        (fb.stream_imu if kind == "imu" else fb.stream_vision)(k)
    fb.synchronize()
    return len(ev) / (time.perf_counter() - t0), sum(1 for e in ev if e[0] != "imu")


def update_us(fb, st):
    fb.profile_enable(True)
    _, nf = run(fb, st)
    p = fb.profile()
    fb.profile_enable(False)
    ms = p["k_chol_resident"][1] + p["k_downdate"][1]  # (EQF_PROF_CHOL_RESIDENT + EQF_PROF_DOWNDATE)
    steps = {name: v for name, v in p.items() if v[0]}
    return 1000.0 * ms / nf, steps


print(f"# i8 downdate A/B: slices={slices}, rounds={rounds} (alternating), stream mode; steps/s = best round; update = resident + downdate "
      f"kernel time per vision frame from eqf_profile_get")
for B, N, dur in SHAPES:
    st = synth.make_stream(N, duration=dur)
    legs = {0: make(B, N, st, 0), slices: make(B, N, st, slices)}
    for fb in legs.values():  # warm-up (first-use allocations, role tables)
        run(fb, st)
    best = {s: 0.0 for s in legs}
    for r in range(rounds):
        for s, fb in legs.items():
            best[s] = max(best[s], run(fb, st)[0] * B)
    upd = {s: update_us(fb, st) for s, fb in legs.items()}
    dev = max(float(np.linalg.norm(legs[slices].sigma(b) - legs[0].sigma(b)) / np.linalg.norm(legs[0].sigma(b))) for b in range(min(B, 4)))
    f64, i8 = best[0], best[slices]
    print(f"B={B:3d} N={N:5d}: steps/s fp64 {f64:10.1f}  i8 {i8:10.1f}  ({100.0 * (i8 / f64 - 1.0):+.1f} %)   update us/frame fp64 "
          f"{upd[0][0]:9.1f}  i8 {upd[slices][0]:9.1f}  ({100.0 * (upd[slices][0] / upd[0][0] - 1.0):+.1f} %)   Sigma dev {dev:.1e}")
    for s in legs:
        print(f"    profile classes (slices={s}): " + ", ".join(f"{k} {v[0]}x {v[1]:.2f} ms" for k, v in upd[s][1].items()))
    for fb in legs.values():
        fb.close()
