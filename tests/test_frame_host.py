"""The landmark bookkeeping of a vision frame (eqf_vio_amd/csrc/eqf_frame.hpp: host only, standard library only) without a GPU and without
loading anything into Python: tests/frame_host_main.cpp is compiled with g++ under the address and undefined-behaviour sanitizers and run as
a child process, cases on stdin, results on stdout.  Every expected value is computed here, with sets and numpy, or by the CPU oracle -- never
by the header."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDIT_MAX, EDIT_SAFE_N = 1024, 59  # kEditMax, kEditSafeN of eqf_churn.hpp (the header takes them as arguments)
THR = 0.05


@pytest.fixture(scope="module")
def frame_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("frame_host") / "frame_host")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "eqf_vio_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "frame_host_main.cpp")], check=True)

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        return [[int(t) for t in ln.split()] for ln in r.stdout.split("\n")[:-1]]

    return run


def test_header_is_host_only_and_compiles_with_plain_gcc(tmp_path):
    path = os.path.join(ROOT, "eqf_vio_amd", "csrc", "eqf_frame.hpp")
    includes = [ln.split()[1] for ln in open(path) if ln.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "eqf_frame.hpp"\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.dirname(path), str(tu)], check=True)


# ---- scenes: (cap, [(active, state ids, measurement ids), ...]); the measurement ascending, the state in any order
def lst(v):
    v = list(v)
    return f"{len(v)} " + " ".join(str(int(x)) for x in v)


def scene_text(sc):
    cap, fl = sc
    return f"{len(fl)} {cap} " + " ".join(f"{int(a)} {lst(ids)} {lst(meas)}" for a, ids, meas in fl)


SCENES = {
    "one filter, some lost, some new": (8, [(1, [3, 5, 6, 7], [2, 5, 7, 9])]),
    "nothing changes": (8, [(1, [1, 2, 3], [1, 2, 3])]),
    "empty state": (8, [(1, [], [4, 8, 9])]),
    "empty measurement": (8, [(1, [4, 8, 9], [])]),
    "both empty": (4, [(1, [], [])]),
    "all lost, others new": (8, [(1, [1, 2, 3], [10, 11])]),
    "returning id: state order not ascending": (8, [(1, [5, 9, 12, 2], [2, 5, 9, 11, 12])]),
    "not ascending and one lost": (8, [(1, [7, 3, 9, 1], [1, 3, 8, 9])]),
    "three filters, the middle one inactive": (6, [(1, [1, 2, 3], [2, 3, 4]), (0, [5, 6], [6, 7, 8]), (1, [9, 4], [4, 9])]),
    "three filters: empty state, all lost, full": (5, [(1, [], [1, 2]), (1, [3, 4], []), (1, [5, 1, 2, 3, 4], [1, 2, 3, 4, 5])]),
    "inactive only": (4, [(0, [1, 2], [2, 3])]),
    "measurement fills the capacity": (4, [(1, [2], [1, 2, 3, 4])]),
}
for _n in (58, 59, 60):  # around kEditSafeN
    SCENES[f"{_n} measurement entries"] = (64, [(1, list(range(0, 2 * _n - 6, 2)), list(range(0, 2 * _n, 2)))])
SCENES["state of kEditMax + 1"] = (EDIT_MAX + 1, [(1, list(range(EDIT_MAX, -1, -1)), list(range(EDIT_MAX + 1)))])
SCENES["kEditMax and kEditMax + 1 side by side"] = (EDIT_MAX + 1, [(1, list(range(EDIT_MAX)), list(range(EDIT_MAX))),
                                                                    (0, list(range(EDIT_MAX + 1)), [])])


def ref_keep(fl):
    keep = [[i for i, x in enumerate(ids) if not a or x in set(meas)] for a, ids, meas in fl]
    return keep, any(len(k) != len(f[1]) for k, f in zip(keep, fl))


def after_keep(sc):
    """the scene once the lost landmarks are gone (every state id of an active filter is in the measurement)"""
    cap, fl = sc
    return cap, [(a, [ids[i] for i in k], meas) for (a, ids, meas), k in zip(fl, ref_keep(fl)[0])]


def test_keep_list_and_apply_keep(frame_host):
    out = iter(frame_host("\n".join("keep " + scene_text(sc) for sc in SCENES.values())))
    for name, (cap, fl) in SCENES.items():
        keep, lost = ref_keep(fl)
        assert next(out) == [int(lost)], name
        assert [next(out) for _ in fl] == keep, name
        assert [next(out) for _ in fl] == [[ids[i] for i in k] for (_, ids, _), k in zip(fl, keep)], name
    assert {n for n, (c, fl) in SCENES.items() if ref_keep(fl)[1]} >= {"all lost, others new", "empty measurement", "not ascending and one lost"}


def ref_perm(fl):
    return [[meas.index(x) for x in ids] if a else [-1] * len(ids) for a, ids, meas in fl]


def test_permutation_identity_and_unmatched_entries(frame_host):
    cases = {n: after_keep(sc) for n, sc in SCENES.items()}
    dropped = {n: [list(range(len(meas)))[1::3] for _, _, meas in fl] for n, (cap, fl) in cases.items()}  # (every third entry from the second)
    out = iter(frame_host("\n".join("perm " + scene_text(sc) + " " + " ".join(lst(d) for d in dropped[n]) for n, sc in cases.items())))
    seen = set()
    for name, (cap, fl) in cases.items():
        perm = ref_perm(fl)
        assert [next(out) for _ in fl] == perm, name
        ident = [p == list(range(len(p))) for p in perm]
        want = [int(all(ident)), int(all(i for i, f in zip(ident, fl) if f[0]))]
        assert next(out) == want, name
        seen.add(tuple(want))
        un = [[k for k in range(len(meas)) if k not in set(p)] for p, (_, _, meas) in zip(perm, fl)]
        assert [next(out) for _ in fl] == un, name
        assert [next(out) for _ in fl] == [[k for k in u if k not in set(d)] for u, d in zip(un, dropped[name])], name
    assert seen == {(1, 1), (0, 1), (0, 0)}  # identity; identity but for an inactive filter; a real permutation


def ref_image(sc, gate_armed):
    cap, fl = sc
    B = len(fl)
    keep, _ = ref_keep(fl)
    maps = np.full((2, B, cap), -1, dtype=np.int64)
    counts = np.zeros((B, 4), dtype=np.int64)
    new_ids = []
    for b, ((a, ids, meas), k) in enumerate(zip(fl, keep)):
        kept = [ids[i] for i in k]
        fresh = [j for j, x in enumerate(meas) if x not in set(kept)] if a else []
        row = ([meas.index(x) for x in kept] + fresh) if a else []
        maps[0, b, :len(k)] = k
        maps[1, b, :len(row)] = row
        counts[b] = [len(k), len(fresh), int(bool(gate_armed and a)), 0]
        new_ids.append(kept + [meas[j] for j in fresh])
    work = [len(n) for n, f in zip(new_ids, fl) if f[0] and n]
    skipped = [b for b, (n, f) in enumerate(zip(new_ids, fl)) if f[0] and not n]
    return np.concatenate([maps.ravel(), counts.ravel()]), new_ids, [len(k) for k in keep], skipped, bool(work), max(work, default=0)


def test_k_edit_eligibility_and_upload_image(frame_host):
    cases = [(n, sc, h, g) for n, sc in SCENES.items() for h in (1, 0) for g in (0, 1)]
    cases.append(("measurement beyond the capacity", (2, [(1, [1], [1, 2, 3])]), 1, 0))
    out = iter(frame_host("\n".join(f"edit {scene_text(sc)} {h} {g} {EDIT_MAX} {EDIT_SAFE_N}" for _, sc, h, g in cases)))
    verdicts = {}
    for name, sc, handle_ok, gate in cases:
        cap, fl = sc
        keep, lost = ref_keep(fl)
        ok = bool(handle_ok) and all(len(ids) <= EDIT_MAX for _, ids, _ in fl) and not (gate and any(a and len(m) < EDIT_SAFE_N for a, _, m in fl))
        fresh = any(a and len(m) > len(k) for (a, _, m), k in zip(fl, keep))
        got = next(out)
        fits = all(len(m) <= cap for a, _, m in fl if a)
        assert got[0] == int(ok) and got[2:] == [int(lost), int(fits)], (name, handle_ok, gate)
        if ok:
            assert got[1] == int(fresh), name  # (only meaningful for an eligible frame)
        verdicts[name, handle_ok, gate] = ok
        if not fits:
            continue
        image, new_ids, n_kept, skipped, any_work, n_max = ref_image(sc, gate)
        assert next(out) == [int(any_work), n_max], name
        assert np.array_equal(np.array(next(out), dtype=np.int64), image), name  # integer for integer
        assert [next(out) for _ in fl] == new_ids, name
        assert next(out) == n_kept and next(out) == skipped, name
    assert not verdicts["58 measurement entries", 1, 1] and verdicts["59 measurement entries", 1, 1] and verdicts["60 measurement entries", 1, 1]
    assert verdicts["58 measurement entries", 1, 0] and not verdicts["state of kEditMax + 1", 1, 0]
    assert not verdicts["kEditMax and kEditMax + 1 side by side", 1, 0] and not verdicts["60 measurement entries", 0, 0]


def test_pinned_image_layout(frame_host):
    """The frame's pinned image against the formula written out: 3 cap B doubles of bearings, then 2 B cap + 4 B ints (keep | perm |
    counts) rounded up to doubles -- what eqf_create has always allocated.  That editImage writes exactly editInts() ints and nothing behind
    them is the canary of the `edit` command (test_k_edit_eligibility_and_upload_image) and the sanitizer."""
    cases = [(B, cap) for B in (1, 3, 8) for cap in (1, 5, 21, 200)]
    for (B, cap), got in zip(cases, frame_host("\n".join(f"layout {B} {cap}" for B, cap in cases))):
        ints = 2 * B * cap + 4 * B
        total = 3 * cap * B + (ints + 1) // 2
        assert got == [3 * cap, 3 * cap * B, 0, B * cap, 2 * B * cap, ints, 3 * cap * B, total], (B, cap)
        keep, perm, counts = got[2:5]
        assert keep + B * cap <= perm and perm + B * cap <= counts and counts + 4 * B == ints  # ascending, no overlap, no gap
        assert (8 * got[6]) % 4 == 0 and 8 * (total - got[6]) >= 4 * ints  # (the ints fit behind the bearings)


# ---- the gate: (scene after the lost landmarks are gone, chords per filter and landmark)
NAN = float("nan")
GATES = {
    "no outlier": ((8, [(1, [2, 5, 7], [2, 5, 7, 9])]), [[0.0, 0.01, 0.05]]),  # (a chord AT the threshold stays)
    "the last landmark": ((8, [(1, [2, 5, 7], [2, 5, 7, 9])]), [[0.0, 0.0, 1.0]]),
    "the only landmark": ((8, [(1, [5], [2, 5])]), [[0.3]]),
    "every landmark": ((8, [(1, [2, 5], [2, 5])]), [[0.06, 2.0]]),
    "a NaN chord keeps its landmark": ((8, [(1, [2, 5, 7], [2, 5, 7])]), [[NAN, 1.0, NAN]]),
    "state order not ascending": ((8, [(1, [9, 2, 12, 5], [2, 5, 9, 11, 12])]), [[1.0, 0.0, 0.0, 1.0]]),
    "empty state": ((4, [(1, [], [1, 2])]), [[]]),
    "three filters, the middle one inactive": ((6, [(1, [1, 2, 3], [1, 2, 3, 4]), (0, [5, 6], [5, 6]), (1, [9, 4], [4, 9])]),
                                               [[0.0, 1.0, 0.0], [1.0, 1.0], [0.0, 0.0]]),
    "three filters, outliers in two": ((6, [(1, [1, 2, 3], [1, 2, 3, 4]), (1, [5, 6], [5, 6]), (1, [9, 4], [4, 9])]),
                                       [[0.0, 0.0, 1.0], [0.0, 0.0], [1.0, 0.0]]),
}


def chords_text(chords):
    return " ".join(repr(float(c)) for row in chords for c in row)


def test_synchronous_gate(frame_host):
    out = iter(frame_host("\n".join(f"gatesync {scene_text(sc)} {THR} {chords_text(ch)}" for sc, ch in GATES.values())))
    for name, ((cap, fl), chords) in GATES.items():
        hit = [[bool(a) and c > THR for c in row] for (a, _, _), row in zip(fl, chords)]
        assert next(out) == [int(any(any(h) for h in hit))], name
        assert [next(out) for _ in fl] == [[i for i, x in enumerate(h) if not x] for h in hit], name
        assert [next(out) for _ in fl] == [sorted(meas.index(ids[i]) for i, x in enumerate(h) if x) for (_, ids, meas), h in zip(fl, hit)], name


def test_host_redo_of_a_speculative_gate(frame_host):
    """the state holds the landmarks the frame appended behind the first nOld: the redo takes them out again with the outliers"""
    cases = []
    for name, ((cap, fl), chords) in GATES.items():
        for flags in ([1] * len(fl), [0] * len(fl), [1, 0, 1][:len(fl)]):
            grown, n_old, ch = [], [], []
            for (a, ids, meas), row in zip(fl, chords):
                new = [x for x in meas if x not in set(ids)] if a else []
                grown.append((a, ids + new, meas))
                n_old.append(len(ids))
                ch.append(list(row) + [7.0] * len(new))  # (chords of the appended ones are never looked at)
            cases.append((name, (cap, grown), flags, n_old, ch))
    out = iter(frame_host("\n".join(f"gateredo {scene_text(sc)} {THR} " + " ".join(f"{f} {n}" for f, n in zip(fl, no)) + " " + chords_text(ch)
                                    for _, sc, fl, no, ch in cases)))
    redone = 0
    for name, (cap, fl), flags, n_old, chords in cases:
        act = [int(bool(f) and bool(a)) for f, (a, _, _) in zip(flags, fl)]
        assert next(out) == [int(any(act))], name
        assert next(out) == act and next(out) == act, name  # (the flags become the mask of the redo)
        if not any(act):
            continue
        redone += 1
        hit = [[bool(t) and i < n and c > THR for i, c in enumerate(row)] for t, n, row in zip(act, n_old, chords)]
        keep = [[i for i in range(len(ids)) if (not t or i < n) and not h[i]] for t, n, (_, ids, _), h in zip(act, n_old, fl, hit)]
        assert [next(out) for _ in fl] == keep, name
        assert [next(out) for _ in fl] == [sorted(meas.index(ids[i]) for i, x in enumerate(h) if x) for (_, ids, meas), h in zip(fl, hit)], name
    assert redone >= len(GATES)


def test_ids_after_the_gate_on_the_device(frame_host):
    """the state is kept landmarks, then the frame's new ones; flag 2 = k_edit switched the queued update off"""
    cases = []
    for name, ((cap, fl), chords) in GATES.items():
        for flags in ([1] * len(fl), [2] * len(fl), [0, 2, 1][:len(fl)]):
            grown, n_kept, ch = [], [], []
            for (a, ids, meas), row in zip(fl, chords):
                new = [x for x in meas if x not in set(ids)] if a else []
                grown.append((a, ids + new, meas))
                n_kept.append(len(ids))
                ch.append(list(row) + [7.0] * len(new))
            cases.append((name, (cap, grown), flags, n_kept, ch))
    out = iter(frame_host("\n".join(f"gatedev {scene_text(sc)} {THR} " + " ".join(f"{f} {n}" for f, n in zip(fl, nk)) + " " + chords_text(ch)
                                    for _, sc, fl, nk, ch in cases)))
    deferred_seen = 0
    for name, (cap, fl), flags, n_kept, chords in cases:
        ids = [[x for j, (x, c) in enumerate(zip(i, row)) if not (f and a) or j >= n or not c > THR]
               for f, n, (a, i, _), row in zip(flags, n_kept, fl, chords)]
        late = [int(f == 2 and bool(a) and bool(i)) for f, (a, _, _), i in zip(flags, fl, ids)]
        assert [next(out) for _ in fl] == ids, name
        assert next(out) == late, name
        assert next(out) == [int(any(late)), max([len(i) for i, t in zip(ids, late) if t], default=0)], name
        deferred_seen += any(late)
    assert deferred_seen >= 5


# ---- random histories: the oracle's verdict per frame supplies the chords, and every route must leave the oracle's id list, in its order
@pytest.fixture(scope="module")
def histories(oracle_lib):
    from eqf_vio_amd import synth

    out = {}
    for seed in (1, 2, 3, 4):
        pool = 40
        st = synth.make_stream(pool, seed=700 + seed, duration=0.8)
        rng = np.random.default_rng(seed)
        F = st.bearings.shape[0]
        out_frames = tuple(int(k) for k in np.where(rng.random(F) < 0.34)[0] if k >= 2)
        meas = synth.churn_measurements(st, seed=50 + seed, max_visible=28, outlier_frames=out_frames, outlier_angle=0.2)
        d = synth.template_settings_dict()
        d["outlierThreshold"] = THR
        fo = oracle_lib.OracleFilter(d)
        frames, removed, lost, added, unsorted = [], 0, 0, 0, 0
        for kind, k in st.events():
            if kind == "imu":
                r = st.imu[k]
                fo.processIMUData(r[0], r[1:4], r[4:7])
                continue
            mi, my = meas[k]
            before = fo.ids().tolist()
            fo.processVisionData(st.vision_stamps[k], mi, my)
            after = fo.ids().tolist()
            gone = sorted((set(before) & set(mi.tolist())) - set(after))  # in the measurement and still thrown out: the gate (chord 1.0)
            frames.append((mi.tolist(), gone, after))
            removed += len(gone)
            lost += len(set(before) - set(mi.tolist()))
            added += len(set(after) - set(before))
            unsorted += int(np.any(np.diff(after) < 0))
        # (or the test would pass without exercising the paths it is about)
        assert removed >= 2 and lost >= 20 and added >= 20 and unsorted >= 10, (seed, removed, lost, added, unsorted)
        out[seed] = (pool, frames)
    return out


@pytest.mark.parametrize("route", [0, 1, 2], ids=["synchronous gate", "speculative probe with host redo", "one launch with the device gate"])
def test_every_route_leaves_the_oracles_ids_on_random_histories(frame_host, histories, route):
    # (the histories see fewer than kEditSafeN landmarks: the one-launch route gets 0 for it, or an armed gate would never take it)
    safe_n = 0 if route == 2 else EDIT_SAFE_N
    text = "\n".join(f"history {route} 1 {pool} {THR} {EDIT_MAX} {safe_n} {len(frames)} " + " ".join(f"1 {lst(mi)} {lst(gone)}" for mi, gone, _ in frames)
                     for pool, frames in histories.values())
    out = iter(frame_host(text))
    for seed, (pool, frames) in histories.items():
        for k, (_, _, after) in enumerate(frames):
            assert next(out) == [route], (seed, k)  # the route the frame took
            assert next(out) == after, (seed, k)
