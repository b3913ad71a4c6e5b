"""What eqf_observe_landmarks_iterated needs on the host, without a GPU: the binding's symbol with its argument types (no handle is
created), and the layouts, the argument checks, the launch count, an entry's rows at a trial point and the stop rule of
eqf_vio_amd/csrc/eqf_iterate_host.hpp (the kernels of csrc/eqf_iterate.hpp call the same functions) -- tests/iterate_host_main.cpp is
compiled FOR THE HOST with g++ under the address and undefined-behaviour sanitizers and run as a child process, cases on stdin as hex
floats, results on stdout.  The rows at a trial point are held to the 50-digit reference of tests/iterate_exact.py inside K_OBS's bound."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import iterate_cases as ic
import iterate_exact as ix
from eqf_vio_amd import consistency as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ID_CAM = [1.0, 0, 0, 0, 0, 0, 0]


def test_binding_exports_the_symbol_with_its_argument_types():
    from eqf_vio_amd import binding

    for s in ("eqf_observe_landmarks_iterated", "eqf_debug_iterate_launches"):
        assert s in binding.EXPORTED_SYMBOLS
    L = binding.lib()
    dp, ip, up, vp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_ubyte), C.c_void_p
    assert L.eqf_observe_landmarks_iterated.argtypes == [vp, C.c_int, dp, C.c_int, ip, ip, C.c_int, dp, dp, C.c_double, C.c_double, up, ip, ip,
                                                         C.c_int, C.c_int, C.c_double, up, dp, dp, dp, C.c_int,
                                                         C.POINTER(binding.LinearReport), dp, C.POINTER(binding.IterReport)]
    assert [f[0] for f in binding.IterReport._fields_] == ["n_lin", "status", "last_step"] and C.sizeof(binding.IterReport) == 16
    one, d = (C.c_int * 1)(1), (C.c_double * 9)()
    # a NULL handle is refused by the library itself, before anything touches a device
    assert L.eqf_observe_landmarks_iterated(None, 0, None, 0, one, one, 1, d, d, 1.0, 1.0, None, None, None, 0, 2, 0.0, None, None, None, None,
                                            0, None, None, None) == binding.ERR_INVALID
    assert L.eqf_debug_iterate_launches(None) == binding.ERR_INVALID
    header = open(os.path.join(ROOT, "include", "eqf_vio_amd.h")).read()
    assert "int eqf_observe_landmarks_iterated(eqf_filter* f, int kind, const double* cam" in header and "} eqf_iter_report;" in header
    assert "#define EQF_ITER_MAX_LIN 16" in header
    assert (cs.ITER_CONVERGED, cs.ITER_EXHAUSTED, cs.ITER_STALLED, cs.ITER_SOLVE_FAILED, cs.ITER_MASKED) == (0, 1, 2, 3, 4)
    cpp = open(os.path.join(ROOT, "eqf_vio_amd", "cpp", "VIOFilter.h")).read()
    assert cpp.count("eqf_iter_report processLandmarkObservations(") == 1 and "int max_lin, double tol, eqf_linear_report* report" in cpp


@pytest.fixture(scope="module")
def iterate_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("iterate_host") / "iterate_host")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I",
                    os.path.join(ROOT, "eqf_vio_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "iterate_host_main.cpp")], check=True)

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        return [ln.split() for ln in r.stdout.split("\n")[:-1]]

    return run


def _hx(a):
    return " ".join(float(v).hex() for v in np.asarray(a, dtype=float).reshape(-1))


def test_argument_checks(iterate_host):
    inf, nan = float("inf"), float("nan")
    cases = [(1, 0.0, 1), (16, 0.0, 1), (2, 1e-9, 1), (8, 5.0, 1), (0, 0.0, 0), (-1, 0.0, 0), (17, 0.0, 0), (2, -1e-300, 0), (2, nan, 0),
             (2, inf, 0), (2, -inf, 0), (2, -0.0, 1)]
    out = iterate_host("\n".join(f"args {m} {float(t).hex()}" for m, t, _ in cases))
    assert [int(o[0]) for o in out] == [c[2] for c in cases]


def test_launch_count_depends_on_stride_rows_and_max_lin_only(iterate_host):
    shapes = [(1, 1, 1), (1, 1, 2), (40, 2, 4), (33, 2, 3), (22, 3, 3), (64, 1, 16), (65, 1, 2), (257, 1, 3), (200, 2, 4)]
    out = iterate_host("\n".join(f"launches {s} {r} {m}" for s, r, m in shapes))
    for (s, r, m), o in zip(shapes, out):
        nb = (s * r + 63) // 64
        want = 0 if m == 1 else (m - 1) * (3 + 3 * nb - 1) + 1
        assert [int(o[0]), int(o[1])] == [want, want], (s, r, m)


def test_layout_offsets(iterate_host):
    lines, want = [], []
    for stride, rows, drec, B, maxlin in ((1, 1, 7, 1, 1), (33, 2, 5120, 3, 4), (45, 3, 5120, 2, 16)):
        lines.append(f"layout {stride} {rows} {drec} {B} {maxlin}")
        mp = (stride * rows + 63) // 64 * 64
        oT = (mp + 1) * mp
        oW = oT + 3 * stride * mp
        oG = oW + mp
        oD = oG + 6 * stride
        e = B * stride
        small = 8 * 7 * B + 8 * e * 3 + 8 * e * rows * rows + 4 * e + 4 * B + B
        want.append([mp, 0, oT, oW, oG, oG + 3 * stride, oD, oD + drec, oD + drec + 1, maxlin * B * stride * 3, small, small + e])
    out = iterate_host("\n".join(lines))
    assert [[int(t) for t in ln] for ln in out] == want


def test_considered_is_a_search_in_the_ascending_list(iterate_host):
    lst = [3, 4, 9, 100, 2000]
    lines = [f"considered {len(lst)} {' '.join(map(str, lst))} {i}" for i in (2, 3, 4, 5, 9, 100, 101, 2000, 2001)] + ["considered 0 7"]
    assert [int(o[0]) for o in iterate_host("\n".join(lines))] == [0, 1, 1, 0, 1, 1, 0, 1, 0, 0]


def _trial_line(kind, p0, q, a, g, cam, meas):
    return f"trial {kind} {_hx(p0)} {_hx(q)} {_hx([a])} {_hx(g)} {_hx(ID_CAM if cam is None else np.concatenate(cam))} {_hx(meas)}"


def test_rows_at_a_trial_point_against_the_exact_reference(iterate_host):
    worst = 0.0
    for c in ic.CASES:
        kind, st, ids, meas, R, cam = ic.case(c)
        host = cs.observe_iterated_host(kind, st["sigma"], st, ids, meas, R, cam, max_lin=2)
        g = host["g_trace"][1]
        assert g.any()
        on = [int(k) for k in np.flatnonzero(host["used"] == 1)]
        ref = ix.one_step(kind, st["sigma"], st, ids, meas, R, g, [], cam)
        rows, sid = cs.OBS_ROWS[kind], [int(i) for i in st["ids"]]
        K = len(ids)
        Ht, rt = np.zeros((K, rows, 3)), np.zeros((K, rows))
        out = iterate_host("\n".join(_trial_line(kind, st["origin"]["p"][sid.index(int(ids[k]))], st["group"]["Qq"][sid.index(int(ids[k]))],
                                                 st["group"]["Qa"][sid.index(int(ids[k]))], g[k], cam, meas[k]) for k in on))
        for k, o in zip(on, out):
            v = [float.fromhex(t) for t in o[:-1]]
            assert int(o[-1]) == 0
            Ht[k], rt[k] = np.array(v[:3 * rows]).reshape(rows, 3), v[3 * rows:]
        rh, rr = ix.row_ratios(Ht, rt, ref)
        print(f"{c}: eqf_iterate_host.hpp / bound: Ht {rh:.3f}, r~ {rr:.3f}")
        worst = max(worst, rh, rr)
    assert worst <= 1.0


def test_a_zero_increment_gives_the_one_shot_rows_and_an_injected_one_stalls(iterate_host):
    q1 = [1.0, 0, 0, 0]
    # g = 0: Q_trial is Q itself (exp of a zero rotation is the unit quaternion exactly), the rows are entryRows's
    kind, st, ids, meas, R, cam = ic.case(ic.CASES[4])
    Ht, resid, _ = cs.observe_rows_host(kind, st, ids, meas, cam)
    out = iterate_host("\n".join(_trial_line(kind, st["origin"]["p"][k], st["group"]["Qq"][k], st["group"]["Qa"][k], [0, 0, 0], cam, meas[k])
                                 for k in range(len(ids))))
    for k, o in enumerate(out):
        v = [float.fromhex(t) for t in o[:-1]]
        assert int(o[-1]) == 0 and np.allclose(v[:3], Ht[k].reshape(-1), rtol=1e-13) and np.allclose(v[3:], resid[k], rtol=1e-12)
    # an increment along p0 large enough for exp to underflow (the scale becomes 0), or to overflow (the point comes to the camera's centre):
    # not observable, rows and r~ zeros -- what stalls a filter
    lines = [_trial_line(kind, [0.0, 0, 2], q1, 1.0, [0.0, 0, s], None, [3.0, 0, 0]) for kind in (0, 1, 2) for s in (2000.0, -2000.0)]
    for o in iterate_host("\n".join(lines)):
        assert int(o[-1]) == 1 and all(float.fromhex(t) == 0.0 for t in o[:-1])


def test_one_linearisation_report_for_every_verdict_word(iterate_host):
    """eqf_iter_report when nothing was iterated (max_lin = 1), from the update's verdict word: only a masked filter (3) took no part; the
    others -- applied, failed, gated, idle (blocks::kInfoIdle = 4), refused by the lift (lift::kWordFailed = 5), singular chart -- used their
    single linearisation, which is all there were (1 = ran out).  Written out, one line per word."""
    want = {0: (1, 1, 0.0), 1: (1, 1, 0.0), 2: (1, 1, 0.0), 3: (0, 4, 0.0), 4: (1, 1, 0.0), 5: (1, 1, 0.0), -1: (1, 1, 0.0)}
    out = iterate_host("\n".join(f"single {w}" for w in want))
    assert len(out) == len(want)
    for (w, (n_lin, status, last)), o in zip(want.items(), out):
        got = (int(o[0]), int(o[1]), float.fromhex(o[2]))
        assert got == (n_lin, status, last) and np.copysign(1.0, got[2]) == 1.0, (w, o)


def test_the_stop_rule_and_all_five_statuses(iterate_host):
    h = lambda v: float(v).hex()  # noqa: E731
    nan = float("nan")
    runs = [
        # (max_lin, tol, masked, [(failed, last_step, stalled) ...])  ->  n_lin, status, last_step, cur
        ((1, 0.0, 0, []), (1, 1, 0.0, 0)),                                            # one linearisation: nothing is solved
        ((4, 1e-3, 0, [(0, 0.5, 0), (0, 1e-2, 0), (0, 1e-3, 0)]), (3, 0, 1e-3, 0)),   # converged: last_step <= tol, the rows of k = 2 stay
        ((4, 1e-3, 0, [(0, 0.5, 0), (0, 9e-4, 0)]), (2, 0, 9e-4, 1)),                 # ... one earlier, not one later
        ((4, 1e-3, 0, [(0, 0.5, 0), (0, 0.4, 0), (0, 0.3, 0)]), (4, 1, 0.3, 1)),      # ran out
        ((4, 0.0, 0, [(0, 0.5, 0), (0, 0.0, 0), (0, 0.0, 0)]), (4, 1, 0.0, 1)),       # tol = 0 never stops early
        ((4, 1e-3, 0, [(0, 0.5, 0), (0, 0.4, 1)]), (2, 2, 0.4, 1)),                   # stalled at the second trial point: the buffer stays
        ((4, 1e-3, 0, [(0, 0.5, 1)]), (1, 2, 0.5, 0)),
        ((4, 1e-3, 0, [(0, 0.5, 0), (1, 0.1, 0)]), (2, 3, nan, 1)),                   # the solve failed
        ((4, 1e-3, 0, [(0, float("inf"), 0)]), (1, 3, nan, 0)),                       # ... or gave a step that is not finite
        ((4, 1e-3, 0, [(0, nan, 0)]), (1, 3, nan, 0)),
        ((4, 1e-3, 1, [(0, 0.5, 0)]), (0, 4, 0.0, 0)),                                # masked out
        ((16, 1e-3, 0, [(0, 0.5, 0)] * 15), (16, 1, 0.5, 1)),
    ]
    lines = [f"run {m} {h(t)} {mk} " + " ".join(f"{f} {h(s)} {st}" for f, s, st in seq) for (m, t, mk, seq), _ in runs]
    out = iterate_host("\n".join(lines))
    for ((m, t, mk, seq), want), o in zip(runs, out):
        got = (int(o[0]), int(o[1]), float.fromhex(o[2]), int(o[3]))
        assert got[:2] == want[:2] and got[3] == want[3], (m, t, mk, seq, got)
        assert (np.isnan(got[2]) and np.isnan(want[2])) or got[2] == want[2], (seq, got)
