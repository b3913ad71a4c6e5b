"""What eqf_score_vision needs on the host, without a GPU: the binding's symbol with its argument types (no handle is created), the numpy
statement and the compatibility test on examples worked by hand, the C++ facade's new member (compiled and linked), and the argument
checks, id matching, chunk plan and record arithmetic of eqf_vio_amd/csrc/eqf_score_host.hpp (host only, standard library only) --
tests/score_host_main.cpp is compiled with g++ under the address and undefined-behaviour sanitizers and run as a child process, cases on
stdin, results on stdout.  Every expected value is computed here."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, CAPACITY, UNSORTED = 0, -1, -4, -5


def test_binding_exports_the_symbol_with_its_argument_types():
    from eqf_vio_amd import binding

    L = binding.lib()
    dp, ip, vp, up = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p, C.POINTER(C.c_ubyte)
    assert "eqf_score_vision" in binding.EXPORTED_SYMBOLS
    assert L.eqf_score_vision.argtypes == [vp, C.c_int, ip, ip, dp, C.c_int, up, C.POINTER(binding.FrameScore), dp, up]
    assert C.sizeof(binding.FrameScore) == 32
    assert [f[0] for f in binding.FrameScore._fields_] == ["nis", "logdet_S", "loglik", "dof", "info"]
    assert callable(binding.FilterBatch.score_vision)
    # a NULL handle is refused by the library itself, before anything touches a device
    assert L.eqf_score_vision(None, 1, None, None, None, 1, None, None, None, None) == binding.ERR_INVALID


@pytest.fixture(scope="module")
def score_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("score_host") / "score_host")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "eqf_vio_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "score_host_main.cpp")], check=True)

    def run(text):
        r = subprocess.run([exe], input=text + "\n", capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        return [ln.split() for ln in r.stdout.split("\n")[:-1]]

    return run


def test_header_is_host_only_and_compiles_with_plain_gcc(tmp_path):
    path = os.path.join(ROOT, "eqf_vio_amd", "csrc", "eqf_score_host.hpp")
    includes = [ln.split()[1] for ln in open(path) if ln.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "eqf_score_host.hpp"\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.dirname(path), str(tu)], check=True)


def _check_line(B, cap, ncand, stride, nb, ids, y, mask=None):
    items = B * ncand
    idm = np.zeros((items, max(stride, 0)), dtype=int)
    ym = np.tile(np.array([0.0, 0.0, 1.0]), (items, max(stride, 0), 1))
    for k in range(items):
        n = len(ids[k])
        idm[k, :n] = ids[k]
        if y is not None and k in y:
            ym[k, :len(y[k])] = y[k]
    parts = [B, cap, ncand, stride, 0 if mask is None else 1] + ([] if mask is None else list(mask)) + list(nb) + list(idm.reshape(-1))
    return "check " + " ".join(str(p) for p in parts) + " " + " ".join(float(v).hex() for v in ym.reshape(-1))


def test_argument_checks(score_host):
    nan, inf = float("nan"), float("inf")
    cases = [
        (_check_line(2, 10, 2, 3, [3, 0, 1, 2], [[1, 2, 3], [], [7], [4, 9]], None), OK),
        (_check_line(1, 10, 1, 3, [0], [[]], None), OK),                                            # an empty candidate
        (_check_line(1, 10, 0, 3, [], [], None), INVALID),                                          # ncand < 1
        (_check_line(1, 10, 1, 0, [0], [[]], None), INVALID),                                       # stride < 1
        (_check_line(1, 10, 1, 3, [-1], [[]], None), INVALID), (_check_line(1, 10, 1, 3, [4], [[1, 2, 3]], None), INVALID),   # nb outside [0, stride]
        (_check_line(1, 2, 1, 3, [3], [[1, 2, 3]], None), CAPACITY),                                # nb beyond the capacity
        (_check_line(1, 10, 1, 3, [3], [[1, 3, 2]], None), UNSORTED), (_check_line(1, 10, 1, 3, [3], [[1, 2, 2]], None), UNSORTED),   # a duplicate is refused
        (_check_line(1, 10, 2, 3, [1, 3], [[5], [3, 2, 1]], None), UNSORTED),                       # in the second candidate
        (_check_line(1, 10, 1, 3, [2], [[1, 3, 2]], None), OK),                                     # behind nb nothing is looked at
        (_check_line(1, 10, 1, 3, [2], [[1, 2]], {0: [[0, 0, 1], [0, nan, 1]]}), INVALID),
        (_check_line(1, 10, 1, 3, [2], [[1, 2]], {0: [[0, 0, 1], [inf, 0, 1]]}), INVALID),
        (_check_line(1, 10, 1, 3, [1], [[1, 2]], {0: [[0, 0, 1], [inf, 0, 1]]}), OK),               # ... nor behind nb here
        (_check_line(2, 10, 1, 3, [3, 2], [[3, 2, 1], [1, 2]], {0: [[nan, 0, 1]]}, mask=[0, 1]), OK),      # a masked filter's lists are not read
        (_check_line(2, 10, 1, 3, [3, 2], [[3, 2, 1], [1, 2]], None, mask=[1, 0]), UNSORTED),
        (_check_line(2, 10, 1, 3, [4, 2], [[], [1, 2]], None, mask=[0, 1]), INVALID),               # ... but its nb is
        (_check_line(2, 2, 1, 3, [3, 2], [[1, 2, 3], [1, 2]], None, mask=[0, 1]), CAPACITY),
    ]
    got = score_host("\n".join(c for c, _ in cases))
    assert [int(g[0]) for g in got] == [w for _, w in cases], [(k, g) for k, ((c, w), g) in enumerate(zip(cases, got)) if int(g[0]) != w]
    got = score_host("\n".join(f"option {v}" for v in (0, 1, 4096, 4097, -1)))
    assert [int(g[0]) for g in got] == [0, 1, 1, 0, 0]


def _match(state, ids):
    want = [(s, ids.index(i)) for s, i in enumerate(state) if i in ids]
    return [len(want)] + [s for s, _ in want] + [p for _, p in want]


def test_matching_is_in_state_order(score_host):
    cases = [([], []), ([], [1, 2]), ([4, 5, 6], []),
             ([10, 11, 12], [1, 2, 3]), ([10, 11, 12], [20, 30]),                  # ids below and above the state's range
             ([10, 11, 12], [5, 11, 40]), ([10, 11, 12], [10, 11, 12]), ([10, 11, 12], [12]), ([10, 11, 12], [10]),
             ([7, 3, 9, 1, 8], [1, 3, 7, 8, 9]),                                   # a state whose ids are not ascending: slots ascend, positions do not
             ([7, 3, 9, 1, 8], [2, 3, 4, 8, 10]), ([50, 2, 40, 3], [3, 50]),
             (list(range(100, 0, -1)), list(range(1, 101, 3))), ([5], [5]), ([5], [4]), ([5], [6]), ([-3, 0, 2], [-3, 2])]
    got = score_host("\n".join(f"match {len(s)} " + " ".join(map(str, s)) + f" {len(i)} " + " ".join(map(str, i)) for s, i in cases))
    for (s, i), g in zip(cases, got):
        assert "BROKEN" not in g and [int(x) for x in g] == _match(s, i), (s, i, g)
    slots = [int(x) for x in got[9][1:6]]
    pos = [int(x) for x in got[9][6:11]]
    assert slots == [0, 1, 2, 3, 4] and pos == [2, 1, 4, 0, 3]


def test_chunk_plan_and_launch_count(score_host):
    for items, option, B in ((15, 0, 3), (15, 2, 3), (15, 1, 3), (1, 1, 64), (256, 0, 64), (7, 4096, 2), (6, 4, 9)):
        got = [int(x) for x in score_host(f"plan {items} {option} {B}")[0]]
        chunk = option if option > 0 else B
        counts = [min(chunk, items - c * chunk) for c in range(-(-items // chunk))]
        assert got == [chunk, len(counts)] + counts and sum(counts) == items
    for cap, m in ((1, 2), (31, 62), (32, 64), (33, 66), (64, 128), (65, 130), (100, 194), (1000, 2000), (100, 0)):
        nb = -(-m // 64)
        launches = 3 + sum((1 if K > 0 else 0) + 1 + (1 if nb - K - 1 > 0 else 0) for K in range(nb))
        assert [int(x) for x in score_host(f"order {cap} {m}")[0]] == [64 * -(-2 * cap // 64), nb, launches]
        assert 64 * -(-2 * cap // 64) >= 2 * cap


def _ascending_parts(offs, sizes, total):
    """Parts [off, off + size) in the order given start at 0, do not overlap and end within the total."""
    ends = [o + s for o, s in zip(offs, sizes)]
    return offs[0] == 0 and all(e <= o for e, o in zip(ends, offs[1:])) and ends[-1] <= total


def test_workspace_and_table_layouts(score_host):
    """W | E | D | bad in doubles and rec | nisLm | y | items | slots in bytes, against the formulas written out; the totals are what the
    call has always allocated: C (ldW^2 + ldW + dRec) + (C + 1) // 2 doubles, and the sum of the five tables."""
    dRec = 5120
    works = [(C, cap) for C in (1, 2, 3, 8) for cap in (1, 5, 21, 200)]
    for (C, cap), got in zip(works, score_host("\n".join(f"work {C} {64 * -(-2 * cap // 64)} {dRec}" for C, cap in works))):
        got = [int(x) for x in got]
        ldW = 64 * -(-2 * cap // 64)
        sizes = [C * ldW * ldW, C * ldW, C * dRec]
        total = C * (ldW * ldW + ldW + dRec) + (C + 1) // 2
        assert got == [0, sizes[0], sizes[0] + sizes[1], sum(sizes), total], (C, cap)
        assert _ascending_parts([8 * o for o in got[:4]], [8 * s for s in sizes] + [4 * C], 8 * total)
        assert (8 * got[3]) % 4 == 0 and 8 * (total - got[3]) >= 4 * C  # (C ints fit, C odd or even)
    tabs = [(i, m) for i in (0, 1, 7) for m in (0, 1, 7)]
    for (nItems, nMatched), got in zip(tabs, score_host("\n".join(f"tab {i} {m}" for i, m in tabs))):
        got = [int(x) for x in got]
        item = got[6]
        assert item == 16  # (four ints: the device's ScoreItem)
        sizes = [8 * 8 * nItems, 8 * nMatched, 8 * 3 * nMatched, item * nItems, 4 * nMatched]
        want, at = [], 0
        for s in sizes:
            want.append(at)
            at += s
        assert got[:6] == want + [at], (nItems, nMatched)
        assert _ascending_parts(got[:5], sizes, got[5])
        assert all(o % 8 == 0 for o in got[:4]) and got[4] % 4 == 0  # (doubles and items on 8 bytes, the int slots on 4)


def test_record_arithmetic(score_host):
    rng = np.random.default_rng(11)
    lines, want = [], []
    for k in range(30):
        nis, ld, dof = rng.uniform(0, 400), rng.normal(0, 900), 2 * int(rng.integers(1, 120))
        lines.append(f"rec {float(nis).hex()} {float(ld).hex()} {dof} 0")
        want.append((nis, ld, -0.5 * (nis + ld + dof * math.log(2 * math.pi)), dof))
    for g, (nis, ld, ll, dof) in zip(score_host("\n".join(lines)), want):
        assert float.fromhex(g[0]) == nis and float.fromhex(g[1]) == ld and int(g[3]) == dof and int(g[4]) == 0
        assert abs(float.fromhex(g[2]) - ll) <= 4 * np.finfo(float).eps * max(abs(ll), 1.0)  # (a compiler may fuse a multiply-add)
        assert [float.fromhex(x) for x in g[5:]] == [0.0, 0.0, 0.0]
    # trouble: a bad pivot or a value that is not finite -> info 1, NaN fields, dof kept
    for line in ("rec 0x1p+0 0x1p+0 4 1", "rec nan 0x1p+0 4 0", "rec 0x1p+0 inf 4 0", "rec 0x1p+0 -inf 4 0", "rec inf 0x1p+0 4 0"):
        g = score_host(line)[0]
        assert all(math.isnan(float.fromhex(x)) if x not in ("nan", "-nan") else True for x in g[:3]) and int(g[3]) == 4 and int(g[4]) == 1, (line, g)
    # an empty measurement: every field exactly +0
    g = score_host("rec 0x0p+0 0x0p+0 0 0")[0]
    assert [math.copysign(1.0, float.fromhex(x)) for x in g[:3]] == [1.0, 1.0, 1.0] and [float.fromhex(x) for x in g[:3]] == [0.0, 0.0, 0.0]
    assert int(g[3]) == 0 and int(g[4]) == 0


def test_numpy_statement_worked_by_hand():
    """Three landmarks with C_i = [I2 0] scaled, Sigma block diagonal plus one coupling: S and its factor by hand."""
    from eqf_vio_amd import consistency as cs

    N, r = 3, 0.25
    Sg = np.eye(11 + 3 * N)
    for i, v in enumerate((1.0, 4.0, 9.0)):
        Sg[11 + 3 * i:14 + 3 * i, 11 + 3 * i:14 + 3 * i] = v * np.eye(3)
    Cb = np.array([np.eye(2, 3) * c for c in (1.0, 0.5, 2.0)])
    delta = np.array([[0.5, -0.5], [100.0, 100.0], [1.0, 2.0]])
    out = cs.score_vision_host(Sg, Cb, delta, r, [0, 2])   # landmark 1 is not part of the measurement: its wild residual must not count
    s0, s2 = 1.0 + r, 4.0 * 9.0 + r
    nis = (0.25 + 0.25) / s0 + (1.0 + 4.0) / s2
    ld = 2 * math.log(s0) + 2 * math.log(s2)
    assert out["dof"] == 4 and abs(out["nis"] - nis) < 1e-14 and abs(out["logdet_S"] - ld) < 1e-13
    assert abs(out["loglik"] + 0.5 * (nis + ld + 4 * math.log(2 * math.pi))) < 1e-13
    assert np.allclose(out["nis_lm"], [0.5 / s0, 5.0 / s2], rtol=1e-15) and abs(out["nis_lm"].sum() - out["nis"]) < 1e-14
    # a coupling between landmarks 0 and 2, in the LOWER triangle only (the upper is garbage the statement must not read)
    Sg[17, 11] = 0.75
    Sg[11, 17] = 1e6
    out = cs.score_vision_host(Sg, Cb, delta, r, [0, 2])
    S = np.diag([s0, s0, s2, s2])
    S[2, 0] = S[0, 2] = 2.0 * 0.75 * 1.0
    d = np.array([0.5, -0.5, 1.0, 2.0])
    assert np.array_equal(out["S"], S) and abs(out["nis"] - d @ np.linalg.solve(S, d)) < 1e-14
    assert abs(out["logdet_S"] - np.linalg.slogdet(S)[1]) < 1e-13
    empty = cs.score_vision_host(Sg, Cb, delta, r, [])
    assert empty["dof"] == 0 and empty["nis"] == 0.0 and empty["logdet_S"] == 0.0 and empty["loglik"] == 0.0
    with pytest.raises(ValueError):
        cs.score_vision_host(Sg, Cb, delta, r, [2, 0])
    # the compatibility test: the chi-square quantile at the record's own dof, and True for an empty record
    assert cs.joint_compatible(dict(nis=5.9, dof=2), 0.95) and not cs.joint_compatible(dict(nis=6.0, dof=2), 0.95)
    got = cs.joint_compatible(dict(nis=np.array([0.0, 9.4, 9.6, np.nan]), dof=np.array([0, 4, 4, 4])), 0.95)   # chi2(4) at 0.95: 9.488
    assert list(got) == [True, True, False, False]


def test_facade_member_compiles_and_links(tmp_path):
    """cpp/VIOFilter.h with scoreVisionData: compiled for the host and linked against the library (nothing is run: no device here)."""
    lib = os.path.join(ROOT, "eqf_vio_amd", "libeqf_vio_amd.so")
    assert os.path.exists(lib)
    tu = tmp_path / "facade.cpp"
    tu.write_text('#include "VIOFilter.h"\nusing namespace eqf_vio_amd;\n'
                  "int main(int argc, char**) {\n"
                  "    if (argc < 100) return 0;  // (never constructed here: a handle needs a device)\n"
                  "    VIOFilter::Settings s;\n"
                  "    VIOFilter f(s);\n"
                  "    VisionMeasurement m;\n"
                  "    const eqf_frame_score r = f.scoreVisionData(m);\n"
                  "    return r.info + r.dof + int(r.nis + r.logdet_S + r.loglik);\n"
                  "}\n")
    exe = str(tmp_path / "facade")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "eqf_vio_amd", "cpp"), "-I", os.path.join(ROOT, "include"), "-o", exe,
                    str(tu), lib, "-Wl,-rpath," + os.path.dirname(lib), "-Wl,--allow-shlib-undefined"], check=True)
    assert os.path.exists(exe)
