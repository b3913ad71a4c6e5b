"""What the innovation lift of the non-vision calls needs on the host, without a GPU: the binding's symbol with its argument types (no handle
is created) and the decisions and layouts of eqf_vio_amd/csrc/eqf_lift_host.hpp (host only, standard library only) --
tests/lift_host_main.cpp is compiled with g++ under the address and undefined-behaviour sanitizers and run as a child process, cases on
stdin, results on stdout.  Every expected value is computed here."""
import ctypes as C
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_binding_exports_the_getter_with_its_argument_types():
    from eqf_vio_amd import binding

    assert "eqf_get_lift_report" in binding.EXPORTED_SYMBOLS
    L = binding.lib()
    assert L.eqf_get_lift_report.argtypes == [C.c_void_p, C.c_int, C.POINTER(binding.LiftReport)]
    assert callable(binding.FilterBatch.lift_report)
    assert [f[0] for f in binding.LiftReport._fields_] == ["kind", "info", "DeltaU", "min_pivot", "pivot_ratio"]
    assert C.sizeof(binding.LiftReport) == 8 + 8 * 8
    # a NULL handle is refused by the library itself, before anything touches a device
    assert L.eqf_get_lift_report(None, 0, None) == binding.ERR_INVALID
    assert L.eqf_set_option(None, b"innovation_lift", 1) == binding.ERR_INVALID


@pytest.fixture(scope="module")
def lift_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lift_host") / "lift_host")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "eqf_vio_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "lift_host_main.cpp")], check=True)

    def run(text, conv=int):
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        return [[conv(t) for t in ln.split()] for ln in r.stdout.split("\n")[:-1]]

    return run


def test_header_is_host_only_and_compiles_with_plain_gcc(tmp_path):
    path = os.path.join(ROOT, "eqf_vio_amd", "csrc", "eqf_lift_host.hpp")
    includes = [ln.split()[1] for ln in open(path) if ln.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "eqf_lift_host.hpp"\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.dirname(path), str(tu)], check=True)


def test_which_lift_a_call_and_a_filter_take(lift_host):
    cases = [(o, l, d, N, nMax) for o in (-1, 0, 1, 2) for l in (0, 1) for d in (0, 1) for N, nMax in ((0, 0), (1, 1), (1, 20), (2, 2), (41, 41))]
    out = lift_host("\n".join("kind %d %d %d %d %d" % c for c in cases))
    for (o, l, d, N, nMax), got in zip(cases, out):
        call = 0 if (o == 0 or not l) else (2 if d else 1)   # (an option the setter refuses never gets here; any non-zero value reads as on)
        want = [int(o in (0, 1)), call, call if N >= 2 else 0, int(call != 0 and nMax >= 2)]
        assert got == want, ((o, l, d, N, nMax), got, want)


def test_orders_pitches_and_grids(lift_host):
    cases = [(N, nMax) for N, nMax in ((0, 0), (1, 1), (2, 2), (3, 20), (19, 19), (20, 20), (41, 41), (85, 85), (85, 200))]
    out = lift_host("\n".join("shape %d %d" % c for c in cases))
    for (N, nMax), got in zip(cases, out):
        assert got == [6 + 3 * N, 6 + 3 * nMax, -(-(6 + 3 * nMax) // 64), -(-nMax // 4), 6 + 3 * (N - 1) + 2 if N else -1], (N, nMax)
    # the sizes of lift_cases.py sit on both sides of one, two and three block columns and past 256
    assert [o[0] for o in lift_host("\n".join("shape %d %d" % (N, N) for N in (2, 3, 19, 20, 41, 85)))] == [12, 15, 63, 66, 129, 261]


def test_right_hand_side_layout(lift_host):
    for N, extra in ((0, 0), (1, 0), (2, 3), (19, 0), (20, 5)):
        out = lift_host(f"pack {N} {extra}")
        m = 6 + 3 * N
        assert len(out) == 7 and all(len(r) == m + extra for r in out)
        for r, row in enumerate(out):
            assert row[:6] == [0] * 6 and row[m:] == [-9] * extra            # five zero rows of Z_P, the pad; beyond the order: untouched
            for i in range(N):
                for c in range(3):
                    want = 100 * (3 * i + c) + r + 1 if r < 6 else -(3 * i + c + 1)
                    assert row[6 + 3 * i + c] == want, (N, r, i, c)


def test_report_and_info_merge(lift_host):
    assert lift_host("report 2 4") == [[2, 4, 1, 2, 3, 4, 5, 6, 7, 8]]
    words = (-1, 0, 1, 2, 3, 4, 5)
    out = lift_host("\n".join(f"merge {w}" for w in words))
    # 5, the word a failed lift leaves, reads as info = 4; 4 is the block update's idle word and passes as it is (its caller maps it)
    assert out == [[-1, 0], [0, 1], [1, 0], [2, 1], [3, 0], [4, 0], [4, 1]]


def test_update_report_for_every_verdict_word(lift_host):
    """What eqf_linear_report says for each verdict word of an update's record {nis 10.5, logdet_S -2.25, loglik 3.125, word}: written out
    here, for the block route (it has the idle word; dof is rows times the entries that took part, which its caller hands in) and for the
    linear route (no idle word; dof = m)."""
    nan, val = float("nan"), (10.5, -2.25, 3.125)
    cases = [
        # (word, dof handed in, route has the idle word) -> nis, logdet_S, loglik, dof, info
        ((0, 6, 1), (*val, 6, 0)),            # applied
        ((1, 6, 1), (nan, nan, nan, 6, 1)),   # S not positive definite / a non-finite value: untouched
        ((2, 6, 1), (*val, 6, 2)),            # gated: the statistics are what was compared
        ((3, 0, 1), (nan, nan, nan, 0, 3)),   # masked out
        ((4, 0, 1), (0.0, 0.0, 0.0, 0, 0)),   # blocks::kInfoIdle: no entry takes part -- an applied update of no rows
        ((5, 6, 1), (*val, 6, 4)),            # lift::kWordFailed: the update solved, the lift refused the filter
        ((-1, 6, 1), (nan, nan, nan, 6, -1)),  # local = 1 and a singular gravity chart
        ((0, 3, 0), (*val, 3, 0)),
        ((1, 3, 0), (nan, nan, nan, 3, 1)),
        ((2, 3, 0), (*val, 3, 2)),
        ((3, 3, 0), (nan, nan, nan, 3, 3)),
        ((4, 3, 0), (nan, nan, nan, 3, 4)),   # the linear route has no idle word: 4 passes like any word that did not solve
        ((5, 3, 0), (*val, 3, 4)),
        ((-1, 3, 0), (nan, nan, nan, 3, -1)),
    ]
    out = lift_host("\n".join("update %d %d %d" % c for c, _ in cases), conv=str)
    assert len(out) == len(cases)
    for (c, want), o in zip(cases, out):
        got = [float.fromhex(t) for t in o[:3]]
        for g, w in zip(got, want[:3]):
            assert (math.isnan(g) and math.isnan(w)) or (g == w and math.copysign(1.0, g) == math.copysign(1.0, w)), (c, o)
        assert (int(o[3]), int(o[4])) == want[3:], (c, o)
