"""What eqf_observe_landmarks needs on the host, without a GPU: the binding's symbol with its argument types (no handle is created), and the
per-entry arithmetic, the layouts and the argument checks of eqf_vio_amd/csrc/eqf_observe_host.hpp (the kernel of csrc/eqf_observe.hpp
calls the same functions) -- tests/observe_host_main.cpp is compiled FOR THE HOST with g++ under the address and undefined-behaviour
sanitizers and run as a child process, cases on stdin as hex floats, results on stdout.  The per-entry results are held to the 50-digit
reference of tests/observe_exact.py inside K_OBS's bound on every entry of every committed case of tests/observe_cases.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import observe_cases as oc
import observe_exact as ox
from eqf_vio_amd import consistency as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_binding_exports_the_symbol_with_its_argument_types():
    from eqf_vio_amd import binding
    from eqf_vio_amd import filter as vf

    assert "eqf_observe_landmarks" in binding.EXPORTED_SYMBOLS
    L = binding.lib()
    dp, ip, up, vp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_ubyte), C.c_void_p
    assert L.eqf_observe_landmarks.argtypes == [vp, C.c_int, dp, C.c_int, ip, ip, C.c_int, dp, dp, C.c_double, C.c_double, up, ip, ip, C.c_int,
                                                up, dp, dp, dp, C.c_int, C.POINTER(binding.LinearReport)]
    assert callable(binding.FilterBatch.observe_landmarks) and callable(vf.VIOFilter.processLandmarkObservations)
    assert vf.VIOFilter.processLandmarkObservations is vf.VIOFilter.process_landmark_observations
    assert (binding.OBS_BEARING, binding.OBS_RANGE, binding.OBS_POSITION) == (cs.OBS_BEARING, cs.OBS_RANGE, cs.OBS_POSITION) == (0, 1, 2)
    # a NULL handle is refused by the library itself, before anything touches a device
    one, d = (C.c_int * 1)(1), (C.c_double * 9)()
    assert L.eqf_observe_landmarks(None, 0, None, 0, one, one, 1, d, d, 1.0, 1.0, None, None, None, 0, None, None, None, None, 0,
                                   None) == binding.ERR_INVALID
    header = open(os.path.join(ROOT, "include", "eqf_vio_amd.h")).read()
    assert "int eqf_observe_landmarks(eqf_filter* f, int kind, const double* cam" in header
    for name, v in (("EQF_OBS_BEARING", 0), ("EQF_OBS_RANGE", 1), ("EQF_OBS_POSITION", 2)):
        assert f"#define {name} {v}" in header
    cpp = open(os.path.join(ROOT, "eqf_vio_amd", "cpp", "VIOFilter.h")).read()
    assert cpp.count("eqf_linear_report processLandmarkObservations(") == 2


@pytest.fixture(scope="module")
def observe_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("observe_host") / "observe_host")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I",
                    os.path.join(ROOT, "eqf_vio_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "observe_host_main.cpp")], check=True)

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        return [ln.split() for ln in r.stdout.split("\n")[:-1]]

    return run


def _hx(a):
    return " ".join(float(v).hex() for v in np.asarray(a, dtype=float).reshape(-1))


ID_CAM = [1.0, 0, 0, 0, 0, 0, 0]


def _entry_line(kind, p0, q, a, cam, meas):
    return f"entry {kind} {_hx(p0)} {_hx(q)} {_hx([a])} {_hx(ID_CAM if cam is None else np.concatenate(cam))} {_hx(meas)}"


def test_per_entry_rows_against_the_exact_reference(observe_host):
    worst = 0.0
    for c in oc.CASES:
        kind, st, ids, meas, cam = oc.case(c)
        ref = ox.reference(kind, st, ids, meas, cam)
        rows, sid = ox.ROWS[kind], [int(i) for i in st["ids"]]
        K = len(ids)
        Ht, resid, used = np.zeros((K, rows, 3)), np.zeros((K, rows)), np.zeros(K, dtype=np.uint8)
        on = [k for k in range(K) if int(ids[k]) in sid]
        out = observe_host("\n".join(_entry_line(kind, st["origin"]["p"][sid.index(int(ids[k]))], st["group"]["Qq"][sid.index(int(ids[k]))],
                                                 st["group"]["Qa"][sid.index(int(ids[k]))], cam, meas[k]) for k in on))
        assert len(out) == len(on)
        for k, o in zip(on, out):
            v = [float.fromhex(t) for t in o[:-1]]
            Ht[k], resid[k], used[k] = np.array(v[:3 * rows]).reshape(rows, 3), v[3 * rows:], 3 if int(o[-1]) else 1
        rh, rr = ox.ratios(Ht, resid, used, ref)
        print(f"{c}: eqf_observe_host.hpp / bound: Ht {rh:.3f}, resid {rr:.3f}")
        worst = max(worst, rh, rr)
    assert worst <= 1.0


def test_not_observable_verdicts_and_an_exact_zero(observe_host):
    q1, y = [1.0, 0, 0, 0], [0.0, 0, 1]
    lines = []
    for kind in (0, 1, 2):
        lines += [_entry_line(kind, [0.0, 0, 0], q1, 1.0, None, y),          # d = 0
                  _entry_line(kind, [0.0, 0, 2], q1, 1.0, None, y),          # a bearing: y_hat at the chart's own pole
                  _entry_line(kind, [0.0, 0, -2], q1, 1.0, None, y),         # a bearing: y at the antipode of y_hat
                  _entry_line(kind, [np.inf, 0, 1], q1, 1.0, None, y),       # p0 not finite
                  _entry_line(kind, [np.nan, 0, 1], q1, 1.0, None, y),
                  _entry_line(kind, [0.1, 0, 0], q1, 1.0, ([1.0, 0, 0, 0], [0.1, 0, 0]), y)]  # the landmark in the second camera's centre
    out = observe_host("\n".join(lines))
    verdicts = [[int(o[-1]) for o in out[6 * k:6 * k + 6]] for k in range(3)]
    assert verdicts == [[1, 1, 1, 1, 1, 1], [1, 0, 0, 1, 1, 1], [1, 0, 0, 1, 1, 1]]
    for o in out:
        if int(o[-1]):
            assert all(float.fromhex(t) == 0.0 for t in o[:-1])
    # on the chart's axis with a power-of-two scale every stage is exact: the prediction's own bits give resid = 0 exactly
    out = observe_host("\n".join(_entry_line(kind, [0.0, 0, -6], q1, 4.0, None, m)
                                 for kind, m in ((0, [0.0, 0, -1]), (1, [1.5, 0, 0]), (2, [0.0, 0, -1.5]))))
    for kind, o in enumerate(out):
        rows = ox.ROWS[kind]
        assert int(o[-1]) == 0 and all(float.fromhex(t) == 0.0 for t in o[3 * rows:-1])
    # the quaternion of the offset is normalised: a scaled one gives the rows of the unit one to rounding
    cam = oc.camera("offset")
    a, b = observe_host(_entry_line(0, [0.3, -0.2, 2.0], q1, 1.0, cam, [0.1, 0, 0.99]) + "\n" +
                        _entry_line(0, [0.3, -0.2, 2.0], q1, 1.0, (3.0 * cam[0], cam[1]), [0.1, 0, 0.99]))
    assert np.allclose([float.fromhex(t) for t in a[:-1]], [float.fromhex(t) for t in b[:-1]], rtol=1e-14, atol=1e-16)


def test_layout_offsets(observe_host):
    lines, want = [], []
    for B, stride, rows in ((1, 1, 1), (3, 33, 2), (2, 45, 3)):
        lines.append(f"layout {B} {stride} {rows}")
        e = B * stride
        oM = 8 * 7 * B
        oR = oM + 8 * e * 3
        oI = oR + 8 * e * rows * rows
        want.append([0, oM, oR, oI, oI + 4 * e, oI + 4 * e + 4 * B, oI + 4 * e + 5 * B, 0, e * rows * 3, e * rows * 4])
    out = observe_host("\n".join(lines))
    assert [[int(t) for t in ln] for ln in out] == want


def test_argument_checks(observe_host):
    inf, nan = float("inf"), float("nan")
    head = lambda kind, campf, stride, gate, lm, nul=0: f"head {kind} {campf} {stride} {float(gate).hex()} {float(lm).hex()} {nul}"  # noqa: E731
    lines = [head(0, 0, 3, inf, inf), head(2, 1, 1, 5.0, 7.0), head(1, 0, 1, inf, 3.0), head(3, 0, 3, inf, inf), head(-1, 0, 3, inf, inf),
             head(0, 2, 3, inf, inf), head(0, -1, 3, inf, inf), head(0, 0, 0, inf, inf), head(0, 0, 3, nan, inf), head(0, 0, 3, 0.0, inf),
             head(0, 0, 3, inf, nan), head(0, 0, 3, inf, -1.0)]
    lines += [head(0, 0, 3, inf, inf, 1 << k) for k in range(4)]
    out = observe_host("\n".join(lines))
    assert [int(o[0]) for o in out] == [1, 1, 1] + [0] * 13

    def args(kind=0, cam_mode=0, stride=3, B=2, cap=8, ldg=0, gamma=0, nk=(3, 2), N=(4, 2), mask=(1, 1), ids=(1, 2, 3, 5, 9, 0), cam=None,
             bad=None):
        """bad = (b, k, what, value): one poisoned number"""
        rows = ox.ROWS[kind]
        parts = [f"args {kind} {cam_mode} {stride} {B} {cap} {ldg} {gamma}", *map(str, nk), *map(str, N), *map(str, mask), *map(str, ids)]
        if cam_mode:
            parts.append(_hx(cam if cam is not None else ID_CAM * (B if cam_mode == 2 else 1)))
        for b in range(B):
            for k in range(stride):
                m, R = np.ones(3), np.eye(rows)
                if bad and bad[:2] == (b, k):
                    if bad[2] in ("m0", "m1", "m2"):
                        m[int(bad[2][1])] = bad[3]
                    elif bad[2] == "R_lower":
                        R[rows - 1, 0] = bad[3]
                    else:
                        R[0, rows - 1] = bad[3]
                parts += [_hx(m), _hx(R)]
        return " ".join(parts)

    two = lambda c0, c1: list(c0) + list(c1)  # noqa: E731
    cases = [(args(), 0), (args(kind=1), 0), (args(kind=2), 0), (args(nk=(4, 2)), 1), (args(nk=(3, -1)), 1), (args(gamma=1, ldg=22), 1),
             (args(gamma=1, ldg=23), 0),
             (args(bad=(0, 2, "m2", nan)), 1), (args(kind=2, bad=(1, 1, "m0", inf)), 1), (args(kind=1, bad=(0, 0, "m0", nan)), 1),
             (args(kind=1, bad=(0, 0, "m1", nan)), 0), (args(kind=1, bad=(0, 0, "m2", inf)), 0),   # a range reads meas[0] only
             (args(bad=(0, 0, "R_lower", nan)), 1), (args(bad=(0, 0, "R_upper", nan)), 0),          # the upper triangle is never read
             (args(bad=(1, 2, "m0", nan)), 0),                                                      # k >= nk[b]: not read
             (args(bad=(0, 2, "m0", nan), mask=(0, 1)), 0),                                         # a masked filter: not read
             (args(cam_mode=1), 0), (args(cam_mode=1, cam=[0.0, 0, 0, 0, 1, 2, 3]), 1),             # a zero quaternion
             (args(cam_mode=1, cam=[1.0, 0, 0, nan, 1, 2, 3]), 1), (args(cam_mode=1, cam=[1.0, 0, 0, 0, 1, inf, 3]), 1),
             (args(cam_mode=1, cam=[0.0, 0, 2.0, 0, 1, 2, 3]), 0),                                  # not of unit length: fine
             (args(cam_mode=2), 0), (args(cam_mode=2, cam=two(ID_CAM, [0.0] * 7)), 1),
             (args(cam_mode=2, cam=two(ID_CAM, [0.0] * 7), mask=(1, 0)), 0),                        # a masked filter's offset: not read
             (args(cam_mode=2, cam=two([nan] * 7, ID_CAM), mask=(0, 1)), 0),
             (args(cam_mode=1, cam=[0.0] * 7, mask=(0, 0)), 1),                                     # the call's single offset is always read
             (args(ids=(1, 3, 3, 5, 9, 0)), 2), (args(ids=(1, 3, 2, 5, 9, 0)), 2), (args(ids=(1, 3, 3, 5, 9, 0), mask=(0, 1)), 0),
             (args(ids=(1, 2, 3, 9, 5, 0), nk=(3, 1)), 0),                                          # beyond nk[b]: not looked at
             (args(cap=2), 3), (args(cap=2, bad=(0, 0, "m0", nan)), 1), (args(nk=(0, 0)), 0)]
    out = observe_host("\n".join(c[0] for c in cases))
    assert [int(o[0]) for o in out] == [c[1] for c in cases]
