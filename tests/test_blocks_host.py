"""What the per-landmark block measurement update needs on the host, without a GPU: the binding's symbol with its argument types (no handle
is created), and the per-entry arithmetic, index arithmetic and argument checks of eqf_vio_amd/csrc/eqf_blocks_host.hpp (host-compilable,
standard library only; the kernels of csrc/eqf_blocks.hpp call the same functions) -- tests/blocks_host_main.cpp is compiled with g++ under
the address and undefined-behaviour sanitizers and run as a child process, cases on stdin as hex floats, results on stdout.  The per-entry
results are held to the longdouble reference of tests/blocks_exact.py on every entry of every committed case of tests/blocks_cases.py; every
other expected value is computed here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import blocks_cases as bc
import blocks_exact as bx
import consistency_exact as cx
from eqf_vio_amd import consistency as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def test_binding_exports_the_symbol_with_its_argument_types():
    from eqf_vio_amd import binding
    from eqf_vio_amd import filter as vf

    assert "eqf_update_landmarks" in binding.EXPORTED_SYMBOLS
    L = binding.lib()
    dp, ip, up, vp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_ubyte), C.c_void_p
    assert L.eqf_update_landmarks.argtypes == [vp, C.c_int, C.c_int, ip, ip, C.c_int, dp, dp, dp, C.c_double, C.c_double, up, up, dp, C.c_int,
                                               C.POINTER(binding.LinearReport)]
    assert callable(binding.FilterBatch.update_landmarks) and callable(vf.VIOFilter.processLandmarkMeasurements)
    # a NULL handle is refused by the library itself, before anything touches a device
    one, d = (C.c_int * 1)(1), (C.c_double * 9)()
    assert L.eqf_update_landmarks(None, 1, 1, one, one, 1, d, d, d, 1.0, 1.0, None, None, None, 0, None) == binding.ERR_INVALID
    header = open(os.path.join(ROOT, "include", "eqf_vio_amd.h")).read()
    assert "int eqf_update_landmarks(eqf_filter* f, int local, int rows," in header


@pytest.fixture(scope="module")
def blocks_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("blocks_host") / "blocks_host")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "eqf_vio_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "blocks_host_main.cpp")], check=True)

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        return [ln.split() for ln in r.stdout.split("\n")[:-1]]

    return run


def _hx(a):
    return " ".join(float(v).hex() for v in np.asarray(a, dtype=float).reshape(-1))


def test_header_is_host_only_and_compiles_with_plain_gcc(tmp_path):
    path = os.path.join(ROOT, "eqf_vio_amd", "csrc", "eqf_blocks_host.hpp")
    includes = [ln.split()[1] for ln in open(path) if ln.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "eqf_blocks_host.hpp"\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.dirname(path), str(tu)], check=True)


def test_per_entry_arithmetic_against_the_exact_reference(blocks_host):
    """Ht inside blocks_exact's dHt (K_BLOCKS times the unit form), d2 inside 64 u cond(S_kk) d2 (a 3 x 3 Cholesky and two substitutions:
    [Higham, Thm 10.3, 8.5] give a few u cond; cond(S_kk) <= 1e6 is asserted), the verdict exact"""
    own = {N: bc.own_sigma_oracle(N) for N in sorted({c[0] for c in bc.CASES.values() if c[5] == "own"})}
    worst_h, worst_d = 0.0, 0.0
    for name in bc.CPU_CASES:
        N = bc.CASES[name][0]
        snap = bc.snapshot(name, own.get(N))
        ops = bc.operands(name, snap)
        ops["R"] = bc.poison(ops["R"])
        Jmp = cx.jacobian_mp(snap["origin"], snap["group"])
        ref = bx.reference(snap["sigma"], ops, Jmp)
        Ht_ref, dHt = bx.entry_rows(ops, Jmp, N)
        J = np.asarray(cs.local_jacobian_blocks(snap["origin"], snap["group"])["lm"]).reshape(-1, 3, 3)
        rows, K = ops["rows"], len(ops["idx"])
        lines = []
        for k in range(K):
            i = max(int(ops["idx"][k]), 0)
            Sii = snap["sigma"][11 + 3 * i:14 + 3 * i, 11 + 3 * i:14 + 3 * i]
            Sii = np.tril(Sii) + 7.0 * np.triu(np.ones((3, 3)), 1)  # (the upper triangle is poison: only the lower may be read)
            lines.append(f"entry {rows} {ops['local']} {float(ops['lm_gate']).hex()} {int(ops['idx'][k])} {_hx(ops['H'][k])} {_hx(J[i])} {_hx(Sii)} "
                         f"{_hx(ops['R'][k])} {_hx(ops['resid'][k])}")
        out = blocks_host("\n".join(lines))
        assert len(out) == K
        for k in range(K):
            v = [float.fromhex(t) for t in out[k][:-1]]
            verdict = int(out[k][-1])
            assert verdict == ref["used"][k], (name, k)
            if ops["idx"][k] < 0:
                continue
            Ht, d2 = np.array(v[:3 * rows]).reshape(rows, 3), v[3 * rows]
            err = np.abs(Ht.astype(bx.LD) - Ht_ref[k]).astype(float)
            bound = bx.K_BLOCKS * dHt[k]
            assert np.all(err[bound == 0] == 0), (name, k)
            worst_h = max(worst_h, float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0)
            i = int(ops["idx"][k])
            Skk = np.asarray(Ht_ref[k], dtype=float) @ bx.mirror_lower(snap["sigma"])[11 + 3 * i:14 + 3 * i, 11 + 3 * i:14 + 3 * i] @ np.asarray(
                Ht_ref[k], dtype=float).T + bx.mirror_lower(ops["R"][k])
            cond = float(np.linalg.cond(Skk))
            assert cond <= 1e6, (name, k, cond)
            worst_d = max(worst_d, abs(d2 - ref["d2"][k]) / (64 * U * cond * ref["d2"][k]))
    print(f"eqf_blocks_host.hpp against the reference: worst Ht / bound {worst_h:.3f}, worst d2 / bound {worst_d:.3f}")
    assert worst_h <= 1.0 and worst_d <= 1.0


def test_d2_of_an_indefinite_block_is_nan_and_a_nan_stays_in(blocks_host):
    z9, e3 = _hx(np.zeros(9)), _hx(np.eye(3))
    out = blocks_host(f"entry 1 0 {float(5.0).hex()} 0 {_hx([1, 0, 0])} {z9} {e3} {_hx([-2.0])} {_hx([1.0])}\n"
                      f"entry 1 0 {float(5.0).hex()} -1 {_hx([1, 0, 0])} {z9} {e3} {_hx([1.0])} {_hx([1.0])}\n"
                      f"entry 1 0 {float(0.2).hex()} 3 {_hx([1, 0, 0])} {z9} {e3} {_hx([3.0])} {_hx([1.0])}\n"
                      f"entry 1 0 {float('inf').hex()} 3 {_hx([1, 0, 0])} {z9} {e3} {_hx([1.0])} {_hx([1e200])}")
    assert np.isnan(float.fromhex(out[0][3])) and int(out[0][4]) == 1   # S = 1 - 2 < 0: NaN, stays in (the joint factorisation reports it)
    assert int(out[1][4]) == 0                                           # id not in the state
    assert float.fromhex(out[2][3]) == 0.25 and int(out[2][4]) == 2     # d2 = 1 / (1 + 3) > 0.2: gated
    assert int(out[3][4]) == 1                                           # +inf disarms the gate


def test_compaction_layouts_and_grids(blocks_host):
    rng = np.random.default_rng(1920)
    lines, want = [], []
    for nk in (0, 1, 5, 64, 67):
        used = rng.integers(0, 3, nk)
        lines.append(f"compact {nk} " + " ".join(str(int(u)) for u in used))
        on = [k for k in range(nk) if used[k] == 1]
        pos = [on.index(k) if k in on else -1 for k in range(nk)]
        want.append([len(on)] + pos + on)
    for B, stride, rows, ld, drec in ((1, 1, 1, 24, 5120), (3, 33, 2, 160, 5120), (2, 45, 3, 280, 5120)):
        lines.append(f"layout {B} {stride} {rows} {ld} {drec}")
        e = B * stride
        oR = 8 * e * rows * 3 + 8 * e * rows
        oI = oR + 8 * e * rows * rows
        mp = -(-rows * stride // 64) * 64
        oHt = (mp + ld + 1) * mp
        want.append([0, 8 * e * rows * 3, oR, oI, oI + 4 * e, oI + 4 * e + 4 * B, oI + 4 * e + 5 * B, mp, mp // 64, 0, oHt, oHt + 9 * stride,
                     oHt + 9 * stride + ld, oHt + 9 * stride + ld + drec, 0, stride, 2 * stride, 3 * stride, 3 * stride + 1, 3 * stride + 4])
    for N, stride in ((0, 1), (4, 16), (17, 17), (43, 33), (86, 45)):
        lines.append(f"grid {N} {stride}")
        nt = -(-(12 + 3 * N) // 64)
        want.append([nt, nt * (nt + 1) // 2, -(-(13 + 3 * N) // 64), -(-stride // 16)])
    lines.append("find 4 12 10 11 12 13")
    want.append([2])
    lines.append("find 4 9 10 11 12 13")
    want.append([-1])
    out = blocks_host("\n".join(lines))
    assert [[int(t) for t in ln] for ln in out] == want
    src = np.arange(1.0, 19.0)
    out = blocks_host(f"gamma 2 0 {_hx(src)}\ngamma 2 1 {_hx(src)}")
    assert [float.fromhex(t) for t in out[0]] == list(src[:11]) + list(src[12:]) and [float.fromhex(t) for t in out[1]] == [0.0] * 17


def test_argument_checks(blocks_host):
    inf, nan = float("inf"), float("nan")
    head = lambda local, rows, stride, gate, lm, nul=0: f"head {local} {rows} {stride} {float(gate).hex()} {float(lm).hex()} {nul}"  # noqa: E731
    lines = [head(1, 2, 3, inf, inf), head(0, 1, 1, 5.0, 7.0), head(2, 2, 3, inf, inf), head(1, 0, 3, inf, inf), head(1, 4, 3, inf, inf),
             head(1, 2, 0, inf, inf), head(1, 2, 3, nan, inf), head(1, 2, 3, 0.0, inf), head(1, 2, 3, inf, nan), head(1, 2, 3, inf, -1.0)]
    lines += [head(1, 2, 3, inf, inf, 1 << k) for k in range(5)]
    out = blocks_host("\n".join(lines))
    assert [int(o[0]) for o in out] == [1, 1] + [0] * 13

    def args(rows=2, stride=3, B=2, cap=8, ldg=0, gamma=0, nk=(3, 2), N=(4, 2), mask=(1, 1), ids=(1, 2, 3, 5, 9, 0), bad=None):
        """bad = (b, k, what, value): one poisoned number"""
        parts = [f"args {rows} {stride} {B} {cap} {ldg} {gamma}", *map(str, nk), *map(str, N), *map(str, mask), *map(str, ids)]
        for b in range(B):
            for k in range(stride):
                H, r, R = np.ones((rows, 3)), np.ones(rows), np.eye(rows)
                if bad and bad[:2] == (b, k):
                    if bad[2] == "H":
                        H[rows - 1, 2] = bad[3]
                    elif bad[2] == "r":
                        r[rows - 1] = bad[3]
                    elif bad[2] == "R_lower":
                        R[rows - 1, 0] = bad[3]
                    else:
                        R[0, rows - 1] = bad[3]
                parts += [_hx(H), _hx(r), _hx(R)]
        return " ".join(parts)

    cases = [(args(), 0), (args(nk=(4, 2)), 1), (args(nk=(3, -1)), 1), (args(gamma=1, ldg=22), 1), (args(gamma=1, ldg=23), 0),
             (args(bad=(0, 2, "H", nan)), 1), (args(bad=(1, 1, "r", inf)), 1), (args(bad=(0, 0, "R_lower", nan)), 1),
             (args(bad=(0, 0, "R_upper", nan)), 0),          # the upper triangle is never read
             (args(bad=(1, 2, "H", nan)), 0),                # k >= nk[b]: not read
             (args(bad=(0, 2, "H", nan), mask=(0, 1)), 0),   # a masked filter: not read
             (args(ids=(1, 3, 3, 5, 9, 0)), 2), (args(ids=(1, 3, 2, 5, 9, 0)), 2), (args(ids=(1, 3, 3, 5, 9, 0), mask=(0, 1)), 0),
             (args(ids=(1, 2, 3, 9, 5, 0), nk=(3, 1)), 0),   # beyond nk[b]: not looked at
             (args(cap=2), 3), (args(cap=2, bad=(0, 0, "r", nan)), 1), (args(nk=(0, 0)), 0)]
    out = blocks_host("\n".join(c[0] for c in cases))
    assert [int(o[0]) for o in out] == [c[1] for c in cases]
