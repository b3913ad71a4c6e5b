"""What the low-rank linear measurement update needs on the host, without a GPU: the binding's symbol with its argument types (no handle is
created), the rows helpers of eqf_vio_amd/consistency.py, and the index arithmetic and argument checks of
eqf_vio_amd/csrc/eqf_linear_host.hpp (host only, standard library only) -- tests/linear_host_main.cpp is compiled with g++ under the address
and undefined-behaviour sanitizers and run as a child process, cases on stdin, results on stdout.  Every expected value is computed here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = (0, 1, 5, 17, 18, 39, 43, 82)


def test_binding_exports_the_symbol_with_its_argument_types():
    from eqf_vio_amd import binding

    assert "eqf_update_linear" in binding.EXPORTED_SYMBOLS
    L = binding.lib()
    dp, vp = C.POINTER(C.c_double), C.c_void_p
    assert L.eqf_update_linear.argtypes == [vp, C.c_int, C.c_int, dp, C.c_int, dp, dp, C.c_double, C.POINTER(C.c_ubyte), dp, C.c_int,
                                            C.POINTER(binding.LinearReport)]
    assert C.sizeof(binding.LinearReport) == 32 and [f[0] for f in binding.LinearReport._fields_] == ["nis", "logdet_S", "loglik", "dof", "info"]
    assert callable(binding.FilterBatch.update_linear)
    from eqf_vio_amd import filter as vf

    assert callable(vf.VIOFilter.process_linear_measurement)
    # a NULL handle is refused by the library itself, before anything touches a device
    assert L.eqf_update_linear(None, 1, 1, None, 0, None, None, 1.0, None, None, 0, None) == binding.ERR_INVALID
    assert binding.PROF_CLASSES == 15
    assert [L.eqf_profile_class_name(c).decode() for c in range(11, 15)] == ["k_lin_rows", "k_lin_gain", "k_lin_solve", "k_lin_downdate"]


def test_rows_helpers():
    from eqf_vio_amd import consistency as cs

    for N in (0, 1, 7):
        n = 11 + 3 * N
        e = np.arange(1.0, n + 1)
        assert np.array_equal(cs.velocity_rows(N) @ e, e[8:11]) and cs.velocity_rows(N).shape == (3, n)
        assert np.array_equal(cs.gravity_rows(N) @ e, e[6:8]) and cs.gravity_rows(N).shape == (2, n)
        for i in range(N):
            assert np.array_equal(cs.landmark_rows(N, i) @ e, e[11 + 3 * i:14 + 3 * i])
        with pytest.raises(ValueError):
            cs.landmark_rows(N, N)
    # the host statement on a two-state example worked by hand: Sigma = diag(4, 1), H = [1 0], R = 4, resid = 2
    out = cs.linear_update_host(np.diag([4.0, 1.0]), [[1.0, 0.0]], [2.0], [[4.0]])
    assert np.allclose(out["Sigma"], np.diag([2.0, 1.0])) and np.allclose(out["gamma"], [1.0, 0.0]) and np.isclose(out["nis"], 0.5)
    assert np.isclose(out["logdet_S"], np.log(8.0)) and out["dof"] == 1
    with pytest.raises(np.linalg.LinAlgError):
        cs.linear_update_host(np.eye(2), [[1.0, 0.0]], [0.0], [[-2.0]])


# ---- the header under the sanitizers
@pytest.fixture(scope="module")
def linear_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("linear_host") / "linear_host")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "eqf_vio_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "linear_host_main.cpp")], check=True)

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        return [[int(t) for t in ln.split()] for ln in r.stdout.split("\n")[:-1]]

    return run


def test_header_is_host_only_and_compiles_with_plain_gcc(tmp_path):
    path = os.path.join(ROOT, "eqf_vio_amd", "csrc", "eqf_linear_host.hpp")
    includes = [ln.split()[1] for ln in open(path) if ln.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "eqf_linear_host.hpp"\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.dirname(path), str(tu)], check=True)


def test_index_maps_and_grids(linear_host):
    out = iter(linear_host("\n".join(f"map {N}\ngrid {N}" for N in COUNTS)))
    for N in COUNTS:
        n = 11 + 3 * N
        assert next(out) == [i if i < 11 else i + 1 for i in range(n)], N
        assert next(out) == list(range(11)) + [-1] + list(range(11, n)), N
        nt = -(-(n + 1) // 64)
        assert next(out) == [n, n + 1, nt, nt * (nt + 1) // 2], N
        tiles = [v for I in range(nt) for J in range(I + 1) for v in (I, J)]
        assert next(out) == tiles, N
    assert [linear_host(f"grid {N}")[0][2] for N in (17, 18, 39, 43, 82)] == [1, 2, 3, 3, 5]  # (internal orders 63, 66, 129, 141, 258)


def test_layouts(linear_host):
    for B, cap, ld in ((1, 7, 48), (4, 77, 256), (64, 207, 640)):
        ldr = 11 + 3 * cap
        got = linear_host(f"layout {B} {cap} {ld}")[0]
        offs = [0, B * 16 * ldr, B * 16 * ldr + B * 16, B * 16 * ldr + B * 16 + B * 256]
        assert got[:4] == offs and got[4] == 8 * offs[3] + B
        assert got[5:] == [0, 16 * ld, 32 * ld, 48 * ld, 49 * ld]
        assert ld >= 12 + 3 * cap  # (what eqf_create guarantees: every row of the workspace holds a padded vector)


def test_pack_and_unpack(linear_host):
    cases = [(m, N, extra) for m in (1, 3, 15, 16) for N in (0, 1, 5, 18) for extra in (0, 4)]
    out = iter(linear_host("\n".join(f"pack {m} {N} {11 + 3 * N + extra} {11 + 3 * (N + 7)}" for m, N, extra in cases)))
    for m, N, extra in cases:
        n, ldr = 11 + 3 * N, 11 + 3 * (N + 7)
        H = np.zeros((16, ldr), dtype=int)
        for k in range(m):
            H[k, :n] = 100 * (k + 1) + np.arange(1, n + 1)
        assert next(out) == H.reshape(-1).tolist(), (m, N, extra)
        assert next(out) == [k + 1 if k < m else 0 for k in range(16)]
        R = np.eye(16, dtype=int)
        for k in range(m):
            for l in range(16):
                R[k, l] = 10 * (k + 1) + l + 1 if l <= k else 0
        assert next(out) == R.reshape(-1).tolist(), (m, N, extra)
    for N in (0, 1, 18):
        n = 11 + 3 * N
        g = linear_host(f"gamma {N} 0\ngamma {N} 1")
        assert g[0] == [j + 1 if j < 11 else j + 2 for j in range(n)] + [-7, -7]  # (the pad entry, 12, is skipped)
        assert g[1] == [0] * n + [-7, -7]


def test_argument_checks(linear_host):
    heads = [("1 1 1 1 1 0", 1), ("0 16 1 1 1 1", 1), ("2 3 1 1 1 0", 0), ("-1 3 1 1 1 0", 0), ("1 0 1 1 1 0", 0), ("1 17 1 1 1 0", 0),
             ("1 3 0 1 1 0", 0), ("1 3 1 0 1 0", 0), ("1 3 1 1 0 0", 0), ("1 3 1 1 1 2", 0), ("1 3 1 1 1 3", 0), ("1 3 1 1 1 4", 0)]
    text = ["head " + c for c, _ in heads]
    # args: m B ldh gamma? ldg mask?  N[B]  mask[B]  what b k i kind
    args = [("3 3 26 1 26 0  5 0 2  1 1 1  0 0 0 0 0", 1),
            ("3 3 25 1 26 0  5 0 2  1 1 1  0 0 0 0 0", 0),      # ldh too small for filter 0
            ("3 3 26 1 25 0  5 0 2  1 1 1  0 0 0 0 0", 0),      # ldg too small
            ("3 3 26 0 0 0   5 0 2  1 1 1  0 0 0 0 0", 1),      # no gamma: ldg is not looked at
            ("3 3 25 0 0 1   5 0 2  0 1 1  0 0 0 0 0", 0),      # a stride is checked for masked filters too
            ("3 3 26 1 26 0  5 0 2  1 1 1  1 0 2 25 1", 0),     # NaN in H, last entry of filter 0's own order
            ("3 3 26 1 26 0  5 0 2  1 1 1  1 1 2 11 2", 1),     # Inf beyond filter 1's own 11 entries: not its row
            ("3 3 26 1 26 0  5 0 2  1 1 1  1 1 2 10 2", 0),
            ("3 3 26 1 26 1  5 0 2  1 0 1  1 1 0 3 1", 1),      # masked out
            ("3 3 26 1 26 1  5 0 2  1 0 1  1 2 0 3 1", 0),
            ("3 3 26 1 26 0  5 0 2  1 1 1  2 2 1 0 1", 0),      # NaN in resid
            ("3 3 26 1 26 1  5 0 2  1 1 0  2 2 1 0 1", 1),
            ("3 3 26 1 26 0  5 0 2  1 1 1  3 0 2 1 2", 0),      # Inf in R's lower triangle
            ("3 3 26 1 26 0  5 0 2  1 1 1  3 0 1 2 1", 1),      # NaN in R's upper triangle: never read
            ("3 3 26 1 26 0  5 0 2  1 1 1  3 0 1 1 1", 0),      # ... the diagonal is
            ("16 1 11 1 11 0  0  1  0 0 0 0 0", 1), ("16 1 10 1 11 0  0  1  0 0 0 0 0", 0), ("0 1 11 0 0 0  0  1  0 0 0 0 0", 0),
            ("17 1 11 0 0 0  0  1  0 0 0 0 0", 0)]
    text += ["args " + c for c, _ in args]
    got = linear_host("\n".join(text))
    want = [w for _, w in heads] + [w for _, w in args]
    assert [g[0] for g in got] == want, [(t, g[0], w) for t, g, w in zip(text, got, want) if g[0] != w]
