"""What the covariance draws need on the host, without a GPU: consistency.local_retract against local_error, the binding's three symbols
with their argument types (no handle is created), and the index arithmetic of eqf_vio_amd/csrc/eqf_sample_host.hpp (host only, standard
library only) -- tests/sample_host_main.cpp is compiled with g++ under the address and undefined-behaviour sanitizers and run as a child
process, cases on stdin, results on stdout.  Every expected value is computed here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- consistency.local_retract
def _estimate(rng, N):
    q = rng.standard_normal(4)
    return dict(q=q / np.linalg.norm(q), x=rng.standard_normal(3), v=rng.standard_normal(3), p=rng.standard_normal((N, 3)) + [0, 0, 5])


@pytest.mark.parametrize("tilt", [1e-9, 1e-3, 0.1, 0.5])
def test_local_error_of_local_retract_is_the_error(tilt):
    """eps up to 0.5 rad of gravity tilt (chart coordinate tan(tilt / 2) in a random direction), to 1e-13."""
    from eqf_vio_amd import consistency as cs

    rng = np.random.default_rng(int(tilt * 1e9))
    for N in (0, 1, 7):
        for _ in range(20):
            est, bias = _estimate(rng, N), rng.standard_normal(6) * 0.1
            phi = rng.uniform(0, 2 * np.pi)
            e = np.concatenate([rng.standard_normal(6) * 0.01, np.tan(tilt / 2) * np.array([np.cos(phi), np.sin(phi)]),
                                rng.standard_normal(3), rng.standard_normal(3 * N)])
            truth = cs.local_retract(est, e, bias=bias)
            back = cs.error_vector(cs.local_error(est, truth, bias=bias, true_bias=truth["bias"]))
            assert np.max(np.abs(back - e)) <= 1e-13, (tilt, N, np.max(np.abs(back - e)))
            # the sampled truth is a state: unit attitude, gravity tilted by `tilt`, yaw untouched (the rotation axis is orthogonal to gravity)
            assert abs(np.linalg.norm(truth["q"]) - 1.0) <= 1e-14
            c = float(cs.gravity_dir(est["q"]) @ cs.gravity_dir(truth["q"]))
            assert abs(np.arccos(np.clip(c, -1, 1)) - tilt) <= 1e-7
            dR = cs.quat_to_matrix(est["q"]).T @ cs.quat_to_matrix(truth["q"])
            axis = np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])
            assert abs(axis @ cs.gravity_dir(est["q"])) <= 1e-12
            # the dictionary form is the same thing
            again = cs.local_retract(est, dict(bias=e[0:6], gravity=e[6:8], velocity=e[8:11], lm=e[11:].reshape(-1, 3)), bias=bias)
            assert all(np.array_equal(truth[k], again[k]) for k in truth)


def test_local_retract_of_zero_is_the_estimate():
    from eqf_vio_amd import consistency as cs

    rng = np.random.default_rng(3)
    est, bias = _estimate(rng, 5), rng.standard_normal(6)
    truth = cs.local_retract(est, np.zeros(11 + 15), bias=bias)
    assert all(np.array_equal(truth[k], est[k]) for k in ("q", "x", "v", "p")) and np.array_equal(truth["bias"], bias)
    assert "bias" not in cs.local_retract(est, np.zeros(11 + 15))
    with pytest.raises(ValueError):
        cs.local_retract(est, np.concatenate([np.zeros(6), [1e100, 0.0], np.zeros(3 + 15)]))  # (a tilt of pi)


# ---- the binding
def test_binding_exports_the_three_symbols_with_their_argument_types():
    from eqf_vio_amd import binding

    for name in ("eqf_sample_sigma", "eqf_apply_increment", "eqf_perturb_filters"):
        assert name in binding.EXPORTED_SYMBOLS
    L = binding.lib()
    dp, vp, st = C.POINTER(C.c_double), C.c_void_p, C.POINTER(binding.SigmaStats)
    assert L.eqf_sample_sigma.argtypes == [vp, C.c_int, C.c_int, C.c_int, dp, C.c_int, dp, dp, C.c_int, st]
    assert L.eqf_apply_increment.argtypes == [vp, dp, C.c_int, C.POINTER(C.c_ubyte)]
    assert L.eqf_perturb_filters.argtypes == [vp, C.c_int, dp, C.c_int, dp, st]
    for m in ("sample_sigma", "apply_increment", "perturb"):
        assert callable(getattr(binding.FilterBatch, m))
    from eqf_vio_amd import filter as vf

    assert callable(vf.VIOFilter.sampleStateError) and callable(vf.VIOFilter.perturbState)
    # a NULL handle is refused by the library itself, before anything touches a device
    assert L.eqf_sample_sigma(None, 1, 0, 0, None, 0, None, None, 0, None) == binding.ERR_INVALID
    assert L.eqf_apply_increment(None, None, 0, None) == binding.ERR_INVALID
    assert L.eqf_perturb_filters(None, 0, None, 0, None, None) == binding.ERR_INVALID


# ---- the header under the sanitizers
@pytest.fixture(scope="module")
def sample_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sample_host") / "sample_host")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "eqf_vio_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "sample_host_main.cpp")], check=True)

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        return [[int(t) for t in ln.split()] for ln in r.stdout.split("\n")[:-1]]

    return run


def test_header_is_host_only_and_compiles_with_plain_gcc(tmp_path):
    path = os.path.join(ROOT, "eqf_vio_amd", "csrc", "eqf_sample_host.hpp")
    includes = [ln.split()[1] for ln in open(path) if ln.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "eqf_sample_host.hpp"\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.dirname(path), str(tu)], check=True)


OFF = {0: 0, 6: 6, 11: 12}
COUNTS = (0, 1, 5, 17, 18, 43)


def test_reference_and_padded_index_maps(sample_host):
    cases = [(first, N) for first in (0, 6, 11) for N in COUNTS]
    out = iter(sample_host("\n".join(f"map {first} {N}" for first, N in cases)))
    for first, N in cases:
        n = 11 + 3 * N
        want = [-1 if i < first else (i if i < 11 else i + 1) - OFF[first] for i in range(n)]
        got = next(out)
        assert got == want, (first, N)
        used = [c for c in got if c >= 0]
        assert used == sorted(set(used)) and (not used or (used[0] == 0 and used[-1] == (n - 1 if n - 1 < 11 else n) - OFF[first]))
        back = next(out)
        assert back == list(range(11)) + [-1] + list(range(11, n)), (first, N)
        assert next(out) == [OFF[first], 12 + 3 * N - OFF[first]]
    assert sample_host("map 5 3")[2][0] == -1 and sample_host("map 12 3")[2][0] == -1  # (not block boundaries)


def test_tile_counts(sample_host):
    cases = [(s, m) for s in (-1, 0, 1, 15, 16, 17, 32, 63, 64) for m in (-3, 0, 1, 63, 64, 65, 128, 129, 612)]
    out = sample_host("\n".join(f"grid {s} {m}" for s, m in cases))
    for (s, m), got in zip(cases, out):
        tiles = 0 if s <= 0 else -(-s // 16)
        assert got == [tiles, 16 * tiles, 0 if m <= 0 else -(-m // 64)], (s, m)


def test_pack_and_unpack_rows(sample_host):
    cases = [(first, N, extra) for first in (0, 6, 11) for N in COUNTS for extra in (0, 5)]
    out = iter(sample_host("\n".join(f"pack {first} {N} {max(12 + 3 * N - OFF[first] + extra, 1)}\nfill {first} {N}" for first, N, extra in cases)))
    for first, N, extra in cases:
        n, m = 11 + 3 * N, 12 + 3 * N - OFF[first]
        row = np.zeros(max(m + extra, 1), dtype=int)
        for i in range(first, n):
            row[(i if i < 11 else i + 1) - OFF[first]] = i + 1
        assert next(out) == row.tolist(), (first, N, extra)
        if first < 11:
            assert row[11 - OFF[first]] == 0  # (the pad column)
        back = [0] * first + list(range(first + 1, n + 1)) + [-7, -7]
        assert next(out) == back, (first, N, extra)
        assert next(out) == [0] * first + [9] * (n - first) + [-7, -7], (first, N)


def test_small_image_and_record_layouts(sample_host):
    """scale | vectors | mask against the formula written out -- 8 B (1 + 12 + 3 cap) + B bytes, as the calls have always allocated --, the
    two upload ranges (the scales in front; the vectors with the mask behind them), and the records [B][4 + 16]."""
    cases = [(B, cap) for B in (1, 3, 8) for cap in (1, 5, 21, 200)]
    for (B, cap), got in zip(cases, sample_host("\n".join(f"small {B} {cap}" for B, cap in cases))):
        n = 12 + 3 * cap
        total = 8 * B * (1 + n) + B
        assert got == [n, 0, B, B * (1 + n), total, 0, 8 * B, 8 * B, 8 * B * n + B], (B, cap)
        offs, sizes = [8 * got[1], 8 * got[2], 8 * got[3]], [8 * B, 8 * B * n, B]
        assert offs == sorted(offs) and all(o + s <= nxt for o, s, nxt in zip(offs, sizes, offs[1:] + [total]))
        # the ranges: exactly the scales; exactly the vectors and the mask, to the end of the image
        assert got[5] + got[6] == offs[1] and got[7] == offs[1] and got[7] + got[8] == total
    for B in (1, 3, 8):
        got = sample_host(f"records {B}")[0]
        assert got[:3] == [20, 20 * B, 160 * B]
        assert got[3:] == [v for b in range(B) for v in (20 * b, 20 * b + 3, 20 * b + 4, 20 * b + 19)]
        assert max(got[3:]) < got[1]


def test_argument_checks(sample_host):
    n = 11 + 3 * 5
    ok = dict(local=1, first=0, nsamp=1, z=1, ldz=n, eps=1, lde=n, stats=1, nMax=5)
    draws = [({}, 1), (dict(stats=0), 1), (dict(local=0, first=6, nsamp=64), 1), (dict(first=11, ldz=n + 3), 1), (dict(nsamp=0, z=0, eps=0, ldz=0, lde=0), 1),
             (dict(local=2), 0), (dict(local=-1), 0), (dict(first=5), 0), (dict(first=12), 0), (dict(nsamp=65), 0), (dict(nsamp=-1), 0),
             (dict(z=0), 0), (dict(eps=0), 0), (dict(ldz=n - 1), 0), (dict(lde=n - 1), 0), (dict(nsamp=0, stats=0), 0)]
    text = ["draw " + " ".join(str({**ok, **kw}[k]) for k in ok) for kw, _ in draws]
    # increments: B ldg mask? N[B] mask[B] bad_b bad_i kind
    incs = [("3 26 0  5 0 2  1 1 1  0 0 0", 1), ("3 26 0  5 0 2  1 1 1  0 25 1", 0), ("3 26 0  5 0 2  1 1 1  2 16 2", 0),
            ("3 26 0  5 0 2  1 1 1  2 17 1", 1),   # (beyond filter 2's own 17 entries: not its increment)
            ("3 26 1  5 0 2  1 0 1  1 3 1", 1),    # (masked out)
            ("3 26 1  5 0 2  1 0 1  0 3 2", 0), ("3 25 0  5 0 2  1 1 1  0 0 0", 0), ("3 25 1  5 0 2  0 1 1  0 0 0", 0), ("1 11 0  0  1  0 10 1", 0),
            ("1 11 0  0  1  0 0 0", 1), ("1 10 0  0  1  0 0 0", 0)]
    text += ["inc " + c for c, _ in incs]
    # perturbations: first z ldz nMax B scale? scale_b kind
    pers = [("0 1 26 5 3 1 0 0", 1), ("6 1 26 5 3 0 0 0", 1), ("11 1 30 5 3 1 0 0", 1), ("5 1 26 5 3 1 0 0", 0), ("0 0 26 5 3 1 0 0", 0),
            ("0 1 25 5 3 1 0 0", 0), ("0 1 26 5 3 1 2 1", 0), ("0 1 26 5 3 1 1 2", 0), ("0 1 26 5 3 0 1 2", 1)]
    text += ["perturb " + c for c, _ in pers]
    got = sample_host("\n".join(text))
    want = [w for _, w in draws] + [w for _, w in incs] + [w for _, w in pers]
    assert [g[0] for g in got] == want, [(t, g[0], w) for t, g, w in zip(text, got, want) if g[0] != w]
