"""What the moment-matched mixture needs on the host, without a GPU: the binding's symbols with their argument types (no handle is created),
consistency.mixture_weights against systematic_resample, a worked example of the numpy statement done by hand, and the argument checks, id
comparison, weight normalisation, member tables and index arithmetic of eqf_vio_amd/csrc/eqf_mixture_host.hpp (host only, standard
library only) -- tests/mixture_host_main.cpp is compiled with g++ under the address and undefined-behaviour sanitizers and run as a child
process, cases on stdin, results on stdout.  Every expected value is computed here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = (0, 1, 3, 4, 5, 63, 64, 65, 130, 257)
ROWS, LANES = 4, 64


def test_binding_exports_the_symbols_with_their_argument_types():
    from eqf_vio_amd import binding

    L = binding.lib()
    dp, ip, vp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p
    for s in ("eqf_get_mixture_moments", "eqf_merge_filters", "eqf_debug_mixture_launches"):
        assert s in binding.EXPORTED_SYMBOLS
    rp = C.POINTER(binding.MixtureReport)
    assert L.eqf_get_mixture_moments.argtypes == [vp, C.c_int, ip, dp, C.c_int, C.c_int, dp, dp, C.c_int, rp]
    assert L.eqf_merge_filters.argtypes == [vp, C.c_int, ip, dp, C.c_int, C.c_int, rp]
    assert C.sizeof(binding.MixtureReport) == 32
    assert [f[0] for f in binding.MixtureReport._fields_] == ["n_eff", "spread_trace", "total_trace", "n", "info"]
    assert callable(binding.FilterBatch.mixture_moments) and callable(binding.FilterBatch.merge)
    # a NULL handle is refused by the library itself, before anything touches a device
    assert L.eqf_get_mixture_moments(None, 1, None, None, 0, 1, None, None, 0, None) == binding.ERR_INVALID
    assert L.eqf_merge_filters(None, 1, None, None, 0, 0, None) == binding.ERR_INVALID
    assert L.eqf_debug_mixture_launches(None) == binding.ERR_INVALID
    assert binding.PROF_CLASSES == 15  # (the new kernels are timed with events, not with a class of their own)


def test_mixture_weights_are_systematic_resamples():
    from eqf_vio_amd import consistency as cs

    ll = np.array([-3.0, -1.0, -np.inf, np.nan, -2.5, -1.2])
    w = cs.mixture_weights(ll)
    ref = np.exp(np.where(np.isfinite(ll), ll, -np.inf) - (-1.0))
    assert np.array_equal(w, ref / ref.sum()) and w[2] == 0.0 and w[3] == 0.0 and abs(w.sum() - 1.0) < 1e-15
    # the same weights drive the resampling: filter i is drawn floor(B w_i) or ceil(B w_i) times, one of weight 0 never
    B = len(ll)
    for u in (0.0, 0.37, 0.999):
        drawn = np.bincount(cs.systematic_resample(ll, u), minlength=B)
        assert np.all(drawn >= np.floor(B * w)) and np.all(drawn <= np.ceil(B * w)) and drawn[2] == 0 and drawn[3] == 0
    for bad in ([], [-np.inf, np.nan], [0.0, np.inf]):
        with pytest.raises(ValueError):
            cs.mixture_weights(bad)
    assert np.array_equal(cs.normalise_weights([1.0, 3.0]), [0.25, 0.75])
    for bad in ([1.0, -1.0], [0.0, 0.0], [np.nan, 1.0]):
        with pytest.raises(ValueError):
            cs.normalise_weights(bad)


def test_two_members_at_plus_and_minus_d_worked_by_hand():
    """Identity attitude and group (J = I but for the gravity block, which multiplies zeros here), two members at +-d in velocity and
    landmark with equal weights, centred on a third of weight 0: eBar = 0 and P = (Sigma_1 + Sigma_2) / 2 + d d^T, exactly (the gravity
    entries, where the same direction goes through a chart, to a rounding)."""
    from eqf_vio_amd import consistency as cs

    q = np.array([np.cos(0.25), np.sin(0.25), 0.0, 0.0])
    group = dict(Aq=np.array([1.0, 0, 0, 0]), Ax=np.zeros(3), w=np.zeros(3), Qq=np.array([[1.0, 0, 0, 0]]), Qa=np.ones(1))
    d = np.zeros(14)
    d[8:11], d[11:14] = [0.25, -0.5, 0.125], [1.0, 0.5, -2.0]
    S1, S2 = np.diag(np.arange(1.0, 15.0)), 4.0 * np.eye(14)
    S1[6:8, :] = S1[:, 6:8] = S2[6:8, :] = S2[:, 6:8] = 0.0
    ms = []
    for sgn, S in ((0.0, S1), (1.0, S1), (-1.0, S2)):
        origin = dict(q=q, x=np.zeros(3), v=np.array([1.0, 2.0, 3.0]) + sgn * d[8:11], p=np.array([[4.0, 4.0, 8.0]]) + sgn * d[11:14])
        ms.append(dict(origin=origin, group=group, bias=np.zeros(6), sigma=S, estimate=dict(q=q, x=np.zeros(3), v=origin["v"], p=origin["p"])))
    out = cs.mixture_moments_host(ms, [0.0, 3.0, 3.0], 0, centred=True)
    assert np.array_equal(out["mean"][8:], np.zeros(6)) and np.abs(out["mean"][6:8]).max() < 4e-16
    assert np.array_equal(out["P"][8:, 8:], (0.5 * (S1 + S2) + np.outer(d, d))[8:, 8:])
    assert out["n_eff"] == 2.0 and out["spread_trace"] == float(d @ d)
    mg = cs.merge_host(ms, [0.0, 3.0, 3.0], 0)
    assert np.array_equal(mg["estimate"]["v"], [1.0, 2.0, 3.0]) and np.array_equal(mg["estimate"]["p"], [[4.0, 4.0, 8.0]])
    assert np.array_equal(mg["P"][8:, 8:], out["P"][8:, 8:])


# ---- the header under the sanitizers
@pytest.fixture(scope="module")
def mixture_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mixture_host") / "mixture_host")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "eqf_vio_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "mixture_host_main.cpp")], check=True)

    def run(text):
        r = subprocess.run([exe], input=text + "\n", capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        return [ln.split() for ln in r.stdout.split("\n")[:-1]]

    return run


def test_header_is_host_only_and_compiles_with_plain_gcc(tmp_path):
    path = os.path.join(ROOT, "eqf_vio_amd", "csrc", "eqf_mixture_host.hpp")
    includes = [ln.split()[1] for ln in open(path) if ln.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "eqf_mixture_host.hpp"\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.dirname(path), str(tu)], check=True)


def test_index_maps_grids_and_layout(mixture_host):
    out = iter(mixture_host("\n".join(f"map {N}\ngrid {N}" for N in COUNTS)))
    for N in COUNTS:
        n = 11 + 3 * N
        assert [int(t) for t in next(out)] == [i if i < 11 else i + 1 for i in range(n)], N
        cx, ry = max(1, -(-N // LANES)), max(1, -(-N // ROWS))
        assert [int(t) for t in next(out)] == [n, n + 1, cx, ry], N
    for B, cap, ld, gw in ((1, 7, 48, 50), (4, 77, 256, 50), (64, 207, 640, 51)):
        got = [int(t) for t in mixture_host(f"layout {B} {cap} {ld} {gw}")[0]]
        js, es = 16 + 9 * cap, 20 + 3 * cap
        offs = [0, js * B, js * B + es * (B + 1)]
        offs.append(offs[-1] + ld * B)       # mean
        offs.append(offs[-1] + ld)           # out
        offs.append(offs[-1] + 4)            # staged p0
        offs.append(offs[-1] + 3 * cap)      # staged Q
        offs.append(offs[-1] + 5 * cap)      # staged Glob
        offs.append(offs[-1] + gw)           # verdict
        assert got == [js, es] + offs + [offs[-1] + 2]
        assert ld >= 12 + 3 * cap  # (what eqf_create guarantees: every row of the workspace holds a padded vector)


def test_argument_checks_and_id_comparison(mixture_host):
    heads = [("4 1 3 0 1 2 1.0 0.0 2.5 0", 1), ("4 1 3 0 1 1 1.0 0.0 2.5 0", 1),   # a repeated index is two members
             ("4 1 0 0", 0), ("4 1 -1 0", 0),                                        # n < 1
             ("4 1 3 0 1 2 1.0 0.0 2.5 1", 0), ("4 1 3 0 1 2 1.0 0.0 2.5 2", 0),     # NULL idx, NULL w
             ("4 1 3 0 1 4 1.0 1.0 1.0 0", 0), ("4 1 3 0 1 -1 1.0 1.0 1.0 0", 0),    # an index out of range
             ("4 4 3 0 1 2 1.0 1.0 1.0 0", 0), ("4 -1 3 0 1 2 1.0 1.0 1.0 0", 0),    # ref out of range
             ("4 3 3 0 1 2 1.0 1.0 1.0 0", 0),                                       # ref not among idx
             ("4 1 3 0 1 2 1.0 -0.5 1.0 0", 0), ("4 1 3 0 1 2 1.0 nan 1.0 0", 0), ("4 1 3 0 1 2 1.0 inf 1.0 0", 0),
             ("4 1 3 0 1 2 0.0 0.0 0.0 0", 0), ("4 1 2 0 1 1e308 1e308 0", 0),       # a sum that is not positive / not finite
             ("0 0 1 0 1.0 0", 0)]
    ids = [("3 5 7 9 3 5 7 9", 1), ("3 5 7 9 3 5 9 7", 0), ("3 5 7 9 2 5 7", 0), ("0 0", 1), ("0 1 4", 0)]
    got = mixture_host("\n".join(["head " + c for c, _ in heads] + ["ids " + c for c, _ in ids]))
    want = [w for _, w in heads] + [w for _, w in ids]
    assert [int(g[0]) for g in got] == want, [(g, w) for g, w in zip(got, want) if int(g[0]) != w]


def test_normalisation_and_tables(mixture_host):
    rng = np.random.default_rng(77)
    for n in (1, 2, 3, 5, 17):
        w = rng.uniform(0.0, 2.0, n)
        if n >= 3:
            w[1] = 0.0
        idx = rng.integers(0, 6, n)
        ref = int(idx[n // 2])
        out = mixture_host("norm %d %s\ntables 6 %d %d %s %s" % (n, " ".join(float(x).hex() for x in w), ref, n, " ".join(map(str, idx)),
                                                                 " ".join(float(x).hex() for x in w)))
        s = 0.0
        for x in w:
            s += float(x)
        wt = w / s
        q = 0.0
        for x in wt:
            q += float(x) * float(x)
        assert float.fromhex(out[0][0]) == 1.0 / q
        assert [float.fromhex(t) for t in out[1]] == list(wt)
        members = [(int(idx[k]), float(wt[k])) for k in range(n) if wt[k] > 0.0]   # a member of weight 0 is not walked
        assert [(int(out[2][2 * i]), float.fromhex(out[2][2 * i + 1])) for i in range(len(members))] == members and len(out[2]) == 2 * len(members)
        uniq = [ref] + [b for i, (b, _) in enumerate(members) if b != ref and b not in [m[0] for m in members[:i]]]
        assert [int(t) for t in out[3]] == uniq
