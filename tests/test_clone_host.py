"""Host side of the copy / fork / resample feature (no GPU): the C ABI declares and exports eqf_copy_filters, consistency.systematic_resample
turns log-likelihoods into parents, FilterBatch.copy_filters has no CPU fallback, and the host's decisions of a copy
(eqf_vio_amd/csrc/eqf_clone_host.hpp: the small state's layout and the copy plan) give the answers written out here when
tests/clone_host_main.cpp runs them under the address and undefined-behaviour sanitizers."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_eqf_copy_filters():
    from eqf_vio_amd import binding

    txt = open(os.path.join(ROOT, "include", "eqf_vio_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+eqf_copy_filters\s*\(\s*eqf_filter\s*\*\s*dst\s*,\s*eqf_filter\s*\*\s*src\s*,\s*int\s+n\s*,\s*const\s+int\s*\*\s*dst_idx\s*,"
                     r"\s*const\s+int\s*\*\s*src_idx\s*\)\s*;", txt)
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "eqf_copy_filters" in {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    assert "eqf_copy_filters" in binding.EXPORTED_SYMBOLS
    assert len(binding.lib().eqf_copy_filters.argtypes) == 5
    # NULL handles are refused before anything is touched (no device needed to say so)
    assert binding.lib().eqf_copy_filters(None, None, 0, None, None) == binding.ERR_INVALID


# ---- eqf_clone_host.hpp under the sanitizers: the small state's layout and the copy plan (tests/clone_host_main.cpp, cases on stdin)
@pytest.fixture(scope="module")
def clone_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("clone_host") / "clone_host")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "eqf_vio_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "clone_host_main.cpp")], check=True)

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        return [[int(t) for t in ln.split()] for ln in r.stdout.split("\n")[:-1]]

    return run


def test_header_is_host_only_and_compiles_with_plain_gcc(tmp_path):
    path = os.path.join(ROOT, "eqf_vio_amd", "csrc", "eqf_clone_host.hpp")
    includes = [ln.split()[1] for ln in open(path) if ln.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "eqf_clone_host.hpp"\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.dirname(path), str(tu)], check=True)


def test_small_state_counts_and_staging_image(clone_host):
    """The six per-filter counts eqf_create allocates, and Glob | p0 | Q | delta | gamma | gammaTot | innov in bytes; the total is what the
    in-place copy has always allocated: (glob + 8 (3 cap + 5 cap + 2 cap + (12 + 3 cap) + (9 + 3 cap) + (head + cap))) B."""
    head = 8
    cases = [(B, cap, glob) for B in (1, 3, 8) for cap in (1, 5, 21, 200) for glob in (240, 328)]
    for (B, cap, glob), got in zip(cases, clone_host("\n".join(f"small {B} {cap} {glob} {head}" for B, cap, glob in cases))):
        counts = [3 * cap, 5 * cap, 2 * cap, 12 + 3 * cap, 9 + 3 * cap, head + cap]
        assert got[:6] == counts, (B, cap)
        sizes = [glob * B] + [8 * c * B for c in counts]
        want, at = [], 0
        for s in sizes:
            want.append(at)
            at += s
        assert got[6:13] == want and got[13] == at == (glob + 8 * sum(counts)) * B, (B, cap, glob)
        offs = got[6:13]
        assert offs[0] == 0 and all(o + s <= nxt for o, s, nxt in zip(offs, sizes, offs[1:] + [got[13]]))  # ascending, no overlap
        assert all(o % 8 == 0 for o in offs)  # (the Globs in front, every array of doubles on 8 bytes)


OK, INVALID, CAPACITY = 0, -1, -4


def _plan(dstB, srcB, cap, in_place, dst, src, srcN):
    assert len(dst) == len(src) and len(srcN) == srcB
    return f"plan {dstB} {srcB} {cap} {int(in_place)} {len(dst)} " + " ".join(str(v) for v in list(dst) + list(src) + list(srcN))


def _answer(code, n_max, pairs, stage):
    return [code, n_max, len(pairs), len(stage)] + [v for p in pairs + stage for v in p]


def test_copy_plan(clone_host):
    """Every case with its expected answer written out: code, nMaxN, the pairs (dst, src, N, fromStage) and the stage pairs."""
    N = [5, 20, 21, 0, 7]  # landmarks of filters 0 .. 4
    cases = [
        ("n = 0", _plan(5, 5, 32, 1, [], [], N), _answer(OK, 0, [], [])),
        ("all identity in place", _plan(5, 5, 32, 1, [0, 1, 2], [0, 1, 2], N), _answer(OK, 0, [], [])),
        ("identity in place beside a real pair", _plan(5, 5, 32, 1, [0, 3], [0, 2], N), _answer(OK, 21, [(3, 2, 21, 0)], [])),
        ("dst below range", _plan(5, 5, 32, 1, [1, -1], [0, 0], N), _answer(INVALID, 0, [], [])),
        ("dst beyond range", _plan(5, 5, 32, 1, [5], [0], N), _answer(INVALID, 0, [], [])),
        ("src below range", _plan(5, 5, 32, 1, [1], [-1], N), _answer(INVALID, 0, [], [])),
        ("src beyond range", _plan(5, 5, 32, 1, [1], [5], N), _answer(INVALID, 0, [], [])),
        ("src beyond the source handle's range", _plan(5, 2, 32, 0, [4], [2], N[:2]), _answer(INVALID, 0, [], [])),
        ("dst within its own handle's range only", _plan(2, 5, 32, 0, [2], [0], N), _answer(INVALID, 0, [], [])),
        ("a destination named twice", _plan(5, 5, 32, 1, [1, 2, 1], [0, 0, 3], N), _answer(INVALID, 0, [], [])),
        ("a destination named twice, both identities", _plan(5, 5, 32, 1, [1, 1], [1, 1], N), _answer(INVALID, 0, [], [])),
        ("a source beyond the capacity", _plan(5, 5, 20, 1, [0], [2], N), _answer(CAPACITY, 0, [], [])),
        ("... also behind a valid pair", _plan(5, 5, 20, 1, [3, 0], [1, 2], N), _answer(CAPACITY, 0, [], [])),
        ("... across handles", _plan(5, 5, 20, 0, [3, 0], [1, 2], N), _answer(CAPACITY, 0, [], [])),
        ("a source that just fits", _plan(5, 5, 21, 1, [0], [2], N), _answer(OK, 21, [(0, 2, 21, 0)], [])),
        ("range is judged before capacity", _plan(5, 5, 20, 1, [0, 9], [2, 1], N), _answer(INVALID, 0, [], [])),
        ("swap in place: both staged, each once", _plan(5, 5, 32, 1, [0, 1], [1, 0], N),
         _answer(OK, 20, [(0, 1, 20, 1), (1, 0, 5, 1)], [(1, 1, 20, 0), (0, 0, 5, 0)])),
        ("chain 0 -> 1, 1 -> 2: only 1 staged", _plan(5, 5, 32, 1, [1, 2], [0, 1], N),
         _answer(OK, 20, [(1, 0, 5, 0), (2, 1, 20, 1)], [(1, 1, 20, 0)])),
        ("the chain named the other way round", _plan(5, 5, 32, 1, [2, 1], [1, 0], N),
         _answer(OK, 20, [(2, 1, 20, 1), (1, 0, 5, 0)], [(1, 1, 20, 0)])),
        ("one staged source read by three pairs", _plan(5, 5, 32, 1, [1, 2, 3, 0], [0, 0, 0, 4], N),
         _answer(OK, 7, [(1, 0, 5, 1), (2, 0, 5, 1), (3, 0, 5, 1), (0, 4, 7, 0)], [(0, 0, 5, 0)])),
        ("fan-out of a source that is nobody's destination", _plan(5, 5, 32, 1, [0, 1, 3], [2, 2, 2], N),
         _answer(OK, 21, [(0, 2, 21, 0), (1, 2, 21, 0), (3, 2, 21, 0)], [])),
        ("across handles: a swap's indices stage nothing", _plan(5, 5, 32, 0, [0, 1], [1, 0], N),
         _answer(OK, 20, [(0, 1, 20, 0), (1, 0, 5, 0)], [])),
        ("across handles: equal indices are no identity", _plan(5, 5, 32, 0, [0, 3], [0, 3], N),
         _answer(OK, 5, [(0, 0, 5, 0), (3, 3, 0, 0)], [])),
        ("across handles of different batch", _plan(2, 5, 32, 0, [1, 0], [4, 2], N), _answer(OK, 21, [(1, 4, 7, 0), (0, 2, 21, 0)], [])),
        ("an empty source", _plan(5, 5, 32, 1, [0], [3], N), _answer(OK, 0, [(0, 3, 0, 0)], [])),
    ]
    got = clone_host("\n".join(text for _, text, _ in cases))
    assert len(got) == len(cases)
    for (name, _, want), g in zip(cases, got):
        assert g == want, (name, g, want)


def test_systematic_resample_equal_weights_give_the_identity():
    from eqf_vio_amd.consistency import systematic_resample

    for B in (1, 2, 7, 64):
        for u in (0.0, 0.3, 0.999):
            p = systematic_resample(np.full(B, -123.4), u)
            assert p.dtype == np.int32 and np.array_equal(p, np.arange(B)), (B, u)


def test_systematic_resample_one_dominant_weight_gives_one_parent():
    from eqf_vio_amd.consistency import systematic_resample

    ll = np.full(9, -50.0)
    ll[6] = 900.0  # (exp(-950) underflows to 0: the maximum is subtracted first, nothing overflows)
    for u in (0.0, 0.5, 0.99):
        assert np.array_equal(systematic_resample(ll, u), np.full(9, 6))


def test_systematic_resample_is_monotone_and_counts_are_within_one():
    from eqf_vio_amd.consistency import systematic_resample

    rng = np.random.default_rng(42)
    for B in (8, 33, 200):
        w = rng.random(B) ** 3
        w /= w.sum()
        for u in (0.0, 0.25, 0.7, 0.999):
            p = systematic_resample(np.log(w) + 17.0, u)
            assert p.shape == (B,) and np.all(np.diff(p) >= 0) and p.min() >= 0 and p.max() < B
            counts = np.bincount(p, minlength=B)
            assert np.all(np.abs(counts - B * w) < 1.0 + 1e-9), (B, u)
            assert np.array_equal(p, systematic_resample(np.log(w) + 17.0, u))  # deterministic for a given u


def test_systematic_resample_gives_invalid_logliks_weight_zero():
    from eqf_vio_amd.consistency import systematic_resample

    ll = np.array([-3.0, -np.inf, np.nan, -3.0, -np.inf])
    for u in (0.0, 0.4, 0.999):
        p = systematic_resample(ll, u)
        assert set(int(x) for x in p) <= {0, 3} and np.all(np.diff(p) >= 0)
        assert abs(int(np.sum(p == 0)) - 2.5) <= 1.0
    for bad in ([-np.inf, np.nan], [np.nan], []):
        with pytest.raises(ValueError):
            systematic_resample(np.array(bad, dtype=float), 0.5)
    for u in (-0.1, 1.0):
        with pytest.raises(ValueError):
            systematic_resample(np.zeros(4), u)


def test_copy_filters_without_a_gpu_fails_as_filterbatch_does():
    """No CPU fallback: without a GPU there is no FilterBatch to copy from or into (tests/test_cabi.py pins the same for eqf_create)."""
    import torch

    from eqf_vio_amd import binding

    assert callable(binding.FilterBatch.copy_filters) and callable(binding.FilterBatch.resample)
    if torch.cuda.is_available():
        fb = binding.FilterBatch({}, capacity=8, batch=2)
        fb.resample([1, 0])
        assert fb.device_error() == 0
        return
    with pytest.raises(binding.EqfError) as ei:
        a = binding.FilterBatch({}, capacity=8)
        a.copy_filters(a, [0], [0])
    assert ei.value.code in (binding.ERR_NO_DEVICE, binding.ERR_HIP)
