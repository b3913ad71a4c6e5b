"""Host side of the copy / fork / resample feature (no GPU): the C ABI declares and exports eqf_copy_filters, consistency.systematic_resample
turns log-likelihoods into parents, and FilterBatch.copy_filters has no CPU fallback."""
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
