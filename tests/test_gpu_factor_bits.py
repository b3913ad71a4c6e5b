"""Every public call that runs the blocked Cholesky of csrc/eqf_factor.hpp -- eqf_get_nees, eqf_sample_sigma, eqf_perturb_filters,
eqf_update_landmarks, eqf_get_merge_costs -- returns the bits that the three-kernels-per-route code before it returned: the digests of
tests/golden/factor_bits.json were recorded on an MI355X from a build of the commit BEFORE the kernels were merged
(tests/golden/make_golden_factor_bits.py; the fixture names that build and the compiler).  Cases and edges: tests/factor_bits_cases.py.
A mismatch names the case and the field.  The fixture pins bits, so it holds for the compiler it names: a compiler that contracts or
schedules the arithmetic differently needs a fresh recording from the same parent sources, not a change here."""
import json
import os

import pytest

import factor_bits_cases as fb

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "factor_bits.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_fixture_covers_the_cases(golden):
    assert sorted(golden["cases"]) == sorted(fb.CASES)
    assert len(golden["build_info"]) == 64 and golden["compiler"]


@pytest.mark.parametrize("name", sorted(fb.CASES))
def test_same_bits_as_before_the_merge(golden, name):
    from eqf_vio_amd import binding

    got, want = fb.CASES[name](binding), golden["cases"][name]
    assert sorted(got) == sorted(want), f"{name}: fields differ"
    bad = [k for k in sorted(got) if got[k] != want[k]]
    assert not bad, f"{name}: {len(bad)} of {len(got)} fields differ from the recording: " + "; ".join(
        f"{k}: got {got[k]}, recorded {want[k]}" for k in bad[:6])
