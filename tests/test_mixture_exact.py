"""The moment-matched mixture against its exact reference on the CPU (tests/mixture_exact.py): the numpy statement of the definition
(consistency.mixture_moments_host / merge_host), the numpy model of the kernels' blocking and the reference itself lie inside the a-priori
bound on every committed case, K_E is what mixture_cases.py records, and every injected fault leaves the bound -- or breaks the bitwise
symmetry of P -- on at least one case."""
import numpy as np
import pytest

import mixture_cases as mc
import mixture_exact as mx
from eqf_vio_amd import consistency as cs


@pytest.fixture(scope="module")
def refs():
    """{(N, n): (members, w, ref, {centred: reference}, merge reference)}, computed once"""
    out = {}
    for N, n in mc.cases():
        ms, w, ref = mc.case(N, n)
        out[(N, n)] = (ms, w, ref, {c: mx.reference(ms, w, ref, c, mc.K_E) for c in (True, False)}, mx.merge_reference(ms, w, ref, mc.K_E))
    return out


def _inside(got, ref):
    r = mx.ratios(got, ref)
    sym = np.array_equal(np.asarray(got["P"]), np.asarray(got["P"]).T)
    return max(r.values()) <= 1.0 and sym, r


def test_statement_model_and_reference_inside_the_bound(refs):
    worst = {}
    for (N, n), (ms, w, ref, rr, mr) in refs.items():
        for centred, R in rr.items():
            assert R["bound"]["validity"] <= mx.VALIDITY
            for name, got in (("statement", cs.mixture_moments_host(ms, w, ref, centred)), ("model", mx.model(ms, w, ref, centred)),
                              ("reference", dict(mean=R["mean"], P=R["P"]))):
                r = mx.ratios(got, R)
                for k, v in r.items():
                    worst[(name, k)] = max(worst.get((name, k), 0.0), v)
                assert max(r.values()) <= 1.0, (N, n, centred, name, r)
            assert np.array_equal(mx.model(ms, w, ref, centred)["P"], mx.model(ms, w, ref, centred)["P"].T)
        for name, got in (("statement", cs.merge_host(ms, w, ref)), ("model", mx.merge_model(ms, w, ref))):
            r = mx.merge_ratios(got["estimate"], got["bias"], got["P"], mr)
            for k, v in r.items():
                worst[(name, "merge " + k)] = max(worst.get((name, "merge " + k), 0.0), v)
            assert max(r.values()) <= 1.0, (N, n, name, r)
    print({f"{a} {b}": round(v, 3) for (a, b), v in sorted(worst.items())})


def test_k_e_is_the_recorded_one(refs):
    """ORACLE_E of mixture_cases.py: the numpy statement's worst |e - e_50digits| / (u scale), to two digits (libm and BLAS may move the last)."""
    worst = 0.0
    for (N, n), (ms, w, ref, rr, mr) in refs.items():
        for R, got in ((rr[True], cs.mixture_moments_host(ms, w, ref, True)["e"]),):
            for k in range(n):
                want = np.array([float(x) for x in R["E"][k]])
                lo = np.array([float(x - float(x)) for x in R["E"][k]])
                d = np.abs((got[k] - want) - lo)
                s = R["scales"][k]
                ok = s > 0
                assert np.all(d[~ok] == 0.0)
                if ok.any():
                    worst = max(worst, float((d[ok] / (mx.U * s[ok])).max()))
    print("measured ORACLE_E", worst)
    assert 0.5 * mc.ORACLE_E <= worst <= 1.05 * mc.ORACLE_E, worst


def test_quaternions_a_few_roundings_off_unit_stay_inside_the_bound():
    """A filter's own quaternions are unit only to a few roundings.  The reference takes them as given, as the kernels do: scaled by up to
    six units in the last place, the statement (which evaluates the device's formulas) stays where it was; a reference that normalised
    them would be 2.7 bounds away in the mean."""
    N = 17
    ms, w, ref = mc.case(N, 3)
    rng = np.random.default_rng(1)
    for m in ms:
        m["group"]["Qq"] = m["group"]["Qq"] * (1 + rng.integers(-6, 7, (N, 1)) * 2.0 ** -52)
        m["group"]["Aq"] = m["group"]["Aq"] * (1 + 4 * 2.0 ** -52)
        m["origin"]["q"] = m["origin"]["q"] * (1 - 5 * 2.0 ** -52)
        m["estimate"] = mc.estimate_np(m["origin"], m["group"])
    r = mx.ratios(cs.mixture_moments_host(ms, w, ref, True), mx.reference(ms, w, ref, True, mc.K_E))
    g = cs.merge_host(ms, w, ref)
    r.update({"merge " + k: v for k, v in mx.merge_ratios(g["estimate"], g["bias"], g["P"], mx.merge_reference(ms, w, ref, mc.K_E)).items()})
    print(r)
    assert max(r.values()) <= 1.0, r
    # ... and a Sigma that is symmetric only to rounding counts with the blocks on and below its block diagonal: those above have no reader
    S = ms[0]["sigma"]
    blk = np.concatenate([np.zeros(11, dtype=int), 1 + np.repeat(np.arange(N), 3)])
    ms[0]["sigma"] = S + (blk[:, None] < blk[None, :]) * S * 1e-13
    assert not np.array_equal(ms[0]["sigma"], S)
    assert cs.mixture_moments_host(ms, w, ref, True)["P"].tobytes() == cs.mixture_moments_host(ms[:0] + [dict(ms[0], sigma=S)] + ms[1:], w, ref, True)["P"].tobytes()


@pytest.mark.parametrize("fault", mx.FAULTS)
def test_every_injected_fault_leaves_the_bound(refs, fault):
    caught = []
    for (N, n), (ms, w, ref, rr, mr) in refs.items():
        if fault in mx.MERGE_FAULTS:
            got = mx.merge_model(ms, w, ref, fault)
            r = mx.merge_ratios(got["estimate"], got["bias"], got["P"], mr)
            if max(r.values()) > 1.0:
                caught.append((N, n))
        else:
            for centred, R in rr.items():
                ok, r = _inside(mx.model(ms, w, ref, centred, fault), R)
                if not ok:
                    caught.append((N, n, centred))
    assert caught, fault
    print(fault, "caught on", len(caught), "cases, first", caught[0])


def test_two_members_at_plus_and_minus_d_by_hand():
    """Two members at +-d in velocity with equal weights, seen from a third member of weight 0 at the middle: eBar = 0 in the velocity
    entries and P = (Sigma_1 + Sigma_2) / 2 + d d^T there (the group is the identity: so is J, but for its gravity block)."""
    N = 2
    base = mc.member(N, 0)
    base["group"] = dict(Aq=np.array([1.0, 0, 0, 0]), Ax=np.zeros(3), w=np.zeros(3), Qq=np.tile([1.0, 0, 0, 0], (N, 1)), Qa=np.ones(N))
    d = np.array([0.25, -0.5, 0.125])
    ms = []
    for sgn, scale in ((0.0, 1.0), (1.0, 1.0), (-1.0, 3.0)):
        m = dict(base)
        m["origin"] = dict(base["origin"], v=base["origin"]["v"] + sgn * d)
        m["sigma"] = scale * base["sigma"]
        m["estimate"] = mc.estimate_np(m["origin"], m["group"])
        ms.append(m)
    out = cs.mixture_moments_host(ms, [0.0, 2.0, 2.0], 0, centred=True)
    assert np.abs(out["mean"]).max() < 1e-15
    want = 0.5 * (ms[1]["sigma"] + ms[2]["sigma"])
    want[8:11, 8:11] += np.outer(d, d)
    Jg = cs.local_jacobian_blocks(base["origin"], base["group"])["G"]
    J = np.eye(11 + 3 * N)
    J[6:8, 6:8] = Jg
    assert np.allclose(out["P"], J @ want @ J.T, rtol=0, atol=1e-14)
    assert out["n_eff"] == 2.0 and abs(out["spread_trace"] - d @ d) < 1e-15
