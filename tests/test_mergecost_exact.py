"""The pairwise merge costs against their exact reference on the CPU (tests/mergecost_exact.py): the numpy statement
(consistency.merge_costs_host) and the numpy model of the kernels' blocking lie inside the a-priori bound on every committed case, pairs
of identical members cost exactly 0, K_LOG1P is what mergecost_cases.py records, every injected fault leaves the bound on at least one
case, and every decision of the greedy reduction on the committed cluster cases has its margin."""
import numpy as np
import pytest

import mergecost_cases as gc
import mergecost_exact as gx
import mixture_cases as mc
from eqf_vio_amd import consistency as cs

SOME = [(0, 1), (5, 1), (2, 4), (3, 5), (3, 0), (1, 2)]  # a repeated index, the weight of 0, the centre, pairs named both ways round


def _pairs(N, first):
    return None if (N < 39 and first == 0) else SOME


@pytest.fixture(scope="module")
def refs():
    """{(N, kind, first): (members, w, ref, pairs, reference)}, computed once"""
    out = {}
    for N in gc.SIZES:
        ms, w, ref = gc.case(N)
        imgs, cache = gx.member_images(ms, ref, mc.K_E), {}
        for kind in gx.KINDS:
            for first in gc.FIRSTS:
                pairs = _pairs(N, first)
                out[(N, kind, first)] = (ms, w, ref, pairs, gx.reference(ms, w, ref, kind, first, pairs, mc.K_E, gc.K_LOG1P, imgs, cache))
    return out


def test_statement_and_model_inside_the_bound(refs):
    worst = {}
    for (N, kind, first), (ms, w, ref, pairs, R) in refs.items():
        assert R["bound"]["validity"] <= gx.VALIDITY
        for name, got in (("statement", cs.merge_costs_host(ms, w, ref, kind, first, pairs)), ("model", gx.model(ms, w, ref, kind, first, pairs))):
            r = gx.ratios(got, R)
            for k, v in r.items():
                worst[(name, k)] = max(worst.get((name, k), 0.0), v)
            assert max(r.values()) <= 1.0, (N, kind, first, name, r)
            # the repeated index: the same member twice costs exactly 0
            for p, (i, j) in enumerate(R["pairs"]):
                if {i, j} == {1, 5}:
                    assert got["cost"][p] == 0.0 and got["maha"][p] == 0.0 and got["logdet_pair"][p] == got["member_logdet"][1], (N, kind, first, name)
    print({f"{a} {b}": round(v, 4) for (a, b), v in sorted(worst.items())})


def test_k_log1p_is_the_recorded_one(refs):
    ts = [t for (N, kind, first), v in refs.items() if kind == "runnalls" for t in v[4]["t"]]
    worst = gx.log1p_error_units(ts)
    print("measured ORACLE_LOG1P", worst)
    assert 0.5 * gc.ORACLE_LOG1P <= worst <= 1.05 * gc.ORACLE_LOG1P, worst


@pytest.mark.parametrize("fault", gx.FAULTS)
def test_every_injected_fault_leaves_the_bound(refs, fault):
    caught = []
    if fault == "upper_triangle_read":  # needs a Sigma that is not symmetric: the reference reads what the kernels read
        for N in (1, 17):
            ms, w, ref = gc.unsymmetric(N)
            R = gx.reference(ms, w, ref, "runnalls", 0, SOME, mc.K_E, gc.K_LOG1P)
            for name, got in (("statement", cs.merge_costs_host(ms, w, ref, "runnalls", 0, SOME)), ("model", gx.model(ms, w, ref, "runnalls", 0, SOME))):
                assert max(gx.ratios(got, R).values()) <= 1.0, (N, name)
            if max(gx.ratios(gx.model(ms, w, ref, "runnalls", 0, SOME, fault), R).values()) > 1.0:
                caught.append(N)
    else:
        for (N, kind, first), (ms, w, ref, pairs, R) in refs.items():
            if N > 18:
                continue
            if max(gx.ratios(gx.model(ms, w, ref, kind, first, pairs, fault), R).values()) > 1.0:
                caught.append((N, kind, first))
    assert caught, fault
    print(fault, "caught on", len(caught), "cases, first", caught[0])


def reduction_margins(ms, w, target, kind):
    """The greedy reduction of consistency.reduce_mixture_host step by step with, per step, the reference's cheapest and second-cheapest
    cost and the sum of their bounds: [(pair, cost, gap, bounds)]"""
    wt = cs.normalise_weights(w)
    alive = list(range(len(ms)))
    cur, wk = {k: m for k, m in enumerate(ms)}, {k: float(wt[k]) for k in alive}
    centre = int(np.argmax(wt))
    steps = []
    while len(alive) > target:
        mem = [cur[k] for k in alive]
        R = gx.reference(mem, [wk[k] for k in alive], alive.index(centre), kind, 0, None, mc.K_E, gc.K_LOG1P)
        order = np.argsort(R["cost"].astype(np.float64), kind="stable")
        c1, c2 = order[0], order[1]
        a, b = (alive[p] for p in R["pairs"][c1])
        steps.append(((a, b), float(R["cost"][c1]), float(R["cost"][c2] - R["cost"][c1]), float(R["bound"]["cost"][c1] + R["bound"]["cost"][c2])))
        keep, drop = (b, a) if b == centre else (a, b)
        cur[keep] = cs.merged_member([cur[a], cur[b]], [wk[a], wk[b]], 0 if keep == a else 1)
        wk[keep] = wk[a] + wk[b]
        del cur[drop], wk[drop]
        alive.remove(drop)
    return steps


@pytest.mark.parametrize("N", gc.CLUSTER_SIZES)
@pytest.mark.parametrize("kind", gx.KINDS)
def test_every_decision_of_the_reduction_has_its_margin(N, kind):
    ms, w, lab = gc.cluster_case(N)
    steps = reduction_margins(ms, w, gc.CLUSTER_TARGET, kind)
    alive, wk, left, log = cs.reduce_mixture_host(ms, w, gc.CLUSTER_TARGET, kind=kind)
    assert len(log) == len(ms) - gc.CLUSTER_TARGET == len(steps)
    for ((keep, drop), c), ((a, b), cr, gap, bnd) in zip(log, steps):
        print(f"N={N} {kind}: merge {(a, b)} cost {cr:.3e} gap {gap:.3e} bounds {bnd:.3e} margin {gap / bnd:.1e}")
        assert {keep, drop} == {a, b} and lab[a] == lab[b], "the reduction left its cluster"
        assert gap > gc.MARGIN * bnd, (N, kind, (a, b), gap, bnd)
        assert abs(c - cr) <= bnd
    assert sorted(lab[k] for k in alive) == [0, 1, 2] and abs(wk.sum() - 1.0) < 1e-15
    # a threshold between the clusters' own costs and the costs between clusters stops the reduction at the same place
    _, _, _, log2 = cs.reduce_mixture_host(ms, w, 1, max_cost=10 * max(s[1] for s in steps), kind=kind)
    assert log2 == log
