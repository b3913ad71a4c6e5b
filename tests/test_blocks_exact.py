"""The per-landmark block measurement update on the CPU (csrc/eqf_blocks.hpp: eqf_update_landmarks; consistency.update_landmarks_host and the
row builders): the reference and the bound of tests/blocks_exact.py on every committed case of tests/blocks_cases.py.

  * K_BLOCKS is re-measured from consistency.update_landmarks_host (4 x its worst ratio to the unit form);
  * update_landmarks_host sits inside every bound, its verdicts and dof are the reference's;
  * no verdict hangs on a rounding: d2 of an entry that stays < 40, of one that leaves > 1e3, lm_gate = 60;
  * every injected fault of blocks_exact.FAULTS leaves some bound by >= 100 (or changes used / dof) on some case (the table is printed);
  * stereo_rows / depth_rows / position_rows against the measurement functions they linearise.
R goes in with its upper triangles negated everywhere: only the lower triangles may be read.  "own" covariances come from the fp64 CPU oracle."""
import numpy as np
import pytest

import blocks_cases as bc
import blocks_exact as bx
import consistency_exact as cx
from eqf_vio_amd import consistency as cs


@pytest.fixture(scope="module")
def setup():
    """{case: (snapshot, operands, J blocks, 50-digit J)}: computed once, shared, never changed"""
    own = {N: bc.own_sigma_oracle(N) for N in sorted({c[0] for c in bc.CASES.values() if c[5] == "own"})}
    Jmp, out = {}, {}
    for name in bc.CPU_CASES:
        N = bc.CASES[name][0]
        snap = bc.snapshot(name, own.get(N))
        if N not in Jmp:
            Jmp[N] = cx.jacobian_mp(snap["origin"], snap["group"])
        ops = bc.operands(name, snap)
        J = cs.local_jacobian_blocks(snap["origin"], snap["group"])["lm"] if ops["local"] else None
        out[name] = (snap, ops, J, Jmp[N])
    return out


@pytest.fixture(scope="module")
def references(setup):
    out = {}
    for name, (snap, ops, J, Jmp) in setup.items():
        ref = bx.reference(snap["sigma"], ops, Jmp)
        out[name] = (ref, bx.bounds(ref))
    return out


def _host(snap, ops, J):
    o = dict(ops, R=bc.poison(ops["R"]))
    return cs.update_landmarks_host(snap["sigma"], o["idx"], o["H"], o["resid"], o["R"], J, lm_gate=o["lm_gate"])


def test_k_blocks_is_four_times_the_host_statements_worst_ratio(setup):
    worst, at = 0.0, None
    for name, (snap, ops, J, Jmp) in setup.items():
        ref = bx.reference(snap["sigma"], ops, Jmp)
        rt = bx.ratios(_host(snap, ops, J), ref, bx.bounds(ref, k_blocks=1.0))
        for k, v in rt.items():
            if v > worst:
                worst, at = v, (name, k)
    print(f"update_landmarks_host against the unit form: worst ratio {worst!r} at {at}; K_BLOCKS = {bx.K_BLOCKS!r}")
    assert np.isfinite(worst)
    assert 4.0 * worst <= bx.K_BLOCKS and bx.K_BLOCKS == 4.0 * bx.K_BLOCKS_MEASURED
    assert worst >= 0.5 * bx.K_BLOCKS_MEASURED, "K_BLOCKS_MEASURED is stale: renew it from the figure above"


def test_host_statement_inside_every_bound(setup, references):
    worst = {}
    for name, (snap, ops, J, Jmp) in setup.items():
        ref, bnd = references[name]
        assert bnd["validity"] <= bx.VALIDITY, (name, bnd["validity"])
        host = _host(snap, ops, J)
        assert host["info"] == 0 and np.array_equal(host["Sigma"], host["Sigma"].T), name
        for k, v in bx.ratios(host, ref, bnd).items():
            worst[k] = max(worst.get(k, 0.0), v)
            assert v <= 1.0, (name, k, v)
    print("worst |host - reference| / bound over the committed cases:", "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_cases_cover_what_they_claim_and_no_verdict_hangs_on_a_rounding(setup, references):
    orders = set()
    for name, (snap, ops, J, Jmp) in setup.items():
        ref = references[name][0]
        orders.add(ref["dof"])
        want = np.ones(len(ops["idx"]), dtype=np.int32)
        want[list(ops["gated"])] = 2
        if ops["absent"] is not None:
            want[ops["absent"]] = 0
        assert np.array_equal(ref["used"], want), name
        d2 = ref["d2"]
        assert np.all(d2[want == 1] < 40.0) and np.all(d2[want == 2] > 1e3) and np.all(np.isnan(d2[want == 0])), (name, d2)
    assert {1, 63, 64, 66, 129} <= orders, orders
    assert {c[1] for c in bc.CASES.values()} == {1, 2, 3}
    # the near-duplicate rows make S ill-conditioned
    ref = references["twins"][0]
    S = np.asarray(ref["S"], dtype=float)
    assert np.linalg.cond(S) > 1e7, np.linalg.cond(S)
    # a correlated R_k
    assert abs(setup["stereo66"][1]["R"][0][1, 0]) > 0


def test_every_injected_fault_leaves_a_bound_by_100(setup, references):
    table = {}
    for name, (snap, ops, J, Jmp) in setup.items():
        ref, bnd = references[name]
        honest = bx.model(snap["sigma"], dict(ops, R=bc.poison(ops["R"])), J)
        assert max(bx.ratios(honest, ref, bnd).values()) <= 1.0, name
        for fault in bx.FAULTS:
            mod = bx.model(snap["sigma"], dict(ops, R=bc.poison(ops["R"])), J, fault=fault)
            bad = max(bx.ratios(mod, ref, bnd).values())
            if bad >= 100.0:
                table.setdefault(fault, []).append((name, bad))
    print("fault -> cases on which some bound is left by >= 100 (count, first case, its ratio):")
    for fault in bx.FAULTS:
        hits = table.get(fault, [])
        print(f"  {fault:22s} {len(hits):3d}", (hits[0][0], f"{hits[0][1]:.3g}") if hits else "")
        assert hits, f"fault {fault} is not seen on any committed case"


def test_row_builders_linearise_their_measurements():
    rng = np.random.default_rng(1910)
    R21 = cs.quat_to_matrix(bc.Q_21)
    for _ in range(5):
        p = np.array([0.0, 0.0, 4.0]) + rng.standard_normal(3)
        e = 1e-6 * rng.standard_normal(3)
        # the second camera's bearing of the displaced point, in the chart around the predicted bearing
        y2 = R21.T @ (p + e - bc.T_21)
        H, r = cs.stereo_rows(p, bc.Q_21, bc.T_21, y2 / np.linalg.norm(y2))
        assert H.shape == (2, 3) and np.allclose(r, H @ e, rtol=0, atol=1e-10), (r, H @ e)
        H, r = cs.stereo_rows(p, bc.Q_21, bc.T_21, R21.T @ (p - bc.T_21) / np.linalg.norm(p - bc.T_21))
        assert np.abs(r).max() < 1e-15
        H, r = cs.depth_rows(p, np.linalg.norm(p + e))
        assert H.shape == (1, 3) and np.allclose(r, H @ e, rtol=0, atol=1e-10)
        H, r = cs.position_rows(p, p + e)
        assert np.array_equal(H, np.eye(3)) and np.allclose(r, e, rtol=0, atol=1e-15)
