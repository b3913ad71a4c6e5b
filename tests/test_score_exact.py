"""The reference and the bound of tests/score_exact.py on the CPU, for exactly the cases tests/test_gpu_score.py holds the device to
(tests/score_cases.py) -- no GPU.  States: the C++ fp64 oracle's; geometry in fp64: the numpy oracle's (oracle/eqf_numpy.py).

(a) the bound is a condition: on every committed case bound <= consistency_exact.VALIDITY (1 + |value|) for every statistic;
(b) the numpy statement consistency.score_vision_host (dense LAPACK Cholesky) and the numpy model of the kernels' 64-wide blocking
    (score_exact.model over mergecost_exact.blocked_cholesky) stay at ratio <= 1 on every committed case;
(c) the longdouble reference against the same in mpmath at 50 digits (|M| <= 17): within 1 % of the bound;
(d) eight injected faults, each leaving the bound on at least one case."""
import numpy as np
import pytest

import lie_edge_cases as ec
import score_cases as sc
import score_exact as sx
from eqf_vio_amd import consistency as cs
from oracle import eqf_numpy as en

_STATE = {}


def state(oracle_lib, b):
    """(snapshot, geometry at 50 digits, fp64 inputs C0 (N, 2, 3) and delta (N, 2), candidates), once per module"""
    if b not in _STATE:
        snap = sc.oracle_state(oracle_lib, b)
        d = sc.settings()
        y = sc.state_bearings(b, snap["ids"])
        geo = sx.geometry(snap, d, y)
        f = ec.numpy_filter(en, snap, d)
        N = len(snap["ids"])
        delta = np.asarray(en.output_coordinate_chart(en.output_group_action(f.X.inverse(), y), en.measure_system_state(f.xi0))).reshape(N, 2)
        C0 = cs.output_blocks(snap["origin"]["p"])
        _STATE[b] = (snap, geo, dict(C0=C0, delta=delta, r=float(d["measurementVariance"])), sc.candidates(b, snap["ids"]))
    return _STATE[b]


_REF = {}


def reference(oracle_lib, b, c):
    if (b, c) not in _REF:
        snap, geo, inp, cands = state(oracle_lib, b)
        ref = sx.reference(snap["sigma"], geo, inp["r"], cands[c][2])
        _REF[(b, c)] = (ref, sx.bounds(ref))
    return _REF[(b, c)]


CASES = [(b, c) for b in range(len(sc.STATE_N)) for c in range(sc.NCAND)]


def test_committed_cases_cover_the_sizes_and_meet_the_condition(oracle_lib):
    seen, worst = set(), 0.0
    for b, c in CASES:
        snap, _, _, cands = state(oracle_lib, b)
        ids, y, slots = cands[c]
        # the matched slots are what the state's own order gives for the candidate's ids
        assert slots == [s for s, i in enumerate(snap["ids"]) if int(i) in set(int(x) for x in ids)]
        assert np.all(np.diff(ids) > 0) and len(y) == len(ids)
        seen.add(len(slots))
        ref, bnd = reference(oracle_lib, b, c)
        q = sx.condition(ref, bnd) if slots else 0.0
        worst = max(worst, q)
        assert q <= 1.0, (b, c, q)
    assert set(sc.MATCHED) <= seen and 0 in seen
    assert list(state(oracle_lib, 1)[0]["ids"]) != sorted(state(oracle_lib, 1)[0]["ids"])   # a state whose ids are not ascending
    print(f"worst bound / (VALIDITY (1 + |value|)) over the committed cases: {worst:.3g}")


def test_statement_and_blocking_model_stay_inside_the_bound(oracle_lib):
    worst = {}
    for b, c in CASES:
        snap, _, inp, cands = state(oracle_lib, b)
        slots = cands[c][2]
        ref, bnd = reference(oracle_lib, b, c)
        for name, got in (("statement", cs.score_vision_host(snap["sigma"], inp["C0"], inp["delta"], inp["r"], slots)),
                          ("model", sx.model(snap["sigma"], inp["C0"], inp["delta"], inp["r"], slots))):
            assert got["dof"] == 2 * len(slots)
            r = sx.ratios(got, ref, bnd)
            for k, v in r.items():
                worst[(name, k)] = max(worst.get((name, k), 0.0), v)
                assert v <= 1.0, (name, b, c, k, v)
            if not slots:
                assert got["nis"] == 0.0 and got["logdet_S"] == 0.0 and got["loglik"] == 0.0
    print("worst ratio to the bound: " + "  ".join(f"{n} {k} {v:.3g}" for (n, k), v in sorted(worst.items())))


def test_longdouble_reference_against_mpmath(oracle_lib):
    done = 0
    for b, c in CASES:
        snap, geo, inp, cands = state(oracle_lib, b)
        slots = cands[c][2]
        if not slots or len(slots) > sx.MP_MAX_N:
            continue
        ref, bnd = reference(oracle_lib, b, c)
        share = sx.mp_share(ref, sx.reference(snap["sigma"], geo, inp["r"], slots, use_mp=True), bnd)
        assert share < 0.01, (b, c, share)
        done += 1
    assert done >= 5


FAULTS = ("r_missing", "unmatched_in_dof", "slot_off_by_one", "upper_block", "logdet_not_doubled", "log2pi_wrong_dof", "sigma_after_update",
          "candidate_order")


def faulty(snap, inp, cand, fault):
    """consistency.score_vision_host's record with one fault of FAULTS injected"""
    ids, _, slots = cand
    Sg, C0, delta, r = np.array(snap["sigma"], dtype=float), inp["C0"], inp["delta"], inp["r"]
    N = len(snap["ids"])
    if fault == "slot_off_by_one":
        slots = [min(s + 1, N - 1) for s in slots]
        slots = sorted(set(slots))
        delta = np.roll(delta, 1, axis=0)  # (the bearings stay with the entries they came with)
    if fault == "upper_block":  # the 3 x 3 block (s_b, s_a) read where (s_a, s_b) is meant: its transpose is the right one
        Sg = np.tril(Sg)
        for s in range(N):
            k = slice(11 + 3 * s, 14 + 3 * s)
            Sg[k, :11 + 3 * s] = np.concatenate([Sg[k, :11], np.concatenate([Sg[k, 11 + 3 * t:14 + 3 * t].T for t in range(s)], axis=1)
                                                 if s else np.zeros((3, 0))], axis=1)
        Sg = np.tril(Sg) + np.tril(Sg, -1).T
    if fault == "sigma_after_update":  # Sigma+ of the update with every landmark of the state in place of Sigma
        full = cs.score_vision_host(Sg, C0, delta, r, list(range(N)))
        Cd = np.zeros((2 * N, 11 + 3 * N))
        for i in range(N):
            Cd[2 * i:2 * i + 2, 11 + 3 * i:14 + 3 * i] = C0[i]
        Y = np.linalg.solve(np.linalg.cholesky(full["S"]), Cd @ Sg)
        Sg = Sg - Y.T @ Y
    if fault == "candidate_order":  # the slots in the state's order, the bearings left in the order of the candidate's ids: S is invariant
        by_id = sorted(slots, key=lambda s: int(snap["ids"][s]))   # under a symmetric permutation, what moves is the delta paired with each row
        d2 = delta.copy()
        for k, s in enumerate(slots):
            d2[s] = delta[by_id[k]]
        delta = d2
    out = cs.score_vision_host(Sg, C0, delta, r, slots)
    m = out["dof"]
    if fault == "r_missing" and m:
        S = out["S"].copy()
        S[0, 0] -= r
        S[1, 1] -= r
        L = np.linalg.cholesky(S)
        dm = np.concatenate([delta[s] for s in slots])
        z = np.linalg.solve(L, dm)
        out["nis"], out["logdet_S"] = float(z @ z), 2.0 * float(np.sum(np.log(np.diag(L))))
        out["loglik"] = -0.5 * (out["nis"] + out["logdet_S"] + m * np.log(2 * np.pi))
        out["nis_lm"][0] = cs.gate_distance(S[0:2, 0:2], dm[0:2])
    if fault == "unmatched_in_dof":
        out["dof"] = 2 * len(ids)
        out["loglik"] = -0.5 * (out["nis"] + out["logdet_S"] + out["dof"] * np.log(2 * np.pi))
    if fault == "logdet_not_doubled":
        out["logdet_S"] = 0.5 * out["logdet_S"]
        out["loglik"] = -0.5 * (out["nis"] + out["logdet_S"] + m * np.log(2 * np.pi))
    if fault == "log2pi_wrong_dof":
        out["loglik"] = -0.5 * (out["nis"] + out["logdet_S"] + (m // 2) * np.log(2 * np.pi))
    return out


def test_injected_faults_leave_the_bound(oracle_lib):
    caught = {f: [] for f in FAULTS}
    for b, c in CASES:
        snap, _, inp, cands = state(oracle_lib, b)
        if not cands[c][2]:
            continue
        ref, bnd = reference(oracle_lib, b, c)
        for f in FAULTS:
            try:
                got = faulty(snap, inp, cands[c], f)
            except np.linalg.LinAlgError:
                caught[f].append((b, c, "not positive definite"))
                continue
            if len(got["nis_lm"]) != len(bnd["nis_lm"]):
                caught[f].append((b, c, "another number of entries"))
                continue
            r = sx.ratios(got, ref, bnd)
            if got["dof"] != ref["m"] or max(r.values()) > 1.0:
                caught[f].append((b, c, max(r.values())))
    for f in FAULTS:
        print(f"{f}: leaves the bound on {len(caught[f])} of {sum(1 for b, c in CASES if state(oracle_lib, b)[3][c][2])} cases")
        assert caught[f], f
    # the order fault can only show where the state's ids are not ascending
    assert all(b == 1 for b, _, _ in caught["candidate_order"])
