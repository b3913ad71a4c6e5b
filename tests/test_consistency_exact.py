"""CPU side of tests/test_gpu_consistency_exact.py: the constants of tests/consistency_cases.py against their yardstick, the bounds of
tests/consistency_exact.py held against plain fp64 restatements on every committed case, and injected faults that must leave them.  No GPU."""
import time

import numpy as np
import pytest

import scipy.linalg

import chol_bounds as cb
import consistency_cases as cc
import consistency_exact as cx
import lie_edge_cases as ec
import riccati_cases as rc
import update_cases as uc
import update_exact as ux
from consistency_helpers import chart_jacobian_blocks_oracle, innovation_reference
from oracle import eqf_numpy as en


def _oracle_blocks(snap):
    N = len(snap["ids"])
    J = chart_jacobian_blocks_oracle(snap["origin"], snap["group"], snap["ids"])
    return dict(G=J[6:8, 6:8].copy(), RAt=J[8:11, 8:11].copy(),
                lm=np.array([J[11 + 3 * i:14 + 3 * i, 11 + 3 * i:14 + 3 * i] for i in range(N)]).reshape(N, 3, 3))


@pytest.fixture(scope="module")
def master():
    """{theta: (snapshot of the master state, its 50-digit J blocks, the numpy oracle's fp64 J blocks)}"""
    out = {}
    t0 = time.time()
    for th in cc.LOCAL_THETAS:
        s = cc.local_state(cc.LOCAL_MASTER, th)
        out[th] = (s, cx.jacobian_mp(s["origin"], s["group"]), _oracle_blocks(s))
    print(f"A: 50-digit J of {len(out)} master states of {cc.LOCAL_MASTER} landmarks in {time.time() - t0:.2f} s")
    return out


@pytest.fixture(scope="module")
def own_sigma():
    """{N: the C++ oracle's Sigma after five vision frames} -- an INPUT of family a, nothing of it is asserted."""
    from eqf_vio_amd import synth
    from oracle import binding as ob

    out = {}
    for N in sorted({n for n in cc.LOCAL_SIZES if n <= cc.LOCAL_OWN_MAX} | set(cc.NEES_SIZES)):
        st = synth.make_stream(N, duration=0.4)
        fo = ob.OracleFilter(cc.settings())
        seen = 0
        for kind, k in st.events():
            if kind == "imu":
                r = st.imu[k]
                fo.processIMUData(r[0], r[1:4], r[4:7])
            else:
                fo.processVisionData(st.vision_stamps[k], st.ids, st.bearings[k])
                seen += 1
                if seen == 5:
                    break
        out[N] = fo.stateCovariance()
    return out


def test_the_states_are_what_the_issue_asks_for(master):
    for th, (s, Jmp, _) in master.items():
        g = s["group"]
        assert abs(2 * np.arccos(g["Aq"][0]) - 2.5) < 1e-12
        ang = 2 * np.arccos(np.clip(np.abs(g["Qq"][:, 0]), 0, 1))
        assert ang.max() <= np.pi - 0.1 and ang.max() > 3.0 and ang.min() < 0.05
        assert 0.05 <= g["Qa"].min() < 0.06 and 18.0 < g["Qa"].max() <= 20.0
        assert abs(Jmp["theta0"] / th - 1) < 1e-9 and Jmp["thetaHat"] > 0.5  # eta0 is theta from the pole, etaHat far from it
        assert th > 1e3 * 1e-8


def test_K_J_against_its_yardstick(master):
    """The numpy oracle's J blocks against the 50-digit ones over the committed states: ratio <= stored, so K_J = 4 x stored cannot drift."""
    worst = {k: 0.0 for k in cc.ORACLE_J}
    for th, (s, Jmp, ob) in master.items():
        r = cx.jacobian_ratios(ob, Jmp)
        print(f"A theta={th:g}: numpy oracle J in units of u max|block| (G: u / theta^2): " + "  ".join(f"{k} {v!r}" for k, v in r.items()))
        for k in worst:
            worst[k] = max(worst[k], r[k])
    print("A measured K_J yardstick " + "  ".join(f"{k} {v!r} (stored {cc.ORACLE_J[k]!r}, K_J {cc.K_J[k]:.3f})" for k, v in worst.items()))
    assert all(worst[k] <= cc.ORACLE_J[k] for k in worst), worst
    assert all(cc.K_J[k] == 4 * cc.ORACLE_J[k] for k in worst)


def _sub(blocks, N):
    return dict(G=blocks["G"], RAt=blocks["RAt"], lm=blocks["lm"][:N])


def _restated(blocks, S, N):
    """J Sigma J^T in plain fp64 with the numpy oracle's J (numpy's matmul: another order of summation than the kernel's)"""
    J = cx.dense_J(_sub(blocks, N), N)
    return J @ S @ J.T


LOCAL_FAULTS = ("J_i transposed", "Sigma_Jb read as Sigma_bJ^T", "lane 256 takes J of lane 0", "row chunk 16 takes J of row 0", "scale a_i not inverted")


def _faulty(blocks, S, N, fault):
    b = dict(G=blocks["G"], RAt=blocks["RAt"], lm=blocks["lm"][:N].copy())
    if fault == "J_i transposed":
        b["lm"][N - 1] = b["lm"][N - 1].T.copy()
    elif fault == "scale a_i not inverted":
        i = min(N - 1, 16)
        b["lm"][i] = b["lm"][i] * (np.linalg.norm(b["lm"][i], axis=1)[0] ** -2)
    J = cx.dense_J(b, N)
    if fault == "Sigma_Jb read as Sigma_bJ^T":
        S = S.copy()
        S[11:, :11] = S[:11, 11:].T
    out = J @ S @ J.T
    if fault == "lane 256 takes J of lane 0" and N > 256:
        Jw = J.copy()
        Jw[11 + 768:14 + 768, 11 + 768:14 + 768] = J[11:14, 11:14]
        out[:, 11 + 768:14 + 768] = (J @ S @ Jw.T)[:, 11 + 768:14 + 768]
    if fault == "row chunk 16 takes J of row 0" and N > 16:
        Jw = J.copy()
        Jw[11 + 48:14 + 48, 11 + 48:14 + 48] = J[11:14, 11:14]
        out[11 + 48:14 + 48, 11:] = (Jw @ S @ J.T)[11 + 48:14 + 48, 11:]
    return out


def test_part_A_bound_holds_for_a_plain_fp64_restatement_and_sees_faults(master, own_sigma):
    worst, ratio_old, faults = {}, [], {f: 0.0 for f in LOCAL_FAULTS}
    faults_old = {f: 0.0 for f in LOCAL_FAULTS}
    t0 = time.time()
    for N in cc.LOCAL_SIZES:
        for th in cc.LOCAL_THETAS:
            s, Jmp, ob = master[th]
            snap = cc.local_state(N, th)
            for fam in cc.local_families(N):
                S = cc.local_sigma(snap, fam, own_sigma.get(N))
                ref = cx.sigma_local_reference(Jmp, S)
                bound, old = cx.sigma_local_bound(Jmp, S, cc.K_J)
                r, nz = cx.bound_ratio(_restated(ob, S, N), ref, bound)
                assert nz == 0, (N, th, fam, nz)
                worst[fam] = max(worst.get(fam, 0.0), r)
                ratio_old.append(float(np.median(bound[old > 0] / old[old > 0])))
                for f in LOCAL_FAULTS:
                    got = _faulty(ob, S, N, f)
                    rf, nzf = cx.bound_ratio(got, ref, bound)
                    ro, nzo = cx.bound_ratio(got, ref, old)
                    faults[f] = max(faults[f], np.inf if nzf else rf)
                    faults_old[f] = max(faults_old[f], np.inf if nzo else ro)
    print(f"A: {time.time() - t0:.1f} s for every case")
    print("A numpy restatement / bound, worst per family: " + "  ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    print(f"A new bound / (256 u) bound, median per case: {min(ratio_old):.4f} .. {max(ratio_old):.4f}")
    print("A fault table (worst ratio over the cases: new bound | 256 u bound):")
    for f in LOCAL_FAULTS:
        print(f"    {f:36s} {faults[f]:12.4g} | {faults_old[f]:12.4g}")
    assert all(v <= 1.0 for v in worst.values()), worst
    assert all(v >= 100.0 for v in faults.values()), faults


# ---- part B ---------------------------------------------------------------------------------------------------------------------------------
NEES_FAULTS = ("dropped trailing tile", "stale pad row", "error vectors miss the last ragged column", "one k-step of four dropped",
               "W_j transposed", "min_pivot includes the pad", "draw with the strict lower triangle")


def model_nees(A, E, first, fault=None):
    """k_factor_diag / _panel / _trail and k_nees_tail composed in numpy fp64 from chol_bounds.model_chol16 (64-wide block columns, 16-wide stages) and
    model_trsm16 (the explicit inverses W_j), on the PADDED matrix: the pad row is a row of the identity, the error vectors are more rows
    under the panel.  Returns (nees (k,), logdet, min_pivot, the padded factor)."""
    pad = cx.pad_index(first)
    Ap = cx.embed(np.asarray(A, dtype=np.float64), pad)
    k, m = len(E), len(Ap)
    Z = np.zeros((k, m))
    Z[:, [i for i in range(m) if i != pad]] = E
    if fault == "stale pad row" and pad >= 0:
        Ap[pad, :pad] = 0.37
        Ap[pad + 1:, pad] = 0.37
        Ap[:pad, pad] = 0.37
        Z[:, pad] = 0.37
    Lp = np.zeros((m, m))
    nb = -(-m // 64)
    edge = lambda K: (64 * K, min(m, 64 * K + 64))  # noqa: E731
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for K in range(nb):
            c0, c1 = edge(K)
            Lkk, Ws = cb.model_chol16(Ap[c0:c1, c0:c1], block=64)
            Lp[c0:c1, c0:c1] = Lkk
            tw = "transpose_w" if fault == "W_j transposed" and K == 0 else None
            if c1 < m:
                Lp[c1:, c0:c1] = cb.model_trsm16(Lkk, Ws, Ap[c1:, c0:c1], right=True, fault=tw)
            Z[:, c0:c1] = cb.model_trsm16(Lkk, Ws, Z[:, c0:c1], right=True)
            for R in range(K + 1, nb):
                r0, r1 = edge(R)
                for C in range(K + 1, R + 1):
                    q0, q1 = edge(C)
                    if fault == "dropped trailing tile" and K == 0 and R == nb - 1 and C == (1 if nb >= 3 else R):
                        continue
                    P = Lp[r0:r1, c0:c1]
                    if fault == "one k-step of four dropped" and K == 0 and R == C == nb - 1:
                        P = P.copy()
                        P[:, 4:8] = 0.0
                    Ap[r0:r1, q0:q1] -= P @ Lp[q0:q1, c0:c1].T
            for C in range(K + 1, nb):
                q0, q1 = edge(C)
                if fault == "error vectors miss the last ragged column" and C == nb - 1 and m % 64:
                    continue
                Z[:, q0:q1] -= Z[:, c0:c1] @ Lp[q0:q1, c0:c1].T
        d = np.diag(Lp)
        piv = d if (fault == "min_pivot includes the pad" or pad < 0) else np.delete(d, pad)
        return (Z * Z).sum(axis=1), 2 * np.log(np.delete(d, pad) if pad >= 0 else d).sum(), (piv ** 2).min(), Lp


def model_draw(Lp, Zin, first, scale, fault=None):
    """k_sample_trmm in numpy fp64: E[:, C] = sum_{K <= C} Z[:, K] L[C, K]^T over 64-wide block columns, K ascending, then the scale"""
    pad = cx.pad_index(first)
    m, k = len(Lp), len(Zin)
    keep = [i for i in range(m) if i != pad]
    Z = np.zeros((k, m))
    Z[:, keep] = Zin
    out = np.zeros((k, m))
    for C in range(-(-m // 64)):
        q0, q1 = 64 * C, min(m, 64 * C + 64)
        for K in range(C + 1):
            c0, c1 = 64 * K, min(m, 64 * K + 64)
            blk = Lp[q0:q1, c0:c1]
            if K == C:
                blk = np.tril(blk, -1 if fault == "draw with the strict lower triangle" else 0)
            out[:, q0:q1] += Z[:, c0:c1] @ blk.T
    return scale * out[:, keep]


@pytest.fixture(scope="module")
def nees_cases(master, own_sigma):
    """[(label, N, first, nrhs, nsamp, scale, FactorRef, E, Z)] over every committed case of part B, A restated on the CPU (local: with the
    numpy oracle's J in plain fp64), and the measured c_log."""
    s, Jmp, ob = master[cc.NEES_THETA]
    raw, pivots = [], []
    t0 = time.time()
    for N in cc.NEES_SIZES:
        J = cx.dense_J(_sub(ob, N), N)
        for fam, local, first, nrhs, nsamp, scale in cc.nees_plan(N):
            S = cc.nees_sigma(N, fam, own_sigma.get(N))
            A = cx.cut(J @ S @ J.T if local else S, first)
            ref = cx.FactorRef(A, first, cc.C_LOG)
            E = cc.nees_vectors(N, fam, local, first, nrhs, "err")[:, first:]
            Z = cc.nees_vectors(N, fam, local, first, nsamp, "z")[:, first:]
            raw.append((f"N={N} {fam} local={local} first={first}", N, first, nrhs, nsamp, scale, ref, E, Z))
            pivots.append(np.diag(ref.L).astype(np.float64))
    print(f"B: {len(raw)} references in {time.time() - t0:.1f} s; orders {sorted({c[6].n for c in raw})}")
    return raw, cx.log_error_units(np.concatenate(pivots))


def test_c_log_against_its_yardstick(nees_cases):
    _, measured = nees_cases
    print(f"B measured c_log yardstick {measured!r} (stored {cc.ORACLE_LOG!r}, c_log {cc.C_LOG})")
    assert measured <= cc.ORACLE_LOG and cc.C_LOG == 4 * cc.ORACLE_LOG


def test_every_committed_matrix_licenses_first_order(nees_cases):
    cases, _ = nees_cases
    worst = max(c[6].validity for c in cases)
    print(f"B: largest max(|L^-1| E1 |L^-T|) over the committed cases {worst:.3e} (condition: <= {cx.VALIDITY:g}); "
          f"kappa_2 {min(c[6].kappa for c in cases):.2e} .. {max(c[6].kappa for c in cases):.2e}")
    assert all(c[6].validity <= cx.VALIDITY for c in cases), [(c[0], c[6].validity) for c in cases if c[6].validity > cx.VALIDITY]
    small = [c for c in cases if c[6].n <= cx.MP_MAX_ORDER]
    assert len(small) >= 6
    share = max(c[6].mp_share(c[7]) for c in small)
    print(f"B: longdouble against mpmath on the {len(small)} cases of order <= {cx.MP_MAX_ORDER}: {share:.2e} of the bound")
    assert share <= 0.01


def _all_ratios(ref, res, E, draw, Z, scale):
    r = cx.nees_ratios(ref, res[0], res[1], res[2], E)
    d = cx.draw_ratios(ref, draw, Z, scale)
    new = max(r["nees"], r["logdet"], r["min_pivot"], d["draw"])
    old = max(r["old"]["nees"], r["old"]["logdet"], r["old"]["min_pivot"], d["old"])
    return new, (np.inf if np.isnan(old) else old), r, d


def test_part_B_bounds_hold_for_lapack_and_the_blocked_model_and_see_faults(nees_cases):
    cases, _ = nees_cases
    worst = {"lapack": {}, "model": {}}
    table = {f: [0.0, 0.0, ""] for f in NEES_FAULTS}
    vs_old = {"nees": [], "logdet": [], "draw": []}
    t0 = time.time()
    for label, N, first, nrhs, nsamp, scale, ref, E, Z in cases:
        Ll = np.linalg.cholesky(ref.A)
        zl = scipy.linalg.solve_triangular(Ll, E.T, lower=True)
        lap = ((zl * zl).sum(axis=0), 2 * np.log(np.diag(Ll)).sum(), (np.diag(Ll) ** 2).min())
        _, _, r, d = _all_ratios(ref, lap, E, scale * (Z @ Ll.T), Z, scale)
        res = model_nees(ref.A, E, first)
        _, _, rm, dm = _all_ratios(ref, res, E, model_draw(res[3], Z, first, scale), Z, scale)
        for who, rr, dd in (("lapack", r, d), ("model", rm, dm)):
            for k in ("nees", "logdet", "min_pivot"):
                worst[who][k] = max(worst[who].get(k, 0.0), rr[k])
            worst[who]["draw"] = max(worst[who].get("draw", 0.0), dd["draw"])
        vs_old["nees"].append(r["bound_vs_old"]["nees"])
        vs_old["logdet"].append(r["bound_vs_old"]["logdet"])
        vs_old["draw"].append(d["bound_vs_old"])
        for f in NEES_FAULTS:
            if f == "draw with the strict lower triangle":
                fres, fdraw = res, model_draw(res[3], Z, first, scale, fault=f)
            else:
                fres = model_nees(ref.A, E, first, fault=f)
                fdraw = model_draw(res[3], Z, first, scale)
            new, old, _, _ = _all_ratios(ref, fres, E, fdraw, Z, scale)
            if new > table[f][0]:
                table[f] = [new, old, label]
    print(f"B: LAPACK, the model and {len(NEES_FAULTS)} faults on {len(cases)} cases in {time.time() - t0:.1f} s")
    for who in worst:
        print(f"B {who:6s} / bound, worst over the cases: " + "  ".join(f"{k} {v:.4f}" for k, v in worst[who].items()))
    print("B new bound / (n u kappa_2) yardstick over the cases: " + "  ".join(f"{k} {min(v):.2e} .. {max(v):.2e}" for k, v in vs_old.items()))
    print("B fault table (worst ratio over the cases under the new bound | the same result under n u kappa_2 | case):")
    for f in NEES_FAULTS:
        print(f"    {f:44s} {table[f][0]:12.4g} | {table[f][1]:12.4g} {'(old yardstick passes it)' if table[f][1] <= 1 else ''} | {table[f][2]}")
    assert all(v <= 1.0 for who in worst for v in worst[who].values()), worst
    assert all(table[f][0] > 1.0 for f in NEES_FAULTS), table


# ---- part C ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def innov_refs(oracle_lib):
    """{(N, family): (S0, call, Case, ref, bounds, reference statistics, their bounds)} from the C++ oracle's snapshot (an input)"""
    out, cases, snaps = {}, {}, {}
    for N, fam in cc.innov_cases():
        t0 = time.time()
        if N not in snaps:
            snaps[N] = rc.oracle_snapshot(oracle_lib, N)
        call = uc.vision_call(N, fam)
        ck = (N, "e" if fam == "e" else "a")
        if ck not in cases:
            cases[ck] = ux.Case(snaps[N], uc.settings(), call[0], call[2])
        S0 = uc.sigma_family(snaps[N], fam)
        ref, bd = cases[ck].reference(S0)
        val, bnd = cx.innovation_stats_reference(ref, bd, cc.C_LOG)
        out[(N, fam)] = (snaps[N], S0, call, cases[ck], ref, bd, val, bnd)
        if N >= 130:
            print(f"C: reference of N={N} family {fam} in {time.time() - t0:.1f} s")
    return out


def _stats_of(S, delta):
    r = innovation_reference(S, delta)
    m = r["m"]
    r["loglik"] = -0.5 * (r["nis"] + r["logdet_S"] + m * cx.LOG_2PI)
    return r


def test_part_C_bounds_hold_for_the_numpy_oracle(innov_refs):
    worst, cec = {}, 0.0
    for (N, fam), (snap, S0, (stamp, ids, y), case, ref, bd, val, bnd) in innov_refs.items():
        f = ec.numpy_filter(en, dict(snap, sigma=S0), uc.settings())
        f.processVisionData(stamp, ids, y)
        r = cx.innovation_ratios(_stats_of(f.last["S"], f.last["delta"]), val, bnd)
        print(f"C N={N} family {fam}: numpy oracle / bound " + "  ".join(f"{k} {v:.4f}" for k, v in r.items())
              + f" | relative bounds nis {bnd['nis'] / float(val['nis']):.1e} logdet_S {bnd['logdet_S']:.1e} (absolute)"
              f" nis_lm {np.max(bnd['nis_lm'] / val['nis_lm'].astype(float)):.1e}")
        w = worst.setdefault(fam, {})
        for k, v in r.items():
            w[k] = max(w.get(k, 0.0), v)
        P = bd["parts"]
        cec = max(cec, max(float(np.max(np.abs(P["CEC"][2 * i:2 * i + 2, 2 * i:2 * i + 2]) / P["dS"][2 * i:2 * i + 2, 2 * i:2 * i + 2])) for i in range(N)))
    for fam, w in worst.items():
        print(f"C family {fam}: numpy oracle / bound, worst over the sizes: " + "  ".join(f"{k} {v:.4f}" for k, v in w.items()))
    print(f"C: largest (|C| E_ric |C|^T)_ii / dS_ii over the landmarks of every case: {cec:.3g}")
    assert all(v <= 1.0 for w in worst.values() for v in w.values()), worst


def test_part_C_longdouble_reference_against_fifty_digits(innov_refs):
    share = 0.0
    for (N, fam), (snap, S0, call, case, ref, bd, val, bnd) in innov_refs.items():
        if N > ux.MP_MAX_N:
            continue
        rm = case.reference_mp(S0)
        z, L, S, delta = rm["z"], rm["L"], rm["S"], rm["delta"]
        nis = sum(v * v for v in z)
        logdet = 2 * sum(cx.mp.log(L[i, i]) for i in range(2 * N))
        tomp = lambda x: cx.mpf(float(x)) + cx.mpf(float(x - cx.LD(float(x))))  # noqa: E731
        share = max(share, float(abs(nis - tomp(val["nis"])) / cx.mpf(bnd["nis"])), float(abs(logdet - tomp(val["logdet_S"])) / cx.mpf(bnd["logdet_S"])))
        for i in range(N):
            a, b, c = S[2 * i, 2 * i], S[2 * i + 1, 2 * i], S[2 * i + 1, 2 * i + 1]
            d0, d1 = delta[2 * i], delta[2 * i + 1]
            q = (c * d0 * d0 - 2 * b * d0 * d1 + a * d1 * d1) / (a * c - b * b)
            share = max(share, float(abs(q - tomp(val["nis_lm"][i])) / cx.mpf(float(bnd["nis_lm"][i]))))
    print(f"C: longdouble against mpmath for N <= {ux.MP_MAX_N}: {share:.2e} of the bound")
    assert share <= 0.01


def test_one_percent_of_the_measurement_variance_leaves_every_bound_a_hundredfold(innov_refs):
    """From the reference alone: the same call with measurementVariance x 1.01 moves every statistic by >= 100 bounds."""
    least = {}
    for (N, fam), (snap, S0, call, case, ref, bd, val, bnd) in innov_refs.items():
        ref2 = ux.update_reference(ref["S1"], case.geo, 1.01 * case.r)
        val2, _ = cx.innovation_stats_reference(ref2, bd, cc.C_LOG)
        r = cx.innovation_ratios({k: val2[k] for k in val2}, val, bnd)
        lm = np.abs(val2["nis_lm"] - val["nis_lm"]).astype(float) / bnd["nis_lm"]
        r["nis_lm"] = float(lm.min())  # (every landmark, not the best one)
        for k, v in r.items():
            if v < least.get(k, (np.inf,))[0]:
                least[k] = (v, N, fam)
    print("C measurementVariance + 1 %: least move in units of the bound " + "  ".join(f"{k} {v[0]:.3g} (N={v[1]} {v[2]})" for k, v in least.items()))
    assert all(v[0] >= 100.0 for v in least.values()), least
