"""The Riccati step's entry-by-entry reference and bound (tests/riccati_exact.py) on the CPU, on exactly the states, Sigma families, sizes and
IMU calls of tests/test_gpu_riccati.py (tests/riccati_cases.py; the state comes from the C++ oracle here, from the device there).

(a) the 50-digit blocks against oracle/eqf_numpy.py's matrices: the oracle's error in units of u max|block| IS the measurement behind tau_blk;
    it is printed, and asserted to be what riccati_exact.TAU_MEASURED records.
(b) a CONDITION of the bound: two fp64 numpy restatements of the step stay inside it (ratio <= 1) on every case the GPU tests use, K-step cases
    included -- the dense one of oracle/eqf_numpy.py:844-850 and a structured one in the kernels' block order,
    M D_j^T + G_i L_j^T + T B_i R B_j^T with M = D_i S_ij + L_i Sigma_bj and G_i = L_i Sigma_bb + D_i Sigma_ib (csrc/eqf_tile.hpp:79-113) -- and a
    float32 run of the structured one stays inside the fp32 bound.  Were one outside, the count k would be wrong: that is what would be fixed.
(c) the bound must SEE a fault.  Deliberate changes of the structured restatement (MUTATIONS) each leave the bound on the Sigma families named
    for them, by factors of 1e6 .. 1e14 for the structural ones.  Measured at N = 33 on the filter's own Sigma,  rel_fro  of the faulty Sigma'
    against the reference -- what the single-step gate  rel_fro < 1e-12  of test_single_propagate_and_single_update_from_an_injected_state and
    the  rel_fro < 1e-9  gates between routes look at:
        Lw transposed on one landmark 4.9e-5, a neighbour's D at the tile edge 1.1e-4 / 1.6e-4, dt for T 8.3e-4, Avg dropped 1.4e-3, wrong
        sign of -T B 1.1e-3: caught by either gate.  Point noise missing on one landmark 1.2e-8 and B R B^T scaled by T^2 3.0e-8: caught at
        1e-12, NOT at 1e-9.  One entry of -T R_A off by 1e3 u relative: 1.6e-16, and off by 1e-8 relative (1e8 u): 1e-13 -- both PASS 1e-12,
        while the bound sees them at ratio 4 and 4e5.
    Sigma carries entries from 5000 down to 1e-8, and 1e-12 |Sigma|_F in a base-block entry is a relative error of 1e-6 and worse there: that is
    the gap this file and tests/test_gpu_riccati.py close.  The test asserts every "caught" and, where the table says so, the "passes 1e-12".
    The faults live here, not in the library."""
import numpy as np
import pytest

import lie_edge_cases as ec
import riccati_cases as rc
import riccati_exact as rx
from helpers import rel_fro
from oracle import eqf_numpy as en

_SNAP, _STEPS, _ORACLE = {}, {}, {}


def snapshot(oracle_lib, N):
    if N not in _SNAP:
        _SNAP[N] = rc.oracle_snapshot(oracle_lib, N)
    return _SNAP[N]


def call_sets(N):
    """[(name, families, calls of a snapshot)] of one size: the single call (families a, b, c), the call after the gap (d), the burst of four."""
    sets = [("one", ("a", "b", "c"), lambda s: rc.one_call(s, "a")), ("gap", ("d",), lambda s: rc.one_call(s, "d"))]
    if N in rc.KSTEP or N in [n for n, _ in rc.TILED]:
        sets.append(("four", rc.FAMILIES_FOUR, rc.four_calls))
    return sets


def exact_steps(oracle_lib, N, name, calls):
    if (N, name) not in _STEPS:
        _STEPS[(N, name)] = rx.exact_steps(snapshot(oracle_lib, N), rc.settings(), calls)
    return _STEPS[(N, name)]


def oracle_steps(oracle_lib, N, name, calls):
    """oracle/eqf_numpy.py's (A0t, Bt, T) of every integrating call, the filter advanced by its own processIMUData in between."""
    if (N, name) not in _ORACLE:
        snap = dict(snapshot(oracle_lib, N))
        snap["sigma"] = np.eye(11 + 3 * N)  # (the oracle's own dense step is not what is looked at here)
        f = ec.numpy_filter(en, snap, rc.settings())
        out = []
        for stamp, w, a in calls:
            dt = stamp - f.currentTime
            if f.currentTime >= 0 and dt > 0:  # VIOFilter.cpp:147-155, :169-170
                T = f.accumulatedTime + dt
                mean = (f.accumulatedVelocity + f.currentVelocity * dt) * (1.0 / T)
                out.append((en.eqf_state_matrix_A(f.X, f.xi0, mean), en.eqf_input_matrix_B(f.X, f.xi0), T))
            f.processIMUData(en.IMUVelocity(stamp, w, a))
        _ORACLE[(N, name)] = out
    return _ORACLE[(N, name)]


# ---- the two restatements ------------------------------------------------------------------------------------------------------------------
def dense_step(A0t, Bt, T, d, S):
    """oracle/eqf_numpy.py:832-850, verbatim but for the names."""
    n = S.shape[0]
    PMat = np.eye(n)
    PMat[0:3, 0:3] *= d["biasOmegaProcessVariance"]
    PMat[3:6, 3:6] *= d["biasAccelProcessVariance"]
    PMat[6:8, 6:8] *= d["gravityProcessVariance"]
    PMat[8:11, 8:11] *= d["velocityProcessVariance"]
    PMat[11:, 11:] *= d["pointProcessVariance"]
    R = np.eye(6)
    R[0:3, 0:3] *= d["velOmegaVariance"]
    R[3:6, 3:6] *= d["velAccelVariance"]
    A0tBiased = np.zeros((n, n))
    A0tBiased[6:, 6:] = A0t
    A0tBiased[6:, 0:6] = -Bt
    F = np.eye(n) + A0tBiased * T
    BtBiased = np.zeros((n, 6))
    BtBiased[6:, :] = Bt
    return T * (PMat + BtBiased @ R @ BtBiased.T) + F @ S @ F.T


def structured_step(sc, Bt, T, d, S, dtype=np.float64, Dcol=None, Lwcol=None, pointvar=None, TB=None):
    """The step in the kernels' block order from the scaled blocks sc (riccati_exact.scaled_from_oracle) and the plain Bt, in `dtype`.
    Faults: Dcol / Lwcol replace D / Lw in the COLUMN role (the right factor D_j^T / L_j^T), pointvar the diagonal point noise per landmark,
    TB the factor of B R B^T (T when correct)."""
    f = lambda x: np.asarray(x, dtype=dtype)  # noqa: E731
    N = len(sc["D"])
    n = 11 + 3 * N
    S, Tn = f(S), dtype(T)
    TB = Tn if TB is None else dtype(TB)
    D = f(sc["D"]).reshape(N, 3, 3)
    L = np.zeros((N, 3, 11), dtype=dtype)
    L[:, :, 0:3], L[:, :, 8:11] = f(sc["Lw"]).reshape(N, 3, 3), f(sc["Lv"]).reshape(N, 3, 3)
    Dc = D if Dcol is None else f(Dcol)
    Lc = L.copy()
    if Lwcol is not None:
        Lc[:, :, 0:3] = f(Lwcol)
    Fbb = np.eye(11, dtype=dtype)
    Fbb[6:8, 0:3], Fbb[8:11, 0:3], Fbb[8:11, 3:6], Fbb[8:11, 6:8] = f(sc["TBg"]), f(sc["TBvw"]), f(sc["TRA"]), f(sc["TAvg"])
    Bb = np.zeros((11, 6), dtype=dtype)
    Bb[6:11] = f(Bt[0:5])
    Bi = f(np.array([Bt[5 + 3 * i:8 + 3 * i, 0:3] for i in range(N)])).reshape(N, 3, 3)
    Rw = f([d["velOmegaVariance"]] * 3)
    R6 = f([d["velOmegaVariance"]] * 3 + [d["velAccelVariance"]] * 3)
    Pb = f([d["biasOmegaProcessVariance"]] * 3 + [d["biasAccelProcessVariance"]] * 3 + [d["gravityProcessVariance"]] * 2 + [d["velocityProcessVariance"]] * 3)
    pv = f(np.full(N, d["pointProcessVariance"]) if pointvar is None else pointvar)
    Sbb, SbJ, SIb, SIJ = S[:11, :11], S[:11, 11:].reshape(11, N, 3), S[11:, :11].reshape(N, 3, 11), S[11:, 11:].reshape(N, 3, N, 3)
    out = np.zeros((n, n), dtype=dtype)
    M = np.einsum("iab,ibjc->iajc", D, SIJ) + np.einsum("iak,kjc->iajc", L, SbJ)
    G = np.einsum("iak,kl->ial", L, Sbb) + np.einsum("iab,ibl->ial", D, SIb)
    LL = np.einsum("iajc,jdc->iajd", M, Dc) + np.einsum("ial,jdl->iajd", G, Lc) + TB * np.einsum("iac,c,jdc->iajd", Bi, Rw, Bi)
    for i in range(N):
        LL[i, :, i, :] += np.diag(np.full(3, Tn * pv[i]))
    out[11:, 11:] = LL.reshape(3 * N, 3 * N)
    FS, FSJ = Fbb @ Sbb, np.einsum("kl,ljc->kjc", Fbb, SbJ)
    bJ = np.einsum("kl,jdl->kjd", FS, Lc) + np.einsum("kjc,jdc->kjd", FSJ, Dc) + TB * np.einsum("kc,c,jdc->kjd", Bb[:, 0:3], Rw, Bi)
    out[:11, 11:] = bJ.reshape(11, 3 * N)
    out[11:, :11] = out[:11, 11:].T
    out[:11, :11] = FS @ Fbb.T + Tn * np.diag(Pb) + TB * (Bb * R6) @ Bb.T
    return out


def run_restatement(kind, osteps, d, S0, dtype=np.float64):
    S = np.array(S0, dtype=float)
    for A0t, Bt, T in osteps:
        N = (A0t.shape[0] - 5) // 3
        S = dense_step(A0t, Bt, T, d, S) if kind == "dense" else structured_step(rx.scaled_from_oracle(A0t, Bt, T, N), Bt, T, d, S, dtype)
    return S


# ---- (a) -----------------------------------------------------------------------------------------------------------------------------------
def test_reference_blocks_agree_with_the_oracle_and_measure_tau(oracle_lib):
    """Every state the GPU tests step from (all sizes; the single call, the call after the 0.1 s gap, every integrating call of the bursts of
    four): oracle/eqf_numpy.py's A0t / Bt, turned into the blocks as they sit in F, against the 50-digit blocks in units of u max|block|.
    The worst over all of them is the measurement behind TAU_BLK = 10 x: asserted <= TAU_MEASURED (with a quarter on top for a BLAS that orders
    the 3 x 3 products differently), and > TAU_MEASURED / 4, so the recorded figure cannot go stale unnoticed."""
    worst = {}
    for N in rc.ALL_SIZES:
        snap = snapshot(oracle_lib, N)
        for name, _, calls in call_sets(N):
            cl = calls(snap)
            for st, (A0t, Bt, T) in zip(exact_steps(oracle_lib, N, name, cl), oracle_steps(oracle_lib, N, name, cl)):
                assert abs(float(st.mp["T"]) - T) <= 2 ** -53 * T
                for k, v in rx.block_units(st, rx.scaled_from_oracle(A0t, Bt, T, N)).items():
                    if v > worst.get(k, (0.0,))[0]:
                        worst[k] = (v, N, name)
    for k, (v, N, name) in sorted(worst.items()):
        print(f"oracle against the 50-digit blocks, {k:5s}: {v:6.3f} u max|block|   (worst at N = {N}, {name})")
    w = max(v for v, _, _ in worst.values())
    print(f"measured {w:.3f} units; recorded TAU_MEASURED = {rx.TAU_MEASURED}, TAU_BLK = {rx.TAU_BLK} (ten times, at least one)")
    assert rx.TAU_MEASURED / 4 < w <= 1.25 * rx.TAU_MEASURED
    assert rx.TAU_BLK == max(1.0, 10 * rx.TAU_MEASURED)


# ---- (b) -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", rc.ALL_SIZES)
def test_fp64_restatements_stay_inside_the_bound(oracle_lib, N):
    """Ratio to the bound <= 1 at every entry, and symmetric to the bound, for the dense and the structured restatement on every case of this
    size; at the fp32 sizes the structured one in float32 against the fp32 bound."""
    d = rc.settings()
    snap = snapshot(oracle_lib, N)
    bad = []
    for name, fams, calls in call_sets(N):
        cl = calls(snap)
        steps, osteps = exact_steps(oracle_lib, N, name, cl), oracle_steps(oracle_lib, N, name, cl)
        assert len(steps) == len(osteps) == (3 if name == "four" else 1)
        for fam in fams:
            S0 = rc.sigma_family(snap, fam)
            assert np.array_equal(S0, S0.T)
            Sref, E = rx.reference_run(steps, S0)
            res = {}
            for kind in ("dense", "structured"):
                S = run_restatement(kind, osteps, d, S0)
                res[kind] = (rx.worst_ratio(S, Sref, E), rx.symmetry_ratio(S, E))
            if N in rc.F32 and name != "gap":
                Sref32, E32 = rx.reference_run(steps, S0, fp32=True)
                S = run_restatement("structured", osteps, d, S0, np.float32)
                res["structured fp32"] = (rx.worst_ratio(S, Sref32, E32), rx.symmetry_ratio(S, E32))
            print(f"N = {N:3d} {name:4s} family {fam}: " + "   ".join(f"{k} {r:.3f} at {ij} (symmetry {s:.3f})" for k, ((r, ij), s) in res.items()))
            bad += [(N, name, fam, k, r, ij, s) for k, ((r, ij), s) in res.items() if not (r <= 1.0 and s <= 1.0)]
    assert not bad, bad


# ---- (c) -----------------------------------------------------------------------------------------------------------------------------------
N_MUT = 33
# name -> (the Sigma families on which the fault must leave the bound, whether rel_fro < 1e-12 on the filter's own Sigma lets it pass)
MUTATIONS = {
    "Lw transposed (column role, last landmark)": (("a", "b", "c"), False),
    "landmark 16 takes landmark 17's D (column role)": (("a", "b", "c"), False),
    "landmark 16 takes landmark 15's D (column role)": (("a", "b", "c"), False),
    "point noise missing on landmark 7": (("a", "b", "c"), False),
    "dt in place of the accumulated T": (("a", "b", "c"), False),
    "Avg (gravity -> velocity) dropped": (("a", "b"), False),
    "B R B^T scaled by T^2 (Bt by T, not sqrt T)": (("a", "b", "c"), False),
    "bias columns -T B with the wrong sign": (("a", "b", "c"), False),
    "F[9, 4] (-T R_A) off by 1e3 u relative": (("c",), True),
    "F[9, 4] (-T R_A) off by 1e-8 relative": (("a", "b", "c"), True),
}


def mutate(name, A0t, Bt, T, dt, N):
    """(scaled blocks, keyword faults of structured_step, T of the noise) of one mutation"""
    sc = rx.scaled_from_oracle(A0t, Bt, T, N)
    kw = {}
    if name.startswith("Lw transposed"):
        kw["Lwcol"] = sc["Lw"].copy()
        kw["Lwcol"][N - 1] = sc["Lw"][N - 1].T
    elif name.startswith("landmark 16 takes"):
        kw["Dcol"] = sc["D"].copy()
        kw["Dcol"][16] = sc["D"][17 if "17" in name else 15]
    elif name.startswith("point noise"):
        kw["pointvar"] = np.full(N, rc.settings()["pointProcessVariance"])
        kw["pointvar"][7] = 0.0
    elif name.startswith("dt in place"):
        return rx.scaled_from_oracle(A0t, Bt, dt, N), kw, dt
    elif name.startswith("Avg"):
        sc["TAvg"] = np.zeros((3, 2))
    elif name.startswith("B R B^T"):
        kw["TB"] = T * T
    elif name.startswith("bias columns"):
        for k in ("TBg", "TBvw", "TRA", "Lw"):
            sc[k] = -sc[k]
    elif name.startswith("F[9, 4]"):  # (family c holds -1 at (accel bias y, landmark i0): Sigma'[9, landmark i0] is F[9, 4] times one D entry)
        sc["TRA"] = sc["TRA"].copy()
        sc["TRA"][1, 1] *= 1 + (1e3 * rx.U64 if "1e3 u" in name else 1e-8)
    else:
        raise KeyError(name)
    return sc, kw, T


def test_mutations_leave_the_bound_and_two_pass_the_frobenius_gate(oracle_lib):
    """Each fault of MUTATIONS, put into the structured restatement at N = 33 (landmarks 15 | 16 | 17 straddle the tile edge kTileLm = 16):
    caught (ratio > 1) on every family named for it, while the unmutated restatement is inside on all of them; and where the table says so,
    the fault's Sigma' on the filter's OWN Sigma is within rel_fro < 1e-12 of the reference -- the existing single-step gate would have passed
    it.  That blindness is the gap this pull request closes."""
    d = rc.settings()
    snap = snapshot(oracle_lib, N_MUT)
    cl = rc.one_call(snap, "a")
    (st,), ((A0t, Bt, T),) = exact_steps(oracle_lib, N_MUT, "one", cl), oracle_steps(oracle_lib, N_MUT, "one", cl)
    dt = cl[0][0] - snap["time"]
    assert T - dt > 1e-3  # (the accumulated time is not this call's dt)
    fam = {k: rc.sigma_family(snap, k) for k in ("a", "b", "c")}
    ref = {k: rx.reference_run([st], S) for k, S in fam.items()}
    for k, S in fam.items():
        r, _ = rx.worst_ratio(structured_step(rx.scaled_from_oracle(A0t, Bt, T, N_MUT), Bt, T, d, S), *ref[k])
        assert r <= 1.0, (k, r)
    bad = []
    for name, (must, blind) in MUTATIONS.items():
        sc, kw, Tn = mutate(name, A0t, Bt, T, dt, N_MUT)
        ratios, where = {}, {}
        for k, S in fam.items():
            ratios[k], where[k] = rx.worst_ratio(structured_step(sc, Bt, Tn, d, S, **kw), *ref[k])
        fro = rel_fro(structured_step(sc, Bt, Tn, d, fam["a"], **kw), np.asarray(ref["a"][0], dtype=float))
        print(f"{name:50s} ratio to the bound  " + "  ".join(f"{k}: {ratios[k]:9.3g} at {where[k]}" for k in fam)
              + f"   rel_fro on the filter's own Sigma {fro:.2e} ({'passes' if fro < 1e-12 else 'fails'} 1e-12)")
        if not all(ratios[k] > 1.0 for k in must):
            bad.append((name, "not caught", ratios))
        if blind and not fro < 1e-12:
            bad.append((name, "expected to pass the Frobenius gate", fro))
    assert not bad, bad
