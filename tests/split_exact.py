"""TEST INFRASTRUCTURE ONLY -- the deterministic split (csrc/eqf_split.hpp: eqf_split_filters; consistency.split_host) entry by entry: a
50-digit reference from the definitions and an a-priori entrywise bound on what an fp64 implementation may differ from it by.  mpmath;
nothing of oracle/ is imported.

THE REFERENCE (exact()).  Sigma (exact doubles, read as stored), the row Ht in Sigma's coordinates as mpf objects -- the caller's row a
itself (local = 0), or a J with J's blocks the fp64 blocks the implementation multiplies by, the product carried at 50 digits (row_mp()):
    B = Sigma Ht^T    S = Ht B    u = B / sqrt(S)    Sigma_k = Sigma - shrink_k u u^T    gamma_k = shift_k u

THE BOUND (bound()), in the project's a-priori form, u = 2^-53 = EPS / 2:
    |Sigma'_ij - exact| <= K_SPLIT EPS (|Sigma_ij| + shrink (beta_i beta_j) / Sbar)
    |gamma_i   - exact| <= K_SPLIT EPS |shift| beta_i / sqrt(Sbar)
    beta_i = sum_k |Sigma_ik| Hbar_k,    Sbar = sum_k Hbar_k beta_k
with Hbar = |Ht| for a row given in Sigma's coordinates and |a| |J| for a local row (the implementation rounds the entries of a J, three
operations each: what it works with differs from the exact row by at most gamma_3 of that).  beta_i bounds every partial sum of B_i, Sbar
every partial sum of S; the forms are homogeneous in Sigma and in the row like the quantities they bound.

K_SPLIT is MEASURED on the host: the worst ratio of consistency.split_host (numpy, fp64) against exact() over the committed cases of
split_cases.py (all rows, all children, Sigma' and gamma), with the bound's constant set to 1:
    measured worst ratio  Sigma' 4.74   gamma 3.59        both at dense_mixed_85 (n = 266, the largest order the device test uses); the
                                                           cases of order <= 74 stay below 2.2 and 1.85.  python tests/split_exact.py
                                                           prints every case; test_split_exact.py asserts that the measurement has not
                                                           moved beyond the values written here
    K_SPLIT = ceil(4 * 4.74) = 19                          margin 4 for the device's different summation order and contraction
It is never calibrated from the device.  The ratio is not 1 and grows with the order because the forms carry no factor n (an n-term sum
errs by up to gamma_n of its absolute-value sum) and because Sbar >= S: where the row's terms cancel, u's relative error is that of S,
about EPS Sbar / S.  The committed cases hold rows of mixed sign (dense_mixed_*, local_*) and the largest order for that reason."""
import numpy as np
from mpmath import mp, mpf

mp.dps = 50
EPS = 2.0 ** -52
MEASURED_WORST = {"Sigma": 4.74, "gamma": 3.59}
K_SPLIT = 19.0


def _obj(A):
    return np.array([mpf(float(v)) for v in np.asarray(A, dtype=float).ravel()], dtype=object).reshape(np.shape(A))


def row_mp(a, J=None):
    """(Ht as mpf objects, Hbar as doubles): the row in Sigma's coordinates.  J: the dense fp64 Jacobian (local rows) or None."""
    a = np.asarray(a, dtype=float).reshape(-1)
    if J is None:
        return _obj(a), np.abs(a)
    J = np.asarray(J, dtype=float)
    return _obj(a) @ _obj(J), np.abs(a) @ np.abs(J)


def exact(Sigma, Ht, shift, shrink):
    """dict(S, u (n,), Sigma (K, n, n), gamma (K, n)) as mpf objects at 50 digits; Ht from row_mp()."""
    Sg = _obj(Sigma)
    B = Sg @ Ht
    S = Ht @ B
    if not S > 0:
        raise ValueError("exact: S is not positive")
    u = B / mp.sqrt(S)
    uu = np.outer(u, u)
    return dict(S=S, u=u, Sigma=[Sg - mpf(float(k)) * uu for k in np.atleast_1d(shrink)],
                gamma=[mpf(float(s)) * u for s in np.atleast_1d(shift)])


def bound(Sigma, Hbar, shift, shrink, K=K_SPLIT):
    """(bSigma (K, n, n), bGamma (K, n)): the entrywise bounds of the module docstring."""
    aS = np.abs(np.asarray(Sigma, dtype=float))
    beta = aS @ Hbar
    Sbar = float(Hbar @ beta)
    bb = np.outer(beta, beta) / Sbar
    bS = np.stack([K * EPS * (aS + float(k) * bb) for k in np.atleast_1d(shrink)])
    bG = np.stack([K * EPS * abs(float(s)) * beta / np.sqrt(Sbar) for s in np.atleast_1d(shift)])
    return bS, bG


def _ratio(got, ref, bnd):
    """worst |got - ref| / bnd; a zero bound wants the reference's value exactly (ratio 0 then, inf otherwise); a NaN is outside every bound"""
    got = np.asarray(got, dtype=float)
    worst = 0.0
    for g, r, b in zip(got.ravel(), np.asarray(ref, dtype=object).ravel(), np.asarray(bnd, dtype=float).ravel()):
        if not np.isfinite(g):
            return np.inf
        d = float(abs(mpf(float(g)) - r))
        if b > 0.0:
            worst = max(worst, d / b)
        elif d != 0.0:
            return np.inf
    return worst


def ratios(got_sigma, got_gamma, ref, bS, bG):
    """{"Sigma", "gamma"}: the worst ratio over all children; got_sigma (K, n, n), got_gamma (K, n) or None"""
    out = {"Sigma": max(_ratio(got_sigma[k], ref["Sigma"][k], bS[k]) for k in range(len(bS)))}
    if got_gamma is not None:
        out["gamma"] = max(_ratio(got_gamma[k], ref["gamma"][k], bG[k]) for k in range(len(bG)))
    return out


def moment_ratio(weights, got_sigma, got_gamma, Sigma, bS, bG):
    """The moment identity sum_k w_k (Sigma_k + gamma_k gamma_k^T) = Sigma, from an implementation's children, summed at 50 digits: the worst
    |sum - Sigma| / bound with bound_ij = sum_k w_k (bS_k + |gamma_k|_i bG_kj + bG_ki |gamma_k|_j + bG_ki bG_kj) + K_SPLIT EPS |Sigma_ij| (the
    children's own bounds carried through the sum; the last term: the weights and moments are doubles, the identity holds for them up to
    their rounding)."""
    n = len(Sigma)
    acc = np.zeros((n, n), dtype=object) + mpf(0)
    bnd = K_SPLIT * EPS * np.abs(np.asarray(Sigma, dtype=float))
    for k, w in enumerate(weights):
        g = _obj(got_gamma[k])
        acc = acc + mpf(float(w)) * (_obj(got_sigma[k]) + np.outer(g, g))
        ag = np.abs(np.asarray(got_gamma[k], dtype=float))
        bnd = bnd + float(w) * (bS[k] + np.outer(ag, bG[k]) + np.outer(bG[k], ag) + np.outer(bG[k], bG[k]))
    return _ratio_obj(acc, _obj(Sigma), bnd)


def _ratio_obj(got, ref, bnd):
    worst = 0.0
    for g, r, b in zip(got.ravel(), ref.ravel(), np.asarray(bnd, dtype=float).ravel()):
        d = float(abs(g - r))
        if b > 0.0:
            worst = max(worst, d / b)
        elif d != 0.0:
            return np.inf
    return worst


# ---- the host statement with switchable faults (what the bound must tell from the real thing) -------------------------------------------
FAULTS = ("u_not_normalised", "shrink_without_1_over_S", "gamma_sign", "upper_from_transposed_product")


def faulty(Sigma, Ht, shift, shrink, fault):
    """consistency.split_host's arithmetic in numpy fp64 with one of FAULTS injected.  Returns (Sigma (K, n, n), gamma (K, n))."""
    Sg = np.asarray(Sigma, dtype=float)
    h = np.asarray(Ht, dtype=float)
    B = Sg @ h
    S = float(h @ B)
    u = B if fault == "u_not_normalised" else B / np.sqrt(S)
    uu = np.outer(B, B) if fault == "shrink_without_1_over_S" else np.outer(u, u)
    if fault == "upper_from_transposed_product":  # above the diagonal u_i v_j with v from Ht Sigma read through the stored lower triangle alone
        v = (np.tril(Sg).T @ h) / np.sqrt(S)
        uu = np.tril(uu) + np.triu(np.outer(u, v), 1)
    sg = [Sg - float(k) * uu for k in np.atleast_1d(shrink)]
    gm = [(-float(s) if fault == "gamma_sign" else float(s)) * u for s in np.atleast_1d(shift)]
    return np.stack(sg), np.stack(gm)


def measure():
    """{"Sigma", "gamma"}: the worst ratio of consistency.split_host over split_cases.CASES with the constant set to 1."""
    import split_cases as sc
    from eqf_vio_amd import consistency as cs

    worst = {"Sigma": 0.0, "gamma": 0.0}
    for case in sc.CASES:
        Sigma, a, J, shift, shrink = sc.build(case)
        Ht, Hbar = row_mp(a, J)
        ref = exact(Sigma, Ht, shift, shrink)
        bS, bG = bound(Sigma, Hbar, shift, shrink, K=1.0)
        got = cs.split_host(Sigma, a if J is None else a @ J, shift, shrink)
        r = ratios(got["Sigma"], got["gamma"], ref, bS, bG)
        print(f"{case['name']:>24s}  n = {len(a):3d}  Sigma {r['Sigma']:.3f}  gamma {r['gamma']:.3f}")
        worst = {k: max(worst[k], r[k]) for k in worst}
    return worst


if __name__ == "__main__":
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("worst:", measure())
