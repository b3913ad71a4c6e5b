"""Exact reference, a-priori bound and blocking model of the pairwise merge costs (eqf_get_merge_costs, csrc/eqf_mergecost.hpp), in the manner
of mixture_exact.py and consistency_exact.py.

THE REFERENCE.  Sigma'_b = J'_b Sigma_b J'_b^T, e_b and the normalised weights are mixture_exact's: the members' Sigma, origin, group and bias
as given (of Sigma the blocks on and below the block diagonal, consistency.lower_mirrored), the estimates, charts, transitions and J blocks
at 50 digits, the sandwich in longdouble; of Sigma' the lower triangle, mirrored, cut at `first`.  SigmaBar_ij = Sigma'_i + alpha (Sigma'_j
- Sigma'_i) and d = e_j - e_i are formed in longdouble with alpha = w~_j / (w~_i + w~_j) from the exact weights (1/2 for the Bhattacharyya
cost and where both weights are 0); the log-determinant and the quadratic form come componentwise from a longdouble factor
(consistency_exact.FactorRef, of SigmaBar rounded once to fp64: that rounding is part of the bound); the costs from those.

THE BOUND, first order, per pair, absolute (a cost is a difference of log-determinants: nothing here is relative to the cost).  u = 2^-53,
gamma_k = k u / (1 - k u), n members.  Operation counts read off csrc/eqf_mergecost.hpp / eqf_mergecost_host.hpp:
  B_b      |d Sigma'_b|: mixture_exact's per-member term without the weight -- (gamma_{K_LOCAL} + REF_SLACK) |J'||Sigma||J'|^T + |dJ'||Sigma||J'|^T
           + |J'||Sigma||dJ'|^T, dJ' with the chart transition's share
  dE_b     |d e_b| <= K_E u scale (mixture_cases.K_E)
  alpha    gamma_{2n+4} alpha: two normalised weights (gamma_{n+1} each), one addition, one division
  Bbar_ij  (1 - alpha) B_i + alpha B_j + (gamma_{2n+4} alpha + u alpha) |Sigma'_j - Sigma'_i| + 2 u |SigmaBar|
           the two roundings of k_pair_form -- the subtraction, the fused multiply-add -- and the reference's own rounding to fp64;
           for a member's own image (a plain copy): B_b + u |Sigma'_b|
  dd_ij    dE_i + dE_j + 2 u |d|
  ld       consistency_exact's bound for the log-determinant of a blocked Cholesky of that order (FactorRef.logdet_bound, with
           consistency_cases.C_LOG) plus sum_ij |A^-1|_ij Bbar_ij
  maha     FactorRef.nees' bound plus |x|^T Bbar |x| + 2 |x|^T dd,   x = SigmaBar^-1 d
  cost     Runnalls: 1/2 [ w~_i (b_ij + b_i) + w~_j (b_ij + b_j) ] + 1/2 (w~_i + w~_j) [ (alpha (1 - alpha) b_maha + (2 gamma_{2n+4} + gamma_3) t)
           / (1 + t) + K_LOG1P u (1 + log1p t) ] + gamma_{n+8} 1/2 [ w~_i |ld_ij - ld_i| + w~_j |ld_ij - ld_j| + (w~_i + w~_j) log1p t ],
           t = alpha (1 - alpha) maha
           Bhattacharyya: 1/8 b_maha + 1/4 (2 b_ij + b_i + b_j) + gamma_6 (1/8 maha + 1/4 (|ld_ij - ld_i| + |ld_ij - ld_j|))
K_LOG1P is measured (mergecost_cases.py) as numpy's worst error of log1p against mp.log1p over the committed cases in units of
u (1 + log1p t), times 4.

VALIDITY.  mixture_exact's condition per member, and per factor max(|L^-1| (E1 + Bbar) |L^-T|) <= consistency_exact.VALIDITY.

THE MODEL.  model(...) states the kernels' blocking in fp64 numpy -- pairs ordered so that i < j, a member's own image a plain copy, the pad
row a row of the identity inside the matrix that is factored, a right-looking Cholesky in 64-wide block columns with the right-hand side
carried along -- and takes the injected faults of FAULTS."""
import numpy as np
from mpmath import mp, mpf

import consistency_cases as cc
import consistency_exact as cx
import mixture_exact as mx
from eqf_vio_amd import consistency as cs
from riccati_exact import LD, gamma

U = 2.0 ** -53
VALIDITY = cx.VALIDITY
KINDS = ("runnalls", "bhattacharyya")


def _alpha_mp(kind, wi, wj):
    return mpf(1) / 2 if (kind == "bhattacharyya" or not wi + wj > 0) else wj / (wi + wj)


def member_images(members, ref, K_E):
    """Per member: Sigma'_b (longdouble, reference index map, lower triangle mirrored), its bound B_b, e_b (longdouble), dE_b; and the
    validity of mixture_exact.  ref: the POSITION of the centre."""
    ests = [mx.estimate_mp(mb) for mb in members]
    E, T, S, th = mx._errors(members, ests, int(ref))
    dim = len(E[0])
    N = (dim - 11) // 3
    out, validity = [], 0.0
    for k, mb in enumerate(members):
        Jmp, Jb, Jl, Db, Dl = mx._cached("jacobian", mb, lambda: mx._jacobian_parts(mb, N))
        Db = Db.copy()
        validity = max(validity, cc.K_J["G"] * U / min(Jmp["theta0"], Jmp["thetaHat"], th[k]) ** 2)
        if T[k] is not None:
            Tl = cx.ldm(T[k])
            aT, aG = np.abs(Tl).astype(float), np.abs(Jb[6:8, 6:8]).astype(float)
            Db[6:8, 6:8] = aT @ Db[6:8, 6:8] + (cc.K_J["G"] * U / th[k] ** 2 + gamma(3, U)) * (np.ones((2, 2)) * aT.max()) @ aG
            Jb = Jb.copy()
            Jb[6:8, 6:8] = Tl @ Jb[6:8, 6:8]
        Sg = cs.lower_mirrored(mb["sigma"])
        Sp = cs.mirror_lower(cx.bd_sandwich(Jb, Jl, Sg.astype(LD), Jb, Jl))
        Ab, Al, aS = np.abs(Jb).astype(float), np.abs(Jl).astype(float), np.abs(Sg)
        B = ((gamma(cx.K_LOCAL, U) + cx.REF_SLACK) * cx.bd_sandwich(Ab, Al, aS, Ab, Al) + cx.bd_sandwich(Db, Dl, aS, Ab, Al)
             + cx.bd_sandwich(Ab, Al, aS, Db, Dl))
        B = np.maximum(B, B.T)
        e = np.array([cx.ld(x) for x in E[k]], dtype=LD)
        out.append(dict(S=Sp, B=B, e=e, dE=K_E * U * S[k]))
    return out, validity


class _Factor:
    """log det and the quadratic form of A + dA, |dA| <= Bx, d + dd' with their bounds (see the module docstring)."""

    def __init__(self, A_ld, Bx, first):
        A64 = A_ld.astype(np.float64)
        self.n = len(A64)
        if self.n == 0:
            self.logdet, self.b_ld, self.validity, self.F = LD(0), 0.0, 0.0, None
            return
        self.F = F = cx.FactorRef(A64, first, cc.C_LOG)
        self.Bx = Bx + U * np.abs(A64)
        aLi = np.abs(F.Linv).astype(np.float64)
        self.validity = float((aLi @ (F.E1 + self.Bx) @ aLi.T).max())
        self.logdet = F.logdet
        self.b_ld = F.logdet_bound + float((F.absAinv * self.Bx).sum())

    def maha(self, d_ld, dd):
        if self.n == 0:
            return LD(0), 0.0
        F = self.F
        d64 = d_ld.astype(np.float64)
        ne, nb = F.nees(d64[None, :])
        x = F.Linv.T @ (F.Linv @ d64.astype(LD))
        ax = np.abs(x).astype(np.float64)
        dd = dd + U * np.abs(d64)
        return ne[0], float(nb[0] + ax @ self.Bx @ ax + 2 * ax @ dd)


def _cost_and_bound(kind, n, wi, wj, a, ldi, ldj, ldij, maha, bi, bj, bij, bm, k_log1p):
    """(cost in longdouble, bound) from longdouble values and fp64 bounds; wi, wj, a: mpf"""
    wi_l, wj_l, a_l = cx.ld(wi), cx.ld(wj), cx.ld(a)
    wi64, wj64, a64 = float(wi), float(wj), float(a)
    di, dj = ldij - ldi, ldij - ldj
    if kind == "bhattacharyya":
        c = maha / 8 + (di + dj) / 4
        b = bm / 8 + (2 * bij + bi + bj) / 4 + gamma(6, U) * (float(abs(maha)) / 8 + (float(abs(di)) + float(abs(dj))) / 4)
        return c, b
    t = a_l * (1 - a_l) * maha
    l1p = np.log1p(t)
    c = (wi_l * di + wj_l * dj + (wi_l + wj_l) * l1p) / 2
    t64, s64 = float(t), wi64 + wj64
    b_t = a64 * (1 - a64) * bm + (2 * gamma(2 * n + 4, U) + gamma(3, U)) * t64
    b = 0.5 * (wi64 * (bij + bi) + wj64 * (bij + bj)) + 0.5 * s64 * (b_t / (1 + t64) + k_log1p * U * (1 + float(l1p)))
    b += gamma(n + 8, U) * 0.5 * (wi64 * float(abs(di)) + wj64 * float(abs(dj)) + s64 * float(l1p))
    return c, b


def reference(members, w, ref, kind, first, pairs, K_E, k_log1p, images=None, cache=None):
    """The records of eqf_get_merge_costs with their bounds.  pairs: list of (i, j) positions (any order) or None: all i < j.  Returns
    dict(pairs, cost, logdet_pair, maha (longdouble arrays), member_logdet, bound = dict(cost, logdet_pair, maha, member_logdet, validity),
    t (the log1p arguments)); images: member_images' result for the same members and ref, to share between calls; cache: a
    dict that keeps the members' factors per `first` between calls with the same images."""
    n = len(members)
    wt = mx._weights(w)
    imgs, validity = images if images is not None else member_images(members, ref, K_E)
    cutm = lambda M: M[first:, first:]  # noqa: E731
    fac = []
    cache = {} if cache is None else cache
    for k in range(n):
        key = (id(imgs[k]), first)
        if key not in cache:
            cache[key] = _Factor(cutm(imgs[k]["S"]), cutm(imgs[k]["B"]), first)
        f = cache[key]
        validity = max(validity, f.validity)
        fac.append(f)
    pp = [(i, j) for i in range(n) for j in range(i + 1, n)] if pairs is None else [tuple(int(x) for x in p) for p in pairs]
    out = dict(pairs=pp, cost=[], logdet_pair=[], maha=[], t=[], member_logdet=np.array([f.logdet for f in fac], dtype=LD))
    bnd = dict(cost=[], logdet_pair=[], maha=[], member_logdet=np.array([f.b_ld for f in fac]))
    for (i, j) in pp:
        i, j = min(i, j), max(i, j)
        a = _alpha_mp(kind, wt[i], wt[j])
        a_l, a64 = cx.ld(a), float(a)
        Si, Sj = cutm(imgs[i]["S"]), cutm(imgs[j]["S"])
        Sbar = Si + a_l * (Sj - Si)
        Bbar = ((1 - a64) * cutm(imgs[i]["B"]) + a64 * cutm(imgs[j]["B"])
                + (gamma(2 * n + 4, U) + U) * a64 * np.abs(Sj - Si).astype(np.float64) + U * np.abs(Sbar).astype(np.float64))
        d = (imgs[j]["e"] - imgs[i]["e"])[first:]
        dd = (imgs[i]["dE"] + imgs[j]["dE"])[first:] + U * np.abs(d).astype(np.float64)
        f = _Factor(Sbar, Bbar, first)
        validity = max(validity, f.validity)
        maha, bm = f.maha(d, dd)
        c, b = _cost_and_bound(kind, n, wt[i], wt[j], a, fac[i].logdet, fac[j].logdet, f.logdet, maha, fac[i].b_ld, fac[j].b_ld, f.b_ld, bm, k_log1p)
        out["cost"].append(c), out["logdet_pair"].append(f.logdet), out["maha"].append(maha)
        out["t"].append(float(cx.ld(a) * (1 - cx.ld(a)) * maha))
        bnd["cost"].append(b), bnd["logdet_pair"].append(f.b_ld), bnd["maha"].append(bm)
    for k in ("cost", "logdet_pair", "maha"):
        out[k] = np.array(out[k], dtype=LD)
        bnd[k] = np.array(bnd[k], dtype=np.float64)
    bnd["validity"] = validity
    out["bound"] = bnd
    return out


def ratios(got, ref):
    """Worst |got - reference| / bound per quantity (cost, logdet_pair, maha, member_logdet); a NaN counts as inf, a bound of 0 demands an
    exact value."""
    out = {}
    for k in ("cost", "logdet_pair", "maha", "member_logdet"):
        if k not in got:
            continue
        g, r, b = np.asarray(got[k], dtype=LD), ref[k], ref["bound"][k]
        if len(r) == 0:
            out[k] = 0.0
            continue
        d = np.abs(g - r).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(b > 0, d / b, np.where(d == 0, 0.0, np.inf))
        out[k] = float(np.where(np.isnan(q), np.inf, q).max())
    return out


def log1p_error_units(ts):
    """worst |numpy log1p - mp.log1p| / (u (1 + log1p t)) over fp64 arguments"""
    worst = 0.0
    for t in np.asarray(ts, dtype=np.float64):
        want = mp.log1p(mpf(float(t)))
        worst = max(worst, float(abs(mpf(float(np.log1p(t))) - want) / (mpf(U) * (1 + abs(want)))))
    return worst


# ---- the kernels' blocking in numpy, with injected faults
FAULTS = ("alpha_swapped", "spread_factor_alpha", "d_sign_gravity_block", "upper_triangle_read", "pad_row_counted", "member_ld_from_sigma",
          "bhattacharyya_half_forgotten", "weights_not_normalised")
PAD_STALE = 2.0  # what the fault "pad_row_counted" finds on the pad's diagonal


def blocked_cholesky(A, rhs, nb=64):
    """Right-looking Cholesky in nb-wide block columns of the lower triangle of A (fp64), z = L^-1 rhs carried along as one more row:
    (L, z); raises numpy.linalg.LinAlgError if a diagonal block is not positive definite."""
    A = np.tril(np.array(A, dtype=np.float64))
    z = np.array(rhs, dtype=np.float64)
    m = len(A)
    for c0 in range(0, m, nb):
        c1 = min(c0 + nb, m)
        Lkk = np.linalg.cholesky(A[c0:c1, c0:c1] + np.tril(A[c0:c1, c0:c1], -1).T)
        A[c0:c1, c0:c1] = Lkk
        z[c0:c1] = np.linalg.solve(Lkk, z[c0:c1])
        if c1 < m:
            A[c1:, c0:c1] = np.linalg.solve(Lkk, A[c1:, c0:c1].T).T
            P = A[c1:, c0:c1]
            A[c1:, c1:] -= np.tril(P @ P.T)
            z[c1:] -= P @ z[c0:c1]
    return A, z


def _factor_model(S, d, first, fault):
    """(logdet, maha) of the image S (reference index map, lower triangle read) as the kernels factor it: cut at first, the pad row a row
    of the identity at internal index 11"""
    A = cx.cut(S, first)
    if len(A) == 0:
        return 0.0, 0.0
    pad = cx.pad_index(first)
    Ap = cx.embed(A, pad)
    dp = np.insert(d[first:], pad, 0.0) if pad >= 0 else d[first:].copy()
    if fault == "pad_row_counted" and pad >= 0:
        Ap[pad, pad] = PAD_STALE
    L, z = blocked_cholesky(Ap, dp)
    return 2.0 * float(np.sum(np.log(np.diag(L)))), float(z @ z)


def model(members, w, ref, kind="runnalls", first=0, pairs=None, fault=None):
    """eqf_get_merge_costs as the kernels block it (fp64 numpy): dict(pairs, cost, logdet_pair, maha, member_logdet)."""
    w = np.asarray(w, dtype=float)
    wt = w.copy() if fault == "weights_not_normalised" else cs.normalise_weights(w)
    n = len(members)
    E, terms = cs.mixture_member_images(members, int(ref))
    if fault == "upper_triangle_read":  # (J' Sigma J'^T from the blocks on and ABOVE the block diagonal)
        flipped = {id(mb): dict(mb, sigma=np.asarray(mb["sigma"]).T) for mb in members}  # (a repeated member stays one object)
        E, terms = cs.mixture_member_images([flipped[id(mb)] for mb in members], int(ref))
    S = [cs.mirror_lower(t) for t in terms]
    zero = np.zeros(len(E[0]))
    mld = []
    for k in range(n):
        src = cs.mirror_lower(cs.lower_mirrored(members[k]["sigma"])) if fault == "member_ld_from_sigma" else S[k]
        mld.append(_factor_model(src.copy(), zero, first, fault)[0])  # a member's own image: a plain copy
    pp = [(i, j) for i in range(n) for j in range(i + 1, n)] if pairs is None else [tuple(int(x) for x in p) for p in pairs]
    cost, ldp, maha = [], [], []
    for (i, j) in pp:
        i, j = min(i, j), max(i, j)
        a = cs.pair_alpha(kind, wt[i], wt[j])
        if fault == "alpha_swapped":
            a = 1.0 - a
        Sbar = S[i] + a * (S[j] - S[i])
        d = E[j] - E[i]
        if fault == "d_sign_gravity_block":
            d[6:8] = -d[6:8]
        ld_, mh = _factor_model(Sbar, d, first, fault)
        if kind == "bhattacharyya":
            c = 0.125 * mh + (0.5 if fault == "bhattacharyya_half_forgotten" else 0.25) * ((ld_ - mld[i]) + (ld_ - mld[j]))
        else:
            sf = a if fault == "spread_factor_alpha" else a * (1.0 - a)
            c = 0.5 * (wt[i] * (ld_ - mld[i]) + wt[j] * (ld_ - mld[j]) + (wt[i] + wt[j]) * np.log1p(sf * mh))
        cost.append(c), ldp.append(ld_), maha.append(mh)
    return dict(pairs=pp, cost=np.array(cost), logdet_pair=np.array(ldp), maha=np.array(maha), member_logdet=np.array(mld))
