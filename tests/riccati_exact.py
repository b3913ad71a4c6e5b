"""TEST INFRASTRUCTURE ONLY -- the Riccati step  Sigma' = F Sigma F^T + T (P + Bt R Bt^T)  entry by entry: a reference, and an a-priori bound
on what any fp64 (or fp32) implementation of it may differ from that reference by.

THE REFERENCE.  The linearisation blocks come from a snapshot (FilterBatch.dump_state format), the settings dictionary and the next stamp, in
mpmath at 50 digits with the primitives of tests/lie_exact.py, written from the DEFINITIONS oracle/eqf_numpy.py:536-594 transcribes
(eqf_state_matrix_A, eqf_input_matrix_B) -- Qhat^-1 is a matrix inverse, nothing is rearranged as buildDLv / buildLw / stepCommon do:
    base       A0[2:5,0:2] = -g cInv          B[0:2,0:3] = cDiff R_A etahat^      B[2:5,0:3] = R_A vhat^        B[2:5,3:6] = R_A
    landmark   A_q = -Qhat (q^ vC^ - 2 vC q^T + q vC^T) Qhat^-1 / |q|^2           A_v = -Qhat R_IC^T R_A^T      B_i = Qhat (q^ R_IC^T + R_IC^T x_IC^)
with T = accumulatedTime + dt and the mean rate (accumulatedVelocity + currentVelocity dt) / T, as VIOFilter::integrateUpToTime takes them.
F = I + T [[0, 0], [-B, A0]], P, Bt = [0; B], R are assembled in the external 11 + 3 N coordinates as oracle/eqf_numpy.py:831-850 does.  The
50-digit products D = I + T A_q, Lv = T A_v, Lw = -T B_i and the base entries of F are rounded ONCE to np.longdouble (64-bit significand);
Sigma' is then formed in longdouble through F's sparsity (<= 9 non-zeros per row: 1 on the diagonal, the six bias columns, two gravity columns
for a velocity row; 1 + 3 + 3 + ... for a landmark row: 3 gyro-bias, 3 velocity, 3 of its own block), O(14 n^2) operations.
    Its own error has the shape of the bound below with 2^-64 in place of 2^-53 and tau = 1/2 (one rounding of each block entry):
    |Sigma'_ref - Sigma'_exact| <= (gamma_k(2^-64) + 2^-64) (|F| |Sigma| |F|^T + |T Q|) <= 2^-11 of the fp64 bound.  It is neglected.
K steps: ExactFilter.process_imu moves the group with lie_exact.group_step (50 digits), a call with dt <= 0 integrates nothing and only
replaces the sample; Sigma is carried in longdouble.

THE BOUND, per entry and for one step.  Write the device's blocks as F + dF, B + dB.  Then
    |Sigma'_dev - Sigma'_ref| <=  gamma_k (|F| |Sigma| |F|^T + |T (P + Bt R Bt^T)|)                                      (rounding of the step)
                                + |dF| |Sigma| |F|^T + |F| |Sigma| |dF|^T + |dF| |Sigma| |dF|^T                          (rounding of the blocks)
                                + T (|dB| R |Bt|^T + |Bt| R |dB|^T + |dB| R |dB|^T)                                     (the same for the noise)
gamma_k = k u / (1 - k u) [Higham, Accuracy and Stability, Lemma 3.1], u = 2^-53.
k counts the rounded operations through which one term F_ia Sigma_ab F_jb (or one noise term) can reach the output entry, whatever the order
of summation and with or without FMA (a sum of m products is within gamma_m of its terms' absolute sum in any order):
     9   the inner sum   Y_ib = sum_a F_ia Sigma_ab     over the <= 9 non-zeros of row i of F
     9   the outer sum   sum_b Y_ib F_jb                over the <= 9 non-zeros of row j
    11   the noise products: B_ic R_c (1), the sum over the <= 6 input channels (6), the scale by T (1), T = accumulatedTime + dt itself (1), and
         the kernels' fold  G[:,0:3] + (sigma_w^2 / T) Lw  in place of a separate product (a division and a product: 2)
     3   the final additions: T P_ii (1), onto the noise sum (1), the noise onto F Sigma F^T (1)
    k = K_OPS = 32.  Of these, 29 follow from the structure of the step alone.  The other 3 -- the rounding of T = accumulatedTime + dt and the
    two operations of the fold -- are an ALLOWANCE for how an implementation may rearrange the noise term (the device's kernels do), not part of
    the structure; they are named here so that nobody takes them for it.  gamma_32 against gamma_29 adds 3 u (|F||Sigma||F|^T + |T Q|) to a bound whose
    tau_blk terms are about 130 u of the same.  Exact zeros and ones add nothing to a sum (x + 0 = x, 1 x = x exactly), so the dense route -- a length-n dot product over
    the same <= 9 non-zeros -- has the same k.  The kernels split the two sums differently ((D S + L Sigma_b) D^T + G L^T); the count is per
    term and does not see that.
|dF| <= tau_blk u max|block| on the positions that block occupies in F (D_i, Lv_i, Lw_i, -T B[0:2,0:3], -T B[2:5,0:3], -T R_A, T A0[2:5,0:2]),
|dB| likewise on Bt: the rounding error of blocks that ANY fp64 implementation computes from the state (a chain of ~10 products of 3 x 3
matrices, a matrix inverse or its rearrangement, the group action).
tau_blk is the one number that is measured and not derived -- from the fp64 ORACLE, never from the device: the worst error of
oracle/eqf_numpy.py's blocks (turned into D, Lv, Lw and the scaled base blocks) against the 50-digit blocks over every state of
riccati_cases.py, K-step states included (there the oracle's own drift of the group is part of it), in units of u max|block|; tau_blk is ten
times that, at least one unit (the margin convention of R13.1).  tests/test_riccati_exact.py measures, prints and asserts it:
    TAU_MEASURED = 6.61 units (x86-64, OpenBLAS; worst on a landmark's Lw = -T B_i in a K-step state at N = 70), TAU_BLK = 66.1.
K steps: e_0 = 0, e_{s+1} = |F_s| e_s |F_s|^T + bound_s evaluated at |Sigma_s| + e_s.
fp32 handles (Sigma and the stored blocks are float, the state and the blocks' arithmetic double): u = 2^-24 in gamma_k, and one storage rounding
each of the input Sigma (u32 |Sigma| pushed through |F| . |F|^T, first step only), of every block entry (u32 |block entry| added to |dF|, |dB|)
and of the output (u32 |Sigma'|)."""
import numpy as np
from mpmath import mpf

import lie_exact as lx

LD = np.longdouble
U64, U32 = 2.0 ** -53, 2.0 ** -24
K_OPS = 32
TAU_MEASURED = 6.61   # units of u max|block|: oracle/eqf_numpy.py against the 50-digit blocks (tests/test_riccati_exact.py prints and checks it)
TAU_BLK = max(1.0, 10.0 * TAU_MEASURED)
G_CONST = mpf(9.81)   # GRAVITY_CONSTANT as every fp64 implementation holds it: the double, not the decimal


def gamma(k, u):
    return k * u / (1.0 - k * u)


def _ld(x):
    """mpf -> longdouble, one rounding (hi + lo carries 106 bits)"""
    hi = float(x)
    return LD(hi) + LD(float(x - hi))


def _ldm(A):
    return np.array([[_ld(x) for x in row] for row in A], dtype=LD)


# ---- the blocks at 50 digits ---------------------------------------------------------------------------------------------------------------
def blocks_mp(X, xi0, cur_w, acc_w, acc_T, dt):
    """X (lie_exact.Group), xi0 (lie_exact.State), currentVelocity's rate (3 doubles), accumulatedVelocity's rate (3 mpf), accumulatedTime and
    this call's dt (mpf): the dictionary of mpf blocks  T, Avg (3 x 2), Bg (2 x 3), Bvw, RA, and per landmark Aq, Av, Bi (lists of 3 x 3)."""
    T = acc_T + dt
    wbar = [(a + mpf(float(c)) * dt) / T for a, c in zip(acc_w, cur_w)]
    eta0, cdiff, cinv = lx.pose_constants(xi0.R)
    est = lx.state_group_action(X, xi0)
    etahat = lx.mv(lx.tr(X.AR), eta0)
    b = {"T": T, "Avg": lx.mscl(-G_CONST, cinv), "Bg": lx.mm(lx.mm(cdiff, X.AR), lx.hat(etahat)), "Bvw": lx.mm(X.AR, lx.hat(est.v)), "RA": X.AR,
         "Aq": [], "Av": [], "Bi": []}
    _, vC = lx._camera_twist(est, wbar)
    RICt = lx.tr(xi0.camR)
    RtRt = lx.mm(RICt, lx.tr(X.AR))
    Kx = lx.mm(RICt, lx.hat(xi0.camx))
    for (RQ, a), q in zip(X.Q, est.p):
        Qhat = lx.mscl(a, RQ)
        inner = lx.madd(lx.mm(lx.hat(q), lx.hat(vC)), lx.madd(lx.mscl(mpf(-2), lx.outer(vC, q)), lx.outer(q, vC)))
        b["Aq"].append(lx.mscl(-1 / lx.dot(q, q), lx.mm(lx.mm(Qhat, inner), lx.inv3(Qhat))))
        b["Av"].append(lx.mscl(mpf(-1), lx.mm(Qhat, RtRt)))
        b["Bi"].append(lx.mm(Qhat, lx.madd(lx.mm(lx.hat(q), RICt), Kx)))
    return b


def scaled_mp(b):
    """The blocks as they sit in F: D = I + T A_q, Lv = T A_v, Lw = -T B_i per landmark, and TBg = -T Bg, TBvw = -T Bvw, TRA = -T R_A, TAvg = T Avg."""
    T = b["T"]
    return {"D": [lx.madd(lx.eye(), lx.mscl(T, A)) for A in b["Aq"]], "Lv": [lx.mscl(T, A) for A in b["Av"]], "Lw": [lx.mscl(-T, B) for B in b["Bi"]],
            "TBg": lx.mscl(-T, b["Bg"]), "TBvw": lx.mscl(-T, b["Bvw"]), "TRA": lx.mscl(-T, b["RA"]), "TAvg": lx.mscl(T, b["Avg"])}


class Step:
    """One step's matrices in longdouble, structured: F = [[Fbb, 0], [L, blockdiag(D)]] (Fbb 11 x 11, L 3 N x 11, D N x 3 x 3), Bt (n x 6), T,
    the diagonals P (n) and R (6); `mp` / `smp` keep the 50-digit blocks (plain and scaled) for comparisons in units."""

    def __init__(self, b, d):
        self.mp, self.smp = b, scaled_mp(b)
        s = self.smp
        N = self.N = len(b["Aq"])
        n = self.n = 11 + 3 * N
        self.T = _ld(b["T"])
        Fbb = np.eye(11, dtype=LD)
        Fbb[6:8, 0:3], Fbb[8:11, 0:3], Fbb[8:11, 3:6], Fbb[8:11, 6:8] = _ldm(s["TBg"]), _ldm(s["TBvw"]), _ldm(s["TRA"]), _ldm(s["TAvg"])
        L = np.zeros((3 * N, 11), dtype=LD)
        D = np.zeros((N, 3, 3), dtype=LD)
        Bt = np.zeros((n, 6), dtype=LD)
        Bt[6:8, 0:3], Bt[8:11, 0:3], Bt[8:11, 3:6] = _ldm(b["Bg"]), _ldm(b["Bvw"]), _ldm(b["RA"])
        for i in range(N):
            L[3 * i:3 * i + 3, 0:3], L[3 * i:3 * i + 3, 8:11], D[i] = _ldm(s["Lw"][i]), _ldm(s["Lv"][i]), _ldm(s["D"][i])
            Bt[11 + 3 * i:14 + 3 * i, 0:3] = _ldm(b["Bi"][i])
        self.F, self.Bt = (Fbb, L, D), Bt
        self.P = np.concatenate([np.full(3, d["biasOmegaProcessVariance"]), np.full(3, d["biasAccelProcessVariance"]), np.full(2, d["gravityProcessVariance"]),
                                 np.full(3, d["velocityProcessVariance"]), np.full(3 * N, d["pointProcessVariance"])]).astype(LD)
        self.R = np.concatenate([np.full(3, d["velOmegaVariance"]), np.full(3, d["velAccelVariance"])]).astype(LD)

    def dense_F(self):
        Fbb, L, D = self.F
        F = np.zeros((self.n, self.n), dtype=LD)
        F[:11, :11], F[11:, :11] = Fbb, L
        for i in range(self.N):
            F[11 + 3 * i:14 + 3 * i, 11 + 3 * i:14 + 3 * i] = D[i]
        return F

    # -- |dF|, |dB| of the bound
    def block_errors(self, tau, u, store_u=0.0):
        """(dF structured like F, dB like Bt): tau u max|block| on each block's positions (+ store_u |entry|: the fp32 storage rounding)."""
        Fbb, L, D = self.F
        dbb, dL, dD, dB = np.zeros_like(Fbb), np.zeros_like(L), np.zeros_like(D), np.zeros_like(self.Bt)

        def fill(dst, src, sl):
            blk = np.abs(src[sl])
            dst[sl] = tau * u * blk.max() + store_u * blk

        for sl in ((slice(6, 8), slice(0, 3)), (slice(8, 11), slice(0, 3)), (slice(8, 11), slice(3, 6)), (slice(8, 11), slice(6, 8))):
            fill(dbb, Fbb, sl)
        for sl in ((slice(6, 8), slice(0, 3)), (slice(8, 11), slice(0, 3)), (slice(8, 11), slice(3, 6))):
            fill(dB, self.Bt, sl)
        for i in range(self.N):
            r = slice(3 * i, 3 * i + 3)
            fill(dL, L, (r, slice(0, 3)))
            fill(dL, L, (r, slice(8, 11)))
            fill(dD, D, (i,))
            fill(dB, self.Bt, (slice(11 + 3 * i, 14 + 3 * i), slice(0, 3)))
        return (dbb, dL, dD), dB


# ---- structured products in longdouble -----------------------------------------------------------------------------------------------------
def _apply(F, S):
    """F S for F = (Fbb, L, D)"""
    Fbb, L, D = F
    N, n = D.shape[0], S.shape[1]
    Y = np.empty((11 + 3 * N, n), dtype=LD)
    Y[:11] = Fbb @ S[:11]
    if N:
        Y[11:] = L @ S[:11] + np.einsum("iab,ibn->ian", D, S[11:].reshape(N, 3, n)).reshape(3 * N, n)
    return Y


def sandwich(A, S, B):
    """A S B^T"""
    return _apply(B, _apply(A, S).T).T


def _absF(F):
    return tuple(np.abs(x) for x in F)


def noise(step):
    """T (P + Bt R Bt^T)"""
    Q = (step.Bt * step.R) @ step.Bt.T
    Q[np.diag_indices(step.n)] += step.P
    return step.T * Q


def reference_sigma(step, S):
    """Sigma' of one step in longdouble (S: any float array; taken as exact)."""
    S = np.asarray(S).astype(LD)
    return sandwich(step.F, S, step.F) + noise(step)


def step_bound(step, S_abs, fp32=False, first=True, tau=None):
    """The per-entry bound of the module docstring for one step from |Sigma| <= S_abs (longdouble)."""
    tau = TAU_BLK if tau is None else tau
    u = U32 if fp32 else U64
    aF, aB = _absF(step.F), np.abs(step.Bt)
    dF, dB = step.block_errors(tau, U64, U32 if fp32 else 0.0)
    S_abs = np.asarray(S_abs).astype(LD)
    main = sandwich(aF, S_abs, aF)
    E = gamma(K_OPS, u) * (main + np.abs(noise(step)))
    Y = sandwich(dF, S_abs, aF)
    E += Y + Y.T + sandwich(dF, S_abs, dF)
    Z = (dB * step.R) @ aB.T
    E += step.T * (Z + Z.T + (dB * step.R) @ dB.T)
    if fp32:
        if first:
            E += U32 * main                      # the input Sigma stored as float
        E += U32 * (main + np.abs(noise(step)))  # the output stored as float (|Sigma'| <= main + |T Q|)
    return E


# ---- the filter's O(N) state, exactly ------------------------------------------------------------------------------------------------------
class ExactFilter:
    """The state a snapshot holds, carried at 50 digits: X, xi0, the zero-order-hold sample and the accumulators.  process_imu follows
    VIOFilter::processIMUData / integrateUpToTime (oracle/eqf_numpy.py:804-858) and returns the Step whose Riccati step the call runs,
    or None when the call does not integrate (dt <= 0, or no sample yet).  The stamps' difference and the bias subtraction are fp64
    operations of the INPUT (as in lie_exact.reference_step); everything after them is exact."""

    def __init__(self, snap, d):
        self.d = d
        self.xi0 = lx.State.from_dict(snap["origin"], d["cameraOffset_q"], d["cameraOffset_x"])
        self.X = lx.Group.from_dict(snap["group"])
        self.time = float(snap["time"])
        self.cur = np.array(snap["currentVelocity"], dtype=float)
        self.acc_w = [mpf(float(x)) for x in np.asarray(snap["accumulatedVelocity"], dtype=float)[0:3]]
        self.acc_T = mpf(float(snap["accumulatedTime"]))
        self.bias = np.array(snap["bias"], dtype=float)

    def process_imu(self, stamp, omega, accel):
        dt = float(stamp) - self.time
        step = None
        if self.time >= 0 and dt > 0:
            step = Step(blocks_mp(self.X, self.xi0, self.cur[0:3], self.acc_w, self.acc_T, mpf(dt)), self.d)
            self.X = lx.group_step(self.X, self.xi0, self.cur[0:3], self.cur[3:6], dt, bool(self.d["useDiscreteVelocityLift"]))
            self.acc_w, self.acc_T = [mpf(0)] * 3, mpf(0)
        self.cur = np.concatenate([np.asarray(omega, dtype=float) - self.bias[0:3], np.asarray(accel, dtype=float) - self.bias[3:6]])
        self.time = float(stamp)
        return step


def exact_steps(snap, d, calls):
    """The Steps of K IMU calls [(stamp, omega, accel)] from a snapshot: the O(N) mpmath work, independent of Sigma.  The group moves at 50
    digits between the steps; a call that does not integrate contributes no Step."""
    f = ExactFilter(snap, d)
    steps = [f.process_imu(stamp, w, a) for stamp, w, a in calls]
    return [s for s in steps if s is not None]


def reference_run(steps, S0, fp32=False):
    """(Sigma_ref, bound) after the Steps from S0, both longdouble: e_0 = 0, e_{s+1} = |F| e_s |F|^T + step_bound at |Sigma_s| + e_s."""
    S = np.asarray(S0).astype(LD)
    e = np.zeros_like(S)
    for k, st in enumerate(steps):
        aF = _absF(st.F)
        e = sandwich(aF, e, aF) + step_bound(st, np.abs(S) + e, fp32, k == 0)
        S = reference_sigma(st, S)
    return S, e


def worst_ratio(S_dev, S_ref, bound):
    """(max |S_dev - S_ref| / bound, its (row, column)); an entry whose bound is 0 must be exact (ratio inf otherwise)."""
    err = np.abs(np.asarray(S_dev).astype(LD) - S_ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, LD(0), err / bound)
    k = int(np.argmax(r))
    return float(r.flat[k]), divmod(k, r.shape[1])


def symmetry_ratio(S_dev, bound):
    """max |S - S^T| / (bound + bound^T)"""
    S = np.asarray(S_dev).astype(LD)
    err = np.abs(S - S.T)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, LD(0), err / (bound + bound.T))
    return float(r.max())


# ---- the fp64 oracle's blocks, and any implementation's, in units of u max|block| -----------------------------------------------------------
def block_units(step, got):
    """got: {"D", "Lv", "Lw": (N, 3, 3), "TBg", "TBvw", "TRA", "TAvg"} as fp64 arrays, as they sit in F.  Returns {name: worst |got - exact| /
    (u max|block|)} per kind of block."""
    out = {}
    for k, want in step.smp.items():
        g = np.asarray(got[k], dtype=float)
        blocks = zip(g, want) if k in ("D", "Lv", "Lw") else [(g, want)]
        worst = 0.0
        for gb, wb in blocks:
            mx = max(abs(x) for row in wb for x in row)
            err = max(abs(mpf(float(gb[i, j])) - wb[i][j]) for i in range(len(wb)) for j in range(len(wb[0])))
            worst = max(worst, float(err / (mpf(U64) * mx)))
        out[k] = worst
    return out


def scaled_from_oracle(A0t, Bt, T, N):
    """oracle/eqf_numpy.py's A0t (5 + 3 N square) and Bt (5 + 3 N x 6) and its accumulated time -> the blocks as they sit in F, in fp64 the way
    line 847 forms them (I + A T)."""
    lm = lambda M, c: np.array([M[5 + 3 * i:8 + 3 * i, c] for i in range(N)]).reshape(N, 3, 3)  # noqa: E731
    return {"D": np.eye(3) + np.array([A0t[5 + 3 * i:8 + 3 * i, 5 + 3 * i:8 + 3 * i] for i in range(N)]).reshape(N, 3, 3) * T,
            "Lv": lm(A0t, slice(2, 5)) * T, "Lw": -lm(Bt, slice(0, 3)) * T,
            "TBg": -Bt[0:2, 0:3] * T, "TBvw": -Bt[2:5, 0:3] * T, "TRA": -Bt[2:5, 3:6] * T, "TAvg": A0t[2:5, 0:2] * T}


def scaled_from_debug_blocks(blk):
    """FilterBatch.debug_blocks() of a split-path step (D, Lw, Lv already scaled by T; Bg, Bvw, RA, Avg plain) -> the same dictionary."""
    T = blk["T"]
    return {"D": blk["D"], "Lv": blk["Lv"], "Lw": blk["Lw"], "TBg": -T * blk["Bg"], "TBvw": -T * blk["Bvw"], "TRA": -T * blk["RA"], "TAvg": T * blk["Avg"]}
