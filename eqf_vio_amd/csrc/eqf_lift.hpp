// The innovation lift (the reference's bundleLift, EqFMatrices.cpp:173-252) for the calls that inform a filter outside a vision frame:
// eqf_update_linear, eqf_update_landmarks, eqf_apply_increment and eqf_perturb_filters (eqf_set_option "innovation_lift").
//
// gamma is the call's increment in the origin chart, gamma_e = gamma[6:], g2 = gamma_e[0:2], gamma_v = gamma_e[2:5], gamma_L = gamma_e[5:].
// With eta0 the unit gravity direction of xi0 and Sigma_e = Sigma[6:, 6:] of the Sigma the call STARTED from:
//   dUw = -eta0^x cInv g2,   dU_f = ((I - eta0 eta0^T) dUw ; 0)
//   Z_P ((5 + 3 N) x 6): five zero rows, then liftRows (eqf_update.hpp) of every landmark
//   Sigma_e = L L^T,   Zt = L^-1 Z_P,   z = L^-1 [0; gamma_L]          -- seven right-hand-side rows of ONE blocked factorisation
//   G6 = Zt^T Zt,   h = Zt^T z,   K = [(eta0; 0) | (0; I3)]:   K^T G6 K x = K^T (-h - G6 dU_f),   DeltaU = dU_f + K x
// then the group step of updateFinishBody (eqf_update.hpp) with DeltaU: X <- VIOExp(liftTotalSpaceInnovation) X or
// liftTotalSpaceInnovationDiscrete, bias += gamma[0:6].  These are updateFinishBody's normal equations with hV - T65 gamma_top replaced
// by h (D alpha = -[0; gamma_L]); the 4 x 4 system goes through the same solve4.
//
//   k_lift_rhs    one wavefront per landmark: its three columns of the six Z_P rows and of the gamma_L row under the scratch image; the
//                 wavefront of landmark 0 also writes the zeros of the top five columns and of the pad.
//   (eqf_factor.hpp's three kernels on LiftArgs: off = 6, kLiftRhs right-hand-side rows, in place in a device copy of Sigma)
//   k_lift_tail   one workgroup per filter: the smallest pivot, G6 and h from the solved rows -- every sum by eight threads, each over
//                 its strided share in ascending order, then a fixed tree, as k_nees_tail does --, the 4 x 4 solve, Delta for the scalars
//                 and for every landmark.  The verdict comes first: every value that would be written is computed and looked at, and only
//                 if all of them are finite the same values are computed again and stored.  A filter that takes the plain lift (the
//                 option is off, useInnovationLift = 0, or fewer than two landmarks: 3 N equations for 4 unknowns) only gets its record
//                 here; k_apply_increment (eqf_sample.hpp) moves it, and passes over the filters this kernel has dealt with.
// Nothing is shared between filters, every sum runs in one fixed order and there are no atomics: bit for bit the same from run to run
// and for a filter alone or anywhere in a batch.  Nothing is written outside rows / columns [6, 6 + m_b) of a filter's scratch image.
#pragma once
#include "eqf_device.hpp"
#include "eqf_factor.hpp"
#include "eqf_math.hpp"
#include "eqf_nees.hpp"
#include "eqf_update.hpp"

namespace eqf {

constexpr int kLiftRhs = 7;        // the six columns of Z_P, then [0; gamma_L]
constexpr int kLiftOff = 6;        // Sigma_e starts at internal index 6
constexpr int kLiftRec = 16;       // per filter: kind, info, DeltaU[6], min_pivot, pivot_ratio, spare
constexpr int kLiftHead = kNeesHead + kNeesRhs;  // doubles of a call's record (eqf_linear.hpp's kLinHead); entry 3 is its verdict word
constexpr int kLiftWordFailed = 5; // verdict word a failed lift leaves in the update's record (4 is eqf_blocks.hpp's idle word)

struct LiftArgs {
    Glob* g;            // current scalar state [B], updated in place
    const double* p0;   // [B][3][cap]
    double* Q;          // [B][5][cap], updated in place
    int cap;
    double* A;          // [B] copies of Sigma, padded layout
    int ld;
    long long strideA;
    double* E;          // [B][kLiftRhs][ldE]: right-hand-side rows, column i = entry 6 + i
    int ldE;
    double* D;          // [B][kDRec]: the record of the current diagonal block
    int* bad;           // [B]: a stage of factor64 met a pivot that was not positive
    const double* gamma;  // filter b: gamma[b * strideG + j] is the increment's entry of internal index offG + j; entries below offG are 0
    long long strideG;
    int offG;
    const unsigned char* mask;  // [B] or nullptr: 0 takes no part
    const double* verdict;      // the call's records [B][kLiftHead] or nullptr: entry 3 != 0 takes no part
    double* fail;               // where a failed lift leaves kLiftWordFailed (the update's records), or nullptr
    int kind;                   // of the call: 0 plain, 1 bundleLift + continuous lift, 2 bundleLift + discrete lift
    double* rec;                // [B][kLiftRec]
    Params prm;
};

EQF_DI double liftGamma(const LiftArgs& a, int b, int j) { return j >= a.offG ? a.gamma[(long long)b * a.strideG + j - a.offG] : 0.0; }
EQF_DI bool liftFinite(double v) { return fabs(v) < __builtin_inf(); }
// the filter is in the call (an increment that is not finite is found by the tail)
EQF_DI bool liftTakesPart(const LiftArgs& a, int b) {
    if (a.mask && !a.mask[b]) return false;
    return !a.verdict || a.verdict[(long long)b * kLiftHead + 3] == 0.0;
}
EQF_DI int liftKind(const LiftArgs& a, int b) { return a.g[b].N >= 2 ? a.kind : 0; }
EQF_DI FactorView factorView(const LiftArgs& a, int b) {
    const int m = (liftKind(a, b) && liftTakesPart(a, b)) ? kLm0 + 3 * a.g[b].N - kLiftOff : 0;
    return FactorView{a.A + (long long)b * a.strideA + (long long)kLiftOff * a.ld + kLiftOff, a.ld, m, kBase - kLiftOff,
        a.D + (long long)b * kDRec, a.bad + b, a.E + (long long)b * kLiftRhs * a.ldE, a.ldE, kLiftRhs};
}

// grid = (landmark groups of the largest filter, B), block = 256 (four wavefronts = four landmarks)
__global__ __launch_bounds__(256) void k_lift_rhs(LiftArgs a) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, i = 4 * (int)blockIdx.x + ((int)threadIdx.x >> 6);
    if (!liftKind(a, b) || !liftTakesPart(a, b)) return;
    const Glob& g = a.g[b];
    const int N = g.N, cap = a.cap;
    if (i >= N) return;
    double* E = a.E + (long long)b * kLiftRhs * a.ldE;
    // Z_P's top five rows and the pad: columns 0 .. 5 of every row
    if (i == 0 && lane < 6 * kLiftRhs) E[(long long)(lane / 6) * a.ldE + lane % 6] = 0.0;
    if (lane >= 3 * kLiftRhs) return;
    const int r = lane / 3, c = lane % 3;  // row r of the right-hand side, component c of the landmark
    double v = 0.0;
    if (r < 6) {
        const double* p0 = a.p0 + (long long)b * 3 * cap;
        const double* Q = a.Q + (long long)b * 5 * cap;
        double Z[18];
        liftRows(liftCommon(g, a.prm), quat{Q[i], Q[cap + i], Q[2 * cap + i], Q[3 * cap + i]}, Q[4 * cap + i],
            mk3(p0[i], p0[cap + i], p0[2 * cap + i]), Z);
#pragma unroll
        for (int k = 0; k < 18; ++k)
            if (k == 6 * c + r) v = Z[k];
    } else {
        v = liftGamma(a, b, kLm0 + 3 * i + c);
    }
    E[(long long)r * a.ldE + (kLm0 - kLiftOff) + 3 * i + c] = v;
}

// the scalar part of a filter's step, computed but not stored
struct LiftScalars {
    double dU[6];
    se3 An;
    d3 wn;
    double bias[6];
    double pivotRatio;
};
// Thread 0's serial part: the 4 x 4 weighted least squares and Delta for the scalars (updateFinishBody's bundleLift branch, expression for
// expression, with h where that has hV - T65 gamma_top).  G6 row-major 6 x 6.
EQF_DI LiftScalars liftScalars(const LiftArgs& a, int b, const double* G6, const double* h) {
    const Glob& g = a.g[b];
    LiftScalars s;
    const d3 v0 = mk3(g.v0[0], g.v0[1], g.v0[2]);
    const d3 gv = mk3(liftGamma(a, b, 8), liftGamma(a, b, 9), liftGamma(a, b, 10));
    const d3 eta0 = unit3(mk3(g.eta0[0], g.eta0[1], g.eta0[2]));
    const double gg0 = liftGamma(a, b, 6), gg1 = liftGamma(a, b, 7);
    const d3 t = mk3(g.cInv[0] * gg0 + g.cInv[1] * gg1, g.cInv[2] * gg0 + g.cInv[3] * gg1, g.cInv[4] * gg0 + g.cInv[5] * gg1);
    const d3 dUw = neg(crs(eta0, t));
    const d3 fx = sub(dUw, scl(dot3(eta0, dUw), eta0));  // DeltaU_fixed = K_perp DeltaU = ((I - eta eta^T) dUw ; 0)
    const double dUf[3] = {fx.x, fx.y, fx.z};
    const double eta[3] = {eta0.x, eta0.y, eta0.z};
    double rhs6[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        double sacc = -h[c];
#pragma unroll
        for (int q = 0; q < 3; ++q) sacc -= G6[6 * c + q] * dUf[q];
        rhs6[c] = sacc;
    }
    // normal equations in the K_par basis, columns (eta;0), (0;e1), (0;e2), (0;e3):  M = Kp^T G6 Kp
    double M[4][4], rhs[4], sol[4];
    double Gw_eta[6];  // G6[:, 0:3] eta
#pragma unroll
    for (int p = 0; p < 6; ++p) Gw_eta[p] = G6[6 * p] * eta[0] + G6[6 * p + 1] * eta[1] + G6[6 * p + 2] * eta[2];
    M[0][0] = eta[0] * Gw_eta[0] + eta[1] * Gw_eta[1] + eta[2] * Gw_eta[2];
    rhs[0] = eta[0] * rhs6[0] + eta[1] * rhs6[1] + eta[2] * rhs6[2];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        M[0][1 + j] = eta[0] * G6[3 + j] + eta[1] * G6[6 + 3 + j] + eta[2] * G6[12 + 3 + j];
        M[1 + j][0] = Gw_eta[3 + j];
        rhs[1 + j] = rhs6[3 + j];
#pragma unroll
        for (int i = 0; i < 3; ++i) M[1 + i][1 + j] = G6[6 * (3 + i) + 3 + j];
    }
    solve4(M, rhs, sol);  // (leaves the pivots on M's diagonal)
    double pmin = fabs(M[0][0]), pmax = pmin;
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        pmin = fmin(pmin, fabs(M[k][k]));
        pmax = fmax(pmax, fabs(M[k][k]));
    }
    s.pivotRatio = pmin / pmax;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        s.dU[i] = dUf[i] + eta[i] * sol[0];
        s.dU[3 + i] = sol[1 + i];
    }
    const se3 DA = se3Exp(mk3(s.dU[0], s.dU[1], s.dU[2]), mk3(s.dU[3], s.dU[4], s.dU[5]));
    d3 Dw;
    if (a.kind == 2) Dw = sub(v0, qrot(DA.q, add(v0, gv)));          // EqFMatrices.cpp:254-258
    else Dw = sub(neg(gv), crs(mk3(s.dU[0], s.dU[1], s.dU[2]), v0));  // :69-79
    const se3 A = se3{quat{g.Aq[0], g.Aq[1], g.Aq[2], g.Aq[3]}, mk3(g.Ax[0], g.Ax[1], g.Ax[2])};
    s.An = se3mul(DA, A);                                           // X = Delta * X  (VIOFilter.cpp:296, VIOGroup.cpp:95)
    s.wn = add(Dw, qrot(DA.q, mk3(g.w[0], g.w[1], g.w[2])));         // :96
#pragma unroll
    for (int i = 0; i < 6; ++i) s.bias[i] = g.bias[i] + liftGamma(a, b, i);  // VIOFilter.cpp:295
    return s;
}
// Q_i <- Delta_i Q_i of landmark i (VIOGroup.cpp:105-107), computed but not stored
EQF_DI void liftLandmark(const LiftArgs& a, int b, int i, quat* Qn, double* an, int* bad) {
    const int cap = a.cap;
    const double* Q = a.Q + (long long)b * 5 * cap;
    const double* p0 = a.p0 + (long long)b * 3 * cap;
    const d3 qi = mk3(p0[i], p0[cap + i], p0[2 * cap + i]);
    const d3 gq = mk3(liftGamma(a, b, kLm0 + 3 * i), liftGamma(a, b, kLm0 + 3 * i + 1), liftGamma(a, b, kLm0 + 3 * i + 2));
    quat dq;
    double da;
    if (a.kind == 2) {  // EqFMatrices.cpp:262-270
        const d3 q1 = add(qi, gq);
        dq = so3FromVectors(q1, qi, bad);
        da = nrm3(qi) / nrm3(q1);
    } else {  // :84-93 then SOT3Exp
        const double n2 = dot3(qi, qi);
        dq = so3Exp(scl(-1.0 / n2, crs(qi, gq)));
        da = exp(-dot3(qi, gq) / n2);
    }
    *Qn = qmul(dq, quat{Q[i], Q[cap + i], Q[2 * cap + i], Q[3 * cap + i]});
    *an = da * Q[4 * cap + i];
}

// grid = B, block = 256
__global__ __launch_bounds__(256) void k_lift_tail(LiftArgs a) {
    __shared__ double sS[256], sMn[256];
    __shared__ double sG[36], sH[6];
    __shared__ int sBad;
    const int b = blockIdx.x, tid = threadIdx.x;
    Glob& g = a.g[b];
    const int N = g.N, cap = a.cap, n = kLm0 + 3 * N;
    double* rec = a.rec + (long long)b * kLiftRec;
    const double nan = __builtin_nan("");
    const int kind = liftKind(a, b);
    // an increment that is not finite moves nothing, as in k_apply_increment (every thread looks at its share)
    const bool part = liftTakesPart(a, b);
    int nf = 0;
    if (part)
        for (int j = max(a.offG, 0) + tid; j < n; j += 256)
            if (!liftFinite(liftGamma(a, b, j))) nf = 1;
    nf = __syncthreads_or(nf);
    if (!part || nf) {
        if (tid < kLiftRec) rec[tid] = tid == 0 ? (double)kind : (tid == 1 ? 3.0 : nan);
        return;
    }
    if (kind == 0) {
        // the plain lift's (dUw; 0), VIOExp(liftInnovation(gamma_e, xi0)): k_apply_increment's expressions
        if (tid == 0) {
            const d3 eta = mk3(g.eta0[0], g.eta0[1], g.eta0[2]);
            const double g6 = liftGamma(a, b, 6), g7 = liftGamma(a, b, 7);
            const d3 t = mk3(g.cInv[0] * g6 + g.cInv[1] * g7, g.cInv[2] * g6 + g.cInv[3] * g7, g.cInv[4] * g6 + g.cInv[5] * g7);
            const d3 Uw = neg(crs(eta, t));
            rec[0] = 0.0; rec[1] = 0.0;
            rec[2] = Uw.x; rec[3] = Uw.y; rec[4] = Uw.z; rec[5] = 0.0; rec[6] = 0.0; rec[7] = 0.0;
            rec[8] = nan; rec[9] = nan;
#pragma unroll
            for (int k = 10; k < kLiftRec; ++k) rec[k] = 0.0;
        }
        return;
    }
    const int m = n - kLiftOff, pad = kBase - kLiftOff;
    const double* A = a.A + (long long)b * a.strideA + (long long)kLiftOff * a.ld + kLiftOff;
    const double* E = a.E + (long long)b * kLiftRhs * a.ldE;
    // the pivots: thread t takes t, t + 256, ...
    double mn = __builtin_inf();
    int npos = 0;
    for (int k = tid; k < m; k += 256) {
        if (k == pad) continue;
        const double l = A[(long long)k * a.ld + k];
        if (!(l > 0.0) || !(l < __builtin_inf())) npos = 1;
        mn = fmin(mn, l * l);
    }
    // sum q = tid >> 3 of the 27: the lower triangle of G6 (q = i (i + 1) / 2 + j, j <= i), then h; its thread s = tid & 7 takes the columns
    // s, s + 8, ... in ascending order
    const int q = tid >> 3, s8 = tid & 7;
    int ri = 0, rj = 6;
    if (q < 21) {
        while ((ri + 1) * (ri + 2) / 2 <= q) ++ri;
        rj = q - ri * (ri + 1) / 2;
    } else {
        ri = q - 21;
    }
    double acc = 0.0;
    if (q < 27) {
        const double* ei = E + (long long)ri * a.ldE;
        const double* ej = E + (long long)rj * a.ldE;
        for (int k = s8; k < m; k += 8)
            if (k != pad) acc = fma(ei[k], ej[k], acc);
    }
    if (tid == 0) sBad = 0;
    sS[tid] = acc;
    sMn[tid] = mn;
    __syncthreads();
    if (npos) sBad = 1;  // (every writer stores the same value)
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) sMn[tid] = fmin(sMn[tid], sMn[tid + w]);
        if (w < 8 && s8 < w) sS[tid] += sS[tid + w];
        __syncthreads();
    }
    if (q < 27 && s8 == 0) {
        if (q < 21) {
            sG[6 * ri + rj] = sS[tid];
            sG[6 * rj + ri] = sS[tid];
        } else {
            sH[ri] = sS[tid];
        }
    }
    __syncthreads();
    // ---- the verdict: everything that would be written, computed and looked at
    int bad = sBad || a.bad[b];
    LiftScalars sc;
    if (tid == 0 && !bad) {
        sc = liftScalars(a, b, sG, sH);
        int ok = liftFinite(sc.pivotRatio) && sc.pivotRatio > 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) ok = ok && liftFinite(sc.dU[i]) && liftFinite(sc.bias[i]);
        ok = ok && liftFinite(sc.An.q.w) && liftFinite(sc.An.q.x) && liftFinite(sc.An.q.y) && liftFinite(sc.An.q.z);
        ok = ok && liftFinite(sc.An.x.x) && liftFinite(sc.An.x.y) && liftFinite(sc.An.x.z);
        ok = ok && liftFinite(sc.wn.x) && liftFinite(sc.wn.y) && liftFinite(sc.wn.z);
        if (!ok) bad = 1;
    }
    if (!bad)
        for (int i = tid; i < N; i += 256) {
            quat Qn;
            double an;
            int bl = 0;
            liftLandmark(a, b, i, &Qn, &an, &bl);
            if (bl || !liftFinite(Qn.w) || !liftFinite(Qn.x) || !liftFinite(Qn.y) || !liftFinite(Qn.z) || !liftFinite(an)) bad = 1;
        }
    bad = __syncthreads_or(bad);
    if (bad) {
        if (tid < kLiftRec) rec[tid] = tid == 0 ? (double)kind : (tid == 1 ? 4.0 : nan);
        if (tid == 0 && a.fail) a.fail[(long long)b * kLiftHead + 3] = (double)kLiftWordFailed;
        return;
    }
    // ---- the same values again, stored
    if (tid == 0) {
        g.Aq[0] = sc.An.q.w; g.Aq[1] = sc.An.q.x; g.Aq[2] = sc.An.q.y; g.Aq[3] = sc.An.q.z;
        g.Ax[0] = sc.An.x.x; g.Ax[1] = sc.An.x.y; g.Ax[2] = sc.An.x.z;
        g.w[0] = sc.wn.x; g.w[1] = sc.wn.y; g.w[2] = sc.wn.z;
#pragma unroll
        for (int i = 0; i < 6; ++i) g.bias[i] = sc.bias[i];
        rec[0] = (double)kind; rec[1] = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) rec[2 + i] = sc.dU[i];
        rec[8] = sMn[0]; rec[9] = sc.pivotRatio;
#pragma unroll
        for (int k = 10; k < kLiftRec; ++k) rec[k] = 0.0;
    }
    double* Q = a.Q + (long long)b * 5 * cap;
    for (int i = tid; i < N; i += 256) {
        quat Qn;
        double an;
        int bl = 0;
        liftLandmark(a, b, i, &Qn, &an, &bl);
        Q[i] = Qn.w; Q[cap + i] = Qn.x; Q[2 * cap + i] = Qn.y; Q[3 * cap + i] = Qn.z;
        Q[4 * cap + i] = an;
    }
}

}  // namespace eqf
