// Moment matching over the filters of one handle (eqf_get_mixture_moments, eqf_merge_filters).
//
// Members idx[0..n) with normalised weights w~ are summarised in the chart chi_c of a centre state c (the chart of consistency.local_error:
// differences for bias, body velocity and body-frame landmarks, stereoSphereChart(eta, pole = eta_c) for the gravity direction):
//   e_b  = chi_c(xHat_b), xHat_b = phi_X(xi0) the estimate of member b (what eqf_get_state_estimate / eqf_get_bias return)
//   J'_b = J_b of eqf_local.hpp with its gravity block G_b replaced by T_b G_b, T_b = stereoChartDiff(eta_b, pole eta_c)
//          stereoChartInvDiff(0, pole eta_b) the differential at 0 of chi_c o chi_xHat_b^-1 (every other block of it is the identity);
//          T_b = I BY DEFINITION when c is member b's own estimate taken by index
//   eBar = sum_k w~_k e_k,   P = sum_k w~_k [ J'_k Sigma_k J'_k^T + (e_k - m)(e_k - m)^T ],  m = eBar (centred) or 0
// All in fp64, in one fixed order (the order of idx), without atomics: every entry has one writer.
//
//   k_mix_estimate  per distinct filter: the estimate image [kMixEstHead + 3 cap] -- bias, eta, velocity, pose position, pose attitude,
//                   landmarks -- formed from Glob / p0 / Q exactly as k_state_estimate forms them
//   k_mix_error     per distinct filter: e_b in the padded index map (entry 11 zero), J'_b as a copy of k_local_jacobian's record with
//                   T_b G_b in it, and the singular-chart verdict.  Launched after k_local_jacobian.
//   k_mix_mean      eBar, one lane per entry, the members walked serially
//   k_mix_retract   (merge) xBar = local_retract(xHat_ref, eBar): its estimate image (the centre of the second pass) and the staged small
//                   state of the destination -- origin = xBar, X = identity
//   k_mix_reduce    THE HOT PATH: P.  A workgroup of one wavefront owns one tile of the lower triangle of P in the internal 12 + 3 N layout
//                   (eqf_device.hpp): kMixRows row landmarks x kMixLanes column landmarks, one column landmark per lane; the workgroups
//                   of the first row block also own the base columns of their landmarks' rows, the first workgroup the base block.  It
//                   walks the members in the order of idx with the next 3 x 3 block's loads in flight (across members), applies J' with
//                   the pinned roundings of localBlock / baseApply -- J'_J of the member in registers, J'_I through wave-uniform loads --
//                   accumulates with one fused multiply-add per member and entry, adds the spread term in the same order, and writes the
//                   tile and its mirror from the same registers: P is bit-for-bit symmetric, pad row and column 11 are zero.  The first
//                   member's term is a product, not an addition to zero, and a spread product that is zero is not added: with n = 1 the
//                   lower triangle is k_sigma_local's, bit for bit.  Reads every member's Sigma once -- the blocks on and below the block diagonal: the 11 x 11 base block and the
//                   diagonal 3 x 3 blocks whole, as stored --, writes P once.
//   k_mix_report    the traces of the report, the verdict word
//   k_mix_store / k_mix_commit / k_mix_restore   (merge) behind the verdict: P from the scratch image into the destination's Sigma, the
//                   staged small state into the destination (with the records of the last update, as k_clone_small copies them), and
//                   what k_clone_restore does.  With a verdict other than 0 none of them writes anything.
#pragma once
#include <cstddef>

#include "eqf_device.hpp"
#include "eqf_innov.hpp"
#include "eqf_local.hpp"
#include "eqf_math.hpp"
#include "eqf_propagate.hpp"
#include "eqf_update.hpp"

namespace eqf {

constexpr int kMixRows = 4;      // row landmarks per tile of k_mix_reduce
constexpr int kMixLanes = 64;    // column landmarks per tile: one wavefront
constexpr int kMixEstHead = 20;  // estimate image: bias (6) at 0, eta (3) at 6, velocity (3) at 9, pose x (3) at 12, pose q (4) at 15, landmarks at 20 + 3 i

struct MixMember {
    int b, pad_;
    double w;  // normalised, > 0
};

struct MixArgs {
    Glob* g;               // the handle's state: read by every kernel, written (filter dst only) by k_mix_commit / k_mix_restore
    double *p0, *Q;        // [B][3][cap], [B][5][cap]
    int cap, B;
    const double* jac;     // k_local_jacobian's records [B][jacStride(cap)]
    double* jacT;          // J' records, same layout
    double* est;           // estimate images [B + 1][kMixEstHead + 3 cap]; slot B: the merged state
    double* err;           // e_b [B][ld], padded index map
    double* mean;          // eBar [ld], padded index map
    const MixMember* mem;  // members of non-zero weight, in the order of idx
    int n;
    const int* uniq;       // the distinct filters among them, and ref
    int nUniq;
    int N;                 // landmarks of every member
    int centre;            // slot of `est` that holds the centre
    int centreFilter;      // the filter whose OWN estimate that is (T = I, e = 0 exactly), or -1
    int centred;           // spread about eBar (1) or about 0
    int ref, dst;
    double* Sigma;         // the handle's covariance: read by k_mix_reduce, written (filter dst only) by k_mix_store
    int ld;
    long long sigmaStride;
    double* P;             // the image P is written to (leading dimension ld)
    double* out;           // [4]: spread trace, total trace
    int* verdict;          // [0] a chart needed is singular, [1] a non-finite value met, [2] info (k_mix_report)
    // merge: the staged small state and the handle's arrays it goes to
    Glob* stG;
    double *stP0, *stQ;    // [3][cap], [5][cap]
    double* lmc;
    double *delta, *gamma, *gammaTot, *innov;  // records of the last update (innov may be nullptr)
};

__host__ __device__ inline long long mixEstStride(int cap) { return kMixEstHead + 3LL * cap; }

// stereoSphereChart^-1(y, pole) (VIOState.cpp:236-240)
EQF_DI d3 stereoChartInv(double y0, double y1, d3 pole, int* bad) {
    const double s = 2.0 / (y0 * y0 + y1 * y1 + 1.0);
    const d3 r = mk3(s * y0, s * y1, 1.0 + s * (0.0 - 1.0));
    return qrot(qinv(sphereRotQ(pole, bad)), r);
}

// grid = (ceil(max(N, 1) / 256), nUniq), block = 256
__global__ __launch_bounds__(256) void k_mix_estimate(MixArgs a) {
    const int b = a.uniq[blockIdx.y];
    const Glob& s = a.g[b];
    const int cap = a.cap;
    double* X = a.est + b * mixEstStride(cap);
    const int i = blockIdx.x * 256 + threadIdx.x;
    const quat Aq = quat{s.Aq[0], s.Aq[1], s.Aq[2], s.Aq[3]};
    if (i == 0) {
        // k_state_estimate's pose and velocity; eta = R^T e3 of that pose (VIOState.cpp:90)
        const se3 P = se3mul(se3{quat{s.P0q[0], s.P0q[1], s.P0q[2], s.P0q[3]}, mk3(s.P0x[0], s.P0x[1], s.P0x[2])}, se3{Aq, mk3(s.Ax[0], s.Ax[1], s.Ax[2])});
        const d3 v = qrot(qinv(Aq), mk3(s.v0[0] - s.w[0], s.v0[1] - s.w[1], s.v0[2] - s.w[2]));
        const d3 eta = qrot(qinv(P.q), mk3(0, 0, 1));
#pragma unroll
        for (int k = 0; k < 6; ++k) X[k] = s.bias[k];
        X[6] = eta.x; X[7] = eta.y; X[8] = eta.z;
        X[9] = v.x; X[10] = v.y; X[11] = v.z;
        X[12] = P.x.x; X[13] = P.x.y; X[14] = P.x.z;
        X[15] = P.q.w; X[16] = P.q.x; X[17] = P.q.y; X[18] = P.q.z;
        X[19] = 0.0;
    }
    if (i < a.N) {
        const double* P = a.p0 + (long long)b * 3 * cap;
        const double* q = a.Q + (long long)b * 5 * cap;
        const quat Qq = quat{q[i], q[cap + i], q[2 * cap + i], q[3 * cap + i]};
        const d3 qh = scl(1.0 / q[4 * cap + i], qrot(qinv(Qq), mk3(P[i], P[cap + i], P[2 * cap + i])));
        X[kMixEstHead + 3 * i] = qh.x; X[kMixEstHead + 3 * i + 1] = qh.y; X[kMixEstHead + 3 * i + 2] = qh.z;
    }
}

// grid = (ceil(max(N, 1) / 256), nUniq), block = 256
__global__ __launch_bounds__(256) void k_mix_error(MixArgs a) {
    const int b = a.uniq[blockIdx.y];
    const int cap = a.cap;
    const double* X = a.est + b * mixEstStride(cap);
    const double* C = a.est + a.centre * mixEstStride(cap);
    const double* jac = a.jac + b * jacStride(cap);
    double* jt = a.jacT + b * jacStride(cap);
    double* e = a.err + (long long)b * a.ld;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) {
        int bad = jac[13] != 0.0 ? 1 : 0;
#pragma unroll
        for (int k = 0; k < 6; ++k) e[k] = X[k] - C[k];
        if (b == a.centreFilter) {  // the centre is this member's own estimate: T = I by definition, not computed
            e[6] = 0.0;
            e[7] = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) jt[k] = jac[k];
        } else {
            const d3 eta = mk3(X[6], X[7], X[8]), pole = mk3(C[6], C[7], C[8]);
            double y0, y1, cd[6], ci[6], T[4];
            stereoChart(eta, pole, &y0, &y1, &bad);
            stereoChartDiff(eta, pole, cd, &bad);
            stereoChartInvDiffAtZero(eta, ci, &bad);
            e[6] = y0;
            e[7] = y1;
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int c = 0; c < 2; ++c) T[2 * r + c] = dot3(cd[3 * r], ci[c], cd[3 * r + 1], ci[2 + c], cd[3 * r + 2], ci[4 + c]);
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int c = 0; c < 2; ++c) jt[2 * r + c] = fma(T[2 * r + 1], jac[2 + c], T[2 * r] * jac[c]);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) e[8 + k] = X[9 + k] - C[9 + k];
        e[11] = 0.0;
#pragma unroll
        for (int k = 4; k < 13; ++k) jt[k] = jac[k];
        jt[13] = bad ? 1.0 : 0.0;
        jt[14] = 0.0;
        jt[15] = 0.0;
        if (bad) a.verdict[0] = 1;
    }
    if (i < a.N) {
#pragma unroll
        for (int c = 0; c < 3; ++c) e[kLm0 + 3 * i + c] = X[kMixEstHead + 3 * i + c] - C[kMixEstHead + 3 * i + c];
#pragma unroll
        for (int k = 0; k < 9; ++k) jt[kJacHead + 9LL * i + k] = jac[kJacHead + 9LL * i + k];
    }
}

// grid = ceil((12 + 3 N) / 256), block = 256
__global__ __launch_bounds__(256) void k_mix_mean(MixArgs a) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= kLm0 + 3 * a.N) return;
    double acc = 0.0;
    for (int k = 0; k < a.n; ++k) {
        const MixMember m = a.mem[k];
        const double v = a.err[(long long)m.b * a.ld + j];
        acc = k == 0 ? m.w * v : fma(m.w, v, acc);
    }
    a.mean[j] = acc;
    if (!isfinite(acc)) a.verdict[1] = 1;
}

// One workgroup.  xBar = local_retract(xHat_ref, eBar) with bias_ref + eBar[0:6]; pose position sum w~_k x_k.  block = 256
__global__ __launch_bounds__(256) void k_mix_retract(MixArgs a) {
    const int cap = a.cap, N = a.N, tid = threadIdx.x;
    const double* R = a.est + a.ref * mixEstStride(cap);
    double* X = a.est + a.B * mixEstStride(cap);
    const double* m = a.mean;
    if (tid == 0) {
        int bad = 0;
        const quat qr = quat{R[15], R[16], R[17], R[18]};
        quat qn = qr;
        if (m[6] != 0.0 || m[7] != 0.0) {  // (eBar_gravity = 0 is the reference's own direction: the attitude keeps every bit)
            const d3 etaR = mk3(R[6], R[7], R[8]);
            const d3 eta = stereoChartInv(m[6], m[7], etaR, &bad);
            // the shortest rotation that takes eta_ref to eta (Rodrigues, as SO3.cpp:155-167): R_new = R_ref D^T
            qn = qmul(qr, qinv(m2q(rotFromUnitVectors(etaR, eta, &bad))));
        }
        const d3 etaN = qrot(qinv(qn), mk3(0, 0, 1));
        double x[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k < a.n; ++k) {
            const MixMember mm = a.mem[k];
            const double* Xk = a.est + mm.b * mixEstStride(cap);
#pragma unroll
            for (int c = 0; c < 3; ++c) x[c] = k == 0 ? mm.w * Xk[12 + c] : fma(mm.w, Xk[12 + c], x[c]);
        }
        Glob G = a.g[a.ref];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            X[k] = R[k] + m[k];
            G.bias[k] = X[k];
        }
        X[6] = etaN.x; X[7] = etaN.y; X[8] = etaN.z;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            X[9 + k] = R[9 + k] + m[8 + k];
            X[12 + k] = x[k];
            G.v0[k] = X[9 + k];
            G.P0x[k] = x[k];
            G.Ax[k] = 0.0;
            G.w[k] = 0.0;
        }
        X[15] = qn.w; X[16] = qn.x; X[17] = qn.y; X[18] = qn.z;
        X[19] = 0.0;
        G.P0q[0] = qn.w; G.P0q[1] = qn.x; G.P0q[2] = qn.y; G.P0q[3] = qn.z;
        G.Aq[0] = 1.0; G.Aq[1] = 0.0; G.Aq[2] = 0.0; G.Aq[3] = 0.0;
        G.updateOk = 0;  // (as eqf_set_state and eqf_copy_filters leave it)
        *a.stG = G;
        if (bad) a.verdict[0] = 1;
    }
    for (int i = tid; i < cap; i += 256) {
        const bool in = i < N;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double p = in ? R[kMixEstHead + 3 * i + c] + m[kLm0 + 3 * i + c] : 0.0;
            if (in) X[kMixEstHead + 3 * i + c] = p;
            a.stP0[(long long)c * cap + i] = p;  // with X = identity the origin landmark is the estimate's
        }
        a.stQ[i] = in ? 1.0 : 0.0;
        a.stQ[cap + i] = 0.0;
        a.stQ[2 * cap + i] = 0.0;
        a.stQ[3 * cap + i] = 0.0;
        a.stQ[4 * cap + i] = in ? 1.0 : 0.0;
    }
}

// acc += (w d_row) d_col, skipped when the product is an exact zero (so that a member at the centre changes no bit, not even a zero's sign)
EQF_DI double mixSpread(double wd, double d, double acc) { return (wd != 0.0 && d != 0.0) ? fma(wd, d, acc) : acc; }

// grid = (chunks of kMixLanes column landmarks, blocks of kMixRows row landmarks) (at least (1, 1)), block = kMixLanes
__global__ __launch_bounds__(kMixLanes) void k_mix_reduce(MixArgs a) {
    const int N = a.N, tid = threadIdx.x;
    const int I0 = blockIdx.y * kMixRows, J0 = blockIdx.x * kMixLanes, J = J0 + tid;
    const bool firstWg = blockIdx.x == 0 && blockIdx.y == 0;
    const int nI = max(0, min(kMixRows, N - I0));
    if (blockIdx.y != 0 && (nI == 0 || I0 + nI - 1 < J0)) return;  // (nothing of the lower triangle in this tile; the first row block also owns base columns)
    const int ld = a.ld, cap = a.cap, n = a.n;
    const bool validJ = J < N;
    const int Jc = validJ ? J : 0;
    const double* mean = a.mean;
    const bool cen = a.centred != 0;
    double* P = a.P;
    bool nonFinite = false;
    double mJ[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) mJ[c] = (cen && N > 0) ? mean[kLm0 + 3 * Jc + c] : 0.0;

    if (blockIdx.y == 0) {
        // ---- the base columns of this lane's landmark rows: sum_k w~_k J'_J Sigma_Jb J'_b^T + spread, and the mirror
        if (validJ) {
            double acc[3][11] = {};
            for (int k = 0; k < n; ++k) {
                const MixMember mm = a.mem[k];
                const double w = mm.w;
                const double* jac = a.jacT + mm.b * jacStride(cap);
                const double* e = a.err + (long long)mm.b * ld;
                const double* rowIn = a.Sigma + (long long)mm.b * a.sigmaStride + (long long)(kLm0 + 3 * J) * ld;
                double JJ[9], U[3][11];
#pragma unroll
                for (int q = 0; q < 9; ++q) JJ[q] = jac[kJacHead + 9LL * J + q];
#pragma unroll
                for (int q = 0; q < 11; ++q) {
                    const double s0 = rowIn[q], s1 = rowIn[ld + q], s2 = rowIn[2 * (long long)ld + q];
#pragma unroll
                    for (int r = 0; r < 3; ++r) U[r][q] = dot3(JJ[3 * r], s0, JJ[3 * r + 1], s1, JJ[3 * r + 2], s2);
                }
                double dB[11];
#pragma unroll
                for (int q = 0; q < 11; ++q) dB[q] = e[q] - (cen ? mean[q] : 0.0);
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    double o[11];
                    baseApply(jac, jac + 4, U[r], o);
                    const double wd = w * (e[kLm0 + 3 * J + r] - mJ[r]);
#pragma unroll
                    for (int q = 0; q < 11; ++q) {
                        const double t = k == 0 ? w * o[q] : fma(w, o[q], acc[r][q]);
                        acc[r][q] = mixSpread(wd, dB[q], t);
                    }
                }
            }
            double* rowOut = P + (long long)(kLm0 + 3 * J) * ld;
            double* colOut = P + kLm0 + 3 * J;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int q = 0; q < 11; ++q) {
                    nonFinite = nonFinite || !isfinite(acc[r][q]);
                    rowOut[(long long)r * ld + q] = acc[r][q];
                    colOut[(long long)q * ld + r] = acc[r][q];
                }
                rowOut[(long long)r * ld + 11] = 0.0;  // the structural pad row / column 11
                colOut[(long long)11 * ld + r] = 0.0;
            }
        }
        // ---- the base block: row tid of sum_k w~_k J'_b Sigma_bb J'_b^T + spread; its lower triangle and the mirror
        if (firstWg) {
            __shared__ double sT[11][12];
            double acc[11] = {};
            for (int k = 0; k < n; ++k) {
                const MixMember mm = a.mem[k];
                const double w = mm.w;
                const double* jac = a.jacT + mm.b * jacStride(cap);
                const double* e = a.err + (long long)mm.b * ld;
                const double* S = a.Sigma + (long long)mm.b * a.sigmaStride;
                if (tid < 11) {  // column tid of J'_b Sigma_bb (localBaseBlock's two steps)
                    double in[11], o[11];
#pragma unroll
                    for (int q = 0; q < 11; ++q) in[q] = S[(long long)q * ld + tid];
                    baseApply(jac, jac + 4, in, o);
#pragma unroll
                    for (int q = 0; q < 11; ++q) sT[q][tid] = o[q];
                }
                __syncthreads();
                if (tid < 11) {
                    double in[11], o[11];
#pragma unroll
                    for (int q = 0; q < 11; ++q) in[q] = sT[tid][q];
                    baseApply(jac, jac + 4, in, o);
                    const double wd = w * (e[tid] - (cen ? mean[tid] : 0.0));
#pragma unroll
                    for (int q = 0; q < 11; ++q) {
                        const double t = k == 0 ? w * o[q] : fma(w, o[q], acc[q]);
                        acc[q] = mixSpread(wd, e[q] - (cen ? mean[q] : 0.0), t);
                    }
                }
                __syncthreads();
            }
            if (tid < 11) {
#pragma unroll
                for (int q = 0; q < 11; ++q)
                    if (q <= tid) {
                        nonFinite = nonFinite || !isfinite(acc[q]);
                        P[(long long)tid * ld + q] = acc[q];
                        P[(long long)q * ld + tid] = acc[q];
                    }
            }
            if (tid < 12) {
                P[(long long)tid * ld + 11] = 0.0;
                P[(long long)11 * ld + tid] = 0.0;
            }
        }
    }

    // ---- landmark rows I0 .. I0 + nI - 1 against this lane's column landmark, where row >= column
    if (nI > 0 && J0 < N && I0 + nI - 1 >= J0) {
        double acc[kMixRows][9] = {};
        double S[9] = {};
        const long long colOff = kLm0 + 3 * Jc;
        auto fetch = [&](const double* Sk, int i) {
            if (validJ && I0 + i >= J) {
                const double* p = Sk + (long long)(kLm0 + 3 * (I0 + i)) * ld + colOff;
#pragma unroll
                for (int rr = 0; rr < 3; ++rr)
#pragma unroll
                    for (int cc = 0; cc < 3; ++cc) S[3 * rr + cc] = p[(long long)rr * ld + cc];
            }
        };
        fetch(a.Sigma + (long long)a.mem[0].b * a.sigmaStride, 0);
        for (int k = 0; k < n; ++k) {
            const MixMember mm = a.mem[k];
            const double w = mm.w;
            const double* jac = a.jacT + mm.b * jacStride(cap);
            const double* e = a.err + (long long)mm.b * ld;
            const double* Sk = a.Sigma + (long long)mm.b * a.sigmaStride;
            const double* Sn = a.Sigma + (long long)a.mem[min(k + 1, n - 1)].b * a.sigmaStride;
            double JJ[9], dJ[3];
#pragma unroll
            for (int q = 0; q < 9; ++q) JJ[q] = jac[kJacHead + 9LL * Jc + q];
#pragma unroll
            for (int c = 0; c < 3; ++c) dJ[c] = e[kLm0 + 3 * Jc + c] - mJ[c];
#pragma unroll
            for (int i = 0; i < kMixRows; ++i) {
                if (i < nI) {
                    double Sc[9], O[9];
#pragma unroll
                    for (int q = 0; q < 9; ++q) Sc[q] = S[q];
                    // the next block's loads fly during this block's arithmetic: the next row of this member, or the next member's first
                    if (i + 1 < nI) fetch(Sk, i + 1);
                    else if (k + 1 < n) fetch(Sn, 0);
                    const double* JI = jac + kJacHead + 9LL * (I0 + i);  // (wave-uniform)
                    localBlock(JI, Sc, JJ, O);
                    const double* eI = e + kLm0 + 3 * (I0 + i);
                    const double* mI = mean + kLm0 + 3 * (I0 + i);
#pragma unroll
                    for (int r = 0; r < 3; ++r) {
                        const double wd = w * (eI[r] - (cen ? mI[r] : 0.0));
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            const double t = k == 0 ? w * O[3 * r + c] : fma(w, O[3 * r + c], acc[i][3 * r + c]);
                            acc[i][3 * r + c] = mixSpread(wd, dJ[c], t);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < kMixRows; ++i) {
            const int I = I0 + i;
            if (i < nI && validJ && I >= J) {
                double* lo = P + (long long)(kLm0 + 3 * I) * ld + kLm0 + 3 * J;
                double* up = P + (long long)(kLm0 + 3 * J) * ld + kLm0 + 3 * I;
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        if (I > J || r >= c) {  // (a diagonal block: its lower triangle and the mirror)
                            const double v = acc[i][3 * r + c];
                            nonFinite = nonFinite || !isfinite(v);
                            lo[(long long)r * ld + c] = v;
                            up[(long long)c * ld + r] = v;
                        }
            }
        }
    }
    if (nonFinite) a.verdict[1] = 1;
}

// One workgroup: spread trace, total trace (lane t sums the entries t, t + 256, ... serially, then a fixed tree), and info.  block = 256
__global__ __launch_bounds__(256) void k_mix_report(MixArgs a) {
    const int tid = threadIdx.x, nn = kLm0 + 3 * a.N;
    __shared__ double sS[256], sP[256];
    double s = 0.0, p = 0.0;
    for (int j = tid; j < nn; j += 256) {
        const double mj = a.centred ? a.mean[j] : 0.0;
        double sj = 0.0;
        for (int k = 0; k < a.n; ++k) {
            const MixMember m = a.mem[k];
            const double d = a.err[(long long)m.b * a.ld + j] - mj;
            sj = fma(m.w * d, d, sj);
        }
        s += sj;
        p += a.P[(long long)j * a.ld + j];
    }
    sS[tid] = s;
    sP[tid] = p;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) {
            sS[tid] += sS[tid + h];
            sP[tid] += sP[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {
        a.out[0] = sS[0];
        a.out[1] = sP[0];
        const int nf = a.verdict[1] != 0 || !isfinite(sS[0]) || !isfinite(sP[0]);
        a.verdict[2] = a.verdict[0] ? -1 : (nf ? 1 : 0);
    }
}

// P from the scratch image into the destination's covariance (internal extent 12 + 3 N).  grid = (ceil(nn / 256), nn), block = 256
__global__ __launch_bounds__(256) void k_mix_store(MixArgs a) {
    if (a.verdict[2] != 0) return;
    const int nn = kLm0 + 3 * a.N, c = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (c < nn) a.Sigma[(long long)a.dst * a.sigmaStride + (long long)r * a.ld + c] = a.P[(long long)r * a.ld + c];
}

// The staged small state into the destination; from the reference the records k_clone_small copies.  grid = ceil(max(cap, 1) / 256), block = 256
__global__ __launch_bounds__(256) void k_mix_commit(MixArgs a) {
    if (a.verdict[2] != 0) return;
    const int cap = a.cap, N = a.N, d = a.dst, s = a.ref;
    const int tid = blockIdx.x * 256 + threadIdx.x, nth = gridDim.x * 256;
    if (blockIdx.x == 0 && threadIdx.x < int(sizeof(Glob) / 8)) {
        const unsigned long long* gs = reinterpret_cast<const unsigned long long*>(a.stG);
        reinterpret_cast<unsigned long long*>(a.g + d)[threadIdx.x] = gs[threadIdx.x];
    }
    for (int i = tid; i < cap; i += nth) {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.p0[((long long)d * 3 + c) * cap + i] = a.stP0[(long long)c * cap + i];
#pragma unroll
        for (int c = 0; c < 5; ++c) a.Q[((long long)d * 5 + c) * cap + i] = a.stQ[(long long)c * cap + i];
    }
    if (d != s) {
        for (int i = tid; i < 2 * N; i += nth) a.delta[(long long)d * 2 * cap + i] = a.delta[(long long)s * 2 * cap + i];
        for (int i = tid; i < kLm0 + 3 * N; i += nth) a.gamma[(long long)d * (kLm0 + 3 * cap) + i] = a.gamma[(long long)s * (kLm0 + 3 * cap) + i];
        for (int i = tid; i < 9 + 3 * N; i += nth) a.gammaTot[(long long)d * (9 + 3 * cap) + i] = a.gammaTot[(long long)s * (9 + 3 * cap) + i];
        if (a.innov)
            for (int i = tid; i < kInnovHead + N; i += nth) a.innov[(long long)d * (kInnovHead + cap) + i] = a.innov[(long long)s * (kInnovHead + cap) + i];
    }
}

// What k_clone_restore does for the destination, behind the verdict and without the sticky flag.  grid = ceil(max(N, 1) / 128), block = 128
__global__ __launch_bounds__(128) void k_mix_restore(MixArgs a) {
    if (a.verdict[2] != 0) return;
    const int cap = a.cap, b = a.dst;
    const int tid = blockIdx.x * 128 + threadIdx.x;
    Glob& s = a.g[b];
    int bad = 0;
    for (int i = tid; i < a.N; i += gridDim.x * 128) {
        double cst[15];
        landmarkConstants(mk3(a.p0[((long long)b * 3 + 0) * cap + i], a.p0[((long long)b * 3 + 1) * cap + i], a.p0[((long long)b * 3 + 2) * cap + i]), cst, &bad);
        for (int c = 0; c < 15; ++c) a.lmc[((long long)b * 15 + c) * cap + i] = cst[c];
    }
    if (tid == 0 && s.initialised) {
        double e0[3], cd[6], ci[6];
        poseConstants(quat{s.P0q[0], s.P0q[1], s.P0q[2], s.P0q[3]}, e0, cd, ci, &bad);
        for (int i = 0; i < 3; ++i) s.eta0[i] = e0[i];
        for (int i = 0; i < 6; ++i) {
            s.cDiff[i] = cd[i];
            s.cInv[i] = ci[i];
        }
    }
}

}  // namespace eqf
