// Non-mutating forecast (eqf_forecast): what the filter WOULD hold after K processIMUData calls and an integrateUpToTime(t1), for the
// state, the base block, every landmark's diagonal block and the bearing quantities that follow from them -- read from the handle, written
// to a scratch record, O(N).
//
// With F = [[F_bb, 0], [L, D]], D block-diagonal (eqf_propagate.hpp), the Riccati step closes on the 14 x 14 marginal of the base and ONE
// landmark:
//     Sigma'_bb = F_bb Sigma_bb F_bb^T + T (P_bb + B_b R B_b^T)
//     G_I       = Lw_I Sigma[0:3, b] + Lv_I Sigma[8:11, b] + D_I Sigma_Ib                                   (3 x 11)
//     Sigma'_Ib = G_I F_bb^T - sigma_w^2 Lw_I Nb^T
//     Sigma'_II = (D_I Sigma_II + Lw_I Sigma_wI + Lv_I Sigma_vI) D_I^T + (G_I[:,0:3] + (sigma_w^2 / T) Lw_I) Lw_I^T + G_I[:,8:11] Lv_I^T + T p I
// with Sigma_wI, Sigma_vI the transposes of the panel's columns 0:3 and 8:11.  So a forecast reads the base block, N panels and N diagonal
// blocks of Sigma and nothing else of it.  Two launches whatever K, N and the batch:
//   k_forecast_build   one workgroup per filter (grid.y): walks the steps in order with the scalar state (a Glob) and Sigma_bb in LDS --
//                      stepCommon / stepGlobal, the filter's own device functions -- and leaves one record per step (forecast::kStepRec
//                      doubles: the common linearisation values, the group step's constants, the rows of Sigma_bb the landmarks need and
//                      the non-trivial entries of F_bb), then the state estimate and the base block of the time reached.  As in
//                      k_build_blocks the two scalar chains of a step run on two wavefronts side by side.
//   k_forecast_lm      one lane per landmark, filters in grid.y: Q_i, the 3 x 11 panel and the 3 x 3 block stay in registers through all
//                      steps (buildBlocks, stepLandmark); the per-step record is a wave-uniform read.  Then p, the bearing, the block in the
//                      chart asked for (localBlock), S = C_i Sigma_ii C_i^T + r I (gateMahalanobis' expression) and the bearing covariance.
// Nothing of the handle is written; the order of every sum is fixed and there are no atomics, so a filter gives the same bits alone or
// anywhere in a batch.  Sigma'_bb and Sigma'_II are computed on the upper triangle and mirrored from the same registers.
#pragma once
#include "eqf_device.hpp"
#include "eqf_forecast_host.hpp"
#include "eqf_local.hpp"
#include "eqf_math.hpp"
#include "eqf_propagate.hpp"

namespace eqf {

namespace fc = forecast;
static_assert(sizeof(ImuRec) == sizeof(double) * fc::kImuRec, "uploaded sample = ImuRec");
static_assert(kBase == 11 && kLm0 == 12, "forecast records assume the 11 (+1 pad) base coordinates");
static_assert(fc::kRecNb + 15 <= fc::kStepRec && fc::kLmFlag < fc::kLmRec && fc::kHeadVel + 3 <= fc::kHead && 121 <= fc::kBaseDoubles, "record layout");
static_assert(sizeof(Glob) % 8 == 0 && sizeof(Glob) / 8 <= 64, "Glob copy is one word per lane");

struct FcArgs {
    const Glob* g;
    const double* p0;   // [B][3][cap]
    const double* Q;    // [B][5][cap]
    const double* lmc;  // [B][15][cap]
    const double* Sin;  // [B][rows][ld]
    long long sigmaStride;
    int cap, ld, B;
    int K, nSteps;      // IMU samples; steps = K (+ 1: the closing integrateUpToTime)
    int local;
    const ImuRec* imu;  // [nSteps][B]
    double* rec;        // [B][kMaxSteps + 1][kStepRec]
    double* out;        // [B][outStride]
    long long outStride;
    Params prm;
};

// what stepCommon / stepLandmark / stepGlobal look at of a call: every forecast step runs the Riccati recursion (fastRiccati = 0)
struct FcStepView {
    const Params& prm;
    int isImu;
    int doRiccati;
};

EQF_DI bool fcFinite(double x) { return fabs(x) <= 1.7976931348623157e308; }  // (false for NaN)

// grid = (1, B), block = 128
__global__ __launch_bounds__(fc::kBuildThreads) void k_forecast_build(FcArgs a) {
    const int b = blockIdx.y, tid = threadIdx.x, wv = tid >> 6, ln = tid & 63;
    __shared__ Glob sG[2];
    __shared__ double sS[2][11][12];
    __shared__ double sTb[11][12], sF[11][12], sNb[11][3];
    __shared__ CommonLds sC;
    __shared__ double sHead[kJacHead];
    __shared__ int sBad[2];
    const Glob& G0 = a.g[b];
    double* head = a.out + (long long)b * a.outStride;
    if (!G0.initialised || G0.curTime < 0) return;  // (the host answers for such a filter: every output zero)
    const double* Sin = a.Sin + (long long)b * a.sigmaStride;
    if (wv == 0 && ln < (int)(sizeof(Glob) / 8)) reinterpret_cast<double*>(&sG[0])[ln] = reinterpret_cast<const double*>(&G0)[ln];
    for (int e = tid; e < 132; e += fc::kBuildThreads) sS[0][e / 12][e % 12] = (e % 12 < 11) ? Sin[(long long)(e / 12) * a.ld + e % 12] : 0.0;
    if (tid < 2) sBad[tid] = 0;
    __syncthreads();
    int cur = 0, curS = 0, nInt = 0, bad = 0;
    for (int s = 0; s < a.nSteps; ++s) {
        const FcStepView view{a.prm, s < a.K ? 1 : 0, 1};
        const ImuRec& r = a.imu[(long long)s * a.B + b];
        const Glob& G = sG[cur];
        const bool step = (G.curTime >= 0) && (r.stamp - G.curTime > 0);  // (LDS: the same answer in every lane)
        double* R = a.rec + ((long long)b * (fc::kMaxSteps + 1) + s) * fc::kStepRec;
        if (wv == 0) {
            if (ln == 0) {
                R[fc::kRecStep] = step ? 1.0 : 0.0;
                if (step) {  // the linearisation's common values
                    StepCommon c;
                    stepCommon(G, r, view, c, kPartBase | kPartRicc, &bad);
                    sC.T = c.T;
                    R[fc::kRecT] = c.T;
#pragma unroll
                    for (int k = 0; k < 6; ++k) {
                        sC.Bg[k] = c.Bg[k];
                        sC.Avg[k] = c.Avg[k];
                    }
#pragma unroll
                    for (int k = 0; k < 9; ++k) {
                        sC.Bvw[k] = c.Bvw.a[k];
                        sC.RA[k] = c.RA.a[k];
                        R[fc::kRecRA + k] = c.RA.a[k];
                    }
                    R[fc::kRecVC] = c.vC.x; R[fc::kRecVC + 1] = c.vC.y; R[fc::kRecVC + 2] = c.vC.z;
                }
            }
        } else {
            // the scalar state: word-parallel copy, then one lane patches the changed fields (stepGlobal's contract)
            if (ln < (int)(sizeof(Glob) / 8)) reinterpret_cast<double*>(&sG[cur ^ 1])[ln] = reinterpret_cast<const double*>(&G)[ln];
            if (ln == 0) {
                StepCommon c;
                c.step = 0;
                if (step) {
                    c.camInv = se3{quat{1, 0, 0, 0}, mk3(0, 0, 0)};  // (only the discrete lift forms it)
                    stepCommon(G, r, view, c, kPartBase | kPartLift, &bad);
                    R[fc::kRecDt] = c.dt;
                    R[fc::kRecCamInv] = c.camInv.q.w; R[fc::kRecCamInv + 1] = c.camInv.q.x; R[fc::kRecCamInv + 2] = c.camInv.q.y;
                    R[fc::kRecCamInv + 3] = c.camInv.q.z;
                    R[fc::kRecCamInv + 4] = c.camInv.x.x; R[fc::kRecCamInv + 5] = c.camInv.x.y; R[fc::kRecCamInv + 6] = c.camInv.x.z;
                    R[fc::kRecOC] = c.oCcur.x; R[fc::kRecOC + 1] = c.oCcur.y; R[fc::kRecOC + 2] = c.oCcur.z;
                    R[fc::kRecVCcur] = c.vCcur.x; R[fc::kRecVCcur + 1] = c.vCcur.y; R[fc::kRecVCcur + 2] = c.vCcur.z;
                }
                stepGlobal(G, &sG[cur ^ 1], r, view, c, &bad);
            }
        }
        __syncthreads();
        if (step) {
            const double T = sC.T;
            for (int e = tid; e < 132; e += fc::kBuildThreads) {
                const int rr = e / 12, cc = e % 12;
                // F_bb = I + T * [[0,0,0,0],[-B_g^w,0,0,0],[-B_v^w,-R_A, A_vg, 0]]   (VIOFilter.cpp:178-183)
                double f = (rr == cc) ? 1.0 : 0.0;
                if (rr >= 6 && rr < 8 && cc < 3) f = -T * sC.Bg[3 * (rr - 6) + cc];
                if (rr >= 8) {
                    if (cc < 3) f = -T * sC.Bvw[3 * (rr - 8) + cc];
                    else if (cc < 6) f = -T * sC.RA[3 * (rr - 8) + cc - 3];
                    else if (cc < 8) f = T * sC.Avg[2 * (rr - 8) + cc - 6];
                }
                sF[rr][cc] = (cc < 11) ? f : 0.0;
                if (rr >= 6 && rr < 8 && cc < 3) R[fc::kRecFg + 3 * (rr - 6) + cc] = f;
                if (rr >= 8 && cc < 8) R[fc::kRecFv + 8 * (rr - 8) + cc] = f;
                if (cc < 3) {
                    double nb = 0.0;
                    if (rr >= 6 && rr < 8) nb = sC.Bg[3 * (rr - 6) + cc];
                    if (rr >= 8) nb = sC.Bvw[3 * (rr - 8) + cc];
                    sNb[rr][cc] = nb;
                    if (rr >= 6) R[fc::kRecNb + 3 * (rr - 6) + cc] = nb;
                }
            }
            if (tid < 66) {  // the rows of Sigma_bb the landmarks' G_I reads, as they are BEFORE this step
                const int rr = tid / 11, cc = tid % 11;
                R[fc::kRecSb + tid] = sS[curS][rr < 3 ? rr : rr + 5][cc];
            }
            __syncthreads();
            if (tid < 121) {
                const int rr = tid / 11, cc = tid % 11;
                double acc = 0;
#pragma unroll
                for (int k = 0; k < 11; ++k) acc += sF[rr][k] * sS[curS][k][cc];
                sTb[rr][cc] = acc;
            }
            __syncthreads();
            // Sigma'_bb = F_bb Sigma_bb F_bb^T + T (P_bb + B_b R B_b^T): the upper triangle, mirrored from the same register
            if (tid < 121) {
                const int rr = tid / 11, cc = tid % 11;
                if (rr <= cc) {
                    const double sw2 = a.prm.velOmegaVariance, sa2 = a.prm.velAccelVariance;
                    double acc = 0;
#pragma unroll
                    for (int k = 0; k < 11; ++k) acc += sTb[rr][k] * sF[cc][k];
                    double nz = 0;
#pragma unroll
                    for (int k = 0; k < 3; ++k) nz += sw2 * sNb[rr][k] * sNb[cc][k];
                    if (rr >= 8 && cc >= 8) {  // accel columns of B: rows 8:11 hold R_A
#pragma unroll
                        for (int k = 0; k < 3; ++k) nz += sa2 * sC.RA[3 * (rr - 8) + k] * sC.RA[3 * (cc - 8) + k];
                    }
                    if (rr == cc) {
                        const Params& p = a.prm;
                        nz += rr < 3 ? p.biasOmegaProcessVariance
                                     : (rr < 6 ? p.biasAccelProcessVariance : (rr < 8 ? p.gravityProcessVariance : p.velocityProcessVariance));
                    }
                    acc += T * nz;
                    sS[curS ^ 1][rr][cc] = acc;
                    sS[curS ^ 1][cc][rr] = acc;
                }
            }
            if (tid < 11) sS[curS ^ 1][tid][11] = 0.0;
            curS ^= 1;
            ++nInt;
            __syncthreads();
        }
        cur ^= 1;
    }
    if (ln == 0) sBad[wv] = bad;
    // ---- the state estimate (k_state_estimate's formulas) and the chart of the time reached (k_local_jacobian's)
    const Glob& s = sG[cur];
    if (tid == 0) {
        const se3 P0 = se3{quat{s.P0q[0], s.P0q[1], s.P0q[2], s.P0q[3]}, mk3(s.P0x[0], s.P0x[1], s.P0x[2])};
        const se3 A = se3{quat{s.Aq[0], s.Aq[1], s.Aq[2], s.Aq[3]}, mk3(s.Ax[0], s.Ax[1], s.Ax[2])};
        const se3 P = se3mul(P0, A);
        const d3 v = qrot(qinv(A.q), mk3(s.v0[0] - s.w[0], s.v0[1] - s.w[1], s.v0[2] - s.w[2]));
        head[fc::kHeadTime] = s.curTime;
        head[fc::kHeadSteps] = (double)nInt;
        head[fc::kHeadPoseQ] = P.q.w; head[fc::kHeadPoseQ + 1] = P.q.x; head[fc::kHeadPoseQ + 2] = P.q.y; head[fc::kHeadPoseQ + 3] = P.q.z;
        head[fc::kHeadPoseX] = P.x.x; head[fc::kHeadPoseX + 1] = P.x.y; head[fc::kHeadPoseX + 2] = P.x.z;
        head[fc::kHeadVel] = v.x; head[fc::kHeadVel + 1] = v.y; head[fc::kHeadVel + 2] = v.z;
    }
    if (tid == 64) {
        int jb = 0;
        const quat Aq = quat{s.Aq[0], s.Aq[1], s.Aq[2], s.Aq[3]};
        const m33 RAt = q2m(qinv(Aq));
        const d3 eta0 = qrot(qinv(quat{s.P0q[0], s.P0q[1], s.P0q[2], s.P0q[3]}), mk3(0, 0, 1));  // VIOState.cpp:90
        const d3 etaHat = qrot(qinv(Aq), eta0);                                                    // VIOGroup.cpp:58
        double cd[6], ci[6], M[6];
        stereoChartDiff(etaHat, etaHat, cd, &jb);
        stereoChartInvDiffAtZero(eta0, ci, &jb);
#pragma unroll
        for (int r = 0; r < 2; ++r)  // M = cd R_A^T (2 x 3)
#pragma unroll
            for (int c = 0; c < 3; ++c) M[3 * r + c] = dot3(cd[3 * r], RAt.a[c], cd[3 * r + 1], RAt.a[3 + c], cd[3 * r + 2], RAt.a[6 + c]);
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = 0; c < 2; ++c) sHead[2 * r + c] = dot3(M[3 * r], ci[c], M[3 * r + 1], ci[2 + c], M[3 * r + 2], ci[4 + c]);
#pragma unroll
        for (int k = 0; k < 9; ++k) sHead[4 + k] = RAt.a[k];
        sHead[13] = jb ? 1.0 : 0.0;
    }
    __syncthreads();
    double* base = head + fc::kHead;
    if (a.local) {
        localBaseBlock(sHead, sHead + 4, &sS[curS][0][0], 12, sTb, tid, base, 11);
    } else if (tid < 121) {
        base[tid] = sS[curS][tid / 11][tid % 11];
    }
    if (tid == 0) {
        int flag = (sBad[0] || sBad[1] || (a.local && sHead[13] != 0.0)) ? fc::kFlagChart : 0;
        bool fin = fcFinite(s.curTime);
#pragma unroll
        for (int k = 0; k < 4; ++k) fin = fin && fcFinite(s.Aq[k]);
#pragma unroll
        for (int k = 0; k < 3; ++k) fin = fin && fcFinite(s.Ax[k]) && fcFinite(s.w[k]);
        for (int k = 0; k < 11; ++k) fin = fin && fcFinite(sS[curS][k][k]);
        if (!fin) flag |= fc::kFlagNonFinite;
        head[fc::kHeadFlag] = (double)flag;
    }
}

// grid = (max(1, ceil(max N / 64)), B), block = 64: one lane per landmark
__global__ __launch_bounds__(fc::kLanes) void k_forecast_lm(FcArgs a) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * fc::kLanes + threadIdx.x;
    const Glob& G0 = a.g[b];
    if (!G0.initialised || G0.curTime < 0) return;
    if (i >= G0.N || i >= a.cap) return;
    const int cap = a.cap, ld = a.ld;
    const double* P0 = a.p0 + (long long)b * 3 * cap;
    const double* q = a.Q + (long long)b * 5 * cap;
    const double* Sin = a.Sin + (long long)b * a.sigmaStride;
    quat Qq = quat{q[i], q[cap + i], q[2 * cap + i], q[3 * cap + i]};
    double Qa = q[4 * cap + i];
    const d3 p0 = mk3(P0[i], P0[cap + i], P0[2 * cap + i]);
    double Pn[3][11], S[9];
    {
        const double* row = Sin + (long long)(kLm0 + 3 * i) * ld;
#pragma unroll
        for (int rr = 0; rr < 3; ++rr) {
#pragma unroll
            for (int cc = 0; cc < 11; ++cc) Pn[rr][cc] = row[(long long)rr * ld + cc];
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) S[3 * rr + cc] = row[(long long)rr * ld + kLm0 + 3 * i + cc];
        }
    }
    const FcStepView view{a.prm, 0, 1};
    const double sw2 = a.prm.velOmegaVariance, ppv = a.prm.pointProcessVariance;
    int bad = 0;
    for (int s = 0; s < a.nSteps; ++s) {
        const double* R = a.rec + ((long long)b * (fc::kMaxSteps + 1) + s) * fc::kStepRec;
        if (R[fc::kRecStep] == 0.0) continue;  // (wave-uniform)
        StepCommon c;
        c.step = 1;
        c.T = R[fc::kRecT];
        c.dt = R[fc::kRecDt];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            c.RA.a[k] = R[fc::kRecRA + k];
            c.RIC.a[k] = a.prm.RIC[k];
            c.RICt.a[k] = a.prm.RICt[k];
        }
        c.xIC = mk3(a.prm.camx[0], a.prm.camx[1], a.prm.camx[2]);
        c.vC = mk3(R[fc::kRecVC], R[fc::kRecVC + 1], R[fc::kRecVC + 2]);
        c.camInv = se3{quat{R[fc::kRecCamInv], R[fc::kRecCamInv + 1], R[fc::kRecCamInv + 2], R[fc::kRecCamInv + 3]},
            mk3(R[fc::kRecCamInv + 4], R[fc::kRecCamInv + 5], R[fc::kRecCamInv + 6])};
        c.oCcur = mk3(R[fc::kRecOC], R[fc::kRecOC + 1], R[fc::kRecOC + 2]);
        c.vCcur = mk3(R[fc::kRecVCcur], R[fc::kRecVCcur + 1], R[fc::kRecVCcur + 2]);
        const LmBlocks blk = buildBlocks(c, Qq, Qa, p0);
        const double* D = blk.D.a;
        const double* Lw = blk.Lw.a;
        const double* Lv = blk.Lv.a;
        const double* Sb = R + fc::kRecSb;  // rows 0:3 then 8:11 of Sigma_bb, 11 columns each
        // G_I = Lw Sigma[0:3, b] + Lv Sigma[8:11, b] + D Sigma_Ib
        double Gm[3][11];
#pragma unroll
        for (int rr = 0; rr < 3; ++rr)
#pragma unroll
            for (int cc = 0; cc < 11; ++cc) {
                double acc = 0;
#pragma unroll
                for (int k = 0; k < 3; ++k) acc += Lw[3 * rr + k] * Sb[11 * k + cc] + Lv[3 * rr + k] * Sb[11 * (3 + k) + cc] + D[3 * rr + k] * Pn[k][cc];
                Gm[rr][cc] = acc;
            }
        // H = D Sigma_II + Lw Sigma_wI + Lv Sigma_vI, the base rows of the landmark's columns taken as the panel's transpose
        double H[9];
#pragma unroll
        for (int rr = 0; rr < 3; ++rr)
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) {
                double acc = 0;
#pragma unroll
                for (int k = 0; k < 3; ++k) acc += D[3 * rr + k] * S[3 * k + cc] + Lw[3 * rr + k] * Pn[cc][k] + Lv[3 * rr + k] * Pn[cc][8 + k];
                H[3 * rr + cc] = acc;
            }
        const double TtP = c.T * ppv, fold = sw2 / c.T;
#pragma unroll
        for (int rr = 0; rr < 3; ++rr)
#pragma unroll
            for (int cc = rr; cc < 3; ++cc) {
                double acc = (rr == cc) ? TtP : 0.0;
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    acc += H[3 * rr + k] * D[3 * cc + k] + (Gm[rr][k] + fold * Lw[3 * rr + k]) * Lw[3 * cc + k] + Gm[rr][8 + k] * Lv[3 * cc + k];
                S[3 * rr + cc] = acc;
                S[3 * cc + rr] = acc;
            }
        // Sigma'_Ib = G_I F_bb^T - sigma_w^2 Lw_I Nb^T through F_bb's sparsity (rows 0..5 of F_bb are rows of the identity)
        const double* Fg = R + fc::kRecFg;
        const double* Fv = R + fc::kRecFv;
        const double* Nb = R + fc::kRecNb;
#pragma unroll
        for (int rr = 0; rr < 3; ++rr) {
#pragma unroll
            for (int cc = 0; cc < 6; ++cc) Pn[rr][cc] = Gm[rr][cc];
#pragma unroll
            for (int cc = 6; cc < 8; ++cc) {
                double acc = Gm[rr][cc];
#pragma unroll
                for (int k = 0; k < 3; ++k) acc += Gm[rr][k] * Fg[3 * (cc - 6) + k];
#pragma unroll
                for (int k = 0; k < 3; ++k) acc -= sw2 * Lw[3 * rr + k] * Nb[3 * (cc - 6) + k];
                Pn[rr][cc] = acc;
            }
#pragma unroll
            for (int cc = 8; cc < 11; ++cc) {
                double acc = Gm[rr][cc];
#pragma unroll
                for (int k = 0; k < 8; ++k) acc += Gm[rr][k] * Fv[8 * (cc - 8) + k];
#pragma unroll
                for (int k = 0; k < 3; ++k) acc -= sw2 * Lw[3 * rr + k] * Nb[3 * (cc - 6) + k];
                Pn[rr][cc] = acc;
            }
        }
        // the group step, from the state BEFORE the step like the blocks
        quat Qo;
        double ao;
        stepLandmark(c, view, Qq, Qa, p0, &Qo, &ao, &bad);
        Qq = Qo;
        Qa = ao;
    }
    double* o = a.out + (long long)b * a.outStride + fc::kHead + fc::kBaseDoubles + (long long)fc::kLmRec * i;
    // p as k_state_estimate forms it, the bearing, and the chart block J_i = a_i^-1 R(q_i)^T as k_local_jacobian forms it
    const d3 ph = scl(1.0 / Qa, qrot(qinv(Qq), p0));
    const double np = nrm3(ph);
    const d3 yh = scl(1.0 / np, ph);
    o[fc::kLmP] = ph.x; o[fc::kLmP + 1] = ph.y; o[fc::kLmP + 2] = ph.z;
    o[fc::kLmBearing] = yh.x; o[fc::kLmBearing + 1] = yh.y; o[fc::kLmBearing + 2] = yh.z;
    const m33 RQ = q2m(Qq);
    const double ia = 1.0 / Qa;
    double JJ[9], Sloc[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) JJ[3 * r + cc] = ia * RQ.a[3 * cc + r];
    localBlock(JJ, S, JJ, Sloc);
#pragma unroll
    for (int k = 0; k < 9; ++k) o[fc::kLmCov + k] = a.local ? Sloc[k] : S[k];
    // S = C_i Sigma_ii C_i^T + r I from the ORIGIN-chart block (gateMahalanobis' expression; lower entry mirrored)
    {
        const double* lc = a.lmc + (long long)b * 15 * cap + i;
        double cm[6], T[6];
#pragma unroll
        for (int e = 0; e < 6; ++e) cm[e] = lc[(long long)e * cap];
#pragma unroll
        for (int rw = 0; rw < 2; ++rw)
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) T[3 * rw + cc] = dot3(cm[3 * rw], S[cc], cm[3 * rw + 1], S[3 + cc], cm[3 * rw + 2], S[6 + cc]);
        const double r = a.prm.measurementVariance;
        const double s00 = dot3(T[0], cm[0], T[1], cm[1], T[2], cm[2]) + r;
        const double s10 = dot3(T[3], cm[0], T[4], cm[1], T[5], cm[2]);
        const double s11 = dot3(T[3], cm[3], T[4], cm[4], T[5], cm[5]) + r;
        o[fc::kLmS] = s00; o[fc::kLmS + 1] = s10; o[fc::kLmS + 2] = s10; o[fc::kLmS + 3] = s11;
    }
    // covariance of the unit bearing: Dm Sigma_loc,ii Dm^T, Dm = (I - yhat yhat^T) / |p|, from the ESTIMATE-chart block; upper triangle mirrored
    {
        const double yv[3] = {yh.x, yh.y, yh.z};
        double Dm[9], Y[9];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) Dm[3 * r + cc] = ((r == cc ? 1.0 : 0.0) - yv[r] * yv[cc]) / np;
        localBlock(Dm, Sloc, Dm, Y);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int cc = r; cc < 3; ++cc) {
                o[fc::kLmYcov + 3 * r + cc] = Y[3 * r + cc];
                o[fc::kLmYcov + 3 * cc + r] = Y[3 * r + cc];
            }
    }
    bool fin = fcFinite(np) && fcFinite(Qa);
#pragma unroll
    for (int k = 0; k < 9; ++k) fin = fin && fcFinite(S[k]) && fcFinite(Sloc[k]);
    o[fc::kLmFlag] = (double)((bad ? fc::kFlagChart : 0) | (fin ? 0 : fc::kFlagNonFinite));
}

}  // namespace eqf
