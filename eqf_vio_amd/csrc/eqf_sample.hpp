// Draws from a filter's covariance and the group step that moves a filter by one (eqf_sample_sigma, eqf_apply_increment,
// eqf_perturb_filters).
//
// eqf_get_nees's launches with nrhs = 0 (eqf_factor.hpp, k_nees_tail) leave A = L L^T of a trailing principal submatrix of Sigma or Sigma_loc in the lower triangle of the
// scratch image (padded layout of eqf_device.hpp, the structural pad index 11 a row of the identity).  Two kernels are added:
//   k_sample_trmm      E = Z L^T, sixteen samples (one MFMA tile of rows) per workgroup and 64-wide block column C of the result:
//                        E[:, C] = sum_{K <= C} Z[:, K] L[C, K]^T,   K ascending,
//                      each term a 16 x 64 x 64 product on v_mfma_f64_16x16x4_f64 (mmTile: the short-block-row branch of k_factor_trail with the
//                      sign turned).  The workgroup walks block row C of L, whose rows are contiguous, once; the diagonal block contributes
//                      its lower triangle only.  Rows of Z and E are in the submatrix' own padded index map (column = internal index - off),
//                      which is the host's to build (eqf_sample_host.hpp).  The sum over K and the k-steps of an MFMA run in one fixed order
//                      and nothing is shared between filters: bit for bit the same from run to run and for a filter alone or in a batch.
//   k_apply_increment  bias += gamma[0:6], X <- VIOExp(liftInnovation(gamma[6:], xi0)) X  (VIOFilter.cpp:292-296 with useInnovationLift =
//                      false; EqFMatrices.cpp:35-67, VIOGroup.cpp:92-110, :245-255): the arithmetic of updateFinishBody's plain branch,
//                      expression for expression, as a launch of its own -- one workgroup per filter, lane 0 the SE(3) and scalar part, the
//                      other lanes the landmarks.  Sigma, xi0, the clock and the integrator are not touched.  With the option
//                      "innovation_lift" on, k_lift_tail (eqf_lift.hpp) runs in front of it and moves the filters that take the bundleLift;
//                      this kernel passes over them (IncArgs::lift) and moves the others exactly as before.
#pragma once
#include "eqf_chol64.hpp"
#include "eqf_device.hpp"
#include "eqf_math.hpp"
#include "eqf_nees.hpp"

namespace eqf {

constexpr int kSampleMax = 64;  // samples per call
constexpr int kSampleLdsBytes = int(sizeof(double)) * (kNeesRhs + kSB) * kSP;  // Z tile | L block  (41 KB)

struct SampleArgs {
    const Glob* g;
    const double* A;      // [B] factored images (NeesArgs::A after the factorisation)
    int ld;
    long long strideA;
    const double* Z;      // [B][nsamp][ldE]: row k = sample k, column i = entry off + i
    double* E;            // [B][nsamp][ldE]
    int ldE, nsamp;
    const double* scale;  // [B] or nullptr (all 1)
    int off;
};

// grid = (block columns of the largest submatrix, row tiles, B), block = 256, LDS = kSampleLdsBytes
__global__ __launch_bounds__(256) void k_sample_trmm(SampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smemS[];
    double (*sZ)[kSP] = reinterpret_cast<double (*)[kSP]>(smemS);
    double (*sL)[kSP] = sZ + kNeesRhs;
    const int b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int m = kLm0 + 3 * a.g[b].N - a.off, C0 = kSB * (int)blockIdx.x;
    if (C0 >= m) return;
    const int pad = kBase - a.off;  // index of the structural pad row in the submatrix (negative: not part of it)
    const double* A = a.A + (long long)b * a.strideA + (long long)a.off * a.ld + a.off;
    const int rows = min(kNeesRhs, a.nsamp - kNeesRhs * (int)blockIdx.y);  // (the last tile may be a short one)
    const long long row0 = ((long long)b * a.nsamp + kNeesRhs * (int)blockIdx.y) * a.ldE;
    const double* Z = a.Z + row0;
    double* E = a.E + row0;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int K = 0; K <= (int)blockIdx.x; ++K) {
        const int c0 = kSB * K;
        for (int e = tid; e < kNeesRhs * kSB; e += 256) {
            const int rr = e >> 6, gc = c0 + (e & 63);
            sZ[rr][e & 63] = (rr < rows && gc < m && gc != pad) ? Z[(long long)rr * a.ldE + gc] : 0.0;
        }
        for (int e = tid; e < kSB * kSB; e += 256) {
            const int rr = e >> 6, cc = e & 63, gr = C0 + rr, gc = c0 + cc;
            double v = 0.0;
            if (gr == pad || gc == pad) v = gr == gc ? 1.0 : 0.0;
            else if (gr < m && gc <= gr) v = A[(long long)gr * a.ld + gc];  // (lower triangle only)
            sL[rr][cc] = v;
        }
        __syncthreads();
        // 16 x 64: wave wv owns the 16 columns C0 + 16 wv ..
        acc = mmTile<true, kSB>(acc, &sZ[0][0], kSP, 0, &sL[0][0], kSP, kQB * wv, lane, 1.0);
        __syncthreads();
    }
    const double s = a.scale ? a.scale[b] : 1.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int rr = (lane >> 4) + 4 * q, gc = C0 + kQB * wv + (lane & 15);
        if (rr < rows && gc < m) E[(long long)rr * a.ldE + gc] = s * acc[q];
    }
}

struct IncArgs {
    Glob* g;              // current scalar state [B], updated in place
    const double* p0;     // [B][3][cap]
    double* Q;            // [B][5][cap], updated in place
    int cap;
    const double* gamma;  // filter b: gamma[b * strideG + j] is the increment's entry of internal index off + j; entries below off are 0
    long long strideG;
    int off;
    const unsigned char* mask;  // [B] or nullptr: 0 leaves the filter alone
    const double* info;         // eqf_nees.hpp's result records [B][kNeesHead + kNeesRhs] or nullptr: a failed factorisation leaves it alone
    const double* lift;         // eqf_lift.hpp's records [B][liftStride] or nullptr: a filter whose entry 0 (the kind of its lift) is not 0
    int liftStride;             // has been dealt with by k_lift_tail
};

// grid = B, block = 256
__global__ __launch_bounds__(256) void k_apply_increment(IncArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    if (a.mask && !a.mask[b]) return;
    if (a.info && a.info[(long long)b * (kNeesHead + kNeesRhs) + 3] != 0.0) return;
    if (a.lift && a.lift[(long long)b * a.liftStride] != 0.0) return;
    Glob& g = a.g[b];
    const int N = g.N, cap = a.cap, n = kLm0 + 3 * N;
    const double* G = a.gamma + (long long)b * a.strideG;
    const int off = a.off;
    // an increment that is not finite moves nothing (every thread looks at its share before anybody writes)
    int nf = 0;
    for (int j = off + tid; j < n; j += 256) {
        const double v = G[j - off];
        if (!(fabs(v) < __builtin_inf())) nf = 1;
    }
    if (__syncthreads_or(nf)) return;
    auto gam = [&](int j) { return j >= off ? G[j - off] : 0.0; };
    if (tid == 0) {
        // VIOExp(liftInnovation(gamma_e, xi0)), EqFMatrices.cpp:35-49
        const d3 v0 = mk3(g.v0[0], g.v0[1], g.v0[2]);
        const d3 gv = mk3(gam(8), gam(9), gam(10));
        const d3 eta = mk3(g.eta0[0], g.eta0[1], g.eta0[2]);
        const double g6 = gam(6), g7 = gam(7);
        const d3 t = mk3(g.cInv[0] * g6 + g.cInv[1] * g7, g.cInv[2] * g6 + g.cInv[3] * g7, g.cInv[4] * g6 + g.cInv[5] * g7);
        const d3 Uw = neg(crs(eta, t));
        const se3 DA = se3Exp(Uw, mk3(0, 0, 0));
        const d3 Dw = sub(neg(gv), crs(Uw, v0));
        const se3 A = se3{quat{g.Aq[0], g.Aq[1], g.Aq[2], g.Aq[3]}, mk3(g.Ax[0], g.Ax[1], g.Ax[2])};
        const se3 An = se3mul(DA, A);                                        // X = Delta * X  (VIOFilter.cpp:296, VIOGroup.cpp:95)
        const d3 wn = add(Dw, qrot(DA.q, mk3(g.w[0], g.w[1], g.w[2])));       // :96
        g.Aq[0] = An.q.w; g.Aq[1] = An.q.x; g.Aq[2] = An.q.y; g.Aq[3] = An.q.z;
        g.Ax[0] = An.x.x; g.Ax[1] = An.x.y; g.Ax[2] = An.x.z;
        g.w[0] = wn.x; g.w[1] = wn.y; g.w[2] = wn.z;
#pragma unroll
        for (int i = 0; i < 6; ++i) g.bias[i] += gam(i);  // VIOFilter.cpp:295
    } else if (tid >= 64) {
        // per-landmark part of Delta and Q_i <- Delta_i Q_i   (EqFMatrices.cpp:54-63, SOT3Exp, VIOGroup.cpp:105-107)
        double* Q = a.Q + (long long)b * 5 * cap;
        const double* p0 = a.p0 + (long long)b * 3 * cap;
        for (int i = tid - 64; i < N; i += 192) {
            const d3 qi = mk3(p0[i], p0[cap + i], p0[2 * cap + i]);
            const d3 gq = mk3(gam(kLm0 + 3 * i), gam(kLm0 + 3 * i + 1), gam(kLm0 + 3 * i + 2));
            quat Qn;
            double an;
            landmarkStep(qi, gq, Q, cap, i, &Qn, &an);
            Q[i] = Qn.w; Q[cap + i] = Qn.x; Q[2 * cap + i] = Qn.y; Q[3 * cap + i] = Qn.z;
            Q[4 * cap + i] = an;
        }
    }
}

}  // namespace eqf
