// Covariance in the coordinates of the ESTIMATE (eqf_get_sigma_local, eqf_get_marginals, eqf_get_local_jacobian).
//
// Sigma is the covariance of eps = chart_xi0(phi_{X^-1}(xi)), i.e. of coordinates around the ORIGIN xi0 -- what the reference returns
// too (VIOFilter.cpp:306-309, "TODO: propagate to local tangent space").  The error a caller can measure is
// eps_loc = chart_xiHat(xi), xiHat = phi_X(xi0) the estimate; to first order eps_loc = J eps with a BLOCK-DIAGONAL J, because the group
// action with X fixed acts component by component (VIOGroup.cpp:23-45):
//   [0,6)  bias                 I
//   [6,8)  gravity direction    G = stereoSphereChartDiff(etaHat, etaHat) R_A^T stereoSphereChartInvDiff(0, eta0)      (2 x 2)
//                               eta0 = R_P0^T e3 (VIOState.cpp:90), etaHat = R_A^T eta0
//   [8,11) velocity             R_A^T
//   landmark i                  a_i^-1 R(q_i)^T   (the differential of Q_i^-1 p, SOT3.cpp:121)
// so Sigma_loc = J Sigma J^T block by block: (Sigma_loc)_IJ = J_I Sigma_IJ J_J^T.
//
//   k_local_jacobian  the J blocks of `count` filters from Glob / Q[5][cap]: per filter a record [kJacHead + 9 cap]
//   k_sigma_local     one pass over Sigma (read n^2, write n^2 values): the access pattern of k_riccati_stream -- one lane per COLUMN
//                     landmark with J_J in registers, a workgroup walks kLocalRows ROW landmarks whose J_I are wave-uniform LDS reads --
//                     without the base-panel coupling.  Sigma is only read.
//   k_marginals       the 11 x 11 base block and the N diagonal 3 x 3 blocks, one lane per landmark (O(N))
// The two covariance kernels share the device functions below, with pinned roundings, so a marginal block is bit for bit the block
// of the full matrix.
#pragma once
#include "eqf_device.hpp"
#include "eqf_math.hpp"
#include "eqf_observe_host.hpp"

namespace eqf {

constexpr int kJacHead = 16;  // G (4) at 0, R_A^T (9) at 4, [13] = 1.0 if the gravity chart is singular (SO3.cpp:160), then J_i [cap][9]
constexpr int kLocalRows = 16;

struct LocalArgs {
    const Glob* g;
    const double* Q;  // [B][5][cap]
    int cap, b0;      // filters b0 + blockIdx.z (k_sigma_local) / b0 + blockIdx.y (k_local_jacobian)
    double* jac;      // [B][kJacHead + 9 cap]
    const double* Sin;
    double* Sout;     // same padded layout as Sigma (eqf_device.hpp)
    int ld;
    long long sigmaStride;
};

__host__ __device__ inline long long jacStride(int cap) { return kJacHead + 9LL * cap; }

// Base part of J applied to 11 values (a column of J_b S, or a row of S J_b^T -- J_b is block diagonal, so both are this)
EQF_DI void baseApply(const double* G, const double* RAt, const double* in, double* out) {
#pragma unroll
    for (int k = 0; k < 6; ++k) out[k] = in[k];
    out[6] = fma(G[1], in[7], G[0] * in[6]);
    out[7] = fma(G[3], in[7], G[2] * in[6]);
#pragma unroll
    for (int r = 0; r < 3; ++r) out[8 + r] = dot3(RAt[3 * r], in[8], RAt[3 * r + 1], in[9], RAt[3 * r + 2], in[10]);
}
// A (3x3) S (3x3) B^T (3x3), row-major
EQF_DI void localBlock(const double* A, const double* S, const double* B, double* out) {
    double T[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) T[3 * r + c] = dot3(A[3 * r], S[c], A[3 * r + 1], S[3 + c], A[3 * r + 2], S[6 + c]);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) out[3 * r + c] = dot3(T[3 * r], B[3 * c], T[3 * r + 1], B[3 * c + 1], T[3 * r + 2], B[3 * c + 2]);
}
// Sigma_bb -> J_b Sigma_bb J_b^T, element (rr, cc) by thread tid < 121; sT is an [11][12] LDS scratch, S row-major with leading dimension ld
EQF_DI void localBaseBlock(const double* G, const double* RAt, const double* S, int ld, double (*sT)[12], int tid, double* out, int ldo) {
    if (tid < 11) {  // column tid of J_b Sigma_bb
        double in[11], o[11];
#pragma unroll
        for (int k = 0; k < 11; ++k) in[k] = S[(long long)k * ld + tid];
        baseApply(G, RAt, in, o);
#pragma unroll
        for (int k = 0; k < 11; ++k) sT[k][tid] = o[k];
    }
    __syncthreads();
    if (tid < 11) {  // row tid of (J_b Sigma_bb) J_b^T
        double in[11], o[11];
#pragma unroll
        for (int k = 0; k < 11; ++k) in[k] = sT[tid][k];
        baseApply(G, RAt, in, o);
#pragma unroll
        for (int k = 0; k < 11; ++k) out[(long long)tid * ldo + k] = o[k];
    }
}

// grid = (ceil(max(N, 1) / 256), count), block = 256
__global__ __launch_bounds__(256) void k_local_jacobian(LocalArgs a) {
    const int b = a.b0 + blockIdx.y;
    const Glob& s = a.g[b];
    const int cap = a.cap;
    double* jac = a.jac + b * jacStride(cap);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) {
        int bad = 0;
        const quat Aq = quat{s.Aq[0], s.Aq[1], s.Aq[2], s.Aq[3]};
        const m33 RAt = q2m(qinv(Aq));
        const d3 eta0 = qrot(qinv(quat{s.P0q[0], s.P0q[1], s.P0q[2], s.P0q[3]}), mk3(0, 0, 1));  // VIOState.cpp:90
        const d3 etaHat = qrot(qinv(Aq), eta0);                                                    // VIOGroup.cpp:58
        double cd[6], ci[6], M[6];
        stereoChartDiff(etaHat, etaHat, cd, &bad);
        stereoChartInvDiffAtZero(eta0, ci, &bad);
#pragma unroll
        for (int r = 0; r < 2; ++r)  // M = cd R_A^T (2 x 3)
#pragma unroll
            for (int c = 0; c < 3; ++c) M[3 * r + c] = dot3(cd[3 * r], RAt.a[c], cd[3 * r + 1], RAt.a[3 + c], cd[3 * r + 2], RAt.a[6 + c]);
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = 0; c < 2; ++c) jac[2 * r + c] = dot3(M[3 * r], ci[c], M[3 * r + 1], ci[2 + c], M[3 * r + 2], ci[4 + c]);
#pragma unroll
        for (int k = 0; k < 9; ++k) jac[4 + k] = RAt.a[k];
        jac[13] = bad ? 1.0 : 0.0;
        jac[14] = 0.0;
        jac[15] = 0.0;
    }
    if (i < s.N) {
        const double* q = a.Q + (long long)b * 5 * cap;
        observe::landmarkJ(quat{q[i], q[cap + i], q[2 * cap + i], q[3 * cap + i]}, q[4 * cap + i], jac + kJacHead + 9LL * i);
    }
}

// grid = (ceil(max(N) / 256), ceil(max(N) / kLocalRows) (at least 1), count), block = 256 (4 waves = 4 strips of 64 column landmarks).
// The workgroups of the first row chunk also write the base rows and columns of their column landmarks, its first workgroup the base block.
__global__ __launch_bounds__(256) void k_sigma_local(LocalArgs a) {
    const int b = a.b0 + blockIdx.z;
    const int N = a.g[b].N;
    const int tid = threadIdx.x;
    const int I0 = blockIdx.y * kLocalRows;
    const int J = blockIdx.x * 256 + tid;
    if (I0 >= N && blockIdx.y != 0) return;
    if (blockIdx.x * 256 >= N && !(blockIdx.x == 0 && blockIdx.y == 0)) return;
    const int ld = a.ld;
    const double* Sin = a.Sin + (long long)b * a.sigmaStride;
    double* Sout = a.Sout + (long long)b * a.sigmaStride;
    const double* jac = a.jac + b * jacStride(a.cap);
    const int nI = max(0, min(kLocalRows, N - I0));
    const bool validJ = J < N;
    const double* colIn = Sin + kLm0 + 3 * (validJ ? J : 0);
    double* colOut = Sout + kLm0 + 3 * (validJ ? J : 0);
    __shared__ double sRow[kLocalRows][9];
    __shared__ double sHead[kJacHead];
    __shared__ double sT[11][12];
    for (int e = tid; e < nI * 9; e += 256) sRow[e / 9][e % 9] = jac[kJacHead + 9LL * I0 + e];
    if (tid < kJacHead) sHead[tid] = jac[tid];
    double JJ[9];
    {
        const double* jj = jac + kJacHead + 9LL * (validJ ? J : 0);
#pragma unroll
        for (int k = 0; k < 9; ++k) JJ[k] = validJ ? jj[k] : 0.0;
    }
    double S[9];
    auto fetch = [&](int i) {
        const long long ro = (long long)(kLm0 + 3 * (I0 + i)) * ld;
#pragma unroll
        for (int rr = 0; rr < 3; ++rr)
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) S[3 * rr + cc] = colIn[ro + (long long)rr * ld + cc];
    };
    if (nI > 0) fetch(0);
    __syncthreads();
    if (blockIdx.y == 0) {
        const double* G = sHead;
        const double* RAt = sHead + 4;
        if (validJ) {
            // Sigma_bJ (11 x 3) -> J_b Sigma_bJ J_J^T ; Sigma_Jb (3 x 11) -> J_J Sigma_Jb J_b^T (read as stored, not as the transpose)
            double T[3][11];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                double in[11];
#pragma unroll
                for (int k = 0; k < 11; ++k) in[k] = colIn[(long long)k * ld + c];
                baseApply(G, RAt, in, T[c]);
            }
#pragma unroll
            for (int k = 0; k < 11; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) colOut[(long long)k * ld + c] = dot3(T[0][k], JJ[3 * c], T[1][k], JJ[3 * c + 1], T[2][k], JJ[3 * c + 2]);
            const double* rowIn = Sin + (long long)(kLm0 + 3 * J) * ld;
            double* rowOut = Sout + (long long)(kLm0 + 3 * J) * ld;
            double U[3][11];
#pragma unroll
            for (int k = 0; k < 11; ++k) {
                const double s0 = rowIn[k], s1 = rowIn[ld + k], s2 = rowIn[2 * (long long)ld + k];
#pragma unroll
                for (int r = 0; r < 3; ++r) U[r][k] = dot3(JJ[3 * r], s0, JJ[3 * r + 1], s1, JJ[3 * r + 2], s2);
            }
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                double o[11];
                baseApply(G, RAt, U[r], o);
#pragma unroll
                for (int k = 0; k < 11; ++k) rowOut[(long long)r * ld + k] = o[k];
                rowOut[(long long)r * ld + 11] = 0.0;  // the structural pad row / column 11
                colOut[(long long)11 * ld + r] = 0.0;
            }
        }
        if (blockIdx.x == 0) {
            localBaseBlock(G, RAt, Sin, ld, sT, tid, Sout, ld);
            if (tid < 12) {
                Sout[(long long)tid * ld + 11] = 0.0;
                Sout[(long long)11 * ld + tid] = 0.0;
            }
        }
    }
    for (int i = 0; i < nI; ++i) {
        double Sc[9], O[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) Sc[k] = S[k];
        if (i + 1 < nI) fetch(i + 1);  // next block's loads fly during this block's arithmetic
        localBlock(sRow[i], Sc, JJ, O);  // (sRow[i]: wave-uniform LDS broadcast reads)
        const long long ro = (long long)(kLm0 + 3 * (I0 + i)) * ld;
        if (validJ) {
#pragma unroll
            for (int rr = 0; rr < 3; ++rr)
#pragma unroll
                for (int cc = 0; cc < 3; ++cc) colOut[ro + (long long)rr * ld + cc] = O[3 * rr + cc];
        }
    }
}

// out = base block (11 x 11 row-major) then N diagonal blocks (9 each), in origin (local = 0) or local coordinates.
// grid = ceil(max(N, 1) / 256), block = 256
__global__ __launch_bounds__(256) void k_marginals(LocalArgs a, int local, double* out) {
    const int b = a.b0;
    const int N = a.g[b].N;
    const int tid = threadIdx.x;
    const int i = blockIdx.x * 256 + tid;
    const int ld = a.ld;
    const double* Sin = a.Sin + (long long)b * a.sigmaStride;
    const double* jac = a.jac + b * jacStride(a.cap);
    if (i < N) {
        const double* d = Sin + (long long)(kLm0 + 3 * i) * ld + kLm0 + 3 * i;
        double S[9], O[9];
#pragma unroll
        for (int rr = 0; rr < 3; ++rr)
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) S[3 * rr + cc] = d[(long long)rr * ld + cc];
        if (local) {
            double JJ[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) JJ[k] = jac[kJacHead + 9LL * i + k];
            localBlock(JJ, S, JJ, O);
        } else {
#pragma unroll
            for (int k = 0; k < 9; ++k) O[k] = S[k];
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) out[121 + 9LL * i + k] = O[k];
    }
    if (blockIdx.x == 0) {
        __shared__ double sT[11][12];
        __shared__ double sHead[kJacHead];
        if (local) {
            if (tid < kJacHead) sHead[tid] = jac[tid];
            __syncthreads();
            localBaseBlock(sHead, sHead + 4, Sin, ld, sT, tid, out, 11);
        } else if (tid < 121) {
            out[tid] = Sin[(long long)(tid / 11) * ld + tid % 11];
        }
    }
}

}  // namespace eqf
