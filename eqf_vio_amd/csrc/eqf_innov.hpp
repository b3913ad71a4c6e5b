// Innovation statistics of a vision update (eqf_set_option "innovation_stats", eqf_get_innovation_stats).
//
// The S-chain (eqf_chol64.hpp) factors S = C Sigma C^T + R = L L^T and solves z = L^-1 delta on the device in every update; the two numbers a
// filter is tuned by fall out of what it leaves behind:
//   nis      = delta^T S^-1 delta = z^T z            z is column 11 of the solved right-hand sides (ChainArgs::WO = YO: delta rides in the
//                                                    structurally empty column 11 of C Sigma, yCols in eqf_update.hpp)
//   logdet_S = 2 sum_k log L_kk                      L_kk from the diagonal-factor records (ChainArgs::D = SL, kDRec doubles per block column)
//   loglik   = -(nis + logdet_S + dof log 2 pi) / 2, dof = 2 N
//   nis_lm[i] = delta_i^T S_ii^-1 delta_i            S_ii = C_i Sigma_ii C_i^T + r I from the per-landmark constants and the PRE-update Sigma,
//                                                    which the ping-pong leaves intact
// k_innov_stats is a tail launch behind the update's launches, one workgroup per filter, and only exists in the stream when the option is
// on: with the option off the launches of an update are what they were.  The chains are fp64 in every build, and every launch shape of the
// factorisation leaves the same bits in YO and SL; the sums here run in ONE fixed order (lane t takes the terms t, t + 256, ... in
// sequence, then a fixed tree over the 256 partial sums), so the statistics are bit for bit the same under every launch shape and from
// run to run.  Only the rows [0, 2 N) of the filter's own chain are summed: the identity padding (log 1 = 0, z = 0) is not read at all.
#pragma once
#include "eqf_chol64.hpp"
#include "eqf_device.hpp"
#include "eqf_update.hpp"

namespace eqf {

constexpr int kInnovHead = 8;  // per filter [kInnovHead + cap]: nis, logdet_S, dof, loglik, valid, 3 reserved; then nis_lm[cap]

struct InnovArgs {
    const Glob* g;
    const double* YO;     // solved right-hand sides of the S-chain, row-major, column 11 = z
    int ldY;
    long long strideY;
    const double* SL;     // diagonal-factor records of the S-chain
    long long strideDS;
    const double* delta;  // [B][2 cap]
    const double* lmc;    // [B][15][cap], rows 0..5 = C0i (2 x 3)
    const double* Sin;    // Sigma before the update
    int ld, cap;
    long long sigmaStride;
    double measurementVariance;
    double* out;          // [B][kInnovHead + cap]
};

// grid = B, block = 256
__global__ __launch_bounds__(256) void k_innov_stats(InnovArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const Glob& g = a.g[b];
    const int N = g.N;
    if (!g.updateOk || N == 0) return;  // (no update ran for this filter: its record keeps valid = 0 from the start of the vision call)
    double* out = a.out + (long long)b * (kInnovHead + a.cap);
    const int m = sDim(N);
    const double* z = a.YO + (long long)b * a.strideY + 11;
    const double* D = a.SL + (long long)b * a.strideDS;
    double sz = 0.0, sl = 0.0;
    for (int k = tid; k < m; k += 256) {
        const double zk = z[(long long)k * a.ldY];
        sz = fma(zk, zk, sz);
        sl += log(D[(long long)(k / kSB) * kDRec + (k % kSB) * (kSB + 1)]);
    }
    __shared__ double sA[256], sB[256];
    sA[tid] = sz;
    sB[tid] = sl;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            sA[tid] += sA[tid + w];
            sB[tid] += sB[tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double nis = sA[0], logdet = 2.0 * sB[0], dof = (double)m;
        out[0] = nis;
        out[1] = logdet;
        out[2] = dof;
        out[3] = -0.5 * (nis + logdet + dof * 1.8378770664093453 /* log 2 pi */);
        out[4] = 1.0;
    }
    const double* Sin = a.Sin + (long long)b * a.sigmaStride;
    const double* lmc = a.lmc + (long long)b * 15 * a.cap;
    const double* delta = a.delta + (long long)b * 2 * a.cap;
    for (int i = tid; i < N; i += 256) {
        double C[6], S[9];
#pragma unroll
        for (int k = 0; k < 6; ++k) C[k] = lmc[(long long)k * a.cap + i];
        const double* d = Sin + (long long)(kLm0 + 3 * i) * a.ld + kLm0 + 3 * i;
#pragma unroll
        for (int rr = 0; rr < 3; ++rr)
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) S[3 * rr + cc] = d[(long long)rr * a.ld + cc];
        double T[6];  // C Sigma_ii (2 x 3)
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) T[3 * r + c] = dot3(C[3 * r], S[c], C[3 * r + 1], S[3 + c], C[3 * r + 2], S[6 + c]);
        // the LOWER triangle of S_ii, like the chain
        const double s00 = dot3(T[0], C[0], T[1], C[1], T[2], C[2]) + a.measurementVariance;
        const double s10 = dot3(T[3], C[0], T[4], C[1], T[5], C[2]);
        const double s11 = dot3(T[3], C[3], T[4], C[4], T[5], C[5]) + a.measurementVariance;
        // 2 x 2 Cholesky: l00 = sqrt(s00), l10 = s10 / l00, l11 = sqrt(s11 - l10^2); w = L^-1 delta_i
        const double l00 = sqrt(s00), l10 = s10 / l00, l11 = sqrt(fma(-l10, l10, s11));
        const double w0 = delta[2 * i] / l00, w1 = fma(-l10, w0, delta[2 * i + 1]) / l11;
        out[kInnovHead + i] = fma(w1, w1, w0 * w0);
    }
}

}  // namespace eqf
