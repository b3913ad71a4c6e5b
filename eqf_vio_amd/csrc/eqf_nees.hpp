// Joint NEES and log-determinant of the covariance on the device (eqf_get_nees).
//
// For every filter of a handle: A = L L^T of a trailing principal submatrix of Sigma (local = 0) or Sigma_loc (local = 1), with the forward
// solve z = L^-1 e of up to kNeesRhs error vectors carried along:
//   nees_k    = e_k^T A^-1 e_k = z_k^T z_k
//   logdet    = 2 sum log L_ii          min_pivot = min L_ii^2
// The factorisation is eqf_factor.hpp's (k_factor_diag / _panel / _trail<NeesArgs>), on the padded layout of Sigma (eqf_device.hpp), in
// place in the scratch image NeesArgs::A (eqf_filter::dSigmaLoc: k_sigma_local's output, or a device copy of Sigma).  The submatrix starts
// at internal index `off` (0, 6 or kLm0 for the reference indices 0, 6, 11) and has order m_b = kLm0 + 3 N_b - off, each filter its own.
// The structural pad index 11 is read as a row of the identity whatever the image holds there: it cannot break a pivot, adds log 1 = 0
// and is skipped by min_pivot.  The error vectors are the factorisation's right-hand side, nrhs <= 16 rows under the matrix
// (e^T L^-T = z^T).  What is specific to this route lives here: the arguments, the view of a filter that the factorisation works on
// (factorView) and k_nees_tail, one workgroup per filter, for the reductions and the info word.  The sums of the tail run in one fixed
// order (as k_innov_stats does): the results are bit for bit the same from run to run and for a filter alone or anywhere in a batch.
// Nothing is written outside rows / columns [off, off + m_b) of a filter's image.
#pragma once
#include "eqf_device.hpp"
#include "eqf_factor.hpp"
#include "eqf_local.hpp"

namespace eqf {

constexpr int kNeesRhs = 16;   // error vectors per call (one MFMA tile of rows)
constexpr int kNeesHead = 4;   // per filter [kNeesHead + kNeesRhs]: logdet, min_pivot, dof, info; then nees[kNeesRhs]

struct NeesArgs {
    const Glob* g;
    double* A;          // [B] images, padded layout of Sigma
    int ld;
    long long strideA;
    double* E;          // [B][nrhs][ldE]: row k = error vector k, column i = entry off + i; -> z
    int ldE;
    double* D;          // [B][kDRec]: the record of the current diagonal block
    int* bad;           // [B]: a stage of factor64 met a pivot that was not positive
    const double* jac;  // k_local_jacobian's records (local = 1), else nullptr
    int cap;
    int off, nrhs;
    double* out;        // [B][kNeesHead + kNeesRhs]
};

EQF_DI int neesOrder(const NeesArgs& a, int b) { return kLm0 + 3 * a.g[b].N - a.off; }
EQF_DI FactorView factorView(const NeesArgs& a, int b) {
    return FactorView{a.A + (long long)b * a.strideA + (long long)a.off * a.ld + a.off, a.ld, neesOrder(a, b), kBase - a.off,
        a.D + (long long)b * kDRec, a.bad + b, a.E + (long long)b * a.nrhs * a.ldE, a.ldE, a.nrhs};
}

// grid = B, block = 256: thread t takes the terms t, t + 256, ... in sequence, then a fixed tree over the 256 partial sums (logdet,
// min_pivot); error vector k = t >> 4 is summed by its sixteen threads the same way
__global__ __launch_bounds__(256) void k_nees_tail(NeesArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int m = neesOrder(a, b), pad = kBase - a.off;
    const double* A = a.A + (long long)b * a.strideA + (long long)a.off * a.ld + a.off;
    const double* E = a.E + (long long)b * a.nrhs * a.ldE;
    double* out = a.out + (long long)b * (kNeesHead + kNeesRhs);
    double sl = 0.0, mn = __builtin_inf();
    int neg = 0;
    for (int k = tid; k < m; k += 256) {
        if (k == pad) continue;
        const double l = A[(long long)k * a.ld + k];
        if (!(l > 0.0) || !(l < __builtin_inf())) neg = 1;
        sl += log(l);
        mn = fmin(mn, l * l);
    }
    double sz = 0.0;
    {
        const int k = tid >> 4;
        if (k < a.nrhs)
            for (int i = tid & 15; i < m; i += 16) {
                const double z = E[(long long)k * a.ldE + i];
                sz = fma(z, z, sz);
            }
    }
    __shared__ double sA[256], sB[256], sZ[256];
    __shared__ int sNeg;
    if (tid == 0) sNeg = 0;
    sA[tid] = sl;
    sB[tid] = mn;
    sZ[tid] = sz;
    __syncthreads();
    if (neg) sNeg = 1;  // (every writer stores the same value)
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            sA[tid] += sA[tid + w];
            sB[tid] = fmin(sB[tid], sB[tid + w]);
        }
        if (w < 16 && (tid & 15) < w) sZ[tid] += sZ[tid + w];
        __syncthreads();
    }
    const double nan = __builtin_nan("");
    const int info = (a.jac && a.jac[b * jacStride(a.cap) + 13] != 0.0) ? -1 : ((sNeg || a.bad[b]) ? 1 : 0);
    if (tid == 0) {
        out[0] = info ? nan : 2.0 * sA[0];
        out[1] = info ? nan : sB[0];
        out[2] = (double)(m - (pad >= 0 ? 1 : 0));
        out[3] = (double)info;
    }
    if (tid < kNeesRhs) out[kNeesHead + tid] = tid < a.nrhs ? (info ? nan : sZ[16 * tid]) : 0.0;
}

}  // namespace eqf
