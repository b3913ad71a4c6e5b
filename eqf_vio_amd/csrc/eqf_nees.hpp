// Joint NEES and log-determinant of the covariance on the device (eqf_get_nees).
//
// For every filter of a handle: A = L L^T of a trailing principal submatrix of Sigma (local = 0) or Sigma_loc (local = 1), with the forward
// solve z = L^-1 e of up to kNeesRhs error vectors carried along:
//   nees_k    = e_k^T A^-1 e_k = z_k^T z_k
//   logdet    = 2 sum log L_ii          min_pivot = min L_ii^2
// A batched, blocked, right-looking Cholesky in 64-wide block columns on the padded layout of Sigma (eqf_device.hpp), in place in the
// scratch image NeesArgs::A (eqf_filter::dSigmaLoc: k_sigma_local's output, or a device copy of Sigma).  The submatrix starts at internal
// index `off` (0, 6 or kLm0 for the reference indices 0, 6, 11) and has order m_b = kLm0 + 3 N_b - off, each filter its own.  The
// structural pad index 11 is read as a row of the identity whatever the image holds there: it cannot break a pivot, adds log 1 = 0 and is
// skipped by min_pivot.  Per block column K three launches, the filters of the batch in grid.y (workgroups beyond a filter's own extent
// leave at once):
//   k_nees_diag    block (K, K) -> LDS (identity past m_b, lower triangle only), factor64, L_KK back, the record (L_KK, W_jj) to NeesArgs::D
//   k_nees_panel   L_RK = A_RK L_KK^-T for the block rows R > K, one workgroup per block (solveStrip<true>); the error vectors are sixteen
//                  more rows under the matrix (e^T L^-T = z^T): the last workgroup solves Z_K = E_K L_KK^-T
//   k_nees_trail   A_RC -= L_RK L_CK^T over the lower triangle R >= C > K, one workgroup per 64 x 64 tile on v_mfma_f64_16x16x4_f64 (mmTile);
//                  E_C -= Z_K L_CK^T by one more workgroup per block column C
// and k_nees_tail, one workgroup per filter, for the reductions and the info word.  Every element sees the same operations in the same
// order whatever the batch around its filter is, and the sums of the tail run in one fixed order (as k_innov_stats does): the results are
// bit for bit the same from run to run and for a filter alone or anywhere in a batch.  Nothing is written outside rows / columns
// [off, off + m_b) of a filter's image.
#pragma once
#include "eqf_chol64.hpp"
#include "eqf_device.hpp"
#include "eqf_local.hpp"

namespace eqf {

constexpr int kNeesRhs = 16;   // error vectors per call (one MFMA tile of rows)
constexpr int kNeesHead = 4;   // per filter [kNeesHead + kNeesRhs]: logdet, min_pivot, dof, info; then nees[kNeesRhs]
constexpr int kNeesPanelLdsBytes = int(sizeof(double)) * (2 * kSB * kSP + 4 * kQB * kWP);  // P | L | Wd  (75 KB: two workgroups per CU)
constexpr int kNeesTrailLdsBytes = int(sizeof(double)) * 2 * kSB * kSP;                     // P | Q       (65 KB)

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
EQF_DI Lds64 ldsNeesPanel(unsigned char* smem) {
    double* d = reinterpret_cast<double*>(smem);
    double (*P)[kSP] = reinterpret_cast<double (*)[kSP]>(d);
    double (*L)[kSP] = reinterpret_cast<double (*)[kSP]>(d + kSB * kSP);
    double (*Wd)[kQB][kWP] = reinterpret_cast<double (*)[kQB][kWP]>(d + 2 * kSB * kSP);
    return Lds64{P, nullptr, L, Wd, nullptr, nullptr, nullptr, nullptr};
}

// grid = (1, B), block = 256, LDS = kLdsFactorBytes
__global__ __launch_bounds__(256) void k_nees_diag(NeesArgs a, int K) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smemN[];
    const Lds64 s = ldsFactor(smemN);
    const int b = blockIdx.y, tid = threadIdx.x;
    const int m = neesOrder(a, b), c0 = kSB * K;
    if (K == 0 && tid == 0) a.bad[b] = 0;
    if (c0 >= m) return;
    double* A = a.A + (long long)b * a.strideA + (long long)a.off * a.ld + a.off;
    const int pad = kBase - a.off;  // index of the structural pad row in the submatrix (negative: not part of it)
    for (int e = tid; e < kSB * kSB; e += 256) {
        const int r = e >> 6, c = e & 63, gr = c0 + r, gc = c0 + c;
        double v = r == c ? 1.0 : 0.0;
        if (gr < m && gr != pad && gc != pad && c <= r) v = A[(long long)gr * a.ld + gc];
        s.L[r][c] = v;
    }
    __syncthreads();
    factorPrologue(s, tid);
    __syncthreads();
    int bad = 0;
    factor64(s, tid, &bad, a.D + (long long)b * kDRec, nullptr, realStages(m, c0));
    __syncthreads();
    for (int e = tid; e < kSB * kSB; e += 256) {
        const int r = e >> 6, c = e & 63, gr = c0 + r, gc = c0 + c;
        if (gr < m && c <= r) A[(long long)gr * a.ld + gc] = s.L[r][c];
    }
    if (bad && tid == 0) a.bad[b] = 1;
}

// grid = (nbMax - K - 1 + (nrhs > 0), B), block = 256, LDS = kNeesPanelLdsBytes
__global__ __launch_bounds__(256) void k_nees_panel(NeesArgs a, int K, int rem) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smemN[];
    const Lds64 s = ldsNeesPanel(smemN);
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int m = neesOrder(a, b), c0 = kSB * K;
    const bool rhs = (int)blockIdx.x == rem;
    const int r0 = kSB * (K + 1 + (int)blockIdx.x);
    if (c0 >= m || (!rhs && r0 >= m)) return;
    const int pad = kBase - a.off;
    // rows of this workgroup: 64 rows of the matrix from r0, or the kNeesRhs rows of E
    double* M = rhs ? a.E + (long long)b * a.nrhs * a.ldE : a.A + (long long)b * a.strideA + (long long)(a.off + r0) * a.ld + a.off;
    const int ldM = rhs ? a.ldE : a.ld, rows = rhs ? a.nrhs : min(kSB, m - r0);
    const double* Dk = a.D + (long long)b * kDRec;
    for (int e = tid; e < kSB * kSB; e += 256) {
        const int r = e >> 6, c = e & 63, gc = c0 + c;
        s.P[r][c] = (r < rows && gc < m && gc != pad) ? M[(long long)r * ldM + gc] : 0.0;
        s.L[r][c] = Dk[e];
    }
    for (int e = tid; e < 4 * kQB * kQB; e += 256) s.Wd[e >> 8][(e >> 4) & 15][e & 15] = Dk[kSB * kSB + e];
    __syncthreads();
    if (kQB * wv < rows) solveStrip<true>(&s.P[0][0], kSP, s, kQB * wv, lane);
    __syncthreads();
    for (int e = tid; e < kSB * kSB; e += 256) {
        const int r = e >> 6, c = e & 63, gc = c0 + c;
        if (r < rows && gc < m) M[(long long)r * ldM + gc] = s.P[r][c];
    }
}

// grid = (t (t + 1) / 2 + (nrhs > 0 ? t : 0), B) with t = nbMax - K - 1, block = 256, LDS = kNeesTrailLdsBytes
__global__ __launch_bounds__(256) void k_nees_trail(NeesArgs a, int K, int t) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smemN[];
    double (*sP)[kSP] = reinterpret_cast<double (*)[kSP]>(smemN);
    double (*sQ)[kSP] = sP + kSB;
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int m = neesOrder(a, b), c0 = kSB * K, nA = t * (t + 1) / 2;
    // tile (r, c), r >= c, of the trailing lower triangle, row-major enumeration; behind them the tiles of E, one per block column
    const bool rhs = (int)blockIdx.x >= nA;
    int r = 0, idx = rhs ? (int)blockIdx.x - nA : (int)blockIdx.x;
    if (!rhs)
        while (idx >= r + 1) {
            idx -= r + 1;
            ++r;
        }
    const int R0 = kSB * (K + 1 + r), C0 = kSB * (K + 1 + idx);
    if (C0 >= m || (!rhs && R0 >= m)) return;
    double* A = a.A + (long long)b * a.strideA + (long long)a.off * a.ld + a.off;
    double* M = rhs ? a.E + (long long)b * a.nrhs * a.ldE : A + (long long)R0 * a.ld;
    const int ldM = rhs ? a.ldE : a.ld, rows = rhs ? a.nrhs : min(kSB, m - R0);
    for (int e = tid; e < kSB * kSB; e += 256) {
        const int rr = e >> 6, cc = e & 63, gc = c0 + cc, gq = C0 + rr;  // (gc < m: block column K is a full one, a block row lies below it)
        sP[rr][cc] = rr < rows ? M[(long long)rr * ldM + gc] : 0.0;
        sQ[rr][cc] = gq < m ? A[(long long)gq * a.ld + gc] : 0.0;
    }
    __syncthreads();
    if (rhs) {
        // 16 x 64: wave wv owns the 16 columns C0 + 16 wv ..
        f64x4 acc;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int rr = (lane >> 4) + 4 * q, gc = C0 + kQB * wv + (lane & 15);
            acc[q] = (rr < rows && gc < m) ? M[(long long)rr * ldM + gc] : 0.0;
        }
        acc = mmTile<true, kSB>(acc, &sP[0][0], kSP, 0, &sQ[0][0], kSP, kQB * wv, lane, -1.0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int rr = (lane >> 4) + 4 * q, gc = C0 + kQB * wv + (lane & 15);
            if (rr < rows && gc < m) M[(long long)rr * ldM + gc] = acc[q];
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f64x4 acc;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int rr = kQB * wv + (lane >> 4) + 4 * q, gc = C0 + kQB * i + (lane & 15);
            acc[q] = (rr < rows && gc < m) ? M[(long long)rr * ldM + gc] : 0.0;
        }
        acc = mmTile<true, kSB>(acc, &sP[0][0], kSP, kQB * wv, &sQ[0][0], kSP, kQB * i, lane, -1.0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int rr = kQB * wv + (lane >> 4) + 4 * q, gc = C0 + kQB * i + (lane & 15);
            if (rr < rows && gc < m && gc <= R0 + rr) M[(long long)rr * ldM + gc] = acc[q];  // (lower triangle only)
        }
    }
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
