// The batched, blocked Cholesky factorisation that eqf_get_nees, the covariance draws, eqf_get_merge_costs (NeesArgs, eqf_nees.hpp) and
// eqf_update_landmarks (BlkArgs, eqf_blocks.hpp) share: ONE set of three kernels, templated on the argument struct of the route.
//
// A = L L^T of one symmetric matrix per image, right-looking in 64-wide block columns, in place, the lower triangle only; a right-hand side
// of any number of rows is carried under the matrix (rows^T L^-T: what the forward solve L^-1 rows gives, transposed), in 64-row block
// rows of its own.  The images of a call sit in grid.y, each with its own order; what lies past an image's order is the identity, supplied
// when a block is loaded and never stored.  Per block column K three launches (eqf_capi.hip's enqueueFactor; workgroups beyond an image's
// own extent leave at once):
//   k_factor_diag    block (K, K) -> LDS (identity past the order, lower triangle only), factorPrologue + factor64 with
//                    realStages(m, 64 K), L_KK back, the record (L_KK, W_jj) to FactorView::D.  K = 0 also clears the bad-pivot word.
//   k_factor_panel   M_RK <- M_RK L_KK^-T, one workgroup per block row below K -- the t = nb - K - 1 of the matrix, then those of the
//                    right-hand side -- a wave per 16-row strip (solveStrip<true>)
//   k_factor_trail   M_RC -= M_RK L_CK^T on v_mfma_f64_16x16x4_f64 (mmTile), one workgroup per 64 x 64 tile: the t (t + 1) / 2 tiles
//                    R >= C > K of the matrix' lower triangle, row-major, then t tiles per block row of the right-hand side.  A block row
//                    of at most 16 rows (a short last one; the error vectors of eqf_get_nees) is split over the four waves by columns
//                    instead of by rows: the same mmTile steps on the same operand rows for every output element, so not a bit depends on
//                    which way a tile went.
// What the kernels know about image b of a route is its FactorView, built by the route's factorView(args, b).  Every element sees the
// same operations in the same order whatever the batch around its image is: bit for bit the same from run to run and for an image alone
// or anywhere in a batch.  Nothing is written outside an image's own extent.
#pragma once
#include "eqf_chol64.hpp"
#include "eqf_device.hpp"

namespace eqf {

constexpr int kFactorPanelLdsBytes = int(sizeof(double)) * (2 * kSB * kSP + 4 * kQB * kWP);  // P | L | Wd  (75 KB: two workgroups per CU)
constexpr int kFactorTrailLdsBytes = int(sizeof(double)) * 2 * kSB * kSP;                     // P | Q       (65 KB)

struct FactorView {
    double* A;    // the matrix, entry (0, 0) of what is factored
    int ld;
    int m;        // its order; 0: this image takes no part
    int pad;      // index of a structural pad row / column, read as a row of the identity whatever the image holds there (negative: none)
    double* D;    // [kDRec]: the record of the current diagonal block
    int* bad;     // a stage of factor64 met a pivot that was not positive
    double* rhs;  // [nrhs][ldRhs]: the right-hand side's rows, as wide as the matrix
    int ldRhs, nrhs;
};

EQF_DI Lds64 ldsFactorPanel(unsigned char* smem) {
    double* d = reinterpret_cast<double*>(smem);
    double (*P)[kSP] = reinterpret_cast<double (*)[kSP]>(d);
    double (*L)[kSP] = reinterpret_cast<double (*)[kSP]>(d + kSB * kSP);
    double (*Wd)[kQB][kWP] = reinterpret_cast<double (*)[kQB][kWP]>(d + 2 * kSB * kSP);
    return Lds64{P, nullptr, L, Wd, nullptr, nullptr, nullptr, nullptr};
}

// grid = (1, B), block = 256, LDS = kLdsFactorBytes
template <class Args>
__global__ __launch_bounds__(256) void k_factor_diag(Args a, int K) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smemF[];
    const Lds64 s = ldsFactor(smemF);
    const int b = blockIdx.y, tid = threadIdx.x;
    const FactorView v = factorView(a, b);
    const int m = v.m, c0 = kSB * K;
    if (K == 0 && tid == 0) *v.bad = 0;
    if (c0 >= m) return;
    for (int e = tid; e < kSB * kSB; e += 256) {
        const int r = e >> 6, c = e & 63, gr = c0 + r, gc = c0 + c;
        double x = r == c ? 1.0 : 0.0;
        if (gr < m && gr != v.pad && gc != v.pad && c <= r) x = v.A[(long long)gr * v.ld + gc];
        s.L[r][c] = x;
    }
    __syncthreads();
    factorPrologue(s, tid);
    __syncthreads();
    int bad = 0;
    factor64(s, tid, &bad, v.D, nullptr, realStages(m, c0));
    __syncthreads();
    for (int e = tid; e < kSB * kSB; e += 256) {
        const int r = e >> 6, c = e & 63, gr = c0 + r, gc = c0 + c;
        if (gr < m && c <= r) v.A[(long long)gr * v.ld + gc] = s.L[r][c];
    }
    if (bad && tid == 0) *v.bad = 1;
}

// grid = (t + block rows of the right-hand side, B) with t = nb - K - 1, block = 256, LDS = kFactorPanelLdsBytes
template <class Args>
__global__ __launch_bounds__(256) void k_factor_panel(Args a, int K, int t) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smemF[];
    const Lds64 s = ldsFactorPanel(smemF);
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const FactorView v = factorView(a, b);
    const int m = v.m, c0 = kSB * K;
    if (c0 >= m) return;
    // rows of this workgroup: 64 rows of the matrix from block row K + 1 + x, or 64 rows of the right-hand side from its block row x - t
    const bool rhs = (int)blockIdx.x >= t;
    const int r0 = kSB * (rhs ? (int)blockIdx.x - t : K + 1 + (int)blockIdx.x);
    const int rows = min(kSB, (rhs ? v.nrhs : m) - r0), ldM = rhs ? v.ldRhs : v.ld;
    if (rows <= 0) return;
    double* M = (rhs ? v.rhs : v.A) + (long long)r0 * ldM;
    for (int e = tid; e < kSB * kSB; e += 256) {
        const int r = e >> 6, c = e & 63, gc = c0 + c;
        s.P[r][c] = (r < rows && gc < m && gc != v.pad) ? M[(long long)r * ldM + gc] : 0.0;
        s.L[r][c] = v.D[e];
    }
    for (int e = tid; e < 4 * kQB * kQB; e += 256) s.Wd[e >> 8][(e >> 4) & 15][e & 15] = v.D[kSB * kSB + e];
    __syncthreads();
    if (kQB * wv < rows) solveStrip<true>(&s.P[0][0], kSP, s, kQB * wv, lane);
    __syncthreads();
    for (int e = tid; e < kSB * kSB; e += 256) {
        const int r = e >> 6, c = e & 63, gc = c0 + c;
        if (r < rows && gc < m) M[(long long)r * ldM + gc] = s.P[r][c];
    }
}

// grid = (t (t + 1) / 2 + t * block rows of the right-hand side, B) with t = nb - K - 1, block = 256, LDS = kFactorTrailLdsBytes
template <class Args>
__global__ __launch_bounds__(256) void k_factor_trail(Args a, int K, int t) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smemF[];
    double (*sP)[kSP] = reinterpret_cast<double (*)[kSP]>(smemF);
    double (*sQ)[kSP] = sP + kSB;
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const FactorView v = factorView(a, b);
    const int m = v.m, c0 = kSB * K, nA = t * (t + 1) / 2;
    // tile (r, c), r >= c, of the trailing lower triangle, row-major enumeration; behind them the tiles of the right-hand side, block row
    // by block row, one per block column
    const bool rhs = (int)blockIdx.x >= nA;
    int r = 0, idx = (int)blockIdx.x;
    if (rhs) {
        idx -= nA;
        r = idx / t;
        idx -= r * t;
    } else {
        while (idx >= r + 1) {
            idx -= r + 1;
            ++r;
        }
    }
    const int R0 = kSB * (rhs ? r : K + 1 + r), C0 = kSB * (K + 1 + idx);
    const int rows = min(kSB, (rhs ? v.nrhs : m) - R0), ldM = rhs ? v.ldRhs : v.ld;
    if (C0 >= m || rows <= 0) return;
    double* M = (rhs ? v.rhs : v.A) + (long long)R0 * ldM;
    for (int e = tid; e < kSB * kSB; e += 256) {
        const int rr = e >> 6, cc = e & 63, gc = c0 + cc, gq = C0 + rr;  // (gc < m: block column K is a full one, block column C lies behind it)
        sP[rr][cc] = rr < rows ? M[(long long)rr * ldM + gc] : 0.0;
        sQ[rr][cc] = gq < m ? v.A[(long long)gq * v.ld + gc] : 0.0;
    }
    __syncthreads();
    // of a tile of the matrix only the lower triangle is stored, gc <= R0 + rr; cLim = m lets every gc < m of a right-hand-side tile pass
    // the same comparison (one more condition on the loads, or a second form of the stores, costs the trailing update 3 % at 64 x 200)
    const int cLim = rhs ? m : R0;
    if (rows <= kQB) {
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
            if (rr < rows && gc < m && gc <= cLim + rr) M[(long long)rr * ldM + gc] = acc[q];
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
            if (rr < rows && gc < m && gc <= cLim + rr) M[(long long)rr * ldM + gc] = acc[q];
        }
    }
}

}  // namespace eqf
