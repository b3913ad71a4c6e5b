// A measurement update with m <= 16 caller-supplied linear rows, for every filter of a handle (eqf_update_linear):
//   B = Sigma Ht^T,  S = Ht B + R = L L^T,  Y = L^-1 B^T,  z = L^-1 resid,  gamma = Y^T z,  Sigma <- Sigma - Y^T Y,
// then the group step of eqf_sample.hpp's k_apply_increment with gamma.  Ht = H (local = 0: rows in the origin chart, eqf_get_sigma's
// coordinates) or H J (local = 1: rows in the estimate's chart, eqf_get_sigma_local's; J block diagonal, eqf_local.hpp).  Everything is
// fp64 in the padded index map of eqf_device.hpp; the m rows are padded to 16 (one MFMA tile): rows m.. of Ht are zero and S carries the
// identity there, so Y's rows m.. are exactly zero and take no part in anything.
//
//   k_lin_rows      one workgroup per filter: H (reference map) -> Ht (padded map, column 11 zero), times J's blocks from the right
//                   when local; the verdict word starts here: 3 masked out, -1 local and the gravity chart singular, else 0.
//   k_lin_gain      Bt = (Sigma Ht^T)^T, 16 x n.  One workgroup per 64 rows of Sigma, which it streams once, by rows as stored, in 64-wide
//                   chunks through LDS; wave w owns rows 16 w .. 16 w + 15 of the tile and accumulates their 16 x 16 block of B on
//                   v_mfma_f64_16x16x4_f64 (mmTile), chunks and k-steps ascending.
//   k_lin_solve     one workgroup per filter: S's lower triangle (thread (k, l) sums over the columns ascending, one fused multiply-add
//                   each), the 16 x 16 Cholesky with divisions (no inverses), z by forward substitution, then one thread per column of
//                   Y: forward substitution in registers and gamma_i = sum_k Y_ki z_k, k ascending.  nis, log det, the log-likelihood
//                   and the verdict: 1 if a pivot is not positive or anything met is not finite, 2 if nis > gate.
//   k_lin_downdate  Sigma[I, J] -= Y_I^T Y_J over the lower triangle of 64 x 64 tiles, in place, K = 16 (four MFMA k-steps from a zero
//                   accumulator, then one subtraction); the mirror tile is written from the same registers, and of a diagonal tile only the
//                   entries row >= column are computed values (the others are their mirrors): Sigma stays bit-for-bit symmetric.  Leaves
//                   at once when the verdict is not 0.
// Row and column 11 of Sigma are zero and Ht's column 11 is zero, so Bt's, Y's and gamma's entry 11 are exact zeros and the pad stays zero.
// Nothing is shared between filters and every sum runs in one fixed order: bit for bit the same from run to run and for a filter alone
// or anywhere in a batch.  No atomics.
#pragma once
#include "eqf_chol64.hpp"
#include "eqf_device.hpp"
#include "eqf_local.hpp"
#include "eqf_math.hpp"
#include "eqf_nees.hpp"

namespace eqf {

constexpr int kLinRows = 16;
constexpr int kLinHead = kNeesHead + kNeesRhs;  // the result record: nis, logdet_S, loglik, info (where k_apply_increment looks for it), ..
constexpr int kLinYP = kLinRows + 1;            // LDS pitch of a transposed 64 x 16 block of Y
constexpr int kLinGainLdsBytes = int(sizeof(double)) * (kSB + kLinRows) * kSP;  // Sigma chunk | Ht chunk   (41 KB)

struct LinArgs {
    const Glob* g;
    double* Sigma;  // the current ping-pong buffer, downdated in place
    int ld;
    long long sigmaStride;
    const double* H;      // [B][16][ldr], reference index map
    int ldr;
    const double* resid;  // [B][16]
    const double* R;      // [B][16][16], lower triangle; rows m.. of the identity
    const unsigned char* mask;  // [B]
    const double* jac;    // k_local_jacobian's records, or nullptr (local = 0)
    int cap, m;
    double gate;
    double* ws;           // [B][wsStride]: Ht [16][ld] | Bt [16][ld] | Y [16][ld] | gamma [ld]
    long long wsStride;
    double* out;          // [B][kLinHead]
};

EQF_DI double* linHt(const LinArgs& a, int b) { return a.ws + b * a.wsStride; }
EQF_DI double* linBt(const LinArgs& a, int b) { return a.ws + b * a.wsStride + (long long)kLinRows * a.ld; }
EQF_DI double* linY(const LinArgs& a, int b) { return a.ws + b * a.wsStride + 2LL * kLinRows * a.ld; }
EQF_DI double* linGamma(const LinArgs& a, int b) { return a.ws + b * a.wsStride + 3LL * kLinRows * a.ld; }

// One row's base block: h (reference map, 11 entries) -> o (padded map, 12 entries, the pad 0), times J's base blocks (G at jac, R_A^T at
// jac + 4) from the right when jac is given.  Shared with eqf_split.hpp's k_split_row.
EQF_DI void linRowBase(const double* h, const double* jac, double* o) {
#pragma unroll
    for (int c = 0; c < 6; ++c) o[c] = h[c];
    if (jac) {
        const double* G = jac;
        const double* RAt = jac + 4;
        o[6] = fma(h[7], G[2], h[6] * G[0]);
        o[7] = fma(h[7], G[3], h[6] * G[1]);
#pragma unroll
        for (int c = 0; c < 3; ++c) o[8 + c] = dot3(h[8], RAt[c], h[9], RAt[3 + c], h[10], RAt[6 + c]);
    } else {
#pragma unroll
        for (int c = 6; c < kBase; ++c) o[c] = h[c];
    }
    o[kBase] = 0.0;
}
// ... and landmark i's block: hh = h + kBase + 3 i -> oo = o + kLm0 + 3 i, times J_i (jac + kJacHead + 9 i) when jac is given
EQF_DI void linRowLandmark(const double* hh, const double* jac, int i, double* oo) {
    if (jac) {
        const double* J = jac + kJacHead + 9LL * i;
#pragma unroll
        for (int c = 0; c < 3; ++c) oo[c] = dot3(hh[0], J[c], hh[1], J[3 + c], hh[2], J[6 + c]);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) oo[c] = hh[c];
    }
}

// grid = B, block = 256
__global__ __launch_bounds__(256) void k_lin_rows(LinArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int N = a.g[b].N, ld = a.ld;
    const double* H = a.H + (long long)b * kLinRows * a.ldr;
    double* Ht = linHt(a, b);
    const double* jac = a.jac ? a.jac + b * jacStride(a.cap) : nullptr;
    if (tid == 0) {
        double info = 0.0;
        if (!a.mask[b]) info = 3.0;
        else if (jac && jac[13] != 0.0) info = -1.0;
        double* out = a.out + (long long)b * kLinHead;
        out[0] = 0.0;
        out[1] = 0.0;
        out[2] = 0.0;
        out[3] = info;
    }
    // one item per (row k, block): block 0 the base, block 1 + i landmark i
    for (int e = tid; e < kLinRows * (N + 1); e += 256) {
        const int k = e & (kLinRows - 1), blk = e >> 4;
        const double* h = H + (long long)k * a.ldr;
        double* o = Ht + (long long)k * ld;
        if (blk == 0) {
            linRowBase(h, jac, o);
        } else {
            const int i = blk - 1;
            linRowLandmark(h + kBase + 3 * i, jac, i, o + kLm0 + 3 * i);
        }
    }
}

// grid = (64-row tiles of the largest filter, B), block = 256, LDS = kLinGainLdsBytes
__global__ __launch_bounds__(256) void k_lin_gain(LinArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smemLg[];
    double (*sS)[kSP] = reinterpret_cast<double (*)[kSP]>(smemLg);
    double (*sH)[kSP] = sS + kSB;
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = kLm0 + 3 * a.g[b].N, R0 = kSB * (int)blockIdx.x, ld = a.ld;
    if (R0 >= n) return;
    if (a.out[(long long)b * kLinHead + 3] != 0.0) return;
    const double* S = a.Sigma + (long long)b * a.sigmaStride;
    const double* Ht = linHt(a, b);
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int c0 = 0; c0 < n; c0 += kSB) {
        for (int e = tid; e < kSB * kSB; e += 256) {
            const int rr = e >> 6, cc = e & 63, gr = R0 + rr, gc = c0 + cc;
            sS[rr][cc] = (gr < n && gc < n) ? S[(long long)gr * ld + gc] : 0.0;
        }
        for (int e = tid; e < kLinRows * kSB; e += 256) {
            const int rr = e >> 6, cc = e & 63, gc = c0 + cc;
            sH[rr][cc] = gc < n ? Ht[(long long)rr * ld + gc] : 0.0;
        }
        __syncthreads();
        // rows R0 + 16 wv .. of Sigma (A operand) times Ht^T (B operand: element [k][col] = sH[col][k])
        acc = mmTile<true, kSB>(acc, &sS[0][0], kSP, kQB * wv, &sH[0][0], kSP, 0, lane, 1.0);
        __syncthreads();
    }
    double* Bt = linBt(a, b);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int gr = R0 + kQB * wv + (lane >> 4) + 4 * q, k = lane & 15;
        if (gr < n) Bt[(long long)k * ld + gr] = acc[q];
    }
}

// grid = B, block = 256
__global__ __launch_bounds__(256) void k_lin_solve(LinArgs a) {
    __shared__ double sHc[kLinRows][kSP];
    __shared__ double sBc[kLinRows][kSP];
    __shared__ double sL[kLinRows][kLinRows + 1];
    __shared__ double sZ[kLinRows];
    __shared__ int sBad;
    const int b = blockIdx.x, tid = threadIdx.x;
    double* out = a.out + (long long)b * kLinHead;
    if (out[3] != 0.0) return;
    const int n = kLm0 + 3 * a.g[b].N, ld = a.ld, m = a.m;
    const double* Ht = linHt(a, b);
    const double* Bt = linBt(a, b);
    double* Y = linY(a, b);
    double* gam = linGamma(a, b);
    const int k = tid >> 4, l = tid & 15;
    if (tid == 0) sBad = 0;
    // S_kl = R_kl + sum_j Ht_kj Bt_lj, j ascending (lower triangle; the identity pads rows m..)
    double s = a.R[((long long)b * kLinRows + k) * kLinRows + l];
    for (int c0 = 0; c0 < n; c0 += kSB) {
        for (int e = tid; e < kLinRows * kSB; e += 256) {
            const int rr = e >> 6, cc = e & 63, gc = c0 + cc;
            sHc[rr][cc] = gc < n ? Ht[(long long)rr * ld + gc] : 0.0;
            sBc[rr][cc] = gc < n ? Bt[(long long)rr * ld + gc] : 0.0;
        }
        __syncthreads();
        if (l <= k) {
#pragma unroll 8
            for (int j = 0; j < kSB; ++j) s = fma(sHc[k][j], sBc[l][j], s);
        }
        __syncthreads();
    }
    sL[k][l] = l <= k ? s : 0.0;
    __syncthreads();
    // right-looking Cholesky, column by column
    for (int j = 0; j < kLinRows; ++j) {
        if (tid == 0) {
            const double d = sL[j][j];
            if (!(d > 0.0) || !(d < __builtin_inf())) sBad = 1;
            sL[j][j] = sqrt(d);
        }
        __syncthreads();
        if (l == j && k > j) sL[k][j] = sL[k][j] / sL[j][j];
        __syncthreads();
        if (l > j && l <= k) sL[k][l] = fma(-sL[k][j], sL[l][j], sL[k][l]);
        __syncthreads();
    }
    if (tid == 0) {
        double nis = 0.0, lsum = 0.0;
        for (int r = 0; r < kLinRows; ++r) {
            double v = a.resid[(long long)b * kLinRows + r];
            for (int c = 0; c < r; ++c) v = fma(-sL[r][c], sZ[c], v);
            v = v / sL[r][r];
            sZ[r] = v;
            if (r < m) {
                nis = fma(v, v, nis);
                lsum += log(sL[r][r]);
            }
        }
        const double logdet = 2.0 * lsum;
        out[0] = nis;
        out[1] = logdet;
        out[2] = -0.5 * (nis + logdet + m * 1.8378770664093453);  // log(2 pi)
        if (!(fabs(nis) < __builtin_inf()) || !(fabs(logdet) < __builtin_inf())) sBad = 1;
    }
    __syncthreads();
    // one thread per column of Y
    int nf = 0;
    for (int i = tid; i < n; i += 256) {
        // (L is read from LDS again for every column: hoisted out of this loop its 136 entries would hold 272 registers for the whole kernel)
        __asm__ volatile("" ::: "memory");
        double y[kLinRows];
        double gsum = 0.0;
#pragma unroll
        for (int r = 0; r < kLinRows; ++r) {
            double v = Bt[(long long)r * ld + i];
#pragma unroll
            for (int c = 0; c < r; ++c) v = fma(-sL[r][c], y[c], v);
            v = v / sL[r][r];
            y[r] = v;
            gsum = fma(v, sZ[r], gsum);
            Y[(long long)r * ld + i] = v;
            if (!(fabs(v) < __builtin_inf())) nf = 1;
        }
        gam[i] = gsum;
        if (!(fabs(gsum) < __builtin_inf())) nf = 1;
    }
    nf = __syncthreads_or(nf);
    if (tid == 0) {
        double info = 0.0;
        if (sBad || nf) info = 1.0;
        else if (out[0] > a.gate) info = 2.0;
        out[3] = info;
    }
}

// grid = (tiles of the lower triangle of the largest filter, B), block = 256.  Tile t = I (I + 1) / 2 + J, J <= I.
__global__ __launch_bounds__(256) void k_lin_downdate(LinArgs a) {
    __shared__ double sA[kSB][kLinYP];  // Y_I^T: [row of the tile][k]
    __shared__ double sB[kSB][kLinYP];  // Y_J^T
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (a.out[(long long)b * kLinHead + 3] != 0.0) return;
    const int n = kLm0 + 3 * a.g[b].N, ld = a.ld;
    int I = 0;
    while ((I + 1) * (I + 2) / 2 <= (int)blockIdx.x) ++I;
    const int J = (int)blockIdx.x - I * (I + 1) / 2;
    const int I0 = kSB * I, J0 = kSB * J;
    if (I0 >= n) return;
    double* S = a.Sigma + (long long)b * a.sigmaStride;
    const double* Y = linY(a, b);
    for (int e = tid; e < kLinRows * kSB; e += 256) {
        const int kk = e >> 6, cc = e & 63;
        sA[cc][kk] = I0 + cc < n ? Y[(long long)kk * ld + I0 + cc] : 0.0;
        sB[cc][kk] = J0 + cc < n ? Y[(long long)kk * ld + J0 + cc] : 0.0;
    }
    __syncthreads();
    const bool diag = I == J;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (diag && i > wv) continue;  // (sub-tiles above the diagonal: written as mirrors)
        // the product from a zero accumulator, then ONE subtraction: every entry of Sigma is rounded once (started from Sigma_ij the sixteen
        // additions would each round at the size of Sigma_ij)
        f64x4 acc = {0.0, 0.0, 0.0, 0.0};
        double sig[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int gr = I0 + kQB * wv + (lane >> 4) + 4 * q, gc = J0 + kQB * i + (lane & 15);
            sig[q] = (gr < n && gc < n) ? S[(long long)gr * ld + gc] : 0.0;
        }
        acc = mmTile<true, kLinRows>(acc, &sA[0][0], kLinYP, kQB * wv, &sB[0][0], kLinYP, kQB * i, lane, 1.0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int gr = I0 + kQB * wv + (lane >> 4) + 4 * q, gc = J0 + kQB * i + (lane & 15);
            if (gr < n && gc < n && (!diag || gc <= gr)) {
                const double v = sig[q] - acc[q];
                S[(long long)gr * ld + gc] = v;
                if (gc != gr) S[(long long)gc * ld + gr] = v;
            }
        }
    }
}

}  // namespace eqf
