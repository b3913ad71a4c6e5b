// A measurement update from per-landmark blocks, for every filter of a handle (eqf_update_landmarks): entry k of filter b measures landmark
// i_k alone, with `rows` (1, 2 or 3) rows H_k (rows x 3), a residual and a noise covariance R_k of its own -- the second camera of a stereo
// rig, a range, a surveyed position.  With Ht the block-sparse m x n matrix of the entries that take part, m = rows * (their number):
//   B = Sigma Ht^T,  S = Ht B + blockdiag(R_k) = L L^T,  Y = L^-1 B^T,  z = L^-1 resid,  gamma = Y^T z,  Sigma <- Sigma - Y^T Y,
// then the group step of eqf_sample.hpp's k_apply_increment with gamma.  Everything is fp64 in the padded index map of eqf_device.hpp, and
// Sigma is read by its LOWER triangle only.  The per-entry arithmetic is eqf_blocks_host.hpp's (host-compilable, tested on the CPU).
//
// An entry that does not take part -- its id is not in the state, or its own d2 = resid^T (Ht_k Sigma_ii Ht_k^T + R_k)^-1 resid exceeds
// lm_gate -- is a decoupled block (H = 0, resid = 0, R = I) in the statement of the update; here such a block is never formed: k_blk_rows
// packs the entries that take part to the front, S has the filter's own order m_b = rows * count_b, and what lies past m_b is the
// identity of eqf_factor.hpp's convention (supplied when a block is loaded, never stored).  The result is therefore the one of the call
// without that entry, bit for bit, and the launch shapes depend on stride, rows and the handle's capacity only.
//
// The work of a filter sits in one tall matrix M [mp + n + 1][mp], mp = rows * stride rounded up to 64: rows [0, mp) hold S, rows mp + i
// the row i of B (n x m, state index by measurement index), row mp + n the residual.  eqf_factor.hpp's blocked Cholesky
// (k_factor_diag / _panel / _trail<BlkArgs>) turns S into L and, as its right-hand side of n + 1 rows, B into B L^-T = Y^T and resid^T
// into z^T: no kernel of this file's own.  factorView is what it sees of a filter: M, order m_b (0 when the verdict word is not 0: such
// a filter takes no part), no pad index, the record BlkArgs::D, the pivot word, and the rows from mp on.
//
//   k_blk_rows      one workgroup per filter.  The verdict word starts here (3 masked out, -1 local and the gravity chart singular, 4 no
//                   entry takes part, else 0).  One thread per entry: Ht_k = H_k or H_k J_i, S_kk from Sigma_ii, d2_k, used[k]; then the
//                   compaction and the residual row.
//   k_blk_gain      B and S in one launch.  Workgroups [0, nIB): 64 rows of B each, thread (i, p) reads the three values Sigma(i, l_p ..)
//                   of its entry by the lower triangle (a row segment or a column segment of Sigma) and writes rows dot3's: n x 3 x rows
//                   multiply-adds per entry, no dense product.  The others: 16 x 16 pairs of entries each, thread (p, q <= p) forms
//                   Ht_p Sigma_{pq} Ht_q^T (+ R_p when p = q) from the 3 x 3 block of Sigma, the lower triangle of S only.
//   k_blk_gamma     gamma_i = sum_k Y_ki z_k, one thread per i (64 of them per workgroup), k ascending, one fused multiply-add each; a value
//                   of Y or gamma that is not finite raises the filter's non-finite word (every writer stores the same 1)
//   k_blk_tail      one workgroup per filter: nis = z^T z and log det S = 2 sum log L_kk (thread t the terms t, t + 256, .. in sequence,
//                   then a fixed tree), and the verdict: 1 if a pivot is not positive or anything met is not finite, 2 if nis > gate.
//   k_blk_downdate  Sigma[I, J] -= Y_I^T Y_J over the lower triangle of 64 x 64 tiles, in place: per 64 rows of Y the product from a zero
//                   accumulator, then one subtraction (one rounding per entry and 64 rows of Y, blocks ascending); the mirror tile is
//                   written from the same registers and of a diagonal tile only the entries row >= column are computed values: Sigma
//                   comes out bit-for-bit symmetric.  Leaves at once when the verdict is not 0.
// Row and column 11 of Sigma are zero, so B's row 11, Y's and gamma's entry 11 are exact zeros and the pad stays zero.  Nothing is shared
// between filters and every sum runs in one fixed order: bit for bit the same from run to run and for a filter alone or anywhere in a
// batch.  No atomics.  Launches per call: 2 + (3 nb - 1) + 4 (the factorisation's schedule: the last block column has no trailing
// tiles), nb = mp / 64.
#pragma once
#include "eqf_blocks_host.hpp"
#include "eqf_device.hpp"
#include "eqf_factor.hpp"
#include "eqf_linear.hpp"
#include "eqf_local.hpp"
#include "eqf_math.hpp"

namespace eqf {

constexpr int kBlkDownLdsBytes = int(sizeof(double)) * 2 * kSB * kSP;  // Y_I^T chunk | Y_J^T chunk   (65 KB)

struct BlkArgs {
    const Glob* g;
    double* Sigma;  // the current ping-pong buffer, downdated in place
    int ld;
    long long sigmaStride;
    const double* Hb;     // [B][stride][rows][3]
    const double* resid;  // [B][stride][rows]
    const double* Rb;     // [B][stride][rows][rows], lower triangles
    const int* idx;       // [B][stride]: landmark index of the entry's id, < 0 when it is not in the state
    const int* nk;        // [B]
    const unsigned char* mask;  // [B]
    const double* jac;    // k_local_jacobian's records, or nullptr (local = 0)
    int cap, rows, stride;
    int mp, nb;           // order of S padded to 64 (= M's leading dimension), its block columns (nb: the host's, no kernel reads it)
    double gate, lmGate;
    double* ws;           // [B][wsStride]: M | Ht [stride][9] | gamma [ld] | D [kDRec]   (blocks::WorkLayout)
    long long wsStride, offHt, offGamma, offD;
    int* wi;              // [B][wiStride]: used [stride] | pos [stride] | ent [stride] | count | bad pivot | non-finite
    int wiStride;
    double* out;          // [B][kLinHead]: nis, logdet_S, loglik, the verdict word
};

EQF_DI double* blkM(const BlkArgs& a, int b) { return a.ws + b * a.wsStride; }
EQF_DI double* blkHt(const BlkArgs& a, int b) { return a.ws + b * a.wsStride + a.offHt; }
EQF_DI double* blkGamma(const BlkArgs& a, int b) { return a.ws + b * a.wsStride + a.offGamma; }
EQF_DI double* blkD(const BlkArgs& a, int b) { return a.ws + b * a.wsStride + a.offD; }
EQF_DI int* blkUsed(const BlkArgs& a, int b) { return a.wi + (long long)b * a.wiStride; }
EQF_DI int* blkPos(const BlkArgs& a, int b) { return a.wi + (long long)b * a.wiStride + a.stride; }
EQF_DI int* blkEnt(const BlkArgs& a, int b) { return a.wi + (long long)b * a.wiStride + 2 * a.stride; }
EQF_DI int* blkCount(const BlkArgs& a, int b) { return a.wi + (long long)b * a.wiStride + 3 * a.stride; }
EQF_DI int blkOrder(const BlkArgs& a, int b) { return a.rows * *blkCount(a, b); }
EQF_DI FactorView factorView(const BlkArgs& a, int b) {
    double* M = blkM(a, b);
    const int m = a.out[(long long)b * kLinHead + 3] != 0.0 ? 0 : blkOrder(a, b);
    return FactorView{M, a.mp, m, -1, blkD(a, b), blkCount(a, b) + 1, M + (long long)a.mp * a.mp, a.mp, kLm0 + 3 * a.g[b].N + 1};
}
// Sigma(r, c) by the lower triangle
EQF_DI double blkSym(const double* S, int ld, int r, int c) { return r >= c ? S[(long long)r * ld + c] : S[(long long)c * ld + r]; }

// The three steps of a rows kernel (k_blk_rows here, k_obs_rows of eqf_observe.hpp), so that both leave the same workspace.
// Thread 0 opens the filter's record with the verdict word `info` and zeroes the words of the later kernels.
__device__ __forceinline__ void blkRowsOpen(const BlkArgs& a, int b, int info) {
    double* out = a.out + (long long)b * kLinHead;
    out[0] = 0.0;
    out[1] = 0.0;
    out[2] = 0.0;
    out[3] = (double)info;
    blkCount(a, b)[0] = 0;
    blkCount(a, b)[1] = 0;  // (the pivot word of k_factor_diag)
    blkCount(a, b)[2] = 0;  // (the non-finite word of k_blk_gamma)
}
// Entry k of filter b on landmark i (in the state) with rows H (times J unless it is nullptr) and residual resid: Ht into the workspace,
// S_kk from Sigma_ii, d2_k; returns the verdict.  S: the filter's Sigma.
__device__ __forceinline__ int blkRowsEntry(const BlkArgs& a, int b, int k, int i, const double* S, const double* H, const double* J,
    const double* R, const double* resid) {
    const int rows = a.rows;
    double Ht[9], Sii[9], Skk[9];
    blocks::formRows(rows, H, J, Ht);
    const int l = kLm0 + 3 * i;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) Sii[3 * r + c] = c <= r ? S[(long long)(l + r) * a.ld + l + c] : 0.0;
    blocks::entryS(rows, Ht, Sii, R, Skk);
    double* HtAll = blkHt(a, b);
    for (int q = 0; q < 9; ++q) HtAll[9LL * k + q] = q < 3 * rows ? Ht[q] : 0.0;
    return blocks::entryVerdict(i, blocks::entryD2(rows, Skk, resid), a.lmGate);
}
// Behind the entries (the whole workgroup, used[] written): the compaction, and the residual of the entries that take part as the last
// row of the tall matrix.  resid: [B][stride][rows].
__device__ __forceinline__ void blkRowsClose(const BlkArgs& a, int b, int nkb, int n, int info, const double* resid) {
    const int tid = threadIdx.x, rows = a.rows;
    __syncthreads();
    if (tid == 0) {
        const int cnt = blocks::compact(nkb, blkUsed(a, b), blkPos(a, b), blkEnt(a, b));
        blkCount(a, b)[0] = cnt;
        if (cnt == 0 && info == 0) a.out[(long long)b * kLinHead + 3] = (double)blocks::kInfoIdle;
    }
    __syncthreads();
    const int* pos = blkPos(a, b);
    double* Mz = blkM(a, b) + (long long)(a.mp + n) * a.mp;
    for (int k = tid; k < nkb; k += 256) {
        const int p = pos[k];
        if (p < 0) continue;
        const long long e = (long long)b * a.stride + k;
        for (int r = 0; r < rows; ++r) Mz[rows * p + r] = resid[e * rows + r];
    }
}

// grid = B, block = 256
__global__ __launch_bounds__(256) void k_blk_rows(BlkArgs a) {
    __shared__ int sInfo;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int N = a.g[b].N, n = kLm0 + 3 * N, rows = a.rows;
    const double* jac = a.jac ? a.jac + b * jacStride(a.cap) : nullptr;
    int* used = blkUsed(a, b);
    if (tid == 0) {
        int info = 0;
        if (!a.mask[b]) info = 3;
        else if (jac && jac[13] != 0.0) info = -1;
        blkRowsOpen(a, b, info);
        sInfo = info;
    }
    __syncthreads();
    if (sInfo == 3) return;  // (the operands of a filter that is masked out are never read)
    const int nkb = min(max(a.nk[b], 0), a.stride);
    const double* S = a.Sigma + (long long)b * a.sigmaStride;
    for (int k = tid; k < nkb; k += 256) {
        const long long e = (long long)b * a.stride + k;
        const int i = a.idx[e];
        int verdict = blocks::kAbsent;
        if (i >= 0 && i < N)
            verdict = blkRowsEntry(a, b, k, i, S, a.Hb + e * rows * 3, jac ? jac + kJacHead + 9LL * i : nullptr, a.Rb + e * rows * rows,
                a.resid + e * rows);
        used[k] = verdict;
    }
    blkRowsClose(a, b, nkb, n, sInfo, a.resid);
}

// grid = (nIB + nPT^2, B) with nIB = 64-row tiles of the largest filter, nPT = blocks::pairTiles(stride); block = 256
__global__ __launch_bounds__(256) void k_blk_gain(BlkArgs a, int nIB, int nPT) {
    const int b = blockIdx.y, tid = threadIdx.x;
    if (a.out[(long long)b * kLinHead + 3] != 0.0) return;
    const int n = kLm0 + 3 * a.g[b].N, rows = a.rows, cnt = *blkCount(a, b), ld = a.ld, mp = a.mp;
    const double* S = a.Sigma + (long long)b * a.sigmaStride;
    const double* HtAll = blkHt(a, b);
    const int* ent = blkEnt(a, b);
    const int* idx = a.idx + (long long)b * a.stride;
    double* M = blkM(a, b);
    if ((int)blockIdx.x < nIB) {
        const int i = kSB * (int)blockIdx.x + (tid & 63);
        if (i >= n) return;
        double* Brow = M + (long long)(mp + i) * mp;
        for (int p = tid >> 6; p < cnt; p += 4) {
            const int k = ent[p], l = kLm0 + 3 * idx[k];
            const double* Ht = HtAll + 9LL * k;
            const double s0 = blkSym(S, ld, i, l), s1 = blkSym(S, ld, i, l + 1), s2 = blkSym(S, ld, i, l + 2);
            for (int r = 0; r < rows; ++r) Brow[rows * p + r] = dot3(s0, Ht[3 * r], s1, Ht[3 * r + 1], s2, Ht[3 * r + 2]);
        }
        return;
    }
    const int t = (int)blockIdx.x - nIB, P = t / nPT, Q = t % nPT;
    if (Q > P) return;
    const int p = blocks::kPairs * P + (tid >> 4), q = blocks::kPairs * Q + (tid & 15);
    if (p >= cnt || q > p) return;
    const int k = ent[p], k2 = ent[q], l = kLm0 + 3 * idx[k], l2 = kLm0 + 3 * idx[k2];
    const double* Ht = HtAll + 9LL * k;
    const double* Ht2 = HtAll + 9LL * k2;
    const double* R = a.Rb + ((long long)b * a.stride + k) * rows * rows;
    double A[9];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int j2 = 0; j2 < 3; ++j2) A[3 * j + j2] = blkSym(S, ld, l + j, l2 + j2);
    for (int r2 = 0; r2 < rows; ++r2) {
        double tv[3];
        blocks::blockTimesRow(A, Ht2 + 3 * r2, tv);
        for (int r = (p == q ? r2 : 0); r < rows; ++r) {
            double s = p == q ? R[r * rows + r2] : 0.0;
#pragma unroll
            for (int j = 0; j < 3; ++j) s = fma(Ht[3 * r + j], tv[j], s);
            M[(long long)(rows * p + r) * mp + rows * q + r2] = s;
        }
    }
}

// grid = (64-row tiles of the largest filter, B), block = 64
__global__ __launch_bounds__(64) void k_blk_gamma(BlkArgs a) {
    const int b = blockIdx.y, i = kSB * (int)blockIdx.x + (int)threadIdx.x;
    if (a.out[(long long)b * kLinHead + 3] != 0.0) return;
    const int m = blkOrder(a, b), n = kLm0 + 3 * a.g[b].N, mp = a.mp;
    if (i >= n) return;
    const double* M = blkM(a, b);
    const double* z = M + (long long)(mp + n) * mp;
    const double* y = M + (long long)(mp + i) * mp;
    double gsum = 0.0;
    int nf = 0;
    for (int k = 0; k < m; ++k) {
        const double v = y[k];
        if (!(fabs(v) < __builtin_inf())) nf = 1;
        gsum = fma(v, z[k], gsum);
    }
    blkGamma(a, b)[i] = gsum;
    if (nf || !(fabs(gsum) < __builtin_inf())) blkCount(a, b)[2] = 1;  // (every writer stores the same value)
}

// grid = B, block = 256
__global__ __launch_bounds__(256) void k_blk_tail(BlkArgs a) {
    __shared__ double sA[256], sB[256];
    __shared__ int sNeg;
    const int b = blockIdx.x, tid = threadIdx.x;
    double* out = a.out + (long long)b * kLinHead;
    if (out[3] != 0.0) return;
    const int m = blkOrder(a, b), n = kLm0 + 3 * a.g[b].N, mp = a.mp;
    const double* M = blkM(a, b);
    const double* z = M + (long long)(mp + n) * mp;
    double sz = 0.0, sl = 0.0;
    int neg = 0;
    for (int k = tid; k < m; k += 256) {
        const double l = M[(long long)k * mp + k], v = z[k];
        if (!(l > 0.0) || !(l < __builtin_inf())) neg = 1;
        sl += log(l);
        sz = fma(v, v, sz);
    }
    if (tid == 0) sNeg = 0;
    sA[tid] = sz;
    sB[tid] = sl;
    __syncthreads();
    if (neg) sNeg = 1;  // (every writer stores the same value)
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            sA[tid] += sA[tid + w];
            sB[tid] += sB[tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double nis = sA[0], logdet = 2.0 * sB[0];
        out[0] = nis;
        out[1] = logdet;
        out[2] = -0.5 * (nis + logdet + m * 1.8378770664093453);  // log(2 pi)
        double info = 0.0;
        if (sNeg || blkCount(a, b)[1] || blkCount(a, b)[2] || !(fabs(nis) < __builtin_inf()) || !(fabs(logdet) < __builtin_inf())) info = 1.0;
        else if (nis > a.gate) info = 2.0;
        out[3] = info;
    }
}

// grid = (tiles of the lower triangle of the largest filter, B), block = 256, LDS = kBlkDownLdsBytes.  Tile t = I (I + 1) / 2 + J, J <= I.
__global__ __launch_bounds__(256) void k_blk_downdate(BlkArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smemBk[];
    double (*sA)[kSP] = reinterpret_cast<double (*)[kSP]>(smemBk);  // Y_I^T: [row of the tile][k]
    double (*sB)[kSP] = sA + kSB;                                     // Y_J^T
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (a.out[(long long)b * kLinHead + 3] != 0.0) return;
    const int n = kLm0 + 3 * a.g[b].N, ld = a.ld, m = blkOrder(a, b), mp = a.mp;
    int I = 0;
    while ((I + 1) * (I + 2) / 2 <= (int)blockIdx.x) ++I;
    const int J = (int)blockIdx.x - I * (I + 1) / 2;
    const int I0 = kSB * I, J0 = kSB * J;
    if (I0 >= n) return;
    double* S = a.Sigma + (long long)b * a.sigmaStride;
    const double* Yt = blkM(a, b) + (long long)mp * mp;
    const bool diag = I == J;
    double sig[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int gr = I0 + kQB * wv + (lane >> 4) + 4 * q, gc = J0 + kQB * i + (lane & 15);
            sig[i][q] = (gr < n && gc < n && !(diag && i > wv)) ? S[(long long)gr * ld + gc] : 0.0;
        }
    for (int k0 = 0; k0 < m; k0 += kSB) {
        for (int e = tid; e < kSB * kSB; e += 256) {
            const int rr = e >> 6, cc = e & 63;
            const bool kin = k0 + cc < m;
            sA[rr][cc] = (kin && I0 + rr < n) ? Yt[(long long)(I0 + rr) * mp + k0 + cc] : 0.0;
            sB[rr][cc] = (kin && J0 + rr < n) ? Yt[(long long)(J0 + rr) * mp + k0 + cc] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (diag && i > wv) continue;  // (sub-tiles above the diagonal: written as mirrors)
            // the product of these 64 rows of Y from a zero accumulator, then ONE subtraction
            f64x4 acc = {0.0, 0.0, 0.0, 0.0};
            acc = mmTile<true, kSB>(acc, &sA[0][0], kSP, kQB * wv, &sB[0][0], kSP, kQB * i, lane, 1.0);
#pragma unroll
            for (int q = 0; q < 4; ++q) sig[i][q] = sig[i][q] - acc[q];
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (diag && i > wv) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int gr = I0 + kQB * wv + (lane >> 4) + 4 * q, gc = J0 + kQB * i + (lane & 15);
            if (gr < n && gc < n && (!diag || gc <= gr)) {
                S[(long long)gr * ld + gc] = sig[i][q];
                if (gc != gr) S[(long long)gc * ld + gr] = sig[i][q];
            }
        }
    }
}

}  // namespace eqf
