// Scoring candidate vision frames without applying them (eqf_score_vision): the joint NIS, log det S and log-likelihood a frame WOULD have
// under a filter, from the handle's present state and Sigma, of which not a bit is written.
//
// An ITEM is one candidate of one filter.  The host (eqf_score_host.hpp) has matched its ids against the filter's and left, per item, the
// matched state slots in the state's order and the bearings permuted into that order.  With M the matched landmarks,
//   S = C_M Sigma_MM C_M^T + r I   (order 2 |M|),   S = L L^T,   z = L^-1 delta_M,   nis = z^T z,   logdet_S = 2 sum log L_kk.
// Items are processed in chunks of at most `chunk` images of a workspace of their own (leading dimension ldW >= 2 capacity):
//   k_score_form   THE MEMORY-BOUND HALF: grid (ceil(mLm / 4) + 1, items of the chunk).  A wavefront per row landmark a; its lanes run along
//                  the column landmarks b <= a: lane b reads the 3 x 3 block of Sigma at slots (s_a, s_b) -- three rows of 24-byte pieces,
//                  contiguous runs where the candidate names consecutive slots -- and C_b from lmc, forms T = C_a Sigma_ab and S_ab = T C_b^T
//                  by dot3 in the order of k_update_prep64 / k_innov_stats (C Sigma first), adds r on the diagonal and writes the 2 x 2 block:
//                  one writer per entry, of a diagonal block only the lower triangle.  Per block pair 72 bytes of Sigma are read and 32
//                  written.  The extra workgroup writes delta (gateResidual) into the item's right-hand-side row and the per-landmark
//                  statistic through gateMahalanobis itself (eqf_churn.hpp).
//   the factorisation (eqf_factor.hpp: k_factor_diag / _panel / _trail<ScoreArgs>): the blocked fp64 Cholesky on the matrix cores with the
//                  one right-hand-side row carried along, the images of the chunk in grid.y, each with its own order 2 |M|, no pad index.
//   k_score_tail   one workgroup per item: sum log L_kk and z^T z in k_nees_tail's fixed order (thread t takes the terms t, t + 256, ... in
//                  sequence, then a fixed tree), the info word from the bad-pivot word and a finiteness test, the record through
//                  eqf_score_host.hpp's text.
// No atomics, every sum in one fixed order, nothing depends on an item's place in the chunk or in the call: the record of an item is a
// function of its filter's state, its matched slots and its bearings alone.
#pragma once
#include "eqf_churn.hpp"
#include "eqf_device.hpp"
#include "eqf_factor.hpp"
#include "eqf_score_host.hpp"

namespace eqf {

struct ScoreItem {  // (score::Item)
    int b, m, first, masked;
};

struct ScoreArgs {
    const ScoreItem* items;  // all items of the call; the chunk is items[item0 .. item0 + count)
    int item0, count;
    const int* slots;        // [sum m] matched state slots, state order
    const double* y;         // [sum m][3] bearings in the same order
    const double* Q;         // [B][5][cap]
    const double* lmc;       // [B][15][cap]
    const double* S;         // the current Sigma, padded layout
    long long sigmaStride;
    int ld, cap;
    double measVar;
    double* W;               // [chunk] images, leading dimension ldW, stride strideW
    int ldW;
    long long strideW;
    double* E;               // [chunk][ldW]: delta -> z
    double* D;               // [chunk][kDRec]
    int* bad;                // [chunk]
    double* nisLm;           // [sum m]
    double* rec;             // [items][score::kRec]
};

EQF_DI FactorView factorView(const ScoreArgs& a, int k) {
    return FactorView{a.W + (long long)k * a.strideW, a.ldW, 2 * a.items[a.item0 + k].m, -1, a.D + (long long)k * kDRec, a.bad + k,
        a.E + (long long)k * a.ldW, a.ldW, 1};
}

// grid = (ceil(mLm / 4) + 1, count), block = 256; mLm: the largest matched count of the call
__global__ __launch_bounds__(256) void k_score_form(ScoreArgs a) {
    const int k = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const ScoreItem it = a.items[a.item0 + k];
    const int* slots = a.slots + it.first;
    const double* lmc = a.lmc + (long long)it.b * 15 * a.cap;
    const double* S = a.S + (long long)it.b * a.sigmaStride;
    if (blockIdx.x == gridDim.x - 1) {  // the right-hand side and the per-landmark statistic
        const double* q = a.Q + (long long)it.b * 5 * a.cap;
        double* E = a.E + (long long)k * a.ldW;
        for (int i = tid; i < it.m; i += 256) {
            const int s = slots[i];
            const double* yb = a.y + 3 * (long long)(it.first + i);
            double c[15], B[9];
#pragma unroll
            for (int e = 0; e < 15; ++e) c[e] = lmc[(long long)e * a.cap + s];
            const double* d = S + (long long)(kLm0 + 3 * s) * a.ld + kLm0 + 3 * s;
#pragma unroll
            for (int rw = 0; rw < 3; ++rw)
#pragma unroll
                for (int cc = 0; cc < 3; ++cc) B[3 * rw + cc] = d[(long long)rw * a.ld + cc];
            const quat Qq = quat{q[s], q[a.cap + s], q[2 * a.cap + s], q[3 * a.cap + s]};
            const d3 y = mk3(yb[0], yb[1], yb[2]);
            double d0, d1;
            gateResidual(Qq, y, c, &d0, &d1);
            E[2 * i] = d0;
            E[2 * i + 1] = d1;
            a.nisLm[it.first + i] = gateMahalanobis(Qq, y, c, B, a.measVar);
        }
        return;
    }
    const int ra = 4 * blockIdx.x + wv;  // row landmark of this wavefront
    if (ra >= it.m) return;
    const int sa = slots[ra];
    double Ca[6];
#pragma unroll
    for (int e = 0; e < 6; ++e) Ca[e] = lmc[(long long)e * a.cap + sa];
    const double* rowS = S + (long long)(kLm0 + 3 * sa) * a.ld + kLm0;
    double* W0 = a.W + (long long)k * a.strideW + (long long)(2 * ra) * a.ldW;
    double* W1 = W0 + a.ldW;
    for (int cb = lane; cb <= ra; cb += 64) {
        const int sb = slots[cb];
        double v[9], Cb[6], T[6];
#pragma unroll
        for (int rw = 0; rw < 3; ++rw)
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) v[3 * rw + cc] = rowS[(long long)rw * a.ld + 3 * sb + cc];
#pragma unroll
        for (int e = 0; e < 6; ++e) Cb[e] = lmc[(long long)e * a.cap + sb];
#pragma unroll
        for (int rw = 0; rw < 2; ++rw)
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) T[3 * rw + cc] = dot3(Ca[3 * rw], v[cc], Ca[3 * rw + 1], v[3 + cc], Ca[3 * rw + 2], v[6 + cc]);
        double s00 = dot3(T[0], Cb[0], T[1], Cb[1], T[2], Cb[2]);
        const double s01 = dot3(T[0], Cb[3], T[1], Cb[4], T[2], Cb[5]);
        const double s10 = dot3(T[3], Cb[0], T[4], Cb[1], T[5], Cb[2]);
        double s11 = dot3(T[3], Cb[3], T[4], Cb[4], T[5], Cb[5]);
        if (cb == ra) {  // the LOWER triangle of a diagonal block, like the chain
            s00 += a.measVar;
            s11 += a.measVar;
            W0[2 * cb] = s00;
        } else {
            W0[2 * cb] = s00;
            W0[2 * cb + 1] = s01;
        }
        W1[2 * cb] = s10;
        W1[2 * cb + 1] = s11;
    }
}

// grid = count, block = 256
__global__ __launch_bounds__(256) void k_score_tail(ScoreArgs a) {
    const int k = blockIdx.x, tid = threadIdx.x;
    const ScoreItem it = a.items[a.item0 + k];
    const int m = 2 * it.m;
    const double* W = a.W + (long long)k * a.strideW;
    const double* E = a.E + (long long)k * a.ldW;
    double sl = 0.0, sz = 0.0;
    int neg = 0;
    for (int i = tid; i < m; i += 256) {
        const double l = W[(long long)i * a.ldW + i];
        if (!(l > 0.0) || !(l < __builtin_inf())) neg = 1;
        sl += log(l);
        const double z = E[i];
        sz = fma(z, z, sz);
    }
    __shared__ double sA[256], sB[256];
    __shared__ int sNeg;
    if (tid == 0) sNeg = 0;
    sA[tid] = sl;
    sB[tid] = sz;
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
    if (tid == 0) score::writeRecord(a.rec + (long long)(a.item0 + k) * score::kRec, sB[0], 2.0 * sA[0], m, sNeg || a.bad[k]);
}

}  // namespace eqf
