// Pairwise merge costs of the filters of one handle (eqf_get_merge_costs): Runnalls' Kullback-Leibler bound and the Bhattacharyya distance.
//
// Everything is taken in ONE chart chi_c, c = xHat_ref (eqf_mixture.hpp): per distinct member b the error e_b and J'_b come from
// k_local_jacobian, k_mix_estimate and k_mix_error, and Sigma'_b = J'_b Sigma_b J'_b^T from k_sigma_local run on the J' records -- for the
// member that IS ref J' = J bit for bit, so its image is the one eqf_get_nees(local = 1) factors.  The images stand in the handle's scratch
// image set (eqf_filter::dSigmaLoc), one per distinct member.
//
// An ITEM is one image to factor: a member by itself, or the pair of positions i < j with
//   SigmaBar_ij = Sigma'_i + alpha (Sigma'_j - Sigma'_i)   (one subtraction, one fused multiply-add per entry),   d = e_j - e_i.
// Items are processed in chunks of at most `chunk` images of a workspace of their own:
//   k_pair_form   THE MEMORY-BOUND HALF: grid (rows + 1, items of the chunk).  Workgroup (r, k) streams row r of the lower triangles of the
//                 two member images in 16-byte accesses (two columns per lane, rows are 128-byte aligned) and writes row r of the item's
//                 image: one writer per entry, only the lower triangle (row >= column) is written, as only it is read.  A self item is a
//                 plain copy.  The structural pad row 11 is written as a row of the identity.  The extra workgroup writes d in the padded
//                 index map of the submatrix into the item's right-hand-side row, and the item's landmark count.
//   the factorisation (eqf_factor.hpp: k_factor_diag / _panel / _trail<NeesArgs>) and k_nees_tail (eqf_nees.hpp), as eqf_get_nees runs
//                 them: the blocked fp64 Cholesky on the matrix cores with the right-hand side carried along, the images of the chunk in
//                 grid.y.  eqf_nees.hpp's factorView takes an image's order from Glob[b].N: the workspace carries one Glob per image of
//                 which only N is ever written or read.  Members and pairs go through the same kernels, so identical inputs give
//                 identical bits: a pair of bit-identical members has ld_ij == ld_i, maha == 0, cost == 0.
//   k_pair_tail   one lane per item of the chunk: the info word (-1 if a chart either member needs is singular, else k_nees_tail's), log1p,
//                 the cost (eqf_mergecost_host.hpp's text) from the item's record and the two members' records, which earlier launches
//                 have written: the member items come first, in chunks of their own.
// No atomics, every sum in k_nees_tail's fixed order: the record of an item depends on the two member images and the two weights alone.
#pragma once
#include "eqf_device.hpp"
#include "eqf_local.hpp"
#include "eqf_mergecost_host.hpp"
#include "eqf_nees.hpp"

namespace eqf {

constexpr int kPairRec = 8;  // per item: cost, logdet, maha, info, min_pivot, dof, 0, 0

struct PairItem {  // (mergecost::Item)
    int i, j, bi, bj, self, pad_;
    double alpha, wi, wj;
};

struct PairArgs {
    const PairItem* items;  // all items of the call; the chunk is items[item0 .. item0 + count)
    int item0, count;
    const double* S;        // member images Sigma'_b [B], padded layout of Sigma
    int ld;
    long long strideS;
    const double* err;      // e_b [B][ld], padded index map
    const double* jacT;     // J' records: [13] the singular-chart word of a member
    int cap;
    int N, off, kind;
    double* W;              // [chunk] workspace images, stride strideS
    double* E;              // [chunk][ldE]
    int ldE;
    Glob* wg;               // [chunk]
    const double* neesOut;  // [chunk][kNeesHead + kNeesRhs]
    double* rec;            // [items][kPairRec]
};

// grid = (12 + 3 N + 1, count), block = 256
__global__ __launch_bounds__(256) void k_pair_form(PairArgs a) {
    const int k = blockIdx.y, tid = threadIdx.x, r = blockIdx.x;
    const int nn = kLm0 + 3 * a.N;
    const PairItem it = a.items[a.item0 + k];
    if (r == nn) {  // the right-hand side and the order
        const int m = nn - a.off;
        const double* ei = a.err + (long long)it.bi * a.ld + a.off;
        const double* ej = a.err + (long long)it.bj * a.ld + a.off;
        double* E = a.E + (long long)k * a.ldE;
        for (int c = tid; c < m; c += 256) E[c] = it.self ? 0.0 : ej[c] - ei[c];
        if (tid == 0) a.wg[k].N = a.N;
        return;
    }
    const double* Si = a.S + (long long)it.bi * a.strideS + (long long)r * a.ld;
    const double* Sj = a.S + (long long)it.bj * a.strideS + (long long)r * a.ld;
    double* W = a.W + (long long)k * a.strideS + (long long)r * a.ld;
    const double al = it.alpha;
    if (r == kBase) {  // the structural pad: a row of the identity
        if (tid <= kBase) W[tid] = tid == kBase ? 1.0 : 0.0;
        return;
    }
    // columns c, c + 1 <= r by one lane in one 16-byte access; the row's last entry alone where r is even
    for (int c = 2 * tid; c <= r; c += 512) {
        if (c + 1 <= r) {
            const double2 x = *reinterpret_cast<const double2*>(Si + c);
            double2 o = x;
            if (!it.self) {
                const double2 y = *reinterpret_cast<const double2*>(Sj + c);
                o.x = fma(al, y.x - x.x, x.x);
                o.y = fma(al, y.y - x.y, x.y);
            }
            *reinterpret_cast<double2*>(W + c) = o;
        } else {
            const double x = Si[c];
            W[c] = it.self ? x : fma(al, Sj[c] - x, x);
        }
    }
}

// grid = ceil(count / 256), block = 256
__global__ __launch_bounds__(256) void k_pair_tail(PairArgs a) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= a.count) return;
    const PairItem it = a.items[a.item0 + k];
    const double* o = a.neesOut + (long long)k * (kNeesHead + kNeesRhs);
    double* rec = a.rec + (long long)(a.item0 + k) * kPairRec;
    const double nan = __builtin_nan("");
    const bool sing = a.jacT[it.bi * jacStride(a.cap) + 13] != 0.0 || a.jacT[it.bj * jacStride(a.cap) + 13] != 0.0;
    const double ld = o[0], maha = o[kNeesHead];
    int info = sing ? -1 : (o[3] != 0.0 ? 1 : 0);
    double cost = 0.0;
    if (!info && !it.self) {
        // the members' records: items i and j of the call, written by an earlier launch (members and pairs never share a chunk)
        const double* ri = a.rec + (long long)it.i * kPairRec;
        const double* rj = a.rec + (long long)it.j * kPairRec;
        cost = mergecost::cost(a.kind, ri[1], rj[1], ld, maha, it.wi, it.wj, it.alpha);
        if (!(cost == cost) || !(maha == maha) || !(fabs(cost) < __builtin_inf()) || !(fabs(maha) < __builtin_inf())) info = 1;  // (a member's trouble: NaN)
    }
    rec[0] = info ? nan : cost;
    rec[1] = info ? nan : ld;
    rec[2] = info ? nan : (it.self ? 0.0 : maha);
    rec[3] = (double)info;
    rec[4] = info ? nan : o[1];
    rec[5] = o[2];
    rec[6] = 0.0;
    rec[7] = 0.0;
}

}  // namespace eqf
