// Schmidt (consider) measurement updates (eqf_update_linear_schmidt / eqf_update_landmarks_schmidt).  A chosen set C of a
// filter's landmarks -- c their padded indices -- keeps its estimate and its covariance block; its uncertainty and its cross-correlations
// still enter S and the gain of everything else.  With B, S = L L^T, Y, z of eqf_linear.hpp / eqf_blocks.hpp unchanged (their kernels
// run as they are), the gain with rows c zeroed in the Joseph form gives
//   gamma_i = (Y^T z)_i off c, +0.0 on c;     Sigma_ij -= (Y^T Y)_ij unless i and j are both in c.
// What the host decides (the partition, the image, the grid) is eqf_schmidt_host.hpp's.
//
//   k_schmidt_gamma     writes +0.0 over gamma's consider entries of a filter whose verdict word is 0; in front of the lift and of
//                       k_apply_increment, which then see the masked gamma and need no change.  The same launch brings the partition's
//                       image over: it reads the pinned host image and writes the device copy the downdate reads (no copy command between
//                       the kernels of the call: a copy engine's hand-over costs more than this launch).
//   k_schmidt_downdate  in place of k_lin_downdate (Layout SchLin: Y [16][ld], one 16-chunk) / k_blk_downdate (SchBlk: Yt [n][mp], 64-chunks
//                       of m).  Workgroup (P, J) of a filter gathers the 64 active rows activeIdx[64 P ..] of Y into sA, takes the 64
//                       contiguous columns 64 J .. into sB and forms the 64 x 64 product on v_mfma_f64_16x16x4_f64 (mmTile): per chunk of k
//                       from a zero accumulator, then ONE subtraction, chunks ascending -- the summation order of the kernel it replaces, and
//                       the product's operands commute, so entry (i, j) has the bits of the full call wherever it sits in a tile.  The
//                       grid is (rowTiles(nA) x colTiles(n), B): no workgroup exists for Sigma_cc, the cost follows nA n.
//
// One owner per entry, no atomics.  Entry (a, j), a active, belongs to the workgroup that holds row a and column j iff j is in c, or j is
// active and j <= a (schmidt::owns).  The owner reads Sigma at (max(a, j), min(a, j)) -- the lower triangle, as the kernels it replaces --
// and writes (a, j) and, if j != a, the mirror (j, a) from the same register: Sigma stays bit-for-bit symmetric.
// Why no workgroup reads an entry another one writes (the in-place hazard: a second owner would downdate twice): take an unordered pair
// {i, j} not inside c.  Both active, i >= j: entry (i, j) is owned by the holder of row i and column j; entry (j, i), i > j, is held by
// another workgroup (or the same) but NOT owned there, since i is active and i > j.  One in c, say j: only i is an active row, so (i, j)
// is the only entry of the pair any workgroup holds, and it is owned.  So every pair has exactly one owner, the owner touches Sigma at
// the two positions of its pairs and nowhere else, and a pair inside c has no workgroup row at all.  Y, the lists and the verdict are read
// only.
// Leaves at once when the verdict word is not 0.  Nothing is shared between filters and every sum runs in one fixed order: bit for bit
// the same from run to run and for a filter alone or anywhere in a batch.  The lists stay in global memory (any capacity works): a
// workgroup holds the 64 row indices of its own tile in LDS, a fixed 256 bytes, and a lane reads four column flags once.
#pragma once
#include "eqf_blocks.hpp"
#include "eqf_chol64.hpp"
#include "eqf_device.hpp"
#include "eqf_linear.hpp"
#include "eqf_schmidt_host.hpp"

namespace eqf {

struct SchArgs {
    const Glob* g;
    double* Sigma;  // the current ping-pong buffer, downdated in place
    int ld;
    long long sigmaStride;
    const double* out;          // [B][kLinHead]: entry 3 the verdict word
    const int* cnt;             // [B][2]: {number of active indices, 0}
    const int* act;             // [B][pitch]: the active padded indices, ascending
    const unsigned char* flag;  // [B][pitch]: 1 where the padded index is a consider one
    int pitch;
    const int *cntH, *actH;     // the same three in the pinned host image (k_schmidt_gamma reads them ...
    const unsigned char* flagH;
    int *cntW, *actW;           // ... and writes the device copy: cnt, act, flag above)
    unsigned char* flagW;
    double* gamma;              // filter b: gamma[b * strideG + i]
    long long strideG;
    int nJT;                    // column tiles of the launch (schmidt::colTiles)
};

// Y of eqf_update_linear: [16][ld] per filter, one chunk of 16
struct SchLin {
    static constexpr int kK = kLinRows, kP = kLinYP;
    const double* Y;  // filter b: Y + b * stride
    long long stride;
    int ld;
    EQF_DI int order(int) const { return kLinRows; }
    EQF_DI const double* base(int b) const { return Y + b * stride; }
    // chunk k0 of the rows idx(0..63) -> s[row][k]
    template <class Idx>
    EQF_DI void load(const double* y, int, int, Idx idx, double* s, int tid) const {
        for (int e = tid; e < kK * kSB; e += 256) {
            const int kk = e >> 6, rr = e & 63, i = idx(rr);
            s[rr * kP + kk] = i >= 0 ? y[(long long)kk * ld + i] : 0.0;
        }
    }
};
// Y^T of eqf_update_landmarks: [n][mp] per filter behind S in the tall matrix, m = rows * count in chunks of 64
struct SchBlk {
    static constexpr int kK = kSB, kP = kSP;
    const double* ws;  // filter b: Yt = ws + b * wsStride + mp * mp
    long long wsStride;
    int mp, rows;
    const int* count;  // filter b: count[b * wiStride]
    int wiStride;
    EQF_DI int order(int b) const { return rows * count[(long long)b * wiStride]; }
    EQF_DI const double* base(int b) const { return ws + b * wsStride + (long long)mp * mp; }
    template <class Idx>
    EQF_DI void load(const double* y, int k0, int m, Idx idx, double* s, int tid) const {
        for (int e = tid; e < kSB * kSB; e += 256) {
            const int rr = e >> 6, cc = e & 63, i = idx(rr);
            s[rr * kP + cc] = (i >= 0 && k0 + cc < m) ? y[(long long)i * mp + k0 + cc] : 0.0;
        }
    }
};
template <class L>
constexpr int schmidtLdsBytes() { return int(sizeof(double)) * 2 * kSB * L::kP; }

// grid = (ceil(pitch / 256), B), block = 256
__global__ __launch_bounds__(256) void k_schmidt_gamma(SchArgs s) {
    const int b = blockIdx.y, i = 256 * (int)blockIdx.x + (int)threadIdx.x;
    if (i >= s.pitch) return;
    const long long e = (long long)b * s.pitch + i;
    const unsigned char fl = s.flagH[e];
    s.flagW[e] = fl;
    s.actW[e] = s.actH[e];
    if (i < 2) s.cntW[2 * b + i] = s.cntH[2 * b + i];
    if (s.out[(long long)b * kLinHead + 3] != 0.0) return;
    if (i < kLm0 + 3 * s.g[b].N && fl) s.gamma[b * s.strideG + i] = 0.0;
}

// grid = (schmidt::gridX(largest nA, largest n), B), block = 256, LDS = schmidtLdsBytes<L>()
template <class L>
__global__ __launch_bounds__(256) void k_schmidt_downdate(SchArgs s, L lay) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smemSch[];
    double* sA = reinterpret_cast<double*>(smemSch);  // the gathered active rows of Y^T: [row of the tile][k]
    double* sB = sA + kSB * L::kP;                    // the columns' rows of Y^T
    __shared__ int sAct[kSB];                         // the tile's active indices, -1 past the last
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (s.out[(long long)b * kLinHead + 3] != 0.0) return;
    const int n = kLm0 + 3 * s.g[b].N, ld = s.ld, nA = s.cnt[2 * b];
    const int P = (int)blockIdx.x / s.nJT, J = (int)blockIdx.x % s.nJT;
    const int A0 = kSB * P, J0 = kSB * J;
    if (A0 >= nA || J0 >= n) return;
    if (tid < kSB) sAct[tid] = A0 + tid < nA ? s.act[(long long)b * s.pitch + A0 + tid] : -1;
    __syncthreads();
    const unsigned char* flag = s.flag + (long long)b * s.pitch;
    double* S = s.Sigma + (long long)b * s.sigmaStride;
    // this lane's four rows (the same for every sub-tile i) and four columns (one per sub-tile)
    int ga[4], gc[4];
    bool cons[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        ga[q] = sAct[kQB * wv + (lane >> 4) + 4 * q];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        gc[i] = J0 + kQB * i + (lane & 15);
        cons[i] = gc[i] < n && flag[gc[i]] != 0;
    }
    double sig[4][4];
    bool own[4][4];
    bool any[4];
    int anyTile = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        bool mine = false;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            own[i][q] = ga[q] >= 0 && gc[i] < n && (cons[i] || gc[i] <= ga[q]);
            mine = mine || own[i][q];
            const int hi = max(ga[q], gc[i]), lo = min(ga[q], gc[i]);
            sig[i][q] = own[i][q] ? S[(long long)hi * ld + lo] : 0.0;
        }
        any[i] = __ballot(mine) != 0;  // (wave-uniform: a sub-tile nobody of this wave owns anything in is not formed)
        anyTile |= any[i] ? 1 : 0;
    }
    if (!__syncthreads_or(anyTile)) return;  // (active columns all past the tile's last row: the mirror side's tile)
    const double* y = lay.base(b);
    const int m = lay.order(b);
    for (int k0 = 0; k0 < m; k0 += L::kK) {
        lay.load(y, k0, m, [&](int rr) { return sAct[rr]; }, sA, tid);
        lay.load(y, k0, m, [&](int rr) { return J0 + rr < n ? J0 + rr : -1; }, sB, tid);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (!any[i]) continue;
            // the product of this chunk of Y's rows from a zero accumulator, then ONE subtraction
            f64x4 acc = {0.0, 0.0, 0.0, 0.0};
            acc = mmTile<true, L::kK>(acc, sA, L::kP, kQB * wv, sB, L::kP, kQB * i, lane, 1.0);
#pragma unroll
            for (int q = 0; q < 4; ++q) sig[i][q] = sig[i][q] - acc[q];
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (own[i][q]) {
                S[(long long)ga[q] * ld + gc[i]] = sig[i][q];
                if (gc[i] != ga[q]) S[(long long)gc[i] * ld + ga[q]] = sig[i][q];
            }
}

}  // namespace eqf
