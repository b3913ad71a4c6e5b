// Split filters into mixture components on the device (eqf_split_filters; the host's decisions: eqf_split_host.hpp).
//
// Per named source, with its caller-supplied row a (Ht = a, or a J when local):  B = Sigma Ht^T,  S = Ht B,  u = B / sqrt(S).  A child
// (dst, src, shift, shrink) then is what eqf_copy_filters(src -> dst) leaves, with Sigma_dst = Sigma_src - shrink u u^T and the state
// moved by gamma = shift u with k_apply_increment's plain step.  Everything is fp64 in the padded index map of eqf_device.hpp.
//
//   k_split_row      one workgroup per source: a (reference map) -> Ht (padded map, column 11 zero), times J's blocks from the right
//                    when local -- eqf_linear.hpp's linRowBase / linRowLandmark, the expressions of k_lin_rows.
//   k_split_axis     B = Sigma Ht^T.  A workgroup takes kSplitAxisRows rows of one source, a wavefront one row at a time: lane l reads
//                    the 16 bytes at columns 2 l + 128 t, t ascending -- a wavefront one contiguous kilobyte of the row per step -- and
//                    keeps one sum per column parity (one fused multiply-add per entry); the two are added, then the 64 lanes fold
//                    by halves (32, 16, .. 1).  Sigma is read once; the order depends on nothing but the column index.
//   k_split_verdict  one workgroup per source: S = sum_j Ht_j B_j (thread t sums j = t, t + 256, .. ascending, then a tree over the 256
//                    partial sums), the verdict -- -1 local and the gravity chart singular, 1 S not positive or a value of B, S or u
//                    not finite, else 0 --, u, and for every child of the source its increment shift u into the row of its dst and its
//                    byte of k_apply_increment's mask (shift != 0).  A failed source writes no increment, clears its children's mask
//                    bytes and withdraws their pairs from the clone route's table (dst = -1).
//   k_split_sigma    the fan-out.  One workgroup owns a tile of kSplitTileRows rows x 512 columns of one source: every lane loads its 16
//                    bytes of each row once, forms p = u_i u_j (rounded) and stores fma(-shrink_k, p, Sigma_ij) into every child of the
//                    source, the one in place included.  u_i u_j commutes, so entry (i, j) and (j, i) take the same value from a
//                    symmetric Sigma without a mirror pass; a child with shrink = 0 gets the loaded bits themselves (and the child in
//                    place nothing at all).  The children are walked in the table (no list in LDS); rows and columns beyond the source's
//                    extent 12 + 3 N are not touched.  One tile read, K written: (1 + K) n^2 values per source.
// The small state is copied by eqf_clone.hpp's k_clone_small / k_clone_restore over the pair table, the children with shift != 0 are
// moved by eqf_sample.hpp's k_apply_increment.  Row 11 of Sigma is zero and Ht's column 11 is zero, so B's, u's and every increment's
// entry 11 are exact zeros and the pad stays zero.  Nothing is shared between sources, no atomics, one fixed summation order: bit for bit
// the same from run to run and for a filter alone in a handle or anywhere in a batch.
#pragma once
#include "eqf_clone.hpp"
#include "eqf_device.hpp"
#include "eqf_linear.hpp"
#include "eqf_local.hpp"
#include "eqf_math.hpp"

namespace eqf {

constexpr int kSplitAxisRows = 16;  // rows of Sigma per workgroup of k_split_axis (four per wavefront)
constexpr int kSplitTileRows = 8;   // rows of a tile of k_split_sigma = 16-byte loads in flight per lane
constexpr int kSplitTileCols = 512; // ... and its columns: 256 lanes x 16 bytes

struct SplitSource {
    int src, N;
    int first, count;  // its children in the child table
};
struct SplitChild {
    int dst, pair, call, source;
};

struct SplitArgs {
    const double* Sigma;  // the current ping-pong buffer (read by the first three kernels)
    double* SigmaW;       // ... the same buffer, written by k_split_sigma
    int ld;
    long long sigmaStride;
    const double* rows;   // [ns][ldr], reference index map
    int ldr;
    const double* shift;  // [n], child table's order
    const double* shrink; // [n]
    const SplitSource* sources;
    int ns;
    const SplitChild* children;
    ClonePair* pairs;     // the clone route's table of this call: k_split_verdict withdraws the pairs of a failed source
    const double* jac;    // k_local_jacobian's records, or nullptr (local = 0)
    int cap;
    double *Ht, *Bv, *U;  // [ns][ld]
    double* G;            // [B][ld] increments, by filter
    double* rec;          // [ns][2]: S, info
    unsigned char* mask;  // [B], by filter; zeroed before the launches
};

// grid = ns, block = 256
__global__ __launch_bounds__(256) void k_split_row(SplitArgs a) {
    const int si = blockIdx.x, tid = threadIdx.x;
    const SplitSource s = a.sources[si];
    const double* h = a.rows + (long long)si * a.ldr;
    double* o = a.Ht + (long long)si * a.ld;
    const double* jac = a.jac ? a.jac + s.src * jacStride(a.cap) : nullptr;
    for (int e = tid; e < s.N + 1; e += 256) {
        if (e == 0) linRowBase(h, jac, o);
        else linRowLandmark(h + kBase + 3 * (e - 1), jac, e - 1, o + kLm0 + 3 * (e - 1));
    }
    const int n = kLm0 + 3 * s.N;
    if (tid == 0 && n < a.ld) o[n] = 0.0;  // (the second half of an odd order's last 16 bytes)
}

// grid = (ceil(max n / kSplitAxisRows), ns), block = 256
__global__ __launch_bounds__(256) void k_split_axis(SplitArgs a) {
    typedef double V __attribute__((ext_vector_type(2)));
    const int si = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const SplitSource s = a.sources[si];
    const int n = kLm0 + 3 * s.N, ld = a.ld;
    const double* S = a.Sigma + (long long)s.src * a.sigmaStride;
    const double* Ht = a.Ht + (long long)si * ld;
    double* Bv = a.Bv + (long long)si * ld;
    for (int q = 0; q < kSplitAxisRows / 4; ++q) {
        const int r = blockIdx.x * kSplitAxisRows + 4 * q + wv;
        if (r >= n) break;
        const double* row = S + (long long)r * ld;
        double s0 = 0.0, s1 = 0.0;
        for (int c = 2 * lane; c < n; c += 128) {
            V v = *reinterpret_cast<const V*>(row + c);
            const V h = *reinterpret_cast<const V*>(Ht + c);
            if (c + 1 >= n) v.y = 0.0;  // (beyond the extent: not this filter's)
            s0 = fma(v.x, h.x, s0);
            s1 = fma(v.y, h.y, s1);
        }
        double t = s0 + s1;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) t += __shfl_down(t, d, 64);
        if (lane == 0) Bv[r] = t;
    }
}

// grid = ns, block = 256
__global__ __launch_bounds__(256) void k_split_verdict(SplitArgs a) {
    __shared__ double sSum[256];
    const int si = blockIdx.x, tid = threadIdx.x;
    const SplitSource s = a.sources[si];
    const int n = kLm0 + 3 * s.N, ld = a.ld;
    const double* Ht = a.Ht + (long long)si * ld;
    const double* Bv = a.Bv + (long long)si * ld;
    double* U = a.U + (long long)si * ld;
    const double inf = __builtin_inf();
    double part = 0.0;
    int nf = 0;
    for (int j = tid; j < n; j += 256) {
        const double b = Bv[j];
        if (!(fabs(b) < inf)) nf = 1;
        part = fma(Ht[j], b, part);
    }
    sSum[tid] = part;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if (tid < d) sSum[tid] += sSum[tid + d];
        __syncthreads();
    }
    const double Sv = sSum[0];
    nf = __syncthreads_or(nf);
    int info = 0;
    const double* jac = a.jac ? a.jac + s.src * jacStride(a.cap) : nullptr;
    if (jac && jac[13] != 0.0) info = -1;
    else if (nf || !(Sv > 0.0) || !(Sv < inf)) info = 1;
    const double rs = sqrt(info ? 1.0 : Sv);
    if (!info) {
        int bad = 0;
        for (int j = tid; j < n; j += 256)
            if (!(fabs(Bv[j] / rs) < inf)) bad = 1;
        if (__syncthreads_or(bad)) info = 1;
    }
    if (tid == 0) {
        a.rec[2 * si] = info ? __builtin_nan("") : Sv;
        a.rec[2 * si + 1] = double(info);
    }
    if (!info) {
        for (int j = tid; j < n; j += 256) U[j] = Bv[j] / rs;
        if (tid == 0 && n < ld) U[n] = 0.0;
    }
    // (the children one after the other: O(K n) stores per source, small beside the K n^2 of the fan-out; thread t reads back the entries
    // of u it has just written itself)
    for (int c = s.first; c < s.first + s.count; ++c) {
        const SplitChild ch = a.children[c];
        const double sh = a.shift[c];
        if (!info) {
            double* G = a.G + (long long)ch.dst * ld;
            for (int j = tid; j < n; j += 256) G[j] = sh * U[j];
            if (tid == 0) a.mask[ch.dst] = sh != 0.0;
        } else if (tid == 0) {
            a.mask[ch.dst] = 0;
            if (ch.pair >= 0) a.pairs[ch.pair].dst = -1;
        }
    }
}

// grid = (ceil(max n / 512), ceil(max n / kSplitTileRows), min(ns, 65535)), block = 256
__global__ __launch_bounds__(256) void k_split_sigma(SplitArgs a) {
    typedef double V __attribute__((ext_vector_type(2)));
    const int c0 = (blockIdx.x * 256 + threadIdx.x) * 2;
    const int r0 = blockIdx.y * kSplitTileRows;
    const int ld = a.ld;
    for (int si = blockIdx.z; si < a.ns; si += gridDim.z) {
        const SplitSource s = a.sources[si];
        const int n = kLm0 + 3 * s.N;
        if (r0 >= n || c0 >= n) continue;
        if (a.rec[2 * si + 1] != 0.0) continue;  // (a failed source writes none of its children)
        const int rows = min(kSplitTileRows, n - r0);
        const double* S = a.Sigma + (long long)s.src * a.sigmaStride + (long long)r0 * ld + c0;
        const double* u = a.U + (long long)si * ld;
        const V uj = *reinterpret_cast<const V*>(u + c0);
        V v[kSplitTileRows], p[kSplitTileRows];
#pragma unroll
        for (int r = 0; r < kSplitTileRows; ++r) {
            const int rr = min(r, rows - 1);
            v[r] = *reinterpret_cast<const V*>(S + (long long)rr * ld);
            const double ui = u[r0 + rr];
            p[r].x = __dmul_rn(ui, uj.x);
            p[r].y = __dmul_rn(ui, uj.y);
        }
        const bool full = c0 + 2 <= n;  // (else the row's last, partial 16 bytes: one entry)
        for (int c = s.first; c < s.first + s.count; ++c) {
            const int dst = a.children[c].dst;
            const double k = a.shrink[c];
            if (k == 0.0 && dst == s.src) continue;  // (in place and no shrink: every bit is there)
            double* D = a.SigmaW + (long long)dst * a.sigmaStride + (long long)r0 * ld + c0;
#pragma unroll
            for (int r = 0; r < kSplitTileRows; ++r) {
                if (r >= rows) break;
                V w = v[r];
                if (k != 0.0) {  // (a child without shrink is written by selection: the source's bits, signs of zeros included)
                    w.x = __fma_rn(-k, p[r].x, v[r].x);
                    w.y = __fma_rn(-k, p[r].y, v[r].y);
                }
                if (full) *reinterpret_cast<V*>(D + (long long)r * ld) = w;
                else D[(long long)r * ld] = w.x;
            }
        }
    }
}

}  // namespace eqf
