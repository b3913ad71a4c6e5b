// The iterated (re-linearised) landmark observation update (eqf_observe_landmarks_iterated): Gauss-Newton on the MAP cost between
// k_obs_rows and k_blk_gain of eqf_observe_landmarks.  Nothing of the handle is written here: an intermediate linearisation needs the
// increment on the named landmarks only, and that is
//   T = Sigma_MM Ht_k^T,   S_k = Ht_k T + blockdiag(R_e) = L L^T,   z = L^-1 r~_k,   w = L^-T z,   g_{k+1} = T w
// with M the 3-blocks of the entries that take part (frozen by k_obs_rows) -- no n-wide right-hand side, no downdate.  Per intermediate
// solve, behind k_obs_rows:
//   k_iter_form    16 x 16 pairs of entries per workgroup, thread (p, q): the 3 x 3 block Sigma_{pq} by the lower triangle, in place (Sigma
//                  is read again at every linearisation: nine values per pair, no gathered copy to keep), T's block (p, q) = Sigma_pq
//                  Ht_q^T, and for q <= p S's block as k_blk_gain forms it; thread (p, p) also stores r~ as the right-hand-side row.
//   the shared blocked Cholesky (eqf_factor.hpp, one right-hand-side row): L and z.
//   k_iter_step    one workgroup per filter: w by back substitution (column k of L^T is row k of L: contiguous; k descending, one fused
//                  multiply-add per element), g_{k+1} = T w (one thread per row of T, columns ascending; a considered entry gets +0.0),
//                  lastStep = max |g_{k+1} - g_k| and the stop rule (iterate::afterSolve).
//   k_iter_rows    one workgroup per filter, one thread per entry: the rows at Q_trial = Delta_i(g_{k+1}) Q_i from the handle's unchanged
//                  Q_i into the OTHER row buffer (iterate::trialRows); an entry that is not observable there stalls the filter and the
//                  buffer in use stays.  Otherwise the buffers swap, g <- g_{k+1}, and g_trace's plane k + 1 is written.
// and once behind the last: k_iter_commit copies the rows in use to where k_blk_gain reads them (the workspace's Ht, the residual row of
// the tall matrix) and to row buffer 0, which Ht_out / resid_out are copied from, and closes the report.  A filter that has stopped
// leaves every later launch at once (its order for the factorisation is 0), so its bits do not depend on its neighbours.  No atomics,
// every sum in one fixed order.
#pragma once
#include "eqf_blocks.hpp"
#include "eqf_iterate_host.hpp"
#include "eqf_observe.hpp"

namespace eqf {

struct IterArgs {
    BlkArgs a;
    int kind;
    const double* cam;   // [B][observe::kCam]
    const double* meas;  // [B][stride][3]
    const double* p0;    // [B][3][cap]
    const double* Q;     // [B][5][cap]
    const unsigned char* consider;  // [B][stride]: the entry's landmark is considered
    double* rowsBuf;     // two observe::RowsLayout arrays, bufStride doubles apart
    long long bufStride, offResid;
    double* ws;          // [B][wsStride]: iterate::WorkLayout
    long long wsStride, offT, offW, offG, offGn, offD, offStep;
    int* wi;             // [B][iterate::WorkLayout::kInts]
    double* trace;       // [maxLin][B][stride][3]
    int maxLin, B;
    double tol;
};

EQF_DI double* itS(const IterArgs& t, int b) { return t.ws + b * t.wsStride; }
EQF_DI int* itI(const IterArgs& t, int b) { return t.wi + (long long)b * iterate::WorkLayout::kInts; }
EQF_DI double* itHt(const IterArgs& t, int buf) { return t.rowsBuf + buf * t.bufStride; }
EQF_DI double* itResid(const IterArgs& t, int buf) { return t.rowsBuf + buf * t.bufStride + t.offResid; }
// does filter b still iterate?  (one that is masked out, verdict word 3, never does; one in which no entry takes part, kInfoIdle, has
// order 0 and g = 0 throughout)
EQF_DI bool itLive(const IterArgs& t, int b) {
    const double word = t.a.out[(long long)b * kLinHead + 3];
    return !itI(t, b)[iterate::WorkLayout::kStopped] && (word == 0.0 || word == (double)blocks::kInfoIdle);
}
EQF_DI FactorView factorView(const IterArgs& t, int b) {
    double* S = itS(t, b);
    const int m = itLive(t, b) ? blkOrder(t.a, b) : 0;
    return FactorView{S, t.a.mp, m, -1, S + t.offD, itI(t, b) + iterate::WorkLayout::kBad, S + (long long)t.a.mp * t.a.mp, t.a.mp, 1};
}

// grid = (nPT^2, B) with nPT = blocks::pairTiles(stride); block = 256
__global__ __launch_bounds__(256) void k_iter_form(IterArgs t, int nPT) {
    const BlkArgs& a = t.a;
    const int b = blockIdx.y, tid = threadIdx.x;
    if (!itLive(t, b)) return;
    const int rows = a.rows, cnt = *blkCount(a, b), ld = a.ld, mp = a.mp;
    const int P = (int)blockIdx.x / nPT, Q = (int)blockIdx.x % nPT;
    const int p = blocks::kPairs * P + (tid >> 4), q = blocks::kPairs * Q + (tid & 15);
    if (p >= cnt || q >= cnt) return;
    const int cur = itI(t, b)[iterate::WorkLayout::kCur];
    const double* S = a.Sigma + (long long)b * a.sigmaStride;
    const int* ent = blkEnt(a, b);
    const int* idx = a.idx + (long long)b * a.stride;
    const int k = ent[p], k2 = ent[q], l = kLm0 + 3 * idx[k], l2 = kLm0 + 3 * idx[k2];
    const long long e = (long long)b * a.stride + k, e2 = (long long)b * a.stride + k2;
    const double* Ht = itHt(t, cur) + e * rows * 3;
    const double* Ht2 = itHt(t, cur) + e2 * rows * 3;
    const double* R = a.Rb + e * rows * rows;
    double* M = itS(t, b);
    double* T = M + t.offT;
    double A[9];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int j2 = 0; j2 < 3; ++j2) A[3 * j + j2] = blkSym(S, ld, l + j, l2 + j2);
    for (int r2 = 0; r2 < rows; ++r2) {
        double tv[3];
        blocks::blockTimesRow(A, Ht2 + 3 * r2, tv);
#pragma unroll
        for (int j = 0; j < 3; ++j) T[(long long)(3 * p + j) * mp + rows * q + r2] = tv[j];
        if (q > p) continue;
        for (int r = (p == q ? r2 : 0); r < rows; ++r) {
            double s = p == q ? R[r * rows + r2] : 0.0;
#pragma unroll
            for (int j = 0; j < 3; ++j) s = fma(Ht[3 * r + j], tv[j], s);
            M[(long long)(rows * p + r) * mp + rows * q + r2] = s;
        }
    }
    if (p == q) {
        const double* rt = itResid(t, cur) + e * rows;
        for (int r = 0; r < rows; ++r) M[(long long)mp * mp + rows * p + r] = rt[r];
    }
}

// grid = B, block = 256; k: the solve (the rows in use are linearisation k's)
__global__ __launch_bounds__(256) void k_iter_step(IterArgs t, int k) {
    __shared__ double sMax[256];
    __shared__ int sBad;
    const BlkArgs& a = t.a;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (!itLive(t, b)) return;
    const int rows = a.rows, cnt = *blkCount(a, b), m = rows * cnt, mp = a.mp, stride = a.stride;
    double* M = itS(t, b);
    double* z = M + (long long)mp * mp;
    const double* T = M + t.offT;
    double* w = M + t.offW;
    double* g = M + t.offG;
    double* gn = M + t.offGn;
    int* st = itI(t, b);
    const int* pos = blkPos(a, b);
    const unsigned char* cons = t.consider + (long long)b * stride;
    int bad = st[iterate::WorkLayout::kBad];
    if (tid == 0) sBad = 0;
    // w = L^-T z: w_k = z_k / L_kk, then z_j -= L_kj w_k for j < k
    for (int c = m - 1; c >= 0; --c) {
        __syncthreads();
        const double* Lc = M + (long long)c * mp;
        const double d = Lc[c], wc = z[c] / d;
        if (!(d > 0.0) || !(fabs(wc) < __builtin_inf())) bad = 1;
        for (int j = tid; j < c; j += 256) z[j] = fma(-Lc[j], wc, z[j]);
        if (tid == 0) w[c] = wc;
    }
    __syncthreads();
    // g_{k+1} = T w by entry; what does not take part keeps +0.0
    double dmax = 0.0;
    const int nkb = min(max(a.nk[b], 0), stride);
    for (int i = tid; i < 3 * nkb; i += 256) {
        const int kk = i / 3, j = i - 3 * kk, p = pos[kk];
        double s = 0.0;
        if (p >= 0 && !cons[kk]) {
            const double* Tr = T + (long long)(3 * p + j) * mp;
            for (int c = 0; c < m; ++c) s = fma(Tr[c], w[c], s);
        }
        gn[i] = s;
        const double df = fabs(s - g[i]);
        if (!(df < __builtin_inf())) bad = 1;
        dmax = fmax(dmax, df);
    }
    sMax[tid] = dmax;
    __syncthreads();
    if (bad) sBad = 1;  // (every writer stores the same value)
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) sMax[tid] = fmax(sMax[tid], sMax[tid + h]);
        __syncthreads();
    }
    if (tid == 0) {
        iterate::State s{st[iterate::WorkLayout::kStopped], st[iterate::WorkLayout::kNLin], st[iterate::WorkLayout::kStatus],
            st[iterate::WorkLayout::kCur], M[t.offStep]};
        iterate::afterSolve(s, k, sBad, sMax[0], t.tol);
        st[iterate::WorkLayout::kStopped] = s.stopped;
        st[iterate::WorkLayout::kNLin] = s.nLin;
        st[iterate::WorkLayout::kStatus] = s.status;
        M[t.offStep] = s.lastStep;
    }
}

// grid = B, block = 256; forms linearisation k + 1
__global__ __launch_bounds__(256) void k_iter_rows(IterArgs t, int k) {
    const BlkArgs& a = t.a;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (!itLive(t, b)) return;
    const int N = a.g[b].N, rows = a.rows, cap = a.cap, stride = a.stride;
    const int nkb = min(max(a.nk[b], 0), stride);
    int* st = itI(t, b);
    const int cur = st[iterate::WorkLayout::kCur], nxt = cur ^ 1;
    const int* used = blkUsed(a, b);
    double* M = itS(t, b);
    double* g = M + t.offG;
    const double* gn = M + t.offGn;
    const double* p0 = t.p0 + (long long)b * 3 * cap;
    const double* Q = t.Q + (long long)b * 5 * cap;
    const double* cam = t.cam + (long long)b * observe::kCam;
    int stalled = 0;
    for (int kk = tid; kk < nkb; kk += 256) {
        const long long e = (long long)b * stride + kk;
        double* Ht = itHt(t, nxt) + e * rows * 3;
        double* rt = itResid(t, nxt) + e * rows;
        const int i = a.idx[e];
        if (used[kk] == blocks::kApplied && i >= 0 && i < N) {
            double h[9], r[3];
            stalled |= iterate::trialRows(t.kind, Q, cap, i, mk3(p0[i], p0[cap + i], p0[2 * cap + i]),
                mk3(gn[3 * kk], gn[3 * kk + 1], gn[3 * kk + 2]), cam, t.meas + e * 3, h, r);
            for (int q = 0; q < 3 * rows; ++q) Ht[q] = h[q];
            for (int q = 0; q < rows; ++q) rt[q] = r[q];
        } else {
            // an entry that is not frozen in keeps what linearisation 0 stored for it
            const double* Hc = itHt(t, cur) + e * rows * 3;
            const double* rc = itResid(t, cur) + e * rows;
            for (int q = 0; q < 3 * rows; ++q) Ht[q] = Hc[q];
            for (int q = 0; q < rows; ++q) rt[q] = rc[q];
        }
    }
    stalled = __syncthreads_or(stalled);
    if (tid == 0) {
        iterate::State s{0, 0, st[iterate::WorkLayout::kStatus], cur, 0.0};
        iterate::afterRows(s, k, stalled);
        if (s.stopped) {
            st[iterate::WorkLayout::kStopped] = 1;
            st[iterate::WorkLayout::kNLin] = s.nLin;
            st[iterate::WorkLayout::kStatus] = s.status;
        }
        st[iterate::WorkLayout::kCur] = s.cur;
    }
    if (stalled) return;
    double* tr = t.trace + ((long long)(k + 1) * t.B + b) * stride * 3;
    for (int i = tid; i < 3 * nkb; i += 256) {
        const double v = gn[i];
        g[i] = v;
        tr[i] = v;
    }
}

// grid = B, block = 256
__global__ __launch_bounds__(256) void k_iter_commit(IterArgs t) {
    const BlkArgs& a = t.a;
    const int b = blockIdx.x, tid = threadIdx.x;
    int* st = itI(t, b);
    const double word = a.out[(long long)b * kLinHead + 3];
    const int cur = st[iterate::WorkLayout::kCur];
    if (tid == 0) {
        double* M = itS(t, b);
        iterate::State s{st[iterate::WorkLayout::kStopped], st[iterate::WorkLayout::kNLin], st[iterate::WorkLayout::kStatus], cur, M[t.offStep]};
        iterate::afterAll(s, t.maxLin, word == 3.0);
        st[iterate::WorkLayout::kStopped] = s.stopped;
        st[iterate::WorkLayout::kNLin] = s.nLin;
        st[iterate::WorkLayout::kStatus] = s.status;
        M[t.offStep] = s.lastStep;
    }
    if (word != 0.0) return;
    const int n = kLm0 + 3 * a.g[b].N, rows = a.rows, stride = a.stride;
    const int nkb = min(max(a.nk[b], 0), stride);
    const int* pos = blkPos(a, b);
    double* HtAll = blkHt(a, b);
    double* Mz = blkM(a, b) + (long long)(a.mp + n) * a.mp;
    for (int kk = tid; kk < nkb; kk += 256) {
        const long long e = (long long)b * stride + kk;
        const double* Ht = itHt(t, cur) + e * rows * 3;
        const double* rt = itResid(t, cur) + e * rows;
        const int p = pos[kk];
        if (p >= 0) {
            for (int q = 0; q < 9; ++q) HtAll[9LL * kk + q] = q < 3 * rows ? Ht[q] : 0.0;
            for (int r = 0; r < rows; ++r) Mz[rows * p + r] = rt[r];
        }
        if (cur != 0) {
            double* H0 = itHt(t, 0) + e * rows * 3;
            double* r0 = itResid(t, 0) + e * rows;
            for (int q = 0; q < 3 * rows; ++q) H0[q] = Ht[q];
            for (int r = 0; r < rows; ++r) r0[r] = rt[r];
        }
    }
}

}  // namespace eqf
