// Bearing, range and position rows formed on the device (eqf_observe_landmarks): k_obs_rows takes k_blk_rows's place in the launch
// sequence of eqf_update_landmarks(local = 0) (eqf_blocks.hpp) and every launch behind it is that call's.  One thread per entry gathers
// the landmark's origin p0_i and group element Q_i = (q_i, a_i) by the entry's index, forms J_i = a_i^-1 R(q_i)^T with k_local_jacobian's
// device function (observe::landmarkJ), then the rows Ht and the residual of eqf_observe_host.hpp's entryRows at the estimate
// p_hat = J_i p0_i, and stores both ONCE, as doubles, into the call's rows array (observe::RowsLayout) -- what Ht_out / resid_out are
// copied from.  blkRowsEntry and blkRowsClose then take those stored doubles exactly as k_blk_rows takes a caller's: the update is bit
// for bit eqf_update_landmarks(local = 0) with the rows returned.  An entry that is not observable (used = 3) is a decoupled block that
// is never formed, like an absent or a gated one; its rows are stored as zeros, and so are those of an absent entry.  The gravity chart
// plays no part: the verdict word is never -1.  Nothing is read back by the host, nothing is shared between filters, no atomics.
#pragma once
#include "eqf_blocks.hpp"
#include "eqf_observe_host.hpp"

namespace eqf {

struct ObsArgs {
    BlkArgs a;           // Hb / resid: the rows array below; jac: nullptr
    int kind;
    const double* cam;   // [B][observe::kCam]
    const double* meas;  // [B][stride][3]
    const double* p0;    // [B][3][cap]
    const double* Q;     // [B][5][cap]
    double* Ht;          // [B][stride][rows][3]
    double* resid;       // [B][stride][rows]
};

// grid = B, block = 256
__global__ __launch_bounds__(256) void k_obs_rows(ObsArgs o) {
    const BlkArgs& a = o.a;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int N = a.g[b].N, n = kLm0 + 3 * N, rows = a.rows, cap = a.cap;
    const int info = a.mask[b] ? 0 : 3;
    int* used = blkUsed(a, b);
    if (tid == 0) blkRowsOpen(a, b, info);
    if (info == 3) return;  // (the operands of a filter that is masked out are never read)
    const int nkb = min(max(a.nk[b], 0), a.stride);
    const double* S = a.Sigma + (long long)b * a.sigmaStride;
    const double* p0 = o.p0 + (long long)b * 3 * cap;
    const double* Q = o.Q + (long long)b * 5 * cap;
    const double* cam = o.cam + (long long)b * observe::kCam;
    for (int k = tid; k < nkb; k += 256) {
        const long long e = (long long)b * a.stride + k;
        const int i = a.idx[e];
        double* Ht = o.Ht + e * rows * 3;
        double* rs = o.resid + e * rows;
        int verdict = blocks::kAbsent;
        if (i >= 0 && i < N) {
            double J[9], h[9], r[3];
            observe::landmarkJ(quat{Q[i], Q[cap + i], Q[2 * cap + i], Q[3 * cap + i]}, Q[4 * cap + i], J);
            const int no = observe::entryRows(o.kind, J, mk3(p0[i], p0[cap + i], p0[2 * cap + i]), cam, o.meas + e * 3, h, r);
            for (int q = 0; q < 3 * rows; ++q) Ht[q] = h[q];
            for (int q = 0; q < rows; ++q) rs[q] = r[q];
            verdict = no ? observe::kNotObservable : blkRowsEntry(a, b, k, i, S, Ht, nullptr, a.Rb + e * rows * rows, rs);
        } else {
            for (int q = 0; q < 3 * rows; ++q) Ht[q] = 0.0;
            for (int q = 0; q < rows; ++q) rs[q] = 0.0;
        }
        used[k] = verdict;
    }
    blkRowsClose(a, b, nkb, n, info, o.resid);
}

}  // namespace eqf
