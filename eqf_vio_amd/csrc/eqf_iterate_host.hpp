// What eqf_observe_landmarks_iterated shares between the host and the device (kernels: eqf_iterate.hpp): the argument checks it adds to
// eqf_observe_landmarks's, the layouts of its workspace, the number of launches it adds, an entry's rows at a trial point, and the stop
// rule as a small state machine that one thread per filter steps.  Needs eqf_math.hpp like eqf_observe_host.hpp;
// tests/iterate_host_main.cpp runs all of it under the sanitizers without a GPU.
//
// The iteration is Gauss-Newton on the MAP cost in the chart of the PRIOR estimate.  Chart coordinates are truth minus estimate, so with
// the estimate moved by g the prior's error is eps_0 = eps_k + g, and the measurement linearised at the moved estimate reads
//   meas = h_k + Ht_k eps_k = h_k + Ht_k (eps_0 - g)   =>   r~_k = resid_k + Ht_k g   is the residual of the rows Ht_k on eps_0.
// This holds to the order to which the filter itself treats Sigma as unchanged by a group step.  Only a landmark's own 3-block of g moves
// its group element (eqf_math.hpp's landmarkStep), so the trial point of an entry needs g on that entry's landmark alone.
#pragma once
#include <cmath>
#include <cstddef>

#include "eqf_observe_host.hpp"

namespace eqf::iterate {

constexpr int kMaxLin = 16;
// eqf_iter_report::status
constexpr int kConverged = 0, kExhausted = 1, kStalled = 2, kSolveFailed = 3, kMasked = 4;

// what the call checks beyond eqf_observe_landmarks's own arguments
inline bool argsOk(int maxLin, double tol) { return maxLin >= 1 && maxLin <= kMaxLin && tol >= 0.0 && std::isfinite(tol); }

// ---- launches ------------------------------------------------------------------------------------------------------------------------------
// order of S_k padded to a tile, as blocks::WorkLayout::mp
inline int paddedS(int stride, int rows) { return blocks::roundTile(rows * stride); }
// the shared blocked Cholesky with ONE block row of right-hand side: diag(0), then per block column a diagonal block (behind the first), a
// panel and -- but for the last -- the trailing tiles
inline int factorLaunches(int nb) { return nb <= 0 ? 1 : 3 * nb - 1; }
// The launches the call adds to eqf_observe_landmarks's own, a function of stride, rows and max_lin only: per intermediate solve the form
// kernel, the factorisation, the step kernel and the rows kernel; one commit kernel behind them.  max_lin = 1 adds none.
inline int extraLaunches(int stride, int rows, int maxLin) {
    if (maxLin <= 1) return 0;
    return (maxLin - 1) * (3 + factorLaunches(paddedS(stride, rows) / blocks::kTile)) + 1;
}

// ---- layouts -------------------------------------------------------------------------------------------------------------------------------
// The device workspace, reserved with the call's other buffers.  Per filter, in doubles: the matrix [mp + 1][mp] (rows [0, mp) S_k -> L, row
// mp r~_k -> z) | T [3 stride][mp] (row 3 p + j: state index j of the p-th entry that takes part) | w [mp] | g [stride][3] (the increment
// of the rows in use, by entry) | gNext [stride][3] | the record of the current diagonal block [dRec] | lastStep.  Per filter, in ints:
// stopped | n_lin | status | cur (which of the two row buffers is in use) | bad pivot | 3 spare.
struct WorkLayout {
    int stride, rows, dRec;
    int mp() const { return paddedS(stride, rows); }
    long long offS() const { return 0; }
    long long offT() const { return (long long)(mp() + 1) * mp(); }
    long long offW() const { return offT() + 3LL * stride * mp(); }
    long long offG() const { return offW() + mp(); }
    long long offGn() const { return offG() + 3LL * stride; }
    long long offD() const { return offGn() + 3LL * stride; }
    long long offStep() const { return offD() + dRec; }
    long long strideD() const { return offStep() + 1; }
    static constexpr int kStopped = 0, kNLin = 1, kStatus = 2, kCur = 3, kBad = 4, kInts = 8;
};
// g_trace on the device: [maxLin][B][stride][3] doubles
inline size_t traceDoubles(int maxLin, int B, int stride) { return size_t(maxLin) * B * stride * 3; }
// the call's image is observe::SmallLayout's with one byte per entry behind it: 1 when the entry's landmark is considered
inline size_t offConsider(const observe::SmallLayout& s) { return s.bytes(); }
inline size_t smallBytes(const observe::SmallLayout& s) { return s.bytes() + s.entries(); }
// eqf_iter_report of a filter when the call took one linearisation (nothing was solved on the way), from the update's verdict word: a
// filter that is masked out (word 3) took no part, every other one used up its single linearisation
struct Report {
    int n_lin, status;
    double last_step;
};
inline Report singleReport(int word) { return word == 3 ? Report{0, kMasked, 0.0} : Report{1, kExhausted, 0.0}; }
// is id in the strictly ascending list?
inline bool considered(const int* list, int n, int id) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (list[mid] < id) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && list[lo] == id;
}

// ---- one entry at a trial point ----------------------------------------------------------------------------------------------------------------
// r~ = resid + Ht g, per row: the residual first, then the three products as fused multiply-adds in the order of g's components
EQF_DI void shiftResid(int rows, const double* Ht, d3 g, const double* resid, double* rt) {
    for (int r = 0; r < rows; ++r) rt[r] = fma(Ht[3 * r + 2], g.z, fma(Ht[3 * r + 1], g.y, fma(Ht[3 * r], g.x, resid[r])));
}
// Entry rows at Q_trial = Delta_i(g, p0) Q_i, with Q_i the handle's UNCHANGED group element of landmark i (Q: [5][cap], the handle's
// layout): Ht (rows x 3) and r~ (rows).  Returns 0, or 1 when the entry is not observable there (observe::entryRows; a trial point that
// is not finite ends there too): Ht and r~ are then zeros.
EQF_DI int trialRows(int kind, const double* Q, int cap, int i, d3 p0, d3 g, const double* cam, const double* meas, double* Ht, double* rt) {
    quat qn;
    double an, J[9], resid[3];
    landmarkStep(p0, g, Q, cap, i, &qn, &an);
    observe::landmarkJ(qn, an, J);
    const int rows = observe::rowsOf(kind);
    if (observe::entryRows(kind, J, p0, cam, meas, Ht, resid)) {
        for (int r = 0; r < rows; ++r) rt[r] = 0.0;
        return 1;
    }
    shiftResid(rows, Ht, g, resid, rt);
    return 0;
}

// ---- the stop rule ---------------------------------------------------------------------------------------------------------------------------
// One filter's progress.  cur: the row buffer that holds the rows in use -- the ones committed when the filter stops.
struct State {
    int stopped, nLin, status, cur;
    double lastStep;
};
EQF_DI State start() { return State{0, 0, kExhausted, 0, 0.0}; }
// Behind intermediate solve k (0-based; the rows in use are linearisation k's).  failed: S_k was not positive definite or a value was not
// finite; lastStep = max |g_{k+1} - g_k|.  Returns 1 when linearisation k + 1 is to be formed.  tol = 0 never stops early.
EQF_DI int afterSolve(State& s, int k, int failed, double lastStep, double tol) {
    if (s.stopped) return 0;
    if (failed || !(lastStep < HUGE_VAL)) {
        s.stopped = 1;
        s.nLin = k + 1;
        s.status = kSolveFailed;
        s.lastStep = __builtin_nan("");
        return 0;
    }
    s.lastStep = lastStep;
    if (tol > 0.0 && lastStep <= tol) {
        s.stopped = 1;
        s.nLin = k + 1;
        s.status = kConverged;
        return 0;
    }
    return 1;
}
// Behind the rows of linearisation k + 1.  stalled: an entry was not observable there -- the rows of linearisation k stay in use.
EQF_DI void afterRows(State& s, int k, int stalled) {
    if (s.stopped) return;
    if (stalled) {
        s.stopped = 1;
        s.nLin = k + 1;
        s.status = kStalled;
        return;
    }
    s.cur ^= 1;
}
// Behind the last linearisation: a filter that never stopped ran out of them; one that is masked out took no part.
EQF_DI void afterAll(State& s, int maxLin, int masked) {
    if (masked) {
        s = State{1, 0, kMasked, 0, 0.0};
        return;
    }
    if (!s.stopped) {
        s.stopped = 1;
        s.nLin = maxLin;
        s.status = kExhausted;
    }
}

}  // namespace eqf::iterate
