// What the host decides and packs for the innovation lift of eqf_update_linear, eqf_update_landmarks, eqf_apply_increment and
// eqf_perturb_filters (eqf_lift.hpp): which lift a call and a filter take (option, settings, landmark count), the layout of the
// factorisation's right-hand side, the result record and its unpacking, and how a failed lift shows in eqf_linear_report.  Host only,
// standard library only (no HIP, no other eqf_*.hpp; the layout constants are repeated here and static_assert-ed against the device headers
// where both are seen): tests/lift_host_main.cpp runs it under the sanitizers without a GPU.
#pragma once
#include <cmath>
#include <cstddef>

namespace eqf::lift {

constexpr int kRefBase = 11;   // reference base coordinates (kBase)
constexpr int kPadBase = 12;   // ... padded (kLm0): internal index 11 is the structural pad
constexpr int kOff = 6;        // Sigma_e = Sigma[6:, 6:]: internal index of its first row
constexpr int kRhs = 7;        // right-hand-side rows: the six columns of Z_P, then [0; gamma_L]
constexpr int kRec = 16;       // doubles of a filter's record: kind, info, DeltaU[6], min_pivot, pivot_ratio, spare
constexpr int kHead = 20;      // doubles of an update's result record (kLinHead); entry 3 is its verdict word
constexpr int kMinLandmarks = 2;  // 3 N equations for 4 unknowns: one landmark leaves the 4 x 4 system rank deficient
// verdict word a failed lift leaves in an update's record.  (Not 4: eqf_blocks_host.hpp's kInfoIdle sits there.)
constexpr int kWordFailed = 5;
constexpr int kInfoFailed = 4;    // ... and the code eqf_linear_report / eqf_lift_report show for it
constexpr int kInfoNoPart = 3;

inline bool optionOk(int v) { return v == 0 || v == 1; }
// the lift of a CALL: 0 plain for every filter; 1 bundleLift + VIOExp(liftTotalSpaceInnovation); 2 bundleLift + the discrete lift
inline int callKind(int option, int useInnovationLift, int useDiscreteInnovationLift) {
    if (!option || !useInnovationLift) return 0;
    return useDiscreteInnovationLift ? 2 : 1;
}
// ... and of a FILTER of N landmarks in such a call
inline int filterKind(int kind, int N) { return N >= kMinLandmarks ? kind : 0; }
// a call factors only if some filter takes a bundleLift
inline bool callFactors(int kind, int nMax) { return filterKind(kind, nMax) != 0; }

// order of Sigma_e in the padded index map (the pad is index kPadPos of it), the pitch of a right-hand-side row, and the column of
// component c of landmark i
constexpr int kPadPos = kRefBase - kOff;
inline int order(int N) { return kPadBase + 3 * N - kOff; }
inline int rhsPitch(int nMax) { return order(nMax) < 1 ? 1 : order(nMax); }
inline int rhsColumn(int i, int c) { return kPadBase - kOff + 3 * i + c; }
inline size_t rhsDoubles(int ld) { return size_t(kRhs) * size_t(ld); }  // per filter, from the handle's leading dimension
// 64-wide block columns of the factorisation and landmark groups of k_lift_rhs's grid (four wavefronts, one landmark each)
inline int blockColumns(int nMax) { return (order(nMax) + 63) / 64; }
inline int rhsGroups(int nMax) { return (nMax + 3) / 4; }

// One filter's right-hand side from Z_P's landmark rows (Z[(3 i + r) * 6 + c]) and gamma_L (gl[3 i + r]): row c < 6 is column c of Z_P, row 6
// is [0; gamma_L]; the top five entries and the pad are zero.  (What k_lift_rhs writes; E has kRhs rows of pitch ldE >= order(N).)
inline void packRhs(const double* Z, const double* gl, int N, double* E, int ldE) {
    for (int r = 0; r < kRhs; ++r)
        for (int j = 0; j < order(N); ++j) E[size_t(r) * ldE + j] = 0.0;
    for (int i = 0; i < N; ++i)
        for (int c = 0; c < 3; ++c) {
            for (int r = 0; r < 6; ++r) E[size_t(r) * ldE + rhsColumn(i, c)] = Z[size_t(3 * i + c) * 6 + r];
            E[size_t(6) * ldE + rhsColumn(i, c)] = gl[3 * i + c];
        }
}

// the record k_lift_tail leaves (a mirror of eqf_lift_report, which this header does not see)
struct Report {
    int kind, info;
    double DeltaU[6], min_pivot, pivot_ratio;
};
inline void unpackReport(const double* rec, Report* out) {
    out->kind = int(rec[0]);
    out->info = int(rec[1]);
    for (int i = 0; i < 6; ++i) out->DeltaU[i] = rec[2 + i];
    out->min_pivot = rec[8];
    out->pivot_ratio = rec[9];
}
// an update's verdict word -> eqf_linear_report::info (the other words pass)
inline int mergeInfo(int word) { return word == kWordFailed ? kInfoFailed : word; }
// nis, logdet_S and loglik of an update are valid numbers where the update itself solved: applied, gated, or refused by the lift
inline bool updateSolved(int word) { return word == 0 || word == 2 || word == kWordFailed; }
// the block update's verdict word "no entry takes part" (eqf_blocks_host.hpp's kInfoIdle, which this header does not see)
constexpr int kWordIdle = 4;
// An update's result record -> the fields of eqf_linear_report (a mirror, as Report above).  rec: [kHead], entry 3 the verdict word; dof:
// what the route counts for the filter.  hasIdle: the route has the idle word -- such a filter reads as an applied update of no rows
// (zeros, info 0); on a route without it the word passes like any other that did not solve (NaNs).
struct UpdateReport {
    double nis, logdet_S, loglik;
    int dof, info;
};
inline UpdateReport updateReport(const double* rec, int dof, bool hasIdle) {
    const int word = int(rec[3]);
    const bool solved = updateSolved(word), idle = hasIdle && word == kWordIdle;
    const double none = idle ? 0.0 : std::nan("");
    return UpdateReport{solved ? rec[0] : none, solved ? rec[1] : none, solved ? rec[2] : none, dof, mergeInfo(idle ? 0 : word)};
}

}  // namespace eqf::lift
