// Argument checks, weight normalisation, member tables and index arithmetic of the moment-matched mixture (eqf_get_mixture_moments,
// eqf_merge_filters): what makes a call EQF_ERR_INVALID, the normalised weights the device sees, the table of members it walks, the layout
// of the workspace and the launch grid of k_mix_reduce.  Host only, standard library only (no HIP, no other eqf_*.hpp; the layout constants
// are repeated here and static_assert-ed against eqf_device.hpp / eqf_mixture.hpp where both are seen): tests/mixture_host_main.cpp runs it
// under the sanitizers without a GPU.
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

namespace eqf::mixture {

constexpr int kRefBase = 11;   // reference base coordinates (kBase)
constexpr int kPadBase = 12;   // ... padded (kLm0): internal index 11 is the structural pad
constexpr int kRows = 4;       // row landmarks of a tile of k_mix_reduce (kMixRows)
constexpr int kLanes = 64;     // column landmarks of a tile: one per lane of its one wavefront (kMixLanes)
constexpr int kEstHead = 20;   // head of a filter's estimate image (kMixEstHead)

inline int refOrder(int N) { return kRefBase + 3 * N; }
inline int paddedOrder(int N) { return kPadBase + 3 * N; }
inline int refToPadded(int i) { return i < kRefBase ? i : i + 1; }

// launch grid of k_mix_reduce: x = chunks of kLanes column landmarks, y = blocks of kRows row landmarks (one each for N = 0: the base block)
inline int chunks(int N) { return N > 0 ? (N + kLanes - 1) / kLanes : 1; }
inline int rowBlocks(int N) { return N > 0 ? (N + kRows - 1) / kRows : 1; }
// one member as the device walks it: the filter and its normalised weight
struct Member {
    int b, pad_;
    double w;
};

// What can be checked without the handle's landmark lists: pointers, counts, index ranges, ref among idx, the weights.
inline bool headArgsOk(int n, const int* idx, const double* w, int ref, int B) {
    if (n < 1 || !idx || !w || B < 1 || ref < 0 || ref >= B) return false;
    bool found = false;
    double s = 0.0;
    for (int k = 0; k < n; ++k) {
        if (idx[k] < 0 || idx[k] >= B) return false;
        if (!std::isfinite(w[k]) || w[k] < 0.0) return false;
        found = found || idx[k] == ref;
        s += w[k];
    }
    return found && std::isfinite(s) && s > 0.0;
}

// same landmark count, same ids in the same order
inline bool sameIds(const int* a, int na, const int* b, int nb) {
    if (na != nb) return false;
    for (int i = 0; i < na; ++i)
        if (a[i] != b[i]) return false;
    return true;
}

// w~_k = w_k / s with s the serial sum in the order given; returns n_eff = 1 / sum w~^2 (serial as well)
inline double normalise(int n, const double* w, double* wt) {
    double s = 0.0;
    for (int k = 0; k < n; ++k) s += w[k];
    double q = 0.0;
    for (int k = 0; k < n; ++k) {
        wt[k] = w[k] / s;
        q += wt[k] * wt[k];
    }
    return 1.0 / q;
}

// The tables of a call: the members of non-zero weight in the order of idx (a member of weight 0 contributes nothing and is not walked:
// it cannot change a bit), and the distinct filters whose images the per-member kernels build -- those members' and always ref's.
inline void buildTables(int n, const int* idx, const double* wt, int ref, int B, std::vector<Member>& members, std::vector<int>& uniq) {
    members.clear();
    uniq.clear();
    std::vector<char> seen(size_t(B), 0);
    seen[size_t(ref)] = 1;
    uniq.push_back(ref);
    for (int k = 0; k < n; ++k) {
        if (!(wt[k] > 0.0)) continue;
        members.push_back(Member{idx[k], 0, wt[k]});
        if (!seen[size_t(idx[k])]) {
            seen[size_t(idx[k])] = 1;
            uniq.push_back(idx[k]);
        }
    }
}

// The workspace of a handle, in doubles: J' records [B][jacStride] | estimate images [B + 1][estStride] (slot B: the merged state) | errors
// [B][ld] | mean [ld] | out [4] (spread trace, total trace) | staged origin landmarks [3][cap] | staged Q [5][cap] | staged Glob (globWords)
// | verdict words (4 ints in 2 doubles)
struct WorkLayout {
    int B, cap, ld, globWords;
    size_t jacStride() const { return 16 + size_t(9) * cap; }
    size_t estStride() const { return kEstHead + size_t(3) * cap; }
    size_t offJac() const { return 0; }
    size_t offEst() const { return offJac() + jacStride() * B; }
    size_t offErr() const { return offEst() + estStride() * (size_t(B) + 1); }
    size_t offMean() const { return offErr() + size_t(ld) * B; }
    size_t offOut() const { return offMean() + size_t(ld); }
    size_t offP0() const { return offOut() + 4; }
    size_t offQ() const { return offP0() + size_t(3) * cap; }
    size_t offGlob() const { return offQ() + size_t(5) * cap; }
    size_t offVerdict() const { return offGlob() + size_t(globWords); }
    size_t doubles() const { return offVerdict() + 2; }
};

}  // namespace eqf::mixture
