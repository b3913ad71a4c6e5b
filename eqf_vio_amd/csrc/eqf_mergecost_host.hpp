// Argument checks, pair canonicalisation and enumeration, the chunk plan, the layouts of the two device blocks and the two cost formulas of
// eqf_get_merge_costs.  Host only,
// standard library only (no HIP, no other eqf_*.hpp; the constants repeated here are static_assert-ed against eqf_device.hpp /
// eqf_mergecost.hpp where both are seen): tests/mergecost_host_main.cpp runs it under the sanitizers without a GPU.  The cost formulas are
// __host__ __device__ where a HIP compiler sees them: k_pair_tail evaluates the same text.
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

#if defined(__HIPCC__)
#define EQF_MC_HD __host__ __device__
#else
#define EQF_MC_HD
#endif

namespace eqf::mergecost {

constexpr int kRunnalls = 0;       // EQF_COST_RUNNALLS
constexpr int kBhattacharyya = 1;  // EQF_COST_BHATTACHARYYA
constexpr int kRefBase = 11;       // reference base coordinates (kBase)
constexpr int kPadBase = 12;       // ... padded (kLm0)
constexpr int kBlock = 64;         // block column of the factorisation (kSB)
constexpr int kChunkMax = 4096;    // upper end of the option "merge_cost_chunk"
constexpr int kRec = 8;            // doubles of an item's record on the device (kPairRec)

// One image that is factored: a member by itself (self = 1, i == j: a plain copy) or SigmaBar of the pair of POSITIONS i < j.
struct Item {
    int i, j;      // positions in idx
    int bi, bj;    // their filters
    int self, pad_;
    double alpha;  // w~_j / (w~_i + w~_j); 1/2 where both weights are 0 and for the Bhattacharyya cost
    double wi, wj;
};

inline bool kindOk(int kind) { return kind == kRunnalls || kind == kBhattacharyya; }
inline bool firstOk(int first) { return first == 0 || first == 6 || first == kRefBase; }
inline int offsetOf(int first) { return first == kRefBase ? kPadBase : first; }
inline int paddedOrder(int N, int off) { return kPadBase + 3 * N - off; }
inline int blockColumns(int m) { return (m + kBlock - 1) / kBlock; }
inline long long allPairs(int n) { return (long long)n * (n - 1) / 2; }

// What is checked beyond eqf_get_mixture_moments' own head checks: kind, first, the pair list.
inline bool pairArgsOk(int n, int kind, int first, int npairs, const int* pairs) {
    if (n < 1 || !kindOk(kind) || !firstOk(first) || npairs < 0) return false;
    if (!pairs) return (long long)npairs <= allPairs(n);  // (the first npairs of the enumeration)
    for (int p = 0; p < npairs; ++p) {
        const int i = pairs[2 * p], j = pairs[2 * p + 1];
        if (i < 0 || i >= n || j < 0 || j >= n) return false;
    }
    return true;
}

// the p-th pair of all i < j in lexicographic order
inline void lexPair(int n, long long p, int* i, int* j) {
    int a = 0;
    while (p >= n - 1 - a) {
        p -= n - 1 - a;
        ++a;
    }
    *i = a;
    *j = a + 1 + int(p);
}

EQF_MC_HD inline double alphaOf(int kind, double wi, double wj) {
    if (kind == kBhattacharyya || !(wi + wj > 0.0)) return 0.5;
    return wj / (wi + wj);
}

// The images of a call in the order they are factored: the n members by position, then the pairs as given, each ordered so that i < j
// (a pair (i, i) is the member's own image: alpha SigmaBar = Sigma'_i + alpha 0).
inline void buildItems(int n, const int* idx, const double* wt, int kind, int npairs, const int* pairs, std::vector<Item>& items) {
    items.clear();
    items.reserve(size_t(n) + size_t(npairs));
    for (int k = 0; k < n; ++k) items.push_back(Item{k, k, idx[k], idx[k], 1, 0, 0.5, wt[k], wt[k]});
    for (int p = 0; p < npairs; ++p) {
        int i, j;
        if (pairs) {
            i = pairs[2 * p];
            j = pairs[2 * p + 1];
        } else {
            lexPair(n, p, &i, &j);
        }
        if (i > j) {
            const int t = i;
            i = j;
            j = t;
        }
        items.push_back(Item{i, j, idx[i], idx[j], 0, 0, alphaOf(kind, wt[i], wt[j]), wt[i], wt[j]});
    }
}

// the distinct filters among idx, in the order of first appearance
inline void distinct(int n, const int* idx, int B, std::vector<int>& uniq) {
    uniq.clear();
    std::vector<char> seen(size_t(B), 0);
    for (int k = 0; k < n; ++k)
        if (!seen[size_t(idx[k])]) {
            seen[size_t(idx[k])] = 1;
            uniq.push_back(idx[k]);
        }
}

// chunk plan: images [first, first + count) per round of launches
inline int chunkSize(int option, int B) { return option > 0 ? option : (B > 0 ? B : 1); }
inline bool chunkOptionOk(int value) { return value >= 1 && value <= kChunkMax; }
inline int numChunks(long long items, int chunk) { return int((items + chunk - 1) / chunk); }
inline int chunkCount(long long items, int chunk, int c) {
    const long long left = items - (long long)c * chunk;
    return int(left < chunk ? left : chunk);
}
// kernel launches of a call behind the preparation: per chunk k_pair_form, the factorisation's schedule with the right-hand side,
// k_nees_tail and k_pair_tail
inline int launchesPerChunk(int m) {
    const int nb = blockColumns(m);
    int l = 4;  // k_pair_form, k_nees_diag(0), k_nees_tail, k_pair_tail
    for (int K = 0; K < nb; ++K) {
        const int t = nb - K - 1;
        if (K > 0) ++l;
        ++l;  // the panel: the right-hand side's workgroup is always there
        if (t > 0) ++l;
    }
    return l;
}

// The workspace of a chunk of C images, in doubles: W [C][sigmaStride] the images | E [C][nTot] their right-hand sides | D [C][dRec] the
// records of the current diagonal block | out [C][headDoubles] k_nees_tail's records | Glob [C] of globDoubles doubles each | bad [C] ints
// behind them, rounded up to whole doubles.
struct WorkLayout {
    size_t C, sigmaStride, nTot, dRec, headDoubles, globDoubles;
    size_t offW() const { return 0; }
    size_t offE() const { return C * sigmaStride; }
    size_t offD() const { return offE() + C * nTot; }
    size_t offOut() const { return offD() + C * dRec; }
    size_t offGlob() const { return offOut() + C * headDoubles; }
    size_t offBad() const { return offGlob() + C * globDoubles; }  // (in doubles; the ints start there)
    size_t doubles() const { return offBad() + (C + 1) / 2; }
};
// The items of a call and their records [kRec] behind them, in bytes, for a block that holds itemCap of them
struct ItemsLayout {
    size_t itemCap;
    size_t offItems() const { return 0; }
    size_t offRecords() const { return sizeof(Item) * itemCap; }
    size_t bytes() const { return offRecords() + sizeof(double) * kRec * itemCap; }
};

// ---- the costs from (ld_i, ld_j, ld_ij, maha, w~_i, w~_j)
EQF_MC_HD inline double runnalls(double ldi, double ldj, double ldij, double maha, double wi, double wj, double alpha) {
    const double s = wi + wj;
    return 0.5 * (wi * (ldij - ldi) + wj * (ldij - ldj) + s * log1p(alpha * (1.0 - alpha) * maha));
}
EQF_MC_HD inline double bhattacharyya(double ldi, double ldj, double ldij, double maha) {
    return 0.125 * maha + 0.25 * ((ldij - ldi) + (ldij - ldj));
}
EQF_MC_HD inline double cost(int kind, double ldi, double ldj, double ldij, double maha, double wi, double wj, double alpha) {
    return kind == kBhattacharyya ? bhattacharyya(ldi, ldj, ldij, maha) : runnalls(ldi, ldj, ldij, maha, wi, wj, alpha);
}

}  // namespace eqf::mergecost
