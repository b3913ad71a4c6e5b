// The host's decisions of eqf_copy_filters: what makes a call EQF_ERR_INVALID or EQF_ERR_CAPACITY, which pairs move something, which
// sources of an in-place copy are read from the staging image, and the layout of that image with the per-filter counts of the small state
// it repeats.  Host only, standard library only (no HIP, no other eqf_*.hpp; the layout constants, the pair table and the error codes are
// repeated here and static_assert-ed where both are seen): tests/clone_host_main.cpp runs it under the sanitizers without a GPU.
#pragma once
#include <cstddef>
#include <vector>

namespace eqf::clone {

constexpr int kPadBase = 12;  // padded base coordinates (kLm0)
constexpr int kOk = 0, kInvalid = -1, kCapacity = -4;

struct Pair {  // (eqf_clone.hpp's ClonePair)
    int dst, src, N, fromStage;
};

// The small state of a handle of B filters of capacity cap: doubles per filter of its six arrays (eqf_create allocates them, CloneSide
// names them), and the staging image of the in-place case, in bytes: Glob [B] of globBytes each | p0 | Q | delta | gamma | gammaTot |
// innov, every one [B][its count] doubles.
struct SmallLayout {
    size_t B, cap, globBytes, innovHead;
    size_t p0Count() const { return 3 * cap; }
    size_t qCount() const { return 5 * cap; }
    size_t deltaCount() const { return 2 * cap; }
    size_t gammaCount() const { return size_t(kPadBase) + 3 * cap; }
    size_t gammaTotCount() const { return 9 + 3 * cap; }
    size_t innovCount() const { return innovHead + cap; }
    size_t offGlob() const { return 0; }
    size_t offP0() const { return globBytes * B; }
    size_t offQ() const { return offP0() + sizeof(double) * p0Count() * B; }
    size_t offDelta() const { return offQ() + sizeof(double) * qCount() * B; }
    size_t offGamma() const { return offDelta() + sizeof(double) * deltaCount() * B; }
    size_t offGammaTot() const { return offGamma() + sizeof(double) * gammaCount() * B; }
    size_t offInnov() const { return offGammaTot() + sizeof(double) * gammaTotCount() * B; }
    size_t bytes() const { return offInnov() + sizeof(double) * innovCount() * B; }
};

// What can be checked before the landmark counts are settled: every index in its handle's range, no dst named twice.
inline int headCheck(int dstB, int srcB, int n, const int* dst_idx, const int* src_idx) {
    if (n < 0 || dstB < 0 || srcB < 0 || (n > 0 && (!dst_idx || !src_idx))) return kInvalid;
    std::vector<char> named(size_t(dstB), 0);
    for (int k = 0; k < n; ++k) {
        if (dst_idx[k] < 0 || dst_idx[k] >= dstB || src_idx[k] < 0 || src_idx[k] >= srcB) return kInvalid;
        if (named[size_t(dst_idx[k])]) return kInvalid;
        named[size_t(dst_idx[k])] = 1;
    }
    return kOk;
}

// The plan of a call (srcN: [srcB] landmark counts of the source handle; inPlace: dst and src are one handle): headCheck, then
// EQF_ERR_CAPACITY for a source that does not fit dstCap.  pairs: the pairs that move something, in the caller's order (in place an
// identity pair moves nothing).  In place, a source that is also somebody's destination is read from the staging image (fromStage = 1);
// stagePairs brings it there, once however many pairs read it.  nMaxN: most landmarks of a moved source.
inline int plan(int dstB, int srcB, int dstCap, bool inPlace, int n, const int* dst_idx, const int* src_idx, const int* srcN,
    std::vector<Pair>& pairs, std::vector<Pair>& stagePairs, int& nMaxN) {
    pairs.clear();
    stagePairs.clear();
    nMaxN = 0;
    const int rc = headCheck(dstB, srcB, n, dst_idx, src_idx);
    if (rc) return rc;
    std::vector<char> isDst(inPlace ? size_t(dstB) : 0, 0);
    for (int k = 0; k < n; ++k) {
        if (inPlace && dst_idx[k] == src_idx[k]) continue;
        if (srcN[src_idx[k]] > dstCap) return kCapacity;
        if (inPlace) isDst[size_t(dst_idx[k])] = 1;
    }
    for (int k = 0; k < n; ++k) {
        if (inPlace && dst_idx[k] == src_idx[k]) continue;
        const int s = src_idx[k], N = srcN[s];
        const int staged = inPlace && isDst[size_t(s)] ? 1 : 0;
        if (staged == 1 && isDst[size_t(s)] == 1) {
            stagePairs.push_back(Pair{s, s, N, 0});
            isDst[size_t(s)] = 2;  // (staged once, however many pairs read it)
        }
        pairs.push_back(Pair{dst_idx[k], s, N, staged});
        if (N > nMaxN) nMaxN = N;
    }
    return kOk;
}

}  // namespace eqf::clone
