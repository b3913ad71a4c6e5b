// What the HOST decides for the Schmidt (consider) updates eqf_update_linear_schmidt / eqf_update_landmarks_schmidt (kernels:
// eqf_schmidt.hpp): the checks of the consider lists, the partition of a filter's padded indices into active and consider ones, the image
// the kernels read, the tile arithmetic of the gathered downdate (with the ownership rule, so that a test can count owners) and the
// counted-bytes model.  Host only, standard library only (no HIP, no other eqf_*.hpp): tests/schmidt_host_main.cpp runs it under the
// sanitizers without a GPU.
//
// The consider set C of a filter is a set of its landmarks, c their 3 |C| padded indices.  Every other padded index is ACTIVE: the base
// block 0..10, the pad index 11 and the other landmarks.  The update keeps Sigma_cc and the estimate of C; everything else is the full
// update's.
#pragma once
#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

namespace eqf::schmidt {

constexpr int kOk = 0, kInvalid = -1, kCapacity = -4, kUnsorted = -5;  // EQF_OK, EQF_ERR_INVALID, EQF_ERR_CAPACITY, EQF_ERR_UNSORTED
constexpr int kPadBase = 12;  // eqf_device.hpp's kLm0: landmark i sits at padded indices 12 + 3 i ..
constexpr int kTile = 64;     // eqf_chol64.hpp's kSB

inline int paddedOrder(int N) { return kPadBase + 3 * N; }
inline int tiles(int x) { return (x + kTile - 1) / kTile; }

// The caller's lists before any effect.  nConsider == nullptr: empty sets, nothing else is looked at.  Precedence over the batch:
// kInvalid (a negative count or stride, a list that is not empty but null), kCapacity (a count beyond the handle's capacity or beyond
// cstride), kUnsorted (a list not strictly ascending).
inline int checkLists(int B, int cap, const int* nConsider, const int* considerIds, int cstride) {
    if (!nConsider) return kOk;
    if (cstride < 0) return kInvalid;
    for (int b = 0; b < B; ++b) {
        if (nConsider[b] < 0) return kInvalid;
        if (nConsider[b] > 0 && !considerIds) return kInvalid;
    }
    for (int b = 0; b < B; ++b)
        if (nConsider[b] > cap || nConsider[b] > cstride) return kCapacity;
    for (int b = 0; b < B; ++b)
        for (int k = 1; k < nConsider[b]; ++k)
            if (considerIds[size_t(b) * cstride + k] <= considerIds[size_t(b) * cstride + k - 1]) return kUnsorted;
    return kOk;
}

// The partition of one filter.  ids: the N landmark ids the state holds, in the state's order (any order, no duplicates); considerIds:
// nConsider ids, strictly ascending; one the state does not hold is ignored.  activeIdx: the active padded indices, ascending (0..11, then
// three per active landmark); isConsider: one byte per padded index, 12 + 3 N of them.  Returns the number of consider landmarks found.
inline int buildActive(int N, const int* ids, int nConsider, const int* considerIds, std::vector<int>& activeIdx,
    std::vector<unsigned char>& isConsider) {
    const int n = paddedOrder(N);
    isConsider.assign(size_t(n), 0);
    activeIdx.clear();
    activeIdx.reserve(size_t(n));
    int found = 0;
    // (a state whose ids ascend -- the usual one -- is merged against the list in one pass; an id below its predecessor starts a search)
    const int* const end = considerIds + (nConsider > 0 ? nConsider : 0);
    const int* hit = considerIds;
    for (int i = 0; i < N && nConsider > 0; ++i) {
        if (i > 0 && ids[i] < ids[i - 1]) {
            hit = std::lower_bound(considerIds, end, ids[i]);
        } else {
            while (hit != end && *hit < ids[i]) ++hit;
        }
        if (hit != end && *hit == ids[i]) {
            for (int c = 0; c < 3; ++c) isConsider[size_t(kPadBase + 3 * i + c)] = 1;
            ++found;
        }
    }
    for (int i = 0; i < n; ++i)
        if (!isConsider[size_t(i)]) activeIdx.push_back(i);
    return found;
}

// ---- the image the kernels read: per filter one int record {nA, 0} ... then the lists, all with one pitch ----------------------------------
//   ints  [B][2]        {number of active indices, 0}
//   ints  [B][pitch]    activeIdx, padded with -1
//   bytes [B][pitch]    isConsider, padded with 0
// pitch = the handle's leading dimension ld (>= 12 + 3 cap): one size for the life of the handle.
struct Image {
    size_t B = 0, pitch = 0;
    size_t offCount() const { return 0; }
    size_t offActive() const { return sizeof(int) * 2 * B; }
    size_t offFlag() const { return offActive() + sizeof(int) * B * pitch; }
    size_t bytes() const { return offFlag() + B * pitch; }
};
inline void fillFilter(const Image& im, size_t b, const std::vector<int>& activeIdx, const std::vector<unsigned char>& isConsider, char* h) {
    int* cnt = reinterpret_cast<int*>(h + im.offCount()) + 2 * b;
    int* act = reinterpret_cast<int*>(h + im.offActive()) + b * im.pitch;
    unsigned char* fl = reinterpret_cast<unsigned char*>(h + im.offFlag()) + b * im.pitch;
    cnt[0] = int(activeIdx.size());
    cnt[1] = 0;
    std::copy(activeIdx.begin(), activeIdx.end(), act);
    std::fill(act + activeIdx.size(), act + im.pitch, -1);
    std::copy(isConsider.begin(), isConsider.end(), fl);
    std::fill(fl + isConsider.size(), fl + im.pitch, (unsigned char)0);
}

// ---- the gathered downdate's launch --------------------------------------------------------------------------------------------------------
// grid.x = rowTiles(nAmax) * colTiles(nMax); workgroup t of filter b: P = t / colTiles, J = t % colTiles; it holds the 64 active rows
// activeIdx[64 P ..] and the 64 contiguous columns 64 J ..
inline int rowTiles(int nAmax) { return std::max(tiles(nAmax), 1); }
inline int colTiles(int nMax) { return tiles(nMax); }
inline int gridX(int nAmax, int nMax) { return rowTiles(nAmax) * colTiles(nMax); }
// Is entry (a, j), a an active index, computed -- and written, with its mirror -- by the workgroup that holds row a and column j?
// (the one rule of eqf_schmidt.hpp's k_schmidt_downdate)
inline bool owns(int a, int j, const unsigned char* isConsider) { return isConsider[j] || j <= a; }

// counted bytes of the downdate: every entry outside c x c read once and written once
inline double countedBytes(int n, int nc) { return 16.0 * (double(n) * n - double(nc) * nc); }

}  // namespace eqf::schmidt
