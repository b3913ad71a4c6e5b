// Explicit landmark removal and insertion with priors (eqf_edit_landmarks): everything the HOST decides -- the argument checks, the verdict of
// every named id, the keep map, the id lists the handle holds afterwards, the 3 x 3 Cholesky that accepts or rejects a prior, whether
// anything is removed at all (the launch that moves Sigma) and the image the kernels of eqf_mapedit.hpp read.  Host only, standard library
// only (no HIP, no other eqf_*.hpp): tests/mapedit_host_main.cpp runs it under the sanitizers without a GPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

namespace eqf::mapedit {

using Lists = std::vector<std::vector<int>>;  // one int list per filter

constexpr int kOk = 0, kInvalid = -1, kCapacity = -4, kUnsorted = -5;  // EQF_OK, EQF_ERR_INVALID, EQF_ERR_CAPACITY, EQF_ERR_UNSORTED
constexpr int kPrior = 12;                                             // doubles per accepted insertion in the image: p (3), P mirrored (9)
constexpr unsigned char kDone = 1, kAbsent = 0, kPresent = 0, kRejected = 2;

// the caller's arrays as the C ABI has them
struct Args {
    const int* nRemove;    // [B] or null: nothing is removed
    const int* removeIds;  // [B][rstride]
    int rstride;
    const int* nInsert;    // [B] or null: nothing is inserted
    const int* insertIds;  // [B][istride]
    int istride;
    const double* p;       // [B][istride][3]
    const double* P;       // [B][istride][3][3], lower triangles read
};

// Is the prior usable?  Every entry of p and of P's lower triangle finite, p not the zero vector, and the three pivots of the Cholesky
// factorisation of the lower triangle positive (`!(x > 0)` rejects: a pivot that overflowed into NaN does not pass).  The upper triangle
// is never read.
inline bool priorOk(const double* p, const double* P) {
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(p[c])) return false;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c <= r; ++c)
            if (!std::isfinite(P[3 * r + c])) return false;
    if (p[0] == 0.0 && p[1] == 0.0 && p[2] == 0.0) return false;
    const double d0 = P[0];
    if (!(d0 > 0.0)) return false;
    const double l00 = std::sqrt(d0), l10 = P[3] / l00, l20 = P[6] / l00;
    const double d1 = P[4] - l10 * l10;
    if (!(d1 > 0.0)) return false;
    const double l11 = std::sqrt(d1), l21 = (P[7] - l20 * l10) / l11;
    const double d2 = P[8] - l20 * l20 - l21 * l21;
    return d2 > 0.0;
}

// What a call does, decided before anything is enqueued.
struct Plan {
    std::vector<unsigned char> removed;   // [B][rstride]: 1 gone, 0 not in the state
    std::vector<unsigned char> inserted;  // [B][istride]: 1 done, 0 already in the state after the removals, 2 values rejected
    Lists keep;                           // old indices that stay, ascending (the identity for a filter that loses nothing)
    Lists accepted;                       // positions k of the insert list that come in, ascending
    Lists newIds;                         // the filter's ids afterwards: the kept ones in their order, then the accepted ones
    bool anyRemoved = false;              // some filter loses a landmark: Sigma changes buffers for the whole batch
    bool anyInserted = false;
    int maxNew = 0, maxN = 0;             // largest accepted count / final count of a filter
};

// The checks and the verdicts.  ids[b]: what the handle holds (any order, no duplicates).  Returns kOk, or -- with `plan` half written and
// nothing to be done -- kInvalid (a count outside [0, stride], a list that is not empty but null, a negative stride), kUnsorted (a list not
// strictly ascending), kCapacity (kept + accepted beyond cap in some filter: only accepted entries count).  An id that is still in the
// state after the removals gets verdict 0 whatever its values are; the values of the others decide between 1 and 2.
inline int plan(const Lists& ids, int cap, const Args& a, Plan& pl) {
    const size_t B = ids.size();
    pl = Plan{};
    if (a.rstride < 0 || a.istride < 0) return kInvalid;
    for (size_t b = 0; b < B; ++b) {
        const int nr = a.nRemove ? a.nRemove[b] : 0, ni = a.nInsert ? a.nInsert[b] : 0;
        if (nr < 0 || nr > a.rstride || ni < 0 || ni > a.istride) return kInvalid;
        if (nr > 0 && !a.removeIds) return kInvalid;
        if (ni > 0 && (!a.insertIds || !a.p || !a.P)) return kInvalid;
    }
    for (size_t b = 0; b < B; ++b) {
        const int nr = a.nRemove ? a.nRemove[b] : 0, ni = a.nInsert ? a.nInsert[b] : 0;
        for (int k = 1; k < nr; ++k)
            if (a.removeIds[b * a.rstride + k] <= a.removeIds[b * a.rstride + k - 1]) return kUnsorted;
        for (int k = 1; k < ni; ++k)
            if (a.insertIds[b * a.istride + k] <= a.insertIds[b * a.istride + k - 1]) return kUnsorted;
    }
    pl.removed.assign(B * size_t(a.rstride), 0);
    pl.inserted.assign(B * size_t(a.istride), 0);
    pl.keep.assign(B, {});
    pl.accepted.assign(B, {});
    pl.newIds.assign(B, {});
    for (size_t b = 0; b < B; ++b) {
        const int nr = a.nRemove ? a.nRemove[b] : 0, ni = a.nInsert ? a.nInsert[b] : 0;
        const int* rid = nr ? a.removeIds + b * a.rstride : nullptr;
        const int* iid = ni ? a.insertIds + b * a.istride : nullptr;
        std::vector<int>& keep = pl.keep[b];
        std::vector<int>& nid = pl.newIds[b];
        keep.reserve(ids[b].size());
        for (size_t i = 0; i < ids[b].size(); ++i) {
            const int* hit = nr ? std::lower_bound(rid, rid + nr, ids[b][i]) : nullptr;
            if (hit && hit != rid + nr && *hit == ids[b][i]) {
                pl.removed[b * a.rstride + size_t(hit - rid)] = 1;
            } else {
                keep.push_back(int(i));
                nid.push_back(ids[b][i]);
            }
        }
        if (keep.size() != ids[b].size()) pl.anyRemoved = true;
        std::vector<int> left(nid);  // the ids after the removals, sorted for the look-up
        std::sort(left.begin(), left.end());
        for (int k = 0; k < ni; ++k) {
            unsigned char& v = pl.inserted[b * a.istride + k];
            if (std::binary_search(left.begin(), left.end(), iid[k])) {
                v = kPresent;
            } else if (!priorOk(a.p + (b * a.istride + k) * 3, a.P + (b * a.istride + k) * 9)) {
                v = kRejected;
            } else {
                v = kDone;
                pl.accepted[b].push_back(k);
                nid.push_back(iid[k]);
            }
        }
        if (nid.size() > size_t(cap)) return kCapacity;
        if (!pl.accepted[b].empty()) pl.anyInserted = true;
        pl.maxNew = std::max(pl.maxNew, int(pl.accepted[b].size()));
        pl.maxN = std::max(pl.maxN, int(nid.size()));
    }
    return kOk;
}

// The image the kernels read, for a call planned by plan():
//   doubles [B][ns][kPrior]   the accepted insertions of filter b in their order: p, then P's lower triangle mirrored, row-major
//   ints    [B][4]            {kept count, accepted count, count before the call, 0}
//   ints    [B][cap]          the keep map, padded with -1 -- only when something is removed (the insert-only launch does not read it)
// with ns = max(1, maxNew).
struct Image {
    size_t B = 0, cap = 0, ns = 1;
    bool withMap = false;
    size_t offPrior() const { return 0; }
    size_t offCounts() const { return sizeof(double) * B * ns * kPrior; }
    size_t offMap() const { return offCounts() + sizeof(int) * 4 * B; }
    size_t bytes() const { return offMap() + (withMap ? sizeof(int) * B * cap : 0); }
};
inline Image imageLayout(size_t B, int cap, const Plan& pl) { return Image{B, size_t(cap), size_t(std::max(1, pl.maxNew)), pl.anyRemoved}; }
// the most a call on a handle of this shape can ask for
inline size_t imageCapacityBytes(size_t B, int cap) { return sizeof(double) * B * size_t(std::max(1, cap)) * kPrior + sizeof(int) * B * (4 + size_t(cap)); }

inline void fillImage(const Lists& ids, const Args& a, const Plan& pl, const Image& im, char* h) {
    double* pr = reinterpret_cast<double*>(h + im.offPrior());
    int* cnt = reinterpret_cast<int*>(h + im.offCounts());
    int* map = reinterpret_cast<int*>(h + im.offMap());
    for (size_t b = 0; b < im.B; ++b) {
        double* d = pr + b * im.ns * kPrior;
        std::fill(d, d + im.ns * kPrior, 0.0);
        for (size_t j = 0; j < pl.accepted[b].size(); ++j) {
            const size_t e = b * a.istride + size_t(pl.accepted[b][j]);
            const double *p = a.p + 3 * e, *P = a.P + 9 * e;
            double* o = d + j * kPrior;
            for (int c = 0; c < 3; ++c) o[c] = p[c];
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) o[3 + 3 * r + c] = r >= c ? P[3 * r + c] : P[3 * c + r];
        }
        cnt[4 * b] = int(pl.keep[b].size());
        cnt[4 * b + 1] = int(pl.accepted[b].size());
        cnt[4 * b + 2] = int(ids[b].size());
        cnt[4 * b + 3] = 0;
        if (im.withMap) {
            std::copy(pl.keep[b].begin(), pl.keep[b].end(), map + b * im.cap);
            std::fill(map + b * im.cap + pl.keep[b].size(), map + (b + 1) * im.cap, -1);
        }
    }
}

}  // namespace eqf::mapedit
