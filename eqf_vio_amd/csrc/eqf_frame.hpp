// Landmark bookkeeping of a vision frame: the index arithmetic of eqf_capi.hip's visionCore / resolveGate, and nothing else -- which state
// landmarks survive, the measurement permutation, which measurement entries become landmarks, what the outlier gate removed on each of its
// three routes.  Host only, standard library only (no HIP, no other eqf_*.hpp; thresholds arrive as arguments): tests/frame_host_main.cpp
// runs it under the sanitizers without a GPU.  Nothing here allocates per landmark; a vector per filter at the most, as the code it came from.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

namespace eqf::frame {

using Lists = std::vector<std::vector<int>>;   // one int list per filter
using Marks = std::vector<std::vector<char>>;  // one mask per filter

// the measurement of a frame: ids[b][0 .. n[b]) strictly ascending; active[b] = filter b takes part (integrated up to the stamp, initialised)
struct Meas {
    const std::vector<const int*>& ids;
    const std::vector<int>& n;
    const std::vector<char>& active;
    bool has(size_t b, int id) const { return std::binary_search(ids[b], ids[b] + n[b], id); }
    int index(size_t b, int id) const { return int(std::lower_bound(ids[b], ids[b] + n[b], id) - ids[b]); }
};

// removeOldLandmarks (VIOFilter.cpp:393-419): keep[b] = indices of the state ids present in the measurement, ascending (all of them for an
// inactive filter).  True if any filter lost a landmark.
inline bool keepPresent(const Lists& ids, const Meas& m, Lists& keep) {
    bool anyLost = false;
    keep.assign(ids.size(), {});
    for (size_t b = 0; b < ids.size(); ++b) {
        keep[b].reserve(ids[b].size());
        for (size_t i = 0; i < ids[b].size(); ++i)
            if (!m.active[b] || m.has(b, ids[b][i])) keep[b].push_back(int(i));
        if (keep[b].size() != ids[b].size()) anyLost = true;
    }
    return anyLost;
}

// ids <- ids[keep] (keep[b] ascending: in place)
inline void applyKeep(Lists& ids, const Lists& keep) {
    for (size_t b = 0; b < ids.size(); ++b) {
        size_t j = 0;
        for (int o : keep[b]) ids[b][j++] = ids[b][o];
        ids[b].resize(j);
    }
}

// matchMeasurementsToState (:211-230): perm[b][i] = measurement index of state landmark i; -1 throughout an inactive filter
inline void matchPerm(const Lists& ids, const Meas& m, Lists& perm) {
    perm.resize(ids.size());
    for (size_t b = 0; b < ids.size(); ++b) {
        perm[b].assign(ids[b].size(), -1);
        if (!m.active[b]) continue;
        for (size_t i = 0; i < ids[b].size(); ++i) perm[b][i] = m.index(b, ids[b][i]);
    }
}

// f(k) for the measurement entries k of 0 .. nb-1, ascending, that perm[0 .. n) does not name and `dropped` (may be null) does not mark.
// perm is read completely before the first call: f may write behind perm + n
template <typename F>
void forUnmatched(const int* perm, int n, int nb, const char* dropped, F&& f) {
    std::vector<char> used(nb, 0);
    for (int i = 0; i < n; ++i)
        if (perm[i] >= 0 && perm[i] < nb) used[perm[i]] = 1;
    for (int k = 0; k < nb; ++k)
        if (!used[k] && !(dropped && dropped[k])) f(k);
}

// is every perm[b][i] == i?  With `active`, only in the filters it marks
inline bool isIdentity(const Lists& perm, const std::vector<char>* active = nullptr) {
    for (size_t b = 0; b < perm.size(); ++b) {
        if (active && !(*active)[b]) continue;
        for (size_t i = 0; i < perm[b].size(); ++i)
            if (perm[b][i] != int(i)) return false;
    }
    return true;
}

// May k_edit take the frame (`ok` comes in as what the handle allows)?  Not with a filter beyond editMax landmarks, nor -- gate armed -- with
// an active one below editSafeN measurement entries (kept + new landmarks = the measurement's entries).  anyFresh: some active filter gains a
// landmark (every kept id is in the measurement); only meaningful with ok.
struct EditChoice { bool ok, anyFresh; };
inline EditChoice editEligible(const Lists& ids, const Lists& keep, const Meas& m, bool ok, bool gateArmed, int editMax, int editSafeN) {
    bool anyFresh = false;
    for (size_t b = 0; b < ids.size() && ok; ++b) {
        if (int(ids[b].size()) > editMax) ok = false;
        if (!m.active[b]) continue;
        if (gateArmed && m.n[b] < editSafeN) ok = false;
        if (m.n[b] > int(keep[b].size())) anyFresh = true;
    }
    return {ok, anyFresh};
}

// What a k_edit launch leaves when no outlier is found: the id lists (kept landmarks, then the new ones in measurement order), the kept
// counts, the active filters left without a landmark, whether any active filter has one, and the largest count among those.
struct EditPlan {
    Lists newIds;
    std::vector<int> nKept, skipped;
    bool anyWork = false;
    int Nmax = 0;
};
// The pinned image of a frame: the bearings [B][3][cap] in doubles, and behind them k_edit's image in ints -- [B][cap] keep map | [B][cap]
// permutation | [B][4] counts --, so that one copy brings both; the whole rounded up to doubles.  The edit image alone is what the stream
// API's staging ring and its device copy hold.
struct ImageLayout {
    size_t B, cap;
    size_t bearingStride() const { return 3 * cap; }
    size_t bearingDoubles() const { return bearingStride() * B; }
    size_t offKeep() const { return 0; }
    size_t offPerm() const { return B * cap; }
    size_t offCounts() const { return 2 * B * cap; }
    size_t editInts() const { return offCounts() + 4 * B; }
    size_t offEdit() const { return bearingDoubles(); }  // (in doubles; the ints start there)
    size_t doubles() const { return offEdit() + (editInts() + 1) / 2; }
};
// k_edit's upload image into h (ImageLayout's ints): the keep map and the permutation (kept landmarks, then the new ones), both padded
// with -1, and {nK, nNew, gate, 0} per filter.  False if a measurement exceeds cap (h is then half written).
inline bool editImage(const Lists& ids, const Lists& keep, const Meas& m, bool gateArmed, int cap, int* h, EditPlan& p) {
    const size_t B = ids.size();
    const ImageLayout il{B, size_t(cap)};
    p = EditPlan{};
    p.newIds.resize(B);
    p.nKept.assign(B, 0);
    for (size_t b = 0; b < B; ++b) {
        int *hm = h + il.offKeep() + b * cap, *hp = h + il.offPerm() + b * cap, *hc = h + il.offCounts() + 4 * b;
        const int nK = p.nKept[b] = int(keep[b].size());
        std::copy(keep[b].begin(), keep[b].end(), hm);
        std::fill(hm + nK, hm + cap, -1);
        std::vector<int>& nid = p.newIds[b];
        for (int o : keep[b]) nid.push_back(ids[b][o]);
        int nNew = 0;
        std::fill(hp, hp + cap, -1);
        if (m.active[b]) {
            if (m.n[b] > cap) return false;
            for (int j = 0; j < nK; ++j) hp[j] = m.index(b, nid[j]);
            forUnmatched(hp, nK, m.n[b], nullptr, [&](int k) { hp[nK + nNew++] = k; nid.push_back(m.ids[b][k]); });
        }
        hc[0] = nK; hc[1] = nNew; hc[2] = (gateArmed && m.active[b]) ? 1 : 0; hc[3] = 0;
        if (!m.active[b]) continue;
        if (nid.empty()) {
            p.skipped.push_back(int(b));
            continue;
        }
        p.anyWork = true;
        p.Nmax = std::max(p.Nmax, int(nid.size()));
    }
    return true;
}

// ---- removeOutliers (:429-443), one function per route.  chord[b * cap + i] belongs to state landmark i of filter b.  `x > thr` drops and
// `!(x > thr)` keeps: a NaN chord keeps its landmark.

// The synchronous gate: keep[b] = the landmarks that stay, dropped[b][k] = 1 for the measurement entries of those that go.  True if any goes.
inline bool gateSync(const Lists& ids, const Lists& perm, const std::vector<char>& active, const double* chord, int cap, double thr,
    Lists& keep, Marks& dropped) {
    bool anyOut = false;
    for (size_t b = 0; b < ids.size(); ++b) {
        keep[b].clear();
        for (size_t i = 0; i < ids[b].size(); ++i) {
            if (active[b] && chord[b * cap + i] > thr) {
                anyOut = true;
                dropped[b][perm[b][i]] = 1;
            } else {
                keep[b].push_back(int(i));
            }
        }
    }
    return anyOut;
}

// The host's redo of a frame whose speculative probe raised flag[b]: act[b] = filter b is redone (flagged and active in that frame), and
// flag[b] becomes that mask.  False if none is; otherwise keep[b] = everything for the others, and for those the first nOld[b] landmarks
// minus the outliers (the frame's appended landmarks go too: the redo adds them again), gated[b][k] = 1 for the outliers' measurement entries.
inline bool gateRedo(const Lists& ids, int* flag, const std::vector<char>& active, const Lists& measIds, const std::vector<int>& nb,
    const std::vector<int>& nOld, const double* chord, int cap, double thr, std::vector<char>& act, Lists& keep, Marks& gated) {
    const size_t B = ids.size();
    bool any = false;
    act.assign(B, 0);
    for (size_t b = 0; b < B; ++b) {
        act[b] = flag[b] && active[b];
        flag[b] = act[b];
        any = any || act[b];
    }
    if (!any) return false;
    keep.assign(B, {});
    gated.assign(B, {});
    for (size_t b = 0; b < B; ++b) {
        const int n = int(ids[b].size());
        const int* mi = measIds[b].data();
        gated[b].assign(nb[b], 0);
        if (!act[b]) {
            for (int i = 0; i < n; ++i) keep[b].push_back(i);
            continue;
        }
        for (int i = 0; i < std::min(n, nOld[b]); ++i) {
            if (chord[b * cap + i] > thr) gated[b][std::lower_bound(mi, mi + nb[b], ids[b][i]) - mi] = 1;
            else keep[b].push_back(i);
        }
    }
    return true;
}

// The device route: k_edit took the outliers out itself.  In the filters it flagged (and that were active) the ids follow -- of the first
// nKept[b], those whose chord passes; the new ones behind them all stay.  Flag 2: the filter became so small that k_edit switched the queued
// update off; flag[b] becomes 1 for those that still have a landmark (their update runs now, shaped for Nmax) and 0 for the rest.
struct DeviceGate { bool deferred; int Nmax; };
inline DeviceGate gateOnDevice(Lists& ids, int* flag, const std::vector<char>& active, const std::vector<int>& nKept, const double* chord,
    int cap, double thr) {
    DeviceGate d{false, 0};
    for (size_t b = 0; b < ids.size(); ++b) {
        if (flag[b] && active[b]) {
            size_t n = 0;
            for (size_t j = 0; j < ids[b].size(); ++j)
                if (int(j) >= nKept[b] || !(chord[b * cap + j] > thr)) ids[b][n++] = ids[b][j];
            ids[b].resize(n);
        }
        const bool late = flag[b] == 2 && active[b] && !ids[b].empty();
        flag[b] = late ? 1 : 0;
        if (!late) continue;
        d.deferred = true;
        d.Nmax = std::max(d.Nmax, int(ids[b].size()));
    }
    return d;
}

}  // namespace eqf::frame
