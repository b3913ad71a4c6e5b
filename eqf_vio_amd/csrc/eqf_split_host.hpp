// The host's decisions of eqf_split_filters: what makes a call EQF_ERR_INVALID, the dst/src rule, the grouping of the children by source
// and the plan image the kernels of eqf_split.hpp read.  Host only, standard library only (no HIP, no other eqf_*.hpp; the layout
// constants and the error codes are repeated here and static_assert-ed where both are seen): tests/split_host_main.cpp runs it under the
// sanitizers without a GPU.
//
// A child is one record (dst, src, shift, shrink).  The children are grouped by source, sources in the order of their first appearance,
// the children of a source in the caller's order: the kernels walk a source's children as one contiguous run of the child table, so one
// workgroup reads a tile of the source once and writes all of them.  That is what the dst/src rule buys: a filter named as a dst has no
// source but itself -- one that a child of another source overwrites is nobody's source --, so the only destination that is also read is the
// child that stays in its parent's slot, and nothing has to be staged.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

namespace eqf::split {

constexpr int kRefBase = 11;  // reference base coordinates (kBase)
constexpr int kPadBase = 12;  // ... padded (kLm0): internal index 11 is the structural pad
constexpr int kOk = 0, kInvalid = -1;

inline int refOrder(int N) { return kRefBase + 3 * N; }
inline int paddedOrder(int N) { return kPadBase + 3 * N; }
inline int refToPadded(int i) { return i < kRefBase ? i : i + 1; }

// the tables of the image (the device's structs of eqf_split.hpp have these layouts)
struct Source {
    int src, N;        // filter and its landmark count
    int first, count;  // its children: entries [first, first + count) of the child table
};
struct Child {
    int dst;
    int pair;    // its entry of the pair table (the clone route's kernels copy the small state), -1: the child that stays in place
    int call;    // position in the caller's arrays
    int source;  // entry of the source table
};
struct Pair {  // (eqf_clone.hpp's ClonePair)
    int dst, src, N, fromStage;
};

// What can be checked before the landmark counts are settled: pointers, n, local, the indices, a repeated dst, the dst/src rule, shift
// and shrink.  B: the handle's batch.
inline int headCheck(int B, int local, const double* a, int n, const int* dst_idx, const int* src_idx, const double* shift,
    const double* shrink) {
    if (n < 0 || (local != 0 && local != 1) || B < 0) return kInvalid;
    if (n == 0) return kOk;
    if (!a || !dst_idx || !src_idx || !shift || !shrink) return kInvalid;
    std::vector<char> isDst(size_t(B), 0), overwritten(size_t(B), 0);
    for (int k = 0; k < n; ++k) {
        const int d = dst_idx[k], s = src_idx[k];
        if (d < 0 || d >= B || s < 0 || s >= B) return kInvalid;
        if (isDst[size_t(d)]) return kInvalid;
        isDst[size_t(d)] = 1;
        if (!std::isfinite(shift[k]) || !std::isfinite(shrink[k]) || shrink[k] < 0.0 || shrink[k] > 1.0) return kInvalid;
    }
    // a filter named as a dst has no source but itself: one that another source overwrites is nobody's source
    for (int k = 0; k < n; ++k)
        if (src_idx[k] != dst_idx[k]) overwritten[size_t(dst_idx[k])] = 1;
    for (int k = 0; k < n; ++k)
        if (overwritten[size_t(src_idx[k])]) return kInvalid;
    return kOk;
}
// ... and what needs them: the strides against every named source, and the read part of its row.  N: [B] landmark counts.  ldg < 0:
// no gamma is asked for.
inline int rowCheck(const double* a, int lda, int n, const int* src_idx, int ldg, const int* N) {
    for (int k = 0; k < n; ++k) {
        const int s = src_idx[k], m = refOrder(N[s]);
        if (lda < m || (ldg >= 0 && ldg < m)) return kInvalid;
        const double* row = a + size_t(s) * size_t(lda);
        for (int i = 0; i < m; ++i)
            if (!std::isfinite(row[i])) return kInvalid;
    }
    return kOk;
}

struct Plan {
    std::vector<Source> sources;
    std::vector<Child> children;  // grouped by source
    std::vector<Pair> pairs;      // the children with dst != src, in the child table's order
    int maxN = 0;                 // most landmarks of a named source
};
// (headCheck has passed)
inline void group(int B, int n, const int* dst_idx, const int* src_idx, const int* N, Plan& p) {
    p = Plan{};
    std::vector<int> slot(size_t(B), -1);
    for (int k = 0; k < n; ++k) {
        const int s = src_idx[k];
        if (slot[size_t(s)] < 0) {
            slot[size_t(s)] = int(p.sources.size());
            p.sources.push_back(Source{s, N[s], 0, 0});
            if (N[s] > p.maxN) p.maxN = N[s];
        }
        ++p.sources[size_t(slot[size_t(s)])].count;
    }
    int at = 0;
    for (auto& s : p.sources) {
        s.first = at;
        at += s.count;
    }
    p.children.resize(size_t(n));
    std::vector<int> fill(p.sources.size(), 0);
    for (int k = 0; k < n; ++k) {
        const int si = slot[size_t(src_idx[k])];
        p.children[size_t(p.sources[size_t(si)].first + fill[size_t(si)]++)] = Child{dst_idx[k], -1, k, si};
    }
    for (auto& c : p.children)
        if (c.dst != p.sources[size_t(c.source)].src) {
            c.pair = int(p.pairs.size());
            p.pairs.push_back(Pair{c.dst, p.sources[size_t(c.source)].src, p.sources[size_t(c.source)].N, 0});
        }
}

// The image a call uploads, per handle (B filters of capacity cap; at most B sources and B children, for dst may not repeat), in bytes:
//   rows   [B][ldr] doubles  the row of source table entry i, reference index map, ldr = refOrder(cap)
//   shift  [B], shrink [B]   doubles, in the child table's order
//   sources [B] Source | children [B] Child | pairs [B] Pair
struct Image {
    size_t B, cap;
    size_t ldr() const { return size_t(refOrder(int(cap))); }
    size_t offRows() const { return 0; }
    size_t offShift() const { return sizeof(double) * B * ldr(); }
    size_t offShrink() const { return offShift() + sizeof(double) * B; }
    size_t offSources() const { return offShrink() + sizeof(double) * B; }
    size_t offChildren() const { return offSources() + sizeof(Source) * B; }
    size_t offPairs() const { return offChildren() + sizeof(Child) * B; }
    size_t bytes() const { return offPairs() + sizeof(Pair) * B; }
};
inline void fillImage(const Image& im, const Plan& p, const double* a, int lda, const double* shift, const double* shrink, char* out) {
    double* rows = reinterpret_cast<double*>(out + im.offRows());
    double* sh = reinterpret_cast<double*>(out + im.offShift());
    double* sk = reinterpret_cast<double*>(out + im.offShrink());
    for (size_t i = 0; i < p.sources.size(); ++i) {
        const int m = refOrder(p.sources[i].N);
        double* r = rows + i * im.ldr();
        for (size_t j = 0; j < im.ldr(); ++j) r[j] = j < size_t(m) ? a[size_t(p.sources[i].src) * size_t(lda) + j] : 0.0;
    }
    for (size_t k = 0; k < p.children.size(); ++k) {
        sh[k] = shift[p.children[k].call];
        sk[k] = shrink[p.children[k].call];
    }
    if (!p.sources.empty()) std::memcpy(out + im.offSources(), p.sources.data(), sizeof(Source) * p.sources.size());
    if (!p.children.empty()) std::memcpy(out + im.offChildren(), p.children.data(), sizeof(Child) * p.children.size());
    if (!p.pairs.empty()) std::memcpy(out + im.offPairs(), p.pairs.data(), sizeof(Pair) * p.pairs.size());
}

// The device workspace, in doubles (padded index map, ld = Sigma's leading dimension): Ht [B][ld] | Bv [B][ld] | U [B][ld], all by source
// table entry | G [B][ld] the increments by FILTER | rec [B][2] (S, info) by source table entry | mask [B] bytes by filter
struct Work {
    size_t B, ld;
    size_t offHt() const { return 0; }
    size_t offB() const { return B * ld; }
    size_t offU() const { return 2 * B * ld; }
    size_t offG() const { return 3 * B * ld; }
    size_t offRec() const { return 4 * B * ld; }
    size_t offMask() const { return offRec() + 2 * B; }  // (in doubles; the bytes start there)
    size_t bytes() const { return sizeof(double) * offMask() + B; }
};

// k_split_axis: rows of Sigma per workgroup; k_split_sigma: rows and columns of a tile (256 lanes x 16 bytes)
constexpr int kAxisRows = 16, kTileRows = 8, kTileCols = 512;
inline int axisBlocks(int maxN) { return (paddedOrder(maxN) + kAxisRows - 1) / kAxisRows; }
inline int tileRowBlocks(int maxN) { return (paddedOrder(maxN) + kTileRows - 1) / kTileRows; }
inline int tileColBlocks(int maxN) { return (paddedOrder(maxN) + kTileCols - 1) / kTileCols; }

}  // namespace eqf::split
