// Index arithmetic and argument checks of the covariance draws (eqf_sample_sigma, eqf_apply_increment, eqf_perturb_filters): the reference <->
// padded index map of a trailing submatrix, the tile counts of k_sample_trmm's grid, the packing of the caller's vectors into the device's
// rows and back, the layouts of the staged small operands and of the factorisation's records, and what makes a call EQF_ERR_INVALID.  Host only, standard library only (no HIP, no other eqf_*.hpp; the layout constants
// arrive as arguments where eqf_device.hpp defines them): tests/sample_host_main.cpp runs it under the sanitizers without a GPU.
#pragma once
#include <cmath>
#include <cstddef>
#include <limits>

namespace eqf::sample {

constexpr int kRefBase = 11;    // reference base coordinates (kBase)
constexpr int kPadBase = 12;    // ... padded (kLm0): internal index 11 is the structural pad
constexpr int kTileRows = 16;   // samples per row tile (kNeesRhs)
constexpr int kBlock = 64;      // block-column width (kSB)
constexpr int kMaxSamples = 64;

// first = 0 | 6 | 11 (reference) -> internal index of the submatrix' first row; -1: not a block boundary
inline int cutOffset(int first) { return first == 0 ? 0 : (first == 6 ? 6 : (first == kRefBase ? kPadBase : -1)); }
// reference index i -> internal index, and back (-1 for the pad)
inline int refToPadded(int i) { return i < kRefBase ? i : i + 1; }
inline int paddedToRef(int j) { return j < kRefBase ? j : (j == kRefBase ? -1 : j - 1); }
// order of a filter's reference state and of its padded submatrix from internal index off
inline int refOrder(int N) { return kRefBase + 3 * N; }
inline int paddedOrder(int N, int off) { return kPadBase + 3 * N - off; }
// k_sample_trmm's grid: block columns of the largest submatrix, row tiles of the samples, rows of the device's sample image
inline int blockColumns(int m) { return m <= 0 ? 0 : (m + kBlock - 1) / kBlock; }
inline int rowTiles(int nsamp) { return nsamp <= 0 ? 0 : (nsamp + kTileRows - 1) / kTileRows; }
inline int paddedRows(int nsamp) { return kTileRows * rowTiles(nsamp); }

// The small operands of a call as one staged image, in doubles: scale [B] | vectors [B][vecLen()] (z of a perturbation or the increments,
// padded index map) | the mask, one byte per filter, behind them.  eqf_sample_sigma uploads the scales alone, eqf_apply_increment the
// vectors with the mask.
struct Range {
    size_t offset, bytes;
};
struct SmallLayout {
    size_t B, cap;
    size_t vecLen() const { return size_t(kPadBase) + 3 * cap; }
    size_t offScale() const { return 0; }
    size_t offVec() const { return B; }
    size_t offMask() const { return B * (1 + vecLen()); }  // (in doubles; the bytes start there)
    size_t bytes() const { return sizeof(double) * offMask() + B; }
    Range scaleRange() const { return {0, sizeof(double) * B}; }
    Range vecMaskRange() const { return {sizeof(double) * offVec(), bytes() - sizeof(double) * offVec()}; }
};
// k_nees_tail's records, in doubles: per filter logdet, min_pivot, dof, info | nees [kTileRows]
constexpr int kRecHead = 4;  // (kNeesHead)
constexpr int kRecInfo = 3;
struct RecordsLayout {
    size_t B;
    static constexpr size_t record() { return size_t(kRecHead + kTileRows); }
    size_t offRecord(size_t b) const { return b * record(); }
    size_t offInfo(size_t b) const { return offRecord(b) + kRecInfo; }
    size_t offNees(size_t b, size_t k) const { return offRecord(b) + kRecHead + k; }
    size_t doubles() const { return B * record(); }
    size_t bytes() const { return sizeof(double) * doubles(); }
};

// eqf_sample_sigma's arguments (nMax: the most landmarks any filter of the handle holds).  True: the call may go on.
inline bool drawArgsOk(int local, int first, int nsamp, const double* z, int ldz, const double* eps, int lde, const void* stats, int nMax) {
    if ((local != 0 && local != 1) || cutOffset(first) < 0 || nsamp < 0 || nsamp > kMaxSamples) return false;
    if (nsamp == 0) return stats != nullptr;  // (only the factorisation's report is asked for)
    return z && eps && ldz >= refOrder(nMax) && lde >= refOrder(nMax);
}

// One caller's vector (reference index map, entries [first, n) used) -> one row of the device image (column = internal index - off; the
// pad column and everything from the filter's own order to `width` are zero).  first <= n.
inline void packRow(const double* src, int first, int N, double* dst, int width) {
    const int off = cutOffset(first), n = refOrder(N);
    for (int j = 0; j < width; ++j) dst[j] = 0.0;
    for (int i = first; i < n; ++i) dst[refToPadded(i) - off] = src[i];
}
// ... and back: entries below first are written as 0, entries from n on are left alone.  fill != nullptr: every entry [first, n) is *fill
inline void unpackRow(const double* src, int first, int N, double* dst, const double* fill) {
    const int off = cutOffset(first), n = refOrder(N);
    for (int i = 0; i < first && i < n; ++i) dst[i] = 0.0;
    for (int i = first; i < n; ++i) dst[i] = fill ? *fill : src[refToPadded(i) - off];
}

// eqf_apply_increment: every entry of the increments of the filters that take part is finite (mask == nullptr: all of them)
inline bool incrementArgsOk(const double* gamma, int ldg, const unsigned char* mask, int B, const int* N) {
    if (!gamma || !N || B < 0) return false;
    for (int b = 0; b < B; ++b) {
        if (ldg < refOrder(N[b])) return false;
        if (mask && !mask[b]) continue;
        for (int i = 0; i < refOrder(N[b]); ++i)
            if (!std::isfinite(gamma[(size_t)b * ldg + i])) return false;
    }
    return true;
}
// eqf_perturb_filters: one z per filter; a scale must be a number (0 switches its filter off)
inline bool perturbArgsOk(int first, const double* z, int ldz, const double* scale, int B, int nMax) {
    if (cutOffset(first) < 0 || !z || ldz < refOrder(nMax)) return false;
    for (int b = 0; scale && b < B; ++b)
        if (!std::isfinite(scale[b])) return false;
    return true;
}

}  // namespace eqf::sample
