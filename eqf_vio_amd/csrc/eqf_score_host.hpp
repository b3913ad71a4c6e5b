// Argument checks, id matching, the chunk plan, the layouts of the two device blocks and the record arithmetic of eqf_score_vision.  Host
// only, standard library only (no HIP, no
// other eqf_*.hpp; the constants repeated here are static_assert-ed against eqf_device.hpp / the C header where both are seen):
// tests/score_host_main.cpp runs it under the sanitizers without a GPU.  The record arithmetic is __host__ __device__ where a HIP compiler
// sees it: k_score_tail evaluates the same text.
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

#if defined(__HIPCC__)
#define EQF_SC_HD __host__ __device__
#else
#define EQF_SC_HD
#endif

namespace eqf::score {

constexpr int kBlock = 64;       // block column of the factorisation (kSB)
constexpr int kChunkMax = 4096;  // upper end of the option "score_chunk"
constexpr int kRec = 8;          // per item on the device: nis, logdet_S, loglik, dof, info, 0, 0, 0
// what checkArgs answers (the C header's codes)
constexpr int kOk = 0, kInvalid = -1, kCapacity = -4, kUnsorted = -5;
// info words of a record
constexpr int kInfoOk = 0, kInfoNumeric = 1, kInfoMasked = 3;

// One candidate of one filter as the kernels see it: its filter, the number of entries that matched a landmark of the state and where its
// matched slots / permuted bearings / per-landmark outputs start in the call's tables.
struct Item {
    int b, m;
    int first, masked;
};

// The argument checks behind the NULL checks, in eqf_process_vision's order per candidate: nb's range, the capacity, ascending ids, and
// finite bearings.  A filter that is masked out is checked for nb's range and the capacity only.
inline int checkArgs(int B, int cap, int ncand, const int* nb, const int* ids, const double* bearings, int stride, const unsigned char* mask) {
    if (B < 1 || ncand < 1 || stride < 1 || !nb || !ids || !bearings) return kInvalid;
    for (int b = 0; b < B; ++b)
        for (int c = 0; c < ncand; ++c) {
            const size_t it = size_t(b) * ncand + c;
            const int n = nb[it];
            if (n < 0 || n > stride) return kInvalid;
            if (n > cap) return kCapacity;
            if (mask && !mask[b]) continue;
            const int* id = ids + it * stride;
            for (int k = 1; k < n; ++k)
                if (id[k] <= id[k - 1]) return kUnsorted;
            const double* y = bearings + it * stride * 3;
            for (int k = 0; k < 3 * n; ++k)
                if (!std::isfinite(y[k])) return kInvalid;
        }
    return kOk;
}

// The entries of a candidate (n ids, strictly ascending) that name a landmark of the state (nState ids in the state's own order, which need
// not be ascending: landmarks are appended and compacted, never sorted), IN THE STATE'S ORDER: slots gets the state slots, pos the
// candidate's entry positions.  Returns the count.  Ids that the state does not hold take no part.
inline int matchItem(int nState, const int* stateIds, int n, const int* ids, std::vector<int>& slots, std::vector<int>& pos) {
    int count = 0;
    for (int s = 0; s < nState && n > 0; ++s) {
        int lo = 0, hi = n - 1;
        while (lo < hi) {  // the first entry that is not below the slot's id
            const int mid = lo + (hi - lo) / 2;
            if (ids[mid] < stateIds[s]) lo = mid + 1;
            else hi = mid;
        }
        if (ids[lo] == stateIds[s]) {
            slots.push_back(s);
            pos.push_back(lo);
            ++count;
        }
    }
    return count;
}

// chunk plan: items [first, first + count) per round of launches (eqf_mergecost_host.hpp's arrangement)
inline int chunkSize(int option, int B) { return option > 0 ? option : (B > 0 ? B : 1); }
inline bool chunkOptionOk(int value) { return value >= 1 && value <= kChunkMax; }
inline int numChunks(long long items, int chunk) { return int((items + chunk - 1) / chunk); }
inline int chunkCount(long long items, int chunk, int c) {
    const long long left = items - (long long)c * chunk;
    return int(left < chunk ? left : chunk);
}
inline int blockColumns(int m) { return (m + kBlock - 1) / kBlock; }
// leading dimension of an image: the order 2 * capacity padded to whole block columns
inline int paddedOrder(int cap) { return kBlock * blockColumns(2 * (cap > 0 ? cap : 1)); }
// kernel launches per chunk for the largest order m of the call: k_score_form, the factorisation's schedule with the one right-hand-side
// row, k_score_tail
inline int launchesPerChunk(int m) {
    const int nb = blockColumns(m);
    int l = 3;  // k_score_form, k_factor_diag(0), k_score_tail
    for (int K = 0; K < nb; ++K) {
        const int t = nb - K - 1;
        if (K > 0) ++l;
        ++l;  // the panel: the right-hand side's workgroup is always there
        if (t > 0) ++l;
    }
    return l;
}

// The workspace of a chunk of C images of leading dimension ldW = paddedOrder(capacity), in doubles: W [C][ldW][ldW] the images | E [C][ldW]
// their right-hand-side rows | D [C][dRec] the records of the current diagonal block | bad [C] ints behind them, rounded up to whole doubles
struct WorkLayout {
    size_t C, ldW, dRec;
    size_t offW() const { return 0; }
    size_t offE() const { return C * ldW * ldW; }
    size_t offD() const { return offE() + C * ldW; }
    size_t offBad() const { return offD() + C * dRec; }  // (in doubles; the ints start there)
    size_t doubles() const { return offBad() + (C + 1) / 2; }
};
// The tables of a call in one block, in bytes: rec [nItems][kRec] doubles | nisLm [nMatched] doubles | y [nMatched][3] doubles | items
// [nItems] Item | slots [nMatched] ints
struct TabLayout {
    size_t nItems, nMatched;
    size_t offRec() const { return 0; }
    size_t offNisLm() const { return sizeof(double) * kRec * nItems; }
    size_t offY() const { return offNisLm() + sizeof(double) * nMatched; }
    size_t offItems() const { return offY() + sizeof(double) * 3 * nMatched; }
    size_t offSlots() const { return offItems() + sizeof(Item) * nItems; }
    size_t bytes() const { return offSlots() + sizeof(int) * nMatched; }
};

// ---- the record from (nis, logdet_S, dof)
EQF_SC_HD inline double logLikelihood(double nis, double logdet, int dof) {
    return -0.5 * (nis + logdet + double(dof) * 1.8378770664093453 /* log 2 pi */);
}
EQF_SC_HD inline bool finiteValue(double x) { return x == x && (x < 0.0 ? -x : x) < HUGE_VAL; }
// rec[kRec] of an item: bad = a pivot of S was not positive (or not finite)
EQF_SC_HD inline void writeRecord(double* rec, double nis, double logdet, int dof, bool bad) {
    const double ll = dof > 0 ? logLikelihood(nis, logdet, dof) : 0.0;  // (an empty measurement: exactly 0, not -0)
    const int info = (bad || !finiteValue(nis) || !finiteValue(logdet) || !finiteValue(ll)) ? kInfoNumeric : kInfoOk;
    const double nan = NAN;
    rec[0] = info ? nan : nis;
    rec[1] = info ? nan : logdet;
    rec[2] = info ? nan : ll;
    rec[3] = double(dof);
    rec[4] = double(info);
    rec[5] = 0.0;
    rec[6] = 0.0;
    rec[7] = 0.0;
}

}  // namespace eqf::score
