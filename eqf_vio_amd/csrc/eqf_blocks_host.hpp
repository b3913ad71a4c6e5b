// The per-entry arithmetic, the index arithmetic and the argument checks of the per-landmark block measurement update
// (eqf_update_landmarks; kernels: eqf_blocks.hpp): forming an entry's rows in Sigma's coordinates, its own Mahalanobis distance, the verdict
// on it (applied / id not in the state / gated), the compaction of the entries that take part, the launch grids, the layouts of the
// uploaded image and of the per-filter workspace, and what makes a call EQF_ERR_INVALID / _UNSORTED / _CAPACITY.  Standard library only (no
// HIP, no other eqf_*.hpp; the layout constants are repeated here and static_assert-ed against eqf_device.hpp where both are seen): the
// kernels call the EQF_BLK_HD functions on the device, tests/blocks_host_main.cpp runs all of it under the sanitizers without a GPU.
#pragma once
#include <cmath>
#include <cstddef>

#if defined(__HIPCC__)
#define EQF_BLK_HD __host__ __device__ inline
#else
#define EQF_BLK_HD inline
#endif

namespace eqf::blocks {

constexpr int kRefBase = 11;   // reference base coordinates (kBase)
constexpr int kPadBase = 12;   // ... padded (kLm0): internal index 11 is the structural pad
constexpr int kTile = 64;      // rows / columns of a tile of Sigma, of S and of Y (kSB)
constexpr int kMaxRows = 3;    // rows of one entry
constexpr int kHead = 20;      // doubles of a filter's result record (kLinHead: k_apply_increment reads entry 3)
constexpr int kPairs = 16;     // entries per side of a workgroup's tile of S (16 x 16 pairs of entries)
// the verdict on an entry (used[])
constexpr int kAbsent = 0, kApplied = 1, kGated = 2;
// the verdict word of a filter beyond eqf_linear_report's codes: no entry takes part (reported as info = 0, dof = 0; nothing runs)
constexpr int kInfoIdle = 4;

inline int refOrder(int N) { return kRefBase + 3 * N; }
inline int paddedOrder(int N) { return kPadBase + 3 * N; }
inline int refToPadded(int i) { return i < kRefBase ? i : i + 1; }
inline int roundTile(int x) { return (x + kTile - 1) / kTile * kTile; }
inline int rowTiles(int N) { return (paddedOrder(N) + kTile - 1) / kTile; }
inline int triTiles(int nt) { return nt * (nt + 1) / 2; }

// ---- one entry ---------------------------------------------------------------------------------------------------------------------------
// Ht = H (J == nullptr) or H J: rows x 3, row-major; J = a^-1 R(q)^T row-major (k_local_jacobian's block).  One product and two fused
// multiply-adds per entry (eqf_math.hpp's dot3).
EQF_BLK_HD void formRows(int rows, const double* H, const double* J, double* Ht) {
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < 3; ++c)
            Ht[3 * r + c] = J ? std::fma(H[3 * r + 2], J[6 + c], std::fma(H[3 * r + 1], J[3 + c], H[3 * r] * J[c])) : H[3 * r + c];
}
// t = A h for a 3 x 3 block A (row-major, every entry read) and a row h of Ht: dot3 per entry
EQF_BLK_HD void blockTimesRow(const double* A, const double* h, double* t) {
    for (int j = 0; j < 3; ++j) t[j] = std::fma(A[3 * j + 2], h[2], std::fma(A[3 * j + 1], h[1], A[3 * j] * h[0]));
}
// the entry's own S_kk = Ht Sii Ht^T + R (lower triangle, rows x rows in a 3 x 3 array) from the landmark's diagonal block of Sigma (Sii:
// 3 x 3 row-major, ONLY its lower triangle is read) and R (rows x rows row-major, ONLY its lower triangle is read): s = R_kl, then three
// fused multiply-adds
EQF_BLK_HD void entryS(int rows, const double* Ht, const double* Sii, const double* R, double* S) {
    const double A[9] = {Sii[0], Sii[3], Sii[6], Sii[3], Sii[4], Sii[7], Sii[6], Sii[7], Sii[8]};
    for (int l = 0; l < rows; ++l) {
        double t[3];
        blockTimesRow(A, Ht + 3 * l, t);
        for (int k = l; k < rows; ++k) {
            double s = R[k * rows + l];
            for (int j = 0; j < 3; ++j) s = std::fma(Ht[3 * k + j], t[j], s);
            S[3 * k + l] = s;
        }
    }
}
// d2 = resid^T S_kk^-1 resid through the Cholesky factor of S_kk (divisions, no inverses); NaN when a pivot is not positive or not finite
EQF_BLK_HD double entryD2(int rows, const double* S, const double* resid) {
    double L[9], z[3], d2 = 0.0;
    for (int j = 0; j < rows; ++j) {
        double d = S[3 * j + j];
        for (int c = 0; c < j; ++c) d = std::fma(-L[3 * j + c], L[3 * j + c], d);
        if (!(d > 0.0) || !(d < HUGE_VAL)) return __builtin_nan("");
        L[3 * j + j] = std::sqrt(d);
        for (int k = j + 1; k < rows; ++k) {
            double v = S[3 * k + j];
            for (int c = 0; c < j; ++c) v = std::fma(-L[3 * k + c], L[3 * j + c], v);
            L[3 * k + j] = v / L[3 * j + j];
        }
    }
    for (int r = 0; r < rows; ++r) {
        double v = resid[r];
        for (int c = 0; c < r; ++c) v = std::fma(-L[3 * r + c], z[c], v);
        z[r] = v / L[3 * r + r];
        d2 = std::fma(z[r], z[r], d2);
    }
    return d2;
}
// idx: the landmark's index in the filter's state, < 0 when its id is not there.  A NaN distance stays in; lm_gate = +inf disarms.
EQF_BLK_HD int entryVerdict(int idx, double d2, double lm_gate) { return idx < 0 ? kAbsent : (d2 > lm_gate ? kGated : kApplied); }
// The entries that take part, in their order, packed to the front: pos[k] = position of entry k among them (-1: does not take part),
// ent[p] = the entry at position p.  Returns their number.  An entry that does not take part is thereby a decoupled block that is never
// formed: the filter's S has order rows * (return value), and the result is the one of the call without that entry, bit for bit.
EQF_BLK_HD int compact(int nk, const int* used, int* pos, int* ent) {
    int p = 0;
    for (int k = 0; k < nk; ++k) {
        const bool in = used[k] == kApplied;
        pos[k] = in ? p : -1;
        if (in) ent[p++] = k;
    }
    return p;
}

// ---- a call --------------------------------------------------------------------------------------------------------------------------------
// The image a call uploads (bytes): Hb [B][stride][rows][3] | resid [B][stride][rows] | Rb [B][stride][rows][rows] (doubles, the caller's
// arrays as they are) | idx [B][stride] | nk [B] (ints) | mask [B] (bytes)
struct SmallLayout {
    int B, stride, rows;
    size_t entries() const { return size_t(B) * stride; }
    size_t offH() const { return 0; }
    size_t offResid() const { return sizeof(double) * entries() * rows * 3; }
    size_t offR() const { return offResid() + sizeof(double) * entries() * rows; }
    size_t offIdx() const { return offR() + sizeof(double) * entries() * rows * rows; }
    size_t offNk() const { return offIdx() + sizeof(int) * entries(); }
    size_t offMask() const { return offNk() + sizeof(int) * size_t(B); }
    size_t bytes() const { return offMask() + size_t(B); }
};
// The device workspace.  Per filter, in doubles: the tall matrix M [mp + ld + 1][mp] with mp = roundTile(rows * stride): rows [0, mp) S ->
// L (lower triangle; nothing past the filter's own order is ever touched), rows mp + i the row i of B = Sigma Ht^T -> of Y^T (padded index
// map, i < n), row mp + n resid -> z | Ht [stride][9] | gamma [ld] | the record of the current diagonal block [kDRec].  Per filter, in
// ints: used [stride] | pos [stride] | ent [stride] | count | bad pivot | non-finite | 1 spare.
struct WorkLayout {
    int ld, stride, rows, dRec;
    int mp() const { return roundTile(rows * stride); }
    int nb() const { return mp() / kTile; }
    long long offM() const { return 0; }
    long long offHt() const { return (long long)(mp() + ld + 1) * mp(); }
    long long offGamma() const { return offHt() + 9LL * stride; }
    long long offD() const { return offGamma() + ld; }
    long long strideD() const { return offD() + dRec; }  // doubles per filter
    int offUsed() const { return 0; }
    int offPos() const { return stride; }
    int offEnt() const { return 2 * stride; }
    int offCount() const { return 3 * stride; }
    int offBad() const { return 3 * stride + 1; }
    int strideI() const { return 3 * stride + 4; }  // ints per filter
};
// 64-row blocks below block column K of the tall matrix: those of S, then those of B and resid (n + 1 rows of the largest filter)
inline int rhsBlocks(int nMaxPadded) { return (nMaxPadded + 1 + kTile - 1) / kTile; }
inline int pairTiles(int stride) { return (stride + kPairs - 1) / kPairs; }

// What can be checked before the landmark counts are settled ...
inline bool headArgsOk(int local, int rows, const int* nk, const int* ids, int stride, const double* Hb, const double* resid, const double* Rb,
    double gate, double lm_gate) {
    if ((local != 0 && local != 1) || rows < 1 || rows > kMaxRows || stride < 1 || !nk || !ids || !Hb || !resid || !Rb) return false;
    return gate > 0.0 && lm_gate > 0.0;  // (NaN and <= 0 fail; +inf disarms)
}
// ... and what needs them.  0 fine, 1 EQF_ERR_INVALID, 2 EQF_ERR_UNSORTED, 3 EQF_ERR_CAPACITY (in this order of precedence over the batch)
inline int argsCheck(int rows, const int* nk, const int* ids, int stride, const double* Hb, const double* resid, const double* Rb,
    const unsigned char* mask, const double* gamma, int ldg, int B, const int* N, int cap) {
    for (int b = 0; b < B; ++b) {
        if (nk[b] < 0 || nk[b] > stride) return 1;
        if (gamma && ldg < refOrder(N[b])) return 1;
    }
    for (int b = 0; b < B; ++b) {
        if (mask && !mask[b]) continue;
        for (int k = 0; k < nk[b]; ++k) {
            const size_t e = size_t(b) * stride + k;
            for (int i = 0; i < 3 * rows; ++i)
                if (!std::isfinite(Hb[e * rows * 3 + i])) return 1;
            for (int r = 0; r < rows; ++r) {
                if (!std::isfinite(resid[e * rows + r])) return 1;
                for (int l = 0; l <= r; ++l)  // (only the lower triangle is read)
                    if (!std::isfinite(Rb[(e * rows + r) * rows + l])) return 1;
            }
        }
    }
    for (int b = 0; b < B; ++b) {
        if (mask && !mask[b]) continue;
        for (int k = 1; k < nk[b]; ++k)
            if (ids[size_t(b) * stride + k] <= ids[size_t(b) * stride + k - 1]) return 2;
    }
    for (int b = 0; b < B; ++b)
        if (nk[b] > cap) return 3;
    return 0;
}
// the landmark index of id in a filter's id list (any order), -1 when it is not there
inline int findId(const int* stateIds, int N, int id) {
    for (int i = 0; i < N; ++i)
        if (stateIds[i] == id) return i;
    return -1;
}
// gamma of one filter, padded map -> reference map; zero != 0: every entry is written as 0 (an untouched filter)
inline void unpackGamma(const double* src, int N, double* dst, int zero) {
    for (int i = 0; i < refOrder(N); ++i) dst[i] = zero ? 0.0 : src[refToPadded(i)];
}

}  // namespace eqf::blocks
