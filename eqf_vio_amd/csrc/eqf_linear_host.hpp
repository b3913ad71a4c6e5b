// Index arithmetic and argument checks of the low-rank linear measurement update (eqf_update_linear): the launch grids of eqf_linear.hpp's
// kernels, the layout of the per-filter workspace, the packing of the caller's rows, residuals and noise covariance into the image that is
// uploaded, the unpacking of gamma, and what makes a call EQF_ERR_INVALID.  Host only, standard library only (no HIP, no other eqf_*.hpp;
// the layout constants are repeated here and static_assert-ed against eqf_device.hpp where both are seen): tests/linear_host_main.cpp runs
// it under the sanitizers without a GPU.
#pragma once
#include <cmath>
#include <cstddef>

namespace eqf::linear {

constexpr int kRefBase = 11;   // reference base coordinates (kBase)
constexpr int kPadBase = 12;   // ... padded (kLm0): internal index 11 is the structural pad
constexpr int kRows = 16;      // measurement rows of a call, padded (one MFMA tile)
constexpr int kTile = 64;      // rows / columns of a Sigma tile (kSB)
constexpr int kHead = 20;      // doubles of a filter's result record (eqf_nees.hpp's kNeesHead + kNeesRhs: k_apply_increment reads entry 3)

inline int refOrder(int N) { return kRefBase + 3 * N; }
inline int paddedOrder(int N) { return kPadBase + 3 * N; }
inline int refToPadded(int i) { return i < kRefBase ? i : i + 1; }
inline int paddedToRef(int j) { return j < kRefBase ? j : (j == kRefBase ? -1 : j - 1); }
// 64-row tiles of a filter of N landmarks, and tiles of the lower triangle (diagonal included)
inline int rowTiles(int N) { return (paddedOrder(N) + kTile - 1) / kTile; }
inline int triTiles(int nt) { return nt * (nt + 1) / 2; }
// tile t of the lower triangle, rows first: t = I (I + 1) / 2 + J, J <= I
inline void triTile(int t, int* I, int* J) {
    int i = 0;
    while ((i + 1) * (i + 2) / 2 <= t) ++i;
    *I = i;
    *J = t - i * (i + 1) / 2;
}

// The image a call uploads, per handle, in doubles: [B][kRows][ldr] rows of H (reference index map, ldr = refOrder(cap)) | [B][kRows] resid
// | [B][kRows][kRows] R | the mask, one byte per filter, behind them.
struct SmallLayout {
    int B, ldr;
    size_t offH() const { return 0; }
    size_t offResid() const { return size_t(B) * kRows * ldr; }
    size_t offR() const { return offResid() + size_t(B) * kRows; }
    size_t offMask() const { return offR() + size_t(B) * kRows * kRows; }  // (in doubles; the bytes start there)
    size_t bytes() const { return sizeof(double) * offMask() + size_t(B); }
};
// The device workspace, per filter, in doubles: Ht [kRows][ld] | Bt [kRows][ld] | Y [kRows][ld] | gamma [ld]   (padded index map)
struct WorkLayout {
    int ld;
    long long offHt() const { return 0; }
    long long offBt() const { return (long long)kRows * ld; }
    long long offY() const { return 2LL * kRows * ld; }
    long long offGamma() const { return 3LL * kRows * ld; }
    long long stride() const { return (3LL * kRows + 1) * ld; }
};

// What can be checked before the landmark counts are settled ...
inline bool headArgsOk(int local, int m, const double* H, const double* resid, const double* R, double gate) {
    if ((local != 0 && local != 1) || m < 1 || m > kRows || !H || !resid || !R) return false;
    return gate > 0.0;  // (NaN and <= 0 fail; +inf disarms)
}
// ... and what needs them: the strides, and every entry of the operands of the filters that take part
inline bool argsOk(int m, const double* H, int ldh, const double* resid, const double* R, const unsigned char* mask, const double* gamma,
    int ldg, int B, const int* N) {
    if (!H || !resid || !R || !N || B < 0 || m < 1 || m > kRows) return false;
    for (int b = 0; b < B; ++b) {
        const int n = refOrder(N[b]);
        if (ldh < n || (gamma && ldg < n)) return false;
        if (mask && !mask[b]) continue;
        for (int k = 0; k < m; ++k) {
            const double* h = H + (size_t(b) * m + k) * ldh;
            for (int i = 0; i < n; ++i)
                if (!std::isfinite(h[i])) return false;
            if (!std::isfinite(resid[size_t(b) * m + k])) return false;
            for (int l = 0; l <= k; ++l)  // (only the lower triangle is read)
                if (!std::isfinite(R[(size_t(b) * m + k) * m + l])) return false;
        }
    }
    return true;
}

// One filter's operands -> its part of the uploaded image: rows m .. 15 of H and resid are zero, R's are rows of the identity, R's upper
// triangle is written as 0 (never read by the device).
inline void packFilter(int m, int N, const double* H, int ldh, const double* resid, const double* R, double* dH, int ldr, double* dResid,
    double* dR) {
    const int n = refOrder(N);
    for (int k = 0; k < kRows; ++k) {
        for (int i = 0; i < ldr; ++i) dH[size_t(k) * ldr + i] = (k < m && i < n) ? H[size_t(k) * ldh + i] : 0.0;
        dResid[k] = k < m ? resid[k] : 0.0;
        for (int l = 0; l < kRows; ++l) dR[k * kRows + l] = k < m ? (l <= k ? R[size_t(k) * m + l] : 0.0) : (l == k ? 1.0 : 0.0);
    }
}
// gamma of one filter, padded map -> reference map; zero != 0: every entry is written as 0 (an untouched filter)
inline void unpackGamma(const double* src, int N, double* dst, int zero) {
    for (int i = 0; i < refOrder(N); ++i) dst[i] = zero ? 0.0 : src[refToPadded(i)];
}

}  // namespace eqf::linear
