// The per-entry arithmetic, the layouts and the argument checks of eqf_observe_landmarks (kernel: eqf_observe.hpp): a bearing, a range or
// a position of landmark i, measured by a camera at the pose (q_c, t_c) in the primary camera's frame, linearised at the handle's own
// estimate.  With J = a^-1 R(q)^T the landmark's block of eqf_get_local_jacobian (landmarkJ: k_local_jacobian's expression), R_c = R(q_c):
//   p_hat = J p0,   p_c = R_c^T (p_hat - t_c),   d = |p_c|,   y_hat = p_c / d
//   bearing   H = stereoSphereChartDiff(y_hat, y_hat) (I - y_hat y_hat^T) R_c^T / d      resid = stereoSphereChart(y, pole y_hat)
//   range     H = y_hat^T R_c^T                                                          resid = rho - d
//   position  H = R_c^T                                                                  resid = m - p_c
// and Ht = H J (blocks::formRows), the rows in eqf_get_sigma's coordinates.  Every sum runs in one fixed order with explicit fused
// multiply-adds (eqf_math.hpp's dot3); the chart functions are eqf_math.hpp's.  An entry is NOT OBSERVABLE when d is zero or not finite,
// or, for a bearing, when a chart function raises its singular flag (y_hat at the chart's own pole e3) or the chart's value is not finite
// (y at the antipode of y_hat).  Needs eqf_math.hpp, which compiles for the host with -D__HIP_PLATFORM_AMD__ and the HIP include
// directory; tests/observe_host_main.cpp runs all of it under the sanitizers without a GPU.
#pragma once
#include <cmath>
#include <cstddef>

#include "eqf_blocks_host.hpp"
#include "eqf_math.hpp"

namespace eqf::observe {

constexpr int kBearing = 0, kRange = 1, kPosition = 2;  // EQF_OBS_BEARING / _RANGE / _POSITION
constexpr int kNotObservable = 3;                       // the verdict on an entry beside blocks::kAbsent / kApplied / kGated
constexpr int kCam = 7;                                 // (q_c: w, x, y, z; t_c)

// rows of an entry; 0: not a kind
EQF_DI int rowsOf(int kind) { return kind == kBearing ? 2 : (kind == kRange ? 1 : (kind == kPosition ? 3 : 0)); }
// values of meas [3] that an entry reads
EQF_DI int measRead(int kind) { return kind == kRange ? 1 : 3; }

// J = a^-1 R(q)^T, row-major: the landmark's block of k_local_jacobian
EQF_DI void landmarkJ(quat q, double a, double* J) {
    const m33 R = q2m(q);
    const double ia = 1.0 / a;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) J[3 * r + c] = ia * R.a[3 * c + r];
}

// One entry: Ht (rows x 3, row-major) and resid (rows) from J (landmarkJ), the origin p0, the offset cam (kCam values, q_c of unit length:
// unitCam) and the measurement.  Returns 0, or 1 when the entry is not observable: Ht and resid are then zeros.
EQF_DI int entryRows(int kind, const double* J, d3 p0, const double* cam, const double* meas, double* Ht, double* resid) {
    const int rows = rowsOf(kind);
    for (int q = 0; q < 3 * rows; ++q) Ht[q] = 0.0;
    for (int r = 0; r < rows; ++r) resid[r] = 0.0;
    const m33 Rc = q2m(quat{cam[0], cam[1], cam[2], cam[3]});
    const d3 ph = mk3(dot3(J[0], p0.x, J[1], p0.y, J[2], p0.z), dot3(J[3], p0.x, J[4], p0.y, J[5], p0.z), dot3(J[6], p0.x, J[7], p0.y, J[8], p0.z));
    const d3 v = mk3(ph.x - cam[4], ph.y - cam[5], ph.z - cam[6]);
    const d3 pc = mk3(dot3(Rc.a[0], v.x, Rc.a[3], v.y, Rc.a[6], v.z), dot3(Rc.a[1], v.x, Rc.a[4], v.y, Rc.a[7], v.z),
        dot3(Rc.a[2], v.x, Rc.a[5], v.y, Rc.a[8], v.z));
    const double d = sqrt(dot3(pc.x, pc.x, pc.y, pc.y, pc.z, pc.z));
    if (!(d > 0.0) || !(d < HUGE_VAL)) return 1;
    const d3 yh = mk3(pc.x / d, pc.y / d, pc.z / d);
    double H[9], rs[3];
    if (kind == kPosition) {
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) H[3 * r + c] = Rc.a[3 * c + r];
        rs[0] = meas[0] - pc.x;
        rs[1] = meas[1] - pc.y;
        rs[2] = meas[2] - pc.z;
    } else if (kind == kRange) {
#pragma unroll
        for (int c = 0; c < 3; ++c) H[c] = dot3(yh.x, Rc.a[3 * c], yh.y, Rc.a[3 * c + 1], yh.z, Rc.a[3 * c + 2]);
        rs[0] = meas[0] - d;
    } else {
        int bad = 0;
        double cd[6];
        stereoChartDiff(yh, yh, cd, &bad);
        stereoChart(mk3(meas[0], meas[1], meas[2]), yh, &rs[0], &rs[1], &bad);
        if (bad || !(fabs(rs[0]) < HUGE_VAL) || !(fabs(rs[1]) < HUGE_VAL)) return 1;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            // row r of cd (I - y_hat y_hat^T), then of ... R_c^T / d
            const double s = dot3(cd[3 * r], yh.x, cd[3 * r + 1], yh.y, cd[3 * r + 2], yh.z);
            const double a0 = fma(-s, yh.x, cd[3 * r]), a1 = fma(-s, yh.y, cd[3 * r + 1]), a2 = fma(-s, yh.z, cd[3 * r + 2]);
#pragma unroll
            for (int c = 0; c < 3; ++c) H[3 * r + c] = dot3(a0, Rc.a[3 * c], a1, Rc.a[3 * c + 1], a2, Rc.a[3 * c + 2]) / d;
        }
    }
    blocks::formRows(rows, H, J, Ht);
    for (int r = 0; r < rows; ++r) resid[r] = rs[r];
    return 0;
}

// ---- a call --------------------------------------------------------------------------------------------------------------------------------
// the offset as the kernel takes it: q_c / |q_c| and t_c; nullptr: the identity
inline void unitCam(const double* cam, double* out) {
    if (!cam) {
        const double id[kCam] = {1, 0, 0, 0, 0, 0, 0};
        for (int i = 0; i < kCam; ++i) out[i] = id[i];
        return;
    }
    const double s = std::sqrt(std::fma(cam[3], cam[3], std::fma(cam[2], cam[2], std::fma(cam[1], cam[1], cam[0] * cam[0]))));
    for (int i = 0; i < 4; ++i) out[i] = cam[i] / s;
    for (int i = 4; i < kCam; ++i) out[i] = cam[i];
}
// The image a call uploads (bytes): cam [B][kCam] (unitCam of each filter's offset) | meas [B][stride][3] | Rb [B][stride][rows][rows]
// (doubles) | idx [B][stride] | nk [B] (ints) | mask [B] (bytes): blocks::SmallLayout with cam and meas in place of Hb and resid
struct SmallLayout {
    int B, stride, rows;
    size_t entries() const { return size_t(B) * stride; }
    size_t offCam() const { return 0; }
    size_t offMeas() const { return sizeof(double) * size_t(B) * kCam; }
    size_t offR() const { return offMeas() + sizeof(double) * entries() * 3; }
    size_t offIdx() const { return offR() + sizeof(double) * entries() * rows * rows; }
    size_t offNk() const { return offIdx() + sizeof(int) * entries(); }
    size_t offMask() const { return offNk() + sizeof(int) * size_t(B); }
    size_t bytes() const { return offMask() + size_t(B); }
};
// The rows the kernel forms, a device array of the call (doubles): Ht [B][stride][rows][3] | resid [B][stride][rows]
struct RowsLayout {
    int B, stride, rows;
    size_t offHt() const { return 0; }
    size_t offResid() const { return size_t(B) * stride * rows * 3; }
    size_t doubles() const { return offResid() + size_t(B) * stride * rows; }
};

// What can be checked before the landmark counts are settled ...
inline bool headArgsOk(int kind, int cam_per_filter, const int* nk, const int* ids, int stride, const double* meas, const double* Rb,
    double gate, double lm_gate) {
    if (rowsOf(kind) == 0 || (cam_per_filter != 0 && cam_per_filter != 1) || stride < 1 || !nk || !ids || !meas || !Rb) return false;
    return gate > 0.0 && lm_gate > 0.0;  // (NaN and <= 0 fail; +inf disarms)
}
inline bool camOk(const double* c) {
    for (int i = 0; i < kCam; ++i)
        if (!std::isfinite(c[i])) return false;
    const double s = std::sqrt(std::fma(c[3], c[3], std::fma(c[2], c[2], std::fma(c[1], c[1], c[0] * c[0]))));
    return s > 0.0 && std::isfinite(s);
}
// ... and what needs them: blocks::argsCheck with cam and meas in place of Hb and resid.  0 fine, 1 EQF_ERR_INVALID, 2 EQF_ERR_UNSORTED,
// 3 EQF_ERR_CAPACITY (in this order of precedence over the batch).  Nothing beyond nk[b] and nothing of a masked filter is read -- its
// own offset included.
inline int argsCheck(int kind, const double* cam, int cam_per_filter, const int* nk, const int* ids, int stride, const double* meas,
    const double* Rb, const unsigned char* mask, const double* gamma, int ldg, int B, const int* N, int cap) {
    const int rows = rowsOf(kind), nm = measRead(kind);
    for (int b = 0; b < B; ++b) {
        if (nk[b] < 0 || nk[b] > stride) return 1;
        if (gamma && ldg < blocks::refOrder(N[b])) return 1;
    }
    if (cam && !cam_per_filter && !camOk(cam)) return 1;
    for (int b = 0; b < B; ++b) {
        if (mask && !mask[b]) continue;
        if (cam && cam_per_filter && !camOk(cam + size_t(b) * kCam)) return 1;
        for (int k = 0; k < nk[b]; ++k) {
            const size_t e = size_t(b) * stride + k;
            for (int i = 0; i < nm; ++i)
                if (!std::isfinite(meas[e * 3 + i])) return 1;
            for (int r = 0; r < rows; ++r)
                for (int l = 0; l <= r; ++l)  // (only the lower triangle is read)
                    if (!std::isfinite(Rb[(e * rows + r) * rows + l])) return 1;
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

}  // namespace eqf::observe
