// Index arithmetic and argument checks of the non-mutating forecast (eqf_forecast): the launch grids of eqf_forecast.hpp's two kernels, the
// layout of the uploaded sample image, of the per-step records the builder leaves for the landmark lanes and of the output record that is
// copied back, and what makes a call EQF_ERR_INVALID.  Host only, standard library only (no HIP, no other eqf_*.hpp; the layout constants
// are repeated here and static_assert-ed against eqf_device.hpp / eqf_forecast.hpp where both are seen): tests/forecast_host_main.cpp runs
// it under the sanitizers without a GPU.
#pragma once
#include <cmath>
#include <cstddef>

namespace eqf::forecast {

constexpr int kMaxSteps = 256;  // IMU samples of one call (K)
constexpr int kImuRec = 8;      // doubles of one uploaded sample: stamp, omega (3), accel (3), pad -- ImuRec, eqf_stream_upload's record + pad
constexpr int kLanes = 64;      // landmarks per workgroup of the landmark kernel (one wavefront, one lane per landmark)
constexpr int kBuildThreads = 128;

// ---- per-step record (doubles) the builder writes and every landmark lane reads, wave-uniform
constexpr int kRecStep = 0;     // 1.0: the step integrates (dt > 0), 0.0: it only replaces the sample
constexpr int kRecT = 1;        // accumulated time T of the linearisation
constexpr int kRecDt = 2;       // this step's dt
constexpr int kRecRA = 3;       // R_A (9)
constexpr int kRecVC = 12;      // v_C (3)
constexpr int kRecCamInv = 15;  // SE3Exp(-dt U_C): quaternion (4), translation (3)
constexpr int kRecOC = 22;      // omega_C of the current sample (3)
constexpr int kRecVCcur = 25;   // v_C of the current sample (3)
constexpr int kRecSb = 28;      // rows 0:3 and 8:11 of Sigma_bb BEFORE the step (6 x 11)
constexpr int kRecFg = 94;      // F_bb[6:8, 0:3]   (2 x 3)
constexpr int kRecFv = 100;     // F_bb[8:11, 0:8]  (3 x 8)
constexpr int kRecNb = 124;     // gyro columns of B for base rows 6..10 (5 x 3)
constexpr int kStepRec = 144;   // (139 used)

// ---- output record of one filter (doubles): head | base block | one record per landmark
constexpr int kHeadTime = 0, kHeadSteps = 1, kHeadFlag = 2, kHeadPoseQ = 3, kHeadPoseX = 7, kHeadVel = 10;
constexpr int kHead = 16;
constexpr int kBaseDoubles = 128;  // 11 x 11 row-major, padded
constexpr int kLmP = 0, kLmBearing = 3, kLmCov = 6, kLmS = 15, kLmYcov = 19, kLmFlag = 28;
constexpr int kLmRec = 32;

// head[kHeadFlag]: 0 fine; bit 1 a singular chart (SO3FromVectors' antipodal case); bit 2 a value that is not finite
constexpr int kFlagChart = 1, kFlagNonFinite = 2;

inline int steps(int K, bool hasT1) { return K + (hasT1 ? 1 : 0); }
// the uploaded image: [steps][B] samples, the closing integrateUpToTime(t1) as a last sample that carries only its stamp
inline size_t imageDoubles(int K, bool hasT1, int B) { return size_t(steps(K, hasT1)) * size_t(B) * kImuRec; }
inline size_t imageIndex(int s, int b, int B) { return (size_t(s) * size_t(B) + size_t(b)) * kImuRec; }
inline size_t imageCapacityDoubles(int B) { return size_t(kMaxSteps + 1) * size_t(B) * kImuRec; }
// the step records: [B][kMaxSteps + 1][kStepRec]
inline size_t recIndex(int b, int s) { return (size_t(b) * (kMaxSteps + 1) + size_t(s)) * kStepRec; }
inline size_t recDoubles(int B) { return size_t(B) * (kMaxSteps + 1) * kStepRec; }
// the output record
inline size_t outStride(int cap) { return size_t(kHead) + kBaseDoubles + size_t(kLmRec) * size_t(cap); }
inline size_t outBase(int cap, int b) { return outStride(cap) * size_t(b) + kHead; }
inline size_t outLm(int cap, int b, int i) { return outStride(cap) * size_t(b) + kHead + kBaseDoubles + size_t(kLmRec) * size_t(i); }
// doubles of filter b's record that hold something when it has N landmarks (what is copied back)
inline size_t outUsed(int N) { return size_t(kHead) + kBaseDoubles + size_t(kLmRec) * size_t(N); }

// grids: the builder runs one workgroup per filter (grid.y), the landmark kernel one lane per landmark with the filters in grid.y; a batch
// whose largest filter has no landmark still launches one (idle) workgroup per filter, so the number of launches never depends on N
struct Grid {
    int x, y, threads;
};
inline Grid buildGrid(int B) { return Grid{1, B, kBuildThreads}; }
inline Grid lmGrid(int nMax, int B) { return Grid{nMax > 0 ? (nMax + kLanes - 1) / kLanes : 1, B, kLanes}; }

// Which outputs need a row per landmark (and with them a stride)
struct Wants {
    bool p, bearing, lm, S, ycov;
    bool perLandmark() const { return p || bearing || lm || S || ycov; }
};

// What can be checked before the landmark counts are settled ...
inline bool headArgsOk(const void* handle, const void* out, int K, const double* imu, int local, int stride) {
    if (!handle || !out) return false;
    if (K < 0 || K > kMaxSteps) return false;
    if ((K > 0) != (imu != nullptr)) return false;  // (imu is NULL iff K = 0)
    if (local != 0 && local != 1) return false;
    return stride >= 0;
}
// ... every stamp of the samples and of t1 finite (the samples' rates are the caller's: a NaN rate makes that filter's outputs NaN) ...
inline bool stampsOk(int K, const double* imu /* [K][B][7] */, const double* t1, int B) {
    for (int k = 0; k < K; ++k)
        for (int b = 0; b < B; ++b)
            if (!std::isfinite(imu[(size_t(k) * size_t(B) + size_t(b)) * 7])) return false;
    if (t1)
        for (int b = 0; b < B; ++b)
            if (!std::isfinite(t1[b])) return false;
    return true;
}
// ... and what needs the counts: a per-landmark output wants a row for every landmark of every filter
inline bool strideOk(const Wants& w, int stride, int B, const int* N) {
    if (!w.perLandmark()) return true;
    for (int b = 0; b < B; ++b)
        if (stride < N[b]) return false;
    return true;
}

// one caller sample [7] -> its uploaded record [kImuRec]
inline void packSample(const double* src7, double* dst) {
    for (int i = 0; i < 7; ++i) dst[i] = src7[i];
    dst[7] = 0.0;
}
inline void packStamp(double t1, double* dst) {
    dst[0] = t1;
    for (int i = 1; i < kImuRec; ++i) dst[i] = 0.0;
}

}  // namespace eqf::forecast
