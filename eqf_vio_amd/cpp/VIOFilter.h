// C++ host facade of the MI355X EqF path: the reference's VIOFilter interface over the C ABI.
//
// Mirrors eqf_vio/include/eqf_vio/VIOFilter.h:41-88 (same class and member names, same argument meaning,
// same silent early-outs) so that a caller of the reference -- eqf_vio/src/main.cpp:86,116,129,134,
// eqf_vio_ros/src/eqf_vio_ros_node.cpp:59,90,104 -- compiles against this header after replacing the Eigen
// value types by the plain arrays below (Eigen is not a dependency of this library).  All arithmetic runs in
// the HIP kernels behind include/eqf_vio_amd.h; this header is plumbing only and has no CPU fallback.
#pragma once
#include <array>
#include <cmath>
#include <limits>
#include <memory>
#include <ostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/eqf_vio_amd.h"

namespace eqf_vio_amd {

using Vector3d = std::array<double, 3>;
struct Quaterniond {  // Eigen::Quaterniond order of the reference's CSV output: w, x, y, z
    double w = 1, x = 0, y = 0, z = 0;
};
struct SE3 {  // libs/core/include/SE3.h: rotation (quaternion backed, SO3.cpp:25) + translation
    Quaterniond R;
    Vector3d x{0, 0, 0};
};

constexpr double GRAVITY_CONSTANT = 9.81;  // eqf_vio/include/eqf_vio/IMUVelocity.h:22

struct IMUVelocity {  // eqf_vio/include/eqf_vio/IMUVelocity.h:24-37
    double stamp = 0;
    Vector3d omega{0, 0, 0};
    Vector3d accel{0, 0, 0};
};

struct Point3d {  // eqf_vio/include/eqf_vio/VIOState.h:38-41
    Vector3d p{0, 0, 0};
    int id = -1;
};

struct VisionMeasurement {  // eqf_vio/include/eqf_vio/VisionMeasurement.h:24-28 (bearings sorted by ascending id)
    double stamp = 0;
    int numberOfBearings = 0;
    std::vector<Point3d> bearings;
};

struct VIOState {  // eqf_vio/include/eqf_vio/VIOState.h:51-60
    SE3 pose;
    Vector3d velocity{0, 0, 0};
    std::vector<Point3d> bodyLandmarks;
    SE3 cameraOffset;
};

struct SOT3 {  // libs/core/include/SOT3.h
    Quaterniond R;
    double a = 1;
};
struct VIOGroup {  // eqf_vio/include/eqf_vio/VIOGroup.h:24-33
    SE3 A;
    Vector3d w{0, 0, 0};
    std::vector<SOT3> Q;
    std::vector<int> id;
};

// Dense row-major covariance returned by stateCovariance() (the reference returns Eigen::MatrixXd).
struct MatrixXd {
    int n = 0;
    std::vector<double> data;
    double operator()(int i, int j) const { return data[size_t(i) * n + j]; }
    int rows() const { return n; }
    int cols() const { return n; }
};

struct AuxiliaryFilterData {  // eqf_vio/include/eqf_vio/VIOFilter.h:30-39
    Quaterniond initialAttitude;
    Vector3d initialPosition{0, 0, 0};
    double initialTime = 0;
    double measurementVariance = 0.1;
    double processVariance = 1.0;
    double omegaVariance = 0.1;
    double accelVariance = 0.1;
    SE3 cameraOffset;
};

class VIOFilter {
  public:
    // eqf_vio/include/eqf_vio/VIOFilterSettings.h:28-54.  YAML parsing is host plumbing outside this path: fill
    // the fields directly (same names and defaults as the reference).
    struct Settings : eqf_settings {
        Settings() { eqf_settings_default(this); }
        SE3 cameraOffsetSE3() const {
            SE3 T;
            T.R = {cameraOffset_q[0], cameraOffset_q[1], cameraOffset_q[2], cameraOffset_q[3]};
            T.x = {cameraOffset_x[0], cameraOffset_x[1], cameraOffset_x[2]};
            return T;
        }
    };
    std::unique_ptr<Settings> settings;

    // VIOFilter(const VIOFilter::Settings&) (VIOFilter.cpp:60-73).  capacity = most landmarks ever tracked at once
    // (the reference grows Sigma on demand; device buffers are sized once).
    explicit VIOFilter(const Settings& s, int capacity = 256, int device = 0, int precision = EQF_PRECISION_F64)
        : settings(std::make_unique<Settings>(s)) {
        eqf_filter* h = nullptr;
        const int rc = eqf_create(settings.get(), capacity, 1, device, precision, &h);
        if (rc != EQF_OK) throw std::runtime_error("eqf_create failed with status " + std::to_string(rc) + " (no CPU fallback)");
        handle_.reset(h);
    }
    // VIOFilter(const AuxiliaryFilterData&, const VIOFilter::Settings&) (VIOFilter.cpp:51-58)
    VIOFilter(const AuxiliaryFilterData& auxiliaryData, const Settings& s, int capacity = 256, int device = 0,
        int precision = EQF_PRECISION_F64)
        : VIOFilter(s, capacity, device, precision) {
        setAuxiliaryData(auxiliaryData);
    }
    VIOFilter(VIOFilter&&) = default;             // move-only, like the reference (unique_ptr settings)
    VIOFilter& operator=(VIOFilter&&) = default;  // eqf_vio_ros_node.cpp:59 move-assigns

    void reset() { check(eqf_reset(handle_.get()), "eqf_reset"); }  // VIOFilter.cpp:84-91

    // VIOFilter.cpp:133-144: origin pose = identity position + the attitude that takes the measured specific-force
    // direction to e3, zero origin velocity, initialised.  processIMUData does this lazily on the device at the first
    // sample (with the bias-corrected sample); this member is the explicit form of the reference's public method and takes
    // the velocity as given.  Throws std::domain_error like SO3FromVectors (SO3.cpp:160-161) for accel = -|accel| e3.
    void initialiseFromIMUData(const IMUVelocity& imuVelocity) {
        Snapshot st = dump();
        st.pq = so3FromVectors(imuVelocity.accel, {0, 0, 1});
        st.px = {0, 0, 0};
        st.v = {0, 0, 0};
        st.initialised = 1;
        restore(st);
    }

    // VIOFilter.cpp:120-131
    void processIMUData(const IMUVelocity& imuVelocity) {
        check(eqf_process_imu(handle_.get(), &imuVelocity.stamp, imuVelocity.omega.data(), imuVelocity.accel.data(), &lastStatus_),
            "eqf_process_imu");
    }
    // VIOFilter.cpp:232-302.  Throws std::domain_error where the reference's SO3FromVectors would (SO3.cpp:160).
    void processVisionData(const VisionMeasurement& measurement) {
        const int nb = int(measurement.bearings.size());
        ids_.resize(nb);
        y_.resize(size_t(3) * nb);
        for (int i = 0; i < nb; ++i) {
            ids_[i] = measurement.bearings[i].id;
            for (int c = 0; c < 3; ++c) y_[size_t(3) * i + c] = measurement.bearings[i].p[c];
        }
        check(eqf_process_vision(handle_.get(), &measurement.stamp, &nb, ids_.data(), y_.data(), nb, &lastStatus_), "eqf_process_vision");
    }

    // How likely the frame is BEFORE it is applied (eqf_score_vision): the joint NIS, log det S, log-likelihood and dof of the entries whose
    // id the state holds, at the filter's present state -- measurement.stamp is not used: bring the IMU up to date first.  Nothing of the
    // filter changes; entries the state does not hold take no part, landmarks the frame does not name are not removed.
    eqf_frame_score scoreVisionData(const VisionMeasurement& measurement) const {
        const int nb = int(measurement.bearings.size()), stride = nb > 0 ? nb : 1;
        std::vector<int> ids(size_t(stride), 0);
        std::vector<double> y(size_t(3) * stride, 0.0);
        for (int i = 0; i < nb; ++i) {
            ids[i] = measurement.bearings[i].id;
            for (int c = 0; c < 3; ++c) y[size_t(3) * i + c] = measurement.bearings[i].p[c];
        }
        eqf_frame_score rec{};
        check(eqf_score_vision(handle_.get(), 1, &nb, ids.data(), y.data(), stride, nullptr, &rec, nullptr, nullptr), "eqf_score_vision");
        return rec;
    }

    // Handle option by name (include/eqf_vio_amd.h: eqf_set_option), e.g. setOption("downdate_slices", 6): the covariance downdate on the
    // integer matrix pipe from six 7-bit slices per column of Y (off by default: fp64).
    void setOption(const char* name, int value) { check(eqf_set_option(handle_.get(), name, value), "eqf_set_option"); }

    // VIOFilter.cpp:74-82: origin pose from the given attitude / position, zero origin velocity, camera offset replaced,
    // filter marked initialised (so the first IMU sample does no gravity alignment).
    void setAuxiliaryData(const AuxiliaryFilterData& auxiliaryData) {
        auxData = auxiliaryData;
        Snapshot st = dump();
        st.pq = {auxiliaryData.initialAttitude.w, auxiliaryData.initialAttitude.x, auxiliaryData.initialAttitude.y, auxiliaryData.initialAttitude.z};
        st.px = auxiliaryData.initialPosition;
        st.v = {0, 0, 0};
        st.initialised = 1;
        const SE3& T = auxiliaryData.cameraOffset;
        const double cq[4] = {T.R.w, T.R.x, T.R.y, T.R.z};
        check(eqf_set_camera_offset(handle_.get(), cq, T.x.data()), "eqf_set_camera_offset");
        for (int i = 0; i < 4; ++i) settings->cameraOffset_q[i] = cq[i];
        for (int i = 0; i < 3; ++i) settings->cameraOffset_x[i] = T.x[i];
        restore(st);
    }
    // VIOFilter.cpp:93-118: the landmark set becomes the given inertial-frame points (ids as given), Q_i = identity,
    // Sigma = initialPointVariance * I outside the 11 x 11 base block.
    void setInertialPoints(const std::vector<Point3d>& inertialPoints) {
        const int N = int(inertialPoints.size());
        Snapshot st = dump();
        // inertialToCameraTF = (xi0.pose * xi0.cameraOffset)^-1
        const double* cq = settings->cameraOffset_q;
        const double* cx = settings->cameraOffset_x;
        const std::array<double, 4> tq = qmul(st.pq, {cq[0], cq[1], cq[2], cq[3]});
        const Vector3d rx = qrot(st.pq, {cx[0], cx[1], cx[2]});
        const Vector3d tx = {st.px[0] + rx[0], st.px[1] + rx[1], st.px[2] + rx[2]};
        const std::array<double, 4> tqi = {tq[0], -tq[1], -tq[2], -tq[3]};
        st.ids.resize(N);
        st.p0.assign(size_t(3) * N, 0.0);
        st.Qq.assign(size_t(4) * N, 0.0);
        st.Qa.assign(N, 1.0);
        for (int i = 0; i < N; ++i) {
            const Vector3d& p = inertialPoints[i].p;
            const Vector3d q = qrot(tqi, {p[0] - tx[0], p[1] - tx[1], p[2] - tx[2]});
            st.ids[i] = inertialPoints[i].id;
            for (int c = 0; c < 3; ++c) st.p0[size_t(3) * i + c] = q[c];
            st.Qq[size_t(4) * i] = 1.0;
        }
        const int n = 11 + 3 * N;
        std::vector<double> S(size_t(n) * n, 0.0);
        for (int i = 0; i < n; ++i) S[size_t(i) * n + i] = settings->initialPointVariance;
        for (int r = 0; r < 11; ++r)
            for (int c = 0; c < 11; ++c) S[size_t(r) * n + c] = st.sigma[size_t(r) * st.n + c];
        st.sigma.swap(S);
        st.n = n;
        restore(st);
    }

    double getTime() const {  // VIOFilter.cpp:343
        double t = 0;
        eqf_get_time(handle_.get(), &t);
        return t;
    }
    VIOState stateEstimate() const {  // VIOFilter.cpp:304
        VIOState s;
        const int N = eqf_num_landmarks(handle_.get(), 0);
        std::vector<double> p(size_t(3) * (N > 0 ? N : 1));
        std::vector<int> ids(N > 0 ? N : 1);
        double q[4], x[3], v[3];
        check(eqf_get_state_estimate(handle_.get(), 0, q, x, v, p.data()), "eqf_get_state_estimate");
        check(eqf_get_ids(handle_.get(), 0, ids.data()), "eqf_get_ids");
        s.pose.R = {q[0], q[1], q[2], q[3]};
        s.pose.x = {x[0], x[1], x[2]};
        s.velocity = {v[0], v[1], v[2]};
        s.bodyLandmarks.resize(N);
        for (int i = 0; i < N; ++i) {
            s.bodyLandmarks[i].p = {p[3 * i], p[3 * i + 1], p[3 * i + 2]};
            s.bodyLandmarks[i].id = ids[i];
        }
        s.cameraOffset = settings->cameraOffsetSE3();
        check(eqf_device_error(handle_.get()) == 0 ? 0 : EQF_ERR_NUMERIC, "device");
        return s;
    }
    MatrixXd stateCovariance() const {  // VIOFilter.cpp:306-309
        MatrixXd S;
        S.n = 11 + 3 * eqf_num_landmarks(handle_.get(), 0);
        S.data.resize(size_t(S.n) * S.n);
        check(eqf_get_sigma(handle_.get(), 0, S.data.data(), S.n), "eqf_get_sigma");
        return S;
    }
    // The covariance in the coordinates of the ESTIMATE, J Sigma J^T (eqf_get_sigma_local): stateCovariance() -- like the reference's,
    // VIOFilter.cpp:306-309 "TODO: propagate to local tangent space" -- is in the chart around the origin xi0.
    MatrixXd stateCovarianceLocal() const {
        MatrixXd S;
        S.n = 11 + 3 * eqf_num_landmarks(handle_.get(), 0);
        S.data.resize(size_t(S.n) * S.n);
        check(eqf_get_sigma_local(handle_.get(), 0, S.data.data(), S.n), "eqf_get_sigma_local");
        return S;
    }
    // Where the state and the features WILL be (eqf_forecast): what this filter would hold after the IMU samples `imu` and, with hasStamp,
    // the integration up to `stamp` with which processVisionData begins -- the filter itself is only read.  state: the estimate at the time
    // reached; base (11 x 11) and lm (3 x 3 per landmark) its marginal covariances, in the estimate's chart (local) or the origin's;
    // bearing the predicted unit bearings; S (2 x 2 per landmark) what the Mahalanobis gate will divide by; ycov (3 x 3 per landmark) the
    // covariance of the predicted bearing, for a search region.  status: EQF_OK, an EQF_SKIPPED_* code (not initialised: everything zero;
    // no step integrated: the present values) -- EQF_ERR_NUMERIC throws.
    struct Forecast {
        int status = 0, steps = 0;
        double time = 0.0;
        VIOState state;
        std::vector<std::array<double, 3>> bearing;
        std::array<double, 121> base{};
        std::vector<std::array<double, 9>> lm, ycov;
        std::vector<std::array<double, 4>> S;
    };
    Forecast forecast(const std::vector<IMUVelocity>& imu, bool hasStamp, double stamp, bool local = true) const {
        Forecast fc;
        const int N = eqf_num_landmarks(handle_.get(), 0), K = int(imu.size()), M = N > 0 ? N : 1;
        std::vector<double> rec(size_t(7) * (K > 0 ? K : 1)), p(size_t(3) * M), y(size_t(3) * M), lm(size_t(9) * M), S(size_t(4) * M), yc(size_t(9) * M);
        for (int k = 0; k < K; ++k) {
            rec[7 * k] = imu[k].stamp;
            for (int c = 0; c < 3; ++c) {
                rec[7 * k + 1 + c] = imu[k].omega[c];
                rec[7 * k + 4 + c] = imu[k].accel[c];
            }
        }
        std::vector<int> ids(M);
        double q[4], x[3], v[3];
        eqf_forecast_out out{&fc.time, &fc.steps, q, x, v, p.data(), y.data(), fc.base.data(), lm.data(), S.data(), yc.data()};
        check(eqf_forecast(handle_.get(), K, K > 0 ? rec.data() : nullptr, hasStamp ? &stamp : nullptr, local ? 1 : 0, M, &out, &fc.status),
            "eqf_forecast");
        check(fc.status < 0 ? fc.status : 0, "eqf_forecast");
        check(eqf_get_ids(handle_.get(), 0, ids.data()), "eqf_get_ids");
        fc.state.pose.R = {q[0], q[1], q[2], q[3]};
        fc.state.pose.x = {x[0], x[1], x[2]};
        fc.state.velocity = {v[0], v[1], v[2]};
        fc.state.cameraOffset = settings->cameraOffsetSE3();
        fc.state.bodyLandmarks.resize(N);
        fc.bearing.resize(N);
        fc.lm.resize(N);
        fc.ycov.resize(N);
        fc.S.resize(N);
        for (int i = 0; i < N; ++i) {
            fc.state.bodyLandmarks[i].p = {p[3 * i], p[3 * i + 1], p[3 * i + 2]};
            fc.state.bodyLandmarks[i].id = ids[i];
            fc.bearing[i] = {y[3 * i], y[3 * i + 1], y[3 * i + 2]};
            for (int e = 0; e < 9; ++e) {
                fc.lm[i][e] = lm[9 * i + e];
                fc.ycov[i][e] = yc[9 * i + e];
            }
            for (int e = 0; e < 4; ++e) fc.S[i][e] = S[4 * i + e];
        }
        return fc;
    }
    // The features of the frame that is about to be matched, stamped `stamp`: predicted bearings, gate matrices and search covariances
    // from the samples the filter already has (the K = 0 forecast).
    Forecast predictFeatures(double stamp) const { return forecast({}, true, stamp, true); }
    // Innovation statistics of the most recent vision update (setOption("innovation_stats", 1) first; eqf_get_innovation_stats):
    // NIS, log det S, log-likelihood, degrees of freedom and the per-landmark NIS in the state's landmark order.
    struct InnovationStats : eqf_innovation_stats {
        std::vector<double> nis_lm;
    };
    InnovationStats innovationStats() const {
        InnovationStats st;
        const int N = eqf_num_landmarks(handle_.get(), 0);
        st.nis_lm.assign(size_t(N > 0 ? N : 1), 0.0);
        check(eqf_get_innovation_stats(handle_.get(), 0, &st, st.nis_lm.data()), "eqf_get_innovation_stats");
        st.nis_lm.resize(st.valid ? size_t(N) : 0);
        return st;
    }
    // The outlier gate (eqf_set_outlier_gate): EQF_GATE_CHORD, the reference's removeOutliers with settings->outlierThreshold (the default),
    // or EQF_GATE_MAHALANOBIS, delta_i^T (C_i Sigma_ii C_i^T + r I)^-1 delta_i against a chi-square threshold (2 degrees of freedom:
    // -2 ln(1 - p)).  From the next vision call on; throws std::runtime_error for an unknown kind, a NaN or (kind 1) non-positive threshold.
    void setOutlierGate(int kind, double threshold) { check(eqf_set_outlier_gate(handle_.get(), kind, threshold), "eqf_set_outlier_gate"); }
    // What the gate of the most recent vision call examined (eqf_get_gate_report): ids, chord or d2, and whether the landmark was thrown
    // out, in the state's order before the removals; empty when the gate was disarmed or the call skipped.
    struct GateReport {
        std::vector<int> ids;
        std::vector<double> stat;
        std::vector<int> removed;
    };
    GateReport gateReport() const {
        GateReport r;
        int n = 0;
        check(eqf_get_gate_report(handle_.get(), 0, &n, nullptr, nullptr, nullptr), "eqf_get_gate_report");
        r.ids.resize(n);
        r.stat.resize(n);
        r.removed.resize(n);
        check(eqf_get_gate_report(handle_.get(), 0, &n, r.ids.data(), r.stat.data(), r.removed.data()), "eqf_get_gate_report");
        return r;
    }
    // Joint NEES err^T A^-1 err with log det A, the smallest pivot and the definiteness word (eqf_get_nees): A = the covariance in the
    // coordinates of the estimate (local) or of the origin, from reference index `first` (0 whole state | 6 without the bias | 11 landmarks
    // only) on; err has 11 + 3 N entries in Sigma's index map (those below `first` are ignored).  A matrix that is not positive definite is
    // reported in `info`, not thrown.
    struct StateNEES : eqf_sigma_stats {
        double nees = 0.0;
    };
    template <typename Vec>
    StateNEES stateNEES(const Vec& err, bool local = true, int first = 0) const {
        StateNEES st;
        const int n = 11 + 3 * eqf_num_landmarks(handle_.get(), 0);
        if (int(err.size()) < n) throw std::invalid_argument("stateNEES: err needs 11 + 3 N entries");
        std::vector<double> e(size_t(n), 0.0);
        for (int i = 0; i < n; ++i) e[i] = err[i];
        check(eqf_get_nees(handle_.get(), local ? 1 : 0, first, 1, e.data(), n, &st.nees, &st), "eqf_get_nees");
        return st;
    }
    // A draw from the covariance (eqf_sample_sigma): scale * L z with L L^T = the covariance in the coordinates of the estimate (local) or of
    // the origin, from reference index `first` on; z has 11 + 3 N standard normal entries in Sigma's index map (those below `first` are
    // ignored, the result is 0 there).  With local = true this is a sampled estimation error (eqf_vio_amd.consistency.local_retract turns
    // it into a sampled truth).  A matrix that is not positive definite is reported in `info` (the draw is NaN then), not thrown.
    struct StateSample : eqf_sigma_stats {
        std::vector<double> eps;
    };
    template <typename Vec>
    StateSample sampleStateError(const Vec& z, bool local = true, int first = 0, double scale = 1.0) const {
        StateSample st;
        const int n = 11 + 3 * eqf_num_landmarks(handle_.get(), 0);
        if (int(z.size()) < n) throw std::invalid_argument("sampleStateError: z needs 11 + 3 N entries");
        std::vector<double> zz(size_t(n), 0.0);
        for (int i = 0; i < n; ++i) zz[i] = z[i];
        st.eps.assign(size_t(n), 0.0);
        check(eqf_sample_sigma(handle_.get(), local ? 1 : 0, first, 1, zz.data(), n, &scale, st.eps.data(), n, &st), "eqf_sample_sigma");
        return st;
    }
    // Moves the filter by scale * L z, L L^T = the covariance in the coordinates of the origin from `first` on, on the device
    // (eqf_perturb_filters): bias += gamma[0:6], X <- VIOExp(liftInnovation(gamma[6:], xi0)) X; the covariance, the origin, the clock and the
    // integrator stay.  Two forks of one filter (copyStateFrom) that see the same stream stay equal for ever; this tells them apart.  The
    // filter is not moved when the covariance is not positive definite (`info`).
    template <typename Vec>
    eqf_sigma_stats perturbState(const Vec& z, int first = 0, double scale = 1.0) {
        eqf_sigma_stats st;
        const int n = 11 + 3 * eqf_num_landmarks(handle_.get(), 0);
        if (int(z.size()) < n) throw std::invalid_argument("perturbState: z needs 11 + 3 N entries");
        std::vector<double> zz(size_t(n), 0.0);
        for (int i = 0; i < n; ++i) zz[i] = z[i];
        check(eqf_perturb_filters(handle_.get(), first, zz.data(), n, &scale, &st), "eqf_perturb_filters");
        return st;
    }
    // A measurement update with m <= 16 linear rows (eqf_update_linear): resid = H eps + noise, noise ~ N(0, R), eps "truth minus estimate"
    // in the coordinates of stateCovarianceLocal() (local: gravity direction 6..7, body velocity 8..10, body-frame landmark i 11 + 3 i ..) or
    // of stateCovariance().  H: m rows of 11 + 3 N entries, row-major without gaps; resid: m; R: m x m row-major, lower triangle read; gate: a
    // chi-square threshold on the m-dof nis (the default never trips).  The filter is untouched when the report's info is not 0.
    eqf_linear_report processLinearMeasurement(const double* H, int m, const double* resid, const double* R, bool local = true,
        double gate = std::numeric_limits<double>::infinity()) {
        eqf_linear_report rep;
        const int n = 11 + 3 * eqf_num_landmarks(handle_.get(), 0);
        check(eqf_update_linear(handle_.get(), local ? 1 : 0, m, H, n, resid, R, gate, nullptr, nullptr, 0, &rep), "eqf_update_linear");
        return rep;
    }
    // A measurement update from per-landmark blocks (eqf_update_landmarks): entry k measures the landmark ids[k] (strictly ascending) alone,
    // resid_k = H_k eps_i + noise, noise ~ N(0, R_k), with `rows` (1, 2 or 3) rows per entry -- the second camera of a stereo rig, a range, a
    // surveyed position.  H: K blocks of rows x 3, resid: K x rows, R: K blocks of rows x rows (lower triangles read), all row-major without
    // gaps; local: eps_i is the plain difference of camera-frame positions (the estimate's chart), else the origin chart's block.  gate: a
    // chi-square threshold on the joint nis, lm_gate: on every entry's own distance (the defaults never trip).  used (K bytes, or nullptr):
    // 1 applied, 0 id not in the state, 2 gated.  The filter is untouched when the report's info is not 0.
    eqf_linear_report processLandmarkMeasurements(const int* ids, int K, int rows, const double* H, const double* resid, const double* R,
        bool local = true, double gate = std::numeric_limits<double>::infinity(), double lm_gate = std::numeric_limits<double>::infinity(),
        unsigned char* used = nullptr) {
        eqf_linear_report rep;
        const int zero = 0;
        std::vector<double> pad(9, 0.0);  // (stride is at least 1: K = 0 hands over one unread entry)
        check(eqf_update_landmarks(handle_.get(), local ? 1 : 0, rows, &K, K ? ids : &zero, K ? K : 1, K ? H : pad.data(), K ? resid : pad.data(),
                  K ? R : pad.data(), gate, lm_gate, nullptr, K ? used : nullptr, nullptr, 0, &rep),
            "eqf_update_landmarks");
        return rep;
    }
    // The Schmidt (consider) variants of the two updates above (eqf_update_linear_schmidt / eqf_update_landmarks_schmidt): the landmarks
    // considerIds (strictly ascending; one the state does not hold is ignored) keep their estimate and their covariance block, while their
    // cross-correlations still enter S and the gain of everything else -- a large persistent map, a surveyed point.  The measurement may
    // observe them.  The report is the full update's.
    eqf_linear_report processLinearMeasurement(const double* H, int m, const double* resid, const double* R,
        const std::vector<int>& considerIds, bool local = true, double gate = std::numeric_limits<double>::infinity()) {
        eqf_linear_report rep;
        const int n = 11 + 3 * eqf_num_landmarks(handle_.get(), 0), nc = int(considerIds.size());
        check(eqf_update_linear_schmidt(handle_.get(), local ? 1 : 0, m, H, n, resid, R, gate, nullptr, &nc, considerIds.data(), nc, nullptr,
                  0, &rep),
            "eqf_update_linear_schmidt");
        return rep;
    }
    eqf_linear_report processLandmarkMeasurements(const int* ids, int K, int rows, const double* H, const double* resid, const double* R,
        const std::vector<int>& considerIds, bool local = true, double gate = std::numeric_limits<double>::infinity(),
        double lm_gate = std::numeric_limits<double>::infinity(), unsigned char* used = nullptr) {
        eqf_linear_report rep;
        const int zero = 0, nc = int(considerIds.size());
        std::vector<double> pad(9, 0.0);  // (stride is at least 1: K = 0 hands over one unread entry)
        check(eqf_update_landmarks_schmidt(handle_.get(), local ? 1 : 0, rows, &K, K ? ids : &zero, K ? K : 1, K ? H : pad.data(),
                  K ? resid : pad.data(), K ? R : pad.data(), gate, lm_gate, nullptr, &nc, considerIds.data(), nc, K ? used : nullptr, nullptr,
                  0, &rep),
            "eqf_update_landmarks_schmidt");
        return rep;
    }
    // processLandmarkMeasurements with the rows formed on the device at the filter's own estimate (eqf_observe_landmarks): kind
    // EQF_OBS_BEARING / _RANGE / _POSITION, meas [K][3] (a bearing, a range in meas[3 k], a position in the measuring camera's frame), R
    // [K][rows][rows] (lower triangles), cam NULL (this camera) or [7] = (q_c: w, x, y, z; t_c), the measuring camera's pose in this
    // camera's frame.  used [K]: 1 applied, 0 id not in the state, 2 gated, 3 not observable; Ht [K][rows][3] and resid [K][rows], where
    // given, receive the rows the device formed.  The overload with considerIds is the Schmidt variant.
    eqf_linear_report processLandmarkObservations(int kind, const int* ids, int K, const double* meas, const double* R, const double* cam = nullptr,
        double gate = std::numeric_limits<double>::infinity(), double lm_gate = std::numeric_limits<double>::infinity(),
        unsigned char* used = nullptr, double* Ht = nullptr, double* resid = nullptr) {
        return observeLandmarks(kind, ids, K, meas, R, cam, nullptr, gate, lm_gate, used, Ht, resid);
    }
    eqf_linear_report processLandmarkObservations(int kind, const int* ids, int K, const double* meas, const double* R, const double* cam,
        const std::vector<int>& considerIds, double gate = std::numeric_limits<double>::infinity(),
        double lm_gate = std::numeric_limits<double>::infinity(), unsigned char* used = nullptr, double* Ht = nullptr, double* resid = nullptr) {
        return observeLandmarks(kind, ids, K, meas, R, cam, &considerIds, gate, lm_gate, used, Ht, resid);
    }
    // ... ITERATED (eqf_observe_landmarks_iterated): the rows are re-formed at the estimate the update would give, at most max_lin (1 ..
    // EQF_ITER_MAX_LIN) linearisations, until the increment on the named landmarks changes by no more than tol (chart units; 0: never stop
    // early), and only the last linearisation is applied.  Returns the iteration report {n_lin, status, last_step}: status 0 converged, 1 ran
    // out of linearisations, 2 stalled at a trial point that was not observable, 3 an intermediate solve failed; report, where given,
    // receives the update's own report.  considerIds: NULL, or the Schmidt variant's list.  resid receives r~ = resid + Ht g of the
    // committed linearisation.
    eqf_iter_report processLandmarkObservations(int kind, const int* ids, int K, const double* meas, const double* R, const double* cam,
        int max_lin, double tol, eqf_linear_report* report = nullptr, const std::vector<int>* considerIds = nullptr,
        double gate = std::numeric_limits<double>::infinity(), double lm_gate = std::numeric_limits<double>::infinity(),
        unsigned char* used = nullptr, double* Ht = nullptr, double* resid = nullptr) {
        eqf_linear_report rep;
        eqf_iter_report iter;
        const int zero = 0, nc = considerIds ? int(considerIds->size()) : 0;
        std::vector<double> pad(9, 0.0);  // (stride is at least 1: K = 0 hands over one unread entry)
        check(eqf_observe_landmarks_iterated(handle_.get(), kind, cam, 0, &K, K ? ids : &zero, K ? K : 1, K ? meas : pad.data(),
                  K ? R : pad.data(), gate, lm_gate, nullptr, considerIds ? &nc : nullptr, considerIds ? considerIds->data() : nullptr, nc,
                  max_lin, tol, K ? used : nullptr, K ? Ht : nullptr, K ? resid : nullptr, nullptr, 0, &rep, nullptr, &iter),
            "eqf_observe_landmarks_iterated");
        if (report) *report = rep;
        return iter;
    }
    // How processLinearMeasurement, processLandmarkMeasurements, perturbState (and eqf_apply_increment) turn their increment into a group
    // step (eqf_set_option "innovation_lift"): false (default) the plain lift, which leaves the whole correction to the body-frame landmarks;
    // true the filter's own useInnovationLift / useDiscreteInnovationLift, as a vision frame does -- a stereo, range or zero-velocity update
    // then moves the pose.  A lift that fails (Sigma_e not positive definite) leaves the filter untouched: info = 4 in the reports.
    void setUpdateLift(bool on) { check(eqf_set_option(handle_.get(), "innovation_lift", on ? 1 : 0), "eqf_set_option"); }
    // The lift of the most recent of those calls (eqf_get_lift_report): kind, info, DeltaU, the smallest pivot of Sigma_e's factor and the
    // pivot ratio of the 4 x 4 solve.  Throws std::runtime_error before the first such call.
    eqf_lift_report lastLiftReport() const {
        eqf_lift_report rep;
        check(eqf_get_lift_report(handle_.get(), 0, &rep), "eqf_get_lift_report");
        return rep;
    }
    // This filter continues from the state of `other` (fork, or snapshot and roll back), copied on the device (eqf_copy_filters): landmarks,
    // origin, group element, bias, covariance, time and integrator.  Settings, camera offset and capacity stay this filter's own; throws
    // std::runtime_error if `other` tracks more landmarks than this filter's capacity or differs in precision or device.
    void copyStateFrom(const VIOFilter& other) {
        const int zero = 0;
        check(eqf_copy_filters(handle_.get(), other.handle_.get(), 1, &zero, &zero), "eqf_copy_filters");
    }
    // The landmarks `ids` (strictly ascending) leave the filter, on the device (eqf_edit_landmarks): their rows and columns of the covariance
    // go, the order of the rest is kept.  Returns one verdict per id: 1 gone, 0 not in the state (no error).  Throws std::runtime_error for
    // ids that are not strictly ascending.
    std::vector<unsigned char> removeLandmarks(const std::vector<int>& ids) {
        const int K = int(ids.size()), zero = 0;
        std::vector<unsigned char> removed(size_t(K ? K : 1), 0);
        check(eqf_edit_landmarks(handle_.get(), &K, K ? ids.data() : &zero, K ? K : 1, nullptr, nullptr, 0, nullptr, nullptr, removed.data(),
                  nullptr),
            "eqf_edit_landmarks");
        removed.resize(size_t(K));
        return removed;
    }
    // New landmarks `ids` (strictly ascending) behind the ones the filter has, in the order given, where the CALLER measured them: p (3 per
    // id) the camera-frame positions, P (3 x 3 per id, row-major, lower triangles read) the covariances of their errors (a range, a stereo
    // triangulation); no cross-covariance with the rest of the state.  Returns one verdict per id: 1 done, 0 the id is already in the state, 2
    // values rejected (not finite, p = 0, P not positive definite).  Throws std::runtime_error for ids that are not strictly ascending, or
    // beyond the capacity.
    std::vector<unsigned char> insertLandmarks(const std::vector<int>& ids, const double* p, const double* P) {
        const int K = int(ids.size()), zero = 0;
        std::vector<unsigned char> inserted(size_t(K ? K : 1), 0);
        std::vector<double> pad(9, 0.0);  // (K = 0 hands over one unread entry)
        check(eqf_edit_landmarks(handle_.get(), nullptr, nullptr, 0, &K, K ? ids.data() : &zero, K ? K : 1, K ? p : pad.data(), K ? P : pad.data(),
                  nullptr, inserted.data()),
            "eqf_edit_landmarks");
        inserted.resize(size_t(K));
        return inserted;
    }
    int lastStatus() const { return lastStatus_; }  // EQF_SKIPPED_* where the reference returns early
    eqf_filter* handle() const { return handle_.get(); }

    // operator<<(ostream&, const VIOFilter&) (VIOFilter.cpp:311-341): xi0, X, N, per-landmark (id, p0, Q, a), Sigma
    friend std::ostream& operator<<(std::ostream& os, const VIOFilter& f) {
        const int N = eqf_num_landmarks(f.handle_.get(), 0);
        std::vector<double> p(size_t(3) * (N > 0 ? N : 1)), Qq(size_t(4) * (N > 0 ? N : 1)), Qa(N > 0 ? N : 1);
        std::vector<int> ids(N > 0 ? N : 1);
        double q[4], x[3], v[3], Aq[4], Ax[3], w[3];
        eqf_get_origin(f.handle_.get(), 0, q, x, v, p.data());
        eqf_get_group(f.handle_.get(), 0, Aq, Ax, w, Qq.data(), Qa.data());
        eqf_get_ids(f.handle_.get(), 0, ids.data());
        os << x[0] << ", " << x[1] << ", " << x[2] << ", " << q[0] << ", " << q[1] << ", " << q[2] << ", " << q[3] << ", ";
        os << v[0] << ", " << v[1] << ", " << v[2] << ", ";
        os << Ax[0] << ", " << Ax[1] << ", " << Ax[2] << ", " << Aq[0] << ", " << Aq[1] << ", " << Aq[2] << ", " << Aq[3] << ", ";
        os << w[0] << ", " << w[1] << ", " << w[2] << ", " << N;
        for (int i = 0; i < N; ++i) {
            os << ", " << ids[i] << ", " << p[3 * i] << ", " << p[3 * i + 1] << ", " << p[3 * i + 2];
            os << ", " << Qq[4 * i] << ", " << Qq[4 * i + 1] << ", " << Qq[4 * i + 2] << ", " << Qq[4 * i + 3] << ", " << Qa[i];
        }
        const MatrixXd S = f.stateCovariance();
        for (double s : S.data) os << ", " << s;
        return os;
    }

    AuxiliaryFilterData auxData;  // VIOFilter.h:43

  private:
    // full-precision snapshot of the filter (what eqf_set_state takes)
    struct Snapshot {
        std::vector<int> ids;
        std::array<double, 4> pq{1, 0, 0, 0}, Aq{1, 0, 0, 0};
        Vector3d px{0, 0, 0}, v{0, 0, 0}, Ax{0, 0, 0}, w{0, 0, 0};
        std::vector<double> p0, Qq, Qa, sigma;
        double bias[6], curVel[6], accVel[6], accTime = 0, time = -1;
        int initialised = 0, n = 11;
    };
    Snapshot dump() const {
        Snapshot st;
        eqf_filter* h = handle_.get();
        const int N = eqf_num_landmarks(h, 0);
        const int M = N > 0 ? N : 1;
        st.ids.resize(M);
        st.p0.resize(size_t(3) * M);
        st.Qq.resize(size_t(4) * M);
        st.Qa.resize(M);
        check(eqf_get_ids(h, 0, st.ids.data()), "eqf_get_ids");
        check(eqf_get_origin(h, 0, st.pq.data(), st.px.data(), st.v.data(), st.p0.data()), "eqf_get_origin");
        check(eqf_get_group(h, 0, st.Aq.data(), st.Ax.data(), st.w.data(), st.Qq.data(), st.Qa.data()), "eqf_get_group");
        check(eqf_get_bias(h, 0, st.bias), "eqf_get_bias");
        check(eqf_get_integrator(h, 0, st.curVel, st.accVel, &st.accTime, &st.initialised), "eqf_get_integrator");
        check(eqf_get_time(h, &st.time), "eqf_get_time");
        st.ids.resize(N);
        st.n = 11 + 3 * N;
        st.sigma.resize(size_t(st.n) * st.n);
        check(eqf_get_sigma(h, 0, st.sigma.data(), st.n), "eqf_get_sigma");
        return st;
    }
    void restore(const Snapshot& st) {
        const int N = int(st.ids.size());
        check(eqf_set_state(handle_.get(), 0, N, st.ids.data(), st.pq.data(), st.px.data(), st.v.data(), st.p0.data(), st.Aq.data(),
                  st.Ax.data(), st.w.data(), st.Qq.data(), st.Qa.data(), st.bias, st.sigma.data(), st.n, st.time, st.curVel, st.accVel,
                  st.accTime, st.initialised),
            "eqf_set_state");
    }
    static std::array<double, 4> qmul(const std::array<double, 4>& a, const std::array<double, 4>& b) {
        return {a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]};
    }
    // SO3::SO3FromVectors (libs/core/src/SO3.cpp:155-167): R = I + v^ + v^ v^ / (1 + c) for the normalised inputs, stored as
    // a quaternion the way Eigen converts a rotation matrix (SO3.cpp:100).
    static std::array<double, 4> so3FromVectors(const Vector3d& origin, const Vector3d& dest) {
        auto unit = [](const Vector3d& a) {
            const double n = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
            return Vector3d{a[0] / n, a[1] / n, a[2] / n};
        };
        const Vector3d o = unit(origin), d = unit(dest);
        const Vector3d v = {o[1] * d[2] - o[2] * d[1], o[2] * d[0] - o[0] * d[2], o[0] * d[1] - o[1] * d[0]};
        const double c = o[0] * d[0] + o[1] * d[1] + o[2] * d[2];
        if (std::fabs(1 + c) <= 1e-8) throw std::domain_error("The vectors cannot be exactly opposing.");
        const double k = 1 / (1 + c);
        double m[3][3];
        const double vx[3][3] = {{0, -v[2], v[1]}, {v[2], 0, -v[0]}, {-v[1], v[0], 0}};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                double sq = 0;
                for (int l = 0; l < 3; ++l) sq += vx[i][l] * vx[l][j];
                m[i][j] = (i == j ? 1.0 : 0.0) + vx[i][j] + k * sq;
            }
        std::array<double, 4> q{};
        double t = m[0][0] + m[1][1] + m[2][2];
        if (t > 0) {
            t = std::sqrt(t + 1.0);
            q[0] = 0.5 * t;
            t = 0.5 / t;
            q[1] = (m[2][1] - m[1][2]) * t;
            q[2] = (m[0][2] - m[2][0]) * t;
            q[3] = (m[1][0] - m[0][1]) * t;
        } else {
            int i = 0;
            if (m[1][1] > m[0][0]) i = 1;
            if (m[2][2] > m[i][i]) i = 2;
            const int j = (i + 1) % 3, l = (j + 1) % 3;
            t = std::sqrt(m[i][i] - m[j][j] - m[l][l] + 1.0);
            q[1 + i] = 0.5 * t;
            t = 0.5 / t;
            q[0] = (m[l][j] - m[j][l]) * t;
            q[1 + j] = (m[j][i] + m[i][j]) * t;
            q[1 + l] = (m[l][i] + m[i][l]) * t;
        }
        return q;
    }
    static Vector3d qrot(const std::array<double, 4>& q, const Vector3d& v) {
        const Vector3d u = {q[1], q[2], q[3]};
        const Vector3d t = {2 * (u[1] * v[2] - u[2] * v[1]), 2 * (u[2] * v[0] - u[0] * v[2]), 2 * (u[0] * v[1] - u[1] * v[0])};
        return {v[0] + q[0] * t[0] + u[1] * t[2] - u[2] * t[1], v[1] + q[0] * t[1] + u[2] * t[0] - u[0] * t[2],
            v[2] + q[0] * t[2] + u[0] * t[1] - u[1] * t[0]};
    }
    struct Deleter {
        void operator()(eqf_filter* h) const { eqf_destroy(h); }
    };
    static void check(int rc, const char* what) {
        if (rc == EQF_ERR_NUMERIC) throw std::domain_error("The vectors cannot be exactly opposing.");  // SO3.cpp:160-161
        if (rc < 0) throw std::runtime_error(std::string(what) + " failed with status " + std::to_string(rc));
    }
    eqf_linear_report observeLandmarks(int kind, const int* ids, int K, const double* meas, const double* R, const double* cam,
        const std::vector<int>* considerIds, double gate, double lm_gate, unsigned char* used, double* Ht, double* resid) {
        eqf_linear_report rep;
        const int zero = 0, nc = considerIds ? int(considerIds->size()) : 0;
        std::vector<double> pad(9, 0.0);  // (stride is at least 1: K = 0 hands over one unread entry)
        check(eqf_observe_landmarks(handle_.get(), kind, cam, 0, &K, K ? ids : &zero, K ? K : 1, K ? meas : pad.data(), K ? R : pad.data(), gate,
                  lm_gate, nullptr, considerIds ? &nc : nullptr, considerIds ? considerIds->data() : nullptr, nc, K ? used : nullptr,
                  K ? Ht : nullptr, K ? resid : nullptr, nullptr, 0, &rep),
            "eqf_observe_landmarks");
        return rep;
    }
    std::unique_ptr<eqf_filter, Deleter> handle_;
    std::vector<int> ids_;
    std::vector<double> y_;
    int lastStatus_ = 0;
};

}  // namespace eqf_vio_amd
