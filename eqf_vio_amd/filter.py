"""Python mirror of the reference's VIOFilter interface on the MI355X path.

Same member names and argument meaning as eqf_vio/include/eqf_vio/VIOFilter.h:64-88 so that parity tests read
like tests of the reference: VIOFilter(settings), processIMUData, processVisionData, getTime, stateEstimate,
stateCovariance.  All arithmetic happens in the HIP kernels behind the C ABI (no CPU fallback).
"""
from dataclasses import dataclass, field

import numpy as np

from . import binding


@dataclass
class IMUVelocity:
    """eqf_vio/include/eqf_vio/IMUVelocity.h:24-37"""

    stamp: float = 0.0
    omega: np.ndarray = field(default_factory=lambda: np.zeros(3))
    accel: np.ndarray = field(default_factory=lambda: np.zeros(3))


@dataclass
class VisionMeasurement:
    """eqf_vio/include/eqf_vio/VisionMeasurement.h:24-28: bearings sorted by ascending id."""

    stamp: float = 0.0
    ids: np.ndarray = field(default_factory=lambda: np.zeros(0, dtype=np.int32))
    bearings: np.ndarray = field(default_factory=lambda: np.zeros((0, 3)))

    @property
    def numberOfBearings(self):
        return len(self.ids)


@dataclass
class VIOState:
    """eqf_vio/include/eqf_vio/VIOState.h:51-60 with the pose as (quaternion wxyz, position)."""

    pose_q: np.ndarray
    pose_x: np.ndarray
    velocity: np.ndarray
    bodyLandmarks: np.ndarray  # (N, 3)
    ids: np.ndarray


@dataclass
class AuxiliaryFilterData:
    """eqf_vio/include/eqf_vio/VIOFilter.h:30-39 (the fields the filter reads: VIOFilter.cpp:74-82)."""

    initialAttitude: np.ndarray = field(default_factory=lambda: np.array([1.0, 0.0, 0.0, 0.0]))  # quaternion wxyz
    initialPosition: np.ndarray = field(default_factory=lambda: np.zeros(3))
    initialTime: float = 0.0
    cameraOffset_q: np.ndarray = field(default_factory=lambda: np.array([1.0, 0.0, 0.0, 0.0]))
    cameraOffset_x: np.ndarray = field(default_factory=lambda: np.zeros(3))


def _qmul(a, b):
    return np.array([
        a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
        a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
        a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3],
        a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1],
    ])


def _qrot(q, v):
    u, w = np.asarray(q[1:]), q[0]
    t = 2.0 * np.cross(u, v)
    return v + w * t + np.cross(u, t)


class VIOFilter:
    """Drop-in for the reference's VIOFilter on one MI355X (batch of one)."""

    def __init__(self, settings, capacity=256, device=0, precision=binding.PRECISION_F64, auxiliaryData=None):
        self._fb = binding.FilterBatch(settings, capacity, 1, device, precision)
        self._settings = self._fb.settings
        if auxiliaryData is not None:  # VIOFilter(AuxiliaryFilterData, Settings), VIOFilter.cpp:51-58
            self.setAuxiliaryData(auxiliaryData)

    def setAuxiliaryData(self, aux):
        """VIOFilter.cpp:74-82: origin pose from the given attitude/position, zero velocity, camera offset replaced,
        filter marked initialised (no gravity alignment at the first IMU sample)."""
        st = self._fb.dump_state(0)
        st["origin"]["q"] = np.asarray(aux.initialAttitude, dtype=np.float64)
        st["origin"]["x"] = np.asarray(aux.initialPosition, dtype=np.float64)
        st["origin"]["v"] = np.zeros(3)
        st["initialised"] = 1
        self._fb.set_camera_offset(aux.cameraOffset_q, aux.cameraOffset_x)
        self._cam = (np.asarray(aux.cameraOffset_q, dtype=np.float64), np.asarray(aux.cameraOffset_x, dtype=np.float64))
        self._fb.restore_state(st, 0)

    def setInertialPoints(self, points, ids):
        """VIOFilter.cpp:93-118: replace the landmark set by points given in the inertial frame (ids as given);
        Q_i = identity, Sigma = initialPointVariance * I outside the 11x11 base block."""
        points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
        ids = np.asarray(ids, dtype=np.int32)
        N = len(ids)
        st = self._fb.dump_state(0)
        cq, cx = getattr(self, "_cam", (np.asarray(self._settings.cameraOffset_q[:]), np.asarray(self._settings.cameraOffset_x[:])))
        pq, px = st["origin"]["q"], st["origin"]["x"]
        tq, tx = _qmul(pq, cq), px + _qrot(pq, cx)  # xi0.pose * xi0.cameraOffset
        tqi = np.array([tq[0], -tq[1], -tq[2], -tq[3]])
        st["origin"]["p"] = np.array([_qrot(tqi, p - tx) for p in points]).reshape(-1, 3)
        st["ids"] = ids
        st["group"]["Qq"] = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (N, 1))
        st["group"]["Qa"] = np.ones(N)
        n = 11 + 3 * N
        S = np.eye(n) * float(self._settings.initialPointVariance)
        S[:11, :11] = st["sigma"][:11, :11]
        st["sigma"] = S
        self._fb.restore_state(st, 0)

    def processIMUData(self, imu):
        """VIOFilter.cpp:120-131"""
        return int(self._fb.process_imu([imu.stamp], imu.omega, imu.accel)[0])

    def processVisionData(self, meas):
        """VIOFilter.cpp:232-302"""
        return int(self._fb.process_vision([meas.stamp], meas.ids, meas.bearings)[0])

    def scoreVisionData(self, meas, want_lm=False):
        """NIS, log det S, log-likelihood, dof and info the frame WOULD have, at the filter's present state, without applying it; entries
        whose id the state does not hold take no part (include/eqf_vio_amd.h: eqf_score_vision).  meas.stamp is not used: bring the IMU up
        to date first.  With want_lm also nis_lm and used per entry."""
        r = self._fb.score_vision([[np.asarray(meas.ids).reshape(-1)]], [[np.asarray(meas.bearings, dtype=float).reshape(-1, 3)]], want_lm=want_lm)
        out = dict(nis=float(r.nis[0, 0]), logdet_S=float(r.logdet_S[0, 0]), loglik=float(r.loglik[0, 0]), dof=int(r.dof[0, 0]),
                   info=int(r.info[0, 0]))
        if want_lm:
            n = len(np.asarray(meas.ids).reshape(-1))
            out["nis_lm"], out["used"] = r.nis_lm[0, 0, :n], r.used[0, 0, :n]
        return out

    score = scoreVisionData

    def getTime(self):
        return float(self._fb.get_time()[0])

    def stateEstimate(self):
        s = self._fb.state_estimate(0)
        return VIOState(s["q"], s["x"], s["v"], s["p"], self._fb.ids(0))

    def stateCovariance(self):
        return self._fb.sigma(0)

    def stateCovarianceLocal(self):
        """The covariance in the coordinates of the ESTIMATE, J Sigma J^T (include/eqf_vio_amd.h: eqf_get_sigma_local); stateCovariance()
        -- like the reference's, VIOFilter.cpp:306-309 "TODO: propagate to local tangent space" -- is in the chart around the origin."""
        return self._fb.sigma_local(0)

    def innovationStats(self):
        """NIS, log det S, log-likelihood, dof and per-landmark NIS of the most recent vision update (set_option("innovation_stats", 1)
        first); include/eqf_vio_amd.h: eqf_get_innovation_stats."""
        return self._fb.innovation_stats(0)

    def setOutlierGate(self, kind, threshold):
        """Which number removeOutliers compares with its threshold: binding.GATE_CHORD (the reference's chord, the default with
        settings.outlierThreshold) or binding.GATE_MAHALANOBIS (chi-square with 2 degrees of freedom; consistency.chi2_gate_threshold);
        include/eqf_vio_amd.h: eqf_set_outlier_gate."""
        self._fb.set_outlier_gate(kind, threshold)

    def outlierGate(self):
        return self._fb.outlier_gate()

    def gateReport(self):
        """ids, statistic and removed flag of every landmark the gate of the most recent vision call examined; eqf_get_gate_report."""
        return self._fb.gate_report(0)

    def stateNEES(self, err, local=True, first=0):
        """Joint NEES err^T A^-1 err, log det A, smallest pivot, dof and the definiteness word `info` of the covariance from reference index
        `first` on, in the coordinates of the estimate (local) or of the origin; include/eqf_vio_amd.h: eqf_get_nees."""
        r = self._fb.nees([np.asarray(err, dtype=float).reshape(1, -1)], local=local, first=first)
        return dict(nees=float(r["nees"][0, 0]), logdet=float(r["logdet"][0]), min_pivot=float(r["min_pivot"][0]), dof=int(r["dof"][0]),
                    info=int(r["info"][0]))

    def sampleStateError(self, z, local=True, first=0, scale=1.0):
        """A draw from the covariance: scale * L z with L L^T the covariance from reference index `first` on, in the coordinates of the
        estimate (local; consistency.local_retract turns it into a sampled truth) or of the origin.  z: 11 + 3 N standard normal numbers, or
        a numpy.random.Generator.  Returns dict(eps (11 + 3 N,), logdet, min_pivot, dof, info); include/eqf_vio_amd.h: eqf_sample_sigma."""
        r = self._fb.sample_sigma(z if isinstance(z, np.random.Generator) else [np.asarray(z, dtype=float).reshape(1, -1)], local=local,
                                  first=first, scale=[scale])
        return dict(eps=r["eps"][0, 0], logdet=float(r["logdet"][0]), min_pivot=float(r["min_pivot"][0]), dof=int(r["dof"][0]),
                    info=int(r["info"][0]))

    def perturbState(self, z, first=0, scale=1.0):
        """Moves the filter by scale * L z (origin chart, from `first` on) on the device: bias += gamma[0:6], X <- VIOExp(liftInnovation(
        gamma[6:], xi0)) X; covariance, origin, clock and integrator stay (include/eqf_vio_amd.h: eqf_perturb_filters).  Returns dict(logdet,
        min_pivot, dof, info); the filter is not moved when info != 0."""
        r = self._fb.perturb(z if isinstance(z, np.random.Generator) else [np.asarray(z, dtype=float).reshape(1, -1)], first=first,
                             scale=[scale], stats=True)
        return dict(logdet=float(r["logdet"][0]), min_pivot=float(r["min_pivot"][0]), dof=int(r["dof"][0]), info=int(r["info"][0]))

    def process_linear_measurement(self, H, resid, R, local=True, gate=float("inf"), want_gamma=False, consider=None):
        """A measurement update with m <= 16 linear rows: resid = H eps + noise, noise ~ N(0, R), eps "truth minus estimate" in the
        coordinates of stateCovarianceLocal() (local; consistency.velocity_rows / gravity_rows / landmark_rows write the usual rows) or of
        stateCovariance().  gate: chi-square threshold on the m-dof nis (consistency.chi2_gate_threshold(p, dof=m)).  Returns dict(nis,
        logdet_S, loglik, dof, info[, gamma]); the filter is untouched when info != 0 (include/eqf_vio_amd.h: eqf_update_linear).
        consider: landmark ids (strictly ascending) that keep their estimate and covariance block (eqf_update_linear_schmidt)."""
        r = self._fb.update_linear(np.atleast_2d(np.asarray(H, dtype=float)), resid, R, local=local, gate=gate, want_gamma=want_gamma,
                                   consider=None if consider is None else [np.asarray(consider).reshape(-1)])
        out = dict(nis=float(r["nis"][0]), logdet_S=float(r["logdet_S"][0]), loglik=float(r["loglik"][0]), dof=int(r["dof"][0]),
                   info=int(r["info"][0]))
        if want_gamma:
            out["gamma"] = r["gamma"][0]
        return out

    processLinearMeasurement = process_linear_measurement

    def process_landmark_measurements(self, ids, H, resid, R, rows=None, local=True, gate=float("inf"), lm_gate=float("inf"), consider=None):
        """A measurement update from per-landmark blocks: entry k measures the landmark ids[k] (strictly ascending) alone with H (K, rows, 3),
        resid (K, rows) and its own noise covariance R (K, rows, rows) or (rows, rows) -- the second camera of a stereo rig, a range, a
        surveyed position (consistency.stereo_rows / depth_rows / position_rows).  Returns dict(nis, logdet_S, loglik, dof, info, used (K,),
        gamma); the filter is untouched when info != 0 (include/eqf_vio_amd.h: eqf_update_landmarks).
        consider: landmark ids (strictly ascending) that keep their estimate and covariance block (eqf_update_landmarks_schmidt)."""
        K = len(np.asarray(ids).reshape(-1))
        r = self._fb.update_landmarks([np.asarray(ids).reshape(-1)], [H], [resid], [R], rows=rows, local=local, gate=gate, lm_gate=lm_gate,
                                      consider=None if consider is None else [np.asarray(consider).reshape(-1)])
        return dict(nis=float(r["nis"][0]), logdet_S=float(r["logdet_S"][0]), loglik=float(r["loglik"][0]), dof=int(r["dof"][0]),
                    info=int(r["info"][0]), used=r["used"][0, :K], gamma=r["gamma"][0])

    processLandmarkMeasurements = process_landmark_measurements

    def process_landmark_observations(self, kind, ids, meas, R, cam=None, gate=float("inf"), lm_gate=float("inf"), consider=None,
                                      want_rows=False, max_lin=1, tol=0.0):
        """process_landmark_measurements with the rows formed on the device at the filter's own estimate (include/eqf_vio_amd.h:
        eqf_observe_landmarks): kind binding.OBS_BEARING / OBS_RANGE / OBS_POSITION, entry k the measurement meas[k] (a bearing, a range,
        a position in the measuring camera's frame) of the landmark ids[k] (strictly ascending) with noise covariance R (K, rows, rows),
        (rows, rows) or a scalar variance; cam: None (this camera) or (q_c, t_c), the measuring camera's pose in this camera's frame.
        Returns dict(nis, logdet_S, loglik, dof, info, used (K,): 1 applied, 0 id not in the state, 2 gated, 3 not observable; gamma) and,
        with want_rows, Ht (K, rows, 3) and resid (K, rows) as the device formed them.  max_lin > 1: the iterated update
        (eqf_observe_landmarks_iterated) with at most max_lin linearisations and the step tolerance tol; the dict then also holds n_lin,
        status and last_step."""
        K = len(np.asarray(ids).reshape(-1))
        r = self._fb.observe_landmarks(kind, [np.asarray(ids).reshape(-1)], [meas], [R], cam=cam, gate=gate, lm_gate=lm_gate,
                                       consider=None if consider is None else [np.asarray(consider).reshape(-1)], want_rows=want_rows,
                                       max_lin=max_lin, tol=tol)
        out = dict(nis=float(r["nis"][0]), logdet_S=float(r["logdet_S"][0]), loglik=float(r["loglik"][0]), dof=int(r["dof"][0]),
                   info=int(r["info"][0]), used=r["used"][0, :K], gamma=r["gamma"][0])
        if "n_lin" in r:
            out.update(n_lin=int(r["n_lin"][0]), status=int(r["status"][0]), last_step=float(r["last_step"][0]))
        if want_rows:
            out.update(Ht=r["Ht"][0, :K], resid=r["resid"][0, :K])
        return out

    processLandmarkObservations = process_landmark_observations

    def copyStateFrom(self, other):
        """This filter continues from the state of `other` (fork, or snapshot and roll back), copied on the device
        (include/eqf_vio_amd.h: eqf_copy_filters).  Settings, camera offset and capacity stay this filter's own."""
        self._fb.copy_filters(other._fb, [0], [0])

    def reset(self):
        self._fb.reset()

    def set_option(self, name, value):
        """Handle option by name (include/eqf_vio_amd.h: eqf_set_option), e.g. ``set_option("downdate_slices", 6)``: the covariance downdate
        on the integer matrix pipe (off by default)."""
        self._fb.set_option(name, value)

    @property
    def batch(self):
        return self._fb
