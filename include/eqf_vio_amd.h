/* eqf_vio_amd -- C ABI of the MI355X-native EqF propagate/update hot path.
 *
 * Drop-in boundary for pvangoor/eqf_vio's VIOFilter (eqf_vio/include/eqf_vio/VIOFilter.h:41-88).  The
 * reference has no FFI: the C++ class *is* the boundary, so every entry point below names the member
 * it replaces.  A handle owns a BATCH of `batch` independent filters (batch = 1 for the drop-in
 * case; >1 for Monte-Carlo / multi-sequence runs, BASELINE cfg 4); per-filter arguments are arrays of
 * length `batch`.  One handle = one HIP stream; calls on a handle must be serialised by the caller
 * (the reference is single-threaded too).  Calls enqueue GPU work and return; getters synchronise.
 *
 * Sigma index map (unchanged from the reference, VIOFilter.cpp:54-57,163-167,425):
 *   [0,3) gyro bias  [3,6) accel bias  [6,8) gravity dir  [8,11) velocity  [11+3i,14+3i) landmark i
 *
 * Status codes: 0 ok; >0 "silently skipped" exactly where the reference returns early;
 *               <0 error.  The library NEVER computes on the CPU: without a GPU eqf_create fails.
 */
#ifndef EQF_VIO_AMD_H
#define EQF_VIO_AMD_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EQF_OK 0
#define EQF_SKIPPED_BEFORE_FIRST_IMU 1 /* VIOFilter.cpp:147-148 (currentTime < 0)            */
#define EQF_SKIPPED_NONPOSITIVE_DT 2   /* VIOFilter.cpp:150-152, :234-236 (dt <= 0)          */
#define EQF_SKIPPED_NOT_INITIALISED 3  /* VIOFilter.cpp:235 (!initialisedFlag)               */
#define EQF_SKIPPED_NO_BEARINGS 4      /* VIOFilter.cpp:258-259                              */
#define EQF_ERR_INVALID -1
#define EQF_ERR_NO_DEVICE -2
#define EQF_ERR_HIP -3
#define EQF_ERR_CAPACITY -4      /* more landmarks than the handle was created for          */
#define EQF_ERR_UNSORTED -5      /* bearings not sorted by ascending id (VIOFilter.cpp:239)  */
#define EQF_ERR_NUMERIC -6       /* NaN / antipodal SO3FromVectors (SO3.cpp:160) on device   */
#define EQF_ERR_UNSUPPORTED -7

#define EQF_PRECISION_F64 0 /* Sigma stored and contracted in fp64 (parity grade, default)    */
#define EQF_PRECISION_F32 1 /* Sigma stored fp32, propagate + downdate in fp32 (MFMA f32)      */

/* VIOFilter::Settings, eqf_vio/include/eqf_vio/VIOFilterSettings.h:28-54 (same names, same defaults). */
typedef struct eqf_settings {
    double biasOmegaProcessVariance;
    double biasAccelProcessVariance;
    double gravityProcessVariance;
    double velocityProcessVariance;
    double pointProcessVariance;
    double velOmegaVariance;
    double velAccelVariance;
    double measurementVariance;
    double initialGravityVariance;
    double initialVelocityVariance;
    double initialPointVariance;
    double initialBiasOmegaVariance;
    double initialBiasAccelVariance;
    double initialSceneDepth;
    double outlierThreshold;
    int useInnovationLift;
    int useDiscreteInnovationLift;
    int useDiscreteVelocityLift;
    int fastRiccati;
    double initialAccelBias[3];
    double initialOmegaBias[3];
    double cameraOffset_x[3]; /* SE3 cameraOffset: translation ...                             */
    double cameraOffset_q[4]; /* ... and attitude quaternion (w, x, y, z), YAML order "xw"      */
} eqf_settings;

/* Fills the defaults of VIOFilterSettings.h:29-50. */
void eqf_settings_default(eqf_settings* s);

typedef struct eqf_filter eqf_filter; /* opaque */

/* VIOFilter(const Settings&) (VIOFilter.cpp:60-73) for `batch` filters with room for
 * `capacity_landmarks` landmarks each, on HIP device `device`, Sigma precision EQF_PRECISION_*. */
int eqf_create(const eqf_settings* settings, int capacity_landmarks, int batch, int device, int precision,
    eqf_filter** out);
void eqf_destroy(eqf_filter* f);
/* Back to the freshly constructed state (every filter of the batch): no landmarks, identity group element, Sigma and
 * bias from the settings, not initialised, time -1.  Takes the place of VIOFilter::reset() (VIOFilter.cpp:84-91), which
 * no caller in the reference uses and which is deliberately NOT reproduced literally: it also forgets xi0.cameraOffset,
 * sets Sigma to the 11x11 identity and keeps initialisedFlag / inputBias -- with a level identity pose its next Riccati
 * step throws from SO3FromVectors (SO3.cpp:160). */
int eqf_reset(eqf_filter* f);

/* VIOFilter::processIMUData (VIOFilter.cpp:120-131).  stamps[batch], omega[batch][3], accel[batch][3].
 * status (may be NULL) receives one code per filter. */
int eqf_process_imu(eqf_filter* f, const double* stamps, const double* omega, const double* accel, int* status);

/* VIOFilter::processVisionData (VIOFilter.cpp:232-302).  For filter b: nb[b] bearings with ids
 * ids[b*stride + k] (STRICTLY ascending) and unit vectors bearings[(b*stride + k)*3 + c].
 * EQF_ERR_INVALID / EQF_ERR_CAPACITY (nb[b] > capacity) / EQF_ERR_UNSORTED are returned before any effect: the
 * filters are exactly as before the call.  status[] is written whenever the call got past those checks.
 * The call enqueues and returns: the landmark bookkeeping (VIOFilter.cpp:345-443) including the outlier gate is decided and carried out
 * on the device, the update follows in the stream; the handle's id lists (eqf_num_landmarks, eqf_get_ids) are brought up to date from the
 * device's answer when the caller next touches the handle.  One consequence for status[]: a frame in which EVERY landmark of a filter is
 * thrown out as an outlier and none is new reports EQF_OK, not EQF_SKIPPED_NO_BEARINGS (the update is skipped on the device). */
int eqf_process_vision(eqf_filter* f, const double* stamps, const int* nb, const int* ids, const double* bearings,
    int stride, int* status);

/* Stream mode: the whole input stream is made resident in HBM once, then events are replayed by index
 * with no host->device traffic in the loop (how bench.py times the path).
 *   imu:      [K][batch][7]  (stamp, wx, wy, wz, ax, ay, az)      -- IMUVelocity.h:24-37
 *   vstamps:  [F][batch]; ids: [nbear] shared by all frames and filters, ascending;
 *   bearings: [F][batch][nbear][3]                                 -- VisionMeasurement.h:24-28 */
int eqf_stream_upload(eqf_filter* f, int K, const double* imu, int F, const double* vstamps, int nbear,
    const int* ids, const double* bearings);
int eqf_stream_imu(eqf_filter* f, int k);    /* == eqf_process_imu on record k    */
int eqf_stream_vision(eqf_filter* f, int fr); /* == eqf_process_vision on frame fr */

/* Getters (copy to caller memory, synchronise the handle's stream). b = filter index in the batch. */
int eqf_synchronize(eqf_filter* f);
int eqf_get_time(eqf_filter* f, double* t /* [batch] */);               /* VIOFilter::getTime          */
int eqf_num_landmarks(eqf_filter* f, int b);                             /* xi0.bodyLandmarks.size()     */
int eqf_get_ids(eqf_filter* f, int b, int* ids);
/* VIOFilter::stateEstimate (VIOFilter.cpp:304): pose q[4] (w,x,y,z), pose x[3], velocity[3],
 * landmarks p[N][3] (camera frame). */
int eqf_get_state_estimate(eqf_filter* f, int b, double* pose_q, double* pose_x, double* velocity, double* p);
/* Filter internals (what operator<<(VIOFilter) dumps, VIOFilter.cpp:311-341): origin state xi0 ...   */
int eqf_get_origin(eqf_filter* f, int b, double* pose_q, double* pose_x, double* velocity, double* p);
/* ... group element X = (A, w, Q_i = (q_i, a_i)) ...                                                   */
int eqf_get_group(eqf_filter* f, int b, double* A_q, double* A_x, double* w, double* Q_q /*[N][4]*/,
    double* Q_a /*[N]*/);
/* ... and input bias (b_omega, b_accel).                                                               */
int eqf_get_bias(eqf_filter* f, int b, double* bias6);
/* VIOFilter::stateCovariance (VIOFilter.cpp:306-309): n x n, n = 11 + 3N, row-major with leading
 * dimension ld >= n, in the reference's index map. */
int eqf_get_sigma(eqf_filter* f, int b, double* dst, int ld);
/* The same covariance in the coordinates of the ESTIMATE.  eqf_get_sigma -- like VIOFilter::stateCovariance, VIOFilter.cpp:306-309, whose
 * own comment reads "TODO: propagate to local tangent space" -- returns Sigma in the chart around the origin xi0: the covariance of
 * eps = chart_xi0(phi_{X^-1}(xi)).  The error a caller can measure against eqf_get_state_estimate is eps_loc = chart_xiHat(xi), xiHat =
 * phi_X(xi0); to first order eps_loc = J eps with a block-diagonal J (the group action with X fixed acts component by component):
 *   [0,6) bias I;  [6,8) gravity direction G = stereoSphereChartDiff(etaHat, etaHat) R_A^T stereoSphereChartInvDiff(0, eta0) (2 x 2),
 *   eta0 = R_P0^T e3, etaHat = R_A^T eta0;  [8,11) velocity R_A^T;  landmark i: a_i^-1 R(q_i)^T (the differential of Q_i^-1 p),
 * and Sigma_loc = J Sigma J^T, formed on the device in one pass over Sigma (csrc/eqf_local.hpp); Sigma itself is only read.  Layout and
 * index map of eqf_get_sigma.  The first call allocates a device buffer of Sigma's size (EQF_ERR_HIP if that fails; nothing else is
 * affected).  All three getters below flush queued IMU calls and synchronise like every getter; EQF_ERR_INVALID for bad arguments (b, a
 * NULL output, ld < n), EQF_ERR_UNSUPPORTED on an EQF_PRECISION_F32 handle, EQF_ERR_NUMERIC (not sticky) while the gravity chart of xiHat
 * or xi0 is singular (SO3.cpp:160: a level identity pose, i.e. a filter that has not been initialised).  A filter without landmarks
 * answers with the base part only. */
int eqf_get_sigma_local(eqf_filter* f, int b, double* dst, int ld);
/* The marginals a consumer normally wants, without the n^2 pass and the n^2 copy: base (11 x 11, row-major) and the N diagonal 3 x 3
 * blocks lm[N][3][3], in the origin's coordinates (local = 0: blocks of eqf_get_sigma) or the estimate's (local = 1: blocks of
 * eqf_get_sigma_local, bit for bit).  O(N) work and traffic.  lm may be NULL for a filter without landmarks. */
int eqf_get_marginals(eqf_filter* f, int b, int local, double* base, double* lm);
/* The blocks of J as the device built them: G[2][2], RAt[3][3] = R_A^T, lmJ[N][3][3] = a_i^-1 R(q_i)^T -- what a caller needs to map
 * vectors of its own between the two charts. */
int eqf_get_local_jacobian(eqf_filter* f, int b, double* G, double* RAt, double* lmJ);
/* A forecast that changes nothing (csrc/eqf_forecast.hpp): where the state and the features will be after K more IMU samples and, where t1
 * is given, the integrateUpToTime(t1) with which processVisionData begins (VIOFilter.cpp:120-131, :234) -- and how sure the filter is of
 * that.  Per filter the call computes what the filter WOULD hold: each sample has the filter's bias subtracted; each step integrates with
 * the previous sample (zero-order hold) and then replaces it; a step with dt <= 0 integrates nothing and still replaces the sample; every
 * step is the reference's step at the state after the step before, nothing is composed algebraically.  Both velocity lifts are supported.
 * O(N): with F = [[F_bb, 0], [L, D]] and D block-diagonal the base block, each landmark's 3 x 11 panel and each landmark's own diagonal
 * block evolve without the rest of Sigma, so the call reads those and writes nothing of the handle -- every getter answers with the same
 * bits afterwards (sticky error flags included), every later call gives the bits it gives on a handle that never forecast.  Two kernel
 * launches whatever K, N and the batch; results are bit for bit the same from run to run and for a filter alone or anywhere in a batch.
 * Like every getter the call first settles what the handle has deferred (queued IMU calls, the speculative gate) and synchronises.
 *   imu     [K][batch][7]: eqf_stream_upload's record (stamp, omega, accel); NULL iff K = 0
 *   t1      [batch] or NULL
 *   local   the chart of base and lm, as in eqf_get_marginals; the Jacobian is that of the FORECAST state
 *   stride  rows per filter of the per-landmark outputs (rows behind a filter's landmarks are written as zero)
 * status[b]: EQF_OK; EQF_SKIPPED_NOT_INITIALISED / EQF_SKIPPED_BEFORE_FIRST_IMU: every output of that filter is zero (a forecast does not
 * initialise a filter); EQF_SKIPPED_NONPOSITIVE_DT: samples or t1 were given and no step integrated, the outputs are the present values;
 * EQF_ERR_NUMERIC: a singular chart or a value that is not finite was met on the way -- nothing is raised in the handle, that filter's
 * outputs are NaN (steps 0).  With K = 0 and t1 NULL, or when no step integrates, pose_*, velocity, p, base and lm equal
 * eqf_get_state_estimate and eqf_get_marginals(local) bit for bit.  base and lm in the origin chart, S and ycov are exactly symmetric; base
 * and lm in the estimate chart are what eqf_get_marginals' products give.
 * Before any effect: EQF_ERR_INVALID (NULL f or out; K < 0 or K > 256; imu NULL with K > 0 or given with K = 0; local not 0 or 1; stride
 * smaller than a filter's landmark count while a per-landmark output is requested; a stamp that is not finite); EQF_ERR_UNSUPPORTED on an
 * EQF_PRECISION_F32 handle and with settings.fastRiccati = 1, whose accumulated-velocity Riccati step is a different recursion;
 * EQF_ERR_HIP if the workspace, allocated by the first call from capacity and batch, cannot be had (nothing else is affected). */
typedef struct eqf_forecast_out {   /* any pointer may be NULL: that output is not produced */
    double* time;      /* [batch]            time reached                                             */
    int*    steps;     /* [batch]            integrateUpToTime calls that integrated (dt > 0)          */
    double* pose_q;    /* [batch][4]  pose_x [batch][3]  velocity [batch][3]: eqf_get_state_estimate's */
    double* pose_x;
    double* velocity;
    double* p;         /* [batch][stride][3] landmarks of the estimate, camera frame, state order      */
    double* bearing;   /* [batch][stride][3] p / |p|                                                    */
    double* base;      /* [batch][11][11]    eqf_get_marginals' base block at the time reached          */
    double* lm;        /* [batch][stride][3][3]  ... and its diagonal blocks                            */
    double* S;         /* [batch][stride][2][2]  C_i Sigma_ii C_i^T + r I: what EQF_GATE_MAHALANOBIS and
                          nis_lm divide by, in the update's delta coordinates, from the ORIGIN-chart block
                          whatever `local` is                                                            */
    double* ycov;      /* [batch][stride][3][3]  D Sigma_loc,ii D^T, D = (I - yhat yhat^T) / |p|: covariance
                          of the predicted unit bearing (rank 2, no measurement noise), from the
                          ESTIMATE-chart block whatever `local` is                                       */
} eqf_forecast_out;
int eqf_forecast(eqf_filter* f, int K, const double* imu /* [K][batch][7]; NULL iff K = 0 */, const double* t1 /* [batch] or NULL */,
    int local, int stride, const eqf_forecast_out* out, int* status /* [batch] or NULL */);
/* Test hook: overwrite Sigma (same layout as eqf_get_sigma). */
int eqf_set_sigma(eqf_filter* f, int b, const double* src, int ld);
/* Checkpoint / resume (full precision; the reference's only dump is the lossy, write-only operator<<,
 * VIOFilter.cpp:311-341).  eqf_set_state overwrites filter b with: N landmarks with ids[N]; origin state xi0
 * (pose_q, pose_x, velocity, p0[N][3]); group element X (A_q, A_x, w, Q_q[N][4], Q_a[N]); bias6; Sigma (n x n, n =
 * 11 + 3N, leading dimension ld, reference index map); currentTime; currentVelocity6 (omega, accel) and the
 * accumulated velocity/time of the fastRiccati path; initialised flag.  Everything eqf_get_* returns can be fed back. */
int eqf_set_state(eqf_filter* f, int b, int N, const int* ids, const double* pose_q, const double* pose_x,
    const double* velocity, const double* p0, const double* A_q, const double* A_x, const double* w, const double* Q_q,
    const double* Q_a, const double* bias6, const double* sigma, int ld, double currentTime, const double* currentVelocity6,
    const double* accumulatedVelocity6, double accumulatedTime, int initialised);
/* Copy, fork and resample on the device (csrc/eqf_clone.hpp): for k in [0, n), filter dst_idx[k] of dst becomes what filter src_idx[k] of src was
 * BEFORE the call -- a gather, also with dst == src (swaps, cycles, shifts and fan-out come out right; an identity pair moves nothing).  A
 * copied filter cannot be told from its source through this header: every getter answers bit for bit the same (eqf_get_innovation_stats when
 * the option is on in both handles, otherwise valid = 0), and every later call gives the bits it gives on a handle restored through
 * eqf_set_state from the source's getters.  The STATE is copied; capacity, batch size and settings (noise variances, camera offset) stay
 * dst's.  Filters of dst that are not named are untouched, src is only read.  A fixed number of launches whatever n; Sigma moves once, at
 * the extent (12 + 3 N)^2 of each source, never over the host.  Both handles first settle what they have deferred (speculative gate, queued
 * IMU calls).  The call enqueues and returns; the two streams are ordered with EVENTS, both ways: the copy waits for what src has enqueued,
 * and src's later work waits for the copy.  Before any effect: EQF_ERR_INVALID (NULL handle or array, n < 0, an index out of range, a
 * dst_idx named twice; src_idx may repeat; n = 0 is EQF_OK), EQF_ERR_UNSUPPORTED (the handles differ in precision or device; F32 -> F32 is
 * supported), EQF_ERR_CAPACITY (a source has more landmarks than dst's capacity), EQF_ERR_HIP (the staging images of the in-place case,
 * allocated on first need, cannot be had).  The sticky error flag of either handle is neither copied nor cleared, and a copy does not
 * count as a restore towards the recovery from bit 128 (eqf_device_error). */
int eqf_copy_filters(eqf_filter* dst, eqf_filter* src, int n, const int* dst_idx, const int* src_idx);
/* Explicit landmark removal and insertion with priors (csrc/eqf_mapedit.hpp; the host's decisions: csrc/eqf_mapedit_host.hpp).  Per filter
 * the removals come first, then the insertions are appended behind what is left, in the order given; an id named in both lists is REPLACED:
 * it leaves its slot and comes back last with the new prior.  Both id lists of a filter are strictly ascending; a NULL count array means
 * "none for any filter".
 *   Removal is removeLandmarkAtIndex (VIOFilter.cpp:421-427) for every named id the state holds: its rows and columns of Sigma go, p0, Q, the
 *   per-landmark constants and the ids are compacted, the order of the rest is kept.  removed[b][k] = 1 gone, 0 the id is not in the state
 *   (no error, nothing changes on its account).
 *   Insertion is addNewLandmarks (:345-391) with the caller's values in place of the median depth and initialPointVariance: the origin
 *   landmark is p0 = p (a camera-frame position, as eqf_get_state_estimate reports it), Q the identity, every new row and column of Sigma zero
 *   except the landmark's own 3 x 3 block, which is the LOWER triangle of P, mirrored (the upper triangle is never read) and rounded to the
 *   handle's precision.  With Q = I the origin chart and the estimate's chart agree on that block: P is the covariance of the camera-frame
 *   position error (eqf_get_marginals gives it back in either chart).  inserted[b][k] = 1 done; 0 the id is already in the state after the
 *   removals (its values are not looked at); 2 values rejected: an entry of p or of P's lower triangle is not finite, p = 0, or P has a
 *   pivot <= 0 in its 3 x 3 Cholesky factorisation (judged in double precision on the caller's numbers).
 * All verdicts are decided on the host from the caller's arrays and the handle's id lists before anything is enqueued: removed / inserted
 * (either may be NULL) are complete at return, and an entry that is not applied changes no bit.  A landmark that passes the host check but
 * lies on the pole of the landmark chart raises bit 16 of eqf_device_error, like a new landmark of a vision frame.
 * Nothing of a filter but its landmarks is touched: xi0's pose and velocity, X.A, X.w, the bias, the clock, the integrator, the base block and
 * the kept blocks of Sigma, the sticky flag and the options keep every bit -- also in a filter with nothing to do, or all of whose entries
 * got verdict 0 or 2.  The records of the last update (eqf_get_last_update, eqf_get_innovation_stats, eqf_get_gate_report,
 * eqf_get_lift_report) are NOT re-ordered: they stay in the order of the landmark set they were taken on.
 * Afterwards every getter answers bit for bit like a handle restored through eqf_set_state from this handle's getters with the same edit
 * applied on the host (consistency.edit_landmarks_host), and every later call gives the bits it gives on that handle: eqf_copy_filters'
 * contract.  The result is the same from run to run and for a filter alone in a handle or anywhere in a batch (no atomics on values).
 * Settles what the handle has deferred first (queued IMU calls, speculative gate), then enqueues ONE launch and returns without waiting for
 * the device.  When some filter loses a landmark, every filter's Sigma moves once into the other buffer (the ping-pong parity is shared by
 * the batch); a call in which no filter loses anything writes only the new rows, columns and blocks in place, O(n * new).  Any capacity:
 * no list is held in LDS.  A stream uploaded by eqf_stream_upload stays valid: the next eqf_stream_vision does its bookkeeping against the
 * edited set.
 * Before any effect: EQF_ERR_INVALID (NULL handle; a negative stride; a count outside [0, stride]; a count > 0 whose id list -- or p or P --
 * is NULL), EQF_ERR_UNSORTED (an id list of a filter not strictly ascending), EQF_ERR_CAPACITY (a filter would hold more than its capacity
 * after its ACCEPTED insertions), EQF_ERR_HIP (the plan's device image, allocated by the first call that has work, cannot be had).
 * EQF_PRECISION_F32 handles are supported. */
int eqf_edit_landmarks(eqf_filter* f, const int* n_remove /* [batch] or NULL */, const int* remove_ids /* [batch][rstride] */, int rstride,
    const int* n_insert /* [batch] or NULL */, const int* insert_ids /* [batch][istride] */, int istride,
    const double* p /* [batch][istride][3] */, const double* P /* [batch][istride][3][3] */,
    unsigned char* removed /* [batch][rstride] or NULL */, unsigned char* inserted /* [batch][istride] or NULL */);
/* xi0.cameraOffset = T_IC for the whole batch (VIOFilter::setAuxiliaryData, VIOFilter.cpp:74-82, overwrites the value
 * taken from the settings at construction, :68).  q must be a unit quaternion (w,x,y,z). */
int eqf_set_camera_offset(eqf_filter* f, const double* q, const double* x);
/* The remaining scalar state needed for a lossless dump: currentVelocity6, accumulatedVelocity6, accumulatedTime,
 * initialised flag (any pointer may be NULL). */
int eqf_get_integrator(eqf_filter* f, int b, double* currentVelocity6, double* accumulatedVelocity6, double* accumulatedTime,
    int* initialised);

/* Internals of the most recent update of filter b: delta[2N], gamma[11+3N] (K*delta), Gamma[9+3N]. */
int eqf_get_last_update(eqf_filter* f, int b, double* delta, double* gamma, double* Gamma);
/* Sticky device-side error flag, 0 if none; a bit mask (any bit -> the C++ facade throws std::domain_error, like the reference's
 * SO3FromVectors, SO3.cpp:160): 1 antipodal vectors / singular gravity chart in a propagate step; 2 reserved, never raised (the residual
 * and C0i are built from per-landmark constants: a landmark on the chart pole raises 16 or 32 when it comes in); 4 a pivot of S or Sigma_e
 * not positive; 8 antipodal vectors in the innovation lift (numeric, one filter: the other filters of a batch handle keep running);
 * 16 / 32 a new / restored landmark on the chart pole (exactly ON the pole its constants are not finite and the update of the same call
 * raises 4 as well; the other filters of the handle are not touched); 64 singular gravity chart met by the builder of the dense Riccati
 * backend, which computes the chart constants itself only in a call that both initialises the pose and steps (a restored filter with a
 * valid time and initialised = 0); an ordinary level start raises 1 under either backend;
 * 128 an in-launch hand-off of k_chol_resident / k_burst_fused timed out (0.5 s: the GPU was taken away from the launch for that long) --
 * that launch did not write Sigma and the handle must be reset (eqf_reset) or restored (eqf_set_state on EVERY filter of the handle: the call
 * that restores the last one clears bit 128, and bit 4 with it -- a chain that unwinds may have judged pivots of operands it never got): until
 * then every later launch with hand-offs leaves at once.  (After a timeout inside an IMU burst the covariance the handle points at is the other ping-pong
 * buffer, i.e. NOT a valid state: restore, do not continue.)
 * About the hand-offs behind bit 128: k_chol_resident (one launch per vision update, csrc/eqf_resident.hpp) lets workgroups of ONE launch
 * wait for each other.  It is free of deadlock on any grid -- also many times larger than the chip -- under ONE assumption about the
 * hardware that HIP does not document: workgroups are started in the order of their linear index (a workgroup only ever waits for
 * lower indices, so whatever is resident contains a runnable one).  If a device or driver ever broke that order, or took the GPU away
 * for more than 0.5 s (preemption, a debugger), nothing hangs and nothing wrong is written: the first wait that times out sets bit 128 at
 * once, every other wait of the launch sees the bit within microseconds and gives up, no workgroup publishes anything after a failed
 * wait, the covariance downdate does not run (Sigma keeps its pre-update value), and the call that next touches the handle returns
 * EQF_ERR_NUMERIC.  The flag is sticky: later updates of the handle leave at once until eqf_reset.
 * EQF_CHOL_RESIDENT=0 selects one launch per 64-wide block column instead (no in-launch dependency at all).
 * (Fault injection for these hand-offs, the developer toggles, the per-kernel timers and the dense tile kernels behind the partitioned
 * filter are test / measurement hooks: include/eqf_vio_amd_debug.h -- a caller of the reference's interface needs none of them.) */
int eqf_device_error(eqf_filter* f);
/* IMU bursts.  processIMUData calls (VIOFilter.cpp:120-131) only depend on each other and on the state, so the library
 * queues them on the host and launches up to 15 of them -- plus the integrateUpToTime of the processVisionData call
 * that follows (VIOFilter.cpp:233) -- as ONE pair of kernels that reads and writes Sigma once (csrc/eqf_burst.hpp).
 * Each step is the reference's step, in order; the result does not depend on where the bursts are cut.  A queued call
 * is launched when the queue is full, when the next vision call arrives, or when any other entry point of the handle
 * is called (getters, eqf_synchronize, ...): the deferral is invisible apart from timing.  max_steps = 0 launches
 * every call at once through the single-step kernel (k_propagate); default 15 (environment: EQF_IMU_BURST). */
int eqf_set_imu_burst(eqf_filter* f, int max_steps);
/* Handle options by name.  EQF_ERR_INVALID (no effect) for a NULL handle or name, an unknown name or a value out of range.
 *   "downdate_slices" 0 (default) | 5 | 6 | 7: the covariance downdate Sigma - Y^T Y of every vision update (VIOFilter.cpp:297) on the
 *       INTEGER matrix pipe: Y's columns are scaled by powers of two and cut into that many 7-bit slices, multiplied with exact int32
 *       accumulation and recombined in fp64 (csrc/eqf_i8.hpp).  Sigma stays fp64 and exactly symmetric.  Six slices keep Sigma within
 *       1e-4 of the fp64 downdate on the bench streams; FIVE DO NOT and are there for measurement; seven come within
 *       ~1e-8.  A NaN / Inf in Y makes the rows and columns of Sigma it touches non-finite, as in fp64.  Takes effect at the next vision
 *       update, per call and in stream mode alike; 0 returns to the fp64 downdate (bit for bit the default).  The first non-zero value
 *       allocates the slices' workspace from capacity and batch (about capacity^2 * 6 * slices bytes per filter): EQF_ERR_HIP if that fails
 *       (the option stays as it was).  EQF_ERR_UNSUPPORTED on an EQF_PRECISION_F32 handle.
 *   "res_tickets" 0 (default) | 1 | 2: arrival tickets for the workgroups of the one-launch factorisation on grids larger than the chip (1:
 *       grids of at least six times the resident slots, 2: all of them) -- for a device or driver that might not start workgroups in the
 *       order of their index (see eqf_device_error); the result is bit for bit the same.
 *   "innovation_stats" 0 (default) | 1: every vision update that actually runs also leaves its innovation statistics (eqf_get_innovation_stats,
 *       below): one small launch behind the update's own (csrc/eqf_innov.hpp).  With 0 the launches and every output bit of an update are
 *       what they are without the option.  EQF_ERR_UNSUPPORTED on an EQF_PRECISION_F32 handle; EQF_ERR_HIP (option unchanged) if the
 *       records cannot be allocated.  Switching the option forgets the statistics of the last update.
 *   "innovation_lift" 0 (default) | 1: how eqf_update_linear, eqf_update_landmarks, eqf_apply_increment and eqf_perturb_filters turn their
 *       increment into a group step.  0: the plain lift VIOExp(liftInnovation(gamma_e, xi0)), whatever the handle's settings say; every
 *       output bit of those calls is what it is without the option.  1: what eqf_process_vision does with the handle's useInnovationLift /
 *       useDiscreteInnovationLift -- the reference's bundleLift (EqFMatrices.cpp:173-252), a weighted least squares over yaw and position
 *       weighted by Sigma_e^-1 that moves the POSE so that the inertial landmark positions stay as still as possible (see
 *       eqf_get_lift_report, below).  Any other value: EQF_ERR_INVALID.  EQF_ERR_UNSUPPORTED on an EQF_PRECISION_F32 handle. */
int eqf_set_option(eqf_filter* f, const char* name, int value);
/* The lift of the most recent eqf_update_linear, eqf_update_landmarks, eqf_apply_increment or eqf_perturb_filters, for filter b
 * (csrc/eqf_lift.hpp).  With the option "innovation_lift" at 1 and useInnovationLift set, a filter of at least two landmarks that takes part
 * in such a call is moved by bundleLift(gamma_e, xi0, X, Sigma_e), all in fp64, with Sigma_e = Sigma[6:, 6:] of the Sigma the call STARTED
 * from (as processVisionData passes it):
 *   gamma_e = gamma[6:], g2 = gamma_e[0:2], gamma_L = gamma_e[5:], eta0 the unit gravity direction of xi0,
 *   dUw = -eta0^x stereoSphereChartInvDiff(0, eta0) g2,   dU_f = ((I - eta0 eta0^T) dUw ; 0),
 *   Z_P ((5 + 3 N) x 6): five zero rows, then Qhat_i R_C^T [(x0 - pHat_i)^x R0 , R0] per landmark,
 *   Sigma_e = L L^T (blocked Cholesky on the matrix cores),  Zt = L^-1 Z_P,  z = L^-1 [0; gamma_L],  G6 = Zt^T Zt,  h = Zt^T z,
 *   K = [(eta0; 0) | (0; I3)]:   K^T G6 K x = K^T (-h - G6 dU_f)  (4 x 4, partial pivoting),   DeltaU = dU_f + K x,
 * then X <- Delta X with liftTotalSpaceInnovationDiscrete (useDiscreteInnovationLift = 1, EqFMatrices.cpp:254-275) or
 * VIOExp(liftTotalSpaceInnovation) (:69-96), and bias += gamma[0:6].  Sigma is not touched by the lift.  A filter with fewer than two
 * landmarks (3 N equations for 4 unknowns) takes the plain lift.  The lift's verdict comes before any effect: if Sigma_e is not positive
 * definite or any value that would be written is not finite the filter keeps every bit, Sigma included (info = 4; an update reports
 * info = 4 in its eqf_linear_report too); eqf_device_error and the sticky flag are not touched.  Bit for bit the same from run to run and
 * for a filter alone in a handle or anywhere in a batch (no atomics, one fixed summation order).  EQF_ERR_INVALID for bad arguments or
 * before the first such call.  Synchronises.  Not covered: the partitioned filter (eqf_tf_*, eqf_tiled_*). */
typedef struct eqf_lift_report {
    int kind;          /* 0 plain lift (option 0, useInnovationLift = 0, or N < 2); 1 bundleLift + continuous lift; 2 bundleLift + discrete lift */
    int info;          /* 0 applied; 3 the filter took no part (masked, gated, update's own info != 0, dof = 0); 4 lift failed: untouched */
    double DeltaU[6];  /* se(3) part of the lifted innovation (EqFMatrices.cpp:243); the plain lift's (dUw; 0) for kind 0; NaN unless info = 0 */
    double min_pivot;  /* smallest squared pivot of Sigma_e's factor (NaN for kind 0) */
    double pivot_ratio;/* min |pivot| / max |pivot| of the 4 x 4 elimination (NaN for kind 0) */
} eqf_lift_report;
int eqf_get_lift_report(eqf_filter* f, int b, eqf_lift_report* out);
/* What the update's factorisation S = C Sigma C^T + R = L L^T and z = L^-1 delta (VIOFilter.cpp:276-280 forms S.inverse() instead) say about
 * the most recent vision update of filter b -- the numbers a filter is tuned by, which need the PRE-update Sigma that no getter can reach:
 *   nis = delta^T S^-1 delta = z^T z;  logdet_S = 2 sum_k log L_kk;  dof = 2 N of that update;
 *   loglik = -(nis + logdet_S + dof log 2 pi) / 2, the measurement log-likelihood;
 *   nis_lm[i] = delta_i^T (S_ii)^-1 delta_i with the 2 x 2 diagonal block of S (2 degrees of freedom; what a chi-square gate or an outlier
 *   report needs), in the state's landmark order; nis_lm [N] may be NULL.
 * valid = 0 (and every other field 0) when that filter's last vision call was skipped (EQF_SKIPPED_*), was gated down to nothing, or
 * the option "innovation_stats" was off.  fp64 in every build, also with "downdate_slices" on, and bit for bit the same under every launch
 * shape of the factorisation and from run to run (one fixed summation order).  Flushes and synchronises like every getter. */
typedef struct eqf_innovation_stats {
    double nis;
    double logdet_S;
    double loglik;
    int dof;
    int valid;
} eqf_innovation_stats;
int eqf_get_innovation_stats(eqf_filter* f, int b, eqf_innovation_stats* out, double* nis_lm);
/* The outlier gate of a handle: which number removeOutliers (VIOFilter.cpp:429-443) compares with its threshold, for every landmark that is
 * in the state after removeOldLandmarks (the frame's new landmarks are not examined, as in the reference), before the update:
 *   EQF_GATE_CHORD        the reference's: |y_i - yHat_i|, the chord between the measured and the predicted bearing -- the same for a
 *                         landmark initialised a frame ago and a converged one;
 *   EQF_GATE_MAHALANOBIS  d2_i = delta_i^T (C_i Sigma_ii C_i^T + r I)^-1 delta_i: the residual delta_i the update will form, against the 2 x 2
 *                         diagonal block of S from the landmark's own 3 x 3 block of the CURRENT Sigma and r = measurementVariance -- what
 *                         eqf_get_innovation_stats reports as nis_lm[i], but BEFORE the outlier is absorbed.  Chi-square with 2 degrees of
 *                         freedom for a consistent filter: the quantile at probability p is -2 ln(1 - p) (5.991 / 9.210 / 13.816 at 0.95 /
 *                         0.99 / 0.999).  A quantile is a threshold for a CONVERGED filter: while Sigma is still as wide as
 *                         initialPointVariance leaves it, a gross error (0.2 rad) measures d2 of about 2.
 * A landmark goes when its number is GREATER than the threshold (a NaN stays).  Both kinds are decided and carried out on the device, in the
 * launches of the frame (csrc/eqf_churn.hpp); O(1) per landmark, no factorisation (C0 is block diagonal, EqFMatrices.cpp:319-344).
 * Until eqf_set_outlier_gate is called a handle is (EQF_GATE_CHORD, settings.outlierThreshold), and every launch and output bit are what they
 * were before this call existed.  The setter first settles what the handle has deferred (queued IMU calls; a pending gate answer is
 * resolved with the OLD kind and threshold) and takes effect at the next vision call, per call and in stream mode alike.  The chord gate is
 * disarmed from threshold 2 on, the Mahalanobis gate at +inf: no probe, no read of pinned memory.  EQF_ERR_INVALID, before any effect, for an
 * unknown kind, a NaN threshold, or kind 1 with threshold <= 0; EQF_ERR_UNSUPPORTED for kind 1 on an EQF_PRECISION_F32 handle.  The gate is a
 * setting of the handle: eqf_reset keeps it, eqf_set_state does not touch it, eqf_copy_filters does not copy it (settings stay dst's);
 * eqf_settings and settings.outlierThreshold are unchanged.
 * eqf_get_gate_report: what the gate of the most recent vision call of filter b looked at -- *n landmarks, in the state's order before the
 * removals: their ids, the chord or d2, and removed[i] = 1 for those thrown out.  ids / stat / removed hold capacity entries, any may be
 * NULL.  *n = 0 when the gate was disarmed, the call was skipped, the filter had no landmarks, after eqf_reset, and for a filter that
 * eqf_set_state or eqf_copy_filters has overwritten since.  The numbers are the ones the device left in pinned memory for the host's id
 * bookkeeping: the report costs no transfer.  Flushes and resolves like every getter.
 * Out of scope: the partitioned filter (eqf_tf_*, eqf_tiled_*) keeps its host-side chord gate -- a landmark's diagonal block lives on one
 * rank of the grid, a gate on it needs an exchange; fp32 handles (kind 1 refused). */
#define EQF_GATE_CHORD 0       /* removeOutliers as the reference has it: |y - yHat| > threshold */
#define EQF_GATE_MAHALANOBIS 1 /* delta_i^T (C_i Sigma_ii C_i^T + r I)^-1 delta_i > threshold, chi-square with 2 dof */
int eqf_set_outlier_gate(eqf_filter* f, int kind, double threshold);
int eqf_get_outlier_gate(eqf_filter* f, int* kind, double* threshold);
int eqf_get_gate_report(eqf_filter* f, int b, int* n, int* ids, double* stat, int* removed);
/* The joint NEES e^T A^-1 e, log det A and the definiteness of the covariance, for EVERY filter of the handle in one call, from a batched
 * Cholesky factorisation A = L L^T with the forward solve z = L^-1 e on the device (csrc/eqf_nees.hpp) -- the marginals of
 * eqf_get_marginals ignore every landmark-landmark and landmark-base correlation, and the host route is eqf_get_sigma_local for every filter
 * plus a factorisation of order 11 + 3 N each.
 *   local = 0: A is taken from Sigma as eqf_get_sigma returns it; local = 1: from Sigma_loc as eqf_get_sigma_local returns it.
 *   first = 0 | 6 | 11: the trailing principal submatrix from that reference index is factored -- the whole state, the state without the
 *       bias (the EqF part), the landmarks only.  These are block boundaries of J, so both charts are defined for all three.
 *   err[(b * nrhs + k) * lde + i] is entry i (reference index map) of error vector k of filter b; entries below `first` are ignored;
 *       lde >= 11 + 3 N_b for every b.  0 <= nrhs <= 16; with nrhs = 0 err and nees may be NULL and only stats is produced.
 *   nees [batch][nrhs], stats [batch].  Only the lower triangle (row >= column) of A is read.
 * Flushes queued IMU calls and synchronises like every getter; Sigma, the state and the ping-pong indices are only read (the factor
 * overwrites the scratch image of eqf_get_sigma_local).  EQF_ERR_INVALID for bad arguments, before any effect; EQF_ERR_UNSUPPORTED on an
 * EQF_PRECISION_F32 handle; EQF_ERR_HIP if the buffers, allocated by the first call, cannot be had (the handle stays as it was).  Trouble of
 * ONE filter goes into stats[b].info, the call returns EQF_OK and eqf_device_error is not touched.  A filter without landmarks answers for
 * its base part; with first = 11 its dof, nees and logdet are 0 (min_pivot: +inf).  Bit for bit the same from run to run and for a filter
 * alone in a handle or anywhere in a batch (no atomics, one fixed summation order). */
typedef struct eqf_sigma_stats {
    double logdet;     /* log det of the factored matrix = 2 sum log L_kk                          */
    double min_pivot;  /* smallest L_kk^2                                                          */
    int dof;           /* 11 + 3 N_b - first                                                       */
    int info;          /* 0 ok; 1 a pivot was not positive (logdet, min_pivot, nees are NaN);      */
                       /* -1 local = 1 and the gravity chart of this filter is singular (the same) */
} eqf_sigma_stats;
int eqf_get_nees(eqf_filter* f, int local, int first, int nrhs, const double* err, int lde, double* nees /* [batch][nrhs] */,
    eqf_sigma_stats* stats /* [batch] */);
/* Draws from the covariance, for EVERY filter of the handle in one call: eps = scale[b] L_b z with L_b L_b^T = A_b, the matrix eqf_get_nees
 * factors for the same `local` and `first` (the same launches; then one product on the matrix cores, csrc/eqf_sample.hpp).  With z ~ N(0, I)
 * eps ~ N(0, scale^2 A): the initial error of a Monte-Carlo run, or the move of a roughened resample.  The caller supplies z: there is no
 * random-number generator on the device.
 *   z[(b * nsamp + k) * ldz + i], eps[(b * nsamp + k) * lde + i]: entry i (reference index map) of sample k of filter b.  Entries of z below
 *       `first` are ignored, entries of eps below `first` are written as 0, entries from 11 + 3 N_b on are left alone.  ldz, lde >= 11 + 3 N_b
 *       for every b.  1 <= nsamp <= 64 (row tiles of 16); nsamp = 0 needs stats and answers what eqf_get_nees(nrhs = 0) answers.
 *   scale [batch] may be NULL (all 1), stats [batch] may be NULL.
 * Flushes queued IMU calls and synchronises like every getter; Sigma, the state and the ping-pong indices are only read.  EQF_ERR_INVALID for
 * bad arguments, before any effect; EQF_ERR_UNSUPPORTED on an EQF_PRECISION_F32 handle; EQF_ERR_HIP if the buffers, allocated on first need,
 * cannot be had (the handle stays as it was).  Trouble of ONE filter goes into stats[b].info (eqf_get_nees's codes): that filter's eps rows
 * are NaN, the call returns EQF_OK and eqf_device_error is not touched.  Feeding eps (scale 1) back to eqf_get_nees gives z^T z.  Bit for bit
 * the same from run to run and for a filter alone in a handle or anywhere in a batch (no atomics, one fixed summation order). */
int eqf_sample_sigma(eqf_filter* f, int local, int first, int nsamp, const double* z, int ldz, const double* scale /* [batch] or NULL */,
    double* eps, int lde, eqf_sigma_stats* stats /* [batch] or NULL */);
/* Moves filters by an increment of the origin chart, without an update around it: for every filter b with mask[b] != 0 (mask = NULL: all),
 * gamma_b = gamma[b * ldg + .] in the reference index map (the coordinates of eqf_get_sigma and of eqf_get_last_update's gamma),
 *   bias += gamma_b[0:6],   X <- VIOExp(liftInnovation(gamma_b[6:], xi0)) X
 * -- what processVisionData does with useInnovationLift = false (VIOFilter.cpp:292-296, EqFMatrices.cpp:35-67, VIOGroup.cpp:92-110,
 * :245-255) BY DEFAULT, whatever the handle's lift settings are; with the option "innovation_lift" at 1 the step follows those settings
 * (bundleLift from the present Sigma, eqf_get_lift_report; a lift that fails leaves the filter untouched).  Sigma,
 * xi0, the clock, the integrator, the ids, eqf_get_last_update, the innovation statistics and the gate report stay as they are; a masked-out
 * filter keeps every bit.  ldg >= 11 + 3 N_b for every b.  A NaN or Inf in the increment of a filter that takes part refuses the call
 * (EQF_ERR_INVALID, like every bad argument before any effect).  Settles what the handle has deferred first, enqueues one launch
 * (csrc/eqf_sample.hpp) and returns without waiting for the device.  Works in both precisions (the state is fp64 in either). */
int eqf_apply_increment(eqf_filter* f, const double* gamma, int ldg, const unsigned char* mask /* [batch] or NULL */);
/* eqf_sample_sigma(local = 0, nsamp = 1) and eqf_apply_increment in one enqueued sequence: filter b moves by scale[b] L_b z_b, which never
 * leaves the device -- bit for bit what the two calls give.  z[b * ldz + i], one vector per filter; scale [batch] may be NULL (all 1).
 * scale[b] == 0 leaves filter b untouched, every bit (roughen only the duplicates of a resample); so does a failed factorisation (info != 0)
 * and a product that is not finite.  With stats == NULL the call enqueues and returns, with stats [batch] it synchronises and reports per
 * filter as eqf_sample_sigma does.  EQF_ERR_INVALID for bad arguments (a scale that is not finite among them), before any effect;
 * EQF_ERR_UNSUPPORTED on an EQF_PRECISION_F32 handle.  The step is eqf_apply_increment's, so it follows the option "innovation_lift" too. */
int eqf_perturb_filters(eqf_filter* f, int first, const double* z, int ldz, const double* scale /* [batch] or NULL */,
    eqf_sigma_stats* stats /* [batch] or NULL */);
/* A measurement update with 1 <= m <= 16 caller-supplied LINEAR rows, for every filter of the handle in one call (csrc/eqf_linear.hpp): a
 * zero-velocity detection, a wheel or GNSS speed, a range, a surveyed landmark, an attitude reference.  The convention is the header's:
 * chart coordinates are "truth minus estimate" and the model is resid = H eps + noise, noise ~ N(0, R).
 *   H[(b * m + k) * ldh + i]: row k of filter b's measurement matrix, i in the reference index map (eqf_get_sigma's); ldh >= 11 + 3 N_b.
 *   resid[b * m + k]: measured minus predicted.  R[(b * m + k) * m + l]: the m x m noise covariance; only the lower triangle is read.
 *   local = 0: eps is the error in the ORIGIN chart -- the coordinates of eqf_get_sigma, of eqf_get_last_update's gamma and of
 *       eqf_apply_increment.  local = 1: eps is eps_loc = J eps of eqf_get_sigma_local, the error around the ESTIMATE, which is what a
 *       user can write rows for; the library forms H J on the device from eqf_get_local_jacobian's blocks.
 * Per filter that takes part, in fp64 (Ht = H or H J):
 *   B = Sigma Ht^T,  S = Ht B + R = L L^T,  Y = L^-1 B^T,  z = L^-1 resid,  gamma = Y^T z,  Sigma <- Sigma - Y^T Y (in place, bit-for-bit
 *   symmetric when Sigma was),  bias += gamma[0:6],  X <- VIOExp(liftInnovation(gamma[6:], xi0)) X  -- eqf_apply_increment's step with
 *   gamma: BY DEFAULT the plain lift, whatever the handle's lift settings are.  With the option "innovation_lift" at 1 the step follows
 *   those settings: after gamma is known and before the downdate commits, the pre-update Sigma_e is factored and bundleLift forms Delta
 *   (eqf_get_lift_report); the filter is touched only if the update's own verdict is 0 AND the lift succeeded.
 * xi0, the clock, the integrator, the ids, eqf_get_last_update, the innovation statistics, the gate report, the outlier gate and the
 * sticky flag stay as they are; eqf_device_error is never touched.  Trouble of ONE filter goes into report[b].info and that filter keeps
 * every bit, Sigma included:
 *   gate: a chi-square threshold on the m-dof nis (consistency.chi2_gate_threshold(p, dof = m)); +inf disarms it.
 *   mask [batch] or NULL (all): 0 leaves the filter alone.
 *   gamma [batch][ldg] or NULL: the increments in the reference index map, rows of untouched filters written as 0; ldg >= 11 + 3 N_b.
 * Settles what the handle has deferred first (queued IMU calls, a pending gate).  With gamma == NULL and report == NULL the call enqueues
 * and returns; otherwise it synchronises and copies out.  EQF_ERR_INVALID, before any effect: NULL f, H, resid or R; m out of range; local
 * not 0 or 1; ldh or ldg too small for some filter; an entry of H, resid or R's lower triangle of a filter that takes part that is not
 * finite; a gate that is NaN or <= 0.  EQF_ERR_UNSUPPORTED on an EQF_PRECISION_F32 handle.  EQF_ERR_HIP if the workspace, allocated by the
 * first call from capacity and batch, cannot be had (the handle stays as it was).  Bit for bit the same from run to run and for a filter
 * alone in a handle or anywhere in a batch (no atomics, one fixed summation order).
 * Not covered: the partitioned filter (eqf_tf_*, eqf_tiled_*), fp32 handles, m > 16; the innovation lift (bundleLift) by default only. */
typedef struct eqf_linear_report {
    double nis;       /* r^T S^-1 r = z^T z                                        */
    double logdet_S;  /* 2 sum log L_kk                                            */
    double loglik;    /* -(nis + logdet_S + m log 2 pi) / 2                        */
    int dof;          /* m                                                          */
    int info;         /* 0 applied; 1 S not positive definite or a non-finite value met: filter untouched (nis, logdet_S, loglik NaN);
                         2 gated (nis > gate): untouched; 3 masked out: untouched (NaN);
                         4 innovation lift failed: Sigma_e not positive definite or a non-finite value; filter untouched;
                         -1 local = 1 and this filter's gravity chart is singular: untouched (NaN) */
} eqf_linear_report;
int eqf_update_linear(eqf_filter* f, int local, int m, const double* H, int ldh, const double* resid, const double* R, double gate,
    const unsigned char* mask /* [batch] or NULL */, double* gamma /* [batch][ldg] or NULL */, int ldg,
    eqf_linear_report* report /* [batch] or NULL */);
/* A measurement update from PER-LANDMARK blocks, for every filter of the handle in one call (csrc/eqf_blocks.hpp): the bearings of the
 * second camera of a rigid stereo rig (2 rows per landmark), a depth camera's or a lidar's range on a tracked feature (1 row), surveyed
 * landmark positions (3 rows) -- a few rows each for many landmarks at once, every entry with a noise covariance of its own.  `rows` is 1,
 * 2 or 3, the same for the whole call (mixed kinds: call twice).  Filter b names nk[b] landmarks by id, 0 <= nk[b] <= stride, strictly
 * ascending as in eqf_process_vision:
 *   ids[b * stride + k]; Hb[((b * stride + k) * rows + r) * 3 + c]: the rows x 3 block H_k; resid[(b * stride + k) * rows + r];
 *   Rb[((b * stride + k) * rows + r) * rows + l]: the rows x rows noise covariance R_k, only its lower triangle is read.
 * The conventions are eqf_update_linear's: resid_k = H_k eps_i + noise, noise ~ N(0, R_k), chart coordinates "truth minus estimate", eps_i
 * the landmark's 3-block in the ORIGIN chart (local = 0: eqf_get_sigma's coordinates) or in the ESTIMATE's chart (local = 1:
 * eqf_get_sigma_local's, where the landmark block is the plain difference of camera-frame positions; the library forms H_k J_i with
 * J_i = a_i^-1 R(q_i)^T on the device).  consistency.stereo_rows / depth_rows / position_rows write the usual blocks.
 * An entry does NOT take part if its id is not in filter b's state (the vision frame's gate may have thrown it out) or if its own
 * d2_k = resid_k^T (Ht_k Sigma_ii Ht_k^T + R_k)^-1 resid_k exceeds lm_gate (taken before anything is factored; a NaN stays in, +inf
 * disarms).  It then is a decoupled block (H_k = 0, resid_k = 0, R_k = I): it changes no bit of Sigma or gamma, adds exactly 0 to nis and
 * logdet_S and is not counted in dof -- the result is bit for bit the one of the call without that entry at the same stride.
 * used[b * stride + k] reports 1 applied, 0 id not in the state (and everything of a masked filter or beyond nk[b]), 2 gated.
 * Per filter that takes part, in fp64, with Ht the block-sparse m x n matrix of the entries that take part, m = rows * (their number),
 * and Sigma read by its lower triangle:
 *   B = Sigma Ht^T,  S = Ht B + blockdiag(R_k) = L L^T,  Y = L^-1 B^T,  z = L^-1 resid,  gamma = Y^T z,  Sigma <- Sigma - Y^T Y (in place,
 *   bit-for-bit symmetric),  bias += gamma[0:6],  X <- VIOExp(liftInnovation(gamma[6:], xi0)) X  -- eqf_apply_increment's step: BY DEFAULT
 *   the plain lift; with the option "innovation_lift" at 1 the handle's lift, as in eqf_update_linear (info = 4 where it fails).
 * report[b] is eqf_update_linear's record with the same info codes and dof = m; gate is the chi-square threshold on the joint nis.  A
 * filter whose info is not 0 keeps every bit; a filter with no entry taking part reports info = 0, dof = 0, nis = logdet_S = loglik = 0
 * and is untouched.  mask, gamma, ldg as in eqf_update_linear.  xi0, the clock, the integrator, the ids, eqf_get_last_update, the
 * innovation statistics, the gate report, the outlier gate and the sticky flag stay as they are; eqf_device_error is never touched.
 * Settles what the handle has deferred first.  With used, gamma and report all NULL the call enqueues and returns; otherwise it
 * synchronises and copies out.  EQF_ERR_INVALID, before any effect: a NULL f, nk, ids, Hb, resid or Rb; rows not 1..3; local not 0 or 1;
 * stride < 1; an nk[b] outside [0, stride]; ldg too small for some filter; a gate or lm_gate that is NaN or <= 0; an entry of Hb, resid or
 * Rb's lower triangles that is not finite for k < nk[b] of a filter that is not masked out.  EQF_ERR_UNSORTED: ids of such a filter not
 * strictly ascending.  EQF_ERR_CAPACITY: nk[b] beyond the handle's capacity.  EQF_ERR_UNSUPPORTED on an EQF_PRECISION_F32 handle.
 * EQF_ERR_HIP if the workspace, allocated on first need and grown when stride or rows ask for more ((rows * stride + 3 capacity)
 * x rows * stride doubles per filter), cannot be had (the handle stays as it was).  Bit for bit the same from run to run and for a filter
 * alone in a handle or anywhere in a batch; the number of kernel launches depends on stride and rows only.
 * Not covered: the partitioned filter, fp32 handles, a second camera offset in the state; the innovation lift by default only. */
int eqf_update_landmarks(eqf_filter* f, int local, int rows, const int* nk /* [batch] */, const int* ids /* [batch][stride] */, int stride,
    const double* Hb /* [batch][stride][rows][3] */, const double* resid /* [batch][stride][rows] */,
    const double* Rb /* [batch][stride][rows][rows] */, double gate, double lm_gate, const unsigned char* mask /* [batch] or NULL */,
    unsigned char* used /* [batch][stride] or NULL */, double* gamma /* [batch][ldg] or NULL */, int ldg,
    eqf_linear_report* report /* [batch] or NULL */);
/* The Schmidt-Kalman (consider) variants of the two updates above (csrc/eqf_schmidt.hpp): filter b names a CONSIDER set of
 * n_consider[b] of its landmarks by id (consider_ids[b * cstride + k], strictly ascending; n_consider == NULL: empty sets); c are their
 * state indices.  Those landmarks keep their estimate and their own covariance block -- a surveyed or long-converged map point is not
 * dragged by one frame -- while their uncertainty and their cross-correlations still enter S and the gain of everything else.  The
 * measurement may observe them: that is the point.  With B, S, L, Y, z as above (they, nis, logdet_S, loglik, dof, used, every gate and every
 * verdict are those of the full update), the gain has its rows c set to zero and the Joseph form gives
 *   gamma_i = (Y^T z)_i off c and +0.0 on c;   Sigma_ij <- Sigma_ij - (Y^T Y)_ij unless i and j are both in c: Sigma_cc keeps every bit.
 * Every entry outside c x c, and gamma off c, has the bits of the full call with the same arguments; the returned gamma is the masked one.
 * The downdate gathers the active rows, so its cost follows (n - |c|) n, not n^2.  An id the state does not hold is ignored (a map id
 * may have left).  Before any effect, after the checks of the full call: EQF_ERR_INVALID (a negative n_consider[b] or cstride, a non-empty
 * list with consider_ids NULL), EQF_ERR_CAPACITY (n_consider[b] beyond the handle's capacity or beyond cstride), EQF_ERR_UNSORTED;
 * EQF_ERR_UNSUPPORTED on an EQF_PRECISION_F32 handle.  Everything is decided on the host from the handle's ids before anything is
 * enqueued; the call waits for the device only where the full call does.  Bit for bit the same from run to run and for a filter alone or
 * anywhere in a batch.  Not covered: consider sets on the base states, a set stored in the handle, eqf_process_vision, the partitioned
 * filter, fp32 handles. */
int eqf_update_linear_schmidt(eqf_filter* f, int local, int m, const double* H, int ldh, const double* resid, const double* R, double gate,
    const unsigned char* mask, const int* n_consider /* [batch] or NULL */, const int* consider_ids /* [batch][cstride] */, int cstride,
    double* gamma, int ldg, eqf_linear_report* report);
int eqf_update_landmarks_schmidt(eqf_filter* f, int local, int rows, const int* nk, const int* ids, int stride, const double* Hb,
    const double* resid, const double* Rb, double gate, double lm_gate, const unsigned char* mask, const int* n_consider,
    const int* consider_ids, int cstride, unsigned char* used, double* gamma, int ldg, eqf_linear_report* report);
/* eqf_update_landmarks with the rows FORMED ON THE DEVICE, at the handle's own estimate (csrc/eqf_observe.hpp): a second
 * camera's bearings, a depth sensor's ranges or surveyed positions go in as they were measured, nothing of the state is read back, and a
 * call with every output NULL enqueues and returns.  `kind` sets the rows and what meas[(b * stride + k) * 3 + ..] holds: */
#define EQF_OBS_BEARING 0  /* 2 rows; meas = y, a bearing in the measuring camera's frame, taken as given (as eqf_process_vision's) */
#define EQF_OBS_RANGE 1    /* 1 row;  meas[0] = rho, the distance from that camera's centre */
#define EQF_OBS_POSITION 2 /* 3 rows; meas = m, a position in that camera's frame */
/* cam = (q_c: w, x, y, z; t_c): the pose of the measuring camera in the primary camera's frame, the frame the landmarks live in; q_c is
 * normalised by the library.  NULL: the identity (a bearing is then the primary camera's own); cam_per_filter = 0: one offset [7] for the
 * call; cam_per_filter = 1: one per filter [batch][7], a bank of extrinsic hypotheses.  Per entry whose id the state holds, with i its
 * landmark, J_i = a_i^-1 R(q_i)^T (eqf_get_local_jacobian's block), p_hat = J_i p0_i and R_c = R(q_c):
 *   p_c = R_c^T (p_hat - t_c),  d = |p_c|,  y_hat = p_c / d
 *   BEARING   H = stereoSphereChartDiff(y_hat, y_hat) (I - y_hat y_hat^T) R_c^T / d     resid = stereoSphereChart(y, pole y_hat)
 *   RANGE     H = y_hat^T R_c^T                                                         resid = rho - d
 *   POSITION  H = R_c^T                                                                 resid = m - p_c
 *   Ht = H J_i, the rows in eqf_get_sigma's coordinates
 * -- consistency.stereo_rows / depth_rows / position_rows at the device's estimate (consistency.observe_rows_host is the numpy
 * statement).  From there on the call IS eqf_update_landmarks(local = 0) with (Ht, resid, Rb) at the same stride and rows, bit for bit
 * and launch for launch (one rows kernel in the other's place): each entry's d2 and lm_gate, S, the factorisation, gamma, gate, mask, the
 * report and its info codes, the option "innovation_lift", the in-place downdate and the group step; a non-NULL n_consider makes it
 * eqf_update_landmarks_schmidt.  The gravity chart plays no part: info -1 never occurs.
 * used has one more value, 3 NOT OBSERVABLE: d is zero or not finite, or, for a bearing, the chart is singular (y_hat at the chart's own
 * pole e3, where the chart functions raise their flag, or y at the antipode of y_hat, where the chart's value is not finite).  Such an
 * entry is a decoupled block that is never formed, like an absent or a gated one: the result is bit for bit the call's without it.
 * Ht_out [batch][stride][rows][3] / resid_out [batch][stride][rows] return what the device formed -- every entry's Jacobian and
 * innovation, for a tracker or a log; zeros for an entry that is absent or not observable, of a masked filter or beyond nk[b].
 * With used, Ht_out, resid_out, gamma and report all NULL the call enqueues and returns; otherwise it synchronises and copies out.  The
 * errors are eqf_update_landmarks's (and eqf_update_landmarks_schmidt's), before any effect; in addition EQF_ERR_INVALID for an unknown
 * kind, a cam_per_filter that is not 0 or 1, a zero quaternion, or a value of cam or meas that is not finite where it is read (k < nk[b]
 * of a filter that is not masked out; meas[1], meas[2] of a range are not read; the single offset of a call is always read).
 * EQF_ERR_UNSUPPORTED on an EQF_PRECISION_F32 handle.
 * Not covered: the partitioned filter; a camera offset carried in the state; a dry run that only predicts the rows. */
int eqf_observe_landmarks(eqf_filter* f, int kind, const double* cam /* NULL | [7] | [batch][7] */, int cam_per_filter,
    const int* nk /* [batch] */, const int* ids /* [batch][stride] */, int stride, const double* meas /* [batch][stride][3] */,
    const double* Rb /* [batch][stride][rows][rows], lower triangles */, double gate, double lm_gate,
    const unsigned char* mask /* [batch] or NULL */, const int* n_consider /* [batch] or NULL */,
    const int* consider_ids /* [batch][cstride] */, int cstride, unsigned char* used /* [batch][stride] or NULL */,
    double* Ht_out /* [batch][stride][rows][3] or NULL */, double* resid_out /* [batch][stride][rows] or NULL */,
    double* gamma /* [batch][ldg] or NULL */, int ldg, eqf_linear_report* report /* [batch] or NULL */);
/* eqf_observe_landmarks ITERATED: the rows are re-formed at the estimate the update would give until the increment settles -- the
 * iterated Kalman update, Gauss-Newton on the MAP cost -- and only the last linearisation is applied (csrc/eqf_iterate.hpp; DESIGN
 * 4.5q).  For a measurement whose one linearisation at the prior is poor: a second camera's bearing or a range on a landmark that entered
 * at the median depth, a surveyed position after drift.  Every argument of eqf_observe_landmarks has its meaning, its checks and its
 * errors here; max_lin (1 .. EQF_ITER_MAX_LIN) is the largest number of linearisations and tol (absolute, in chart units, >= 0 and
 * finite; 0: never stop early) the step below which a filter stops; EQF_ERR_INVALID otherwise.  Everything is fp64, per filter, and
 * neither Sigma nor the state is written before the commit:
 *   0  Linearisation 0 is eqf_observe_landmarks's, at the handle's estimate.  Each entry's verdict `used` is decided here and FROZEN:
 *      later linearisations re-form the entries with verdict 1 only, and no entry is gated again, then or at the commit.
 *   k  With M the landmark 3-blocks of the frozen-in entries: S_k = Ht_k Sigma_MM Ht_k^T + blockdiag(R_e), w = S_k^-1 r~_k,
 *      g_{k+1} = Sigma_MM Ht_k^T w -- gamma = Sigma Ht^T S^-1 r~ on those rows; +0.0 on an entry whose landmark is considered.
 *      last_step = max over entries and components |g_{k+1} - g_k|.  last_step <= tol (tol > 0): converged, the rows of linearisation k
 *      are committed.  Otherwise Q_trial = Delta_i(g_{k+1,e}, p0_i) Q_i from the handle's UNCHANGED Q_i (eqf_apply_increment's plain
 *      step on that landmark), the rows Ht_{k+1}, resid_{k+1} there, and r~_{k+1} = resid_{k+1} + Ht_{k+1} g_{k+1,e} (per row: the
 *      residual, then one fused multiply-add per component of g in order).  Chart coordinates are truth minus estimate, so moving the
 *      estimate by g leaves eps_0 = eps_k + g: r~ is the residual of the rows on the PRIOR's error, to the order to which the filter
 *      itself treats Sigma as unchanged by a group step.  Intermediate points use the plain step whatever "innovation_lift" says.
 *   K  The commit IS eqf_update_landmarks(local = 0) on the prior state with the committed rows (Ht_K, r~_K, Rb) and the frozen verdicts,
 *      bit for bit and launch for launch from k_blk_gain on: gate, mask, "innovation_lift", the consider lists, gamma and report are
 *      that call's, and a filter whose info is not 0 keeps every bit.  Ht_out / resid_out return the committed rows (resid_out is r~_K).
 * iter_report[b] = {n_lin, status, last_step}: the linearisations taken, the last step seen (NaN with status 3), and status
 *   0 converged; 1 ran out of linearisations (always so with max_lin = 1); 2 STALLED: an entry was not observable at a trial point (d
 *   zero or not finite, a singular chart) -- the rows of the previous linearisation are committed; 3 an intermediate solve failed (S_k
 *   not positive definite or a value not finite) -- the rows of linearisation k are committed and the commit's own info says what the
 *   full factorisation makes of them; 4 masked out (n_lin = 0).
 * g_trace [max_lin][batch][stride][3]: the increment on each entry's landmark block at which linearisation k was TAKEN; plane 0 is all
 * zeros, and so are the planes of a filter behind its last linearisation (a trial point that stalled was not taken).
 * All max_lin linearisations are enqueued without waiting; a per-filter flag on the device turns every later launch into a no-op for a
 * filter that has stopped, so a filter's result has the same bits alone in a handle or anywhere in a batch, whatever its neighbours do.
 * No atomics, every sum in one fixed order.  max_lin = 1 is eqf_observe_landmarks bit for bit and launch for launch; otherwise the call
 * adds (max_lin - 1) (3 + the factorisation's 3 nb - 1) + 1 launches, nb = ceil(rows stride / 64) (iterate::extraLaunches).  With used,
 * Ht_out, resid_out, gamma, report, g_trace and iter_report all NULL the call enqueues and returns.
 * Workspace, per filter and beyond eqf_observe_landmarks's: (mp + 2 + 3 stride) mp + 6 stride + 5121 doubles, mp = rows stride rounded
 * up to 64, a second rows array, and max_lin stride 3 doubles of trace.
 * Not covered: the partitioned filter, fp32 handles (EQF_ERR_UNSUPPORTED), eqf_update_linear and eqf_process_vision, re-gating between
 * linearisations, a line search, linearisation points taken with the innovation lift. */
#define EQF_ITER_MAX_LIN 16
typedef struct {
    int n_lin;
    int status;
    double last_step;
} eqf_iter_report;
int eqf_observe_landmarks_iterated(eqf_filter* f, int kind, const double* cam /* NULL | [7] | [batch][7] */, int cam_per_filter,
    const int* nk /* [batch] */, const int* ids /* [batch][stride] */, int stride, const double* meas /* [batch][stride][3] */,
    const double* Rb /* [batch][stride][rows][rows], lower triangles */, double gate, double lm_gate,
    const unsigned char* mask /* [batch] or NULL */, const int* n_consider /* [batch] or NULL */,
    const int* consider_ids /* [batch][cstride] */, int cstride, int max_lin, double tol, unsigned char* used /* [batch][stride] or NULL */,
    double* Ht_out /* [batch][stride][rows][3] or NULL */, double* resid_out /* [batch][stride][rows] or NULL */,
    double* gamma /* [batch][ldg] or NULL */, int ldg, eqf_linear_report* report /* [batch] or NULL */,
    double* g_trace /* [max_lin][batch][stride][3] or NULL */, eqf_iter_report* iter_report /* [batch] or NULL */);

/* Moment matching over the filters of ONE handle, on the device (csrc/eqf_mixture.hpp): a weighted batch -- a Monte-Carlo study, a particle
 * set, a bank of hypotheses -- turned back into one mean and one covariance that includes the spread between its members, and several
 * filters replaced by one that matches their first two moments.  Everything is fp64 and in the reference index map of eqf_get_sigma.
 *   idx[0..n): the members (need not be distinct: a repeated index is two members); w[k] >= 0 their weights, normalised on the host in
 *   double (s the serial sum in the order of idx, w~_k = w_k / s); ref, one of idx: the reference member.  Every member must have the
 *   reference's landmark ids in the reference's order.
 * Moments are taken in the chart chi_c of a centre state c -- the chart of eqf_get_sigma_local (consistency.local_error): differences for
 * bias, body velocity and body-frame landmarks, stereoSphereChart(eta, pole = eta_c) for the gravity direction eta = R^T e3.  Per member b
 * with estimate xHat_b (eqf_get_state_estimate, eqf_get_bias):
 *   e_b = chi_c(xHat_b);  J'_b = J_b of eqf_get_local_jacobian with its gravity block G_b replaced by T_b G_b, T_b =
 *   stereoSphereChartDiff(eta_b, pole eta_c) stereoSphereChartInvDiff(0, pole eta_b), the differential at 0 of chi_c o chi_xHat_b^-1 (its
 *   other blocks are the identity); T_b = I by definition where c is member b's own estimate.
 *   eBar = sum_k w~_k e_k;   P = sum_k w~_k [ J'_k Sigma_k J'_k^T + (e_k - m)(e_k - m)^T ],  m = eBar (centred = 1) or 0 (centred = 0).
 * eqf_get_mixture_moments: eBar -> mean (or NULL) and P (leading dimension ld >= 11 + 3 N) about c = xHat_ref.  Flushes queued IMU calls and
 * synchronises like every getter; only reads the handle (it overwrites the scratch image of eqf_get_sigma_local, as eqf_get_nees does).
 * eqf_merge_filters: eBar about xHat_ref; xBar = consistency.local_retract(xHat_ref, eBar) with bias_ref + eBar[0:6] -- the attitude turned by
 * the shortest rotation that takes eta_ref to the merged direction, yaw the reference's, the pose position sum_k w~_k x_k (not part of the
 * chart: it has no covariance); P about c = xBar with centred = 0, the mean-square error about the new estimate.  Filter dst then is what
 * eqf_copy_filters(ref -> dst) would leave, except: origin = xBar, X = identity (A = (1, 0), w = 0, Q_i = (1, 1)), the merged bias,
 * Sigma = P (with X = identity J is the identity: Sigma is Sigma_loc), pose and per-landmark constants recomputed.  dst may be a member,
 * ref included: every member is read as it was before the call.  Settles what the handle has deferred, enqueues a fixed number of launches
 * whatever n is and, with report == NULL, returns without waiting -- unless dst's host bookkeeping (ids, clock, flags, gate report) differs
 * from what the merge leaves, where the verdict is waited for so that it changes only if the device wrote.
 * P is bit-for-bit symmetric (the lower triangle is computed, the upper is its mirror), the same from run to run and for members alone in
 * a handle or anywhere in a batch (no atomics, one fixed order: idx's); with n = 1 its lower triangle is eqf_get_sigma_local's, bit for
 * bit, and a member of weight 0 changes no bit.
 * report->info != 0: mean and P are NaN, a merge writes nothing (dst keeps every bit), the call returns EQF_OK; eqf_device_error is never
 * touched.  Before any effect: EQF_ERR_INVALID for NULL arguments; n < 1; an index, ref or dst out of range; ref not among idx; ld < 11 +
 * 3 N; a weight that is negative or not finite, or a weight sum that is not positive; centred not 0 or 1; members whose landmark count or
 * ids differ from the reference's; for the merge, members whose eqf_get_time differs from the reference's or that are not initialised.
 * EQF_ERR_UNSUPPORTED on an EQF_PRECISION_F32 handle.  EQF_ERR_HIP if the workspace, allocated on first need from capacity and batch,
 * cannot be had (the handle stays as it was).
 * Not covered: the partitioned filter (eqf_tf_*, eqf_tiled_*), fp32 handles, members in different handles, the C++ facade VIOFilter.h
 * (one filter per handle). */
typedef struct eqf_mixture_report {
    double n_eff;          /* 1 / sum w~^2                                             */
    double spread_trace;   /* trace of the spread term sum_k w~_k (e_k - m)(e_k - m)^T */
    double total_trace;    /* trace of P                                               */
    int n;
    int info;              /* 0 ok; 1 a non-finite value met; -1 a gravity chart needed is singular */
} eqf_mixture_report;
int eqf_get_mixture_moments(eqf_filter* f, int n, const int* idx, const double* w, int ref, int centred,
    double* mean /* [11 + 3 N] or NULL */, double* P, int ld, eqf_mixture_report* report /* or NULL */);
int eqf_merge_filters(eqf_filter* f, int n, const int* idx, const double* w, int ref, int dst, eqf_mixture_report* report /* or NULL */);

/* The deterministic split: filters become mixture components placed along one functional, on the device (csrc/eqf_split.hpp; the host's
 * decisions: csrc/eqf_split_host.hpp).  Everything is fp64 in the origin chart and the reference index map -- the coordinates of
 * eqf_get_sigma and eqf_apply_increment.  Per source filter s (order 11 + 3 N_s, covariance Sigma) with its row a + s * lda:
 *   Ht = a (local = 0) or a J_s (local = 1: the row is written against eqf_get_sigma_local's error around the estimate; a J is formed on
 *   the device by the code that forms H J for eqf_update_linear(local = 1));  B = Sigma Ht^T,  S = Ht B (the variance of the functional),
 *   u = B / sqrt(S), so that u u^T <= Sigma and Ht u = sqrt(S).
 * Child k is the record (dst_idx[k], src_idx[k], shift[k], shrink[k]).  Afterwards filter dst is what eqf_copy_filters(src -> dst) would
 * leave, except that Sigma_dst = Sigma_src - shrink u u^T (product u_i u_j first, then one fused multiply-add: bit-for-bit symmetric when
 * Sigma_src was) and that the state is moved by gamma = shift u with eqf_apply_increment's step, bias += gamma[0:6],
 * X <- VIOExp(liftInnovation(gamma[6:], xi0)) X -- ALWAYS the plain lift, whatever the option "innovation_lift" says: the moment identity
 * below holds in this chart for the plain step only.  The functional moves by shift sqrt(S) and keeps the variance (1 - shrink) S;
 * shrink = 1 leaves Sigma singular along u.  With weights w~_k of the caller's (the handle holds none, as for eqf_merge_filters),
 * sum w~_k = 1, sum w~_k shift_k = 0 and sum w~_k (shift_k^2 - shrink_k) = 0, the children of a source satisfy
 * sum_k w~_k (Sigma_k + gamma_k gamma_k^T) = Sigma exactly (consistency.split_components gives such triples).
 * Gather semantics, eqf_copy_filters': every source is read as it was before the call; src_idx may repeat (fan-out), dst_idx may not;
 * dst == src is the child that stays in the parent's slot, written in place.  A filter named as a dst may be a source only of ITSELF --
 * one that a child of another source overwrites may be nobody's source: no swaps, no permutations through other sources (EQF_ERR_INVALID) --,
 * so that one pass reads a tile of a source once and writes all its children without staging.  Rows of a that
 * belong to no child's source are never read.  Filters that are not named keep every bit.
 * The verdict is per SOURCE and decided on the device: info 0 done; 1 S is not positive or a value is not finite; -1 local = 1 and the
 * source's gravity chart is singular.  A source with info != 0 writes none of its children -- every such dst keeps every bit, the one in
 * place included --, their gamma rows are 0 and their S is NaN; the call returns EQF_OK and eqf_device_error is never touched.
 * Exactness: a child with shrink == 0 has the source's Sigma bit for bit (signs of zeros included), a child with shift == 0 the source's
 * state bit for bit, with both it is eqf_copy_filters' result; a child with shift != 0 has the state eqf_apply_increment (option
 * "innovation_lift" off) leaves on a fork when given the returned gamma row.  gamma (or NULL): row k, leading dimension ldg, is child k's
 * increment; report (or NULL): entry k is child k's source's verdict.
 * Settles what the handle has deferred, then enqueues a fixed number of launches whatever n and the fan-out are; with gamma == NULL and
 * report == NULL it returns without waiting -- unless a dst's host bookkeeping (ids, clock, flags, gate report) differs from what the copy
 * leaves, where the verdicts are waited for so that it changes only if the device wrote (eqf_merge_filters' rule).  Bit for bit the same
 * from run to run and for a filter alone in a handle or anywhere in a batch (no atomics, one fixed summation order).
 * n = 0 does nothing at all (nothing is settled either).  Before any effect other than settling what was deferred (the checks that need
 * the landmark counts come behind it, as in the sibling calls): EQF_ERR_INVALID for a NULL f, or with n > 0 a NULL a, index array, shift or shrink; n < 0 (n = 0 is EQF_OK); local not
 * 0 or 1; an index out of range; a dst named twice; a dst with another source that is itself some child's source; lda -- or ldg with gamma given -- smaller than
 * 11 + 3 N of a named source; a shift that is not finite; a shrink that is not finite or outside [0, 1]; an entry of the read part of a
 * named source's row that is not finite.  EQF_ERR_UNSUPPORTED on an EQF_PRECISION_F32 handle.  EQF_ERR_HIP if the workspace, allocated on
 * first need from capacity and batch, cannot be had (the handle stays as it was).
 * Not covered: the partitioned filter (eqf_tf_*, eqf_tiled_*), fp32 handles, sources and destinations in different handles, the C++ facade
 * VIOFilter.h (one filter per handle). */
typedef struct eqf_split_report {
    double S;   /* variance of the functional in the source; NaN when info != 0 */
    int info;   /* 0 done; 1 S not positive or a value not finite; -1 local = 1 and the gravity chart singular */
} eqf_split_report;
int eqf_split_filters(eqf_filter* f, int local, const double* a /* [batch][lda] */, int lda, int n, const int* dst_idx, const int* src_idx,
    const double* shift /* [n] */, const double* shrink /* [n] */, double* gamma /* [n][ldg] or NULL */, int ldg,
    eqf_split_report* report /* [n] or NULL */);

/* WHICH members to merge: the pairwise merge costs of the members of a mixture, on the device (csrc/eqf_mergecost.hpp).  Members, weights,
 * ref, the normalisation of w and the checks on ids are eqf_get_mixture_moments'; first is eqf_get_nees's (0 | 6 | 11: the trailing
 * principal submatrix from that reference index).  Everything is taken in the ONE chart chi_c, c = xHat_ref: e_b and J'_b as above,
 * Sigma'_b = J'_b Sigma_b J'_b^T (the lower triangle of Sigma is read).  A cost is invariant under a common LINEAR change of chart --
 * log-determinants shift by the same constant, the quadratic form does not move -- and to first order the transition between two members'
 * charts is linear: that is why one centre serves all pairs.
 * For the pair of POSITIONS (i, j) in idx, ordered by the library so that i < j, alpha = w~_j / (w~_i + w~_j) (1/2 if both weights are 0):
 *   SigmaBar_ij = Sigma'_i + alpha (Sigma'_j - Sigma'_i)  entry by entry,   d = e_j - e_i,   SigmaBar_ij = L L^T (blocked fp64 Cholesky on
 *   the matrix cores, d carried as a right-hand side),   logdet_pair = 2 sum log L_kk,   maha = |L^-1 d|^2;
 * per member ld_b from the same route applied to Sigma'_b.
 *   EQF_COST_RUNNALLS        cost = 1/2 [ w~_i (ld_ij - ld_i) + w~_j (ld_ij - ld_j) + (w~_i + w~_j) log1p(alpha (1 - alpha) maha) ]
 *                            (Runnalls' bound on the Kullback-Leibler discrimination; log det(SigmaBar + alpha (1 - alpha) d d^T) through
 *                            the determinant lemma: no second factorisation)
 *   EQF_COST_BHATTACHARYYA   weights ignored, alpha = 1/2:  cost = 1/8 maha + 1/4 [ (ld_ij - ld_i) + (ld_ij - ld_j) ]
 * pairs: npairs pairs of positions, or NULL: the first npairs (at most n (n - 1) / 2) of all i < j in lexicographic order.  out [npairs];
 * member [n] (by position) or NULL.  npairs = 0 with member given is allowed.
 *   Read-only: settles what the handle has deferred and synchronises like every getter; every getter answers with the same bits afterwards
 *   and every later call gives the bits it gives on a handle that never asked (the scratch image of eqf_get_sigma_local is overwritten, as
 *   eqf_get_nees does).
 *   Reproducible: no atomics, one fixed summation order; bit for bit the same from run to run.
 *   Independent of context: the record of a pair does not depend on which other pairs are in the call, on their order, on the chunking, on
 *   whether it was named (i, j) or (j, i), or on which slots of which handle hold the members.
 *   Identical members cost exactly 0: a pair whose two members are the same filter, or bit-identical copies made by eqf_copy_filters, has
 *   cost == 0.0, maha == 0.0 and logdet_pair == member[i].logdet exactly -- members and pairs go through the same kernels.  (A copy OF ref
 *   is not identical to ref in this sense where its T_b, computed, is not the identity that ref has by definition.)
 *   member[k].logdet, min_pivot, dof and info of the member that IS ref equal bit for bit what eqf_get_nees(local = 1, first, nrhs = 0)
 *   reports for that filter.
 *   Trouble of ONE pair goes into its info (fields NaN): the call returns EQF_OK and eqf_device_error is never touched.
 * Before any effect: EQF_ERR_INVALID for everything eqf_get_mixture_moments refuses, a kind or first out of range, npairs < 0 (or beyond all
 * pairs with pairs == NULL), a pair position out of range, out == NULL with npairs > 0.  EQF_ERR_UNSUPPORTED on an EQF_PRECISION_F32 handle.
 * EQF_ERR_HIP if the workspace cannot be had (the handle stays as it was): one image per item of a chunk -- by default as many as the
 * handle has filters, one more scratch image set; eqf_set_option(f, "merge_cost_chunk", c), 1 <= c <= 4096 (0: the default), overrides it.
 * Members are factored first, then the pairs, never in one chunk together; the number of launches depends only on the number of distinct
 * members, n, npairs, N, first and the chunk.
 * Not covered: the partitioned filter, members in different handles, the C++ facade. */
#define EQF_COST_RUNNALLS 0
#define EQF_COST_BHATTACHARYYA 1
typedef struct eqf_pair_cost {
    double cost;         /* see above                                                        */
    double logdet_pair;  /* log det SigmaBar_ij                                              */
    double maha;         /* d^T SigmaBar_ij^-1 d,  d = e_j - e_i                              */
    int info;            /* 0 ok; 1 a pivot not positive or a non-finite value (NaN fields);  */
                         /* -1 a gravity chart needed by either member is singular (NaN)      */
    int pad_;
} eqf_pair_cost;
int eqf_get_merge_costs(eqf_filter* f, int n, const int* idx, const double* w, int ref, int kind, int first, int npairs,
    const int* pairs /* [npairs][2] POSITIONS in idx, or NULL: all i < j in lexicographic order */, eqf_pair_cost* out /* [npairs] */,
    eqf_sigma_stats* member /* [n] or NULL */);

/* HOW LIKELY a vision frame is under a filter BEFORE the filter absorbs it: ncand candidate frames per filter scored on the device without
 * applying any of them (csrc/eqf_score.hpp) -- alternative data associations of one frame (the joint-compatibility test), an ambiguous
 * re-detection, a look-ahead likelihood to weight particles with before resampling.
 *   Candidate c of filter b names nb[b * ncand + c] bearings, ids[(b * ncand + c) * stride + k] strictly ascending and
 *   bearings[((b * ncand + c) * stride + k) * 3 ..], k < nb[b * ncand + c], as in eqf_process_vision.
 *   An entry takes part if and only if its id is a landmark of filter b's state.  The other entries carry no information about the state
 *   (a new landmark would only be appended): used = 0, and they add exactly nothing.  Landmarks of the state that the candidate does not
 *   name are simply not part of the measurement: nothing is removed -- the intended difference from processVisionData, whose bookkeeping
 *   throws out every landmark a frame does not name.
 *   With M the matching landmarks IN THE STATE'S OWN ORDER, delta_i the residual the update would form, C_i the 2 x 3 output block of
 *   landmark i and r = measurementVariance:
 *     S = C_M Sigma_MM C_M^T + r I  (order 2 |M|),   S = L L^T (blocked fp64 Cholesky on the matrix cores),   z = L^-1 delta_M,
 *     nis = z^T z,   logdet_S = 2 sum log L_kk,   dof = 2 |M|,   loglik = -(nis + logdet_S + dof log 2 pi) / 2.
 *   nis_lm[(b * ncand + c) * stride + k] of a matching entry is delta_i^T (C_i Sigma_ii C_i^T + r I)^-1 delta_i, the number
 *   EQF_GATE_MAHALANOBIS and eqf_get_innovation_stats report, at the caller's entry position k; 0 elsewhere.  used likewise, 1 | 0.
 *   The score is taken at the handle's PRESENT state and Sigma.  The integrateUpToTime(stamp) with which processVisionData begins is not
 *   part of it: the caller brings the IMU up to date first (eqf_process_imu).  What is left out is Q dt of less than one IMU period.
 *   A candidate without a matching entry -- nb = 0, no id of the state, a filter that is not initialised or has no landmarks -- reports
 *   info = 0, dof = 0, nis = logdet_S = loglik = 0.  A filter with mask[b] == 0 reports info = 3 and NaN; its ids and bearings are not looked at.
 *   Trouble of ONE candidate goes into its info (fields NaN): the call returns EQF_OK and eqf_device_error is never touched.
 *   Read-only, like eqf_forecast: settles what the handle has deferred (queued IMU calls, a pending gate) and synchronises like every
 *   getter; writes a workspace of its own -- not the scratch image of eqf_get_sigma_local / eqf_get_nees either --; every getter answers
 *   with the same bits afterwards, sticky flags included, and every later call gives the bits it gives on a handle that never scored.
 *   Reproducible and independent of context: no atomics, one fixed summation order; a candidate's record and its nis_lm do not depend on
 *   which other candidates or filters are in the call, on their order, on the chunking, or on stride.
 * Before any effect: EQF_ERR_INVALID for a NULL f, nb, ids, bearings or out; ncand < 1; stride < 1; an nb outside [0, stride]; a bearing
 * component that is not finite for an entry below nb of a filter that is not masked out.  EQF_ERR_UNSORTED: ids of such a filter not strictly
 * ascending.  EQF_ERR_CAPACITY: an nb beyond the handle's capacity.  EQF_ERR_UNSUPPORTED on an EQF_PRECISION_F32 handle.  EQF_ERR_HIP if the
 * workspace, allocated on first need and grown when needed, cannot be had (the handle stays as it was): one image per item of a chunk, a
 * square of the padded order 2 capacity each -- by default as many images as the handle has filters; eqf_set_option(f, "score_chunk", c),
 * 1 <= c <= 4096 (0: the default), overrides it.  The number of launches depends only on ncand, the batch, the largest order and the chunk.
 * Not covered: the partitioned filter (eqf_tf_*, eqf_tiled_*), fp32 handles, propagation to the stamp. */
typedef struct eqf_frame_score {
    double nis;       /* delta^T S^-1 delta = z^T z                                   */
    double logdet_S;  /* 2 sum log L_kk                                                */
    double loglik;    /* -(nis + logdet_S + dof log 2 pi) / 2                          */
    int dof;          /* 2 x (entries that matched a landmark of the state)            */
    int info;         /* 0 scored; 1 a pivot of S not positive or a non-finite value   */
                      /* (nis, logdet_S, loglik NaN); 3 masked out (NaN)               */
} eqf_frame_score;
int eqf_score_vision(eqf_filter* f, int ncand, const int* nb /* [batch][ncand] */,
    const int* ids /* [batch][ncand][stride] */, const double* bearings /* [batch][ncand][stride][3] */, int stride,
    const unsigned char* mask /* [batch] or NULL */, eqf_frame_score* out /* [batch][ncand] */,
    double* nis_lm /* [batch][ncand][stride] or NULL */, unsigned char* used /* [batch][ncand][stride] or NULL */);

/* Propagate backend: 0 = block-structured HBM-bound kernel (default, product path),
 * 1 = dense F Sigma F^T on MFMA (what the reference executes; BASELINE cfg 3 cross-check). */
int eqf_set_dense_propagate(eqf_filter* f, int on);

/* ================================================================================================================================
 * BASELINE configs[4]: ONE filter with N = 4000 landmarks whose Sigma (1.15 GB) is 2-D block-partitioned over the GPUs of a node.
 * One process per GPU; process (pr, pc) of a Pr x Pc grid owns the landmark blocks I = pr, pr + Pr, ... as rows and J = pc, pc + Pc,
 * ... as columns of ONE dense local matrix Sll (3 nlr x 3 nlc doubles, row-major, CALLER-OWNED device memory, e.g. a torch tensor, so
 * that torch.distributed can move pieces of it).  The O(N) filter state and the 11-row base panel Sigma[0:11, :] are REPLICATED: every
 * rank advances its own identical copy inside its eqf_tiled handle, with the same device functions as the single-GPU path.  The
 * exchange schedule (which block row is factored where, the RCCL broadcasts of the solved block rows) is eqf_vio_amd/tiled.py; the
 * entry points below (and the dense tile kernels eqf_tile_* of eqf_vio_amd_debug.h, for a host that writes its own schedule) are what a rank
 * runs between two exchanges.  They enqueue on the handle's stream (eqf_tiled_set_stream; NULL = the
 * default stream) and return; getters synchronise.  fp64 only.
 * Landmark churn (VIOFilter.cpp:345-443) works on SLOTS: the partition is over the handle's N physical landmark slots, a removed
 * landmark leaves an inactive slot behind (zero rows / columns of Sigma with a unit diagonal block, identity linearisation, no
 * measurement rows: a decoupled block that both factorisations carry along as exact zeros), a new landmark takes a free slot -- nothing
 * ever moves between ranks (eqf_tiled_edit_landmarks).  Which landmark sits in which slot, and the reference's landmark ORDER, are the
 * caller's (eqf_vio_amd/tiled.py: TiledFilter); every per-landmark array of the getters below is in SLOT order, holes included.
 * ================================================================================================================================ */
typedef struct eqf_tiled eqf_tiled; /* opaque */

/* VIOFilter(const Settings&) (VIOFilter.cpp:60-73) for the replicated part of one filter with room for capacity_landmarks. */
int eqf_tiled_create(const eqf_settings* settings, int capacity_landmarks, int device, eqf_tiled** out);
void eqf_tiled_destroy(eqf_tiled* t);
int eqf_tiled_set_stream(eqf_tiled* t, void* stream);
/* The rank's share: rowMap[nlr] / colMap[nlc] = global landmark index of every local row / column landmark (host arrays, copied). */
int eqf_tiled_set_geometry(eqf_tiled* t, int nlr, const int* rowMap, int nlc, const int* colMap);

/* VIOFilter::processIMUData (is_imu = 1, VIOFilter.cpp:120-131) or the integrateUpToTime of processVisionData (is_imu = 0, :233;
 * omega / accel ignored): state, base panel and -- when the call does a Riccati step -- the local blocks Sll in place
 * (VIOFilter.cpp:188-189, F = [[F_bb, 0], [L, D]]).  Sll may be NULL while there are no landmarks.  Returns EQF_OK or the
 * EQF_SKIPPED_* code of the reference's silent early-outs. */
int eqf_tiled_propagate(eqf_tiled* t, double stamp, const double* omega, const double* accel, int is_imu, double* Sll, int ldl);
/* K <= 16 consecutive calls of eqf_tiled_propagate as ONE pass over the local blocks: the IMU calls between two vision frames and, with
 * last_is_vision, the vision call's integrateUpToTime as the last one (stamps[K]; omega / accel [K][3], rows of IMU calls only are read).
 * Every call keeps its own linearisation and its own base panel (K small O(N) launches), the Riccati steps of the local blocks are applied
 * back to back in registers (VIOFilter.cpp:188-189 K times; Sll is read and written once).  status[k] = what eqf_tiled_propagate would have
 * returned for call k; the state afterwards is the state after the K calls, call for call. */
int eqf_tiled_propagate_burst(eqf_tiled* t, int K, const double* stamps, const double* omega, const double* accel, int last_is_vision,
    double* Sll, int ldl, int* status);
/* addNewLandmarks on an empty state (VIOFilter.cpp:345-391, :361-366): n landmarks p0 = y * initialSceneDepth, Q = identity;
 * bearings[n][3] host memory.  Sll (geometry set for n landmarks) is initialised: initialPointVariance on the diagonal.
 * EQF_ERR_UNSUPPORTED if the filter already has landmarks. */
int eqf_tiled_add_landmarks(eqf_tiled* t, int n, const double* bearings, double* Sll, int ldl);
/* removeLandmarkAtIndex (VIOFilter.cpp:421-427; called by removeOldLandmarks :393-419 and removeOutliers :429-443) for the n_remove
 * slots remove_slots[], then addNewLandmarks (:345-391) into the n_add free slots add_slots[] (slots freed by this very call included):
 * p0 = add_bearings[k] * depth (the caller's median scene depth, :358-366), Q = identity, zero cross-covariances,
 * initialPointVariance I on the diagonal.  new_num_slots = slots in use afterwards (>= 1 + the highest active slot; eqf_tiled_num_landmarks
 * returns it).  The geometry in force (eqf_tiled_set_geometry) must cover max(old, new) slots -- the rank's blocks of the marked slots
 * are cleared in Sll through it; shrink the geometry AFTER the call.  Host arrays; synchronises.  EQF_ERR_INVALID (before any effect) if
 * a removed slot is empty, an added slot taken, an active slot would fall above new_num_slots, or the working set would GROW over a slot
 * that this call does not fill (every slot in [old count, new_num_slots) must be in add_slots: a slot that was never initialised has no
 * unit diagonal block to decouple it); EQF_ERR_CAPACITY beyond the capacity. */
int eqf_tiled_edit_landmarks(eqf_tiled* t, int n_remove, const int* remove_slots, int n_add, const int* add_slots,
    const double* add_bearings, double depth, int new_num_slots, double* Sll, int ldl);
/* First half of the update (VIOFilter.cpp:264-277, EqFMatrices.cpp:319-344, :221-235): residual, C0i, lift rows; then the operands of
 * the two factorisations from the local blocks:
 *   M (2 nlr x ldm): columns [0, 2 nlc) S_IJ = C_I Sigma_IJ C_J^T (+ measurementVariance on the global diagonal), [2 nlc, 5 nlc)
 *     (C Sigma)_IJ, [5 nlc, 5 nlc + 18) the narrow right-hand sides [(C Sigma)_Ib (11) | delta_I | V_I = C_I Z_I (6)];
 *   E (3 nlr x lde): columns [0, 3 nlc) Sigma_IJ - Pg_I^T Pg_J (Schur complement of Sigma_e = Sigma[6:, 6:] after its five base
 *     coordinates, EqFMatrices.cpp:239), [3 nlc, 3 nlc + 11) [Z_I (6) | -Pg_I^T Lg^-1 (5)];  G11 (11 x 11): the base part of
 *     [Zt | Et]^T [Zt | Et].
 * bearings[N][3] host memory, in SLOT order (an inactive slot's entry is ignored); copied into a pinned staging buffer before the call
 * returns -- the upload and everything else is enqueued, nothing waits for the device.  bearings = NULL: already staged by
 * eqf_tiled_stage_bearings (a caller that replays a captured hipGraph of the update stages, then launches the graph).
 * eqf_tiled_pingpong: bit 0 / bit 1 = which of the two state / base-panel buffers is current (the device pointers of an update's launches
 * depend on it: a captured graph is valid for one value). */
int eqf_tiled_stage_bearings(eqf_tiled* t, const double* bearings);
int eqf_tiled_pingpong(eqf_tiled* t);
int eqf_tiled_update_prep(eqf_tiled* t, const double* bearings, const double* Sll, int ldl, double* M, int ldm, double* E, int lde,
    double* G11);
/* Second half (VIOFilter.cpp:279-297, EqFMatrices.cpp:173-275): acc (18 x ldacc, columns = 3 N in GLOBAL landmark order) = sum_k
 * Yn_k^T Y_k, Gnn (18 x 18) = sum_k Yn_k^T Yn_k, G11 (11 x 11) complete; gamma = K delta, bundleLift, Delta, X <- Delta X, bias +=
 * gamma[0:6]; the base panel's share of Sigma - K C Sigma.  (The local blocks were downdated by eqf_tile_gemm_tn as the solved block
 * rows arrived.) */
int eqf_tiled_update_finish(eqf_tiled* t, const double* acc, int ldacc, const double* Gnn, const double* G11);

int eqf_tiled_synchronize(eqf_tiled* t);
int eqf_tiled_num_landmarks(eqf_tiled* t);
int eqf_tiled_get_time(eqf_tiled* t, double* time);
int eqf_tiled_device_error(eqf_tiled* t);
/* as eqf_get_state_estimate / eqf_get_origin / eqf_get_group / eqf_get_bias / eqf_get_last_update / eqf_get_integrator */
int eqf_tiled_get_state_estimate(eqf_tiled* t, double* pose_q, double* pose_x, double* velocity, double* p);
int eqf_tiled_get_origin(eqf_tiled* t, double* pose_q, double* pose_x, double* velocity, double* p);
int eqf_tiled_get_group(eqf_tiled* t, double* A_q, double* A_x, double* w, double* Q_q, double* Q_a);
int eqf_tiled_get_bias(eqf_tiled* t, double* bias6);
int eqf_tiled_get_last_update(eqf_tiled* t, double* delta, double* gamma, double* Gamma);
int eqf_tiled_get_integrator(eqf_tiled* t, double* currentVelocity6, double* accumulatedVelocity6, double* accumulatedTime, int* initialised);
/* The replicated base rows Sigma[0:11, 0:11+3N] in the reference's index map (11 x ld, host memory). */
int eqf_tiled_get_base(eqf_tiled* t, double* dst, int ld);
/* State injection (as eqf_set_state; sigma_base = the first 11 rows of Sigma, 11 x ld, reference index map).  The caller fills Sll. */
int eqf_tiled_set_state(eqf_tiled* t, int N, const double* pose_q, const double* pose_x, const double* velocity, const double* p0,
    const double* A_q, const double* A_x, const double* w, const double* Q_q, const double* Q_a, const double* bias6,
    const double* sigma_base, int ld, double currentTime, const double* currentVelocity6, const double* accumulatedVelocity6,
    double accumulatedTime, int initialised);

/* ================================================================================================================================
 * The HOST LOOP of the partitioned filter behind the C ABI (csrc/eqf_tiledf.hip; round 5 -- until then it was Python): one eqf_tf per
 * rank of a Pr x Pc process grid (Pr | Pc; rank = pr * Pc + pc) IS VIOFilter (VIOFilter.h:41-88) for one filter whose Sigma is
 * partitioned over the grid.  Every rank makes the same calls with the same arguments.  The handle owns its eqf_tiled, its local matrix,
 * every exchange buffer and four HIP streams (two pairs with disjoint CU sets: reserve_cus CUs for the look-ahead factorisations, < 0 =
 * default 24 / EQF_TILED_RESERVE_CUS, 0 = plain streams).  What the ranks exchange goes through ONE callback:
 *   bcast(ctx, group, chain, root, buf, bytes, stream): broadcast `bytes` bytes of DEVICE memory at `buf` from `root` to the other members
 *   of `group` -- 0: my process row (root = process COLUMN of the sender), 1: my process column (root = process ROW), 2: every rank (root =
 *   rank) -- ordered on the HIP stream `stream` (the transfer may start when the stream reaches it; later work on the stream sees the data).
 *   chain = 0 / 1: the two factorisations of an update run side by side on different streams -- a collective library that cannot have two
 *   operations of one communicator in flight gets one communicator per chain.  Returns 0 on success.  With RCCL: ncclBroadcast(buf, buf,
 *   bytes, ncclChar, root, rowComm / colComm / worldComm [chain], stream).  A 1 x 1 grid needs no callback (comm = NULL).
 * eqf_tf_process_imu / eqf_tf_process_vision return EQF_OK, the EQF_SKIPPED_* code of the reference's silent early-outs, or an error
 * (EQF_ERR_UNSORTED: ids not strictly ascending, VIOFilter.cpp:239-240; EQF_ERR_CAPACITY; EQF_ERR_NUMERIC: a pivot of S or Sigma_e not
 * positive, looked at every check_every-th update).  Getters answer in the REFERENCE's landmark order (insertion order, :211-230); the
 * landmark slots behind it (eqf_tiled, above) are internal.  eqf_tf_get_sigma is collective (every rank calls it).
 * Options (eqf_tf_set_option): "lookahead" (1), "overlap_chains" (1 on one rank, 0 on a grid: the interleaved chains are not validated over RCCL on a node; EQF_TILED_OVERLAP_CHAINS), "burst" (1: IMU calls queued and sent as
 * bursts), "check_every" (1), "downdate_slices" (0: the covariance downdate Sigma - Y^T Y on the fp64 matrix cores, parity grade; 5 / 6 / 7: on the INTEGER matrix pipe from
 * that many 7-bit slices of Y's columns with exact accumulation -- Sigma within 1e-4 of the fp64 path from 6 slices on (measured 2e-6 at N = 200 .. 6e-5 at N = 4000), two thirds of the downdate's time;
 * round 6, csrc/eqf_i8.hpp), "chain_slices" (0: the two factorisations' trailing products on the fp64 matrix cores; 5 / 6 / 7: on the integer pipe in the same
 * way -- they forgive more than the downdate: five slices keep Sigma to 1e-8 and the pose to 3e-9 of the fp64 path on the bench stream), "downdate_early" (50: with the chains side by side and the fp64 downdate, the shares Y_k^T Y_k of this percentage of the S-chain's block rows are subtracted on the
 * E-chain's stream as soon as each block row is solved, the rest in one product behind the S-chain; 0: the whole downdate behind the S-chain, as until round 6),
 * "trsm_leaf" (0: a block row's triangular solve is split once into two solves and a product; > 0: recursively, down to this many 64-row blocks -- measured slower at N = 4000),
 * "profiling" (0: event brackets per phase, eqf_tf_get_phases in eqf_vio_amd_debug.h), "graphs" (0: hipGraph replay of an update on a
 * one-rank grid, see eqf_tf_graph_launches in eqf_vio_amd_debug.h).
 * ================================================================================================================================ */
typedef struct eqf_tf eqf_tf; /* opaque */
typedef struct eqf_tf_comm {
    void* ctx;
    int (*bcast)(void* ctx, int group, int chain, int root, void* buf, size_t bytes, void* stream);
} eqf_tf_comm;
int eqf_tf_create(const eqf_settings* settings, int capacity_landmarks, int block_landmarks, int Pr, int Pc, int rank, int device,
    int reserve_cus, const eqf_tf_comm* comm, eqf_tf** out);
void eqf_tf_destroy(eqf_tf* f);
int eqf_tf_set_option(eqf_tf* f, const char* name, int value);
/* VIOFilter::processIMUData (VIOFilter.cpp:120-131) / processVisionData (:232-302; ids[n] strictly ascending, bearings[n][3], host) */
int eqf_tf_process_imu(eqf_tf* f, double stamp, const double* omega, const double* accel);
int eqf_tf_process_vision(eqf_tf* f, double stamp, int n, const int* ids, const double* bearings);
int eqf_tf_synchronize(eqf_tf* f);
int eqf_tf_check(eqf_tf* f);        /* EQF_ERR_NUMERIC if a pivot was not positive since the last look (synchronises) */
int eqf_tf_device_error(eqf_tf* f); /* as eqf_device_error */
int eqf_tf_num_landmarks(eqf_tf* f);
int eqf_tf_num_slots(eqf_tf* f);
int eqf_tf_get_ids(eqf_tf* f, int* ids, int* slots); /* reference order; slots may be NULL */
int eqf_tf_get_time(eqf_tf* f, double* time);
int eqf_tf_get_state_estimate(eqf_tf* f, double* pose_q, double* pose_x, double* velocity, double* p);
int eqf_tf_get_bias(eqf_tf* f, double* bias6);
int eqf_tf_get_last_update(eqf_tf* f, double* delta, double* gamma, double* Gamma);
/* VIOFilter::stateCovariance (:306-309): dst (n x n, ld), n = 11 + 3 N in the reference's order (slot_order = 0) or 11 + 3 * slots over
 * all slots in use, holes included (slot_order = 1: tests of the hole invariants).  Host memory. */
int eqf_tf_get_sigma(eqf_tf* f, double* dst, int ld, int slot_order);
/* restart from a snapshot, as eqf_set_state (sigma: the DENSE covariance, every rank holds it once) */
int eqf_tf_set_state(eqf_tf* f, int N, const int* ids, const double* pose_q, const double* pose_x, const double* velocity, const double* p0,
    const double* A_q, const double* A_x, const double* w, const double* Q_q, const double* Q_a, const double* bias6, const double* sigma, int ld,
    double currentTime, const double* currentVelocity6, const double* accumulatedVelocity6, double accumulatedTime, int initialised);
int eqf_tf_get_churn_stats(eqf_tf* f, long long* stats3); /* removed_old, removed_outliers, added */
int eqf_tf_local_matrix(eqf_tf* f, double** ptr, int* rows, int* cols, int* ld);
const char* eqf_tf_last_error(eqf_tf* f);
const char* eqf_version(void);
/* "src_sha256=<hex>": sha256 over the library's sources (every .hip and .hpp file of csrc/, the two headers of include/, csrc/Makefile; concatenated in sorted
 * order) at build time -- lets a caller prove that the .so it loaded was built from the sources beside it (bench.py's `build` block). */
const char* eqf_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* EQF_VIO_AMD_H */
