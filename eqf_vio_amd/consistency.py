"""Filter consistency on the host (pure numpy): what turns the covariance in the coordinates of the estimate
(FilterBatch.sigma_local / marginals, include/eqf_vio_amd.h: eqf_get_sigma_local) into a number for a Monte-Carlo batch.

Sigma is the covariance of eps = chart_xi0(phi_{X^-1}(xi)): coordinates around the ORIGIN xi0 (VIOFilter.cpp:306-309, "TODO: propagate to
local tangent space").  The error one can measure against a ground truth is eps_loc = chart_xiHat(xi), xiHat = phi_X(xi0) the estimate;
to first order eps_loc = J eps with the block-diagonal J of local_jacobian_blocks, and Sigma_loc = J Sigma J^T.

  local_jacobian_blocks(origin, group)   the J blocks (the device builds the same ones: FilterBatch.local_jacobian)
  local_error(estimate, truth, ...)      eps_loc for gravity direction, velocity and landmarks, plus the bias difference
  local_retract(estimate, eps, ...)      its inverse: a drawn eps_loc (FilterBatch.sample_sigma) -> a sampled truth for a Monte-Carlo start
  nees_marginal(marginals, error)        navigation-state NEES (11 or 5 dof) and per-landmark NEES (3 dof), O(N)
  error_vector(error)                    local_error's dict flattened into Sigma's index map
  nees_joint(Sigma, e, first)            the joint NEES e^T A^-1 e, log det A and the smallest pivot over the whole state or a trailing part of
                                         it -- the host counterpart of FilterBatch.nees (include/eqf_vio_amd.h: eqf_get_nees)
  systematic_resample(loglik, u)         log-likelihoods (FilterBatch.innovation_stats) -> parents for FilterBatch.resample
  chi2_gate_threshold(p, dof)            the chi-square quantile: dof = 2 for FilterBatch.set_outlier_gate(GATE_MAHALANOBIS, ...), dof = m for
                                         FilterBatch.update_linear's gate
  velocity_rows / gravity_rows / landmark_rows(N, i)   measurement rows in the estimate's chart for FilterBatch.update_linear(local=True)
  linear_update_host(Sigma, H, resid, R) the numpy statement of that update (include/eqf_vio_amd.h: eqf_update_linear)
  stereo_rows / depth_rows / position_rows   per-landmark blocks (H_k, resid_k) for FilterBatch.update_landmarks(local=True)
  update_landmarks_host(Sigma, idx, H, resid, R, ...)  the dense numpy statement of that update (eqf_update_landmarks)
  schmidt_update_host(Sigma, Ht, R, resid, consider_idx)  the numpy statement of the Schmidt (consider) variants of both updates
  mixture_weights(loglik)                log-likelihoods -> the normalised weights of a mixture (systematic_resample's)
  mixture_moments_host(members, w, centre, centred)   mean and covariance of a weighted batch in the chart of a centre state, the spread
                                         between the members included -- the numpy statement of FilterBatch.mixture_moments
  merge_host(members, w, ref)            ... and of FilterBatch.merge: the one state and covariance that match the batch's first two moments
  forecast_host(flt, imu, t1, ...)       the numpy statement of FilterBatch.forecast (include/eqf_vio_amd.h: eqf_forecast) on a filter object
                                         with the reference's interface: a copy runs the calls, the handle's outputs are read off it
  output_blocks(origin_p)                C_i (2 x 3) of every landmark, the diagonal blocks of the output matrix C0 (EqFMatrices.cpp:319-344)
  bearing_cov_host(p, P_loc)             covariance of the unit bearing p / |p| from the landmark's block in the estimate's chart (`ycov`)
  search_ellipse(ycov, dpix_dy, p)       ... as a 2 x 2 pixel covariance and the semi-axes of its chi-square ellipse, for a tracker
  gate_distance(S, delta)                the d2 a hypothesised residual would get from forecast's S (the Mahalanobis gate's number)

`origin`, `group`, `estimate` are the dicts of FilterBatch.origin() / group() / state_estimate(): quaternions (w, x, y, z), Eigen semantics.
"""
import numpy as np

E3 = np.array([0.0, 0.0, 1.0])


# ---- quaternions / sphere charts with the reference's formulas (libs/core SO3.cpp, VIOState.cpp:199-251)
def quat_to_matrix(q):
    """Eigen toRotationMatrix (SO3.cpp:94)."""
    w, x, y, z = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def _quat_from_matrix(m):
    """Eigen matrix -> quaternion (SO3.cpp:100)."""
    t = m[0, 0] + m[1, 1] + m[2, 2]
    q = np.zeros(4)
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[0] = 0.5 * t
        t = 0.5 / t
        q[1], q[2], q[3] = (m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t
        return q
    i = 0
    if m[1, 1] > m[0, 0]:
        i = 1
    if m[2, 2] > m[i, i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
    q[1 + i] = 0.5 * t
    t = 0.5 / t
    q[0] = (m[k, j] - m[j, k]) * t
    q[1 + j] = (m[j, i] + m[i, j]) * t
    q[1 + k] = (m[k, i] + m[i, k]) * t
    return q


def _quat_inverse(q):
    q = np.asarray(q, dtype=float)
    return np.array([q[0], -q[1], -q[2], -q[3]]) / float(q @ q)


def _quat_rotate(q, v):
    """Eigen _transformVector (SO3.cpp:66)."""
    u = np.asarray(q[1:4], dtype=float)
    uv = np.cross(u, v)
    uv = uv + uv
    return v + q[0] * uv + np.cross(u, uv)


def _skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def _sphere_rot(pole):
    """SO3FromVectors(-pole, e3) as the quaternion the reference stores (VIOState.cpp:231, SO3.cpp:155-167)."""
    o = -np.asarray(pole, dtype=float)
    o = o / np.linalg.norm(o)
    v = np.cross(o, E3)
    c = float(o @ E3)
    if abs(1 + c) <= 1e-8:
        raise ValueError("the gravity chart is singular: its pole is e3 (SO3.cpp:160)")
    vx = _skew(v)
    return _quat_from_matrix(np.eye(3) + (vx + 1.0 / (1.0 + c) * vx @ vx))


def stereo_sphere_chart(eta, pole):
    """VIOState.cpp:230-234."""
    r = _quat_rotate(_sphere_rot(pole), np.asarray(eta, dtype=float))
    return (r - E3)[0:2] / (1 - r[2])


def stereo_sphere_chart_diff(eta, pole):
    """VIOState.cpp:242-246, 2 x 3."""
    q = _sphere_rot(pole)
    r = _quat_rotate(q, np.asarray(eta, dtype=float))
    D = np.eye(3)[0:2, :] @ (np.eye(3) * (1 - r[2]) + np.outer(r - E3, E3))
    return (1 - r[2]) ** -2.0 * D @ quat_to_matrix(q)


def stereo_sphere_chart_inv_diff_at_zero(pole):
    """VIOState.cpp:248-251 at y = 0, 3 x 2."""
    D = np.zeros((3, 2))
    D[0, 0] = D[1, 1] = 2.0
    return quat_to_matrix(_quat_inverse(_sphere_rot(pole))) @ D


def gravity_dir(pose_q):
    """R^T e3 (VIOState.cpp:90)."""
    return _quat_rotate(_quat_inverse(pose_q), E3)


# ---- the three functions
def local_jacobian_blocks(origin, group):
    """Blocks of J = d chart_xiHat(phi_X(chart_xi0^-1(eps))) / d eps at eps = 0, in Sigma's index map:
    [0,6) bias I (not returned); [6,8) G (2,2); [8,11) RAt (3,3) = R_A^T; landmark i lm[i] (3,3) = a_i^-1 R(q_i)^T."""
    Aq = np.asarray(group["Aq"], dtype=float)
    RAt = quat_to_matrix(_quat_inverse(Aq))
    eta0 = gravity_dir(origin["q"])
    etaHat = _quat_rotate(_quat_inverse(Aq), eta0)
    G = stereo_sphere_chart_diff(etaHat, etaHat) @ RAt @ stereo_sphere_chart_inv_diff_at_zero(eta0)
    return dict(G=G, RAt=RAt, lm=landmark_jacobian_blocks(group))


def landmark_jacobian_blocks(group):
    """The landmark blocks of local_jacobian_blocks alone, (N, 3, 3): a_i^-1 R(q_i)^T.  They do not depend on the gravity chart."""
    Qq = np.asarray(group["Qq"], dtype=float).reshape(-1, 4)
    Qa = np.asarray(group["Qa"], dtype=float).reshape(-1)
    lm = np.zeros((len(Qa), 3, 3))
    for i in range(len(Qa)):
        lm[i] = quat_to_matrix(Qq[i]).T / Qa[i]
    return lm


def jacobian_matrix(blocks):
    """The dense (11 + 3N) x (11 + 3N) J of the blocks (tests, small N)."""
    N = len(blocks["lm"])
    J = np.zeros((11 + 3 * N, 11 + 3 * N))
    J[0:6, 0:6] = np.eye(6)
    J[6:8, 6:8] = blocks["G"]
    J[8:11, 8:11] = blocks["RAt"]
    for i in range(N):
        J[11 + 3 * i : 14 + 3 * i, 11 + 3 * i : 14 + 3 * i] = blocks["lm"][i]
    return J


def local_error(estimate, truth, bias=None, true_bias=None):
    """eps_loc = chart_xiHat(xi_true): dict with `gravity` (2,), `velocity` (3,), `lm` (N,3) and `bias` (6,), all "truth minus estimate"
    like every chart coordinate here (the bias difference is zero if no bias is given).
    estimate / truth: dicts with q (pose attitude), v (body velocity), p (N,3) body-frame landmarks."""
    etaHat = gravity_dir(estimate["q"])
    eta = gravity_dir(truth["q"])
    b = np.zeros(6)
    if bias is not None and true_bias is not None:
        b = np.asarray(true_bias, dtype=float) - np.asarray(bias, dtype=float)
    return dict(
        bias=b,
        gravity=stereo_sphere_chart(eta, etaHat),
        velocity=np.asarray(truth["v"], dtype=float) - np.asarray(estimate["v"], dtype=float),
        lm=np.asarray(truth["p"], dtype=float).reshape(-1, 3) - np.asarray(estimate["p"], dtype=float).reshape(-1, 3),
    )


def stereo_sphere_chart_inv(y, pole):
    """VIOState.cpp:236-240 (e3ProjectSphereInv, :206-211, turned back by the chart's rotation)."""
    ybar = np.array([y[0], y[1], 0.0])
    r = E3 + 2.0 / (float(ybar @ ybar) + 1.0) * (ybar - E3)
    return _quat_rotate(_quat_inverse(_sphere_rot(pole)), r)


def _quat_mul(a, b):
    """SO3.cpp:76."""
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def local_retract(estimate, eps, bias=None):
    """Inverse of local_error: the state xi = chart_xiHat^-1(eps) whose error against `estimate` is eps -- what turns a draw eps_loc ~ N(0,
    Sigma_loc) (FilterBatch.sample_sigma(local=True)) into a sampled TRUTH for a Monte-Carlo start.
    eps: local_error's dict, or one vector in the reference's index map (error_vector; (11 + 3N,)).  Returns a dict with q, v, p, and
    `bias` = bias + eps_bias when a bias is given.  The gravity direction is stereo_sphere_chart^-1(eps_gravity, etaHat); the attitude is the
    estimate's turned by the SHORTEST rotation that takes its gravity direction there.  The chart only fixes the direction of gravity: yaw
    is unobservable, is not part of the error and stays the estimate's.  A tilt of pi (eps_gravity at infinity) has no shortest rotation."""
    if not isinstance(eps, dict):
        e = np.asarray(eps, dtype=float)
        eps = dict(bias=e[0:6], gravity=e[6:8], velocity=e[8:11], lm=e[11:].reshape(-1, 3))
    q = np.asarray(estimate["q"], dtype=float)
    etaHat = gravity_dir(q)
    eta = stereo_sphere_chart_inv(np.asarray(eps["gravity"], dtype=float), etaHat)
    # R_true^T e3 = eta with R_true = R_hat D^T, D the rotation etaHat -> eta about etaHat x eta (Rodrigues, as SO3.cpp:155-167)
    v = np.cross(etaHat, eta)
    c = float(etaHat @ eta)
    if abs(1.0 + c) <= 1e-8:
        raise ValueError("a gravity tilt of pi has no shortest rotation")
    vx = _skew(v)
    D = np.eye(3) + vx + vx @ vx / (1.0 + c)
    # (eps_gravity = 0 is the estimate's own direction: the attitude keeps every bit)
    qn = _quat_mul(q, _quat_inverse(_quat_from_matrix(D))) if np.any(np.asarray(eps["gravity"], dtype=float) != 0.0) else q.copy()
    out = dict(q=qn, v=np.asarray(estimate["v"], dtype=float) + np.asarray(eps["velocity"], dtype=float),
               p=np.asarray(estimate["p"], dtype=float).reshape(-1, 3) + np.asarray(eps["lm"], dtype=float).reshape(-1, 3))
    if "x" in estimate:
        out["x"] = np.asarray(estimate["x"], dtype=float).copy()
    if bias is not None:
        out["bias"] = np.asarray(bias, dtype=float) + np.asarray(eps["bias"], dtype=float)
    return out


def nees_marginal(marginals, error, with_bias=True):
    """Normalised estimation error squared from the marginals of Sigma_loc (FilterBatch.marginals(local=True): base (11,11), lm (N,3,3)):
    `nav` = e^T P^-1 e over the navigation state -- 11 dof with the bias, 5 (gravity direction + velocity) without -- and `lm` (N,), 3 dof each."""
    base = np.asarray(marginals["base"], dtype=float)
    e = np.concatenate([error["bias"], error["gravity"], error["velocity"]])
    if not with_bias:
        base, e = base[6:, 6:], e[6:]
    nav = float(e @ np.linalg.solve(base, e))
    P = np.asarray(marginals["lm"], dtype=float).reshape(-1, 3, 3)
    el = np.asarray(error["lm"], dtype=float).reshape(-1, 3)
    lm = np.array([el[i] @ np.linalg.solve(P[i], el[i]) for i in range(len(el))])
    return dict(nav=nav, nav_dof=len(e), lm=lm, lm_dof=3)


def error_vector(error, with_bias=True):
    """local_error's dict as one vector in the reference's index map: [0,6) bias, [6,8) gravity direction, [8,11) velocity, then the
    landmarks (11 + 3N,); without the bias the first six entries are zero (use first=6 with nees_joint / FilterBatch.nees)."""
    b = np.asarray(error["bias"], dtype=float) if with_bias else np.zeros(6)
    return np.concatenate([b, error["gravity"], error["velocity"], np.asarray(error["lm"], dtype=float).reshape(-1)])


def nees_joint(Sigma, e, first=0):
    """Joint NEES over the trailing principal submatrix A = Sigma[first:, first:] (first = 0 whole state, 6 without the bias, 11 landmarks
    only): numpy Cholesky A = L L^T of the LOWER triangle, z = L^-1 e.  e: (n,) or (nrhs, n) in Sigma's index map (entries below `first`
    are ignored).  Returns dict(nees (scalar or (nrhs,)), logdet = 2 sum log L_kk, min_pivot = min L_kk^2, dof); an empty A gives
    nees 0, logdet 0, min_pivot inf.  Raises numpy.linalg.LinAlgError if A is not positive definite."""
    S = np.asarray(Sigma, dtype=float)
    A = np.tril(S[first:, first:])
    A = A + np.tril(A, -1).T
    ev = np.asarray(e, dtype=float)
    E = np.atleast_2d(ev)[:, first:]
    if A.shape[0] == 0:
        nees, logdet, mp = np.zeros(E.shape[0]), 0.0, np.inf
    else:
        L = np.linalg.cholesky(A)
        d = np.diag(L)
        z = np.linalg.solve(L, E.T)
        nees, logdet, mp = np.sum(z * z, axis=0), 2.0 * float(np.sum(np.log(d))), float(np.min(d * d))
    return dict(nees=float(nees[0]) if ev.ndim == 1 else nees, logdet=logdet, min_pivot=mp, dof=A.shape[0])


def _gamma_p(a, t):
    """Regularised lower incomplete gamma function P(a, t), a > 0, t >= 0: the series t^a e^-t sum_n t^n / Gamma(a + n + 1) for t < a + 1,
    otherwise 1 - Q from the continued fraction (modified Lentz).  Both stop at the rounding level."""
    import math

    if t <= 0.0:
        return 0.0
    pre = math.exp(-t + a * math.log(t) - math.lgamma(a))
    if t < a + 1.0:
        term = total = 1.0 / a
        n = 0
        while abs(term) > 1e-17 * abs(total) and n < 10000:
            n += 1
            term *= t / (a + n)
            total += term
        return pre * total
    tiny = 1e-300
    b = t + 1.0 - a
    c, d = 1.0 / tiny, 1.0 / b
    h = d
    for i in range(1, 10000):
        an = -i * (i - a)
        b += 2.0
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1.0 / d
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 1e-16:
            break
    return 1.0 - pre * h


def chi2_cdf(x, dof):
    """CDF of the chi-square distribution with `dof` degrees of freedom.  Even dof: the closed form 1 - e^(-x/2) sum_{j < dof/2} (x/2)^j / j!;
    odd dof: the regularised gamma function P(dof / 2, x / 2) (series / continued fraction).  No scipy."""
    import math

    x, dof = float(x), int(dof)
    if dof < 1:
        raise ValueError("dof must be at least 1")
    if x <= 0.0:
        return 0.0
    t = 0.5 * x
    if dof % 2 == 0 and t < 30.0:  # (beyond, 1 - tail cancels less well than the continued fraction's 1 - Q: both are 1 to rounding)
        term = total = 1.0
        for j in range(1, dof // 2):
            term *= t / j
            total += term
        return -math.expm1(-t + math.log(total))
    return _gamma_p(0.5 * dof, t)


def chi2_gate_threshold(p, dof=2):
    """Threshold of a chi-square gate that keeps an honest measurement with probability p: the quantile of the chi-square distribution with
    `dof` degrees of freedom.  dof = 2 (the Mahalanobis outlier gate of a landmark's bearing, FilterBatch.set_outlier_gate(GATE_MAHALANOBIS,
    ...)): the CDF is 1 - exp(-x / 2), the quantile exactly -2 ln(1 - p) (5.991 / 9.210 / 13.816 at 0.95 / 0.99 / 0.999).  Any other dof
    (FilterBatch.update_linear's gate: dof = m): bisection on chi2_cdf down to neighbouring doubles.  It presumes a converged, consistent
    filter: while Sigma is as wide as initialPointVariance leaves it, d2 of a gross error is small."""
    p = float(p)
    if not 0.0 < p < 1.0:
        raise ValueError("p must lie in (0, 1)")
    if int(dof) != dof or dof < 1:
        raise ValueError("dof must be a positive integer")
    if dof == 2:
        return -2.0 * float(np.log1p(-p))
    lo, hi = 0.0, float(dof)
    while chi2_cdf(hi, dof) < p:
        lo, hi = hi, 2.0 * hi
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            break
        if chi2_cdf(mid, dof) < p:
            lo = mid
        else:
            hi = mid
    return hi


# ---- rows of the usual linear measurements for FilterBatch.update_linear(local=True): eps_loc is "truth minus estimate" in the estimate's
# chart -- gravity direction [6, 8), body velocity [8, 11), body-frame landmark i [11 + 3 i, 14 + 3 i) -- so a measurement of one of these
# quantities has unit rows, and its residual is "measured minus the estimate's value"
def _unit_rows(N, first, count):
    H = np.zeros((count, 11 + 3 * int(N)))
    H[np.arange(count), first + np.arange(count)] = 1.0
    return H


def velocity_rows(N):
    """(3, 11 + 3N): the body velocity -- a zero-velocity detection (resid = 0 - v_hat), wheel or GNSS speed in the body frame."""
    return _unit_rows(N, 8, 3)


def gravity_rows(N):
    """(2, 11 + 3N): the gravity direction in the stereographic chart around the estimate's (resid = stereo_sphere_chart(eta_measured,
    gravity_dir(q_hat))) -- an attitude reference."""
    return _unit_rows(N, 6, 2)


def landmark_rows(N, i):
    """(3, 11 + 3N): body-frame position of landmark i -- a surveyed or range-and-bearing point (resid = p_measured - p_hat[i])."""
    if not 0 <= int(i) < int(N):
        raise ValueError("no such landmark")
    return _unit_rows(N, 11 + 3 * int(i), 3)


def linear_update_host(Sigma, H, resid, R):
    """The numpy statement of FilterBatch.update_linear's arithmetic for one filter (include/eqf_vio_amd.h: eqf_update_linear), H already in
    Sigma's coordinates (for local rows pass H @ jacobian_matrix(blocks), or Sigma_loc):
        B = Sigma H^T, S = H B + R = L L^T (lower triangle of R), Y = L^-1 B^T, z = L^-1 resid, gamma = Y^T z, Sigma+ = Sigma - Y^T Y.
    Returns dict(Sigma, gamma, nis = z^T z, logdet_S = 2 sum log L_kk, loglik = -(nis + logdet_S + m log 2 pi) / 2, dof = m, Y, L).
    Raises numpy.linalg.LinAlgError if S is not positive definite."""
    Sg = np.asarray(Sigma, dtype=float)
    H = np.atleast_2d(np.asarray(H, dtype=float))
    r = np.asarray(resid, dtype=float).reshape(-1)
    m = H.shape[0]
    Rl = np.tril(np.asarray(R, dtype=float).reshape(m, m))
    Rl = Rl + np.tril(Rl, -1).T
    B = Sg @ H.T
    S = H @ B + Rl
    L = np.linalg.cholesky(np.tril(S) + np.tril(S, -1).T)
    Y = np.linalg.solve(L, B.T)
    z = np.linalg.solve(L, r)
    nis = float(z @ z)
    logdet = 2.0 * float(np.sum(np.log(np.diag(L))))
    return dict(Sigma=Sg - Y.T @ Y, gamma=Y.T @ z, nis=nis, logdet_S=logdet, loglik=-0.5 * (nis + logdet + m * float(np.log(2.0 * np.pi))), dof=m,
                Y=Y, L=L)


def consider_indices(landmarks):
    """The state indices c (reference index map: 11 + 3 i ..) of the landmark INDICES `landmarks`, ascending: what schmidt_update_host takes."""
    return np.array([11 + 3 * int(i) + k for i in sorted(int(j) for j in landmarks) for k in range(3)], dtype=np.int64)


def schmidt_update_host(Sigma, Ht, R, resid, consider_idx):
    """The numpy statement of the Schmidt (consider) updates for one filter (include/eqf_vio_amd.h: eqf_update_linear_schmidt /
    eqf_update_landmarks_schmidt; FilterBatch.update_linear / update_landmarks with consider=...).  Ht (m, n) already in Sigma's coordinates
    (the dense rows: landmark_blocks_matrix(...) for per-landmark blocks), R (m, m: lower triangle read), consider_idx: the state indices
    c that keep their estimate and their covariance block (consider_indices(...)).  With B, S = L L^T, Y, z of linear_update_host -- the full
    update's, Ht may have columns in c -- the gain K = Y^T L^-1 has its rows c set to zero and the Joseph form
    (I - K Ht) Sigma (I - K Ht)^T + K R K^T gives
        gamma = Y^T z off c, +0.0 on c;    Sigma+ = Sigma - Y^T Y except on c x c, where Sigma+ = Sigma.
    Returns dict(gamma, Sigma, nis, logdet_S, loglik, dof): nis, logdet_S, loglik, dof are the full update's.  With an empty set every value
    is linear_update_host's.  Raises numpy.linalg.LinAlgError if S is not positive definite."""
    Sg = np.asarray(Sigma, dtype=float)
    c = np.asarray(consider_idx, dtype=np.int64).reshape(-1)
    if len(c) and (c.min() < 0 or c.max() >= len(Sg) or len(np.unique(c)) != len(c)):
        raise ValueError("consider_idx: distinct state indices")
    r = linear_update_host(Sg, Ht, resid, R)
    Sp, gamma = r["Sigma"].copy(), r["gamma"].copy()
    if len(c):
        Sp[np.ix_(c, c)] = Sg[np.ix_(c, c)]
        gamma[c] = 0.0
    return dict(gamma=gamma, Sigma=Sp, nis=r["nis"], logdet_S=r["logdet_S"], loglik=r["loglik"], dof=r["dof"])


# ---- the deterministic split (FilterBatch.split_filters; include/eqf_vio_amd.h: eqf_split_filters)
def split_host(Sigma, Ht, shift, shrink):
    """The numpy statement of FilterBatch.split_filters' arithmetic for one source: Ht (n,) already in Sigma's coordinates (for a local row
    pass a @ jacobian_matrix(blocks)), shift and shrink (K,).
        B = Sigma Ht^T, S = Ht B, u = B / sqrt(S);   Sigma_k = Sigma - shrink_k u u^T,   gamma_k = shift_k u.
    Returns dict(S, u, Sigma (K, n, n), gamma (K, n)).  Raises numpy.linalg.LinAlgError if S is not positive."""
    Sg = np.asarray(Sigma, dtype=float)
    h = np.asarray(Ht, dtype=float).reshape(-1)
    sh = np.atleast_1d(np.asarray(shift, dtype=float))
    sk = np.atleast_1d(np.asarray(shrink, dtype=float))
    B = Sg @ h
    S = float(h @ B)
    if not (S > 0.0 and np.isfinite(S)):
        raise np.linalg.LinAlgError("split_host: the functional's variance is not positive")
    u = B / np.sqrt(S)
    uu = np.outer(u, u)
    return dict(S=S, u=u, Sigma=np.stack([Sg - k * uu for k in sk]), gamma=np.stack([s * u for s in sh]))


def split_components(K, spread, outer_weight=None):
    """Moment-matched components of a split along one functional: (weights, shift, shrink), each (K,), with sum w = 1, sum w shift = 0 and
    sum w (shift^2 - shrink) = 0, so that the children of FilterBatch.split_filters carry the parent's first two moments.  spread: the
    outer components sit at -+spread standard deviations of the functional.
        K = 2: weights (1/2, 1/2), shift (-spread, spread), shrink spread^2.
        K = 3: weights (q, 1 - 2 q, q) with q = outer_weight (default 1/4), shift (-spread, 0, spread), common shrink 2 q spread^2.
    Parameters that would give a shrink outside [0, 1] (or a weight outside (0, 1)) are refused."""
    s = float(spread)
    if not np.isfinite(s) or s < 0.0:
        raise ValueError("split_components: spread must be finite and >= 0")
    if int(K) == 2:
        if outer_weight is not None and float(outer_weight) != 0.5:
            raise ValueError("split_components: two components weigh 1/2 each")
        w, shift, k = np.array([0.5, 0.5]), np.array([-s, s]), s * s
    elif int(K) == 3:
        q = 0.25 if outer_weight is None else float(outer_weight)
        if not 0.0 < q < 0.5:
            raise ValueError("split_components: outer_weight must lie in (0, 1/2)")
        w, shift, k = np.array([q, 1.0 - 2.0 * q, q]), np.array([-s, 0.0, s]), 2.0 * q * s * s
    else:
        raise ValueError("split_components: K is 2 or 3")
    if not 0.0 <= k <= 1.0:
        raise ValueError("split_components: these parameters give a shrink outside [0, 1]")
    return w, shift, np.full(len(w), k)


def depth_axis_row(p_hat, i, n):
    """(n,) the LOCAL row (sigma_local()'s coordinates, split_filters(local=True)) that measures landmark i's camera-frame position along
    its own bearing p_hat / |p_hat|: the depth of the landmark.  n = 11 + 3 N.  The depth-hypothesis split: K children along this row,
    weighted afterwards by score_vision or an innovation log-likelihood and reduced with reduce_mixture."""
    p = np.asarray(p_hat, dtype=float).reshape(3)
    d = float(np.linalg.norm(p))
    n, i = int(n), int(i)
    if i < 0 or 11 + 3 * i + 3 > n or not d > 0.0:
        raise ValueError("depth_axis_row: no such landmark")
    row = np.zeros(n)
    row[11 + 3 * i:14 + 3 * i] = p / d
    return row


# ---- per-landmark blocks for FilterBatch.update_landmarks(local=True): entry k measures landmark i_k alone, resid_k = H_k eps_i + noise with
# eps_i = p_true - p_hat, the plain difference of camera-frame positions (the landmark block of the estimate's chart)
def stereo_rows(p_hat, q_21, t_21, y2):
    """The second camera of a rigid stereo rig sees landmark p_hat (first camera's frame) along the unit bearing y2.  (q_21, t_21): the pose
    of camera 2 in camera 1's frame (quaternion w, x, y, z and position), so p_2 = R_21^T (p_hat - t_21) and y2_hat = p_2 / |p_2|.
    Returns (H (2, 3), resid (2,)): H = stereoSphereChartDiff(y2_hat, y2_hat) (I - y2_hat y2_hat^T) R_21^T / |p_2|,
    resid = stereoSphereChart(y2, pole y2_hat)."""
    R21 = quat_to_matrix(np.asarray(q_21, dtype=float))
    p2 = R21.T @ (np.asarray(p_hat, dtype=float) - np.asarray(t_21, dtype=float))
    d = float(np.linalg.norm(p2))
    yh = p2 / d
    H = stereo_sphere_chart_diff(yh, yh) @ (np.eye(3) - np.outer(yh, yh)) @ R21.T / d
    return H, stereo_sphere_chart(np.asarray(y2, dtype=float), yh)


def depth_rows(p_hat, rng):
    """A range to landmark p_hat (depth camera, lidar).  Returns (H (1, 3), resid (1,)): H = p_hat^T / |p_hat|, resid = rng - |p_hat|."""
    p = np.asarray(p_hat, dtype=float)
    d = float(np.linalg.norm(p))
    return (p / d)[None, :], np.array([float(rng) - d])


def position_rows(p_hat, p_meas):
    """A surveyed position of landmark p_hat in the camera frame (relocalisation).  Returns (H = I (3, 3), resid = p_meas - p_hat)."""
    return np.eye(3), np.asarray(p_meas, dtype=float) - np.asarray(p_hat, dtype=float)


OBS_BEARING, OBS_RANGE, OBS_POSITION = 0, 1, 2
OBS_ROWS = {OBS_BEARING: 2, OBS_RANGE: 1, OBS_POSITION: 3}


def observe_rows_host(kind, state, ids, meas, cam=None):
    """What FilterBatch.observe_landmarks forms for ONE filter, in numpy: the three row functions above at the estimate of a dump_state
    dictionary `state`, followed by local_jacobian_blocks' landmark blocks
    (landmark_jacobian_blocks: the gravity chart plays no part).  kind: OBS_BEARING / OBS_RANGE / OBS_POSITION; ids (K,) landmark ids; meas (K, 3):
    a bearing y, (rho, -, -) or a position m in the measuring camera's frame; cam: None (the primary camera) or (q_c (w, x, y, z), t_c), the
    measuring camera's pose in the primary camera's frame -- q_c is normalised.  Per entry whose id the state holds: p_hat = J_i p0_i,
    p_c = R_c^T (p_hat - t_c), the kind's (H, resid) at p_c with H taken back to the primary frame by R_c^T, and Ht = H J_i.
    Returns (Ht (K, rows, 3), resid (K, rows), used (K,)): used 1 formed, 0 id not in the state, 3 not observable (|p_c| zero or not
    finite, a singular chart, a chart value that is not finite); rows of entries that are not formed are zeros."""
    rows = OBS_ROWS[kind]
    sid = [int(i) for i in state["ids"]]
    ids = np.asarray(ids, dtype=int).reshape(-1)
    meas = np.asarray(meas, dtype=float).reshape(len(ids), 3)
    J = landmark_jacobian_blocks(state["group"])
    p0 = np.asarray(state["origin"]["p"], dtype=float).reshape(-1, 3)
    q_c, t_c = np.array([1.0, 0.0, 0.0, 0.0]), np.zeros(3)
    if cam is not None:
        q_c, t_c = np.asarray(cam[0], dtype=float), np.asarray(cam[1], dtype=float)
        q_c = q_c / np.sqrt(float(q_c @ q_c))
    Rc = quat_to_matrix(q_c)
    Ht, resid, used = np.zeros((len(ids), rows, 3)), np.zeros((len(ids), rows)), np.zeros(len(ids), dtype=np.uint8)
    for k, lid in enumerate(ids):
        if int(lid) not in sid:
            continue
        i = sid.index(int(lid))
        with np.errstate(all="ignore"):
            p_hat = J[i] @ p0[i]
            p_c = Rc.T @ (p_hat - t_c)
            d = float(np.linalg.norm(p_c))
        used[k] = 3
        if not (d > 0.0 and np.isfinite(d)):
            continue
        if kind == OBS_BEARING:
            try:
                with np.errstate(all="ignore"):
                    H, r = stereo_rows(p_hat, q_c, t_c, meas[k])
            except ValueError:
                continue
            if not np.all(np.isfinite(r)):
                continue
        elif kind == OBS_RANGE:
            H, r = depth_rows(p_c, meas[k, 0])
            H = H @ Rc.T
        else:
            H, r = position_rows(p_c, meas[k])
            H = H @ Rc.T
        Ht[k], resid[k], used[k] = H @ J[i], r, 1
    return Ht, resid, used


# ---- the iterated (re-linearised) observation update (FilterBatch.observe_landmarks(max_lin > 1); eqf_observe_landmarks_iterated)
ITER_CONVERGED, ITER_EXHAUSTED, ITER_STALLED, ITER_SOLVE_FAILED, ITER_MASKED = 0, 1, 2, 3, 4


def landmark_step_state(state, ids, g):
    """A copy of the dump_state dictionary `state` whose landmarks ids[k] (those the state holds) took the plain group step
    Q_i <- Delta_i(g[k], p0_i) Q_i of eqf_apply_increment: q <- exp(-(p0 x g) / |p0|^2) q, a <- exp(-p0 . g / |p0|^2) a.  Everything else is
    shared with `state`.  The trial point of a linearisation."""
    sid = [int(i) for i in state["ids"]]
    p0 = np.asarray(state["origin"]["p"], dtype=float).reshape(-1, 3)
    Qq = np.array(state["group"]["Qq"], dtype=float).reshape(-1, 4)
    Qa = np.array(state["group"]["Qa"], dtype=float).reshape(-1)
    g = np.asarray(g, dtype=float).reshape(-1, 3)
    for k, lid in enumerate(np.asarray(ids, dtype=int).reshape(-1)):
        if int(lid) not in sid:
            continue
        i = sid.index(int(lid))
        n2 = float(p0[i] @ p0[i])
        with np.errstate(all="ignore"):
            Qq[i] = _quat_mul(_quat_from_matrix(_so3_exp_matrix(-np.cross(p0[i], g[k]) / n2)), Qq[i])
            Qa[i] = np.exp(-float(p0[i] @ g[k]) / n2) * Qa[i]
    return dict(state, group=dict(state["group"], Qq=Qq, Qa=Qa))


def _iter_blocks(Sigma, state, ids, on, Ht, R):
    """(idx of the entries `on`, the dense rows over their landmark blocks M only (m, 3 |on|), Sigma_MM, blockdiag(R))"""
    sid = [int(i) for i in state["ids"]]
    rows = Ht.shape[1]
    idx = [sid.index(int(ids[k])) for k in on]
    M = np.array([11 + 3 * i + c for i in idx for c in range(3)], dtype=np.int64)
    Hd = np.zeros((rows * len(on), 3 * len(on)))
    Rd = np.zeros((rows * len(on), rows * len(on)))
    for p, k in enumerate(on):
        Hd[rows * p:rows * (p + 1), 3 * p:3 * (p + 1)] = Ht[k]
        Rd[rows * p:rows * (p + 1), rows * p:rows * (p + 1)] = np.tril(R[k]) + np.tril(R[k], -1).T
    Sg = np.tril(Sigma) + np.tril(Sigma, -1).T
    return idx, Hd, Sg[np.ix_(M, M)], Rd


def observe_iterated_step(kind, Sigma, state, ids, meas, R, g, on, cam=None, consider=None):
    """ONE step of the iteration for one filter: the rows at the trial point g (K, 3) -- increments on each entry's landmark block, from the
    UNCHANGED state --, r~ = resid + Ht g, and g_next = Sigma_MM Ht^T (Ht Sigma_MM Ht^T + R)^-1 r~ over the entries `on`, zero on an entry
    whose landmark id is in `consider`.  Returns (Ht (K, rows, 3), rt (K, rows), g_next (K, 3), stalled).  Raises numpy.linalg.LinAlgError
    when S is not positive definite."""
    ids = np.asarray(ids, dtype=int).reshape(-1)
    g = np.asarray(g, dtype=float).reshape(len(ids), 3)
    R = np.asarray(R, dtype=float)
    with np.errstate(all="ignore"):  # (a trial point that is not finite is a verdict, not a warning)
        Ht, resid, u = observe_rows_host(kind, landmark_step_state(state, ids, g), ids, meas, cam)
    stalled = any(u[k] != 1 for k in on)
    rt = resid + np.einsum("krc,kc->kr", Ht, g)
    g_next = np.zeros_like(g)
    if stalled or not len(on):
        return Ht, rt, g_next, stalled
    _, Hd, Smm, Rd = _iter_blocks(np.asarray(Sigma, dtype=float), state, ids, on, Ht, R)
    T = Smm @ Hd.T
    L = np.linalg.cholesky(Hd @ T + Rd)
    w = np.linalg.solve(L.T, np.linalg.solve(L, rt[on].reshape(-1)))
    g_next[on] = (T @ w).reshape(len(on), 3)
    for k in on:
        if consider is not None and int(ids[k]) in [int(c) for c in consider]:
            g_next[k] = 0.0
    return Ht, rt, g_next, stalled


def observe_iterated_host(kind, Sigma, state, ids, meas, R, cam=None, max_lin=1, tol=0.0, consider=None, gate=np.inf, lm_gate=np.inf):
    """The numpy statement of FilterBatch.observe_landmarks(max_lin=..., tol=...) for ONE filter (include/eqf_vio_amd.h:
    eqf_observe_landmarks_iterated).  Sigma (n, n), state: a dump_state dictionary, ids (K,), meas (K, 3), R (K, rows, rows), cam as
    observe_rows_host's, consider: landmark IDS that keep estimate and covariance.  Linearisation 0 at the state decides and freezes used
    (update_landmarks_host's verdicts with lm_gate; 3 not observable); then g_{k+1}, last_step = max |g_{k+1} - g_k| and the stop rule
    (last_step <= tol with tol > 0: converged) as observe_iterated_step states them, and the commit: update_landmarks_host -- or, with
    consider, schmidt_update_host -- with the committed rows (Ht_K, r~_K) on the prior Sigma.
    Returns dict(Ht, resid (= r~_K), used, g_trace (max_lin, K, 3), n_lin, status, last_step, gamma, Sigma, nis, info)."""
    Sg = np.asarray(Sigma, dtype=float)
    ids = np.asarray(ids, dtype=int).reshape(-1)
    K, rows = len(ids), OBS_ROWS[kind]
    R = np.broadcast_to(np.asarray(R, dtype=float), (K, rows, rows)) if np.ndim(R) >= 2 else np.broadcast_to(float(R) * np.eye(rows), (K, rows, rows))
    sid = [int(i) for i in state["ids"]]
    idx = np.array([sid.index(int(i)) if int(i) in sid else -1 for i in ids])
    Ht, rt, used3 = observe_rows_host(kind, state, ids, meas, cam)
    first = update_landmarks_host(Sg, np.where(used3 == 1, idx, -1), Ht, rt, R, lm_gate=lm_gate)
    used = np.where(used3 == 3, 3, first["used"]).astype(np.uint8)
    on = [int(k) for k in np.flatnonzero(used == 1)]
    g = np.zeros((K, 3))
    trace = np.zeros((int(max_lin), K, 3))
    n_lin, status, last_step = int(max_lin), ITER_EXHAUSTED, 0.0
    for k in range(int(max_lin) - 1):
        try:
            _, Hd, Smm, Rd = _iter_blocks(Sg, state, ids, on, Ht, R)
            T = Smm @ Hd.T
            L = np.linalg.cholesky(Hd @ T + Rd)
            w = np.linalg.solve(L.T, np.linalg.solve(L, rt[on].reshape(-1)))
            gn = np.zeros((K, 3))
            gn[on] = (T @ w).reshape(len(on), 3)
            for e in on:
                if consider is not None and int(ids[e]) in [int(c) for c in consider]:
                    gn[e] = 0.0
            step = float(np.max(np.abs(gn - g))) if K else 0.0
            if not np.isfinite(step):
                raise np.linalg.LinAlgError("not finite")
        except np.linalg.LinAlgError:
            n_lin, status, last_step = k + 1, ITER_SOLVE_FAILED, np.nan
            break
        last_step = step
        if tol > 0.0 and step <= tol:
            n_lin, status = k + 1, ITER_CONVERGED
            break
        with np.errstate(all="ignore"):  # (a trial point that is not finite is a verdict, not a warning)
            Hn, rn, u = observe_rows_host(kind, landmark_step_state(state, ids, gn), ids, meas, cam)
        if any(u[e] != 1 for e in on):
            n_lin, status = k + 1, ITER_STALLED
            break
        for e in on:
            Ht[e], rt[e] = Hn[e], rn[e] + Hn[e] @ gn[e]
        g = gn
        trace[k + 1] = g
    cidx = consider_indices([sid.index(int(c)) for c in (consider if consider is not None else []) if int(c) in sid])
    fin = update_landmarks_host(Sg, np.where(used == 1, idx, -1), Ht, rt, R, gate=gate)
    gamma, Sp = fin["gamma"], fin["Sigma"]
    if fin["info"] == 0 and len(cidx) and len(on):
        N = (len(Sg) - 11) // 3
        Rd = np.zeros((rows * len(on), rows * len(on)))
        for p, e in enumerate(on):
            Rd[rows * p:rows * (p + 1), rows * p:rows * (p + 1)] = np.tril(R[e]) + np.tril(R[e], -1).T
        s = schmidt_update_host(np.tril(Sg) + np.tril(Sg, -1).T, landmark_blocks_matrix(N, idx[on], Ht[on]), Rd, rt[on].reshape(-1), cidx)
        gamma, Sp = s["gamma"], s["Sigma"]
    return dict(Ht=Ht, resid=rt, used=used, g_trace=trace, n_lin=n_lin, status=status, last_step=last_step, gamma=gamma, Sigma=Sp,
                nis=fin["nis"], info=fin["info"])


def map_cost(kind, Sigma, state, ids, meas, R, gamma, used, cam=None, gradient=False):
    """The iteration's own objective at an increment gamma (n,) of the prior estimate, over the entries with used == 1:
        1/2 gamma^T Sigma^-1 gamma + 1/2 r(gamma)^T R^-1 r(gamma),
    r(gamma) the kind's residual at the state whose landmarks took the plain step with their blocks of gamma (landmark_step_state).
    gradient=True returns (cost, Sigma^-1 gamma - Ht(gamma)^T R^-1 r(gamma)) -- a moved estimate lowers the residual by Ht times the
    move -- whose norm an iterated update drives towards zero."""
    Sg = np.asarray(Sigma, dtype=float)
    Sg = np.tril(Sg) + np.tril(Sg, -1).T
    ids = np.asarray(ids, dtype=int).reshape(-1)
    K, rows = len(ids), OBS_ROWS[kind]
    R = np.broadcast_to(np.asarray(R, dtype=float), (K, rows, rows)) if np.ndim(R) >= 2 else np.broadcast_to(float(R) * np.eye(rows), (K, rows, rows))
    sid = [int(i) for i in state["ids"]]
    gamma = np.asarray(gamma, dtype=float).reshape(-1)
    g = np.zeros((K, 3))
    for k in range(K):
        if int(ids[k]) in sid:
            i = sid.index(int(ids[k]))
            g[k] = gamma[11 + 3 * i:14 + 3 * i]
    Ht, r, _ = observe_rows_host(kind, landmark_step_state(state, ids, g), ids, meas, cam)
    a = np.linalg.solve(Sg, gamma)
    cost, grad = 0.5 * float(gamma @ a), a.copy()
    for k in np.flatnonzero(np.asarray(used) == 1):
        Rl = np.tril(R[k]) + np.tril(R[k], -1).T
        v = np.linalg.solve(Rl, r[k])
        cost += 0.5 * float(r[k] @ v)
        i = sid.index(int(ids[k]))
        grad[11 + 3 * i:14 + 3 * i] -= Ht[k].T @ v
    return (cost, grad) if gradient else cost


# ---- explicit landmark edits (FilterBatch.edit_landmarks): the host statement of the edit and the usual priors
def edit_landmarks_host(state_dump, remove_ids, insert_ids, p, P):
    """What FilterBatch.edit_landmarks does to ONE filter, on a dump_state dictionary, in numpy: a new dictionary with ids, origin p, group
    Qq / Qa and sigma (reference index map, 11 + 3N) edited and everything else as it was; restore_state of it is the host route the device
    call replaces.  The named ids the state holds leave (rows and columns of sigma with them, the order of the rest kept); then the
    insertions are appended in the order given: p0 = p, Q the identity, zero rows and columns but for the landmark's own block, which is
    P's lower triangle mirrored.  Entries the call would not apply (an id still in the state, values rejected) are skipped by the same
    rules.  Returns (new dump, removed, inserted)."""
    ids = [int(x) for x in np.asarray(state_dump["ids"]).reshape(-1)]
    rem = [int(x) for x in np.asarray(remove_ids).reshape(-1)]
    iid = [int(x) for x in np.asarray(insert_ids).reshape(-1)]
    p = np.asarray(p, dtype=float).reshape(-1, 3)
    P = np.asarray(P, dtype=float).reshape(-1, 3, 3)
    removed = np.array([int(r in ids) for r in rem], dtype=np.uint8)
    keep = [i for i, x in enumerate(ids) if x not in set(rem)]
    left = {ids[i] for i in keep}
    inserted = np.zeros(len(iid), dtype=np.uint8)
    for k, i in enumerate(iid):
        if i in left:
            continue
        low = P[k][np.tril_indices(3)]
        ok = bool(np.all(np.isfinite(p[k])) and np.all(np.isfinite(low)) and np.any(p[k] != 0.0))
        if ok:
            S = mirror_lower(P[k])
            d0 = S[0, 0]
            ok = bool(d0 > 0)
            if ok:
                l10, l20 = S[1, 0] / np.sqrt(d0), S[2, 0] / np.sqrt(d0)
                d1 = S[1, 1] - l10 * l10
                ok = bool(d1 > 0) and bool(S[2, 2] - l20 * l20 - ((S[2, 1] - l20 * l10) / np.sqrt(d1)) ** 2 > 0)
        inserted[k] = 1 if ok else 2
    acc = [k for k in range(len(iid)) if inserted[k] == 1]
    nK, nA = len(keep), len(acc)
    rows = list(range(11)) + [11 + 3 * i + c for i in keep for c in range(3)]
    Sold = np.asarray(state_dump["sigma"], dtype=float)
    S = np.zeros((11 + 3 * (nK + nA), 11 + 3 * (nK + nA)))
    S[:11 + 3 * nK, :11 + 3 * nK] = Sold[np.ix_(rows, rows)]
    for j, k in enumerate(acc):
        a = 11 + 3 * (nK + j)
        S[a:a + 3, a:a + 3] = mirror_lower(P[k])
    out = dict(state_dump)
    o, g = dict(state_dump["origin"]), dict(state_dump["group"])
    o["p"] = np.concatenate([np.asarray(o["p"], dtype=float).reshape(-1, 3)[keep], p[acc]]).reshape(-1, 3)
    g["Qq"] = np.concatenate([np.asarray(g["Qq"], dtype=float).reshape(-1, 4)[keep], np.tile([1.0, 0.0, 0.0, 0.0], (nA, 1))]).reshape(-1, 4)
    g["Qa"] = np.concatenate([np.asarray(g["Qa"], dtype=float).reshape(-1)[keep], np.ones(nA)])
    out.update(ids=np.array([ids[i] for i in keep] + [iid[k] for k in acc], dtype=np.int32), origin=o, group=g, sigma=S)
    return out, removed, inserted


def depth_prior(y, rng, var_rng, var_y):
    """A landmark seen along the unit bearing y at range rng (depth camera, lidar): p = rng y, P = var_rng y y^T + rng^2 var_y (I - y y^T)
    -- variance var_rng along the ray, rng^2 var_y across it (var_y: the bearing's variance on the sphere, per axis).  Returns (p (3,),
    P (3, 3)), P symmetric bit for bit."""
    y = np.asarray(y, dtype=float).reshape(3)
    rng, var_rng, var_y = float(rng), float(var_rng), float(var_y)
    yy = np.outer(y, y)
    return rng * y, var_rng * yy + (rng * rng * var_y) * (np.eye(3) - yy)


def triangulation_prior(y1, y2, q_21, t_21, var_y):
    """A landmark seen by both cameras of a rigid stereo rig along the unit bearings y1 (camera 1) and y2 (camera 2), (q_21, t_21) the pose
    of camera 2 in camera 1's frame as in stereo_rows.  Everything in camera 1's frame: the rays start at c_1 = 0 and c_2 = t_21 with the
    directions y_1 and R_21 y2; p is their least-squares intersection, the solution of the 3 x 3 normal equations of
    sum_k |(I - y_k y_k^T)(p - c_k)|^2, and P = (sum_k (I - y_k y_k^T) / (d_k^2 var_y))^-1 with d_k = |p - c_k|.
    P is a FIRST-ORDER covariance (the bearings' noise pushed through the linearised intersection): along the ray it grows like
    d^4 / baseline^2 var_y, so for a distant point it says little more than "somewhere along this ray", and the point's true distribution is
    far from Gaussian there.  Raises ValueError for parallel rays (a normal matrix that is not positive definite).  Returns (p, P)."""
    y1 = np.asarray(y1, dtype=float).reshape(3)
    R21 = quat_to_matrix(np.asarray(q_21, dtype=float))
    c = [np.zeros(3), np.asarray(t_21, dtype=float).reshape(3)]
    ys = [y1, R21 @ np.asarray(y2, dtype=float).reshape(3)]
    M = [np.eye(3) - np.outer(y, y) for y in ys]
    A = M[0] + M[1]
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        raise ValueError("triangulation_prior: the rays are parallel") from None
    if not np.all(np.isfinite(L)) or np.min(np.diag(L)) ** 2 <= 4.0 * np.finfo(float).eps:
        raise ValueError("triangulation_prior: the rays are parallel")
    p = np.linalg.solve(A, M[0] @ c[0] + M[1] @ c[1])
    W = sum(Mk / (float(np.dot(p - ck, p - ck)) * float(var_y)) for Mk, ck in zip(M, c))
    P = np.linalg.inv(W)
    return p, 0.5 * (P + P.T)


def landmark_blocks_matrix(N, idx, Ht):
    """The block-sparse measurement matrix as a dense one: (rows * K, 11 + 3N) with block k (rows, 3) at landmark idx[k]'s columns."""
    Ht = np.asarray(Ht, dtype=float)
    K, rows = Ht.shape[0], Ht.shape[1]
    out = np.zeros((rows * K, 11 + 3 * int(N)))
    for k in range(K):
        out[rows * k:rows * (k + 1), 11 + 3 * int(idx[k]):14 + 3 * int(idx[k])] = Ht[k]
    return out


def update_landmarks_host(Sigma, idx, H, resid, R, J=None, gate=np.inf, lm_gate=np.inf):
    """The dense numpy statement of FilterBatch.update_landmarks' arithmetic for one filter (include/eqf_vio_amd.h: eqf_update_landmarks).
    Sigma (n, n) in eqf_get_sigma's coordinates, read by its LOWER triangle; idx (K,): the landmark INDEX of every entry, < 0 for an id that
    is not in the state; H (K, rows, 3), resid (K, rows), R (K, rows, rows: lower triangles read); J: local_jacobian_blocks(...)["lm"] for
    rows written in the estimate's chart (H_k J_i is formed here), None for rows in the origin chart.  An entry whose id is absent or whose
    own d2_k = resid_k^T (Ht_k Sigma_ii Ht_k^T + R_k)^-1 resid_k exceeds lm_gate (NaN stays in) is a decoupled block (H = 0, resid = 0,
    R = I) that is not counted in dof.  Then
        B = Sigma Ht^T, S = Ht B + blockdiag(R_k) = L L^T, Y = L^-1 B^T, z = L^-1 resid, gamma = Y^T z, Sigma+ = Sigma - Y^T Y.
    Returns dict(Sigma, gamma, nis, logdet_S, loglik, dof, used (K,): 1 applied, 0 absent, 2 gated, d2 (K,), info: 0 applied, 1 S not positive
    definite, 2 nis > gate; Sigma and gamma are the input's and 0 when info != 0)."""
    Sg = np.asarray(Sigma, dtype=float)
    Sg = np.tril(Sg) + np.tril(Sg, -1).T
    n = len(Sg)
    N = (n - 11) // 3
    H = np.asarray(H, dtype=float)
    K, rows = H.shape[0], H.shape[1]
    resid = np.asarray(resid, dtype=float).reshape(K, rows)
    R = np.asarray(R, dtype=float).reshape(K, rows, rows)
    Rl = np.tril(R) + np.transpose(np.tril(R, -1), (0, 2, 1))
    used = np.zeros(K, dtype=np.int32)
    d2 = np.full(K, np.nan)
    Ht = np.zeros((K, rows, 3))
    for k in range(K):
        i = int(idx[k])
        if not 0 <= i < N:
            continue
        Ht[k] = H[k] @ np.asarray(J, dtype=float).reshape(-1, 3, 3)[i] if J is not None else H[k]
        Skk = Ht[k] @ Sg[11 + 3 * i:14 + 3 * i, 11 + 3 * i:14 + 3 * i] @ Ht[k].T + Rl[k]
        try:
            zk = np.linalg.solve(np.linalg.cholesky(Skk), resid[k])
            d2[k] = float(zk @ zk)
        except np.linalg.LinAlgError:
            pass
        used[k] = 2 if d2[k] > lm_gate else 1
    on = np.flatnonzero(used == 1)
    m = rows * len(on)
    out = dict(Sigma=Sg.copy(), gamma=np.zeros(n), nis=0.0, logdet_S=0.0, loglik=0.0, dof=m, used=used, d2=d2, info=0)
    if m == 0:
        return out
    Hd = landmark_blocks_matrix(N, [idx[k] for k in on], Ht[on])
    Rd = np.zeros((m, m))
    for p, k in enumerate(on):
        Rd[rows * p:rows * (p + 1), rows * p:rows * (p + 1)] = Rl[k]
    try:
        r = linear_update_host(Sg, Hd, resid[on].reshape(-1), Rd)
    except np.linalg.LinAlgError:
        r = None
    if r is None or not (np.isfinite(r["nis"]) and np.isfinite(r["gamma"]).all() and np.isfinite(r["Sigma"]).all()):
        out.update(nis=np.nan, logdet_S=np.nan, loglik=np.nan, info=1)
        return out
    out.update(nis=r["nis"], logdet_S=r["logdet_S"], loglik=r["loglik"])
    if r["nis"] > gate:
        out["info"] = 2
        return out
    Sp = np.tril(r["Sigma"])
    out.update(Sigma=Sp + np.tril(Sp, -1).T, gamma=r["gamma"])
    return out


def systematic_resample(loglik, u):
    """Systematic resampling of a batch of B filters by weight: parents (B,) int32 for FilterBatch.resample, filter b continues from
    parents[b].  Weights are exp(loglik - max) normalised; a log-likelihood of -inf or NaN (an update that did not run, a filter that
    diverged) gets weight 0.  The B points (u + b) / B, u in [0, 1), are looked up in the cumulative weights: deterministic for a given u,
    parents ascending, and filter i is drawn floor(B w_i) or ceil(B w_i) times.  Raises ValueError if no weight is positive or u is out
    of range."""
    ll = np.asarray(loglik, dtype=float).reshape(-1)
    B = len(ll)
    if not 0.0 <= float(u) < 1.0:
        raise ValueError("u must lie in [0, 1)")
    ok = ~np.isnan(ll) & (ll > -np.inf)
    if B == 0 or not ok.any():
        raise ValueError("no filter with a finite log-likelihood")
    if np.isposinf(ll[ok]).any():
        raise ValueError("a log-likelihood of +inf")
    w = np.zeros(B)
    w[ok] = np.exp(ll[ok] - ll[ok].max())
    c = np.cumsum(w)
    pts = (float(u) + np.arange(B)) / B * c[-1]
    # (side="right": a point on a boundary belongs to the next filter, so a filter of weight 0 is never drawn -- also not at u = 0)
    parents = np.searchsorted(c, pts, side="right")
    last = int(np.flatnonzero(w > 0)[-1])
    return np.minimum(parents, last).astype(np.int32)


# ---- moment matching over a weighted batch (include/eqf_vio_amd.h: eqf_get_mixture_moments / eqf_merge_filters)
def mixture_weights(loglik):
    """Normalised weights of a batch from its log-likelihoods: systematic_resample's exp(loglik - max), divided by their sum; a
    log-likelihood of -inf or NaN gets weight 0.  Raises ValueError if no weight is positive or one is +inf."""
    ll = np.asarray(loglik, dtype=float).reshape(-1)
    ok = ~np.isnan(ll) & (ll > -np.inf)
    if len(ll) == 0 or not ok.any():
        raise ValueError("no filter with a finite log-likelihood")
    if np.isposinf(ll[ok]).any():
        raise ValueError("a log-likelihood of +inf")
    w = np.zeros(len(ll))
    w[ok] = np.exp(ll[ok] - ll[ok].max())
    return w / w.sum()


def normalise_weights(w):
    """w~_k = w_k / s, s the serial sum in the order given (what the library does on the host, in double)."""
    w = np.asarray(w, dtype=float).reshape(-1)
    if len(w) == 0 or not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError("weights must be finite and not negative")
    s = 0.0
    for x in w:
        s += float(x)
    if not s > 0.0:
        raise ValueError("the weight sum must be positive")
    return w / s


def chart_transition(eta_b, eta_c):
    """T_b (2, 2): the differential at 0 of chi_c o chi_b^-1 on the gravity sphere, stereoSphereChartDiff(eta_b, pole eta_c)
    stereoSphereChartInvDiff(0, pole eta_b)."""
    return stereo_sphere_chart_diff(eta_b, eta_c) @ stereo_sphere_chart_inv_diff_at_zero(eta_b)


def lower_mirrored(S):
    """The Sigma the mixture kernels see.  They read the blocks on and below the block diagonal of every member's covariance -- the 11 x 11
    base block and the diagonal 3 x 3 landmark blocks whole, as stored, the blocks below them -- never a block above it; what they compute
    is the lower triangle of P, mirrored.  So a Sigma that its own updates have left symmetric only to rounding counts with those blocks:
    the blocks above the block diagonal are returned as the transposes of the ones below."""
    S = np.array(S, dtype=float)
    edges = [0, 11] + list(range(14, S.shape[0] + 1, 3))
    for a, b in zip(edges[:-1], edges[1:]):
        S[a:b, b:] = S[b:, a:b].T
    return S


def mirror_lower(P):
    """P's lower triangle with its mirror above it: how the mixture kernels write P (bit-for-bit symmetric)."""
    P = np.asarray(P)
    return np.tril(P) + np.tril(P, -1).T


def _member_error(member, centre_est, centre_bias):
    e = local_error(centre_est, member["estimate"], bias=centre_bias, true_bias=member["bias"])
    return error_vector(e)


def mixture_member_images(members, centre):
    """The pieces of mixture_moments_host per member, in the chart of the centre (an index into members: T = I for that member by
    definition; or a dict with `estimate` and `bias`: every T is computed): (E, terms) with E[k] = e_k and terms[k] = J'_k Sigma_k J'_k^T."""
    own = centre if isinstance(centre, (int, np.integer)) else None
    c = members[own] if own is not None else centre
    eta_c = gravity_dir(c["estimate"]["q"])
    E, terms = [], []
    for k, mb in enumerate(members):
        same = own is not None and (mb is members[own])
        e = _member_error(mb, c["estimate"], c["bias"])
        blocks = dict(local_jacobian_blocks(mb["origin"], mb["group"]))
        if same:
            e[6:8] = 0.0
        else:
            blocks["G"] = chart_transition(gravity_dir(mb["estimate"]["q"]), eta_c) @ blocks["G"]
        J = jacobian_matrix(blocks)
        E.append(e)
        terms.append(J @ lower_mirrored(mb["sigma"]) @ J.T)
    return E, terms


def mixture_moments_host(members, w, centre, centred=True):
    """The numpy statement of FilterBatch.mixture_moments.  members: a list of dicts with `estimate` (state_estimate(): q, v, p), `bias`,
    `origin`, `group` and `sigma` (the filter's Sigma, origin chart; its blocks on and below the block diagonal count: lower_mirrored); w their weights (normalised here); centre: the index of the member
    whose estimate is the centre c (its T is the identity by definition), or a dict with `estimate` and `bias` (every T is computed).
    e_b = chi_c(xHat_b), J'_b = J_b with T_b G_b for G_b, eBar = sum w~ e, P = sum w~ [J' Sigma J'^T + (e - m)(e - m)^T], m = eBar if
    centred else 0.  Returns dict(mean, P, e (n, dim), spread, n_eff, spread_trace, total_trace)."""
    wt = normalise_weights(w)
    if len(wt) != len(members):
        raise ValueError("one weight per member")
    E, terms = mixture_member_images(members, centre)
    E = np.array(E)
    mean = np.zeros(E.shape[1])
    for k in range(len(wt)):
        mean = mean + wt[k] * E[k]
    m = mean if centred else np.zeros_like(mean)
    P = np.zeros_like(terms[0])
    spread = np.zeros_like(terms[0])
    for k in range(len(wt)):
        d = E[k] - m
        P = P + wt[k] * terms[k]
        spread = spread + wt[k] * np.outer(d, d)
    P = mirror_lower(P + spread)
    return dict(mean=mean, P=P, e=E, spread=spread, n_eff=1.0 / float(np.sum(wt * wt)), spread_trace=float(np.trace(spread)),
                total_trace=float(np.trace(P)))


def merge_host(members, w, ref):
    """The numpy statement of FilterBatch.merge: eBar about member `ref`'s estimate; xBar = local_retract(xHat_ref, eBar) with bias_ref +
    eBar[0:6] and pose position sum w~_k x_k; P about xBar with centred = 0.  Returns dict(estimate (q, x, v, p), bias, P, mean, n_eff,
    spread_trace, total_trace): what filter dst's state_estimate(), bias() and sigma_local() show afterwards."""
    wt = normalise_weights(w)
    first = mixture_moments_host(members, wt, int(ref), centred=True)
    r = members[int(ref)]
    xbar = local_retract(r["estimate"], first["mean"], bias=r["bias"])
    x = np.zeros(3)
    for k, mb in enumerate(members):
        x = x + wt[k] * np.asarray(mb["estimate"]["x"], dtype=float)
    xbar["x"] = x
    bias = xbar.pop("bias")
    second = mixture_moments_host(members, wt, dict(estimate=xbar, bias=bias), centred=False)
    return dict(estimate=xbar, bias=bias, P=second["P"], mean=first["mean"], n_eff=second["n_eff"], spread_trace=second["spread_trace"],
                total_trace=second["total_trace"])


# ---- which members to merge (FilterBatch.merge_costs / reduce_mixture; include/eqf_vio_amd.h: eqf_get_merge_costs) on the host
COST_KINDS = ("runnalls", "bhattacharyya")


def _logdet_maha(A, d):
    """log det A and d^T A^-1 d of a symmetric A (numpy.linalg.slogdet / solve); (nan, nan) if A is not positive definite to slogdet."""
    if A.shape[0] == 0:
        return 0.0, 0.0
    sign, ld = np.linalg.slogdet(A)
    if not sign > 0:
        return np.nan, np.nan
    return float(ld), float(d @ np.linalg.solve(A, d))


def pair_cost(kind, ld_i, ld_j, ld_ij, maha, wi, wj):
    """The two costs from the three log-determinants, the quadratic form and the normalised weights (include/eqf_vio_amd.h)."""
    if kind == "bhattacharyya":
        return 0.125 * maha + 0.25 * ((ld_ij - ld_i) + (ld_ij - ld_j))
    if kind != "runnalls":
        raise ValueError(f"kind must be one of {COST_KINDS}")
    a = pair_alpha(kind, wi, wj)
    return 0.5 * (wi * (ld_ij - ld_i) + wj * (ld_ij - ld_j) + (wi + wj) * np.log1p(a * (1.0 - a) * maha))


def pair_alpha(kind, wi, wj):
    return 0.5 if (kind == "bhattacharyya" or not wi + wj > 0.0) else wj / (wi + wj)


def merge_costs_host(members, w, ref, kind="runnalls", first=0, pairs=None):
    """The numpy statement of FilterBatch.merge_costs.  members, w: as mixture_moments_host; ref: the POSITION in members of the member whose
    estimate is the chart centre; first: 0, 6 or 11; pairs: (npairs, 2) positions or None (all i < j).  Per pair, ordered so that i < j:
    SigmaBar = S'_i + alpha (S'_j - S'_i) over the lower triangles, d = e_j - e_i, slogdet and solve.  Returns the dict of
    FilterBatch.merge_costs (without the info words: a matrix that is not positive definite gives NaN)."""
    wt = normalise_weights(w)
    n = len(members)
    if len(wt) != n:
        raise ValueError("one weight per member")
    E, terms = mixture_member_images(members, int(ref))
    S = [mirror_lower(t)[first:, first:] for t in terms]
    e = [np.asarray(x)[first:] for x in E]
    mld = np.array([_logdet_maha(S[k], np.zeros(S[k].shape[0]))[0] for k in range(n)])
    if pairs is None:
        pp = np.array([(i, j) for i in range(n) for j in range(i + 1, n)], dtype=np.int32).reshape(-1, 2)
    else:
        pp = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    cost, ldp, maha = np.zeros(len(pp)), np.zeros(len(pp)), np.zeros(len(pp))
    for k, (i, j) in enumerate(pp):
        i, j = (int(i), int(j)) if i <= j else (int(j), int(i))
        a = pair_alpha(kind, wt[i], wt[j])
        ldp[k], maha[k] = _logdet_maha(S[i] + a * (S[j] - S[i]), e[j] - e[i])
        cost[k] = pair_cost(kind, mld[i], mld[j], ldp[k], maha[k], wt[i], wt[j])
    out = dict(pairs=pp, cost=cost, logdet_pair=ldp, maha=maha, member_logdet=mld, ref=int(ref))
    if pairs is None:
        M = np.zeros((n, n))
        for k, (i, j) in enumerate(pp):
            M[i, j] = M[j, i] = cost[k]
        out["matrix"] = M
    return out


def merged_member(members, w, ref):
    """What FilterBatch.merge leaves in filter dst, as a member dict: merge_host's state with origin = the merged estimate, X = identity,
    Sigma = P."""
    m = merge_host(members, w, ref)
    est = m["estimate"]
    N = len(np.asarray(est["p"]).reshape(-1, 3))
    group = dict(Aq=np.array([1.0, 0, 0, 0]), Ax=np.zeros(3), w=np.zeros(3), Qq=np.tile([1.0, 0, 0, 0], (N, 1)), Qa=np.ones(N))
    return dict(estimate=est, bias=m["bias"], origin=dict(q=est["q"], x=est["x"], v=est["v"], p=est["p"]), group=group, sigma=m["P"])


def reduce_mixture_host(members, w, target, max_cost=np.inf, kind="runnalls"):
    """The numpy statement of FilterBatch.reduce_mixture: greedy merging of the cheapest pair (ties: the lower pair in lexicographic order of
    positions) into the lower position -- into the centre's if the higher position is the centre, the heaviest member at the start -- until
    `target` members are left or the cheapest cost exceeds max_cost.  Returns (surviving positions, their weights, the surviving member
    dicts, log) with log a list of ((position kept, position dropped), cost)."""
    wt = normalise_weights(w)
    ms = {k: m for k, m in enumerate(members)}
    wk = {k: float(wt[k]) for k in ms}
    alive = sorted(ms)
    centre = int(np.argmax(wt))
    log = []

    def ask(pairs_pos):
        loc = {p: k for k, p in enumerate(alive)}
        r = merge_costs_host([ms[p] for p in alive], [wk[p] for p in alive], loc[centre], kind, 0, [(loc[a], loc[b]) for a, b in pairs_pos])
        return {pr: (float(c) if np.isfinite(c) else np.inf) for pr, c in zip(pairs_pos, r["cost"])}

    cache = ask([(a, b) for x, a in enumerate(alive) for b in alive[x + 1:]]) if len(alive) > 1 else {}
    while len(alive) > max(int(target), 1):
        (a, b), c = min(cache.items(), key=lambda kv: (kv[1], kv[0]))
        if not c <= max_cost:
            break
        keep, drop = (b, a) if b == centre else (a, b)
        ms[keep] = merged_member([ms[a], ms[b]], [wk[a], wk[b]], 0 if keep == a else 1)
        wk[keep] = wk[a] + wk[b]
        del ms[drop], wk[drop]
        alive.remove(drop)
        log.append(((keep, drop), c))
        cache = {pr: v for pr, v in cache.items() if a not in pr and b not in pr}
        fresh = [tuple(sorted((keep, o))) for o in alive if o != keep]
        if fresh:
            cache.update(ask(fresh))
    return alive, np.array([wk[k] for k in alive]), [ms[k] for k in alive], log


# ---- the forecast (FilterBatch.forecast; include/eqf_vio_amd.h: eqf_forecast) on the host
class ImuSample:
    """One IMU sample with the arithmetic the reference's IMUVelocity has (IMUVelocity.cpp:35-58): minus a bias 6-vector, times a scalar,
    plus another sample."""

    def __init__(self, stamp=0.0, omega=None, accel=None):
        self.stamp = float(stamp)
        self.omega = np.zeros(3) if omega is None else np.array(omega, dtype=float)
        self.accel = np.zeros(3) if accel is None else np.array(accel, dtype=float)

    def __add__(self, other):
        if hasattr(other, "omega"):
            return ImuSample(self.stamp if self.stamp > 0 else other.stamp, self.omega + other.omega, self.accel + other.accel)
        return ImuSample(self.stamp, self.omega + other[0:3], self.accel + other[3:6])

    def __sub__(self, vec):
        return self + (-np.asarray(vec))

    def __mul__(self, c):
        return ImuSample(self.stamp, self.omega * c, self.accel * c)

    def __getitem__(self, k):  # (omega, accel) as the 6-vector a sample of another type adds to itself
        return np.concatenate([self.omega, self.accel])[k]


def output_blocks(origin_p):
    """C_i = |p0_i|^-1 stereoSphereChartDiff(y0_i, y0_i) (I - y0_i y0_i^T), y0_i = p0_i / |p0_i| (EqFMatrices.cpp:319-344): (N, 2, 3) from
    the ORIGIN's landmarks, FilterBatch.origin()["p"]."""
    p0 = np.asarray(origin_p, dtype=float).reshape(-1, 3)
    C = np.zeros((len(p0), 2, 3))
    for i, q in enumerate(p0):
        nrm = np.linalg.norm(q)
        y = q / nrm
        C[i] = 1.0 / nrm * stereo_sphere_chart_diff(y, y) @ (np.eye(3) - np.outer(y, y))
    return C


def bearing_cov_host(p, P_loc):
    """D P_loc D^T with D = (I - yhat yhat^T) / |p|, yhat = p / |p|: the covariance of the predicted unit bearing of a landmark at p (camera
    frame) whose position has covariance P_loc in the estimate's chart.  Rank 2 (yhat is its null vector); no measurement noise.  p (3,) and
    P_loc (3, 3), or (N, 3) and (N, 3, 3)."""
    p = np.asarray(p, dtype=float)
    P = np.asarray(P_loc, dtype=float)
    if p.ndim == 2:
        return np.array([bearing_cov_host(p[i], P[i]) for i in range(len(p))]).reshape(len(p), 3, 3)
    n = np.linalg.norm(p)
    y = p / n
    D = (np.eye(3) - np.outer(y, y)) / n
    return D @ P @ D.T


def search_ellipse(ycov, dpix_dy, p=0.99):
    """The region of the image in which a tracker should look for a feature: dpix_dy (2 x 3) is the caller's camera Jacobian d pixel / d
    bearing at the predicted bearing, ycov (3 x 3) forecast's covariance of that bearing.  Returns dict(cov (2, 2) = J ycov J^T, axes (2,)
    the semi-axes in pixels, long one first, of the ellipse that holds the feature with chi-square probability p, and dirs (2, 2) their unit
    directions as rows).  Add the detector's own pixel variance to cov before use if it matters."""
    J = np.asarray(dpix_dy, dtype=float).reshape(2, 3)
    cov = J @ np.asarray(ycov, dtype=float).reshape(3, 3) @ J.T
    cov = 0.5 * (cov + cov.T)
    lam, vec = np.linalg.eigh(cov)
    k2 = chi2_gate_threshold(p, 2)
    order = [1, 0]
    return dict(cov=cov, axes=np.sqrt(k2 * np.maximum(lam[order], 0.0)), dirs=vec[:, order].T.copy())


def gate_distance(S, delta):
    """delta^T S^-1 delta through the Cholesky factor of S's LOWER triangle, as the device's gate forms it: what a residual delta (2,) in
    the update's coordinates would score against forecast's S (2, 2).  S (N, 2, 2) with delta (N, 2) gives (N,)."""
    S = np.asarray(S, dtype=float)
    d = np.asarray(delta, dtype=float)
    if S.ndim == 3:
        return np.array([gate_distance(S[i], d[i]) for i in range(len(S))])
    l00 = np.sqrt(S[0, 0])
    l10 = S[1, 0] / l00
    l11 = np.sqrt(S[1, 1] - l10 * l10)
    w0 = d[0] / l00
    w1 = (d[1] - l10 * w0) / l11
    return float(w0 * w0 + w1 * w1)


def score_vision_host(Sigma, C, delta, r, slots):
    """The numpy statement of FilterBatch.score_vision for ONE candidate of one filter (include/eqf_vio_amd.h: eqf_score_vision).  Sigma
    (11 + 3 N square, the reference's index map, FilterBatch.sigma(); its lower triangle is read), C (N, 2, 3) = output_blocks(origin p),
    delta (N, 2) the residual the update would form per landmark of the state (rows of landmarks that do not take part are not read), r the
    measurement variance, slots the state slots of the matching landmarks IN THE STATE'S ORDER.  S = C_M Sigma_MM C_M^T + r I = L L^T by a
    dense Cholesky, z = L^-1 delta_M.  Returns dict(nis, logdet_S, loglik, dof, nis_lm (len(slots),), S); an empty list scores exactly 0."""
    Sg = np.asarray(Sigma, dtype=float)
    Cb = np.asarray(C, dtype=float).reshape(-1, 2, 3)
    d = np.asarray(delta, dtype=float).reshape(-1, 2)
    sl = [int(k) for k in slots]
    if any(b <= a for a, b in zip(sl, sl[1:])):
        raise ValueError("score_vision_host: slots must be strictly ascending (the state's own order)")
    m = 2 * len(sl)
    if m == 0:
        return dict(nis=0.0, logdet_S=0.0, loglik=0.0, dof=0, nis_lm=np.zeros(0), S=np.zeros((0, 0)))
    S = np.zeros((m, m))
    for a, sa in enumerate(sl):
        for b, sb in enumerate(sl[:a + 1]):
            blk = Cb[sa] @ Sg[11 + 3 * sa:14 + 3 * sa, 11 + 3 * sb:14 + 3 * sb] @ Cb[sb].T
            S[2 * a:2 * a + 2, 2 * b:2 * b + 2] = blk
            S[2 * b:2 * b + 2, 2 * a:2 * a + 2] = blk.T
    S = np.tril(S) + np.tril(S, -1).T + float(r) * np.eye(m)
    dm = np.concatenate([d[k] for k in sl])
    L = np.linalg.cholesky(S)
    z = np.linalg.solve(L, dm)
    nis = float(z @ z)
    logdet = 2.0 * float(np.sum(np.log(np.diag(L))))
    nis_lm = np.array([gate_distance(S[2 * a:2 * a + 2, 2 * a:2 * a + 2], dm[2 * a:2 * a + 2]) for a in range(len(sl))])
    return dict(nis=nis, logdet_S=logdet, loglik=-0.5 * (nis + logdet + m * np.log(2.0 * np.pi)), dof=m, nis_lm=nis_lm, S=S)


def joint_compatible(score, p):
    """The joint-compatibility test on a result of FilterBatch.score_vision (or one record of it): nis <= the chi-square threshold of
    probability p at the record's own dof; a record without a matching entry (dof = 0) is compatible.  Arrays give arrays.  A record whose
    info is not 0 has nis = NaN and is not compatible."""
    nis, dof = np.asarray(score["nis"], dtype=float), np.asarray(score["dof"])
    thr = np.array([chi2_gate_threshold(p, dof=int(k)) if k > 0 else np.inf for k in dof.reshape(-1)]).reshape(dof.shape)
    out = np.where(dof > 0, nis <= thr, True)
    return bool(out) if out.ndim == 0 else out


def forecast_host(flt, imu=None, t1=None, local=True, measurement_variance=0.0, sample=ImuSample):
    """The numpy statement of FilterBatch.forecast for ONE filter.  `flt` is a filter object with the reference's interface (processIMUData
    (sample), integrateUpToTime(t), getTime(), initialisedFlag, xi0, X, Sigma, stateEstimate()); it is deep-copied, the copy is given the
    samples imu (K, 7) -- stamp, omega, accel; the filter subtracts its bias -- and, where t1 is given, integrateUpToTime(t1), and the
    handle's outputs are read off the copy: time, steps, pose_q, pose_x, velocity, p, bearing, base, lm (in the estimate's chart if local),
    S = C_i Sigma_ii C_i^T + r I from the origin-chart block and ycov from the estimate-chart block.  `sample(stamp, omega, accel)` builds the
    filter's own sample type."""
    import copy

    f = copy.deepcopy(flt)
    steps = 0
    for r in ([] if imu is None else np.asarray(imu, dtype=float).reshape(-1, 7)):
        steps += int(f.getTime() >= 0 and r[0] - f.getTime() > 0)
        f.processIMUData(sample(r[0], r[1:4], r[4:7]))
    if t1 is not None:
        steps += int(bool(f.integrateUpToTime(float(t1))))
    est = f.stateEstimate()
    N = len(f.xi0.ids)
    origin = dict(q=f.xi0.pose.q, x=f.xi0.pose.x, v=f.xi0.velocity, p=np.asarray(f.xi0.p, dtype=float).reshape(N, 3))
    group = dict(Aq=f.X.A.q, Ax=f.X.A.x, w=f.X.w, Qq=np.array([Q.q for Q in f.X.Q]).reshape(N, 4), Qa=np.array([Q.a for Q in f.X.Q]).reshape(N))
    Sg = np.asarray(f.Sigma, dtype=float)
    blocks = local_jacobian_blocks(origin, group)
    lm0 = np.array([Sg[11 + 3 * i:14 + 3 * i, 11 + 3 * i:14 + 3 * i] for i in range(N)]).reshape(N, 3, 3)
    lmloc = np.array([blocks["lm"][i] @ lm0[i] @ blocks["lm"][i].T for i in range(N)]).reshape(N, 3, 3)
    base = Sg[:11, :11].copy()
    if local:
        Jb = jacobian_matrix(dict(G=blocks["G"], RAt=blocks["RAt"], lm=np.zeros((0, 3, 3))))
        base = Jb @ base @ Jb.T
    p = np.asarray(est.p, dtype=float).reshape(N, 3)
    C = output_blocks(origin["p"])
    S = np.array([C[i] @ lm0[i] @ C[i].T + measurement_variance * np.eye(2) for i in range(N)]).reshape(N, 2, 2)
    return dict(time=float(f.getTime()), steps=steps, pose_q=np.array(est.pose.q, dtype=float), pose_x=np.array(est.pose.x, dtype=float),
                velocity=np.array(est.velocity, dtype=float), p=p, bearing=p / np.linalg.norm(p, axis=1, keepdims=True) if N else p,
                base=base, lm=lmloc if local else lm0, S=S, ycov=bearing_cov_host(p, lmloc) if N else np.zeros((0, 3, 3)))


# ---- the innovation lift of the calls that inform a filter outside a vision frame (include/eqf_vio_amd.h: eqf_get_lift_report)
def _so3_exp_matrix(w):
    """SO3.cpp:122-140."""
    th = np.linalg.norm(w)
    A, B = (np.sin(th) / th, (1 - np.cos(th)) / th**2) if abs(th) >= 1e-8 else (1.0, 0.5)
    wx = _skew(w)
    return np.eye(3) + A * wx + B * wx @ wx


def _se3_exp(u):
    """SE3.cpp:139-164 -> (quaternion, translation)."""
    w, v = np.asarray(u[0:3], dtype=float), np.asarray(u[3:6], dtype=float)
    th = np.linalg.norm(w)
    if abs(th) >= 1e-12:
        A = np.sin(th) / th
        B = (1 - np.cos(th)) / th**2
        C = (1 - A) / th**2
    else:
        A, B, C = 1.0, 0.5, 1.0 / 6.0
    wx = _skew(w)
    return _quat_from_matrix(np.eye(3) + A * wx + B * wx @ wx), (np.eye(3) + B * wx + C * wx @ wx) @ v


def _so3_from_vectors(origin, dest):
    """SO3.cpp:155-167."""
    o, d = origin / np.linalg.norm(origin), dest / np.linalg.norm(dest)
    v, c = np.cross(o, d), float(o @ d)
    if abs(1 + c) <= 1e-8:
        raise ValueError("the vectors cannot be exactly opposing (SO3.cpp:160)")
    vx = _skew(v)
    return _quat_from_matrix(np.eye(3) + (vx + 1.0 / (1.0 + c) * vx @ vx))


def lift_rows(state):
    """Z_P's landmark rows (3N, 6): Qhat_i R_C^T [(x0 - pHat_i)^x R0, R0] (EqFMatrices.cpp:221-235 with D and the coefficient matrix
    multiplied out).  state: see bundle_lift_host."""
    o, g, cam = state["origin"], state["group"], state["camera"]
    P0q, x0 = np.asarray(o["q"], dtype=float), np.asarray(o["x"], dtype=float)
    p0 = np.asarray(o["p"], dtype=float).reshape(-1, 3)
    Aq, Ax = np.asarray(g["Aq"], dtype=float), np.asarray(g["Ax"], dtype=float)
    Qq, Qa = np.asarray(g["Qq"], dtype=float).reshape(-1, 4), np.asarray(g["Qa"], dtype=float).reshape(-1)
    cq, cx = np.asarray(cam["q"], dtype=float), np.asarray(cam["x"], dtype=float)
    Pq, Px = _quat_mul(P0q, Aq), x0 + _quat_rotate(P0q, Ax)        # xiHat.pose = xi0.pose * X.A
    PCq, PCx = _quat_mul(Pq, cq), Px + _quat_rotate(Pq, cx)        # ... * cameraOffset
    RCt = quat_to_matrix(_quat_inverse(PCq))
    R0 = quat_to_matrix(P0q)
    Z = np.zeros((3 * len(Qa), 6))
    for i in range(len(Qa)):
        qhat = _quat_rotate(_quat_inverse(Qq[i]), p0[i]) / Qa[i]
        pHat = _quat_rotate(PCq, qhat) + PCx
        M = Qa[i] * quat_to_matrix(Qq[i]) @ RCt
        Z[3 * i : 3 * i + 3, 0:3] = M @ _skew(x0 - pHat) @ R0
        Z[3 * i : 3 * i + 3, 3:6] = M @ R0
    return Z


def bundle_lift_host(gamma, state, Sigma):
    """The numpy statement of the innovation lift FilterBatch.update_linear / update_landmarks / apply_increment / perturb take with
    set_option("innovation_lift", 1) (include/eqf_vio_amd.h: eqf_get_lift_report; the reference's bundleLift, EqFMatrices.cpp:173-252,
    then the group step of VIOFilter.cpp:292-296).
    gamma (11 + 3N,): the increment in the reference's index map.  Sigma (11 + 3N, 11 + 3N): the covariance the call STARTED from.
    state: dict with origin (FilterBatch.origin()), group (FilterBatch.group()), bias (6,), camera = dict(q, x) the camera offset, and
    discrete: useDiscreteInnovationLift.  Returns a dict with DeltaU (6,), group (the new X, as FilterBatch.group()), bias, min_pivot (the
    smallest squared pivot of Sigma_e's Cholesky factor) and pivot_ratio (min / max |pivot| of the 4 x 4 elimination, here the R factor's)."""
    gamma = np.asarray(gamma, dtype=float)
    o, g = state["origin"], state["group"]
    N = len(np.asarray(g["Qa"]).reshape(-1))
    ge = gamma[6:]
    eta0 = gravity_dir(o["q"])
    eta0 = eta0 / np.linalg.norm(eta0)
    dUw = -_skew(eta0) @ stereo_sphere_chart_inv_diff_at_zero(eta0) @ ge[0:2]
    dUf = np.concatenate([(np.eye(3) - np.outer(eta0, eta0)) @ dUw, np.zeros(3)])
    ZP = np.zeros((5 + 3 * N, 6))
    ZP[5:] = lift_rows(state)
    rhs = np.zeros(5 + 3 * N)
    rhs[5:] = ge[5:]
    L = np.linalg.cholesky(np.asarray(Sigma, dtype=float)[6:, 6:])
    Zt = _solve_lower(L, ZP)
    z = _solve_lower(L, rhs)
    G6, h = Zt.T @ Zt, Zt.T @ z
    K = np.zeros((6, 4))
    K[0:3, 0] = eta0
    K[3:6, 1:4] = np.eye(3)
    M = K.T @ G6 @ K
    x = np.linalg.solve(M, K.T @ (-h - G6 @ dUf))
    dU = dUf + K @ x
    piv = np.abs(np.diag(np.linalg.qr(M)[1]))
    # X <- Delta X
    v0 = np.asarray(o["v"], dtype=float)
    p0 = np.asarray(o["p"], dtype=float).reshape(-1, 3)
    DAq, DAx = _se3_exp(dU)
    if state.get("discrete", True):
        Dw = v0 - _quat_rotate(DAq, v0 + ge[2:5])                  # EqFMatrices.cpp:254-258
    else:
        Dw = -ge[2:5] - np.cross(dU[0:3], v0)                      # :69-79
    Aq, Ax = np.asarray(g["Aq"], dtype=float), np.asarray(g["Ax"], dtype=float)
    Qq, Qa = np.asarray(g["Qq"], dtype=float).reshape(-1, 4).copy(), np.asarray(g["Qa"], dtype=float).reshape(-1).copy()
    for i in range(N):
        qi, gq = p0[i], ge[5 + 3 * i : 8 + 3 * i]
        if state.get("discrete", True):                            # :262-270
            q1 = qi + gq
            dq, da = _so3_from_vectors(q1, qi), np.linalg.norm(qi) / np.linalg.norm(q1)
        else:                                                      # :84-93, SOT3Exp
            n2 = float(qi @ qi)
            dq, da = _quat_from_matrix(_so3_exp_matrix(-np.cross(qi, gq) / n2)), np.exp(-float(qi @ gq) / n2)
        Qq[i], Qa[i] = _quat_mul(dq, Qq[i]), da * Qa[i]
    group = dict(Aq=_quat_mul(DAq, Aq), Ax=DAx + _quat_rotate(DAq, Ax), w=Dw + _quat_rotate(DAq, np.asarray(g["w"], dtype=float)), Qq=Qq, Qa=Qa)
    return dict(DeltaU=dU, group=group, bias=np.asarray(state["bias"], dtype=float) + gamma[0:6], min_pivot=float(np.min(np.diag(L)) ** 2),
                pivot_ratio=float(piv.min() / piv.max()))


def _solve_lower(L, B):
    """L^-1 B by forward substitution, row by row (no inverse is formed)."""
    X = np.array(B, dtype=float)
    for k in range(L.shape[0]):
        X[k] = (X[k] - L[k, :k] @ X[:k]) / L[k, k]
    return X
