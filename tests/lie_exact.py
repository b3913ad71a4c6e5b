"""TEST INFRASTRUCTURE ONLY -- the Lie-group and sphere-chart operations of the filter's O(N) geometric state in mpmath at 50 digits,
written from the DEFINITIONS and not from the device's (or the oracles') formulas:

    SO(3)       Rodrigues from the angle, with mp.sin / mp.cos (no series, no branch on the angle other than theta == 0)
    SE(3)       V = I + (1 - cos th)/th^2 W + (th - sin th)/th^3 W^2 from the same angle
    a -> b      the minimal rotation: axis a x b, angle atan2(|a x b|, a . b), then Rodrigues -- never 1/(1 + c)
    rotations   always 3 x 3 matrices; a quaternion only enters through rot_of_quat (its normalised rotation), so q / -q is no error
    charts      stereographic projection from e3 after the minimal rotation -pole -> e3; differentials by hand from the projection
    SOT(3)      (R, a) acting as a R p; exp(w, s) = (exp w, e^s)

Inputs are taken as exact doubles (mpf(float) is exact).  The STRUCTURE of the group step (lift, product, action) is the project's own and
follows oracle/eqf_numpy.py: lift_velocity, lift_velocity_discrete, VIOGroup.__mul__, state_group_action, the innovation lifts.
tests/test_lie_exact.py pins this file against that oracle on benign input and measures the oracle against it on edge input."""
import numpy as np
from mpmath import mp, mpf

mp.dps = 50
GRAVITY = mpf("9.81")
U = 2.0 ** -53


# ---- plain 3-vectors / 3 x 3 matrices as lists of mpf ------------------------------------------------------------------------------------
def vec(a):
    return [mpf(float(x)) for x in np.asarray(a, dtype=float).reshape(-1)]


def mat(a):
    a = np.asarray(a, dtype=float)
    return [[mpf(float(x)) for x in row] for row in a]


def eye():
    return [[mpf(int(i == j)) for j in range(3)] for i in range(3)]


def E3():
    return [mpf(0), mpf(0), mpf(1)]


def dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def norm(a):
    return mp.sqrt(dot(a, a))


def unit(a):
    n = norm(a)
    return [x / n for x in a]


def add(a, b):
    return [x + y for x, y in zip(a, b)]


def sub(a, b):
    return [x - y for x, y in zip(a, b)]


def scl(c, a):
    return [c * x for x in a]


def mm(A, B):
    return [[sum(A[i][k] * B[k][j] for k in range(len(B))) for j in range(len(B[0]))] for i in range(len(A))]


def mv(A, v):
    return [sum(A[i][k] * v[k] for k in range(len(v))) for i in range(len(A))]


def tr(A):
    return [[A[j][i] for j in range(len(A))] for i in range(len(A[0]))]


def madd(A, B):
    return [[x + y for x, y in zip(ra, rb)] for ra, rb in zip(A, B)]


def mscl(c, A):
    return [[c * x for x in row] for row in A]


def hat(w):
    z = mpf(0)
    return [[z, -w[2], w[1]], [w[2], z, -w[0]], [-w[1], w[0], z]]


def outer(a, b):
    return [[x * y for y in b] for x in a]


def inv3(A):
    """The inverse of a 3 x 3 matrix from its definition (adjugate / determinant)."""
    c = [cross(A[1], A[2]), cross(A[2], A[0]), cross(A[0], A[1])]
    det = dot(A[0], c[0])
    return [[c[j][i] / det for j in range(3)] for i in range(3)]


def to_np(A):
    return np.array([[float(x) for x in row] for row in A]) if isinstance(A[0], list) else np.array([float(x) for x in A])


# ---- SO(3), SE(3), SOT(3) ------------------------------------------------------------------------------------------------------------------
def exp_coefficients(t):
    """A = sin th / th, B = (1 - cos th)/th^2, C = (th - sin th)/th^3 of t = th^2 (their limits at 0)."""
    t = mpf(t)
    if t == 0:
        return mpf(1), mpf(1) / 2, mpf(1) / 6
    th = mp.sqrt(t)
    return mp.sin(th) / th, (1 - mp.cos(th)) / t, (th - mp.sin(th)) / (t * th)


def so3_exp(w):
    A, B, _ = exp_coefficients(dot(w, w))
    W = hat(w)
    return madd(eye(), madd(mscl(A, W), mscl(B, mm(W, W))))


def se3_exp(w, v):
    """(R, x) = exp of the twist (w, v): x = V v."""
    A, B, C = exp_coefficients(dot(w, w))
    W = hat(w)
    W2 = mm(W, W)
    return madd(eye(), madd(mscl(A, W), mscl(B, W2))), mv(madd(eye(), madd(mscl(B, W), mscl(C, W2))), v)


def rot_a_to_b(a, b):
    """The minimal rotation taking the direction of a to the direction of b."""
    a, b = unit(a), unit(b)
    n = cross(a, b)
    s, c = norm(n), dot(a, b)
    if s == 0:
        if c > 0:
            return eye()
        raise ValueError("antipodal")
    return so3_exp(scl(mp.atan2(s, c) / s, n))


def rot_of_quat(q):
    """The rotation of the quaternion (w, x, y, z) / |q| from its definition v -> q v q^-1."""
    w, x, y, z = unit(vec(q))
    u = [x, y, z]
    ux = hat(u)
    return madd(eye(), madd(mscl(2 * w, ux), mscl(mpf(2), mm(ux, ux))))


def se3_mul(a, b):
    return mm(a[0], b[0]), add(a[1], mv(a[0], b[1]))


def se3_inv(a):
    Rt = tr(a[0])
    return Rt, scl(-1, mv(Rt, a[1]))


def se3_apply(a, p):
    return add(mv(a[0], p), a[1])


def se3_adjoint_apply(T, w, v):
    """Ad(T)(w; v) = (R w; x x R w + R v)."""
    Rw = mv(T[0], w)
    return Rw, add(cross(T[1], Rw), mv(T[0], v))


def sot3_exp(w, s):
    return so3_exp(w), mp.exp(s)


def sot3_apply(Q, p):
    return scl(Q[1], mv(Q[0], p))


def sot3_apply_inv(Q, p):
    return scl(1 / Q[1], mv(tr(Q[0]), p))


# ---- sphere charts -------------------------------------------------------------------------------------------------------------------------
def sphere_rot(pole):
    """R_s(pole): the minimal rotation -pole -> e3."""
    return rot_a_to_b(scl(-1, pole), E3())


def project(eta):
    """Stereographic projection of the unit sphere from e3 onto the plane z = 0."""
    return [eta[0] / (1 - eta[2]), eta[1] / (1 - eta[2])]


def project_diff(eta):
    """d project / d eta (2 x 3), eta as a point of R^3."""
    s = 1 / (1 - eta[2])
    return [[s, mpf(0), eta[0] * s * s], [mpf(0), s, eta[1] * s * s]]


def chart(eta, pole):
    return project(mv(sphere_rot(pole), eta))


def chart_diff(eta, pole):
    Rs = sphere_rot(pole)
    return mm(project_diff(mv(Rs, eta)), Rs)


def chart_inv_diff_at_zero(pole):
    """d/dy at y = 0 of R_s^T project^-1(y), project^-1(y) = e3 + 2/(|y|^2 + 1) ((y, 0) - e3): 2 R_s^T [e1 e2]   (3 x 2)."""
    Rt = tr(sphere_rot(pole))
    return [[2 * Rt[i][0], 2 * Rt[i][1]] for i in range(3)]


# ---- the filter's constants ----------------------------------------------------------------------------------------------------------------
def landmark_constants(p0):
    """C0i (2 x 3) = 1/|p| chart_diff(y, y) (I - y y^T) and R_s(y), y = p/|p|, of an origin landmark."""
    p0 = vec(p0)
    y = unit(p0)
    P = madd(eye(), mscl(-1, outer(y, y)))
    return mscl(1 / norm(p0), mm(chart_diff(y, y), P)), sphere_rot(y)


def pose_constants(R0):
    """eta0 = R0^T e3, cDiff = chart_diff(eta0, eta0), cInv = chart_inv_diff_at_zero(eta0)."""
    eta0 = mv(tr(R0), E3())
    return eta0, chart_diff(eta0, eta0), chart_inv_diff_at_zero(eta0)


def residual(y, RQ, p0):
    """output_coordinate_chart of one landmark: chart(R_Q y, p0/|p0|) (the output action of X^-1 is y -> R_Q y)."""
    return chart(mv(RQ, vec(y)), unit(vec(p0)))


# ---- the group ------------------------------------------------------------------------------------------------------------------------------
class Group:
    """X = (A in SE(3), w in R^3, Q_i in SOT(3)); every rotation a matrix."""

    def __init__(self, AR, Ax, w, Q):
        self.AR, self.Ax, self.w, self.Q = AR, Ax, w, Q

    @staticmethod
    def from_dict(g):
        """The dictionary of FilterBatch.group() / OracleFilter.group()."""
        return Group(rot_of_quat(g["Aq"]), vec(g["Ax"]), vec(g["w"]),
                     [(rot_of_quat(q), mpf(float(a))) for q, a in zip(np.asarray(g["Qq"]).reshape(-1, 4), np.asarray(g["Qa"]).reshape(-1))])

    def __mul__(self, o):
        R, x = se3_mul((self.AR, self.Ax), (o.AR, o.Ax))
        return Group(R, x, add(self.w, mv(self.AR, o.w)), [(mm(a[0], b[0]), a[1] * b[1]) for a, b in zip(self.Q, o.Q)])


class State:
    """xi0: pose (R, x), body velocity, landmarks in the camera frame, camera offset (R, x)."""

    def __init__(self, R, x, v, p, camR, camx):
        self.R, self.x, self.v, self.p, self.camR, self.camx = R, x, v, p, camR, camx

    @staticmethod
    def from_dict(o, camq, camx):
        return State(rot_of_quat(o["q"]), vec(o["x"]), vec(o["v"]), [vec(p) for p in np.asarray(o["p"]).reshape(-1, 3)], rot_of_quat(camq), vec(camx))


def state_group_action(X, s):
    Rt = tr(X.AR)
    R, x = se3_mul((s.R, s.x), (X.AR, X.Ax))
    return State(R, x, mv(Rt, sub(s.v, X.w)), [sot3_apply_inv(Q, p) for Q, p in zip(X.Q, s.p)], s.camR, s.camx)


def _camera_twist(s, omega):
    return se3_adjoint_apply(se3_inv((s.camR, s.camx)), omega, s.v)


def lift_velocity_discrete(s, omega, accel, dt):
    """The group element of one step of length dt from the state s under the sample (omega, accel)."""
    eta = mv(tr(s.R), E3())
    AR, Ax = se3_exp(scl(dt, omega), scl(dt, s.v))
    inner = add(s.v, scl(dt, add(add(scl(-1, cross(omega, s.v)), accel), scl(-GRAVITY, eta))))
    w = sub(s.v, mv(AR, inner))
    oC, vC = _camera_twist(s, omega)
    cam = se3_exp(scl(-dt, oC), scl(-dt, vC))
    Q = []
    for p0 in s.p:
        p1 = se3_apply(cam, p0)
        Q.append((rot_a_to_b(p1, p0), norm(p0) / norm(p1)))
    return Group(AR, Ax, w, Q)


def lift_velocity_exp(s, omega, accel, dt):
    """exp(dt * lift_velocity(s, (omega, accel)))."""
    eta = mv(tr(s.R), E3())
    AR, Ax = se3_exp(scl(dt, omega), scl(dt, s.v))
    w = scl(dt, add(scl(-1, accel), scl(GRAVITY, eta)))
    oC, vC = _camera_twist(s, omega)
    Q = []
    for p in s.p:
        n2 = dot(p, p)
        Q.append(sot3_exp(scl(dt, add(oC, scl(1 / n2, cross(p, vC)))), dt * dot(p, vC) / n2))
    return Group(AR, Ax, w, Q)


def group_step(X, xi0, omega, accel, dt, discrete):
    """X <- X * lift(xiHat, u, dt), xiHat = X acting on xi0; omega / accel the (unbiased) currentVelocity."""
    cur = state_group_action(X, xi0)
    om, ac, dt = vec(omega), vec(accel), mpf(float(dt))
    return X * (lift_velocity_discrete(cur, om, ac, dt) if discrete else lift_velocity_exp(cur, om, ac, dt))


def innovation_element(xi0, dU, gv, gq, mode, gg=None):
    """Delta for the algebra element (dU (6), gamma_v (3), gamma_q (N, 3)) at the origin xi0.  mode: "discrete" | "continuous" (the
    exponential of the lifted element) | "nolift" (dU is ignored: its rotational part is -eta0 x (cInv gamma_g), gg = gamma_g (2))."""
    gv = vec(gv)
    gq = [vec(g) for g in np.asarray(gq).reshape(-1, 3)]
    if mode == "nolift":
        eta0, _, ci = pose_constants(xi0.R)
        g2 = vec(gg)
        Uw, Uv = scl(-1, cross(eta0, [ci[i][0] * g2[0] + ci[i][1] * g2[1] for i in range(3)])), [mpf(0)] * 3
    else:
        d = vec(dU)
        Uw, Uv = d[0:3], d[3:6]
    AR, Ax = se3_exp(Uw, Uv)
    Q = []
    if mode == "discrete":
        w = sub(xi0.v, mv(AR, add(xi0.v, gv)))
        for q, g in zip(xi0.p, gq):
            q1 = add(q, g)
            Q.append((rot_a_to_b(q1, q), norm(q) / norm(q1)))
    else:
        w = sub(scl(-1, gv), cross(Uw, xi0.v))
        for q, g in zip(xi0.p, gq):
            n2 = dot(q, q)
            Q.append(sot3_exp(scl(-1 / n2, cross(q, g)), -dot(q, g) / n2))
    return Group(AR, Ax, w, Q)


def apply_innovation(X, xi0, dU, gv, gq, mode, gg=None):
    """X <- Delta * X."""
    return innovation_element(xi0, dU, gv, gq, mode, gg) * X


def reference_step(snap, stamp, d):
    """One group step of a snapshot (FilterBatch.dump_state format) to `stamp` under the settings dictionary d: (X, estimate) after it."""
    xi0 = State.from_dict(snap["origin"], d["cameraOffset_q"], d["cameraOffset_x"])
    cv = snap["currentVelocity"]
    X = group_step(Group.from_dict(snap["group"]), xi0, cv[0:3], cv[3:6], float(stamp) - float(snap["time"]), bool(d["useDiscreteVelocityLift"]))
    return X, state_group_action(X, xi0)


def prefix(X, est, n):
    """The first n landmarks of a (Group, State) pair: the step of one landmark does not depend on the others."""
    return Group(X.AR, X.Ax, X.w, X.Q[:n]), State(est.R, est.x, est.v, est.p[:n], est.camR, est.camx)


def pole_ratio(got, want, theta, scale=1.0):
    """max |got - want| / ((u / theta^2) scale): the bound form near the chart pole."""
    w = want if isinstance(want[0], list) else [want]
    g = np.asarray(got, dtype=float).reshape(len(w), -1)
    err = max(abs(mpf(float(g[i, j])) - w[i][j]) for i in range(len(w)) for j in range(len(w[0])))
    return float(err * mpf(float(theta)) ** 2 / (mpf(U) * mpf(float(scale))))


# ---- comparison in the bound form  K u (1 + magnitude)------------------------------------------------------------------------------------
def ratio(got, want, mag=None):
    """max |got - want| / (u (1 + magnitude)), magnitude = max |want| unless given; got a float array, want an mpf vector / matrix."""
    w = want if isinstance(want[0], list) else [want]
    g = np.asarray(got, dtype=float).reshape(len(w), -1)
    err = max(abs(mpf(float(g[i, j])) - w[i][j]) for i in range(len(w)) for j in range(len(w[0])))
    m = max(abs(x) for row in w for x in row) if mag is None else mpf(mag)
    return float(err / (mpf(U) * (1 + m)))


def group_ratios(g, Xref, est=None, est_ref=None):
    """The state of a filter (dictionaries of group() and, optionally, state_estimate()) against the reference, as ratios to u (1 + magnitude):
    {"A.R", "A.x", "w", "Q.R", "Q.a", and "est.R", "est.x", "est.v", "est.p" when est is given}.  Quaternions go through their matrices."""
    from_q = lambda q: to_np(rot_of_quat(q))  # noqa: E731  (exact to 50 digits, then rounded: its own error is below u)
    out = {"A.R": ratio(from_q(g["Aq"]), Xref.AR), "A.x": ratio(g["Ax"], Xref.Ax), "w": ratio(g["w"], Xref.w), "Q.R": 0.0, "Q.a": 0.0}
    for i, Q in enumerate(Xref.Q):
        out["Q.R"] = max(out["Q.R"], ratio(from_q(g["Qq"][i]), Q[0]))
        out["Q.a"] = max(out["Q.a"], ratio([g["Qa"][i]], [Q[1]]))
    if est is not None:
        out.update({"est.R": ratio(from_q(est["q"]), est_ref.R), "est.x": ratio(est["x"], est_ref.x), "est.v": ratio(est["v"], est_ref.v), "est.p": 0.0})
        for i, p in enumerate(est_ref.p):
            out["est.p"] = max(out["est.p"], ratio(est["p"][i], p))
    return out
