"""TEST INFRASTRUCTURE ONLY -- the rows eqf_observe_landmarks forms on the device (csrc/eqf_observe.hpp, eqf_observe_host.hpp), entry by
entry: a reference from the definitions at 50 digits (mpmath, through tests/lie_exact.py: the chart is the stereographic projection
behind the minimal rotation -pole -> e3, Q_i^-1 p = a_i^-1 R(q_i)^T p with R(q) the rotation v -> q v q^-1 of q / |q|), an a-priori
first-order bound, and a restatement of the rows with switchable faults.  Nothing of oracle/ is imported.

THE REFERENCE (reference()).  p0_i, q_i, a_i, q_c, t_c and meas are exact doubles; q_c is normalised exactly.  Per entry
    J = a^-1 R(q)^T   p_hat = J p0   v = p_hat - t_c   p_c = R_c^T v   d = |p_c|   y_hat = p_c / d
    bearing   H = chart_diff(y_hat, y_hat) (I - y_hat y_hat^T) R_c^T / d     resid = chart(y, pole y_hat)
    range     H = y_hat^T R_c^T                                              resid = rho - d
    position  H = R_c^T                                                      resid = m - p_c
    Ht = H J

THE BOUND is K_OBS u times the sum of absolute terms of each entry's evaluation, computed in the reference stage by stage: every stage
adds the sum of the absolute values of its own terms to what its inputs carry, the inputs' share weighted by the absolute partial
derivatives (taken at 50 digits, by central differences where the stage is a chart function).  With |.| entrywise, T(q) the sum of the
absolute terms of Eigen's toRotationMatrix, and s_x the sum carried by x:
    s_J  = T(q)^T / |a|                      s_Rc = T(q_c) + |dR/dq| |q_c|        (the normalisation of q_c)
    s_ph = |J||p0| + s_J |p0|                s_v  = s_ph + |p_hat| + |t_c|
    s_pc = |R_c^T| (s_v + |v|) + s_Rc^T |v|  s_d  = |y_hat|^T s_pc + d            s_y = (s_pc + |y_hat| s_d) / d + |y_hat|
    range     s_H = s_y^T |R_c^T| + |y_hat|^T (s_Rc^T + |R_c^T|)                  s_r = |rho| + s_d
    position  s_H = s_Rc^T                                                        s_r = |m| + s_pc
    bearing   with w = 1 + |n| + |n|^2 / (1 + c), n = -y_hat x e3, c = -y_hat . e3 (the terms of SO3FromVectors' rotation)
              s_Rs = |dR_s/dy_hat| s_y + w          s_cd = |d chart_diff / d y_hat| s_y + w
              s_P  = |y_hat| s_y^T + s_y |y_hat|^T + |y_hat||y_hat|^T + I          A = chart_diff P
              s_A  = s_cd |P| + |cd| s_P + |cd||P|
              s_H  = (s_A |R_c^T| + |A| (s_Rc^T + |R_c^T|)) / d + |H| s_d / d
              rho = R_s y:  s_rho = (s_Rs + |R_s|) |y|
              s_r[j] = s_rho[j] / (1 - rho_z) + |rho_j| (s_rho[z] + 1 + |rho_z|) / (1 - rho_z)^2 + |resid_j|
    Ht:       s_Ht = s_H |J| + |H| (s_J + |J|)
K_OBS is the next power of two above 4 x the worst ratio of consistency.observe_rows_host (numpy, fp64) to this form over the committed
cases of tests/observe_cases.py; tests/test_observe_exact.py re-measures the ratio.  u = 2^-53.  A zero bound means an exact value."""
import numpy as np
from mpmath import mp, mpf

import lie_exact as lx

U = 2.0 ** -53
K_OBS_MEASURED = 4.760364495308264  # the numpy statement's worst ratio to the unit form over the committed cases (test_observe_exact.py re-measures it)
K_OBS = 32.0  # the next power of two above 4 x K_OBS_MEASURED = 19.04
BEARING, RANGE, POSITION = 0, 1, 2
ROWS = {BEARING: 2, RANGE: 1, POSITION: 3}
FAULTS = ("rc_transposed", "tc_sign", "inv_d_squared", "pole_at_y", "j_without_scale", "h_left_in_camera_frame", "resid_sign",
          "j_transposed")
# one more candidate, the projector (I - y_hat y_hat^T) left out, is no fault -- it changes nothing: chart_diff(y_hat, y_hat) y_hat = 0 exactly (the
# chart's differential at its own base point annihilates the radial direction); test_observe_exact.py asserts that instead
NO_FAULT = ("projector_missing",)
_H = mpf(10) ** -25


def _abs(A):
    return [[abs(x) for x in r] for r in A] if isinstance(A[0], list) else [abs(x) for x in A]


def _ones(r, c, v):
    return [[v for _ in range(c)] for _ in range(r)]


def rot_terms(q):
    """T(q): the sums of the absolute terms of Eigen's toRotationMatrix at the unit quaternion q"""
    w, x, y, z = [abs(v) for v in q]
    return [[1 + 2 * y * y + 2 * z * z, 2 * x * y + 2 * w * z, 2 * x * z + 2 * w * y],
            [2 * x * y + 2 * w * z, 1 + 2 * x * x + 2 * z * z, 2 * y * z + 2 * w * x],
            [2 * x * z + 2 * w * y, 2 * y * z + 2 * w * x, 1 + 2 * x * x + 2 * y * y]]


def _dmat(f, x):
    """|d f / d x_j| for a matrix-valued f of a 3- or 4-vector, central differences at 50 digits: a list over j of matrices"""
    out = []
    for j in range(len(x)):
        xp, xm = list(x), list(x)
        xp[j], xm[j] = x[j] + _H, x[j] - _H
        Fp, Fm = f(xp), f(xm)
        out.append([[abs(a - b) / (2 * _H) for a, b in zip(rp, rm)] for rp, rm in zip(Fp, Fm)])
    return out


def _weighted(D, s):
    """sum_j D[j] s[j]"""
    out = _ones(len(D[0]), len(D[0][0]), mpf(0))
    for Dj, sj in zip(D, s):
        out = lx.madd(out, lx.mscl(sj, Dj))
    return out


def entry(kind, p0, q, a, cam, meas, fault=None):
    """One entry at 50 digits: (Ht rows x 3, resid rows, s_Ht, s_resid) as lists of mpf; None when the entry is not observable (d = 0, or
    a bearing with y_hat at e3 or y at the antipode of y_hat).  fault: one of FAULTS / NO_FAULT (the bound terms are then meaningless)."""
    rows = ROWS[kind]
    p0, a = lx.vec(p0), mpf(float(a))
    qn = lx.unit(lx.vec(q))
    qc = lx.unit(lx.vec(cam[:4]))
    tc = lx.vec(cam[4:7])
    R, Rc = lx.rot_of_quat(q), lx.rot_of_quat(cam[:4])
    J = lx.mscl(1 / a, lx.tr(R))
    if fault == "j_without_scale":
        J = lx.tr(R)
    if fault == "j_transposed":
        J = lx.mscl(1 / a, R)
    Jest = lx.mscl(1 / a, lx.tr(R))  # (the estimate itself is never the faulty part)
    s_J = lx.mscl(1 / abs(a), lx.tr(rot_terms(qn)))
    s_Rc = lx.madd(rot_terms(qc), _weighted(_dmat(_rot_unit, qc), _abs(qc)))
    ph = lx.mv(Jest, p0)
    s_ph = lx.add(lx.mv(_abs(Jest), _abs(p0)), lx.mv(s_J, _abs(p0)))
    v = lx.add(ph, tc) if fault == "tc_sign" else lx.sub(ph, tc)
    s_v = lx.add(s_ph, lx.add(_abs(ph), _abs(tc)))
    Rct = Rc if fault == "rc_transposed" else lx.tr(Rc)
    aRct, s_Rct = _abs(lx.tr(Rc)), lx.tr(s_Rc)
    pc = lx.mv(Rct, v)
    s_pc = lx.add(lx.mv(aRct, lx.add(s_v, _abs(v))), lx.mv(s_Rct, _abs(v)))
    d = lx.norm(pc)
    if d == 0:
        return None
    yh = lx.scl(1 / d, pc)
    ay = _abs(yh)
    s_d = lx.dot(ay, s_pc) + d
    s_y = lx.add(lx.scl(1 / d, lx.add(s_pc, lx.scl(s_d, ay))), ay)
    meas = lx.vec(meas)
    if kind == POSITION:
        H, s_H = Rct, s_Rct
        resid, s_r = lx.sub(meas, pc), lx.add(_abs(meas), s_pc)
    elif kind == RANGE:
        H = [lx.mv(lx.tr(Rct), yh)]
        s_H = [lx.add(lx.mv(lx.tr(aRct), s_y), lx.mv(lx.tr(lx.madd(s_Rct, aRct)), ay))]
        resid, s_r = [meas[0] - d], [abs(meas[0]) + s_d]
    else:
        if abs(1 - yh[2]) == 0:
            return None
        cvec = lx.cross(lx.scl(-1, yh), lx.E3())
        c = -yh[2]
        w = 1 + lx.norm(cvec) + lx.dot(cvec, cvec) / (1 + c)
        pole = meas if fault == "pole_at_y" else yh
        Rs = lx.sphere_rot(yh)
        s_Rs = lx.madd(_weighted(_dmat(lx.sphere_rot, yh), s_y), _ones(3, 3, w))
        cd = lx.chart_diff(pole, pole)
        s_cd = lx.madd(_weighted(_dmat(lambda x: lx.chart_diff(x, x), yh), s_y), _ones(2, 3, w))
        P = lx.eye() if fault == "projector_missing" else lx.madd(lx.eye(), lx.mscl(-1, lx.outer(yh, yh)))
        s_P = lx.madd(lx.madd(lx.outer(ay, s_y), lx.outer(s_y, ay)), lx.madd(lx.outer(ay, ay), lx.eye()))
        A = lx.mm(cd, P)
        s_A = lx.madd(lx.madd(lx.mm(s_cd, _abs(P)), lx.mm(_abs(cd), s_P)), lx.mm(_abs(cd), _abs(P)))
        dd = d * d if fault == "inv_d_squared" else d
        H = lx.mscl(1 / dd, lx.mm(A, Rct))
        s_H = lx.madd(lx.mscl(1 / d, lx.madd(lx.mm(s_A, aRct), lx.mm(_abs(A), lx.madd(s_Rct, aRct)))), lx.mscl(s_d / d, _abs(H)))
        try:
            rho = lx.mv(lx.sphere_rot(pole), meas)
        except ValueError:
            return None
        if 1 - rho[2] == 0:
            return None
        resid = lx.project(rho)
        s_rho = lx.mv(lx.madd(s_Rs, _abs(Rs)), _abs(meas))
        g = 1 - rho[2]
        s_r = [s_rho[j] / g + abs(rho[j]) * (s_rho[2] + 1 + abs(rho[2])) / (g * g) + abs(resid[j]) for j in range(2)]
    if fault == "h_left_in_camera_frame" and kind != POSITION:
        H = lx.mm(H, Rc)
    if fault == "h_left_in_camera_frame" and kind == POSITION:
        H = lx.eye()
    if fault == "resid_sign":
        resid = lx.scl(-1, resid)
    Ht = lx.mm(H, J)
    s_Ht = lx.madd(lx.mm(s_H, _abs(Jest)), lx.mm(_abs(H), lx.madd(s_J, _abs(Jest))))
    return Ht, resid, s_Ht, s_r[:rows]


def _rot_unit(q):
    """R of a quaternion taken as it is (lists of mpf), normalised: rot_of_quat on mpf input"""
    w, x, y, z = lx.unit(q)
    ux = lx.hat([x, y, z])
    return lx.madd(lx.eye(), lx.madd(lx.mscl(2 * w, ux), lx.mscl(mpf(2), lx.mm(ux, ux))))


def reference(kind, state, ids, meas, cam=None, fault=None):
    """The rows of one filter from a dump_state dictionary: dict(Ht (K, rows, 3), resid (K, rows) -- lists of mpf per entry, None where the
    entry is not formed --, used (K,): 1 formed, 0 id not in the state, 3 not observable, s_Ht, s_resid: the bound's sums of absolute terms
    as float arrays (zeros where not formed))"""
    rows = ROWS[kind]
    sid = [int(i) for i in state["ids"]]
    camv = np.array([1.0, 0, 0, 0, 0, 0, 0]) if cam is None else np.concatenate([np.asarray(cam[0], dtype=float), np.asarray(cam[1], dtype=float)])
    p0 = np.asarray(state["origin"]["p"], dtype=float).reshape(-1, 3)
    Qq, Qa = np.asarray(state["group"]["Qq"], dtype=float).reshape(-1, 4), np.asarray(state["group"]["Qa"], dtype=float).reshape(-1)
    K = len(ids)
    meas = np.asarray(meas, dtype=float).reshape(K, 3)
    out = dict(Ht=[None] * K, resid=[None] * K, used=np.zeros(K, dtype=np.uint8), s_Ht=np.zeros((K, rows, 3)), s_resid=np.zeros((K, rows)))
    for k, lid in enumerate(ids):
        if int(lid) not in sid:
            continue
        i = sid.index(int(lid))
        e = entry(kind, p0[i], Qq[i], Qa[i], camv, meas[k], fault) if np.all(np.isfinite(p0[i])) else None
        if e is None:
            out["used"][k] = 3
            continue
        out["used"][k] = 1
        out["Ht"][k], out["resid"][k] = e[0], e[1]
        out["s_Ht"][k] = np.array([[float(x) for x in r] for r in e[2]])
        out["s_resid"][k] = np.array([float(x) for x in e[3]])
    return out


def ratios(Ht, resid, used, ref, k_obs=None):
    """(worst |Ht - ref| / bound, worst |resid - ref| / bound) over the entries, the bound K_OBS u s (k_obs = 1: the unit form); inf when
    used differs, when a value is not finite, or when a zero bound does not see the reference's value exactly; rows of entries that are
    not formed must be zeros"""
    k_obs = K_OBS if k_obs is None else k_obs
    if not np.array_equal(np.asarray(used, dtype=np.uint8), ref["used"]):
        return np.inf, np.inf
    worst = [0.0, 0.0]
    for k in range(len(ref["used"])):
        for w, (got, want, s) in enumerate(((np.asarray(Ht[k]), ref["Ht"][k], ref["s_Ht"][k]), (np.asarray(resid[k]), ref["resid"][k], ref["s_resid"][k]))):
            got = np.asarray(got, dtype=float).reshape(-1)
            if want is None:
                if np.any(got != 0.0):
                    worst[w] = np.inf
                continue
            want = [x for r in want for x in r] if isinstance(want[0], list) else list(want)
            s = np.asarray(s).reshape(-1)
            for g, x, b in zip(got, want, s):
                if not np.isfinite(g):
                    worst[w] = np.inf
                    continue
                err, bound = abs(mpf(float(g)) - x), mpf(k_obs) * mpf(U) * mpf(float(b))
                if bound == 0:
                    if err != 0:
                        worst[w] = np.inf
                else:
                    worst[w] = max(worst[w], float(err / bound))
    return worst[0], worst[1]
