"""The numpy side of explicit landmark edits (eqf_vio_amd/consistency.py): edit_landmarks_host, the host statement of
FilterBatch.edit_landmarks that the GPU tests build their twin handles from, and the two usual priors, depth_prior and triangulation_prior.
No GPU."""
import numpy as np
import pytest

from eqf_vio_amd import consistency as cs

EPS = np.finfo(float).eps


# ---- depth_prior
def _unit(v):
    """A unit vector as a caller would hand it over: normalised in double precision (|y|^2 = 1 + O(eps))."""
    v = np.asarray(v, dtype=float)
    return v / np.linalg.norm(v)


# (bearing, range, var_rng, var_y).  COMPARABLE: the two eigenvalues var_rng and rng^2 var_y within a factor 4 of each other; APART: what a
# depth camera gives (centimetres along the ray, a fraction of a millimetre across it, or the other way round at long range).
COMPARABLE = [([0.1, -0.2, 1.0], 2.0, 4e-4, 1e-4), ([0.7, 0.1, 0.7], 3.0, 2e-3, 1e-4), ([-0.3, 0.9, 0.2], 0.5, 1e-4, 1e-3),
              ([0.0, 0.0, 1.0], 12.0, 0.01, 2.5e-5), ([1.0, 1.0, 1.0], 3.0, 3e-2, 1e-2), ([0.2, 0.3, -0.9], 7.0, 1e-2, 8e-4)]
APART = [([0.1, -0.2, 1.0], 4.0, 0.04, 1e-6), ([0.7, 0.1, 0.7], 0.5, 1e-4, 4e-6), ([-0.3, 0.9, 0.2], 37.5, 2.25, 1e-7),
         ([1.0, 1.0, 1.0], 30.0, 1e-4, 1e-4)]


def _eigen_defects(y, rng, var_rng, var_y):
    """(|P y - lam_r y|_max, lam_r), then the same for two unit vectors orthogonal to y and lam_t; also: P symmetric bit for bit."""
    y = _unit(y)
    p, P = cs.depth_prior(y, rng, var_rng, var_y)
    assert p.tobytes() == (rng * y).tobytes()
    assert P.tobytes() == P.T.copy().tobytes()
    lam_r, lam_t = var_rng, (rng * rng) * var_y
    a = _unit(np.cross(y, [1.0, 0.0, 0.0] if abs(y[0]) < 0.9 else [0.0, 1.0, 0.0]))
    b = _unit(np.cross(y, a))
    return [(np.max(np.abs(P @ y - lam_r * y)), lam_r)] + [(np.max(np.abs(P @ v - lam_t * v)), lam_t) for v in (a, b)]


@pytest.mark.parametrize("y,rng,var_rng,var_y", COMPARABLE)
def test_depth_prior_eigen_structure(y, rng, var_rng, var_y):
    """P y = var_rng y and P v = rng^2 var_y v for two unit vectors v orthogonal to y, to 8 ulp of the eigenvalue, relative.
    Why 8, and why these cases.  An entry of P is fl(lam_r fl(y_i y_j) + lam_t fl(delta_ij - fl(y_i y_j))): with u = eps / 2 the unit
    roundoff, 2 u on the first term, 3 u on the second, 1 u for the sum.  P w for a unit vector w is three such entries times w_j, summed:
    3 u more.  To first order a component of P w - lam w is therefore off by about u (5 lam_r |y_i| |y . w| + 6 lam_t |((I - y y^T) w)_i|)
    plus what the test vectors themselves bring: |y|^2 is 1 only to 2 u, y . v is 0 only to 2 u.  Every term is at most a few u of the
    LARGER of the two eigenvalues -- that is a property of any P formed in floating point, not of this function -- so "8 ulp of the
    eigenvalue under test" can be asked where the eigenvalues are comparable: within a factor 4, the sum above stays below
    u (5 + 6 + 2 + 2) = 7.5 eps of the larger one only in the worst case of every term at its bound, and a component of a unit vector in
    three dimensions cannot meet all of them; 8 eps of the smaller eigenvalue leaves a factor 2 to the typical figure.  The cases whose
    eigenvalues lie far apart are in the test below, against the larger eigenvalue."""
    for defect, lam in _eigen_defects(y, rng, var_rng, var_y):
        assert defect <= 8 * EPS * lam, (defect / (EPS * lam), lam)


@pytest.mark.parametrize("y,rng,var_rng,var_y", APART)
def test_depth_prior_eigenvalues_far_apart(y, rng, var_rng, var_y):
    """The same identities where one eigenvalue is hundreds to thousands of times the other: the defect stays within 8 ulp of the LARGER
    eigenvalue (the bound of the docstring above, whatever the ratio), which is all a 3 x 3 matrix of doubles can say about the smaller."""
    top = max(var_rng, (rng * rng) * var_y)
    for defect, _ in _eigen_defects(y, rng, var_rng, var_y):
        assert defect <= 8 * EPS * top, defect / (EPS * top)


# ---- edit_landmarks_host against a direct statement with np.delete and block assembly
def _dump(rng, ids):
    N = len(ids)
    n = 11 + 3 * N
    a = rng.standard_normal((n, n))
    S = a @ a.T
    S = np.tril(S) + np.tril(S, -1).T
    return dict(ids=np.array(ids, dtype=np.int32), sigma=S, time=0.25, bias=rng.standard_normal(6), currentVelocity=np.zeros(6),
                accumulatedVelocity=np.zeros(6), accumulatedTime=0.0, initialised=1,
                origin=dict(q=np.array([1.0, 0, 0, 0]), x=np.zeros(3), v=np.zeros(3), p=rng.standard_normal((N, 3)) + [0, 0, 4.0]),
                group=dict(Aq=np.array([1.0, 0, 0, 0]), Ax=np.zeros(3), w=np.zeros(3), Qq=_unit_rows(rng.standard_normal((N, 4))),
                           Qa=rng.uniform(0.8, 1.2, N)))


def _unit_rows(a):
    return a / np.linalg.norm(a, axis=1, keepdims=True) if len(a) else a.reshape(0, 4)


def _direct(dump, rem, ins_ids, p, P, accept):
    """np.delete on the rows and columns of every removed landmark, then the accepted priors as diagonal blocks."""
    ids = list(dump["ids"])
    gone = [i for i, x in enumerate(ids) if x in set(rem)]
    cut = [11 + 3 * i + c for i in gone for c in range(3)]
    S = np.delete(np.delete(dump["sigma"], cut, axis=0), cut, axis=1)
    m = S.shape[0]
    out = np.zeros((m + 3 * len(accept), m + 3 * len(accept)))
    out[:m, :m] = S
    for j, k in enumerate(accept):
        L = np.tril(P[k])
        out[m + 3 * j:m + 3 * j + 3, m + 3 * j:m + 3 * j + 3] = L + np.tril(L, -1).T
    keep_ids = [x for x in ids if x not in set(rem)]
    return dict(ids=keep_ids + [ins_ids[k] for k in accept], sigma=out,
                p=np.concatenate([np.delete(dump["origin"]["p"], gone, axis=0), p[accept]]),
                Qq=np.concatenate([np.delete(dump["group"]["Qq"], gone, axis=0), np.tile([1.0, 0, 0, 0], (len(accept), 1))]),
                Qa=np.concatenate([np.delete(dump["group"]["Qa"], gone), np.ones(len(accept))]))


NEG = np.array([[1.0, 0, 0], [0, 1.0, 0], [2.0, 0, 3.0]])
HOST_CASES = {
    # state ids, remove, insert ids, what happens to each insert (1 / 0 / 2; 2 by a bad P, 3: 2 by a NaN position)
    "remove some, insert two": ([7, 3, 9, 12, 5], [3, 12, 40], [1, 2], [1, 1]),
    "replace": ([7, 3, 9], [3], [3, 8], [1, 1]),
    "replace, present and rejected": ([7, 3, 9, 4], [3], [3, 7, 8, 10, 11], [1, 0, 2, 1, 3]),
    "empty state": ([], [], [5, 6, 7], [1, 1, 1]),
    "remove all": ([4, 2], [2, 4], [], []),
    "nothing": ([4, 2], [], [], []),
    "insert only": ([4, 2, 8], [], [9], [1]),
}


@pytest.mark.parametrize("name", list(HOST_CASES))
def test_edit_landmarks_host_against_np_delete(name):
    ids, rem, ins_ids, verdict = HOST_CASES[name]
    rng = np.random.default_rng(len(name))
    dump = _dump(rng, ids)
    k = len(ins_ids)
    p = rng.standard_normal((k, 3)) + [0, 0, 5.0]
    a = rng.standard_normal((k, 3, 3))
    P = a @ np.transpose(a, (0, 2, 1)) + 0.1 * np.eye(3)
    P[:, 0, 2] = np.nan  # (upper triangle: never read)
    for j, v in enumerate(verdict):
        if v == 2:
            P[j] = NEG
        if v == 3:
            p[j, 1] = np.nan
    want_verdict = [2 if v == 3 else v for v in verdict]
    keep_bits = {key: np.array(val).tobytes() if not isinstance(val, dict) else {a_: np.array(b_).tobytes() for a_, b_ in val.items()}
                 for key, val in dump.items()}
    new, removed, inserted = cs.edit_landmarks_host(dump, rem, ins_ids, p, P)
    assert removed.tolist() == [int(r in ids) for r in rem] and inserted.tolist() == want_verdict
    ref = _direct(dump, rem, ins_ids, p, P, [j for j, v in enumerate(want_verdict) if v == 1])
    assert new["ids"].tolist() == ref["ids"] and new["ids"].dtype == np.int32
    assert new["sigma"].tobytes() == ref["sigma"].tobytes()
    assert np.asarray(new["origin"]["p"]).tobytes() == ref["p"].tobytes()
    assert np.asarray(new["group"]["Qq"]).tobytes() == ref["Qq"].tobytes() and np.asarray(new["group"]["Qa"]).tobytes() == ref["Qa"].tobytes()
    for key in ("time", "bias", "currentVelocity", "accumulatedVelocity", "accumulatedTime", "initialised"):
        assert np.array(new[key]).tobytes() == keep_bits[key], key
    for key in ("q", "x", "v"):
        assert np.array(new["origin"][key]).tobytes() == keep_bits["origin"][key]
    for key in ("Aq", "Ax", "w"):
        assert np.array(new["group"][key]).tobytes() == keep_bits["group"][key]
    # the input is not modified
    assert np.array(dump["sigma"]).tobytes() == keep_bits["sigma"] and np.array(dump["ids"]).tobytes() == keep_bits["ids"]


# ---- triangulation_prior against the same formulas in mpmath at 50 digits
# (baseline [m], depth [m], lateral offset of the point [m, m], rotation vector of camera 2 in camera 1 [rad]); rays from exact geometry,
# rounded to double: the reference takes those doubles as its input.  The second to last is nearly parallel (0.05 m at 40 m: 1.25 mrad).
GEOMETRIES = [
    (0.05, 0.5, (0.0, 0.0), (0.0, 0.0, 0.0)), (0.12, 0.5, (0.2, -0.1), (0.01, -0.02, 0.005)), (0.5, 0.5, (-0.1, 0.1), (0.0, 0.03, 0.0)),
    (0.05, 2.0, (0.5, 0.3), (0.0, 0.0, 0.0)), (0.12, 2.0, (-0.8, 0.2), (0.02, 0.01, -0.01)), (0.5, 4.0, (1.0, -1.0), (0.0, -0.05, 0.01)),
    (0.12, 8.0, (2.0, 1.0), (0.005, 0.0, 0.0)), (0.3, 15.0, (-3.0, 2.0), (0.0, 0.01, 0.02)), (0.5, 40.0, (5.0, -4.0), (0.01, 0.01, 0.01)),
    (0.12, 40.0, (0.0, 0.0), (0.0, 0.0, 0.0)), (0.05, 40.0, (1.0, 0.5), (0.0, 0.002, 0.0)), (0.2, 1.0, (0.6, 0.6), (-0.03, 0.02, 0.04)),
]
VAR_Y = 1e-6
# K measured with the numpy function on the twelve geometries above, on the CPU (x86-64, numpy with its own LAPACK; the test prints the
# ratios per geometry with -s):
#   p: max |p - p_ref| / (eps cond(A) |p_ref|)            = 0.474   (the 0.05 m baseline at 40 m)
#   P: max |P - P_ref|_F / (eps cond(A)^2 |P_ref|_F)      = 0.0095  (the 0.5 m baseline at 0.5 m; cond^2 is a loose form for P)
# with a factor 4 of margin:
K_P, K_COV = 4 * 0.474, 4 * 0.0095


def _quat_from_rotvec(w):
    w = np.asarray(w, dtype=float)
    th = np.linalg.norm(w)
    if th == 0.0:
        return np.array([1.0, 0.0, 0.0, 0.0])
    return np.concatenate([[np.cos(th / 2)], np.sin(th / 2) * w / th])


def _geometry(g):
    base, depth, (ox, oy), rv = g
    q21 = _quat_from_rotvec(rv)
    t21 = np.array([base, 0.01 * base, -0.02 * base])
    pt = np.array([ox, oy, depth])
    R = cs.quat_to_matrix(q21)
    p2 = R.T @ (pt - t21)
    return _unit(pt), _unit(p2), q21, t21


def _mp_reference(y1, y2, q21, t21, var_y):
    import mpmath as mp

    mp.mp.dps = 50
    w, x, y, z = [mp.mpf(float(v)) for v in q21]
    R = mp.matrix([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                   [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                   [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    d = [mp.matrix([mp.mpf(float(v)) for v in y1]), R * mp.matrix([mp.mpf(float(v)) for v in y2])]
    c = [mp.matrix([0, 0, 0]), mp.matrix([mp.mpf(float(v)) for v in t21])]
    M = [mp.eye(3) - dk * dk.T for dk in d]
    A = M[0] + M[1]
    p = mp.lu_solve(A, M[0] * c[0] + M[1] * c[1])
    W = mp.zeros(3)
    for Mk, ck in zip(M, c):
        e = p - ck
        W += Mk / ((e.T * e)[0] * mp.mpf(var_y))
    P = W ** -1
    ev = mp.eigsy(A, eigvals_only=True)
    cond = max(ev) / min(ev)
    to_np = lambda m_: np.array([[float(m_[i, j]) for j in range(m_.cols)] for i in range(m_.rows)])  # noqa: E731
    return to_np(p).reshape(3), to_np(P), float(cond)


@pytest.fixture(scope="module")
def references():
    return [_mp_reference(*_geometry(g), VAR_Y) for g in GEOMETRIES]


def _ratios(fn, references):
    rp, rP = [], []
    for g, (p_ref, P_ref, cond) in zip(GEOMETRIES, references):
        p, P = fn(*_geometry(g), VAR_Y)
        rp.append(np.linalg.norm(p - p_ref) / (EPS * cond * np.linalg.norm(p_ref)))
        rP.append(np.linalg.norm(P - P_ref) / (EPS * cond ** 2 * np.linalg.norm(P_ref)))
    return np.array(rp), np.array(rP)


def test_triangulation_prior_against_mpmath(references):
    rp, rP = _ratios(cs.triangulation_prior, references)
    print("triangulation_prior: |p - p_ref| / (eps cond |p|) per geometry:", np.round(rp, 3), "max", rp.max())
    print("triangulation_prior: |P - P_ref| / (eps cond^2 |P|) per geometry:", np.round(rP, 3), "max", rP.max())
    assert np.all(rp <= K_P) and np.all(rP <= K_COV)
    for g in GEOMETRIES:
        p, P = cs.triangulation_prior(*_geometry(g), VAR_Y)
        assert P.tobytes() == P.T.copy().tobytes() and np.all(np.linalg.eigvalsh(P) > 0)
        assert np.linalg.norm(p - np.array([g[2][0], g[2][1], g[1]])) < 1e-6 * max(1.0, g[1] ** 2 / g[0])  # the rays do meet at the point
    conds = [r[2] for r in references]
    assert max(conds) > 1e6 and min(conds) < 1e2  # from a wide baseline at arm's length to nearly parallel rays


def test_triangulation_prior_with_the_wrong_sign_of_t21_is_caught(references):
    wrong = lambda y1, y2, q, t, v: cs.triangulation_prior(y1, y2, q, -np.asarray(t), v)  # noqa: E731
    rp, rP = _ratios(wrong, references)
    assert np.all(rp > K_P), rp  # every geometry lands outside the bound


def test_triangulation_prior_parallel_rays_and_covariance_growth():
    y = _unit([0.1, 0.2, 1.0])
    with pytest.raises(ValueError):
        cs.triangulation_prior(y, y, [1.0, 0, 0, 0], [0.1, 0.0, 0.0], VAR_Y)
    # first order: the variance along the ray grows like d^4 / baseline^2
    along = []
    for depth in (5.0, 10.0, 20.0):
        g = (0.1, depth, (0.0, 0.0), (0.0, 0.0, 0.0))
        p, P = cs.triangulation_prior(*_geometry(g), VAR_Y)
        along.append(float(_unit(p) @ P @ _unit(p)))
    assert 12.0 < along[1] / along[0] < 20.0 and 12.0 < along[2] / along[1] < 20.0
