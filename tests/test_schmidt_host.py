"""What the Schmidt (consider) updates need on the host, without a GPU: the binding's two symbols with their argument types (no handle is
created), the partition, the checks, the image and the launch arithmetic of eqf_vio_amd/csrc/eqf_schmidt_host.hpp (standard library only;
csrc/eqf_schmidt.hpp's kernels and the C ABI use the same functions) -- tests/schmidt_host_main.cpp is compiled with g++ under the address
and undefined-behaviour sanitizers and run as a child process, cases on stdin, results on stdout -- and the numpy statement
consistency.schmidt_update_host against the Joseph form with the gain's consider rows zeroed.  Every expected value is computed here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import blocks_cases as bc
from eqf_vio_amd import consistency as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (N, ids of the state in its order, consider ids): the shapes of tests/test_gpu_schmidt.py and the edges
IDS22 = list(range(100, 122))
IDS43 = list(range(100, 143))
SHUFFLED = [7, 3, 19, 11, 5]
PARTITIONS = {
    "empty set": (22, IDS22, []),
    "all landmarks": (22, IDS22, IDS22),
    "all but 3 and 20": (22, IDS22, [i for k, i in enumerate(IDS22) if k not in (3, 20)]),
    "every second of 43": (43, IDS43, IDS43[1::2]),
    "ids not in the state": (22, IDS22, [1, 2, 103, 110, 5000, 6000]),
    "only ids not in the state": (5, SHUFFLED, [1, 2, 4, 6, 20]),
    "state in another order": (5, SHUFFLED, [3, 7, 11]),
    "N = 0": (0, [], [4, 5]),
    "N = 0, empty": (0, [], []),
    "ragged 5": (5, list(range(100, 105)), [101, 104]),
}


def test_binding_exports_both_symbols_with_their_argument_types():
    from eqf_vio_amd import binding
    from eqf_vio_amd import filter as vf

    assert "eqf_update_linear_schmidt" in binding.EXPORTED_SYMBOLS and "eqf_update_landmarks_schmidt" in binding.EXPORTED_SYMBOLS
    L = binding.lib()
    dp, ip, up, vp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_ubyte), C.c_void_p
    rp = C.POINTER(binding.LinearReport)
    assert L.eqf_update_linear_schmidt.argtypes == [vp, C.c_int, C.c_int, dp, C.c_int, dp, dp, C.c_double, up, ip, ip, C.c_int, dp, C.c_int, rp]
    assert L.eqf_update_landmarks_schmidt.argtypes == [vp, C.c_int, C.c_int, ip, ip, C.c_int, dp, dp, dp, C.c_double, C.c_double, up, ip, ip,
                                                       C.c_int, up, dp, C.c_int, rp]
    import inspect

    assert "consider" in inspect.signature(binding.FilterBatch.update_linear).parameters
    assert "consider" in inspect.signature(binding.FilterBatch.update_landmarks).parameters
    assert "consider" in inspect.signature(vf.VIOFilter.processLinearMeasurement).parameters
    assert "consider" in inspect.signature(vf.VIOFilter.processLandmarkMeasurements).parameters
    # a NULL handle is refused by the library itself, before anything touches a device
    one, d = (C.c_int * 1)(1), (C.c_double * 9)()
    assert L.eqf_update_linear_schmidt(None, 1, 1, d, 1, d, d, 1.0, None, one, one, 1, None, 0, None) == binding.ERR_INVALID
    assert L.eqf_update_landmarks_schmidt(None, 1, 1, one, one, 1, d, d, d, 1.0, 1.0, None, one, one, 1, None, None, 0, None) == binding.ERR_INVALID
    header = open(os.path.join(ROOT, "include", "eqf_vio_amd.h")).read()
    assert "int eqf_update_linear_schmidt(eqf_filter* f, int local, int m," in header
    assert "int eqf_update_landmarks_schmidt(eqf_filter* f, int local, int rows," in header
    facade = open(os.path.join(ROOT, "eqf_vio_amd", "cpp", "VIOFilter.h")).read()
    assert "eqf_update_linear_schmidt(" in facade and "eqf_update_landmarks_schmidt(" in facade


def test_header_is_host_only_and_compiles_with_plain_gcc(tmp_path):
    path = os.path.join(ROOT, "eqf_vio_amd", "csrc", "eqf_schmidt_host.hpp")
    includes = [ln.split()[1] for ln in open(path) if ln.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "eqf_schmidt_host.hpp"\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.dirname(path), str(tu)], check=True)


@pytest.fixture(scope="module")
def schmidt_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("schmidt_host") / "schmidt_host")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "eqf_vio_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "schmidt_host_main.cpp")], check=True)

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        return [[int(t) for t in ln.split()] for ln in r.stdout.split("\n")[:-1]]

    return run


def _partition(N, ids, cids):
    """(found, active padded indices, flags) by a set computation"""
    cset = set(cids)
    lm = [i for i in range(N) if ids[i] in cset]
    c = {12 + 3 * i + k for i in lm for k in range(3)}
    n = 12 + 3 * N
    return len(lm), [i for i in range(n) if i not in c], [1 if i in c else 0 for i in range(n)]


def _line(cmd, N, ids, cids):
    return " ".join(map(str, [cmd, N, len(cids), *ids, *cids]))


def test_partitions_against_a_set_computation(schmidt_host):
    names = list(PARTITIONS)
    out = schmidt_host("\n".join(_line("active", *PARTITIONS[k]) for k in names))
    assert len(out) == len(names)
    for k, o in zip(names, out):
        N, ids, cids = PARTITIONS[k]
        found, act, fl = _partition(N, ids, cids)
        assert o[0] == found and o[1] == len(act), k
        assert o[2:2 + len(act)] == act and o[2 + len(act):] == fl, k
        assert act[:12] == list(range(12)) and len(act) == 12 + 3 * (N - found)
    # the shapes the GPU tests rely on
    assert len(_partition(*PARTITIONS["all but 3 and 20"])[1]) == 18 and len(_partition(*PARTITIONS["every second of 43"])[1]) == 78
    assert len(_partition(*PARTITIONS["all landmarks"])[1]) == 12


def test_every_entry_outside_c_x_c_has_one_owner_and_none_inside(schmidt_host):
    names = list(PARTITIONS)
    out = schmidt_host("\n".join(_line("own", *PARTITIONS[k]) for k in names))
    for k, o in zip(names, out):
        N, ids, cids = PARTITIONS[k]
        found, act, _ = _partition(N, ids, cids)
        n, nc = 12 + 3 * N, 3 * found
        grid, one, other, inside_owned, inside = o
        assert grid == max(-(-len(act) // 64), 1) * -(-n // 64), k
        assert one == n * n - nc * nc and other == 0 and inside_owned == 0 and inside == nc * nc, (k, o)
    assert schmidt_host("bytes 612 450\nbytes 3012 2850\nbytes 78 0")[0:3] == [[16 * (612 ** 2 - 450 ** 2)], [16 * (3012 ** 2 - 2850 ** 2)], [16 * 78 ** 2]]


def test_image_layout(schmidt_host):
    pitch = 32
    fs = [PARTITIONS["ragged 5"], PARTITIONS["N = 0"], PARTITIONS["state in another order"]]
    out = schmidt_host(f"image 3 {pitch} " + " ".join(_line("", *f).strip() for f in fs))[0]
    assert out[0] == 4 * 2 * 3 + 4 * 3 * pitch + 3 * pitch
    rec = out[1:]
    per = 2 + 2 * pitch
    for b, f in enumerate(fs):
        _, act, fl = _partition(*f)
        r = rec[per * b:per * (b + 1)]
        assert r[0] == len(act) and r[1] == 0
        assert r[2:2 + pitch] == act + [-1] * (pitch - len(act))
        assert r[2 + pitch:] == fl + [0] * (pitch - len(fl))


def test_argument_checks(schmidt_host):
    OK, INVALID, CAPACITY, UNSORTED = 0, -1, -4, -5
    from eqf_vio_amd import binding

    assert (binding.ERR_INVALID, binding.ERR_CAPACITY, binding.ERR_UNSORTED) == (INVALID, CAPACITY, UNSORTED)

    def chk(B, cap, cstride, n, ids, null_n=0, null_ids=0):
        ids = list(ids) + [0] * (B * max(cstride, 0) - len(ids))
        return " ".join(map(str, ["check", B, cap, cstride, null_n, null_ids, *n, *ids]))

    cases = [
        (chk(2, 4, 3, (2, 3), (1, 2, 0, 4, 5, 9)), OK),
        (chk(2, 4, 3, (0, 0), ()), OK),                              # n_consider of 0
        (chk(2, 4, 3, (0, 0), (), null_ids=1), OK),                  # ... needs no list
        (chk(2, 4, 3, (9, 9), (), null_n=1, null_ids=1), OK),        # n_consider == NULL: empty sets
        (chk(1, 4, 4, (4,), (1, 2, 3, 4)), OK),                      # n_consider of capacity
        (chk(1, 4, 5, (5,), (1, 2, 3, 4, 5)), CAPACITY),             # ... and beyond it
        (chk(2, 8, 3, (2, 4), (1, 2, 0, 4, 5, 9)), CAPACITY),        # beyond cstride
        (chk(2, 4, 3, (2, -1), (1, 2, 0, 4, 5, 9)), INVALID),
        (chk(2, 4, -1, (0, 0), ()), INVALID),
        (chk(2, 4, 3, (2, 1), (), null_ids=1), INVALID),
        (chk(2, 4, 3, (2, 3), (1, 2, 0, 4, 9, 5)), UNSORTED),
        (chk(2, 4, 3, (2, 3), (1, 1, 0, 4, 5, 9)), UNSORTED),        # a repeated id
        (chk(2, 4, 3, (2, 2), (1, 2, 0, 4, 9, 5)), OK),              # beyond n_consider[b]: not looked at
        (chk(2, 4, 3, (5, 3), (1, 2, 0, 9, 5, 4)), CAPACITY),        # capacity before order
        (chk(2, 4, 3, (-1, 5), ()), INVALID),                        # invalid before capacity
    ]
    out = schmidt_host("\n".join(c[0] for c in cases))
    assert [o[0] for o in out] == [c[1] for c in cases]


# ---- the numpy statement
def _case(N, seed, m_lm, consider_lm):
    """own Sigma of the CPU oracle, dense rows on m_lm landmarks (3 rows each: well conditioned), the consider landmarks"""
    S = bc.own_sigma_oracle(N)
    S = np.tril(S) + np.tril(S, -1).T
    rng = np.random.default_rng([2701, N, seed])
    n = 11 + 3 * N
    Ht = cs.landmark_blocks_matrix(N, m_lm, rng.standard_normal((len(m_lm), 3, 3)))
    m = Ht.shape[0]
    P = Ht @ S @ Ht.T
    A = rng.standard_normal((m, m))
    R = np.mean(np.diag(P)) * (A @ A.T / m + 0.5 * np.eye(m))
    resid = np.sqrt(np.diag(P + R)) * rng.standard_normal(m)
    return S, Ht, R, resid, cs.consider_indices(consider_lm), n


def _joseph(S, Ht, R, c):
    Rl = np.tril(R) + np.tril(R, -1).T
    K = np.linalg.solve(Ht @ S @ Ht.T + Rl, Ht @ S).T
    K[c] = 0.0
    A = np.eye(len(S)) - K @ Ht
    return A @ S @ A.T + K @ Rl @ K.T, K


CASES = [(22, 0, (1, 3, 7, 20), [i for i in range(22) if i not in (3, 20)]), (43, 1, tuple(range(0, 43, 3)), list(range(0, 43, 2))),
         (22, 2, (0, 5), list(range(22))), (5, 3, (0, 2), [0])]


@pytest.mark.parametrize("case", CASES, ids=[f"N{c[0]}-{c[1]}" for c in CASES])
def test_statement_against_the_joseph_form_with_zeroed_gain_rows(case):
    S, Ht, R, resid, c, n = _case(*case)
    r = cs.schmidt_update_host(S, Ht, R, resid, c)
    J, K = _joseph(S, Ht, R, c)
    rel = np.linalg.norm(r["Sigma"] - J) / np.linalg.norm(J)
    print(f"N={case[0]}: |Sigma+ - Joseph| / |Joseph| = {rel:.2e}")
    assert rel <= 1e-12
    assert np.linalg.eigvalsh(r["Sigma"]).min() > 0.0 and np.array_equal(r["Sigma"], r["Sigma"].T)
    assert np.array_equal(r["Sigma"][np.ix_(c, c)], S[np.ix_(c, c)])
    assert np.array_equal(r["gamma"][c], np.zeros(len(c))) and not np.signbit(r["gamma"][c]).any()
    full = cs.linear_update_host(S, Ht, resid, R)
    a = np.setdiff1d(np.arange(n), c)
    assert np.array_equal(r["gamma"][a], full["gamma"][a]) and np.linalg.norm(r["gamma"] - K @ resid) <= 1e-10 * np.linalg.norm(K @ resid)
    assert r["nis"] == full["nis"] and r["logdet_S"] == full["logdet_S"] and r["loglik"] == full["loglik"] and r["dof"] == full["dof"]
    off = np.ones((n, n), dtype=bool)
    off[np.ix_(c, c)] = False
    assert np.array_equal(r["Sigma"][off], full["Sigma"][off])
    # the measurement observes consider landmarks, and the cross block moves
    assert np.abs(Ht[:, c]).max() > 0 and not np.array_equal(r["Sigma"][np.ix_(a, c)], S[np.ix_(a, c)])


def test_empty_set_is_the_existing_statements_exactly():
    N = 22
    S, Ht, R, resid, _, n = _case(N, 4, (1, 3, 7, 20), [])
    r = cs.schmidt_update_host(S, Ht, R, resid, [])
    full = cs.linear_update_host(S, Ht, resid, R)
    for k in ("Sigma", "gamma"):
        assert r[k].tobytes() == full[k].tobytes(), k
    assert (r["nis"], r["logdet_S"], r["loglik"], r["dof"]) == (full["nis"], full["logdet_S"], full["loglik"], full["dof"])
    # ... and update_landmarks_host's, given the same blocks (its Sigma+ is the lower triangle mirrored)
    idx = np.array([1, 3, 7, 20])
    H = np.stack([Ht[3 * k:3 * k + 3, 11 + 3 * i:14 + 3 * i] for k, i in enumerate(idx)])
    Rb = np.stack([R[3 * k:3 * k + 3, 3 * k:3 * k + 3] for k in range(4)])
    Rd = np.zeros_like(R)
    for k in range(4):
        Rd[3 * k:3 * k + 3, 3 * k:3 * k + 3] = Rb[k]
    u = cs.update_landmarks_host(S, idx, H, resid.reshape(4, 3), Rb)
    r2 = cs.schmidt_update_host(S, Ht, Rd, resid, [])
    assert u["info"] == 0 and np.array_equal(np.tril(u["Sigma"]), np.tril(r2["Sigma"])) and u["gamma"].tobytes() == r2["gamma"].tobytes()
    assert (u["nis"], u["logdet_S"], u["loglik"], u["dof"]) == (r2["nis"], r2["logdet_S"], r2["loglik"], r2["dof"])
    with pytest.raises(ValueError):
        cs.schmidt_update_host(S, Ht, R, resid, [11, 11])


def test_three_injected_faults_are_outside_the_checks():
    """a zeroed cross block, a downdated cc block and an unmasked gamma: each is far outside what the checks above allow"""
    S, Ht, R, resid, c, n = _case(*CASES[0])
    r = cs.schmidt_update_host(S, Ht, R, resid, c)
    J, _ = _joseph(S, Ht, R, c)
    full = cs.linear_update_host(S, Ht, resid, R)
    a = np.setdiff1d(np.arange(n), c)
    zeroed = r["Sigma"].copy()
    zeroed[np.ix_(a, c)] = 0.0
    zeroed[np.ix_(c, a)] = 0.0
    assert np.linalg.norm(zeroed - J) / np.linalg.norm(J) > 1e-6
    assert np.linalg.norm(full["Sigma"] - J) / np.linalg.norm(J) > 1e-6        # the cc block downdated too: the full update
    assert not np.array_equal(full["Sigma"][np.ix_(c, c)], S[np.ix_(c, c)])
    assert np.abs(full["gamma"][c]).min() > 0.0                                # the unmasked gamma is nowhere zero on c
