"""What the host decides in eqf_edit_landmarks (eqf_vio_amd/csrc/eqf_mapedit_host.hpp: host only, standard library only) without a GPU and
without loading anything into Python: tests/mapedit_host_main.cpp is compiled with g++ under the address and undefined-behaviour
sanitizers and run as a child process, cases on stdin, results on stdout.  Every expected value is computed here, with sets and numpy --
never by the header."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, CAPACITY, UNSORTED = 0, -1, -4, -5
NAN = float("nan")
EYE = np.eye(3)


@pytest.fixture(scope="module")
def mapedit_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mapedit_host") / "mapedit_host")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "eqf_vio_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "mapedit_host_main.cpp")], check=True)

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        return [ln.split() for ln in r.stdout.split("\n")[:-1]]

    return run


def test_header_is_host_only_and_compiles_with_plain_gcc(tmp_path):
    path = os.path.join(ROOT, "eqf_vio_amd", "csrc", "eqf_mapedit_host.hpp")
    includes = [ln.split()[1] for ln in open(path) if ln.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "eqf_mapedit_host.hpp"\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.dirname(path), str(tu)], check=True)


# ---- a case: cap, per filter (state ids, remove ids, [(insert id, p, P), ...]); strides default to the longest list
def spd(seed):
    r = np.random.default_rng(seed)
    a = r.standard_normal((3, 3))
    return a @ a.T + 0.5 * EYE


def ins(i, seed=None, p=None, P=None):
    s = i if seed is None else seed
    return (i, np.array([0.3 * s + 0.1, -0.2 * s, 1.0 + s]) if p is None else np.asarray(p, dtype=float),
            spd(s) if P is None else np.asarray(P, dtype=float))


ZERO_PIVOT = np.array([[1.0, 0, 0], [1.0, 1.0, 0], [0, 0, 1.0]])        # second pivot 1 - 1 = 0
NEG_PIVOT = np.array([[1.0, 0, 0], [0, 1.0, 0], [2.0, 0, 3.0]])         # third pivot 3 - 4 < 0
NEG_FIRST = np.array([[-1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]])
NAN_LOWER = np.array([[1.0, 0, 0], [NAN, 1.0, 0], [0, 0, 1.0]])
NAN_UPPER = np.array([[1.0, NAN, NAN], [0.25, 1.0, NAN], [0.125, 0.0625, 1.0]])  # only where nothing is read: accepted
INF_DIAG = np.array([[float("inf"), 0, 0], [0, 1.0, 0], [0, 0, 1.0]])

CASES = {
    "empty state, nothing to do": (4, [([], [], [])]),
    "empty state, two come in": (4, [([], [], [ins(3), ins(9)])]),
    "remove all": (4, [([7, 3, 9], [3, 7, 9], [])]),
    "remove none": (4, [([7, 3, 9], [], [])]),
    "ids not in the state": (6, [([7, 3, 9], [1, 4, 8, 10], [])]),
    "some in, some not": (6, [([7, 3, 9, 12], [3, 4, 12], [])]),
    "replace: an id in both lists": (6, [([7, 3, 9], [3], [ins(3)])]),
    "replace and already present": (6, [([7, 3, 9], [3], [ins(3), ins(7), ins(8)])]),
    "state order not ascending": (8, [([12, 2, 30, 5, 9], [5, 12], [ins(1), ins(40)])]),
    "fill to capacity exactly": (5, [([4, 1], [], [ins(2), ins(3), ins(5)])]),
    "fill to capacity through a removal": (3, [([4, 1, 6], [1], [ins(2)])]),
    "a rejected entry between accepted ones": (8, [([4], [], [ins(1), ins(2, P=NEG_PIVOT), ins(3)])]),
    "capacity holds because of a rejected entry": (3, [([4], [], [ins(1), ins(2, P=ZERO_PIVOT), ins(3), ins(4, P=NEG_FIRST)])]),
    "three filters, the middle one idle": (6, [([1, 2, 3], [2], [ins(9)]), ([5, 6], [], []), ([9, 4], [4, 9], [ins(4), ins(11)])]),
    "three filters, nobody removes": (6, [([1, 2, 3], [8], [ins(9)]), ([5, 6], [], []), ([], [], [ins(4), ins(11), ins(12)])]),
    "zero pivot": (4, [([1], [], [ins(2, P=ZERO_PIVOT)])]),
    "negative pivot": (4, [([1], [], [ins(2, P=NEG_PIVOT)])]),
    "negative first pivot": (4, [([1], [], [ins(2, P=NEG_FIRST)])]),
    "NaN in the lower triangle": (4, [([1], [], [ins(2, P=NAN_LOWER)])]),
    "NaN only in the unread upper triangle": (4, [([1], [], [ins(2, P=NAN_UPPER)])]),
    "infinite variance": (4, [([1], [], [ins(2, P=INF_DIAG)])]),
    "NaN position": (4, [([1], [], [ins(2, p=[0.0, NAN, 1.0]), ins(3)])]),
    "zero position": (4, [([1], [], [ins(2, p=[0.0, 0.0, 0.0]), ins(3, p=[0.0, 0.0, -1e-300])])]),
    "present id with bad values is verdict 0": (4, [([1, 2], [], [ins(2, P=NAN_LOWER)])]),
}
ERRORS = {
    "one over capacity, only accepted entries count": (3, [([4], [], [ins(1), ins(2, P=ZERO_PIVOT), ins(3), ins(5)])], CAPACITY),
    "over capacity in the last filter": (2, [([1], [], []), ([1, 2], [], [ins(3)])], CAPACITY),
    "unsorted removals": (6, [([1, 2, 3], [3, 2], [])], UNSORTED),
    "duplicate removals": (6, [([1, 2, 3], [2, 2], [])], UNSORTED),
    "unsorted insertions": (6, [([1], [], [ins(5), ins(4)])], UNSORTED),
    "duplicate insertions in the second filter": (6, [([1], [], []), ([1], [], [ins(4), ins(4)])], UNSORTED),
}


def case_text(cap, fl, rs=None, istr=None, nullmask=0, counts=None):
    rs = max([len(f[1]) for f in fl] + [0]) if rs is None else rs
    istr = max([len(f[2]) for f in fl] + [0]) if istr is None else istr
    out = [f"{len(fl)} {cap} {rs} {istr} {nullmask}"]
    for b, (ids, rem, insl) in enumerate(fl):
        nr, ni = counts[b] if counts else (len(rem), len(insl))
        rid = (list(rem) + [-77] * (rs - len(rem)))[:max(rs, 0)]
        iid = ([i[0] for i in insl] + [-77] * (istr - len(insl)))[:max(istr, 0)]
        p = np.full((max(istr, 0), 3), NAN)   # (what lies beyond the count is never read: NaN there must not matter)
        P = np.full((max(istr, 0), 3, 3), NAN)
        for k, (_, pk, Pk) in enumerate(insl[:max(istr, 0)]):
            p[k], P[k] = pk, Pk
        nums = [len(ids)] + list(ids) + [nr] + rid + [ni] + iid
        out.append(" ".join(str(int(x)) for x in nums) + " " + " ".join(float(x).hex() if np.isfinite(x) else repr(float(x)) for x in
                                                                      list(p.reshape(-1)) + list(P.reshape(-1))))
    return " ".join(out), rs, istr


def prior_ok(p, P):
    """The issue's rule, stated with numpy: finite p and lower triangle, p != 0, positive pivots of the 3 x 3 Cholesky."""
    low = P[np.tril_indices(3)]
    if not (np.all(np.isfinite(p)) and np.all(np.isfinite(low))) or not np.any(p != 0.0):
        return False
    S = np.tril(P) + np.tril(P, -1).T
    d0 = S[0, 0]
    if not d0 > 0:
        return False
    l10, l20 = S[1, 0] / np.sqrt(d0), S[2, 0] / np.sqrt(d0)
    d1 = S[1, 1] - l10 * l10
    if not d1 > 0:
        return False
    l21 = (S[2, 1] - l20 * l10) / np.sqrt(d1)
    return bool(S[2, 2] - l20 * l20 - l21 * l21 > 0)


def expected(cap, fl, rs, istr):
    out = dict(removed=[], inserted=[], keep=[], accepted=[], new_ids=[], priors=[])
    for ids, rem, insl in fl:
        gone = set(rem) & set(ids)
        out["removed"].append([int(r in gone) for r in rem] + [0] * (rs - len(rem)))
        keep = [i for i, x in enumerate(ids) if x not in gone]
        left = {ids[i] for i in keep}
        verdict = [0 if i in left else (1 if prior_ok(p, P) else 2) for i, p, P in insl]
        acc = [k for k, v in enumerate(verdict) if v == 1]
        out["inserted"].append(verdict + [0] * (istr - len(insl)))
        out["keep"].append(keep)
        out["accepted"].append(acc)
        out["new_ids"].append([ids[i] for i in keep] + [insl[k][0] for k in acc])
        out["priors"].append([np.concatenate([insl[k][1], (np.tril(insl[k][2]) + np.tril(insl[k][2], -1).T).reshape(-1)]) for k in acc])
    out["any_removed"] = any(len(k) != len(f[0]) for k, f in zip(out["keep"], fl))
    out["any_inserted"] = any(out["accepted"])
    out["max_new"] = max(len(a) for a in out["accepted"])
    out["max_n"] = max(len(n) for n in out["new_ids"])
    assert out["max_n"] <= cap
    return out


def ints(line):
    return [int(t) for t in line]


def check_ok_case(out, name, cap, fl, rs, istr):
    ex = expected(cap, fl, rs, istr)
    assert ints(next(out)) == [OK], name
    assert ints(next(out)) == [int(ex["any_removed"]), int(ex["any_inserted"]), ex["max_new"], ex["max_n"]], name
    for b in range(len(fl)):
        assert ints(next(out)) == ex["removed"][b], name
        assert ints(next(out)) == ex["inserted"][b], name
        assert ints(next(out)) == ex["keep"][b], name
        assert ints(next(out)) == ex["accepted"][b], name
        assert ints(next(out)) == ex["new_ids"][b], name
    ns = max(1, ex["max_new"])
    assert ints(next(out)) == [ns, int(ex["any_removed"]), 1], name
    for b, (ids, _, _) in enumerate(fl):
        assert ints(next(out)) == [len(ex["keep"][b]), len(ex["accepted"][b]), len(ids), 0], name
        if ex["any_removed"]:
            assert ints(next(out)) == ex["keep"][b] + [-1] * (cap - len(ex["keep"][b])), name
        got = np.array([float.fromhex(t) for t in next(out)])
        want = np.zeros(ns * 12)
        for j, v in enumerate(ex["priors"][b]):
            want[12 * j:12 * j + 12] = v
        assert got.tobytes() == want.tobytes(), name
    return ex


def test_verdicts_keep_maps_id_lists_and_image(mapedit_host):
    texts = {n: case_text(cap, fl) for n, (cap, fl) in CASES.items()}
    out = iter(mapedit_host("\n".join(t[0] for t in texts.values())))
    seen = {}
    for name, (cap, fl) in CASES.items():
        seen[name] = check_ok_case(out, name, cap, fl, texts[name][1], texts[name][2])
    assert next(out, None) is None
    # the cases are what their names say
    assert seen["remove all"]["new_ids"] == [[]] and seen["remove all"]["any_removed"]
    assert not seen["ids not in the state"]["any_removed"] and not seen["three filters, nobody removes"]["any_removed"]
    assert seen["replace: an id in both lists"]["new_ids"] == [[7, 9, 3]]
    assert seen["replace and already present"]["inserted"] == [[1, 0, 1]]
    assert seen["state order not ascending"]["new_ids"] == [[2, 30, 9, 1, 40]]
    assert len(seen["fill to capacity exactly"]["new_ids"][0]) == 5 and len(seen["fill to capacity through a removal"]["new_ids"][0]) == 3
    assert seen["a rejected entry between accepted ones"]["inserted"] == [[1, 2, 1]]
    assert seen["capacity holds because of a rejected entry"]["inserted"] == [[1, 2, 1, 0]]
    assert seen["three filters, the middle one idle"]["new_ids"] == [[1, 3, 9], [5, 6], [4, 11]]
    for n in ("zero pivot", "negative pivot", "negative first pivot", "NaN in the lower triangle", "infinite variance"):
        assert seen[n]["inserted"] == [[2]] and not seen[n]["any_inserted"], n
    assert seen["NaN only in the unread upper triangle"]["inserted"] == [[1]]
    assert seen["NaN position"]["inserted"] == [[2, 1]] and seen["zero position"]["inserted"] == [[2, 1]]
    assert seen["present id with bad values is verdict 0"]["inserted"] == [[0]]


def test_errors_before_any_effect(mapedit_host):
    lines = [case_text(cap, fl)[0] for cap, fl, _ in ERRORS.values()]
    fl = [([1, 2, 3], [2], [ins(9)]), ([5], [5], [ins(6)])]
    bad = {
        "remove count beyond the stride": (dict(counts=[(1, 1), (2, 1)]), INVALID),
        "negative insert count": (dict(counts=[(1, -1), (1, 1)]), INVALID),
        "negative stride": (dict(rs=-1, counts=[(0, 1), (0, 1)]), INVALID),
        "remove list NULL with a count": (dict(nullmask=2), INVALID),
        "insert list NULL with a count": (dict(nullmask=8), INVALID),
        "p NULL with a count": (dict(nullmask=16), INVALID),
        "P NULL with a count": (dict(nullmask=32), INVALID),
    }
    lines += [case_text(6, fl, **kw)[0] for kw, _ in bad.values()]
    out = mapedit_host("\n".join(lines))
    assert [ints(ln) for ln in out] == [[rc] for _, _, rc in ERRORS.values()] + [[rc] for _, rc in bad.values()]
    # an invalid count wins over an unsorted list, an unsorted list over the capacity (the checks run in that order over the whole batch)
    both = [([1, 2], [2, 1], []), ([1], [], [])]
    got = mapedit_host("\n".join([case_text(2, both, counts=[(2, 0), (5, 0)])[0],
                                  case_text(2, [([1, 2], [], [ins(5), ins(4)])])[0]]))
    assert [ints(ln) for ln in got] == [[INVALID], [UNSORTED]]


def test_null_arrays_mean_nothing_to_do(mapedit_host):
    """A NULL count array switches its half of the call off, whatever the lists hold; NULL lists with zero counts are fine."""
    fl = [([1, 2, 3], [2], [ins(9)]), ([5], [5], [ins(6)])]
    only_insert = [(ids, [], insl) for ids, _, insl in fl]
    only_remove = [(ids, rem, []) for ids, rem, _ in fl]
    idle = [(ids, [], []) for ids, _, _ in fl]
    texts = [case_text(6, fl, nullmask=1)[0], case_text(6, fl, nullmask=4)[0], case_text(6, idle, nullmask=2 | 8 | 16 | 32)[0],
             case_text(6, fl, nullmask=1 | 2 | 4 | 8 | 16 | 32)[0]]
    out = iter(mapedit_host("\n".join(texts)))
    check_ok_case(out, "n_remove NULL", 6, only_insert, 1, 1)
    # (the removed / inserted rows keep the strides of the call)
    check_ok_case(out, "n_insert NULL", 6, only_remove, 1, 1)
    check_ok_case(out, "NULL lists, zero counts", 6, idle, 0, 0)
    check_ok_case(out, "everything NULL", 6, idle, 1, 1)
    assert next(out, None) is None


def test_large_state_past_any_list_bound(mapedit_host):
    """1030 landmarks in descending order, every third removed, five inserted: nothing in the plan knows a bound on N."""
    ids = list(range(2060, 0, -2))
    fl = [(ids, sorted(ids[::3]), [ins(1), ins(3), ins(5, P=NEG_PIVOT), ins(7), ins(2060)])]
    text, rs, istr = case_text(1030, fl)
    out = iter(mapedit_host(text))
    ex = check_ok_case(out, "large", 1030, fl, rs, istr)
    assert len(ex["keep"][0]) == 1030 - 344 and ex["inserted"] == [[1, 1, 2, 1, 1]]
