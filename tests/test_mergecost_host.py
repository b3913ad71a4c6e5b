"""What the pairwise merge costs need on the host, without a GPU: the binding's symbol with its argument types (no handle is created), the
numpy statement on an example worked by hand, and the argument checks, pair canonicalisation, lexicographic enumeration, chunk plan and
cost formulas of eqf_vio_amd/csrc/eqf_mergecost_host.hpp (host only, standard library only) -- tests/mergecost_host_main.cpp is compiled
with g++ under the address and undefined-behaviour sanitizers and run as a child process, cases on stdin, results on stdout.  Every
expected value is computed here."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_binding_exports_the_symbol_with_its_argument_types():
    from eqf_vio_amd import binding

    L = binding.lib()
    dp, ip, vp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p
    assert "eqf_get_merge_costs" in binding.EXPORTED_SYMBOLS
    assert L.eqf_get_merge_costs.argtypes == [vp, C.c_int, ip, dp, C.c_int, C.c_int, C.c_int, C.c_int, ip, C.POINTER(binding.PairCost),
                                              C.POINTER(binding.SigmaStats)]
    assert C.sizeof(binding.PairCost) == 32
    assert [f[0] for f in binding.PairCost._fields_] == ["cost", "logdet_pair", "maha", "info", "pad_"]
    assert binding.COST_KINDS == {"runnalls": 0, "bhattacharyya": 1}
    assert callable(binding.FilterBatch.merge_costs) and callable(binding.FilterBatch.reduce_mixture)
    # a NULL handle is refused by the library itself, before anything touches a device
    assert L.eqf_get_merge_costs(None, 1, None, None, 0, 0, 0, 0, None, None, None) == binding.ERR_INVALID


@pytest.fixture(scope="module")
def mergecost_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mergecost_host") / "mergecost_host")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "eqf_vio_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "mergecost_host_main.cpp")], check=True)

    def run(text):
        r = subprocess.run([exe], input=text + "\n", capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        return [ln.split() for ln in r.stdout.split("\n")[:-1]]

    return run


def test_header_is_host_only_and_compiles_with_plain_gcc(tmp_path):
    path = os.path.join(ROOT, "eqf_vio_amd", "csrc", "eqf_mergecost_host.hpp")
    includes = [ln.split()[1] for ln in open(path) if ln.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "eqf_mergecost_host.hpp"\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.dirname(path), str(tu)], check=True)


def test_argument_checks(mergecost_host):
    cases = [("3 0 0 3 1", 1), ("3 1 6 3 1", 1), ("3 0 11 2 1", 1),           # all pairs, or the first of them
             ("3 0 0 4 1", 0),                                                  # more than all pairs without a list
             ("3 2 0 3 1", 0), ("3 -1 0 3 1", 0),                               # kind
             ("3 0 5 3 1", 0), ("3 0 12 3 1", 0), ("3 0 -1 3 1", 0),            # first
             ("3 0 0 -1 1", 0),                                                 # npairs < 0
             ("0 0 0 0 1", 0),                                                  # n < 1
             ("1 0 0 0 1", 1), ("1 0 0 0 0", 1),                                # n = 1: no pairs, the member record alone
             ("1 0 0 1 1", 0),
             ("3 0 0 2 0 0 1 2 0", 1), ("3 0 0 2 0 1 1 2 2", 1),                # a named pair may be (j, i) or (i, i)
             ("3 0 0 2 0 0 1 2 3", 0), ("3 0 0 2 0 0 -1 2 1", 0),               # a position out of range
             ("3 0 0 5 0 0 1 0 1 0 1 0 1 0 1", 1)]                              # a list may repeat and be longer than all pairs
    got = mergecost_host("\n".join("args " + c for c, _ in cases))
    assert [int(g[0]) for g in got] == [w for _, w in cases], [(c, g) for (c, w), g in zip(cases, got) if int(g[0]) != w]
    got = mergecost_host("\n".join(f"option {v}" for v in (0, 1, 4096, 4097, -1)))
    assert [int(g[0]) for g in got] == [0, 1, 1, 0, 0]


def test_enumeration_items_and_distinct(mergecost_host):
    for n in (1, 2, 3, 7):
        want = [(i, j) for i in range(n) for j in range(i + 1, n)]
        got = mergecost_host(f"lex {n}")[0] if n > 1 else []
        assert [(int(got[2 * k]), int(got[2 * k + 1])) for k in range(len(want))] == want and len(got) == 2 * len(want)
    # repeated indices, a weight of 0, pairs named both ways round and a pair of one position with itself
    idx, wt = [4, 1, 4, 0], [0.5, 0.0, 0.25, 0.25]
    pairs = [(2, 0), (1, 3), (3, 3), (0, 1)]
    for kind in (0, 1):
        for null in (1, 0):
            pp = [(i, j) for i in range(4) for j in range(i + 1, 4)] if null else pairs
            line = f"items 4 {kind} {len(pp)} {null} " + " ".join(map(str, idx)) + " " + " ".join(float(x).hex() for x in wt)
            if not null:
                line += " " + " ".join(f"{a} {b}" for a, b in pp)
            t = mergecost_host(line)[0]
            assert len(t) == 8 * (4 + len(pp))
            rec = [t[8 * k:8 * k + 8] for k in range(4 + len(pp))]
            for k in range(4):   # the members first, by position, as self images
                assert [int(x) for x in rec[k][:5]] == [k, k, idx[k], idx[k], 1]
            for k, (a, b) in enumerate(pp):
                i, j = min(a, b), max(a, b)
                r = rec[4 + k]
                assert [int(x) for x in r[:5]] == [i, j, idx[i], idx[j], 0]
                alpha = 0.5 if (kind == 1 or not wt[i] + wt[j] > 0.0) else wt[j] / (wt[i] + wt[j])
                assert [float.fromhex(x) for x in r[5:]] == [alpha, wt[i], wt[j]]
    assert [int(x) for x in mergecost_host("distinct 6 7 4 1 4 0 1 5 4")[0]] == [4, 1, 0, 5]
    # both weights 0: alpha is one half, not 0 / 0
    t = mergecost_host("items 2 0 1 1 0 1 0x0p+0 0x0p+0")[0]
    assert float.fromhex(t[16 + 5]) == 0.5


def test_chunk_plan_and_launch_count(mergecost_host):
    for items, option, B in ((10, 0, 5), (10, 3, 5), (10, 4, 5), (1, 1, 64), (0, 0, 4), (2016, 0, 64), (7, 4096, 2), (6, 3, 9), (6, 4, 9)):
        got = [int(x) for x in mergecost_host(f"plan {items} {option} {B}")[0]]
        chunk = option if option > 0 else B
        counts = [min(chunk, items - c * chunk) for c in range(-(-items // chunk))]
        assert got == [chunk, len(counts)] + counts and sum(counts) == items
    for N, first, m in ((0, 0, 12), (1, 0, 15), (17, 0, 63), (18, 0, 66), (39, 0, 129), (82, 0, 258), (0, 11, 0), (17, 6, 57), (18, 11, 54)):
        off = 12 if first == 11 else first
        nb = -(-m // 64)
        launches = 4 + sum((1 if K > 0 else 0) + 1 + (1 if nb - K - 1 > 0 else 0) for K in range(nb))
        assert [int(x) for x in mergecost_host(f"order {N} {first}")[0]] == [off, m, nb, launches]


def _parts_ascend_without_overlap(offs, sizes, total):
    """Parts [off, off + size) in the order given: ascending, none overlapping the next, the last within the total."""
    ends = [o + s for o, s in zip(offs, sizes)]
    return offs[0] == 0 and all(e <= o for e, o in zip(ends, offs[1:])) and all(a < b or s == 0 for a, b, s in zip(offs, offs[1:], sizes)) \
        and ends[-1] <= total


def test_workspace_and_item_block_layouts(mergecost_host):
    """W | E | D | out | Glob | bad, in doubles, against the formula written out; the total is what the call has always allocated:
    C (sigmaStride + nTot + dRec + head + glob) + (C + 1) // 2 doubles."""
    head, dRec = 20, 5120
    cases = [(C, cap, glob) for C in (1, 2, 3, 8) for cap in (1, 5, 21, 200) for glob in (30, 41)]
    lines = []
    for C, cap, glob in cases:
        nTot = 12 + 3 * cap
        lines.append(f"work {C} {nTot * (-(-nTot // 16) * 16)} {nTot} {dRec} {head} {glob}")
    for (C, cap, glob), got in zip(cases, mergecost_host("\n".join(lines))):
        got = [int(x) for x in got]
        nTot = 12 + 3 * cap
        stride = nTot * (-(-nTot // 16) * 16)
        sizes = [C * stride, C * nTot, C * dRec, C * head, C * glob]
        want, at = [], 0
        for s in sizes:
            want.append(at)
            at += s
        want.append(at)  # (the int tail starts behind the Globs)
        total = C * (stride + nTot + dRec + head + glob) + (C + 1) // 2
        assert got == want + [total], (C, cap, glob)
        offs, tail_bytes = got[:6], 4 * C
        assert _parts_ascend_without_overlap([8 * o for o in offs], [8 * s for s in sizes] + [tail_bytes], 8 * total)
        assert (8 * offs[4]) % 8 == 0 and (8 * offs[5]) % 4 == 0
        assert 8 * (total - offs[5]) >= tail_bytes  # (C ints fit, C odd or even)
    for cap in (0, 1, 7, 2016):
        offI, offR, nbytes, item = [int(x) for x in mergecost_host(f"itemblock {cap}")[0]]
        assert item == 6 * 4 + 3 * 8  # (six ints and three doubles: the device's PairItem)
        assert [offI, offR, nbytes] == [0, item * cap, cap * (item + 8 * 8)] and offR % 8 == 0


def test_cost_formulas(mergecost_host):
    rng = np.random.default_rng(5)
    lines, want = [], []
    for k in range(40):
        ldi, ldj = rng.normal(0, 30, 2)
        ldij = max(ldi, ldj) + rng.uniform(0, 5)
        maha = rng.uniform(0, 50) if k % 5 else 0.0
        wi, wj = rng.uniform(0, 1, 2)
        if k == 7:
            wi = 0.0
        if k == 8:
            wi = wj = 0.0
        for kind in (0, 1):
            lines.append("cost %d %s" % (kind, " ".join(float(x).hex() for x in (ldi, ldj, ldij, maha, wi, wj))))
            a = 0.5 if (kind == 1 or not wi + wj > 0.0) else wj / (wi + wj)
            if kind == 0:
                c = 0.5 * (wi * (ldij - ldi) + wj * (ldij - ldj) + (wi + wj) * math.log1p(a * (1.0 - a) * maha))
            else:
                c = 0.125 * maha + 0.25 * ((ldij - ldi) + (ldij - ldj))
            want.append((a, c))
    got = mergecost_host("\n".join(lines))
    for g, (a, c) in zip(got, want):
        assert float.fromhex(g[0]) == a
        assert abs(float.fromhex(g[1]) - c) <= 4 * np.finfo(float).eps * max(abs(c), 1.0)  # (a compiler may fuse a multiply-add)
    # identical members: exactly 0, whatever the weights
    for kind in (0, 1):
        g = mergecost_host("cost %d %s" % (kind, " ".join(float(x).hex() for x in (-12.5, -12.5, -12.5, 0.0, 0.3, 0.2))))[0]
        assert float.fromhex(g[1]) == 0.0


def test_numpy_statement_worked_by_hand():
    """Identity attitude and group (J = I; the gravity block multiplies zeros), two members at +-d in velocity with Sigma = s I: SigmaBar =
    ((1 - alpha) s_1 + alpha s_2) I on the 9 coordinates that carry variance, d = 2 d_v."""
    from eqf_vio_amd import consistency as cs

    q = np.array([np.cos(0.25), np.sin(0.25), 0.0, 0.0])
    group = dict(Aq=np.array([1.0, 0, 0, 0]), Ax=np.zeros(3), w=np.zeros(3), Qq=np.zeros((0, 4)), Qa=np.zeros(0))
    dv = np.array([0.25, -0.5, 0.125])

    def member(v, s):
        est = dict(q=q, x=np.zeros(3), v=v, p=np.zeros((0, 3)))
        return dict(estimate=est, bias=np.zeros(6), origin=dict(est), group=group, sigma=s * np.eye(11))

    ms = [member(dv, 2.0), member(-dv, 8.0), member(dv, 2.0)]
    w = [1.0, 3.0, 4.0]
    r = cs.merge_costs_host(ms, w, 1, "runnalls")  # (centre: member 1, so that members 0 and 2 go through the same chart transition)
    wt = np.array(w) / 8.0
    a = wt[1] / (wt[0] + wt[1])
    sbar = 2.0 + a * 6.0
    maha = 4 * float(dv @ dv) / sbar
    cost = 0.5 * (wt[0] * 11 * math.log(sbar / 2.0) + wt[1] * 11 * math.log(sbar / 8.0) + (wt[0] + wt[1]) * math.log1p(a * (1 - a) * maha))
    assert [tuple(p) for p in r["pairs"]] == [(0, 1), (0, 2), (1, 2)]
    assert abs(r["cost"][0] - cost) < 1e-13 and abs(r["maha"][0] - maha) < 1e-13 and abs(r["logdet_pair"][0] - r["member_logdet"][0] - 11 * math.log(sbar / 2.0)) < 1e-13
    assert r["cost"][1] == 0.0 and r["maha"][1] == 0.0 and r["logdet_pair"][1] == r["member_logdet"][0]  # identical members
    assert np.array_equal(r["matrix"], r["matrix"].T) and np.all(np.diag(r["matrix"]) == 0.0) and r["matrix"][0, 1] == r["cost"][0]
    b = cs.merge_costs_host(ms, w, 1, "bhattacharyya", pairs=[(1, 0)])
    assert abs(b["cost"][0] - (0.125 * 4 * float(dv @ dv) / 5.0 + 0.25 * 11 * (2 * math.log(5.0) - math.log(2.0) - math.log(8.0)))) < 1e-13
    # the greedy reduction merges the two equal members first, into the centre's slot (the heaviest: member 2, whose chart transition is
    # the identity by definition while member 0's is computed: a cost of a rounding, not exactly 0), then stops at the threshold
    alive, wk, left, log = cs.reduce_mixture_host(ms, w, 1, max_cost=1e-9)
    assert alive == [1, 2] and len(log) == 1 and log[0][0] == (2, 0) and abs(log[0][1]) < 1e-25 and list(wk) == [0.375, 0.625]
    assert len(left) == 2 and left[0] is ms[1] and np.allclose(left[1]["estimate"]["v"], dv, atol=1e-15)
