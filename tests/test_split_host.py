"""What eqf_split_filters decides on the host, without a GPU: eqf_vio_amd/csrc/eqf_split_host.hpp (host only, standard library only) --
tests/split_host_main.cpp is compiled with g++ under the address and undefined-behaviour sanitizers and run as a child process, cases on
stdin, results on stdout -- and the binding's symbol with its argument types (no handle is created).  Every expected value is computed
here."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID = 0, -1


@pytest.fixture(scope="module")
def split_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("split_host") / "split_host")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "eqf_vio_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "split_host_main.cpp")], check=True)

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        return [[int(t) for t in ln.split()] for ln in r.stdout.split("\n")[:-1]]

    return run


def test_header_is_host_only_and_compiles_with_plain_gcc(tmp_path):
    path = os.path.join(ROOT, "eqf_vio_amd", "csrc", "eqf_split_host.hpp")
    includes = [ln.split()[1] for ln in open(path) if ln.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "eqf_split_host.hpp"\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.dirname(path), str(tu)], check=True)


def test_binding_exports_the_symbol_with_its_argument_types():
    from eqf_vio_amd import binding

    assert "eqf_split_filters" in binding.EXPORTED_SYMBOLS
    L = binding.lib()
    dp, ip, vp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p
    assert L.eqf_split_filters.argtypes == [vp, C.c_int, dp, C.c_int, C.c_int, ip, ip, dp, dp, dp, C.c_int, C.POINTER(binding.SplitReport)]
    assert [f[0] for f in binding.SplitReport._fields_] == ["S", "info"] and C.sizeof(binding.SplitReport) == 16
    assert callable(binding.FilterBatch.split_filters)
    # a NULL handle is refused by the library itself, before anything touches a device
    assert L.eqf_split_filters(None, 0, None, 0, 0, None, None, None, None, None, 0, None) == binding.ERR_INVALID


def _head(B, dst, src, local=1, a=1, n=None, bad=(0, 0, 0)):
    n = len(dst) if n is None else n
    return f"head {B} {local} {a} {n} " + " ".join(map(str, list(dst) + list(src))) + " " + " ".join(map(str, bad))


def test_head_checks(split_host):
    cases = [
        (_head(4, [0, 1, 2], [0, 0, 0]), OK),                       # fan-out with the child in place
        (_head(4, [1, 2, 3], [0, 0, 0]), OK),                       # fan-out, the parent's slot not named
        (_head(4, [0, 1, 2, 3], [0, 0, 2, 2]), OK),                 # two sources, each with its child in place
        (_head(4, [], [], n=0), OK),                                # n = 0
        (_head(4, [], [], n=0, a=0), OK),                           # ... whatever the pointers are
        (_head(4, [], [], n=-1), INVALID),
        (_head(4, [0, 1], [0, 0], local=2), INVALID),
        (_head(4, [0, 1], [0, 0], local=-1), INVALID),
        (_head(4, [0, 1], [0, 0], a=0), INVALID),                   # NULL a
        (_head(4, [0, 1], [0, 0], bad=(0, 0, 2)), INVALID),         # NULL dst_idx
        (_head(4, [0, 1], [0, 0], bad=(0, 0, 3)), INVALID),         # NULL src_idx
        (_head(4, [0, 1], [0, 0], bad=(0, 0, 4)), INVALID),         # NULL shift
        (_head(4, [0, 1], [0, 0], bad=(0, 0, 5)), INVALID),         # NULL shrink
        (_head(4, [0, 4], [0, 0]), INVALID),                        # dst out of range
        (_head(4, [0, -1], [0, 0]), INVALID),
        (_head(4, [0, 1], [0, 4]), INVALID),                        # src out of range
        (_head(4, [0, 1], [0, -1]), INVALID),
        (_head(4, [1, 1], [0, 0]), INVALID),                        # a repeated dst
        (_head(4, [0, 0], [0, 1]), INVALID),
        (_head(4, [1, 0], [0, 1]), INVALID),                        # a swap: a dst that is another child's source
        (_head(4, [1, 2], [0, 1]), INVALID),                        # a shift through other sources
        (_head(4, [0, 1, 2], [0, 0, 1]), INVALID),                  # filter 1 is a dst and the source of 2
        (_head(4, [0, 1], [0, 0], bad=(1, 1, 0)), INVALID),         # shift NaN
        (_head(4, [0, 1], [0, 0], bad=(0, 2, 0)), INVALID),         # shift Inf
        (_head(4, [0, 1], [0, 0], bad=(1, 1, 1)), INVALID),         # shrink NaN
        (_head(4, [0, 1], [0, 0], bad=(1, 2, 1)), INVALID),         # shrink Inf
        (_head(4, [0, 1], [0, 0], bad=(0, 3, 1)), INVALID),         # shrink < 0
        (_head(4, [0, 1], [0, 0], bad=(1, 4, 1)), INVALID),         # shrink > 1
        (_head(4, [0, 1], [0, 0], bad=(1, 3, 0)), OK),              # a negative shift is a shift
    ]
    got = split_host("\n".join(c for c, _ in cases))
    assert [g[0] for g in got] == [w for _, w in cases], [(c, g[0], w) for (c, w), g in zip(cases, got) if g[0] != w]


def test_row_checks(split_host):
    # B lda ldg n src[n] N[B] bad_b bad_i kind; filters hold 5, 0, 2 landmarks (orders 26, 11, 17)
    cases = [
        ("row 3 26 26 3  0 0 2  5 0 2  0 0 0", OK),
        ("row 3 26 -1 3  0 0 2  5 0 2  0 0 0", OK),
        ("row 3 25 -1 3  0 0 2  5 0 2  0 0 0", INVALID),     # lda below the largest named source's order
        ("row 3 26 25 3  0 0 2  5 0 2  0 0 0", INVALID),     # ldg below it
        ("row 3 17 17 2  2 1    5 0 2  0 0 0", OK),          # the large filter is not named: its order does not count
        ("row 3 16 -1 2  2 1    5 0 2  0 0 0", INVALID),
        ("row 3 26 -1 2  0 2    5 0 2  0 25 1", INVALID),    # NaN in the last read entry of a named source's row
        ("row 3 26 -1 2  0 2    5 0 2  0 0 2", INVALID),     # Inf in its first
        ("row 3 26 -1 2  0 2    5 0 2  2 16 1", INVALID),
        ("row 3 26 -1 2  0 2    5 0 2  2 17 1", OK),         # beyond filter 2's own 17 entries: not read
        ("row 3 26 -1 2  0 2    5 0 2  1 3 1", OK),          # the row of a filter that is no child's source: not read
        ("row 3 26 -1 1  1      5 0 2  1 10 2", INVALID),
        ("row 3 11 11 1  1      5 0 2  0 0 0", OK),          # a filter without landmarks
    ]
    got = split_host("\n".join(c for c, _ in cases))
    assert [g[0] for g in got] == [w for _, w in cases], [(c, g[0], w) for (c, w), g in zip(cases, got) if g[0] != w]


def _expected_group(dst, src, N):
    order = []
    for s in src:
        if s not in order:
            order.append(s)
    sources, children, pairs, at = [], [], [], 0
    for si, s in enumerate(order):
        ks = [k for k in range(len(src)) if src[k] == s]
        sources.append([s, N[s], at, len(ks)])
        at += len(ks)
        for k in ks:
            pair = -1
            if dst[k] != s:
                pair = len(pairs)
                pairs.append([dst[k], s, N[s], 0])
            children.append([dst[k], pair, k, si])
    head = [len(sources), len(pairs), max(N[s] for s in order)]
    return [head] + sources + children + pairs


GROUPS = [
    ([0, 1, 2], [0, 0, 0], [5, 0, 2, 7]),
    ([3, 1, 2], [0, 0, 0], [5, 0, 2, 7]),
    ([5, 2, 4, 0, 3], [2, 2, 0, 0, 2], [3, 9, 1, 0, 0, 0]),       # interleaved sources, both with their child in place
    ([1], [1], [4, 6]),                                           # one child, in place: no pair
    ([0, 1, 2, 3, 4, 5, 6, 7], [7, 7, 2, 7, 7, 7, 7, 7], [1, 2, 3, 4, 5, 6, 7, 8]),
]


def test_children_are_grouped_by_source(split_host):
    text = "\n".join(f"group {len(N)} {len(d)} " + " ".join(map(str, d + s + N)) for d, s, N in GROUPS)
    out = iter(split_host(text))
    for d, s, N in GROUPS:
        for want in _expected_group(d, s, N):
            assert next(out) == want, (d, s, N)


def test_image_holds_rows_and_children_in_table_order(split_host):
    d, s, N = GROUPS[2]
    B, cap = len(N), 10
    out = split_host(f"image {B} {cap} {len(d)} " + " ".join(map(str, d + s + N)))
    ldr = 11 + 3 * cap
    nbytes = 8 * B * ldr + 16 * B + 16 * B + 16 * B + 16 * B
    assert out[0] == [nbytes, ldr]
    exp = _expected_group(d, s, N)
    ns = exp[0][0]
    for i in range(ns):
        src, Ns = exp[1 + i][0], exp[1 + i][1]
        assert out[1 + i] == [1000 * src + j + 1 if j < 11 + 3 * Ns else 0 for j in range(ldr)]
    calls = [c[2] for c in exp[1 + ns:1 + ns + len(d)]]
    assert out[1 + ns] == [k + 1 for k in calls] and out[2 + ns] == [k + 2 for k in calls]
    assert out[3 + ns] == [1]


def test_launch_grids(split_host):
    counts = (0, 1, 2, 5, 21, 85, 166, 167, 200, 1000)
    out = split_host("\n".join(f"grid {N}" for N in counts))
    for N, got in zip(counts, out):
        n = 12 + 3 * N
        assert got == [-(-n // 16), -(-n // 8), -(-n // 512), n], N
