"""The border rows of the E-chain's last block row, without a GPU: which filters take them and how many role workgroups that leaves
(eqf_vio_amd/csrc/eqf_border_host.hpp, host only, standard library only -- tests/border_host_main.cpp is compiled with g++ under the address
and undefined-behaviour sanitizers and run as a child process, cases on stdin, results on stdout), and the identity the kernel relies on:
with the eleven regressor columns B = [Z_P | E_top] as rows behind the last real 16-column stage of the padded chain matrix and a ZERO
corner, a right-looking elimination that stops in front of those rows leaves -B^T Sigma_e^-1 B in the corner.  Every expected value is
computed here."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "eqf_vio_amd", "csrc", "eqf_border_host.hpp")


@pytest.fixture(scope="module")
def border_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("border_host") / "border_host")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.dirname(HEADER), "-o", exe, os.path.join(ROOT, "tests", "border_host_main.cpp")], check=True)

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        return [[int(t) for t in ln.split()] for ln in r.stdout.split("\n")[:-1]]

    return run


def test_header_is_host_only_and_compiles_with_plain_gcc(tmp_path):
    includes = [ln.split()[1] for ln in open(HEADER) if ln.startswith("#include")]
    assert all(i.startswith("<") and "hip" not in i for i in includes), includes
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "eqf_border_host.hpp"\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(tu)], check=True)


def closed_form_stage(N):
    """-1 when the order of Sigma_e is a multiple of 64 or leaves more than 48 real rows in the last block, else the real stages of it"""
    rem = (6 + 3 * N) % 64
    return -1 if rem == 0 or rem > 48 else -(-rem // 16)


def chain_roles(nb, wt):
    return (nb - 1) + (nb - 1) * (nb - 2) // 2 + wt * nb


def test_eligibility_and_role_counts(border_host):
    assert border_host("const") == [[64, 16, 11, 3]]
    Ns = list(range(1, 401))
    out = border_host("\n".join(f"stage {N}" for N in Ns))
    for N, (stage, on, last, nb, plain, with_border, row0) in zip(Ns, out):
        e = 6 + 3 * N
        assert nb == -(-e // 64)
        assert stage == closed_form_stage(N), N
        assert last == min(4, -(-(e - 64 * (nb - 1)) // 16))
        assert on == int(stage >= 0 and nb >= 2), N
        want_plain = chain_roles(-(-2 * N // 64), -(-(18 + 3 * N) // 64)) + chain_roles(nb, 1)
        assert plain == want_plain, N
        # with the border only the last right-hand-side tile of the E-chain stays (it runs the lift): nb - 1 workgroups fewer
        assert with_border == (want_plain - (nb - 1) if on else want_plain), N
        if stage >= 0:
            # the border sits behind the last real column, inside the last block, with its eleven rows in ONE unpivoted stage
            assert row0 == 64 * (nb - 1) + 16 * stage and row0 >= e and row0 + 11 <= 64 * nb and row0 % 16 == 0
        else:
            assert row0 == -1
    by = dict(zip(Ns, out))
    assert by[200][0] == 2 and by[200][1] == 1
    assert by[41][0] == 1 and by[41][1] == 1
    for N in (36, 40, 62):
        assert by[N][0] == -1 and by[N][1] == 0
    assert [by[N][0] for N in (20, 21, 30, 35, 70)] == [1, 1, 2, 3, 2]
    assert by[14][0] == 3 and by[14][1] == 0  # (room, but one block column: no row head that could finish the corner)


def test_roles_a_batch_may_leave_out(border_host):
    out = border_host("\n".join(["omit 10 200", "omit 10 200 62", "omit 10 200 41", "omit 2 35 36", "omit 10 0 200", "omit 1 12", "omit 3 200"]))
    assert out[0] == [1] * 9 + [0]                     # one eligible filter: only the lift's workgroup stays
    assert out[1] == [0] * 3 + [1] * 6 + [0]           # N = 62 (order 192, three block columns, no border) needs W(0, 0..2); the lift of N = 200 needs 9
    assert out[2] == [1, 1, 0] + [1] * 6 + [0]         # two eligible filters: block rows 2 and 9
    assert out[3] == [0, 0]                            # N = 36 keeps every role
    assert out[4] == [1] * 9 + [0]                     # a filter without landmarks takes no part
    assert out[5] == [0]
    assert out[6] == [0, 0, 0]                         # a table shorter than a filter's chain: nothing is left out


def padded_chain_matrix(N, rng):
    """Sigma_e (order n_e = 6 + 3 N, index 5 the identity pad), B = [Z_P | E_top] (n_e x 11), and the kernel's padded matrix: identity rows
    past n_e, B^T as rows 16 nst .. 16 nst + 10 of the last 64-block, a ZERO 11 x 11 corner"""
    ne = 6 + 3 * N
    nb = -(-ne // 64)
    nst = closed_form_stage(N)
    assert nst >= 0
    A = rng.standard_normal((ne, ne))
    Se = A @ A.T / ne + np.eye(ne)
    Se[5, :] = Se[:, 5] = 0.0
    Se[5, 5] = 1.0
    Bm = np.zeros((ne, 11))
    Bm[6:, :6] = rng.standard_normal((ne - 6, 6))  # Z_P: landmark rows only
    Bm[:5, 6:] = np.eye(5)                         # E_top
    n = 64 * nb
    r0 = 64 * (nb - 1) + 16 * nst
    M = np.eye(n)
    M[:ne, :ne] = Se
    M[r0:r0 + 11, :ne] = Bm.T
    M[:ne, r0:r0 + 11] = Bm
    M[r0:r0 + 11, r0:r0 + 11] = 0.0
    return Se, Bm, M, r0


@pytest.mark.parametrize("N", [20, 21, 30, 35, 41, 200])
def test_elimination_in_front_of_the_border_leaves_minus_G11(N):
    Se, Bm, M, r0 = padded_chain_matrix(N, np.random.default_rng(100 + N))
    for k in range(r0):  # right-looking, every pivot in front of the border rows (real columns and the identity padding between)
        col = M[k + 1:, k] / np.sqrt(M[k, k])
        M[k + 1:, k + 1:] -= np.outer(col, col)
    G11 = Bm.T @ np.linalg.solve(Se, Bm)
    got = -M[r0:r0 + 11, r0:r0 + 11]
    rel = np.abs(got - G11).max() / np.abs(G11).max()
    print(f"N = {N}: border at row {r0}, |corner + G11| / |G11| = {rel:.2e}")
    assert rel <= 1e-12
    # the rows behind the border are untouched identity rows: nothing of the border leaks into the padding
    assert np.array_equal(M[r0 + 11:, r0 + 11:], np.eye(M.shape[0] - r0 - 11))
