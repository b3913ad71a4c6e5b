"""The allocation transaction of a filter handle, without a GPU: eqf_vio_amd/csrc/eqf_workspace_host.hpp (standard library only;
eqf_capi.hip runs the same reserve() over the HIP backend) -- tests/workspace_host_main.cpp is compiled with g++ under the address and
undefined-behaviour sanitizers and run as a child process, cases on stdin, results on stdout.  Its fake backend counts requests
(allocations and the drain) and fails the k-th: every case runs for every k up to the number of requests it makes and one beyond.
Every expected value -- the log of backend calls, the slots, the capacities -- is computed here from the contract."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "eqf_vio_amd", "csrc", "eqf_workspace_host.hpp")
DEV, PIN, EV = 0, 1, 2

# (piece, capacity index or -1, mapped): a route as the handle has them -- a staged image whose two images share one capacity with its
# event, a buffer and a pinned block of one size for the handle's life, a mapped pinned block that grows, a second growing buffer
SLOTS = [(PIN, 0, 0), (DEV, 0, 0), (EV, -1, 0), (DEV, -1, 0), (PIN, -1, 0), (PIN, 1, 1), (DEV, 2, 0), (DEV, -1, 0)]
NCAPS = 3
FIRST = [96, 96, 1, 640, 24, 40, 512, 0]          # (slot 7 is not wanted by the first call)
GROWS = [200, 200, 1, 640, 24, 16, 4096, 0]       # staged image and slot 6 replaced; 3, 4 kept; 5 large enough; 7 still not wanted
ADDS = [96, 96, 1, 640, 24, 40, 512, 72]          # everything kept, slot 7 new: nothing that existed is replaced
SHRINKS = [8, 8, 1, 1, 1, 1, 1, 0]                # needs nothing


def test_header_is_host_only_and_compiles_with_plain_gcc(tmp_path):
    includes = [ln.split()[1] for ln in open(HEADER) if ln.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "eqf_workspace_host.hpp"\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(tu)], check=True)


@pytest.fixture(scope="module")
def workspace_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("workspace_host") / "workspace_host")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.dirname(HEADER), "-o", exe, os.path.join(ROOT, "tests", "workspace_host_main.cpp")], check=True)

    def run(cases):
        """cases: lists of calls (failAt, bytes per slot) -> per case, per call: (ok, installed, log, state, live)"""
        text = "\n".join(" ".join(map(str, [len(SLOTS), NCAPS, len(calls), *[v for s in SLOTS for v in s],
                                            *[v for k, b in calls for v in (k, *b)]])) for calls in cases)
        r = subprocess.run([exe], input=text + "\n", capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])   # (a leak, a double free or a free of a foreign block ends it non-zero)
        lines = [[int(t) for t in ln.split()] for ln in r.stdout.split("\n")[:-1]]
        out, at = [], 0
        for calls in cases:
            res = []
            for _ in calls:
                head, st = lines[at], lines[at + 1]
                at += 2
                log = [tuple(head[3 + 3 * i:6 + 3 * i]) for i in range(head[2])]
                assert len(head) == 3 + 3 * head[2]
                res.append((head[0], head[1], log, [tuple(st[3 * i:3 * i + 3]) for i in range(len(SLOTS))], st[-1]))
            out.append(res)
        assert at == len(lines)
        return out

    return run


class Model:
    """the contract, restated: ids are handed out in the order of successful allocations"""

    def __init__(self):
        self.ids = [0] * len(SLOTS)
        self.caps = [0] * NCAPS
        self.next_id = 1

    def state(self):
        return [(self.ids[i], self.caps[c] if c >= 0 else -1, 1 if (m and self.ids[i]) else 0) for i, (_, c, m) in enumerate(SLOTS)]

    def live(self):
        return sum(1 for i in self.ids if i)

    def requests(self, want):
        need = self.need(want)
        return len(need) + (1 if any(self.ids[i] for i in need) else 0)

    def need(self, want):
        return [i for i, (_, c, _) in enumerate(SLOTS) if (want[i] > self.caps[c] if c >= 0 else (want[i] > 0 and not self.ids[i]))]

    def call(self, fail_at, want):
        """-> (ok, installed, log); the state changes on success only"""
        need, log, req, got = self.need(want), [], 0, []
        if not need:
            return 1, 0, []
        failed = False
        for i in need:
            req += 1
            if req == fail_at:
                log.append((9, SLOTS[i][0], 0))
                failed = True
                break
            got.append((i, self.next_id))
            log.append((1 + SLOTS[i][0], self.next_id, 1 if SLOTS[i][0] == EV else want[i]))
            self.next_id += 1
        if not failed and any(self.ids[i] for i in need):
            req += 1
            failed = req == fail_at
            log.append((7, 0 if failed else 1, 0))
        if failed:
            log += [(4 + SLOTS[i][0], n, 0) for i, n in reversed(got)] + [(8, 0, 0)]
            return 0, 0, log
        for i, n in got:
            if self.ids[i]:
                log.append((4 + SLOTS[i][0], self.ids[i], 0))
            self.ids[i] = n
            if SLOTS[i][1] >= 0:
                self.caps[SLOTS[i][1]] = want[i]
        return 1, sum(1 << i for i in need), log


def _check(res, model, fail_at, want):
    before = (model.state(), model.live())
    ok, installed, log = model.call(fail_at, want)
    assert (res[0], res[1]) == (ok, installed)
    assert res[2] == log
    assert (res[3], res[4]) == (model.state(), model.live())
    if not ok:   # the slots' ids (their pointers) and capacities are what they were, and what the call got is freed exactly once
        assert (res[3], res[4]) == before
        got = [e[1] for e in log if e[0] in (1, 2, 3)]
        assert sorted(e[1] for e in log if e[0] in (4, 5, 6)) == sorted(got) and log[-1] == (8, 0, 0)
    else:        # every replaced piece is freed exactly once, and only behind the drain; no drain unless something is replaced
        frees = [k for k, e in enumerate(log) if e[0] in (4, 5, 6)]
        drains = [k for k, e in enumerate(log) if e[0] == 7]
        assert len(set(log[k][1] for k in frees)) == len(frees)
        assert (len(drains) == 1 and drains[0] < min(frees)) if frees else not drains


def test_first_reserve_of_mixed_slots_for_every_failing_request(workspace_host):
    n_req = Model().requests(FIRST)
    assert n_req == 7   # (seven slots are missing, nothing exists: no drain)
    out = workspace_host([[(k, FIRST)] for k in range(0, n_req + 2)])
    for k, res in zip(range(0, n_req + 2), out):
        m = Model()
        _check(res[0], m, k, FIRST)
        assert res[0][0] == (0 if 1 <= k <= n_req else 1)
        assert not any(e[0] == 7 for e in res[0][2])   # nothing existed: no drain
        if res[0][0]:
            assert res[0][3][5][2] == 1 and res[0][3][7][0] == 0   # the mapped address came along; the slot nobody wanted stays empty


def test_growing_reserve_keeps_replaces_and_drains_once(workspace_host):
    base = Model()
    base.call(0, FIRST)
    n_req = base.requests(GROWS)
    assert n_req == 3 + 1 and base.need(GROWS) == [0, 1, 6]   # (both images of the staged image and slot 6, and the drain)
    ks = list(range(0, n_req + 2))
    out = workspace_host([[(0, FIRST), (k, GROWS)] for k in ks])
    for k, res in zip(ks, out):
        m = Model()
        _check(res[0], m, 0, FIRST)
        _check(res[1], m, k, GROWS)
        assert res[1][0] == (0 if 1 <= k <= n_req else 1)
        if res[1][0]:
            assert res[1][1] == (1 << 0) | (1 << 1) | (1 << 6)
            assert [e for e in res[1][2] if e[0] == 7] == [(7, 1, 0)]
            assert res[1][3][5] == res[0][3][5] and res[1][3][3] == res[0][3][3]   # large enough / of one size: kept, pointer and all
        if k == n_req:   # the drain itself fails: nothing old has been freed
            assert res[1][2][-5:] == [(7, 0, 0), (4, 10, 0), (4, 9, 0), (5, 8, 0), (8, 0, 0)]


def test_a_reserve_that_needs_nothing_makes_no_backend_call(workspace_host):
    out = workspace_host([[(0, FIRST), (1, FIRST), (1, SHRINKS), (1, [0] * len(SLOTS))]])[0]
    m = Model()
    _check(out[0], m, 0, FIRST)
    for res, want in zip(out[1:], (FIRST, SHRINKS, [0] * len(SLOTS))):
        _check(res, m, 1, want)   # (the first request would fail: there is none)
        assert res[:3] == (1, 0, []) and res[3] == out[0][3]


def test_no_drain_when_nothing_that_existed_is_replaced(workspace_host):
    base = Model()
    base.call(0, FIRST)
    assert base.requests(ADDS) == 1
    out = workspace_host([[(0, FIRST), (k, ADDS)] for k in (0, 1, 2)])
    for k, res in zip((0, 1, 2), out):
        m = Model()
        _check(res[0], m, 0, FIRST)
        _check(res[1], m, k, ADDS)
        assert not any(e[0] == 7 for e in res[1][2])
        assert res[1][0] == (0 if k == 1 else 1) and res[1][1] == ((1 << 7) if k != 1 else 0)


def test_a_failed_call_can_be_repeated(workspace_host):
    """after a failure the handle is as before: the same call, not failing, does what it would have done at first"""
    out = workspace_host([[(0, FIRST), (2, GROWS), (4, GROWS), (0, GROWS), (0, GROWS)]])[0]
    m = Model()
    for res, k, want in zip(out, (0, 2, 4, 0, 0), (FIRST, GROWS, GROWS, GROWS, GROWS)):
        _check(res, m, k, want)
    assert [r[0] for r in out] == [1, 0, 0, 1, 1] and out[4][2] == [] and out[3][4] == 7
