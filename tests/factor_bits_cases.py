"""The cases of tests/test_gpu_factor_bits.py and of its recorder tests/golden/make_golden_factor_bits.py: every public call that runs the
blocked Cholesky of csrc/eqf_factor.hpp, at the smallest shapes that meet each edge of the shared kernels, with everything it returns
reduced to digests.  One function per case, `CASES[name](binding) -> {field: digest}`.

Inputs: the states of tests/mixture_cases.member (numpy.random.default_rng, fixed seeds; Sigma symmetric positive definite) through
restore_state, operands from default_rng(SEED + ...) here.  A digest is a list of hex floats for a float array of at most 16 entries
(the scalar outputs: a mismatch then shows the values), else the sha256 of dtype, shape and bytes.

Edges (64-wide block columns, 16-row strips, the right-hand side in 64-row block rows of its own):
  nees              orders 12, 63, 66, 129 at first = 0 (one block column; one short of full; two; three, the last of one row);
                    first = 0 | 6 | 11 (the pad index inside the first block / absent); N = 0 with first = 11: the empty submatrix;
                    nrhs = 0 | 1 | 15 | 16; both charts; one ragged handle [0, 5, 18, 70]
  draws             N = 18 | 39, first = 0 | 6, nsamp = 1 | 17 (two row tiles), both charts; perturb with a scale of 0 in the batch
  update_landmarks  rows = 1 | 2 | 3; N = 18 | 25 | 39, one entry per landmark and one whose id is absent: S padded to 64 or 128, orders 17 ..
                    114; the right-hand side has 12 + 3 N + 1 = 67 | 88 | 130 rows: one, two and three block rows, the last of 3, 24 and 2
                    rows (the trailing update's short-row path and its full path).  One entry gated per filter.  A batch of three
                    with the middle filter masked out.
  merge_costs       three members, all pairs, both kinds, N = 17 | 18, first = 0 | 11
"""
import hashlib

import numpy as np

import mixture_cases as mc

SEED = 9100
CAP_EXTRA = 7


def digest(x):
    a = np.ascontiguousarray(x)
    if a.dtype.kind == "f" and a.size <= 16:
        return [float(v).hex() for v in a.reshape(-1)]
    if a.dtype.kind in "iu" and a.size <= 16:
        return [int(v) for v in a.reshape(-1)]
    h = hashlib.sha256()
    h.update(f"{a.dtype.str}{a.shape}".encode())
    h.update(a.tobytes())
    return h.hexdigest()


def _handle(hip, Ns):
    """one filter per entry of Ns: member b + 1 of the family of its size (tilted off the master state: every chart is a general one)"""
    fg = hip.FilterBatch(mc.cc.settings(), capacity=max(Ns) + CAP_EXTRA, batch=len(Ns))
    for b, N in enumerate(Ns):
        fg.restore_state(mc.member(N, b + 1), b)
    return fg


def _state_fields(fg, b, pre):
    st = fg.dump_state(b)
    out = {f"{pre}bias": st["bias"], f"{pre}sigma": st["sigma"]}
    for grp in ("origin", "group"):
        for k, v in sorted(st[grp].items()):
            out[f"{pre}{grp}.{k}"] = np.asarray(v, dtype=np.float64)
    return out


STATS = ("logdet", "min_pivot", "dof", "info")


def _nees(Ns):
    def run(hip):
        fg = _handle(hip, Ns)
        B, nmax = len(Ns), 11 + 3 * max(Ns)
        out = {}
        for first in (0, 6, 11):
            for nrhs in (0, 1, 15, 16):
                err = np.random.default_rng(SEED + 100 * first + nrhs).standard_normal((B, 16, nmax))[:, :nrhs]
                for local in (0, 1):
                    r = fg.nees(err if nrhs else None, local=bool(local), first=first)
                    for k in ("nees",) + STATS:
                        out[f"first{first}/nrhs{nrhs}/local{local}/{k}"] = r[k]
        assert fg.device_error() == 0
        fg.close()
        return {k: digest(v) for k, v in out.items()}

    return run


def _draws(N):
    def run(hip):
        Ns = [N, N, 5]
        fg = _handle(hip, Ns)
        B, nmax = len(Ns), 11 + 3 * N
        out = {}
        for first in (0, 6):
            for nsamp in (1, 17):
                z = np.random.default_rng(SEED + 1000 + 10 * first + nsamp).standard_normal((B, nsamp, nmax))
                for local in (0, 1):
                    r = fg.sample_sigma(z, local=bool(local), first=first, scale=None if local else [1.0, 0.5, 2.0])
                    for k in ("eps",) + STATS:
                        out[f"sample/first{first}/nsamp{nsamp}/local{local}/{k}"] = r[k]
        for first in (0, 6):
            z = np.random.default_rng(SEED + 2000 + first).standard_normal((B, 1, nmax))
            st = fg.perturb(0.01 * z, first=first, scale=[1.0, 0.0, 0.5], stats=True)
            for k in STATS:
                out[f"perturb/first{first}/{k}"] = st[k]
            for b in range(B):
                out.update(_state_fields(fg, b, f"perturb/first{first}/b{b}/"))
        assert fg.device_error() == 0
        fg.close()
        return {k: digest(v) for k, v in out.items()}

    return run


LM_GATE = 30.0


def _entries(rng, st, rows):
    """one entry per landmark of the snapshot and, in front, one whose id is not in the state; the entry of landmark N // 2 fails LM_GATE"""
    ids = np.concatenate([[5], st["ids"]]).astype(np.int32)
    K = len(ids)
    H = rng.standard_normal((K, rows, 3))
    resid = 0.1 * rng.standard_normal((K, rows))
    resid[1 + len(st["ids"]) // 2] = 50.0
    A = rng.standard_normal((K, rows, rows))
    R = 0.05 * A @ A.transpose(0, 2, 1) + 0.1 * np.eye(rows)
    return ids, H, resid, R


def _blocks(rows, Ns, local, mask=None):
    def run(hip):
        fg = _handle(hip, Ns)
        rng = np.random.default_rng(SEED + 3000 + 100 * rows + Ns[0])
        ops = [_entries(rng, fg.dump_state(b), rows) for b in range(len(Ns))]
        r = fg.update_landmarks(*[[o[j] for o in ops] for j in range(4)], rows=rows, local=bool(local), lm_gate=LM_GATE, mask=mask)
        out = {}
        for b, N in enumerate(Ns):
            if mask is None or mask[b]:
                assert r["info"][b] == 0 and sorted(np.bincount(r["used"][b, : N + 1], minlength=3)) == [1, 1, N - 1], (r["info"], r["used"][b])
            else:
                assert r["info"][b] == 3
            out[f"b{b}/sigma"] = fg.sigma(b)
        for k in ("gamma", "nis", "logdet_S", "loglik", "dof", "info", "used"):
            out[k] = r[k]
        assert fg.device_error() == 0
        fg.close()
        return {k: digest(v) for k, v in out.items()}

    return run


def _merge(N):
    def run(hip):
        fg = hip.FilterBatch(mc.cc.settings(), capacity=N + CAP_EXTRA, batch=3)
        for k in range(3):
            fg.restore_state(mc.member(N, k), k)
        w = np.random.default_rng(SEED + 4000 + N).uniform(0.2, 1.5, 3)
        out = {}
        for kind in ("runnalls", "bhattacharyya"):
            for first in (0, 11):
                r = fg.merge_costs([0, 1, 2], w, ref=1, kind=kind, first=first)
                for k in ("cost", "logdet_pair", "maha", "info", "member_logdet", "member_min_pivot", "member_dof", "member_info"):
                    out[f"{kind}/first{first}/{k}"] = r[k]
        assert fg.device_error() == 0
        fg.close()
        return {k: digest(v) for k, v in out.items()}

    return run


CASES = {}
for _N in (0, 17, 18, 39):
    CASES[f"nees-N{_N}"] = _nees([_N])
CASES["nees-ragged"] = _nees([0, 5, 18, 70])
for _N in (18, 39):
    CASES[f"draws-N{_N}"] = _draws(_N)
for _i, _N in enumerate((18, 25, 39)):
    for _rows in (1, 2, 3):
        CASES[f"blocks-rows{_rows}-N{_N}"] = _blocks(_rows, [_N], (_i + _rows) % 2)
CASES["blocks-rows2-batch"] = _blocks(2, [18, 25, 39], 0, mask=[1, 0, 1])
for _N in (17, 18):
    CASES[f"merge-N{_N}"] = _merge(_N)
