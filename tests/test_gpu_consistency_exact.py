"""The getters a filter is judged by, on the device, entry by entry against the exact references and a-priori bounds of
tests/consistency_exact.py (the cases: tests/consistency_cases.py; the same bounds on the CPU: tests/test_consistency_exact.py).

Part A: eqf_get_sigma_local / eqf_get_marginals / eqf_get_local_jacobian (csrc/eqf_local.hpp) past one 256-lane column chunk and one 16-row
chunk, on states with large rotations, scales over 2.6 decades and a gravity chart 0.5 rad and 1e-2 rad from its pole.  States go in through
restore_state; the inputs of every reference are the device's own sigma(), origin() and group().

Part B: eqf_get_nees / eqf_sample_sigma / eqf_perturb_filters (csrc/eqf_nees.hpp, csrc/eqf_sample.hpp) against the longdouble factor of the
device's own sigma() / sigma_local(), componentwise: internal orders 15 .. 258 (a one-row last block, the 256-stride of the tail's sums), the
pad row at index 11 or 5 of the first block or absent, both charts, 1 / 15 / 16 error vectors, 1 / 16 / 17 / 64 draws, scale 1 and -0.5.

Part C: eqf_get_innovation_stats (csrc/eqf_innov.hpp) of one vision call against update_exact's reference of the same call, with bounds made
of update_bounds' own parts; N up to 257 (the strides of all three sums); bit for bit the same statistics under every launch shape.

Worst ratio to the bound on an MI355X (each test prints its own, next to a CPU restatement's): NOTES.md R17.1 -- A 0.17 .. 0.28 at every size;
B nees <= 0.039, logdet <= 0.086, min_pivot <= 0.20, draws <= 0.14; C nis <= 0.028, logdet_S <= 0.0045, nis_lm <= 0.25.  No case is exempt."""
import ctypes as C

import numpy as np
import pytest

import consistency_cases as cc
import consistency_exact as cx
import lie_edge_cases as ec
import riccati_cases as rc
import update_cases as uc
import update_exact as ux

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from eqf_vio_amd import binding

    return binding


@pytest.fixture(scope="module")
def master_J():
    """{theta: the 50-digit J blocks of the master state}: one reference for every size (a state of N landmarks is a prefix)."""
    out = {}
    for th in cc.LOCAL_THETAS:
        s = cc.local_state(cc.LOCAL_MASTER, th)
        out[th] = cx.jacobian_mp(s["origin"], s["group"])
    return out


@pytest.fixture(scope="module")
def own_sigma(hip):
    """{N: a filter's own Sigma after five vision frames} for family a."""
    from eqf_vio_amd import synth

    out = {}
    for N in sorted({n for n in cc.LOCAL_SIZES + cc.LOCAL_RAGGED if 1 <= n <= cc.LOCAL_OWN_MAX} | {n for n in cc.NEES_SIZES + cc.NEES_RAGGED if n}):
        st = synth.make_stream(N, duration=0.4)
        fg = hip.FilterBatch(cc.settings(), capacity=N + cc.CAP_EXTRA, batch=1)
        seen = 0
        for kind, k in st.events():
            if kind == "imu":
                r = st.imu[k]
                fg.process_imu(r[0], r[1:4], r[4:7])
            else:
                fg.process_vision(st.vision_stamps[k], st.ids, st.bearings[k])
                seen += 1
                if seen == 5:
                    break
        assert fg.num_landmarks(0) == N and fg.device_error() == 0
        out[N] = fg.sigma(0)
        fg.close()
    return out


def _same_state(fg, b, snap):
    """origin() / group() are the doubles that went in (the reference is computed from the snapshot's master state)"""
    o, g = fg.origin(b), fg.group(b)
    for k in ("q", "x", "v", "p"):
        assert np.array_equal(o[k], snap["origin"][k]), k
    for k in ("Aq", "Ax", "w", "Qq", "Qa"):
        assert np.array_equal(g[k], snap["group"][k]), k


def _check_local(fg, b, Jmp, Sset, what):
    """sigma_local(b) against the reference and its bound; returns (ratio to the new bound, ratio to 256 u, median and largest new / old bound, Sl)."""
    S = fg.sigma(b)
    assert np.array_equal(S, Sset), (what, "sigma() is not what set_sigma was given")
    ref = cx.sigma_local_reference(Jmp, S)
    bound, old = cx.sigma_local_bound(Jmp, S, cc.K_J)
    Sl = fg.sigma_local(b)
    assert Sl.shape == S.shape
    r_new, nz = cx.bound_ratio(Sl, ref, bound)
    r_old, _ = cx.bound_ratio(Sl, ref, old)
    q = bound[old > 0] / old[old > 0]
    Jd = cx.dense_J(fg.local_jacobian(b), (len(S) - 11) // 3)
    r_np, _ = cx.bound_ratio(Jd @ S @ Jd.T, ref, bound)  # (numpy's matmul on the device's own J blocks: a CPU restatement, printed only)
    print(f"A {what}: device / new bound {r_new:.4f} (numpy restatement {r_np:.4f}), device / (256 u) bound {r_old:.5f}, "
          f"new bound / old bound median {np.median(q):.4f} max {q.max():.4f}")
    assert nz == 0, (what, "non-zero entries where the bound is exactly zero", nz)
    assert r_new <= 1.0, (what, r_new)
    return r_new, r_old, Sl


@pytest.mark.parametrize("N", cc.LOCAL_SIZES)
def test_sigma_local_entry_by_entry(hip, master_J, own_sigma, N):
    fg = hip.FilterBatch(cc.settings(), capacity=N + cc.CAP_EXTRA, batch=1)
    worst = {}
    for th in cc.LOCAL_THETAS:
        Jmp = master_J[th]
        snap = cc.local_state(N, th)
        for fam in cc.local_families(N):
            snap["sigma"] = cc.local_sigma(snap, fam, own_sigma.get(N))
            fg.restore_state(snap)
            _same_state(fg, 0, snap)
            r_new, r_old, Sl = _check_local(fg, 0, Jmp, snap["sigma"], f"N={N} theta={th:g} family {fam}")
            worst[fam] = max(worst.get(fam, 0.0), r_new)
            # marginals: bit for bit the blocks of sigma() / sigma_local(), second column workgroup of k_marginals included
            for local, M in ((0, snap["sigma"]), (1, Sl)):
                mg = fg.marginals(0, local=bool(local))
                assert np.array_equal(mg["base"], M[:11, :11]), (N, th, fam, local)
                want = np.array([M[11 + 3 * i:14 + 3 * i, 11 + 3 * i:14 + 3 * i] for i in range(N)]).reshape(N, 3, 3)
                assert np.array_equal(mg["lm"], want), (N, th, fam, local, np.argwhere(mg["lm"] != want)[:4])
        # the J blocks as the device built them, inside K_J
        dj = fg.local_jacobian(0)
        assert dj["lm"].shape == (N, 3, 3)
        rj = cx.jacobian_ratios(dj, Jmp)
        print(f"A N={N} theta={th:g}: device J in units of u max|block| (G: u / theta^2): " + "  ".join(f"{k} {v:.3f} (K_J {cc.K_J[k]:.2f})" for k, v in rj.items()))
        assert all(rj[k] <= cc.K_J[k] for k in rj), rj
    print(f"A N={N}: worst device / bound per family: " + "  ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert fg.device_error() == 0


def test_sigma_local_ragged_handle_per_filter_and_many_filter_launch(hip, master_J, own_sigma):
    """nb = [0, 5, 257, 17] in one handle.  sigma_local(b) launches with b0 = b, count = 1: inside the bound per filter.  The launch with
    count = B, b0 = 0 (eqf_debug_sigma_local_all; the one inside eqf_get_nees(local = 1) and eqf_sample_sigma(local = 1)) leaves its image in a
    device buffer that no getter copies out, so it is compared through its readers: a second handle is GIVEN sigma_local(b) of every filter as
    its Sigma, and nees / sample_sigma with local = 0 there run the same factorisation on those bits as local = 1 does here on the many-filter
    image.  NEES of 16 vectors, log det, the smallest pivot and 64 draws per filter must agree bit for bit: they read every entry of the
    image's lower triangle (the upper triangle of the many-filter image has no reader in the interface)."""
    th = cc.LOCAL_THETAS[0]
    nb = cc.LOCAL_RAGGED
    B, cap = len(nb), max(nb) + cc.CAP_EXTRA
    fa, fb = hip.FilterBatch(cc.settings(), capacity=cap, batch=B), hip.FilterBatch(cc.settings(), capacity=cap, batch=B)
    rng = np.random.default_rng(5)
    snaps, images = [], []
    for b, N in enumerate(nb):
        snap = cc.local_state(N, th)
        snap["sigma"] = cc.local_spd(N)
        fa.restore_state(snap, b)
        snaps.append(snap)
    fa.debug_sigma_local_all()
    fa.synchronize()
    for b, N in enumerate(nb):
        _same_state(fa, b, snaps[b])
        _, _, Sl = _check_local(fa, b, master_J[th], snaps[b]["sigma"], f"ragged b={b} N={N}")
        images.append(Sl)
        s2 = dict(snaps[b])
        s2["sigma"] = Sl
        fb.restore_state(s2, b)
    err = [rng.standard_normal((16, 11 + 3 * N)) for N in nb]
    z = [rng.standard_normal((64, 11 + 3 * N)) for N in nb]
    na, nbb = fa.nees(err, local=True), fb.nees(err, local=False)
    assert np.all(na["info"] == 0) and np.all(nbb["info"] == 0)
    for k in ("nees", "logdet", "min_pivot", "dof", "info"):
        assert np.array_equal(na[k], nbb[k]), k
    sa, sb = fa.sample_sigma(z, local=True), fb.sample_sigma(z, local=False)
    assert np.all(sa["info"] == 0) and np.array_equal(sa["eps"], sb["eps"])
    assert np.abs(sa["eps"]).max() > 0
    assert fa.device_error() == 0 and fb.device_error() == 0


# ---- part B ---------------------------------------------------------------------------------------------------------------------------------
SENTINEL = 7.25
EXTRA = 5


def _sample(hip, fg, Z, local, first, scale):
    """eqf_sample_sigma through the C ABI with sentinel-filled buffers EXTRA columns wider than the largest state: (eps (B, nsamp, ld), stats)"""
    B, nsamp, nmax = Z.shape
    ld = nmax + EXTRA
    Zb, eps = np.full((B, nsamp, ld), SENTINEL), np.full((B, nsamp, ld), SENTINEL)
    Zb[:, :, :nmax] = Z
    sc = np.ascontiguousarray(np.broadcast_to(np.asarray(scale, dtype=np.float64), (B,)))
    st = (hip.SigmaStats * B)()
    dp = C.POINTER(C.c_double)
    rc = hip.lib().eqf_sample_sigma(fg._h, int(local), int(first), nsamp, Zb.ctypes.data_as(dp), ld, sc.ctypes.data_as(dp), eps.ctypes.data_as(dp), ld, st)
    assert rc == 0, rc
    return eps, dict(logdet=np.array([x.logdet for x in st]), min_pivot=np.array([x.min_pivot for x in st]), dof=np.array([x.dof for x in st]),
                     info=np.array([x.info for x in st]))


def _check_factor(fg, b, N, local, first, got, E, eps_b, Z, scale, what, worst):
    """filter b's answers of one nees call and one sample call against FactorRef of its own sigma() / sigma_local()"""
    n_full = 11 + 3 * N
    S = fg.sigma_local(b) if local else fg.sigma(b)
    ref = cx.FactorRef(cx.cut(S, first), first, cc.C_LOG)
    assert ref.validity <= cx.VALIDITY, (what, ref.validity)
    assert got["info"][b] == 0 and got["dof"][b] == ref.n, (what, got["info"][b], got["dof"][b])
    r = cx.nees_ratios(ref, got["nees"][b, :len(E)], got["logdet"][b], got["min_pivot"][b], E[:, first:n_full])
    assert np.all(eps_b[:, :first] == 0.0), (what, "draw: entries below first are not exactly zero")
    assert np.all(eps_b[:, n_full:] == SENTINEL), (what, "draw: entries beyond the filter's own order were written")
    d = cx.draw_ratios(ref, eps_b[:, first:n_full], Z[:, first:n_full], scale)
    share = ref.mp_share(E[:, first:n_full]) if ref.n <= cx.MP_MAX_ORDER else 0.0
    Ll = np.linalg.cholesky(ref.A)  # (LAPACK on the same matrix: a CPU restatement, printed only)
    zl = np.linalg.solve(Ll, E[:, first:n_full].T)
    rl = cx.nees_ratios(ref, (zl * zl).sum(axis=0), 2 * np.log(np.diag(Ll)).sum(), (np.diag(Ll) ** 2).min(), E[:, first:n_full])
    dl = cx.draw_ratios(ref, scale * (Z[:, first:n_full] @ Ll.T), Z[:, first:n_full], scale)
    print(f"B {what} n={ref.n} m={ref.m}: device / bound nees {r['nees']:.4f} logdet {r['logdet']:.4f} min_pivot {r['min_pivot']:.4f} draw {d['draw']:.4f}"
          f" (LAPACK {rl['nees']:.4f} {rl['logdet']:.4f} {rl['min_pivot']:.4f} {dl['draw']:.4f})"
          f" | device / (n u kappa_2) nees {r['old']['nees']:.2e} logdet {r['old']['logdet']:.2e} draw {d['old']:.2e}"
          f" | new bound / (n u kappa_2) nees {r['bound_vs_old']['nees']:.2e} logdet {r['bound_vs_old']['logdet']:.2e} draw {d['bound_vs_old']:.2e}"
          f" | kappa_2 {ref.kappa:.1e} validity {ref.validity:.1e}" + (f" | longdouble vs mpmath {share:.1e} of the bound" if share else ""))
    assert share <= 0.01, (what, share)
    for k, v in (("nees", r["nees"]), ("logdet", r["logdet"]), ("min_pivot", r["min_pivot"]), ("draw", d["draw"])):
        worst[k] = max(worst.get(k, 0.0), v)
        assert v <= 1.0, (what, k, v)


@pytest.mark.parametrize("N", cc.NEES_SIZES)
def test_nees_and_draws_componentwise(hip, own_sigma, N):
    fg = hip.FilterBatch(cc.settings(), capacity=N + cc.CAP_EXTRA, batch=1)
    snap = cc.local_state(N, cc.NEES_THETA)
    worst, current = {}, None
    for fam, local, first, nrhs, nsamp, scale in cc.nees_plan(N):
        if fam != current:
            snap["sigma"] = cc.nees_sigma(N, fam, own_sigma.get(N))
            fg.restore_state(snap)
            current = fam
        E = cc.nees_vectors(N, fam, local, first, nrhs, "err")
        Z = cc.nees_vectors(N, fam, local, first, nsamp, "z")
        got = fg.nees([E], local=bool(local), first=first)
        eps, st = _sample(hip, fg, Z[None], local, first, scale)
        for k in ("logdet", "min_pivot", "dof", "info"):  # (the same launches factor for both calls)
            assert np.array_equal(st[k], got[k]), (fam, local, first, k)
        w = worst.setdefault(fam, {})
        _check_factor(fg, 0, N, local, first, got, E, eps[0], Z, scale, f"N={N} {fam} local={local} first={first} nrhs={nrhs} nsamp={nsamp} scale={scale:g}", w)
    for fam, w in worst.items():
        print(f"B N={N} family {fam}: worst device / bound " + "  ".join(f"{k} {v:.4f}" for k, v in w.items()))
    assert fg.device_error() == 0


def test_nees_and_draws_on_a_ragged_handle(hip, own_sigma):
    """nb = [0, 5, 18, 70] in one handle, every `first`, both charts; with first = 11 the filter without landmarks has order 0."""
    nb = cc.NEES_RAGGED
    fams = ("graded", "own", "coupled", "one_small")
    B, nmax = len(nb), 11 + 3 * max(nb)
    fg = hip.FilterBatch(cc.settings(), capacity=max(nb) + cc.CAP_EXTRA, batch=B)
    for b, N in enumerate(nb):
        snap = cc.local_state(N, cc.NEES_THETA)
        snap["sigma"] = cc.nees_sigma(N, fams[b], own_sigma.get(N))
        fg.restore_state(snap, b)
    scale = np.array([1.0, -0.5, 1.0, -0.5])
    worst = {}
    for first in cc.NEES_FIRSTS:
        for local in (0, 1):
            E = [cc.nees_vectors(N, fams[b], local, first, 15, "err") for b, N in enumerate(nb)]
            Z = np.zeros((B, 17, nmax))
            for b, N in enumerate(nb):
                Z[b, :, :11 + 3 * N] = cc.nees_vectors(N, fams[b], local, first, 17, "z")
            got = fg.nees(E, local=bool(local), first=first)
            eps, st = _sample(hip, fg, Z, local, first, scale)
            for k in ("logdet", "min_pivot", "dof", "info"):
                assert np.array_equal(st[k], got[k]), (local, first, k)
            for b, N in enumerate(nb):
                if 11 + 3 * N - first == 0:  # the empty submatrix
                    assert got["dof"][b] == 0 and got["info"][b] == 0 and got["logdet"][b] == 0.0 and got["min_pivot"][b] == np.inf
                    assert np.all(got["nees"][b] == 0.0) and np.all(eps[b, :, :11] == 0.0) and np.all(eps[b, :, 11:] == SENTINEL)
                    continue
                _check_factor(fg, b, N, local, first, got, E[b], eps[b], Z[b], scale[b], f"ragged b={b} N={N} {fams[b]} local={local} first={first}", worst)
    print("B ragged handle: worst device / bound " + "  ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert fg.device_error() == 0


def test_perturb_is_sample_plus_increment_at_258_internal_rows(hip):
    """eqf_perturb_filters at N = 82 (m = 258): bit for bit eqf_sample_sigma(local = 0, nsamp = 1) + eqf_apply_increment."""
    N = cc.NEES_SIZES[-1]
    snap = cc.local_state(N, cc.NEES_THETA)
    snap["sigma"] = cc.nees_sigma(N, "coupled")
    fa, fb = (hip.FilterBatch(cc.settings(), capacity=N + cc.CAP_EXTRA, batch=1) for _ in range(2))
    fa.restore_state(snap)
    fb.restore_state(snap)
    z = cc.nees_vectors(N, "coupled", 0, 0, 1, "z")[None]
    sa = fa.perturb(z, first=0, scale=0.01, stats=True)
    got = fb.sample_sigma(z, local=False, first=0, scale=0.01)
    fb.apply_increment(got["eps"][:, 0, :])
    assert sa["info"][0] == 0 and got["info"][0] == 0 and np.array_equal(sa["logdet"], got["logdet"])
    da, db = fa.dump_state(), fb.dump_state()
    assert not np.array_equal(da["group"]["Qq"], snap["group"]["Qq"])  # (it moved)
    for k in ("Aq", "Ax", "w", "Qq", "Qa"):
        assert np.array_equal(da["group"][k], db["group"][k]), k
    assert np.array_equal(da["bias"], db["bias"]) and np.array_equal(da["sigma"], db["sigma"])
    assert fa.device_error() == 0 and fb.device_error() == 0


# ---- part C ---------------------------------------------------------------------------------------------------------------------------------
ENV_KEYS = ("EQF_RES_FOLD_PREP", "EQF_CHOL_RESIDENT", "EQF_CHOL_SPLIT", "EQF_BURST_FUSED", "EQF_BURST_ROWS", "EQF_IMU_BURST", "EQF_SPLIT_PROPAGATE")


@pytest.fixture(scope="module")
def innov(hip):
    """reference(N, family) -> (snapshot, S0, call, reference statistics, their bounds), and the statistics of the default route per case:
    computed once per module, shared by every route"""
    from consistency_helpers import innovation_reference
    from oracle import eqf_numpy as en

    snaps, cases, refs, default, oracle = {}, {}, {}, {}, {}

    def reference(N, fam):
        if (N, fam) not in refs:
            if N not in snaps:
                snaps[N] = rc.device_snapshot(hip, N)
            call = uc.vision_call(N, fam)
            ck = (N, "e" if fam == "e" else "a")
            if ck not in cases:
                cases[ck] = ux.Case(snaps[N], uc.settings(), call[0], call[2])
            S0 = uc.sigma_family(snaps[N], fam)
            ref, bd = cases[ck].reference(S0)
            refs[(N, fam)] = (snaps[N], S0, call) + cx.innovation_stats_reference(ref, bd, cc.C_LOG)
            # the numpy oracle on the same call, through consistency_helpers.innovation_reference: a CPU restatement, printed only
            fo = ec.numpy_filter(en, dict(snaps[N], sigma=S0), uc.settings())
            fo.processVisionData(*call)
            o = innovation_reference(fo.last["S"], fo.last["delta"])
            o["loglik"] = -0.5 * (o["nis"] + o["logdet_S"] + o["m"] * cx.LOG_2PI)
            oracle[(N, fam)] = cx.innovation_ratios(o, *refs[(N, fam)][3:])
        return refs[(N, fam)]

    return reference, default, oracle


def _handle(hip, monkeypatch, env, capacity, batch=1):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    f = hip.FilterBatch(uc.settings(), capacity=capacity, batch=batch)
    for k in env:
        monkeypatch.delenv(k)
    f.set_option("innovation_stats", 1)
    return f


def _one_call(fg, items):
    """items: [(snapshot, S0, call)] per filter -> [innovation_stats(b)]"""
    B = len(items)
    for b, (snap, S0, _) in enumerate(items):
        fg.restore_state(dict(snap, sigma=S0), b)
    calls = [it[2] for it in items]
    stride = max(len(c[1]) for c in calls)
    ids, y = np.zeros((B, stride), dtype=np.int32), np.zeros((B, stride, 3))
    for b, (_, i, yy) in enumerate(calls):
        ids[b, :len(i)], y[b, :len(i)] = i, yy
    st = fg.process_vision([c[0] for c in calls], ids, y, nb=[len(c[1]) for c in calls])
    assert np.all(st == 0), st
    return [fg.innovation_stats(b) for b in range(B)]


def _inside(s, N, val, bnd, what, worst):
    assert s["valid"] and s["dof"] == 2 * N and s["nis_lm"].shape == (N,), what
    r = cx.innovation_ratios(s, val, bnd)
    print(f"C {what}: device / bound " + "  ".join(f"{k} {v:.4f}" for k, v in r.items())
          + f" | bounds: nis {bnd['nis'] / float(val['nis']):.1e} (relative) logdet_S {bnd['logdet_S']:.1e} (absolute)"
          f" nis_lm {np.max(bnd['nis_lm'] / val['nis_lm'].astype(float)):.1e} (relative)")
    for k, v in r.items():
        worst[k] = max(worst.get(k, 0.0), v)
        assert v <= 1.0, (what, k, v)


def _same_bits(s, t, what):
    for k in ("nis", "logdet_S", "loglik", "dof", "valid"):
        assert s[k] == t[k], (what, k, s[k], t[k])
    assert np.array_equal(s["nis_lm"], t["nis_lm"]), what


def _default(hip, monkeypatch, innov, N, fam):
    reference, default, _ = innov
    if (N, fam) not in default:
        snap, S0, call, val, bnd = reference(N, fam)
        fg = _handle(hip, monkeypatch, {}, N + 5)
        (default[(N, fam)],) = _one_call(fg, [(snap, S0, call)])
        assert fg.device_error() == 0
        fg.close()
    return default[(N, fam)]


@pytest.mark.parametrize("N", cc.INNOV_SIZES + tuple(n for n, _ in cc.INNOV_BIG))
def test_innovation_statistics_default_route(hip, monkeypatch, innov, N):
    """Every statistic inside its bound under the default launch shape.  N = 130: m = 260 crosses the 256-stride of the sums of nis and
    logdet_S; N = 257: the stride of nis_lm (its reference takes about fifteen seconds on the CPU, the one case that does)."""
    worst = {}
    for fam in dict(cc.INNOV_BIG).get(N, cc.INNOV_FAMILIES):
        _, _, _, val, bnd = innov[0](N, fam)
        _inside(_default(hip, monkeypatch, innov, N, fam), N, val, bnd, f"default N={N} family {fam}", worst)
        print(f"C         N={N} family {fam}: numpy oracle / bound " + "  ".join(f"{k} {v:.4f}" for k, v in innov[2][(N, fam)].items()))
    print(f"C default route N={N}: worst device / bound " + "  ".join(f"{k} {v:.4f}" for k, v in worst.items()))


@pytest.mark.parametrize("route", ["EQF_CHOL_RESIDENT=0 EQF_CHOL_SPLIT=0", "EQF_CHOL_RESIDENT=0 EQF_CHOL_SPLIT=1", "downdate_slices=6"])
def test_innovation_statistics_are_the_same_bits_under_every_launch_shape(hip, monkeypatch, innov, route):
    env = dict(kv.split("=") for kv in route.split()) if route.startswith("EQF") else {}
    for N in (cc.INNOV_SLICES if not env else cc.INNOV_PER_COLUMN):
        fg = _handle(hip, monkeypatch, env, N + 5)
        if not env:
            fg.set_option("downdate_slices", 6)
        for fam in cc.INNOV_FAMILIES:
            snap, S0, call, _, _ = innov[0](N, fam)
            (s,) = _one_call(fg, [(snap, S0, call)])
            _same_bits(s, _default(hip, monkeypatch, innov, N, fam), (route, N, fam))
        assert fg.device_error() == 0
        fg.close()


def test_innovation_statistics_on_a_ragged_handle_and_in_a_batch(hip, monkeypatch, innov):
    """update_cases.RAGGED (5, 21, 33) in one handle: the filters of a committed size bit for bit their single-filter statistics, N = 33
    inside its own bound; then three filters of N = 21, one family each, bit for bit the single-filter statistics."""
    worst = {}
    fg = _handle(hip, monkeypatch, {}, max(uc.RAGGED) + 5, batch=len(uc.RAGGED))
    items = [innov[0](N, "a") for N in uc.RAGGED]
    for N, it, s in zip(uc.RAGGED, items, _one_call(fg, [it[:3] for it in items])):
        _inside(s, N, it[3], it[4], f"ragged N={N}", worst)
        if N in cc.INNOV_SIZES:
            _same_bits(s, _default(hip, monkeypatch, innov, N, "a"), ("ragged", N))
    assert fg.device_error() == 0
    fg.close()
    N = cc.INNOV_BATCH
    fg = _handle(hip, monkeypatch, {}, N + 5, batch=len(cc.INNOV_FAMILIES))
    items = [innov[0](N, fam) for fam in cc.INNOV_FAMILIES]
    for fam, it, s in zip(cc.INNOV_FAMILIES, items, _one_call(fg, [it[:3] for it in items])):
        _inside(s, N, it[3], it[4], f"batch N={N} family {fam}", worst)
        _same_bits(s, _default(hip, monkeypatch, innov, N, fam), ("batch", fam))
    assert fg.device_error() == 0
    fg.close()
