"""The covariance downdate of the single-GPU / batched handles on the integer matrix pipe (eqf_set_option "downdate_slices", csrc/eqf_i8.hpp):
Y's columns cut into 7-bit slices, v_mfma_i32_32x32x32_i8 with exact int32 accumulation, fp64 recombination.  "Against fp64" is a second
handle on the same stream with the option off -- the fp64 path itself is pinned to the oracle by the rest of the suite.  The kernels alone
are checked against numpy through eqf_tile_syrk_i8 (include/eqf_vio_amd_debug.h)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-4  # north_star's Sigma tolerance


def _rel(A, B):
    return float(np.linalg.norm(A - B) / np.linalg.norm(B))


def _stream_pair(fa, fb, st):
    """Upload one synthetic stream (B filters share it) to both handles."""
    for f in (fa, fb):
        f.stream_upload(st.imu, st.vision_stamps, st.ids, st.bearings)


def _drive_stream(handles, st, on_frame):
    fr = 0
    for kind, k in st.events():
        for h in handles:
            (h.stream_imu if kind == "imu" else h.stream_vision)(k)
        if kind != "imu":
            on_frame(fr)
            fr += 1
    return fr


def test_cfg2_one_filter_against_fp64_and_the_oracle():
    """BASELINE cfg 2 (N = 200, one filter, 2 s, per-call API) with six slices: Sigma after EVERY update within 1e-4 of the structured fp64
    oracle and of the fp64 handle; pose to 1e-6, the error flag clear, Sigma exactly symmetric, and the integer pipe visibly ran."""
    from eqf_vio_amd import binding, synth
    from oracle import binding as ob

    N = 200
    d = synth.template_settings_dict()
    st = synth.make_stream(N, duration=2.0)
    f8 = binding.FilterBatch(d, capacity=N, batch=1)
    f8.set_option("downdate_slices", 6)
    f64 = binding.FilterBatch(d, capacity=N, batch=1)
    fo = ob.OracleFilter(d, structured=True)
    worst, worst_o, n = 0.0, 0.0, 0
    for kind, k in st.events():
        if kind == "imu":
            r = st.imu[k]
            for f in (f8, f64):
                f.process_imu([r[0]], r[1:4], r[4:7])
            fo.processIMUData(r[0], r[1:4], r[4:7])
        else:
            for f in (f8, f64):
                f.process_vision([st.vision_stamps[k]], st.ids, st.bearings[k])
            fo.processVisionData(st.vision_stamps[k], st.ids, st.bearings[k])
            S8, S0, So = f8.sigma(), f64.sigma(), fo.stateCovariance()
            assert np.array_equal(S8, S8.T)
            worst, worst_o = max(worst, _rel(S8, S0)), max(worst_o, _rel(S8, So))
            n += 1
    e8, eo = f8.state_estimate(), fo.stateEstimate()
    print(f"cfg 2, six slices: worst Sigma deviation over {n} updates {worst:.2e} (fp64 handle), {worst_o:.2e} (oracle)")
    assert n >= 20 and worst <= TOL and worst_o <= TOL
    assert worst > 1e-14  # (the integer pipe really ran)
    assert np.abs(e8["x"] - eo["x"]).max() <= 1e-6 and np.abs(e8["q"] - eo["q"]).max() <= 1e-6
    assert f8.device_error() == 0


def test_cfg4_batch_against_fp64_and_alone():
    """BASELINE cfg 4 (16 filters of N = 200, 1 s, stream mode): every filter, every frame, within 1e-4 of an fp64 batch handle; filter 5
    of the batch agrees with the same stream run alone with the option to 1e-12 (another launch shape, the same downdate)."""
    from eqf_vio_amd import binding, synth

    N, B, bsel = 200, 16, 5
    d = synth.template_settings_dict()
    sts = [synth.make_stream(N, seed=500 + b, duration=1.0) for b in range(B)]
    imu = np.stack([s.imu for s in sts], axis=1)
    vs = np.stack([s.vision_stamps for s in sts], axis=1)
    y = np.stack([s.bearings for s in sts], axis=1)
    f8 = binding.FilterBatch(d, capacity=N, batch=B)
    f8.set_option("downdate_slices", 6)
    f64 = binding.FilterBatch(d, capacity=N, batch=B)
    one = binding.FilterBatch(d, capacity=N, batch=1)
    one.set_option("downdate_slices", 6)
    for f in (f8, f64):
        f.stream_upload(imu, vs, sts[0].ids, y)
    one.stream_upload(sts[bsel].imu, sts[bsel].vision_stamps, sts[bsel].ids, sts[bsel].bearings)
    w = {"batch": 0.0, "alone": 0.0}

    def frame(fr):
        for b in range(B):
            w["batch"] = max(w["batch"], _rel(f8.sigma(b), f64.sigma(b)))
        w["alone"] = max(w["alone"], _rel(one.sigma(), f8.sigma(bsel)))

    n = _drive_stream((f8, f64, one), sts[0], frame)
    print(f"cfg 4, 16 filters, six slices: worst {w['batch']:.2e} against fp64, {w['alone']:.2e} batch against alone")
    assert n >= 10 and w["batch"] <= TOL and w["alone"] <= 1e-12 and w["batch"] > 1e-14
    assert f8.device_error() == 0 and one.device_error() == 0


def test_cfg3_n1000_against_fp64():
    """BASELINE cfg 3 (N = 1000, 0.3 s): within 1e-4 of the fp64 handle after every update."""
    from eqf_vio_amd import binding, synth

    N = 1000
    d = synth.template_settings_dict()
    st = synth.make_stream(N, duration=0.3)
    f8, f64 = binding.FilterBatch(d, capacity=N), binding.FilterBatch(d, capacity=N)
    f8.set_option("downdate_slices", 6)
    _stream_pair(f8, f64, st)
    w = [0.0]
    n = _drive_stream((f8, f64), st, lambda fr: w.__setitem__(0, max(w[0], _rel(f8.sigma(), f64.sigma()))))
    e8, e0 = f8.state_estimate(), f64.state_estimate()
    print(f"N=1000, six slices: worst Sigma deviation over {n} updates {w[0]:.2e}")
    assert n >= 5 and w[0] <= TOL and w[0] > 1e-14 and f8.device_error() == 0
    assert np.abs(e8["x"] - e0["x"]).max() <= 1e-6 and np.abs(e8["q"] - e0["q"]).max() <= 1e-6


def _golden_check(d, f, est, S, tol):
    ref = d["frames"][f]
    assert np.abs(est["q"] - ref[0:4]).max() <= 1e-6 and np.abs(est["x"] - ref[4:7]).max() <= 1e-6, (f, "pose")
    fro, tr = float(np.linalg.norm(S)), float(np.trace(S))
    w = max(abs(fro / ref[16] - 1.0), abs(tr / ref[17] - 1.0))
    smp, want = S[d["sample_rows"], d["sample_cols"]], d["sigma_samples"][f]
    w = max(w, float(np.abs(smp - want).max() / np.abs(want).max()))
    w = max(w, float(np.linalg.norm(S[:11, :11] - d["sigma_base"][f]) / np.linalg.norm(d["sigma_base"][f])))
    assert w <= tol, (f, w)
    return w


@pytest.mark.parametrize("N", [2000, 4000])
def test_large_n_against_the_committed_oracle_vectors(N):
    """The thin margin: N = 2000 / 4000 with six slices against tests/golden/large_N*.npz (pose 1e-6; sampled entries, trace, |Sigma|_F and
    base block 1e-4)."""
    from helpers import events_of, load_golden

    from eqf_vio_amd import binding

    d, settings = load_golden(f"large_N{N}")
    fg = binding.FilterBatch(settings, capacity=N, batch=1)
    fg.set_option("downdate_slices", 6)
    f, worst = 0, 0.0
    for kind, k in events_of(d["imu"], d["vision_stamps"]):
        if kind == "imu":
            r = d["imu"][k]
            fg.process_imu([r[0]], r[1:4], r[4:7])
        else:
            fg.process_vision([d["vision_stamps"][k]], d["ids"], d["bearings"][k])
            S = fg.sigma()
            worst = max(worst, _golden_check(d, f, fg.state_estimate(), S, TOL))
            del S
            f += 1
    print(f"N={N}, six slices: worst deviation from the oracle vectors over {f} updates {worst:.2e}")
    assert f == len(d["vision_stamps"]) and fg.device_error() == 0


def test_n4000_against_fp64_over_six_updates():
    """N = 4000 against the fp64 handle over six updates of a synthetic stream (the partitioned filter's worst frame was the fifth)."""
    from eqf_vio_amd import binding, synth

    N = 4000
    d = synth.template_settings_dict()
    st = synth.make_stream(N, duration=0.36)
    f8, f64 = binding.FilterBatch(d, capacity=N), binding.FilterBatch(d, capacity=N)
    f8.set_option("downdate_slices", 6)
    _stream_pair(f8, f64, st)
    ws = []
    n = _drive_stream((f8, f64), st, lambda fr: ws.append(_rel(f8.sigma(), f64.sigma())))
    print(f"N=4000, six slices: Sigma deviation per update {' '.join(f'{w:.2e}' for w in ws)}")
    assert n >= 6 and max(ws) <= TOL and f8.device_error() == 0


def test_seven_slices_ten_times_closer_than_six():
    from eqf_vio_amd import binding, synth

    N = 200
    d = synth.template_settings_dict()
    st = synth.make_stream(N, duration=1.0)
    hs = [binding.FilterBatch(d, capacity=N) for _ in range(3)]
    hs[1].set_option("downdate_slices", 6)
    hs[2].set_option("downdate_slices", 7)
    for h in hs:
        h.stream_upload(st.imu, st.vision_stamps, st.ids, st.bearings)
    w6, w7 = [0.0], [0.0]

    def frame(fr):
        S0 = hs[0].sigma()
        w6[0] = max(w6[0], _rel(hs[1].sigma(), S0))
        w7[0] = max(w7[0], _rel(hs[2].sigma(), S0))

    _drive_stream(hs, st, frame)
    print(f"N=200: worst deviation six slices {w6[0]:.2e}, seven {w7[0]:.2e}")
    assert w7[0] * 10.0 <= w6[0] <= TOL and w7[0] > 1e-15


def test_churn_same_ids_as_fp64():
    """Landmarks entering and leaving (outlier gate out of reach: 1e9): the landmark ids equal the fp64 handle's every frame, Sigma within 1e-4."""
    from eqf_vio_amd import binding, synth

    N = 60
    d = synth.template_settings_dict()
    d["outlierThreshold"] = 1e9
    st = synth.make_stream(N, duration=1.0)
    meas = synth.churn_measurements(st, seed=3)
    f8, f64 = binding.FilterBatch(d, capacity=N), binding.FilterBatch(d, capacity=N)
    f8.set_option("downdate_slices", 6)
    worst, n = 0.0, 0
    for kind, k in st.events():
        if kind == "imu":
            r = st.imu[k]
            for f in (f8, f64):
                f.process_imu([r[0]], r[1:4], r[4:7])
        else:
            ids, y = meas[k]
            for f in (f8, f64):
                f.process_vision([st.vision_stamps[k]], ids, y)
            assert np.array_equal(f8.ids(), f64.ids()), k
            worst = max(worst, _rel(f8.sigma(), f64.sigma()))
            n += 1
    print(f"churn, six slices: worst Sigma deviation over {n} frames {worst:.2e}")
    assert n >= 10 and worst <= TOL and f8.device_error() == 0


def test_option_semantics():
    from eqf_vio_amd import binding, synth

    L = binding.lib()
    N = 40
    d = synth.template_settings_dict()
    st = synth.make_stream(N, duration=0.4)
    a, b = binding.FilterBatch(d, capacity=N), binding.FilterBatch(d, capacity=N)
    # invalid arguments: no effect, EQF_ERR_INVALID (-1)
    for name, v in (("downdate_slices", 4), ("downdate_slices", 8), ("downdate_slices", -1), ("downdate_slices", 1), ("no_such_option", 0),
                    ("res_tickets", 3), ("res_tickets", -1)):
        assert L.eqf_set_option(a._h, name.encode(), v) == -1, (name, v)
    assert L.eqf_set_option(None, b"downdate_slices", 6) == -1
    assert L.eqf_set_option(a._h, None, 6) == -1
    # on, then off before any update: bit for bit the untouched handle
    a.set_option("downdate_slices", 6)
    a.set_option("downdate_slices", 0)
    for h in (a, b):
        h.stream_upload(st.imu, st.vision_stamps, st.ids, st.bearings)
    n = _drive_stream((a, b), st, lambda fr: None)
    assert n >= 6 and np.array_equal(a.sigma(), b.sigma())
    # fp32 handles: unsupported
    f32 = binding.FilterBatch(d, capacity=N, precision=binding.PRECISION_F32)
    assert L.eqf_set_option(f32._h, b"downdate_slices", 6) == -7


def test_res_tickets_through_the_public_call_bitwise():
    """eqf_set_option "res_tickets" sets what eqf_debug_option sets: 8 filters of N = 200, bit for bit the default."""
    from eqf_vio_amd import binding, synth

    N, B = 200, 8
    sts = [synth.make_stream(N, seed=777 + b, duration=0.36) for b in range(B)]
    d = synth.template_settings_dict()
    out = []
    for tickets in (2, 0):
        fg = binding.FilterBatch(d, capacity=N, batch=B)
        fg.set_option("res_tickets", tickets)
        fg.stream_upload(np.stack([s.imu for s in sts], axis=1), np.stack([s.vision_stamps for s in sts], axis=1), sts[0].ids,
                         np.stack([s.bearings for s in sts], axis=1))
        assert _drive_stream((fg,), sts[0], lambda fr: None) >= 6 and fg.device_error() == 0
        out.append([fg.sigma(b) for b in range(B)])
        fg.close()
    for b in range(B):
        assert np.array_equal(out[0][b], out[1][b]), b


def test_non_finite_sigma_same_pattern_as_fp64():
    """A NaN in one landmark block of filter 1's Sigma (of 2), one update: the same device error bits and the same finite / non-finite pattern
    of each filter's Sigma with the option on as off; filter 0 finite and within 1e-4 of fp64."""
    from eqf_vio_amd import binding, synth

    N = 30
    d = synth.template_settings_dict()
    st = synth.make_stream(N, duration=0.2)
    res = []
    for slices in (6, 0):
        fg = binding.FilterBatch(d, capacity=N, batch=2)
        fg.set_option("downdate_slices", slices)
        frames, poisoned, out = 0, False, None
        for kind, k in st.events():
            if kind == "imu":
                r = st.imu[k]
                fg.process_imu([r[0]], r[1:4], r[4:7])
                continue
            if frames == 2 and not poisoned:
                S = fg.sigma(1)
                S[11 + 3 * 7: 11 + 3 * 8, 11 + 3 * 7: 11 + 3 * 8] = np.nan
                fg.set_sigma(S, 1)
                poisoned = True
            rc = 0
            try:
                fg.process_vision([st.vision_stamps[k]], st.ids, st.bearings[k])
            except binding.EqfError as e:
                rc = e.code
            frames += 1
            if poisoned:
                err = fg.device_error()
                sig = []
                for b in range(2):
                    try:
                        sig.append(fg.sigma(b))
                    except binding.EqfError as e:
                        sig.append(e.code)
                out = (rc, err, sig)
                break
        res.append(out)
        fg.close()
    (rc8, err8, s8), (rc0, err0, s0) = res
    assert rc8 == rc0 and err8 == err0
    for b in range(2):
        if isinstance(s0[b], int) or isinstance(s8[b], int):
            assert s8[b] == s0[b], b
        else:
            assert np.array_equal(np.isfinite(s8[b]), np.isfinite(s0[b])), b
    if not isinstance(s0[0], int):
        assert np.isfinite(s8[0]).all() and _rel(s8[0], s0[0]) <= TOL
    assert not isinstance(s0[1], int) and not np.isfinite(s0[1]).all()  # (the NaN did reach the downdate)


def _syrk(torch, dev, Y, Sin, nv, mp, S):
    """eqf_tile_syrk_i8 on torch tensors Y [B, mpMax, ldY], Sin [B, nvMax, ld]; returns Sout."""
    from eqf_vio_amd import binding

    L = binding.lib()
    B = Y.shape[0]
    Sout = torch.full_like(Sin, 7.0)
    nva, mpa = (C.c_int * B)(*nv), (C.c_int * B)(*mp)
    need = L.eqf_tile_syrk_i8_workspace_bytes(B, max(nv), max(mp), S)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rc = L.eqf_tile_syrk_i8(0, C.c_void_p(torch.cuda.current_stream().cuda_stream), B, nva, mpa, C.c_void_p(Y.data_ptr()), Y.stride(1),
                            Y.stride(0), C.c_void_p(Sin.data_ptr()), C.c_void_p(Sout.data_ptr()), Sin.stride(1), Sin.stride(0), S,
                            C.c_void_p(ws.data_ptr()), need)
    assert rc == 0
    torch.cuda.synchronize()
    return Sout.cpu().numpy()


def test_kernels_against_numpy():
    """eqf_tile_syrk_i8 over batched shapes -- ragged nv / mp, filters of different sizes in one batch, a filter that is only copied, an
    all-zero column, NaN / Inf entries -- against numpy within the statistical bound of tests/test_gpu_tiled.py (random data stay inside it;
    the construction's rigorous bound is larger, tests/i8_emulator.py; bit for bit: tests/test_gpu_i8_exact.py), exact symmetry, nothing
    written outside each filter's nv x nv."""
    import torch

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    for (nv, mp, S) in (((612, 100, 37, 64), (448, 96, 32, 0), 6), ((33, 65, 130), (32, 64, 160), 5), ((1000, 1), (512, 32), 7),
                        ((200, 201, 199, 128, 77, 64, 300, 31), (64, 128, 96, 32, 64, 32, 192, 32), 6)):
        B, nvM, mpM = len(nv), max(nv), max(max(mp), 32)
        ld, ldY = nvM + 3, nvM + 5
        Y = rng.standard_normal((B, mpM, ldY)) * 10.0 ** rng.uniform(-3, 2, size=(B, 1, ldY))
        Sin = rng.standard_normal((B, nvM, ld))
        for b in range(B):
            Sin[b, :, :nvM] = Sin[b, :, :nvM] + Sin[b, :, :nvM].T
        Y[0, :, 3] = 0.0                                  # all-zero column
        bad = {}
        if nv[0] > 20 and B > 1:
            Y[0, mp[0] // 2, 17] = np.nan                     # non-finite entries
            bad[0] = [17]
            if nv[-1] > 9:
                Y[-1, 0, 9] = np.inf
                bad[B - 1] = [9]
        Yd, Sd = torch.from_numpy(Y).to(dev), torch.from_numpy(Sin).to(dev)
        got = _syrk(torch, dev, Yd, Sd, nv, mp, S)
        for b in range(B):
            n, m = nv[b], mp[b]
            G = got[b]
            assert (G[:, n:] == 7.0).all() and (G[n:, :] == 7.0).all(), (nv, b)  # nothing outside nv x nv
            G = G[:n, :n]
            assert np.array_equal(G, G.T, equal_nan=True), (nv, b)
            if m == 0:
                assert np.array_equal(G, Sin[b, :n, :n]), (nv, b)
                continue
            Yb = Y[b, :m, :n].copy()
            cols = bad.get(b, [])
            fin = np.ones(n, dtype=bool)
            fin[cols] = False
            Yb[:, cols] = 0.0
            want = Sin[b, :n, :n] - Yb.T @ Yb
            ca = np.abs(Yb).max(axis=0)
            bound = m * np.outer(ca, ca) * 2.0 ** -(5 + 7 * (S - 1)) * 1.01 + 1e-12 * np.abs(want)
            ok = np.outer(fin, fin)
            assert not np.isfinite(G[~ok]).any(), (nv, b)        # rows / columns of a non-finite column: NaN, as in fp64
            assert (np.abs(G - want)[ok] <= bound[ok]).all(), (nv, b, float(np.abs(G - want)[ok].max()))
            if b == 0:
                assert np.array_equal(G[3][fin], Sin[b, 3, :n][fin]), nv  # (the all-zero column: its row of Sigma is copied exactly)
