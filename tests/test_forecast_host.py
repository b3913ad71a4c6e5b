"""What the non-mutating forecast needs on the host, without a GPU: the binding's symbol with its argument types (no handle is created), the
host statements of eqf_vio_amd/consistency.py that go with it (bearing_cov_host, search_ellipse, gate_distance, output_blocks), and the index
arithmetic and argument checks of eqf_vio_amd/csrc/eqf_forecast_host.hpp (host only, standard library only) -- tests/forecast_host_main.cpp
is compiled with g++ under the address and undefined-behaviour sanitizers and run as a child process, cases on stdin, results on stdout.
Every expected value is computed here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = (0, 1, 63, 64, 65, 257)
K_MAX, IMU_REC, LANES, THREADS, STEP_REC, HEAD, BASE, LM_REC = 256, 8, 64, 128, 144, 16, 128, 32


def test_binding_exports_the_symbol_with_its_argument_types():
    from eqf_vio_amd import binding

    assert "eqf_forecast" in binding.EXPORTED_SYMBOLS
    L = binding.lib()
    dp, ip, vp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p
    assert L.eqf_forecast.argtypes == [vp, C.c_int, dp, dp, C.c_int, C.c_int, C.POINTER(binding.ForecastOut), ip]
    names = [f[0] for f in binding.ForecastOut._fields_]
    assert names == ["time", "steps", "pose_q", "pose_x", "velocity", "p", "bearing", "base", "lm", "S", "ycov"] == list(binding.FORECAST_OUTPUTS)
    assert C.sizeof(binding.ForecastOut) == 11 * C.sizeof(vp)
    assert callable(binding.FilterBatch.forecast)
    # refused by the library itself before anything touches a device: a NULL handle, a NULL out
    out = binding.ForecastOut()
    assert L.eqf_forecast(None, 0, None, None, 1, 0, C.byref(out), None) == binding.ERR_INVALID


def test_the_facade_declares_forecast_and_predict_features():
    txt = open(os.path.join(ROOT, "eqf_vio_amd", "cpp", "VIOFilter.h")).read()
    assert "forecast(" in txt and "predictFeatures(" in txt and "eqf_forecast(" in txt


# ---- the host statements
def test_bearing_covariance_search_ellipse_and_gate_distance():
    from eqf_vio_amd import consistency as cs

    rng = np.random.default_rng(5)
    for _ in range(5):
        p = rng.standard_normal(3) * 3 + np.array([0, 0, 6.0])
        A = rng.standard_normal((3, 3))
        P = A @ A.T
        Y = cs.bearing_cov_host(p, P)
        y = p / np.linalg.norm(p)
        assert np.allclose(Y, Y.T, atol=1e-15) and np.abs(Y @ y).max() < 1e-15 * np.abs(Y).max() * 10  # rank 2: yhat is the null vector
        # against central differences of p -> p / |p| pushed through P: every entry of J carries eps / h = 1e-10 of rounding (the
        # truncation, h^2, is smaller), so J P J^T is good to about 1e-10 |J| |P| |J| in every entry, small ones included
        h = 1e-6
        J = np.array([((p + h * e) / np.linalg.norm(p + h * e) - (p - h * e) / np.linalg.norm(p - h * e)) / (2 * h) for e in np.eye(3)]).T
        assert np.abs(Y - J @ P @ J.T).max() <= 1e-8 * (np.abs(J) @ np.abs(P) @ np.abs(J).T).max()
    both = cs.bearing_cov_host(np.array([[0, 0, 2.0], [1, 2, 3.0]]), np.array([np.eye(3), 2 * np.eye(3)]))
    assert both.shape == (2, 3, 3) and np.allclose(both[0], np.diag([0.25, 0.25, 0.0]))
    # a camera looking along z with focal length 500: the bearing covariance diag(a, b, 0) gives axes 500 sqrt(k2 a), 500 sqrt(k2 b), long first
    Jc = 500.0 * np.eye(3)[0:2]
    e = cs.search_ellipse(np.diag([1e-6, 4e-6, 0.0]), Jc, 0.99)
    k2 = cs.chi2_gate_threshold(0.99, 2)
    assert np.allclose(e["cov"], np.diag([0.25, 1.0])) and np.allclose(e["axes"], [np.sqrt(k2), 0.5 * np.sqrt(k2)])
    assert np.allclose(np.abs(e["dirs"]), [[0, 1], [1, 0]])
    with pytest.raises(ValueError):
        cs.search_ellipse(np.eye(3), Jc, 1.0)
    # d2 against the inverse, from the lower triangle only
    S = np.array([[2.0, 99.0], [0.5, 1.0]])
    d = np.array([0.3, -0.2])
    Ssym = np.array([[2.0, 0.5], [0.5, 1.0]])
    assert np.isclose(cs.gate_distance(S, d), d @ np.linalg.solve(Ssym, d), rtol=1e-14)
    assert np.allclose(cs.gate_distance(np.array([Ssym, np.eye(2)]), np.array([d, d])), [d @ np.linalg.solve(Ssym, d), d @ d])


def test_output_blocks_and_forecast_host_against_the_numpy_filter():
    """output_blocks against the dense output matrix C0 of the numpy filter, and forecast_host on that filter: zero horizon gives the
    filter's own estimate and marginals and leaves the filter alone; K samples and t1 give what a copy that ran them holds."""
    import copy

    import consistency_helpers as ch
    from eqf_vio_amd import consistency as cs, synth
    from oracle import eqf_numpy as O

    N = 4
    st = synth.make_stream(N, duration=0.25)
    d = synth.template_settings_dict()
    fo = ch.numpy_filter(d)
    ev = list(st.events())
    cut = [i for i, (kind, _) in enumerate(ev) if kind == "vision"][2] + 3
    for kind, k in ev[:cut]:
        if kind == "imu":
            ch.np_imu(fo, st.imu[k])
        else:
            fo.processVisionData(st.vision_stamps[k], st.ids, st.bearings[k])
    assert len(fo.xi0.ids) == N
    C0 = O.eqf_output_matrix_C(fo.xi0)
    Cb = cs.output_blocks(fo.xi0.p)
    for i in range(N):
        assert np.allclose(Cb[i], C0[2 * i:2 * i + 2, 5 + 3 * i:8 + 3 * i], rtol=1e-14, atol=1e-16)
    before = copy.deepcopy(fo)
    r = d["measurementVariance"]
    z = cs.forecast_host(fo, local=True, measurement_variance=r, sample=O.IMUVelocity)
    est = fo.stateEstimate()
    assert z["steps"] == 0 and z["time"] == fo.getTime() and np.array_equal(z["p"], est.p) and np.array_equal(z["pose_q"], est.pose.q)
    origin, group = ch.origin_group_of(fo)
    J = cs.jacobian_matrix(cs.local_jacobian_blocks(origin, group))
    Sl = J @ fo.Sigma @ J.T
    assert np.allclose(z["base"], Sl[:11, :11], rtol=1e-13, atol=1e-18)
    for i in range(N):
        assert np.allclose(z["lm"][i], Sl[11 + 3 * i:14 + 3 * i, 11 + 3 * i:14 + 3 * i], rtol=1e-13, atol=1e-18)
    Sfull = C0 @ fo.Sigma[6:, 6:] @ C0.T + r * np.eye(2 * N)
    for i in range(N):
        assert np.allclose(z["S"][i], Sfull[2 * i:2 * i + 2, 2 * i:2 * i + 2], rtol=1e-13, atol=1e-18)
    assert np.array_equal(fo.Sigma, before.Sigma) and fo.getTime() == before.getTime()  # the filter itself is only read
    # K = 3 with a repeated stamp in the middle, and t1
    k0 = ev[cut - 1][1]
    imu = np.array([st.imu[k0 + 1], st.imu[k0 + 2], st.imu[k0 + 3]])
    imu[1, 0] = imu[0, 0]
    t1 = imu[2, 0] + 0.004
    z = cs.forecast_host(fo, imu, t1, local=False, measurement_variance=r, sample=O.IMUVelocity)
    twin = copy.deepcopy(fo)
    for row in imu:
        ch.np_imu(twin, row)
    assert twin.integrateUpToTime(t1)
    assert z["steps"] == 3 and z["time"] == t1
    assert np.array_equal(z["base"], twin.Sigma[:11, :11]) and np.array_equal(z["lm"][2], twin.Sigma[17:20, 17:20])
    assert np.array_equal(z["p"], twin.stateEstimate().p) and np.array_equal(z["velocity"], twin.stateEstimate().velocity)
    assert np.array_equal(fo.Sigma, before.Sigma) and fo.getTime() == before.getTime()
    # the default sample type carries the same arithmetic
    z2 = cs.forecast_host(fo, imu, t1, local=False, measurement_variance=r)
    assert np.array_equal(z2["base"], z["base"]) and np.array_equal(z2["p"], z["p"])


# ---- the header under the sanitizers
@pytest.fixture(scope="module")
def forecast_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("forecast_host") / "forecast_host")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "eqf_vio_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "forecast_host_main.cpp")], check=True)

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        return [[int(t) for t in ln.split()] for ln in r.stdout.split("\n")[:-1]]

    return run


def test_header_is_host_only_and_compiles_with_plain_gcc(tmp_path):
    path = os.path.join(ROOT, "eqf_vio_amd", "csrc", "eqf_forecast_host.hpp")
    includes = [ln.split()[1] for ln in open(path) if ln.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "eqf_forecast_host.hpp"\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.dirname(path), str(tu)], check=True)


def test_constants_and_record_layouts(forecast_host):
    c = forecast_host("const")
    assert c[0] == [K_MAX, IMU_REC, LANES, THREADS, STEP_REC, HEAD, BASE, LM_REC]
    # the step record: fields in order, of sizes 1, 1, 1, 9, 3, 7, 3, 3, 66, 6, 24, 15, without overlap and inside the record
    sizes = [1, 1, 1, 9, 3, 7, 3, 3, 66, 6, 24, 15]
    assert c[1] == list(np.concatenate([[0], np.cumsum(sizes)])) and c[1][-1] <= STEP_REC
    assert c[2] == [0, 1, 2, 3, 7, 10] and c[2][-1] + 3 <= HEAD
    assert c[3] == [0, 3, 6, 15, 19, 28] and c[3][-1] < LM_REC and BASE >= 121


def test_grids(forecast_host):
    cases = [(N, B) for N in COUNTS for B in (1, 3, 64)]
    out = forecast_host("\n".join(f"grid {N} {B}" for N, B in cases))
    for (N, B), g in zip(cases, out):
        # one builder workgroup per filter; one lane per landmark, 64 to a workgroup, and never an empty grid
        assert g == [1, B, THREADS, max(1, -(-N // LANES)), B, LANES], (N, B)
    assert [forecast_host(f"grid {N} 1")[0][3] for N in COUNTS] == [1, 1, 1, 1, 2, 5]


def test_layouts(forecast_host):
    for K, t1, B, cap in ((0, 0, 1, 1), (0, 1, 3, 1), (1, 0, 1, 63), (17, 1, 3, 65), (256, 1, 2, 257), (16, 0, 64, 64)):
        out = forecast_host(f"layout {K} {t1} {B} {cap}")
        steps = K + t1
        stride = HEAD + BASE + LM_REC * cap
        assert out[0] == [steps, steps * B * IMU_REC, (K_MAX + 1) * B * IMU_REC, B * (K_MAX + 1) * STEP_REC, stride]
        assert out[1] == [(s * B + b) * IMU_REC for s in range(steps) for b in range(B)]
        assert steps * B * IMU_REC <= (K_MAX + 1) * B * IMU_REC
        # every filter's record: head | base | landmarks, the last landmark's record ending where the next filter's begins
        assert out[2] == [v for b in range(B) for v in (b * stride + HEAD, b * stride + HEAD + BASE, (b + 1) * stride)]
        assert out[3] == [v for b in range(B) for v in (b * (K_MAX + 1) * STEP_REC, (b * (K_MAX + 1) + K_MAX) * STEP_REC)]
        assert out[3][-1] + STEP_REC == out[0][3]
    assert [forecast_host(f"used {N}")[0][0] for N in COUNTS] == [HEAD + BASE + LM_REC * N for N in COUNTS]


def test_pack(forecast_host):
    for K, t1, B in ((0, 1, 2), (2, 0, 3), (3, 1, 2)):
        got = forecast_host(f"pack {K} {t1} {B}")[0]
        want = []
        for k in range(K):
            for b in range(B):
                want += [1000 * k + 10 * b + j + 1 for j in range(7)] + [0]
        if t1:
            for b in range(B):
                want += [7000 + b] + [0] * 7
        assert got == want, (K, t1, B)


def test_argument_checks(forecast_host):
    # head: f out K imu local stride
    heads = [("1 1 0 0 1 0", 1), ("1 1 256 1 0 300", 1), ("0 1 0 0 1 0", 0), ("1 0 0 0 1 0", 0), ("1 1 -1 0 1 0", 0), ("1 1 257 1 1 0", 0),
             ("1 1 3 0 1 0", 0), ("1 1 0 1 1 0", 0), ("1 1 1 1 2 0", 0), ("1 1 1 1 -1 0", 0), ("1 1 1 1 1 -1", 0)]
    # stamps: K B t1? what k b kind
    stamps = [("3 2 1 0 0 0 0", 1), ("3 2 1 1 2 1 1", 0), ("3 2 1 1 0 0 2", 0), ("3 2 1 2 1 1 1", 1), ("3 2 1 3 0 1 1", 0), ("3 2 1 3 0 0 2", 0),
              ("0 2 1 3 0 1 1", 0), ("0 2 0 0 0 0 0", 1), ("3 2 0 0 0 0 0", 1)]
    # stride: p bearing lm S ycov stride B N[B]
    strides = [("0 0 0 0 0 0 3 0 5 65", 1), ("1 0 0 0 0 65 3 0 5 65", 1), ("1 0 0 0 0 64 3 0 5 65", 0), ("0 1 0 0 0 64 3 0 5 65", 0),
               ("0 0 1 0 0 64 3 0 5 65", 0), ("0 0 0 1 0 64 3 0 5 65", 0), ("0 0 0 0 1 64 3 0 5 65", 0), ("0 0 0 0 1 0 2 0 0", 1),
               ("1 1 1 1 1 257 1 257", 1), ("1 1 1 1 1 256 1 257", 0)]
    text = ["head " + c for c, _ in heads] + ["stamps " + c for c, _ in stamps] + ["stride " + c for c, _ in strides]
    got = forecast_host("\n".join(text))
    want = [w for _, w in heads + stamps + strides]
    assert [g[0] for g in got] == want, [(t, g[0], w) for t, g, w in zip(text, got, want) if g[0] != w]
