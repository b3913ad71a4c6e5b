"""The update launch with the lift's regressors as border rows of the E-chain's last block row (k_chol_resident, the co-resident builds;
eqf_debug_option "res_border", eqf_vio_amd/csrc/eqf_border_host.hpp): G11 = [Z_P | E_top]^T Sigma_e^-1 [Z_P | E_top] comes out of the chain's own
tile updates, the E-chain's right-hand-side roles are not run.  Every frame against the structured oracle with the tolerances of
tests/test_gpu_parity.py; Gamma, the state estimate, the bias and Sigma against the same handle with the border off and against the per-column
launches (EQF_CHOL_RESIDENT=0) within the bound of test_resident_update_kernel_equals_the_per_column_launches; two runs bit for bit.
A filter's oracle run is made once and shared by every comparison that needs it."""
import numpy as np
import pytest

from helpers import rel_fro

pytestmark = pytest.mark.gpu

SIGMA_TOL = 1e-7  # tests/test_gpu_parity.py
POSE_TOL = 1e-8
ROUTE_TOL = 1e-9  # test_resident_update_kernel_equals_the_per_column_launches: x max(1, |reference|)
DURATION = 0.4


@pytest.fixture(scope="module")
def hip():
    from eqf_vio_amd import binding

    return binding


_streams, _oracle = {}, {}


def stream(N, seed):
    from eqf_vio_amd import synth

    if (N, seed) not in _streams:
        _streams[(N, seed)] = synth.make_stream(N, seed=seed, duration=DURATION)
    return _streams[(N, seed)]


def oracle_frames(ob, N, seed):
    """(Sigma, x, q) of the oracle after every vision frame of the stream (N, seed): computed once, never changed"""
    from eqf_vio_amd import synth

    if (N, seed) not in _oracle:
        st = stream(N, seed)
        fo = ob.OracleFilter(synth.template_settings_dict(), structured=True)
        frames = []
        for kind, k in st.events():
            if kind == "imu":
                r = st.imu[k]
                fo.processIMUData(r[0], r[1:4], r[4:7])
            else:
                fo.processVisionData(st.vision_stamps[k], st.ids, st.bearings[k])
                e = fo.stateEstimate()
                frames.append((fo.stateCovariance().copy(), np.array(e["x"]), np.array(e["q"])))
        for f in frames:
            for a in f:
                a.setflags(write=False)
        _oracle[(N, seed)] = frames
    return _oracle[(N, seed)]


def run(hip, Ns, seeds, border, ob=None):
    """The streams of the filters (Ns[b], seeds[b]) through ONE handle; with `ob` every frame of every filter is held against the oracle.
    Returns per filter (Sigma, state estimate, bias, last update)."""
    from eqf_vio_amd import synth

    B = len(Ns)
    sts = [stream(Ns[b], seeds[b]) for b in range(B)]
    refs = [oracle_frames(ob, Ns[b], seeds[b]) for b in range(B)] if ob else None
    stride = max(Ns)
    fg = hip.FilterBatch(synth.template_settings_dict(), capacity=stride, batch=B)
    fg.debug_option("res_border", border)
    nf = 0
    for kind, k in sts[0].events():
        if kind == "imu":
            fg.process_imu([s_.imu[k, 0] for s_ in sts], [s_.imu[k, 1:4] for s_ in sts], [s_.imu[k, 4:7] for s_ in sts])
        else:
            ids = np.zeros((B, stride), dtype=np.int32)
            y = np.zeros((B, stride, 3))
            for b in range(B):
                ids[b, : Ns[b]] = sts[b].ids
                y[b, : Ns[b]] = sts[b].bearings[k]
            fg.process_vision([s_.vision_stamps[k] for s_ in sts], ids, y, nb=np.array(Ns, dtype=np.int32))
            if refs:
                for b in range(B):
                    S, x, q = refs[b][nf]
                    eg = fg.state_estimate(b)
                    fro, dx, dq = rel_fro(fg.sigma(b), S), np.abs(x - eg["x"]).max(), np.abs(q - eg["q"]).max()
                    assert fro < SIGMA_TOL and dx < POSE_TOL and dq < POSE_TOL, (Ns, b, nf, fro, dx, dq)
            nf += 1
    assert nf >= 3
    assert fg.device_error() == 0
    return [(fg.sigma(b), fg.state_estimate(b), fg.bias(b), fg.last_update(b)) for b in range(B)]


def assert_close(got, ref, what):
    """the bound of test_resident_update_kernel_equals_the_per_column_launches, filter by filter"""
    for b, (r1, r0) in enumerate(zip(got, ref)):
        fro = rel_fro(r1[0], r0[0])
        est = max(np.abs(r1[1][k] - r0[1][k]).max() for k in r1[1])
        bias = np.abs(r1[2] - r0[2]).max()
        dgam = np.abs(r1[3]["gamma"] - r0[3]["gamma"]).max() / max(1.0, np.abs(r0[3]["gamma"]).max())
        dGam = np.abs(r1[3]["Gamma"] - r0[3]["Gamma"]).max() / max(1.0, np.abs(r0[3]["Gamma"]).max())
        print(f"{what}, filter {b}: Sigma {fro:.2e}, estimate {est:.2e}, bias {bias:.2e}, gamma {dgam:.2e}, Gamma {dGam:.2e}")
        assert fro < ROUTE_TOL and est < ROUTE_TOL and bias < ROUTE_TOL and dgam < ROUTE_TOL and dGam < ROUTE_TOL, (what, b)


def assert_same_bits(got, ref, what):
    for b, (r1, r0) in enumerate(zip(got, ref)):
        assert np.array_equal(r1[0], r0[0]), (what, b, "Sigma")
        assert all(np.array_equal(r1[1][k], r0[1][k]) for k in r1[1]), (what, b, "estimate")
        assert np.array_equal(r1[2], r0[2]), (what, b, "bias")
        assert np.array_equal(r1[3]["gamma"], r0[3]["gamma"]) and np.array_equal(r1[3]["Gamma"], r0[3]["Gamma"]), (what, b, "update")


def eligible(N):
    rem = (6 + 3 * N) % 64
    return N >= 20 and 0 < rem <= 48


def check_against_the_other_routes(ob, hip, monkeypatch, Ns, seeds):
    on = run(hip, Ns, seeds, 1, ob)
    assert_same_bits(run(hip, Ns, seeds, 1), on, "second run with the border")
    off = run(hip, Ns, seeds, 0, ob)
    assert_close(on, off, "border on against off")
    for b, N in enumerate(Ns):
        if not eligible(N):
            assert_same_bits(on[b:b + 1], off[b:b + 1], f"filter {b} takes no border: the old roles, the old bits")
    monkeypatch.setenv("EQF_CHOL_RESIDENT", "0")
    assert_close(on, run(hip, Ns, seeds, 1), "border on against the per-column launches")


@pytest.mark.parametrize("N", [20, 21, 30, 35, 36, 40, 41, 56, 62, 70, 200])
def test_single_filter_sizes(oracle_lib, hip, monkeypatch, N):
    """N = 20: the smallest size with a row head (two block columns, the last head is H(1)); 30: the border starts exactly at a stage
    boundary (order 96); 35 and 56: three real stages, the border in the only free one -- at N = 35 both chains are two block columns long,
    so the handle runs the per-column launches whatever the option says (the comparisons hold trivially), N = 56 (order 174, three block
    columns against two) is the size that runs three real stages in the one-launch kernel; 36, 40 (more than 48 real rows in the last
    block) and 62 (order 192, a multiple of 64) do not take the border: the old roles run, bit for bit what the option switched off gives;
    41: one real row in the last block; 70, 200: two real stages."""
    assert eligible(N) == (N not in (36, 40, 62))
    check_against_the_other_routes(oracle_lib, hip, monkeypatch, (N,), (1234,))


@pytest.mark.parametrize("Ns", [(35, 36), (56, 62), (184, 62)])
def test_ragged_batch_mixes_filters_with_and_without_the_border(oracle_lib, hip, monkeypatch, Ns):
    """Two filters in one handle, one launch: the first takes the border, the second keeps the E-chain's right-hand-side roles.
    (35, 36): both chains of both filters are two block columns long -- the per-column launches, as for one filter of N = 35; (56, 62) is
    the pair of that kind that runs the one-launch kernel (three block columns against two, three real stages in front of the border).
    Two filters of N = 200 (and so the pair (200, 62)) do NOT run co-resident: the role table of N = 200 has 146 roles per filter, 292 for the
    pair, against 256 compute units with one workgroup each -- that batch takes the build for grids larger than the chip, which keeps its
    present code (test_a_grid_larger_than_the_chip_keeps_its_code).  N = 184 (order 558: 46 real rows in the last block, three real stages) is
    the largest filter with border rows whose pair still fits: 114 roles per filter (N = 191 .. 200 have 130 and more; 185 .. 190 take no
    border)."""
    assert eligible(Ns[0]) and not eligible(Ns[1])
    check_against_the_other_routes(oracle_lib, hip, monkeypatch, Ns, (300, 301))


def test_a_grid_larger_than_the_chip_keeps_its_code(hip):
    """(200, 62) in one handle: more roles than compute units, the build with pipelined row heads -- the option changes nothing there"""
    assert_same_bits(run(hip, (200, 62), (300, 301), 1), run(hip, (200, 62), (300, 301), 0), "grid larger than the chip")


@pytest.mark.parametrize("N", [41, 200])
def test_both_coresident_shapes_give_the_same_bits(hip, monkeypatch, N):
    """The prep work as roles of the same launch (the default for one filter) against a prep launch in front (EQF_RES_FOLD_PREP=0), both
    with the border rows"""
    fold = run(hip, (N,), (1234,), 1)
    monkeypatch.setenv("EQF_RES_FOLD_PREP", "0")
    assert_same_bits(run(hip, (N,), (1234,), 1), fold, "prep launch in front")
