"""ctypes binding of libeqf_vio_amd.so (the C ABI declared in include/eqf_vio_amd.h).

There is no CPU fallback: if the shared library is missing or no MI355X is visible, loading /
eqf_create fails loudly.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (EQF_VIO_AMD_LIB: an instrumented build of the same library for the stamp scripts, scripts/README.md -- never a fallback)
LIB_PATH = os.environ.get("EQF_VIO_AMD_LIB") or os.path.join(_HERE, "libeqf_vio_amd.so")

EQF_OK = 0
SKIPPED_BEFORE_FIRST_IMU = 1
SKIPPED_NONPOSITIVE_DT = 2
SKIPPED_NOT_INITIALISED = 3
SKIPPED_NO_BEARINGS = 4
OBS_BEARING, OBS_RANGE, OBS_POSITION = 0, 1, 2  # EQF_OBS_*: the kinds of observe_landmarks
OBS_ROWS = {OBS_BEARING: 2, OBS_RANGE: 1, OBS_POSITION: 3}
ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_CAPACITY, ERR_UNSORTED, ERR_NUMERIC, ERR_UNSUPPORTED = -1, -2, -3, -4, -5, -6, -7
PRECISION_F64, PRECISION_F32 = 0, 1
GATE_CHORD, GATE_MAHALANOBIS = 0, 1
PROF_CLASSES = 15

_ERR_NAMES = {
    -1: "EQF_ERR_INVALID", -2: "EQF_ERR_NO_DEVICE", -3: "EQF_ERR_HIP", -4: "EQF_ERR_CAPACITY",
    -5: "EQF_ERR_UNSORTED", -6: "EQF_ERR_NUMERIC", -7: "EQF_ERR_UNSUPPORTED",
}


class EqfError(RuntimeError):
    def __init__(self, code, what):
        super().__init__(f"{what}: {_ERR_NAMES.get(code, code)}")
        self.code = code


class Settings(C.Structure):
    """eqf_settings == VIOFilter::Settings (eqf_vio/include/eqf_vio/VIOFilterSettings.h:28-54)."""

    _fields_ = [
        ("biasOmegaProcessVariance", C.c_double), ("biasAccelProcessVariance", C.c_double),
        ("gravityProcessVariance", C.c_double), ("velocityProcessVariance", C.c_double),
        ("pointProcessVariance", C.c_double), ("velOmegaVariance", C.c_double), ("velAccelVariance", C.c_double),
        ("measurementVariance", C.c_double), ("initialGravityVariance", C.c_double),
        ("initialVelocityVariance", C.c_double), ("initialPointVariance", C.c_double),
        ("initialBiasOmegaVariance", C.c_double), ("initialBiasAccelVariance", C.c_double),
        ("initialSceneDepth", C.c_double), ("outlierThreshold", C.c_double),
        ("useInnovationLift", C.c_int), ("useDiscreteInnovationLift", C.c_int), ("useDiscreteVelocityLift", C.c_int),
        ("fastRiccati", C.c_int),
        ("initialAccelBias", C.c_double * 3), ("initialOmegaBias", C.c_double * 3),
        ("cameraOffset_x", C.c_double * 3), ("cameraOffset_q", C.c_double * 4),
    ]


class InnovationStats(C.Structure):
    """eqf_innovation_stats (include/eqf_vio_amd.h)."""

    _fields_ = [("nis", C.c_double), ("logdet_S", C.c_double), ("loglik", C.c_double), ("dof", C.c_int), ("valid", C.c_int)]


class SigmaStats(C.Structure):
    """eqf_sigma_stats (include/eqf_vio_amd.h)."""

    _fields_ = [("logdet", C.c_double), ("min_pivot", C.c_double), ("dof", C.c_int), ("info", C.c_int)]


class LinearReport(C.Structure):
    """eqf_linear_report (include/eqf_vio_amd.h)."""

    _fields_ = [("nis", C.c_double), ("logdet_S", C.c_double), ("loglik", C.c_double), ("dof", C.c_int), ("info", C.c_int)]


class IterReport(C.Structure):
    """eqf_iter_report (include/eqf_vio_amd.h)."""

    _fields_ = [("n_lin", C.c_int), ("status", C.c_int), ("last_step", C.c_double)]


class LiftReport(C.Structure):
    """eqf_lift_report (include/eqf_vio_amd.h)."""

    _fields_ = [("kind", C.c_int), ("info", C.c_int), ("DeltaU", C.c_double * 6), ("min_pivot", C.c_double), ("pivot_ratio", C.c_double)]


class ForecastOut(C.Structure):
    """eqf_forecast_out (include/eqf_vio_amd.h)."""

    _fields_ = [("time", C.POINTER(C.c_double)), ("steps", C.POINTER(C.c_int)), ("pose_q", C.POINTER(C.c_double)),
                ("pose_x", C.POINTER(C.c_double)), ("velocity", C.POINTER(C.c_double)), ("p", C.POINTER(C.c_double)),
                ("bearing", C.POINTER(C.c_double)), ("base", C.POINTER(C.c_double)), ("lm", C.POINTER(C.c_double)),
                ("S", C.POINTER(C.c_double)), ("ycov", C.POINTER(C.c_double))]


FORECAST_OUTPUTS = ("time", "steps", "pose_q", "pose_x", "velocity", "p", "bearing", "base", "lm", "S", "ycov")


class MixtureReport(C.Structure):
    """eqf_mixture_report (include/eqf_vio_amd.h)."""

    _fields_ = [("n_eff", C.c_double), ("spread_trace", C.c_double), ("total_trace", C.c_double), ("n", C.c_int), ("info", C.c_int)]


class SplitReport(C.Structure):
    """eqf_split_report (include/eqf_vio_amd.h)."""

    _fields_ = [("S", C.c_double), ("info", C.c_int)]


class PairCost(C.Structure):
    """eqf_pair_cost (include/eqf_vio_amd.h)."""

    _fields_ = [("cost", C.c_double), ("logdet_pair", C.c_double), ("maha", C.c_double), ("info", C.c_int), ("pad_", C.c_int)]


COST_KINDS = {"runnalls": 0, "bhattacharyya": 1}


class FrameScore(C.Structure):
    """eqf_frame_score (include/eqf_vio_amd.h)."""

    _fields_ = [("nis", C.c_double), ("logdet_S", C.c_double), ("loglik", C.c_double), ("dof", C.c_int), ("info", C.c_int)]


class FrameScores:
    """What FilterBatch.score_vision returns: nis, logdet_S, loglik, dof, info as arrays (B, ncand) -- and nis_lm, used (B, ncand, stride)
    when asked for --, by attribute or by key."""

    def __init__(self, **fields):
        self.__dict__.update(fields)

    def __getitem__(self, key):
        return self.__dict__[key]

    def keys(self):
        return self.__dict__.keys()

_lib = None
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_up = C.POINTER(C.c_ubyte)

EXPORTED_SYMBOLS = [
    "eqf_settings_default", "eqf_create", "eqf_destroy", "eqf_reset", "eqf_process_imu", "eqf_process_vision",
    "eqf_stream_upload", "eqf_stream_imu", "eqf_stream_vision", "eqf_synchronize", "eqf_get_time", "eqf_num_landmarks",
    "eqf_get_ids", "eqf_get_state_estimate", "eqf_get_origin", "eqf_get_group", "eqf_get_bias", "eqf_get_sigma",
    "eqf_get_sigma_local", "eqf_get_marginals", "eqf_get_local_jacobian", "eqf_forecast", "eqf_debug_sigma_local_all", "eqf_get_innovation_stats", "eqf_get_nees",
    "eqf_sample_sigma", "eqf_apply_increment", "eqf_perturb_filters", "eqf_update_linear", "eqf_update_landmarks",
    "eqf_get_mixture_moments", "eqf_merge_filters", "eqf_split_filters", "eqf_debug_mixture_launches", "eqf_debug_sigma_pad",
    "eqf_get_merge_costs", "eqf_score_vision", "eqf_get_lift_report", "eqf_edit_landmarks",
    "eqf_update_linear_schmidt", "eqf_update_landmarks_schmidt", "eqf_observe_landmarks",
    "eqf_observe_landmarks_iterated", "eqf_debug_iterate_launches",
    "eqf_set_outlier_gate", "eqf_get_outlier_gate", "eqf_get_gate_report",
    "eqf_set_sigma", "eqf_set_state", "eqf_copy_filters", "eqf_set_camera_offset", "eqf_get_integrator", "eqf_get_last_update", "eqf_debug_get_blocks", "eqf_device_error", "eqf_debug_drop_role", "eqf_debug_option", "eqf_debug_launch_shape", "eqf_set_dense_propagate", "eqf_set_imu_burst", "eqf_set_option", "eqf_profile_enable",
    "eqf_profile_get", "eqf_profile_class_name", "eqf_version", "eqf_build_info", "eqf_tile_propagate", "eqf_tile_downdate", "eqf_tile_potrf", "eqf_tile_trsm", "eqf_tile_gemm_tn", "eqf_tile_mirror", "eqf_tile_downdate_i8", "eqf_tile_gemm_tn_i8", "eqf_tile_i8_workspace_bytes", "eqf_tile_syrk_i8", "eqf_tile_syrk_i8_workspace_bytes", "eqf_stream_create_masked", "eqf_stream_destroy",
    "eqf_tiled_create", "eqf_tiled_destroy", "eqf_tiled_set_stream", "eqf_tiled_set_geometry", "eqf_tiled_propagate", "eqf_tiled_add_landmarks",
    "eqf_tiled_edit_landmarks", "eqf_tiled_propagate_burst", "eqf_tiled_stage_bearings", "eqf_tiled_pingpong",
    "eqf_tiled_update_prep", "eqf_tiled_update_finish", "eqf_tiled_synchronize", "eqf_tiled_num_landmarks", "eqf_tiled_get_time",
    "eqf_tiled_device_error", "eqf_tiled_get_state_estimate", "eqf_tiled_get_origin", "eqf_tiled_get_group", "eqf_tiled_get_bias",
    "eqf_tiled_get_last_update", "eqf_tiled_get_integrator", "eqf_tiled_get_base", "eqf_tiled_set_state",
    "eqf_tf_create", "eqf_tf_destroy", "eqf_tf_set_option", "eqf_tf_process_imu", "eqf_tf_process_vision", "eqf_tf_synchronize", "eqf_tf_check",
    "eqf_tf_device_error", "eqf_tf_num_landmarks", "eqf_tf_num_slots", "eqf_tf_get_ids", "eqf_tf_get_time", "eqf_tf_get_state_estimate",
    "eqf_tf_get_bias", "eqf_tf_get_last_update", "eqf_tf_get_sigma", "eqf_tf_set_state", "eqf_tf_get_churn_stats", "eqf_tf_local_matrix",
    "eqf_tf_get_phases", "eqf_tf_phase_name", "eqf_tf_last_error", "eqf_tf_tiled_handle", "eqf_tf_graph_launches",
]


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  eqf_vio_amd has no CPU fallback."
            )
        # torch wheels ship their own HIP runtime (torch/lib/libamdhip64.so).  A process must end up with ONE runtime: if this library pulled
        # in the system's first, a later `import torch` + torch.cuda initialisation sees "No HIP GPUs" (measured on the MI355X box: the
        # partitioned filter, whose device memory is torch's, created after a FilterBatch).  So when torch is installed it is imported
        # first and this library binds to the runtime torch loaded; hosts without torch get the system runtime as before.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        vp = C.c_void_p
        L.eqf_settings_default.argtypes = [C.POINTER(Settings)]
        L.eqf_settings_default.restype = None
        L.eqf_create.argtypes = [C.POINTER(Settings), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
        L.eqf_destroy.argtypes = [vp]
        L.eqf_destroy.restype = None
        L.eqf_reset.argtypes = [vp]
        L.eqf_process_imu.argtypes = [vp, _dp, _dp, _dp, _ip]
        L.eqf_process_vision.argtypes = [vp, _dp, _ip, _ip, _dp, C.c_int, _ip]
        L.eqf_stream_upload.argtypes = [vp, C.c_int, _dp, C.c_int, _dp, C.c_int, _ip, _dp]
        L.eqf_stream_imu.argtypes = [vp, C.c_int]
        L.eqf_stream_vision.argtypes = [vp, C.c_int]
        L.eqf_synchronize.argtypes = [vp]
        L.eqf_get_time.argtypes = [vp, _dp]
        L.eqf_num_landmarks.argtypes = [vp, C.c_int]
        L.eqf_get_ids.argtypes = [vp, C.c_int, _ip]
        L.eqf_get_state_estimate.argtypes = [vp, C.c_int, _dp, _dp, _dp, _dp]
        L.eqf_get_origin.argtypes = [vp, C.c_int, _dp, _dp, _dp, _dp]
        L.eqf_get_group.argtypes = [vp, C.c_int, _dp, _dp, _dp, _dp, _dp]
        L.eqf_get_bias.argtypes = [vp, C.c_int, _dp]
        L.eqf_get_sigma.argtypes = [vp, C.c_int, _dp, C.c_int]
        L.eqf_set_sigma.argtypes = [vp, C.c_int, _dp, C.c_int]
        if hasattr(L, "eqf_get_sigma_local"):  # (an older build loaded through EQF_VIO_AMD_LIB for an A/B run may predate them)
            L.eqf_get_sigma_local.argtypes = [vp, C.c_int, _dp, C.c_int]
            L.eqf_get_marginals.argtypes = [vp, C.c_int, C.c_int, _dp, _dp]
            L.eqf_get_local_jacobian.argtypes = [vp, C.c_int, _dp, _dp, _dp]
            L.eqf_forecast.argtypes = [vp, C.c_int, _dp, _dp, C.c_int, C.c_int, C.POINTER(ForecastOut), _ip]
            L.eqf_debug_sigma_local_all.argtypes = [vp]
            L.eqf_get_innovation_stats.argtypes = [vp, C.c_int, C.POINTER(InnovationStats), _dp]
        if hasattr(L, "eqf_get_nees"):
            L.eqf_get_nees.argtypes = [vp, C.c_int, C.c_int, C.c_int, _dp, C.c_int, _dp, C.POINTER(SigmaStats)]
        if hasattr(L, "eqf_sample_sigma"):  # (an older build loaded through EQF_VIO_AMD_LIB for an A/B run may predate them)
            L.eqf_sample_sigma.argtypes = [vp, C.c_int, C.c_int, C.c_int, _dp, C.c_int, _dp, _dp, C.c_int, C.POINTER(SigmaStats)]
            L.eqf_apply_increment.argtypes = [vp, _dp, C.c_int, C.POINTER(C.c_ubyte)]
            L.eqf_perturb_filters.argtypes = [vp, C.c_int, _dp, C.c_int, _dp, C.POINTER(SigmaStats)]
        if hasattr(L, "eqf_update_linear"):  # (an older build loaded through EQF_VIO_AMD_LIB for an A/B run may predate it)
            L.eqf_update_linear.argtypes = [vp, C.c_int, C.c_int, _dp, C.c_int, _dp, _dp, C.c_double, C.POINTER(C.c_ubyte), _dp, C.c_int,
                                            C.POINTER(LinearReport)]
        if hasattr(L, "eqf_update_landmarks"):  # (an older build loaded through EQF_VIO_AMD_LIB for an A/B run may predate it)
            L.eqf_update_landmarks.argtypes = [vp, C.c_int, C.c_int, _ip, _ip, C.c_int, _dp, _dp, _dp, C.c_double, C.c_double,
                                               C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte), _dp, C.c_int, C.POINTER(LinearReport)]
        if hasattr(L, "eqf_update_linear_schmidt"):  # (an older build loaded through EQF_VIO_AMD_LIB for an A/B run may predate them)
            L.eqf_update_linear_schmidt.argtypes = [vp, C.c_int, C.c_int, _dp, C.c_int, _dp, _dp, C.c_double, C.POINTER(C.c_ubyte), _ip, _ip,
                                                    C.c_int, _dp, C.c_int, C.POINTER(LinearReport)]
            L.eqf_update_landmarks_schmidt.argtypes = [vp, C.c_int, C.c_int, _ip, _ip, C.c_int, _dp, _dp, _dp, C.c_double, C.c_double,
                                                       C.POINTER(C.c_ubyte), _ip, _ip, C.c_int, C.POINTER(C.c_ubyte), _dp, C.c_int,
                                                       C.POINTER(LinearReport)]
        if hasattr(L, "eqf_observe_landmarks"):  # (an older build loaded through EQF_VIO_AMD_LIB for an A/B run may predate it)
            L.eqf_observe_landmarks.argtypes = [vp, C.c_int, _dp, C.c_int, _ip, _ip, C.c_int, _dp, _dp, C.c_double, C.c_double,
                                                C.POINTER(C.c_ubyte), _ip, _ip, C.c_int, C.POINTER(C.c_ubyte), _dp, _dp, _dp, C.c_int,
                                                C.POINTER(LinearReport)]
        if hasattr(L, "eqf_observe_landmarks_iterated"):  # (an older build loaded through EQF_VIO_AMD_LIB for an A/B run may predate it)
            L.eqf_observe_landmarks_iterated.argtypes = [vp, C.c_int, _dp, C.c_int, _ip, _ip, C.c_int, _dp, _dp, C.c_double, C.c_double,
                                                         C.POINTER(C.c_ubyte), _ip, _ip, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_ubyte),
                                                         _dp, _dp, _dp, C.c_int, C.POINTER(LinearReport), _dp, C.POINTER(IterReport)]
            L.eqf_debug_iterate_launches.argtypes = [vp]
        if hasattr(L, "eqf_merge_filters"):  # (an older build loaded through EQF_VIO_AMD_LIB for an A/B run may predate them)
            L.eqf_get_mixture_moments.argtypes = [vp, C.c_int, _ip, _dp, C.c_int, C.c_int, _dp, _dp, C.c_int, C.POINTER(MixtureReport)]
            L.eqf_merge_filters.argtypes = [vp, C.c_int, _ip, _dp, C.c_int, C.c_int, C.POINTER(MixtureReport)]
            L.eqf_debug_mixture_launches.argtypes = [vp]
            L.eqf_debug_sigma_pad.argtypes = [vp, C.c_int, C.c_int, _dp]
        if hasattr(L, "eqf_split_filters"):  # (an older build loaded through EQF_VIO_AMD_LIB for an A/B run may predate it)
            L.eqf_split_filters.argtypes = [vp, C.c_int, _dp, C.c_int, C.c_int, _ip, _ip, _dp, _dp, _dp, C.c_int, C.POINTER(SplitReport)]
        if hasattr(L, "eqf_get_merge_costs"):  # (an older build loaded through EQF_VIO_AMD_LIB for an A/B run may predate it)
            L.eqf_get_merge_costs.argtypes = [vp, C.c_int, _ip, _dp, C.c_int, C.c_int, C.c_int, C.c_int, _ip, C.POINTER(PairCost),
                                              C.POINTER(SigmaStats)]
        if hasattr(L, "eqf_score_vision"):  # (an older build loaded through EQF_VIO_AMD_LIB for an A/B run may predate it)
            L.eqf_score_vision.argtypes = [vp, C.c_int, _ip, _ip, _dp, C.c_int, C.POINTER(C.c_ubyte), C.POINTER(FrameScore), _dp,
                                           C.POINTER(C.c_ubyte)]
        if hasattr(L, "eqf_get_lift_report"):  # (an older build loaded through EQF_VIO_AMD_LIB for an A/B run may predate it)
            L.eqf_get_lift_report.argtypes = [vp, C.c_int, C.POINTER(LiftReport)]
        if hasattr(L, "eqf_edit_landmarks"):  # (an older build loaded through EQF_VIO_AMD_LIB for an A/B run may predate it)
            L.eqf_edit_landmarks.argtypes = [vp, _ip, _ip, C.c_int, _ip, _ip, C.c_int, _dp, _dp, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]
        if hasattr(L, "eqf_set_outlier_gate"):  # (an older build loaded through EQF_VIO_AMD_LIB for an A/B run may predate them)
            L.eqf_set_outlier_gate.argtypes = [vp, C.c_int, C.c_double]
            L.eqf_get_outlier_gate.argtypes = [vp, _ip, _dp]
            L.eqf_get_gate_report.argtypes = [vp, C.c_int, _ip, _ip, _dp, _ip]
        L.eqf_get_last_update.argtypes = [vp, C.c_int, _dp, _dp, _dp]
        L.eqf_set_state.argtypes = [vp, C.c_int, C.c_int, _ip] + [_dp] * 11 + [C.c_int, C.c_double, _dp, _dp, C.c_double, C.c_int]
        L.eqf_get_integrator.argtypes = [vp, C.c_int, _dp, _dp, _dp, _ip]
        if hasattr(L, "eqf_copy_filters"):  # (an older build loaded through EQF_VIO_AMD_LIB for an A/B run may predate it)
            L.eqf_copy_filters.argtypes = [vp, vp, C.c_int, _ip, _ip]
        L.eqf_debug_get_blocks.argtypes = [vp, C.c_int, _dp, _dp, _dp]
        L.eqf_device_error.argtypes = [vp]
        L.eqf_debug_drop_role.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
        L.eqf_debug_option.argtypes = [vp, C.c_char_p, C.c_int]
        if hasattr(L, "eqf_debug_launch_shape"):  # (an older build loaded through EQF_VIO_AMD_LIB for an A/B run may predate it)
            L.eqf_debug_launch_shape.argtypes = [vp, C.POINTER(C.c_int)]
        L.eqf_set_dense_propagate.argtypes = [vp, C.c_int]
        L.eqf_set_imu_burst.argtypes = [vp, C.c_int]
        if hasattr(L, "eqf_set_option"):  # (an older build loaded through EQF_VIO_AMD_LIB for an A/B run may predate it)
            L.eqf_set_option.argtypes = [vp, C.c_char_p, C.c_int]
        L.eqf_profile_enable.argtypes = [vp, C.c_int]
        L.eqf_profile_get.argtypes = [vp, C.c_int, C.POINTER(C.c_longlong), _dp]
        L.eqf_profile_class_name.argtypes = [C.c_int]
        L.eqf_profile_class_name.restype = C.c_char_p
        L.eqf_version.restype = C.c_char_p
        L.eqf_build_info.restype = C.c_char_p
        vpp = C.c_void_p
        L.eqf_tile_propagate.argtypes = [C.c_int, vpp, vpp, vpp, C.c_int, C.c_int, C.c_int, vpp, vpp, vpp, vpp, vpp, vpp, C.c_int, vpp, C.c_int,
                                         vpp, vpp, _dp, C.c_double, C.c_double, C.c_int]
        L.eqf_tile_downdate.argtypes = [C.c_int, vpp, vpp, C.c_int, C.c_int, C.c_int, vpp, C.c_int, vpp, C.c_int, C.c_int]
        L.eqf_tile_potrf.argtypes = [C.c_int, vpp, vpp, C.c_int, C.c_int, vpp, vpp]
        L.eqf_tile_trsm.argtypes = [C.c_int, vpp, vpp, C.c_int, C.c_int, vpp, vpp, C.c_int, C.c_int, C.c_int]
        L.eqf_tile_gemm_tn.argtypes = [C.c_int, vpp, vpp, C.c_int, C.c_int, C.c_int, vpp, C.c_int, vpp, C.c_int, C.c_int, C.c_double] + [C.c_int] * 8
        L.eqf_tile_mirror.argtypes = [C.c_int, vpp, vpp, C.c_int, C.c_int, C.c_int]
        if hasattr(L, "eqf_tile_downdate_i8"):  # (an older build loaded through EQF_VIO_AMD_LIB may predate it)
            L.eqf_tile_i8_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
            L.eqf_tile_i8_workspace_bytes.restype = C.c_size_t
            L.eqf_tile_downdate_i8.argtypes = [C.c_int, vpp, vpp, C.c_int, C.c_int, C.c_int, vpp, C.c_int, vpp, C.c_int, C.c_int, C.c_int, C.c_int, vpp, C.c_size_t]
        if hasattr(L, "eqf_tile_gemm_tn_i8"):
            L.eqf_tile_gemm_tn_i8.argtypes = [C.c_int, vpp, vpp, C.c_int, C.c_int, C.c_int, vpp, C.c_int, vpp, C.c_int, C.c_int, C.c_int] + [C.c_int] * 9 + [vpp, C.c_size_t]
        if hasattr(L, "eqf_tile_syrk_i8"):
            L.eqf_tile_syrk_i8_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
            L.eqf_tile_syrk_i8_workspace_bytes.restype = C.c_size_t
            L.eqf_tile_syrk_i8.argtypes = [C.c_int, vpp, C.c_int, _ip, _ip, vpp, C.c_int, C.c_longlong, vpp, vpp, C.c_int, C.c_longlong, C.c_int,
                                           vpp, C.c_size_t]
        L.eqf_stream_create_masked.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vpp)]
        L.eqf_stream_destroy.argtypes = [C.c_int, vpp]
        # the 2-D block-partitioned filter (BASELINE configs[4]); device buffers are plain pointers (torch tensors' data_ptr)
        L.eqf_tiled_create.argtypes = [C.POINTER(Settings), C.c_int, C.c_int, C.POINTER(vp)]
        L.eqf_tiled_destroy.argtypes = [vp]
        L.eqf_tiled_destroy.restype = None
        L.eqf_tiled_set_stream.argtypes = [vp, vpp]
        L.eqf_tiled_set_geometry.argtypes = [vp, C.c_int, _ip, C.c_int, _ip]
        L.eqf_tiled_propagate.argtypes = [vp, C.c_double, _dp, _dp, C.c_int, vpp, C.c_int]
        L.eqf_tiled_add_landmarks.argtypes = [vp, C.c_int, _dp, vpp, C.c_int]
        L.eqf_tiled_propagate_burst.argtypes = [vp, C.c_int, _dp, _dp, _dp, C.c_int, vpp, C.c_int, _ip]
        L.eqf_tiled_edit_landmarks.argtypes = [vp, C.c_int, _ip, C.c_int, _ip, _dp, C.c_double, C.c_int, vpp, C.c_int]
        L.eqf_tiled_update_prep.argtypes = [vp, _dp, vpp, C.c_int, vpp, C.c_int, vpp, C.c_int, vpp]
        L.eqf_tiled_update_finish.argtypes = [vp, vpp, C.c_int, vpp, vpp]
        L.eqf_tiled_synchronize.argtypes = [vp]
        L.eqf_tiled_num_landmarks.argtypes = [vp]
        L.eqf_tiled_get_time.argtypes = [vp, _dp]
        L.eqf_tiled_device_error.argtypes = [vp]
        L.eqf_tiled_get_state_estimate.argtypes = [vp, _dp, _dp, _dp, _dp]
        L.eqf_tiled_get_origin.argtypes = [vp, _dp, _dp, _dp, _dp]
        L.eqf_tiled_get_group.argtypes = [vp, _dp, _dp, _dp, _dp, _dp]
        L.eqf_tiled_get_bias.argtypes = [vp, _dp]
        L.eqf_tiled_get_last_update.argtypes = [vp, _dp, _dp, _dp]
        L.eqf_tiled_get_integrator.argtypes = [vp, _dp, _dp, _dp, _ip]
        L.eqf_tiled_get_base.argtypes = [vp, _dp, C.c_int]
        L.eqf_tiled_set_state.argtypes = [vp, C.c_int] + [_dp] * 11 + [C.c_int, C.c_double, _dp, _dp, C.c_double, C.c_int]
        _lib = L
    return _lib


def build_info():
    """Which library this process loaded and whether it was built from the sources beside it: sha256 of the .so, the source hash the
    library carries (eqf_build_info) and the same hash recomputed now over csrc/*.hip, csrc/*.hpp, include/*.h, csrc/Makefile."""
    import glob
    import hashlib

    L = lib()
    with open(LIB_PATH, "rb") as f:
        so = hashlib.sha256(f.read()).hexdigest()
    embedded = L.eqf_build_info().decode().split("=", 1)[1]
    csrc = os.path.join(_HERE, "csrc")
    names = sorted([os.path.basename(p) for p in glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.hpp"))]
                   + ["../../include/eqf_vio_amd.h", "../../include/eqf_vio_amd_debug.h", "Makefile"])  # (the order of the Makefile's $(sort ...))
    h = hashlib.sha256()
    for n in names:
        with open(os.path.join(csrc, n), "rb") as f:
            h.update(f.read())
    now = h.hexdigest()
    return {"library": os.path.relpath(LIB_PATH, os.path.dirname(_HERE)), "so_sha256": so, "src_sha256_in_library": embedded,
            "src_sha256_now": now, "library_matches_sources": embedded == now}


def default_settings():
    s = Settings()
    lib().eqf_settings_default(C.byref(s))
    return s


def settings_from_dict(d):
    """Reference setting names -> eqf_settings; unknown keys raise."""
    s = default_settings()
    for k, v in d.items():
        if k in ("initialAccelBias", "initialOmegaBias", "cameraOffset_x", "cameraOffset_q"):
            arr = getattr(s, k)
            for i, x in enumerate(np.asarray(v, dtype=float)):
                arr[i] = x
        elif hasattr(s, k):
            setattr(s, k, int(bool(v)) if k.startswith("use") or k == "fastRiccati" else float(v))
        else:
            raise AttributeError(k)
    return s


def _p(a):
    return a.ctypes.data_as(_dp)


def _pn(a, ptr=_dp):
    """an optional array (None: NULL) as a pointer"""
    return None if a is None else a.ctypes.data_as(ptr)


def _check(rc, what):
    if rc < 0:
        raise EqfError(rc, what)
    return rc


class FilterBatch:
    """A batch of independent EqF filters on one MI355X (one handle, one HIP stream)."""

    def __init__(self, settings, capacity, batch=1, device=0, precision=PRECISION_F64):
        if isinstance(settings, dict):
            settings = settings_from_dict(settings)
        self.settings = settings
        self.B = int(batch)
        self.cap = int(capacity)
        self._h = C.c_void_p()
        _check(lib().eqf_create(C.byref(settings), self.cap, self.B, int(device), int(precision), C.byref(self._h)), "eqf_create")

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().eqf_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- inputs
    def process_imu(self, stamps, omega, accel):
        st = np.ascontiguousarray(np.broadcast_to(np.asarray(stamps, dtype=np.float64), (self.B,)))
        w = np.ascontiguousarray(np.broadcast_to(np.asarray(omega, dtype=np.float64), (self.B, 3)))
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(accel, dtype=np.float64), (self.B, 3)))
        status = np.zeros(self.B, dtype=np.int32)
        _check(lib().eqf_process_imu(self._h, _p(st), _p(w), _p(a), status.ctypes.data_as(_ip)), "eqf_process_imu")
        return status

    def process_vision(self, stamps, ids, bearings, nb=None):
        """ids: (B, stride) or (stride,) ascending; bearings: (B, stride, 3) or (stride, 3)."""
        ids = np.asarray(ids, dtype=np.int32)
        y = np.asarray(bearings, dtype=np.float64)
        if ids.ndim == 1:
            ids = np.broadcast_to(ids, (self.B, ids.shape[0]))
        if y.ndim == 2:
            y = np.broadcast_to(y, (self.B,) + y.shape)
        ids = np.ascontiguousarray(ids)
        y = np.ascontiguousarray(y)
        stride = ids.shape[1]
        nbv = np.full(self.B, stride, dtype=np.int32) if nb is None else np.ascontiguousarray(nb, dtype=np.int32)
        st = np.ascontiguousarray(np.broadcast_to(np.asarray(stamps, dtype=np.float64), (self.B,)))
        status = np.zeros(self.B, dtype=np.int32)
        _check(
            lib().eqf_process_vision(self._h, _p(st), nbv.ctypes.data_as(_ip), ids.ctypes.data_as(_ip), _p(y), stride,
                                     status.ctypes.data_as(_ip)),
            "eqf_process_vision",
        )
        return status

    def stream_upload(self, imu, vstamps, ids, bearings):
        """imu (K,B,7) or (K,7); vstamps (F,B) or (F,); ids (nb,); bearings (F,B,nb,3) or (F,nb,3)."""
        imu = np.asarray(imu, dtype=np.float64)
        if imu.ndim == 2:
            imu = np.broadcast_to(imu[:, None, :], (imu.shape[0], self.B, 7))
        vs = np.asarray(vstamps, dtype=np.float64)
        if vs.ndim == 1:
            vs = np.broadcast_to(vs[:, None], (vs.shape[0], self.B))
        y = np.asarray(bearings, dtype=np.float64)
        if y.ndim == 3:
            y = np.broadcast_to(y[:, None], (y.shape[0], self.B) + y.shape[1:])
        imu, vs, y = np.ascontiguousarray(imu), np.ascontiguousarray(vs), np.ascontiguousarray(y)
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        _check(
            lib().eqf_stream_upload(self._h, imu.shape[0], _p(imu), vs.shape[0], _p(vs), len(ids), ids.ctypes.data_as(_ip), _p(y)),
            "eqf_stream_upload",
        )

    def stream_imu(self, k):
        return _check(lib().eqf_stream_imu(self._h, int(k)), "eqf_stream_imu")

    def stream_vision(self, f):
        return _check(lib().eqf_stream_vision(self._h, int(f)), "eqf_stream_vision")

    def set_dense_propagate(self, on=True):
        """Riccati step as dense F Sigma F^T on the matrix cores (BASELINE cfg 3 cross-check backend)."""
        _check(lib().eqf_set_dense_propagate(self._h, int(bool(on))), "eqf_set_dense_propagate")

    def set_imu_burst(self, max_steps):
        """IMU calls are queued and launched as bursts of up to `max_steps` steps (0: one launch per call); see
        include/eqf_vio_amd.h."""
        _check(lib().eqf_set_imu_burst(self._h, int(max_steps)), "eqf_set_imu_burst")

    def set_option(self, name, value):
        """Handle option by name (include/eqf_vio_amd.h: eqf_set_option): ``"downdate_slices"`` 0 (fp64, default) / 5 / 6 / 7 -- the
        covariance downdate on the integer matrix pipe from that many 7-bit slices (6 holds Sigma within 1e-4 of fp64, 5 does not) --
        ``"res_tickets"`` 0 / 1 / 2, ``"innovation_stats"`` 0 / 1 (innovation_stats()), or ``"innovation_lift"`` 0 / 1: with 1
        update_linear, update_landmarks, apply_increment and perturb move the pose by the handle's innovation lift (lift_report())."""
        _check(lib().eqf_set_option(self._h, name.encode(), int(value)), "eqf_set_option")

    def synchronize(self):
        _check(lib().eqf_synchronize(self._h), "eqf_synchronize")

    def reset(self):
        _check(lib().eqf_reset(self._h), "eqf_reset")

    # ---- outputs
    def num_landmarks(self, b=0):
        return _check(lib().eqf_num_landmarks(self._h, b), "eqf_num_landmarks")

    def get_time(self):
        t = np.zeros(self.B)
        _check(lib().eqf_get_time(self._h, _p(t)), "eqf_get_time")
        return t

    def ids(self, b=0):
        out = np.zeros(self.num_landmarks(b), dtype=np.int32)
        _check(lib().eqf_get_ids(self._h, b, out.ctypes.data_as(_ip)), "eqf_get_ids")
        return out

    def _state(self, fn, b, what):
        N = self.num_landmarks(b)
        q, x, v, p = np.zeros(4), np.zeros(3), np.zeros(3), np.zeros((max(N, 1), 3))
        _check(fn(self._h, b, _p(q), _p(x), _p(v), _p(p)), what)
        return dict(q=q, x=x, v=v, p=p[:N])

    def state_estimate(self, b=0):
        return self._state(lib().eqf_get_state_estimate, b, "eqf_get_state_estimate")

    def origin(self, b=0):
        return self._state(lib().eqf_get_origin, b, "eqf_get_origin")

    def group(self, b=0):
        N = self.num_landmarks(b)
        Aq, Ax, w = np.zeros(4), np.zeros(3), np.zeros(3)
        Qq, Qa = np.zeros((max(N, 1), 4)), np.zeros(max(N, 1))
        _check(lib().eqf_get_group(self._h, b, _p(Aq), _p(Ax), _p(w), _p(Qq), _p(Qa)), "eqf_get_group")
        return dict(Aq=Aq, Ax=Ax, w=w, Qq=Qq[:N], Qa=Qa[:N])

    def bias(self, b=0):
        out = np.zeros(6)
        _check(lib().eqf_get_bias(self._h, b, _p(out)), "eqf_get_bias")
        return out

    def sigma(self, b=0):
        n = 11 + 3 * self.num_landmarks(b)
        out = np.zeros((n, n))
        _check(lib().eqf_get_sigma(self._h, b, _p(out), n), "eqf_get_sigma")
        return out

    def sigma_local(self, b=0):
        """Sigma in the coordinates of the estimate, J Sigma J^T (include/eqf_vio_amd.h: eqf_get_sigma_local); layout of sigma()."""
        n = 11 + 3 * self.num_landmarks(b)
        out = np.zeros((n, n))
        _check(lib().eqf_get_sigma_local(self._h, b, _p(out), n), "eqf_get_sigma_local")
        return out

    def marginals(self, b=0, local=True):
        """The 11 x 11 base block and the N diagonal 3 x 3 landmark blocks of sigma_local() (local) or sigma(), O(N)."""
        N = self.num_landmarks(b)
        base, lm = np.zeros((11, 11)), np.zeros((max(N, 1), 3, 3))
        _check(lib().eqf_get_marginals(self._h, b, int(bool(local)), _p(base), _p(lm)), "eqf_get_marginals")
        return dict(base=base, lm=lm[:N])

    def local_jacobian(self, b=0):
        """The blocks of J (origin chart -> estimate chart) as the device built them: G (2,2), RAt (3,3), lm (N,3,3)."""
        N = self.num_landmarks(b)
        G, RAt, lm = np.zeros((2, 2)), np.zeros((3, 3)), np.zeros((max(N, 1), 3, 3))
        _check(lib().eqf_get_local_jacobian(self._h, b, _p(G), _p(RAt), _p(lm)), "eqf_get_local_jacobian")
        return dict(G=G, RAt=RAt, lm=lm[:N])

    def forecast(self, imu=None, t1=None, local=True, want=FORECAST_OUTPUTS):
        """Where the state and the features will be after the IMU samples `imu` ((K, B, 7) or (K, 7): stamp, omega, accel) and, where `t1`
        (scalar or (B,)) is given, the integration up to t1 with which a vision call begins -- without changing the handle
        (include/eqf_vio_amd.h: eqf_forecast; consistency.forecast_host).  Returns a dict: ``status`` (B,) and, for every name in `want`,
        a list with one array per filter, the per-landmark ones trimmed to that filter's N: time, steps, pose_q (4,), pose_x (3,),
        velocity (3,), p (N, 3), bearing (N, 3), base (11, 11), lm (N, 3, 3) -- base and lm in the estimate's chart (local) or the origin's
        -- S (N, 2, 2) = C_i Sigma_ii C_i^T + r I, ycov (N, 3, 3) the covariance of the unit bearing."""
        unknown = [w for w in want if w not in FORECAST_OUTPUTS]
        if unknown:
            raise ValueError(f"unknown forecast outputs {unknown}")
        B = self.B
        K = 0
        imu_p = None
        if imu is not None:
            imu = np.asarray(imu, dtype=np.float64)
            if imu.ndim == 2:
                imu = np.broadcast_to(imu[:, None, :], (imu.shape[0], B, 7))
            if imu.ndim != 3 or imu.shape[1:] != (B, 7):
                raise ValueError(f"imu must have shape (K, {B}, 7) or (K, 7)")
            imu = np.ascontiguousarray(imu)
            K = imu.shape[0]
            imu_p = _p(imu) if K else None
        t1_p = None
        if t1 is not None:
            t1 = np.ascontiguousarray(np.broadcast_to(np.asarray(t1, dtype=np.float64), (B,)))
            t1_p = _p(t1)
        Ns = [self.num_landmarks(b) for b in range(B)]
        stride = max(Ns + [1])
        shapes = dict(time=(B,), pose_q=(B, 4), pose_x=(B, 3), velocity=(B, 3), p=(B, stride, 3), bearing=(B, stride, 3), base=(B, 11, 11),
                      lm=(B, stride, 3, 3), S=(B, stride, 2, 2), ycov=(B, stride, 3, 3))
        bufs = {w: (np.zeros(B, dtype=np.int32) if w == "steps" else np.zeros(shapes[w])) for w in want}
        out = ForecastOut()
        for w, a in bufs.items():
            setattr(out, w, a.ctypes.data_as(_ip if w == "steps" else _dp))
        status = np.zeros(B, dtype=np.int32)
        _check(lib().eqf_forecast(self._h, K, imu_p, t1_p, int(bool(local)), stride, C.byref(out), status.ctypes.data_as(_ip)), "eqf_forecast")
        res = dict(status=status)
        for w, a in bufs.items():
            per_lm = w in ("p", "bearing", "lm", "S", "ycov")
            res[w] = [a[b, :Ns[b]] if per_lm else a[b] for b in range(B)]  # (views of the call's own buffers: nothing else holds them)
        return res

    def innovation_stats(self, b=0):
        """Statistics of filter b's most recent vision update (set_option("innovation_stats", 1) first): dict with nis, logdet_S, loglik,
        dof, valid and nis_lm (N,); include/eqf_vio_amd.h: eqf_get_innovation_stats."""
        N = self.num_landmarks(b)
        st, lm = InnovationStats(), np.zeros(max(N, 1))
        _check(lib().eqf_get_innovation_stats(self._h, b, C.byref(st), _p(lm)), "eqf_get_innovation_stats")
        return dict(nis=st.nis, logdet_S=st.logdet_S, loglik=st.loglik, dof=st.dof, valid=bool(st.valid), nis_lm=lm[:N] if st.valid else np.zeros(0))

    def set_outlier_gate(self, kind, threshold):
        """The handle's outlier gate (include/eqf_vio_amd.h: eqf_set_outlier_gate): GATE_CHORD, the reference's chord between measured and
        predicted bearing, or GATE_MAHALANOBIS, d2 = delta_i^T (C_i Sigma_ii C_i^T + r I)^-1 delta_i (chi-square with 2 degrees of freedom:
        consistency.chi2_gate_threshold(p)); a landmark goes when its number exceeds `threshold`.  From the next vision call on."""
        _check(lib().eqf_set_outlier_gate(self._h, int(kind), float(threshold)), "eqf_set_outlier_gate")

    def outlier_gate(self):
        """(kind, threshold) of the handle's outlier gate."""
        kind, thr = C.c_int(), C.c_double()
        _check(lib().eqf_get_outlier_gate(self._h, C.byref(kind), C.byref(thr)), "eqf_get_outlier_gate")
        return kind.value, thr.value

    def gate_report(self, b=0):
        """What the outlier gate of filter b's most recent vision call looked at: dict with ids (n,), stat (n,) -- the chord or d2 -- and
        removed (n,) bool, in the state's order before the removals; n = 0 when the gate was disarmed or the call skipped."""
        n = C.c_int()
        ids, stat, rem = np.zeros(self.cap, dtype=np.int32), np.zeros(self.cap), np.zeros(self.cap, dtype=np.int32)
        _check(lib().eqf_get_gate_report(self._h, b, C.byref(n), ids.ctypes.data_as(_ip), _p(stat), rem.ctypes.data_as(_ip)),
               "eqf_get_gate_report")
        return dict(ids=ids[: n.value].copy(), stat=stat[: n.value].copy(), removed=rem[: n.value].astype(bool))

    def nees(self, err=None, local=True, first=0):
        """Joint NEES e^T A^-1 e, log det A and the definiteness of A for EVERY filter of the handle in one call, A the trailing principal
        submatrix from reference index `first` (0 | 6 | 11) of sigma_local() (local) or sigma(), factored on the device
        (include/eqf_vio_amd.h: eqf_get_nees).  err: array (B, nrhs, n_max) or a list of per-filter arrays (nrhs, n_b) in the reference's
        index map, nrhs <= 16; None: the statistics only.  Returns a dict with nees (B, nrhs), logdet, min_pivot, dof, info (B,)."""
        B = self.B
        nrhs, lde, E = 0, 0, None
        if err is not None:
            if isinstance(err, np.ndarray) and err.ndim == 3:
                E = np.ascontiguousarray(err, dtype=np.float64)
                assert E.shape[0] == B
            else:
                rows = [np.atleast_2d(np.asarray(e, dtype=np.float64)) for e in err]
                assert len(rows) == B and all(r.shape[0] == rows[0].shape[0] for r in rows)
                E = np.zeros((B, rows[0].shape[0], max(max(r.shape[1] for r in rows), 1)))
                for b, r in enumerate(rows):
                    E[b, :, : r.shape[1]] = r
            nrhs, lde = int(E.shape[1]), int(E.shape[2])
        out = np.zeros((B, max(nrhs, 1)))
        st = (SigmaStats * B)()
        _check(lib().eqf_get_nees(self._h, int(bool(local)), int(first), nrhs, _p(E) if nrhs else None, lde, _p(out) if nrhs else None, st),
               "eqf_get_nees")
        return dict(nees=out[:, :nrhs], logdet=np.array([s.logdet for s in st]), min_pivot=np.array([s.min_pivot for s in st]),
                    dof=np.array([s.dof for s in st], dtype=np.int32), info=np.array([s.info for s in st], dtype=np.int32))

    def _rows(self, v, what):
        """(B, k, n_max) from an array (B, k, n) / (B, n) or a list of per-filter arrays (k, n_b) / (n_b,), zero beyond a filter's own order"""
        B = self.B
        if isinstance(v, np.ndarray) and v.ndim == 3:
            out = np.ascontiguousarray(v, dtype=np.float64)
        elif isinstance(v, np.ndarray) and v.ndim == 2 and v.shape[0] == B and B > 1:
            out = np.ascontiguousarray(v[:, None, :], dtype=np.float64)
        else:
            rows = [np.atleast_2d(np.asarray(e, dtype=np.float64)) for e in v]
            if len(rows) != B or any(r.shape[0] != rows[0].shape[0] for r in rows):
                raise ValueError(f"{what}: one array per filter, all with the same number of vectors")
            out = np.zeros((B, rows[0].shape[0], max(max(r.shape[1] for r in rows), 1)))
            for b, r in enumerate(rows):
                out[b, :, : r.shape[1]] = r
        if out.shape[0] != B:
            raise ValueError(f"{what}: first dimension must be the batch ({B})")
        return out

    @staticmethod
    def _stats(st):
        return dict(logdet=np.array([s.logdet for s in st]), min_pivot=np.array([s.min_pivot for s in st]),
                    dof=np.array([s.dof for s in st], dtype=np.int32), info=np.array([s.info for s in st], dtype=np.int32))

    def sample_sigma(self, z, local=True, first=0, scale=None):
        """Draws from the covariance of EVERY filter of the handle in one call: eps = scale[b] L_b z with L_b L_b^T the matrix nees() factors
        for the same `local` and `first` (include/eqf_vio_amd.h: eqf_sample_sigma).  z: array (B, nsamp, n_max) or a list of per-filter
        arrays (nsamp, n_b) of standard normal numbers in the reference's index map, nsamp <= 64 (entries below `first` are ignored); a
        numpy.random.Generator draws (B, 1, n_max) itself.  Returns a dict with eps (B, nsamp, n_max: zero below `first` and beyond a
        filter's own order, NaN rows where info != 0), z as used, and logdet, min_pivot, dof, info (B,)."""
        B = self.B
        if isinstance(z, np.random.Generator):
            z = z.standard_normal((B, 1, 11 + 3 * max(self.num_landmarks(b) for b in range(B))))
        Z = self._rows(z, "sample_sigma")
        nsamp, ld = int(Z.shape[1]), int(Z.shape[2])
        eps = np.zeros_like(Z)
        sc = None if scale is None else np.ascontiguousarray(np.broadcast_to(np.asarray(scale, dtype=np.float64), (B,)))
        st = (SigmaStats * B)()
        _check(lib().eqf_sample_sigma(self._h, int(bool(local)), int(first), nsamp, _p(Z), ld, None if sc is None else _p(sc), _p(eps), ld, st),
               "eqf_sample_sigma")
        return dict(eps=eps, z=Z, **self._stats(st))

    def apply_increment(self, gamma, mask=None):
        """Moves the filters by increments of the origin chart (the coordinates of sigma() and of last_update()["gamma"]): bias +=
        gamma[0:6], X <- VIOExp(liftInnovation(gamma[6:], xi0)) X, whatever the lift settings are; Sigma, the origin, the clock and the
        integrator stay (include/eqf_vio_amd.h: eqf_apply_increment).  gamma: array (B, n_max) or a list of per-filter vectors (n_b,);
        mask (B,): 0 leaves a filter alone, every bit.  Enqueues and returns."""
        G = self._rows(gamma, "apply_increment")
        if G.shape[1] != 1:
            raise ValueError("apply_increment: one increment per filter")
        _check(lib().eqf_apply_increment(self._h, _p(G), int(G.shape[2]), _pn(self._mask(mask), _up)), "eqf_apply_increment")

    def perturb(self, z, first=0, scale=None, stats=False):
        """sample_sigma(z, local=False, first, scale) with one z per filter and apply_increment of the result as one enqueued sequence on the
        device -- the same bits, no host round trip (include/eqf_vio_amd.h: eqf_perturb_filters).  scale[b] = 0 leaves filter b alone, every
        bit (roughen only the duplicates of a resample(): consistency.systematic_resample's parents tell which).  z as in sample_sigma
        (one vector per filter) or a numpy.random.Generator.  stats: wait for the device and return logdet, min_pivot, dof, info (B,)."""
        B = self.B
        if isinstance(z, np.random.Generator):
            z = z.standard_normal((B, 1, 11 + 3 * max(self.num_landmarks(b) for b in range(B))))
        Z = self._rows(z, "perturb")
        if Z.shape[1] != 1:
            raise ValueError("perturb: one z per filter")
        sc = None if scale is None else np.ascontiguousarray(np.broadcast_to(np.asarray(scale, dtype=np.float64), (B,)))
        st = (SigmaStats * B)() if stats else None
        _check(lib().eqf_perturb_filters(self._h, int(first), _p(Z), int(Z.shape[2]), None if sc is None else _p(sc), st), "eqf_perturb_filters")
        return self._stats(st) if stats else None

    def lift_report(self, b=0):
        """The lift of filter b in the most recent update_linear, update_landmarks, apply_increment or perturb (include/eqf_vio_amd.h:
        eqf_get_lift_report): dict with kind (0 plain, 1 bundleLift + continuous lift, 2 bundleLift + discrete lift), info (0 applied, 3 took
        no part, 4 lift failed: filter untouched), DeltaU (6,), min_pivot and pivot_ratio.  consistency.bundle_lift_host is its numpy
        statement."""
        r = LiftReport()
        _check(lib().eqf_get_lift_report(self._h, int(b), C.byref(r)), "eqf_get_lift_report")
        return dict(kind=r.kind, info=r.info, DeltaU=np.array(r.DeltaU[:]), min_pivot=r.min_pivot, pivot_ratio=r.pivot_ratio)

    def _consider(self, consider, what):
        """consider: one id list per filter, or an int array (B, K) (a single-filter handle also takes the list itself) -> (n_consider,
        ids [B][cstride], cstride)"""
        if self.B == 1 and not (len(consider) == 1 and np.ndim(consider[0]) == 1):
            consider = [np.asarray(consider, dtype=np.int32).reshape(-1)]
        if len(consider) != self.B:
            raise ValueError(f"{what}: consider takes one id list per filter")
        if isinstance(consider, np.ndarray) and consider.ndim == 2:  # (B, K): every filter names K ids, one conversion
            cid = np.ascontiguousarray(consider, dtype=np.int32)
            return np.full(self.B, cid.shape[1], dtype=np.int32), (cid if cid.shape[1] else np.zeros((self.B, 1), dtype=np.int32)), max(1, cid.shape[1])
        cl = [np.asarray(x, dtype=np.int32).reshape(-1) for x in consider]
        cstride = max(1, max(len(c) for c in cl))
        nc = np.array([len(c) for c in cl], dtype=np.int32)
        cid = np.zeros((self.B, cstride), dtype=np.int32)
        for b, c in enumerate(cl):
            cid[b, :len(c)] = c
        return nc, cid, cstride

    def _mask(self, mask):
        """mask (B,), a scalar or None -> uint8 (B,) of zeros and ones, or None"""
        return None if mask is None else np.ascontiguousarray(np.broadcast_to(np.asarray(mask), (self.B,)) != 0, dtype=np.uint8)

    def _padded_ids(self, idl, stride, what):
        """the filters' id lists (int32 vectors) -> their lengths nk (B,), the ids padded with zeros to (B, stride) and stride (None: the
        longest list, at least 1)"""
        longest = max(1, max(len(i) for i in idl))
        stride = longest if stride is None else int(stride)
        if stride < longest:
            raise ValueError(f"{what}: stride is shorter than the longest list")
        idm = np.zeros((self.B, stride), dtype=np.int32)
        for b, i in enumerate(idl):
            idm[b, :len(i)] = i
        return np.array([len(i) for i in idl], dtype=np.int32), idm, stride

    @staticmethod
    def _report(rep, **more):
        """eqf_linear_report [B] as the dict the updates return: nis, logdet_S, loglik, dof, info (B,), then the call's further items"""
        return dict(nis=np.array([s.nis for s in rep]), logdet_S=np.array([s.logdet_S for s in rep]), loglik=np.array([s.loglik for s in rep]),
                    dof=np.array([s.dof for s in rep], dtype=np.int32), info=np.array([s.info for s in rep], dtype=np.int32), **more)

    def update_linear(self, H, resid, R, local=True, gate=float("inf"), mask=None, want_gamma=False, stats=True, consider=None):
        """A measurement update with m <= 16 linear rows for EVERY filter of the handle in one call (include/eqf_vio_amd.h:
        eqf_update_linear): resid = H eps + noise, noise ~ N(0, R), eps "truth minus estimate" in the coordinates of sigma_local() (local)
        or of sigma().  H: one (m, n) array for a single-filter handle, an array (B, m, n_max) or a list of per-filter arrays (m, n_b) in the
        reference's index map (consistency.velocity_rows / landmark_rows / gravity_rows write the usual ones); resid (m,), (B, m) or a list;
        R (m, m), broadcast to every filter, (B, m, m) or a list: only the lower triangle is read.  gate: chi-square threshold on the m-dof
        nis (consistency.chi2_gate_threshold(p, dof=m)); mask (B,): 0 leaves a filter alone.  A filter whose info is not 0 keeps every bit.
        With stats or want_gamma the call waits for the device and returns a dict: nis, logdet_S, loglik (B,), dof, info (B,) and, if
        asked for, gamma (B, n_max) in the reference's index map (rows of untouched filters 0); otherwise it enqueues and returns None.
        consider: None, or one list of landmark ids per filter (strictly ascending): the Schmidt update (eqf_update_linear_schmidt) --
        those landmarks keep their estimate and their covariance block, their cross-correlations still enter S and the gain; gamma comes
        back with exact zeros there; an id the state does not hold is ignored.  consistency.schmidt_update_host is its numpy statement."""
        B = self.B
        if isinstance(H, np.ndarray) and H.ndim == 2:
            H = H[None]
        Hs = self._rows(H, "update_linear")
        m, ldh = int(Hs.shape[1]), int(Hs.shape[2])
        r = np.asarray(resid, dtype=np.float64) if not isinstance(resid, (list, tuple)) else np.stack([np.asarray(x, dtype=np.float64) for x in resid])
        r = np.ascontiguousarray(np.broadcast_to(r, (B, m)))
        Rs = np.asarray(R, dtype=np.float64) if not isinstance(R, (list, tuple)) else np.stack([np.asarray(x, dtype=np.float64) for x in R])
        Rs = np.ascontiguousarray(np.broadcast_to(Rs, (B, m, m)))
        mk = self._mask(mask)
        ldg = max(ldh, 11 + 3 * max(self.num_landmarks(b) for b in range(B))) if want_gamma else 0
        G = np.zeros((B, ldg)) if want_gamma else None
        rep = (LinearReport * B)() if (stats or want_gamma) else None
        head = (self._h, int(bool(local)), m, _p(Hs), ldh, _p(r), _p(Rs), float(gate), _pn(mk, _up))
        if consider is None:
            _check(lib().eqf_update_linear(*head, _pn(G), ldg, rep), "eqf_update_linear")
        else:
            nc, cid, cstride = self._consider(consider, "update_linear")
            _check(lib().eqf_update_linear_schmidt(*head, _pn(nc, _ip), _pn(cid, _ip), cstride, _pn(G), ldg, rep), "eqf_update_linear_schmidt")
        if rep is None:
            return None
        return self._report(rep, gamma=G) if want_gamma else self._report(rep)

    def update_landmarks(self, ids, H, resid, R, rows=None, local=True, gate=float("inf"), lm_gate=float("inf"), mask=None, wait=True,
                         stride=None, consider=None):
        """A measurement update from per-landmark blocks for EVERY filter of the handle in one call (include/eqf_vio_amd.h:
        eqf_update_landmarks): entry k of filter b measures the landmark ids[b][k] alone, resid_k = H_k eps_i + noise, noise ~ N(0, R_k),
        eps_i "truth minus estimate" of the landmark's 3-block in the coordinates of sigma_local() (local: the plain difference of
        camera-frame positions) or of sigma().  consistency.stereo_rows / depth_rows / position_rows write the usual blocks.
        ids, H, resid, R: lists with one item per filter -- ids (K_b,) strictly ascending, H (K_b, rows, 3), resid (K_b, rows), R
        (K_b, rows, rows: lower triangles read) or (rows, rows), broadcast to every entry; K_b may differ between filters and may be 0.  A
        single-filter handle also takes the four arrays themselves.  rows: 1, 2 or 3, taken from H when not given (needed when every K_b is
        0).  gate: chi-square threshold on the joint nis; lm_gate: on every entry's own 'rows'-dof distance
        (consistency.chi2_gate_threshold(p, dof=rows)); mask (B,): 0 leaves a filter alone.  A filter whose info is not 0 keeps every bit.
        stride: the entries per filter the arrays handed to the library are laid out for (default: the longest list); the launch shapes
        follow it.
        With wait the call waits for the device and returns a dict: nis, logdet_S, loglik, dof, info (B,), used (B, stride): 1 applied, 0 id
        not in the state, 2 gated, and gamma (B, n_max) in the reference's index map (rows of untouched filters 0); otherwise it enqueues
        and returns None.
        consider: None, or one list of landmark ids per filter (strictly ascending): the Schmidt update (eqf_update_landmarks_schmidt),
        as in update_linear -- the entries may measure consider landmarks."""
        B = self.B
        if B == 1 and not (isinstance(ids, (list, tuple)) and len(ids) == 1 and np.ndim(ids[0]) == 1):
            ids, H, resid, R = [ids], [H], [resid], [R]
        if not (len(ids) == len(H) == len(resid) == len(R) == B):
            raise ValueError("update_landmarks: one item per filter")
        idl = [np.asarray(x, dtype=np.int32).reshape(-1) for x in ids]
        if rows is None:
            shapes = {np.shape(h)[1] for h, i in zip(H, idl) if len(i)}
            if len(shapes) != 1:
                raise ValueError("update_landmarks: rows cannot be taken from H")
            rows = shapes.pop()
        rows = int(rows)
        nk, idm, stride = self._padded_ids(idl, stride, "update_landmarks")
        Hs = np.zeros((B, stride, rows, 3))
        rs = np.zeros((B, stride, rows))
        Rs = np.zeros((B, stride, rows, rows))
        for b in range(B):
            k = int(nk[b])
            if k == 0:
                continue
            Hs[b, :k] = np.asarray(H[b], dtype=np.float64).reshape(k, rows, 3)
            rs[b, :k] = np.asarray(resid[b], dtype=np.float64).reshape(k, rows)
            Rs[b, :k] = np.broadcast_to(np.asarray(R[b], dtype=np.float64), (k, rows, rows))
        mk = self._mask(mask)
        ldg = 11 + 3 * max(self.num_landmarks(b) for b in range(B))
        G = np.zeros((B, ldg)) if wait else None
        used = np.zeros((B, stride), dtype=np.uint8) if wait else None
        rep = (LinearReport * B)() if wait else None
        head = (self._h, int(bool(local)), rows, _pn(nk, _ip), _pn(idm, _ip), stride, _p(Hs), _p(rs), _p(Rs), float(gate), float(lm_gate),
                _pn(mk, _up))
        tail = (_pn(used, _up), _pn(G), ldg if wait else 0, rep)
        if consider is None:
            _check(lib().eqf_update_landmarks(*head, *tail), "eqf_update_landmarks")
        else:
            nc, cid, cstride = self._consider(consider, "update_landmarks")
            _check(lib().eqf_update_landmarks_schmidt(*head, _pn(nc, _ip), _pn(cid, _ip), cstride, *tail), "eqf_update_landmarks_schmidt")
        return self._report(rep, used=used, gamma=G) if wait else None

    def observe_landmarks(self, kind, ids, meas, R, cam=None, gate=float("inf"), lm_gate=float("inf"), mask=None, consider=None, wait=True,
                          want_rows=False, stride=None, max_lin=1, tol=0.0, want_trace=False):
        """update_landmarks with the rows formed ON THE DEVICE at each filter's own estimate (include/eqf_vio_amd.h:
        eqf_observe_landmarks): no dump_state, no state_estimate, no rows in numpy.  kind: OBS_BEARING (2 rows; meas a bearing in the
        measuring camera's frame), OBS_RANGE (1 row; meas the distance from that camera's centre) or OBS_POSITION (3 rows; meas a position
        in that camera's frame).  ids, meas, R: lists with one item per filter -- ids (K_b,) strictly ascending, meas (K_b, 3) ((K_b,)
        or (K_b, 1) for a range), R (K_b, rows, rows: lower triangles read), (rows, rows) or a scalar variance, broadcast to every entry;
        a single-filter handle also takes the arrays themselves.  cam: None (the primary camera), (q_c, t_c) -- the measuring camera's
        pose in the primary camera's frame, quaternion (w, x, y, z) -- for the call, or a list of B such pairs, one per filter.
        gate, lm_gate, mask, consider, stride: as in update_landmarks.  consistency.observe_rows_host is the numpy statement of the rows.
        With wait or want_rows the call waits for the device and returns update_landmarks' dict -- used has one more value, 3 not
        observable -- and, with want_rows, Ht (B, stride, rows, 3) and resid (B, stride, rows) as the device formed them (zeros where an
        entry is absent or not observable); otherwise it enqueues and returns None.
        max_lin > 1 makes it the ITERATED update (eqf_observe_landmarks_iterated): the rows are re-formed at the estimate the update would
        give, at most max_lin linearisations, until the largest change of the increment on the named landmarks is <= tol (chart units;
        0: never stop early), and only the last linearisation is applied; resid is then r~ = resid + Ht g.  With max_lin > 1 or
        want_trace the dict also holds n_lin, status (0 converged, 1 ran out of linearisations, 2 stalled, 3 an intermediate solve
        failed, 4 masked out) and last_step, each (B,), and with want_trace g_trace (max_lin, B, stride, 3): the increment on each
        entry's landmark at which linearisation k was taken.  consistency.observe_iterated_host is the numpy statement."""
        B = self.B
        kind = int(kind)
        max_lin = int(max_lin)
        iterated = max_lin > 1 or bool(want_trace)
        if kind not in OBS_ROWS:
            raise ValueError("observe_landmarks: kind is OBS_BEARING, OBS_RANGE or OBS_POSITION")
        rows = OBS_ROWS[kind]
        if B == 1 and not (isinstance(ids, (list, tuple)) and len(ids) == 1 and np.ndim(ids[0]) == 1):
            ids, meas, R = [ids], [meas], [R]
        if not isinstance(R, (list, tuple)):
            R = [R] * B
        if not (len(ids) == len(meas) == len(R) == B):
            raise ValueError("observe_landmarks: one item per filter")
        idl = [np.asarray(x, dtype=np.int32).reshape(-1) for x in ids]
        nk, idm, stride = self._padded_ids(idl, stride, "observe_landmarks")
        ms = np.zeros((B, stride, 3))
        Rs = np.zeros((B, stride, rows, rows))
        for b in range(B):
            k = int(nk[b])
            if k == 0:
                continue
            m = np.asarray(meas[b], dtype=np.float64).reshape(k, -1)
            ms[b, :k, :m.shape[1]] = m
            Rb = np.asarray(R[b], dtype=np.float64)
            Rs[b, :k] = np.broadcast_to(Rb * np.eye(rows) if Rb.ndim == 0 else Rb, (k, rows, rows))
        camp, per = None, 0
        if cam is not None:
            per = int(not (len(cam) == 2 and np.ndim(cam[0][0]) == 0))  # (a pair's first item is q, its first item a number)
            pairs = cam if per else [cam]
            if per and len(pairs) != B:
                raise ValueError("observe_landmarks: one camera offset, or one per filter")
            camp = np.ascontiguousarray([np.concatenate([np.asarray(q, dtype=np.float64).reshape(4), np.asarray(t, dtype=np.float64).reshape(3)])
                                         for q, t in pairs])
        mk = self._mask(mask)
        out = bool(wait or want_rows or want_trace)
        ldg = 11 + 3 * max(self.num_landmarks(b) for b in range(B))
        G = np.zeros((B, ldg)) if out else None
        used = np.zeros((B, stride), dtype=np.uint8) if out else None
        rep = (LinearReport * B)() if out else None
        Ht = np.zeros((B, stride, rows, 3)) if want_rows else None
        rs = np.zeros((B, stride, rows)) if want_rows else None
        nc, cid, cstride = (None, None, 0) if consider is None else self._consider(consider, "observe_landmarks")
        # both entry points take the same arguments: the iterated one max_lin and tol between them, the trace and its report behind them
        head = (self._h, kind, _pn(camp), per, _pn(nk, _ip), _pn(idm, _ip), stride, _p(ms), _p(Rs), float(gate), float(lm_gate), _pn(mk, _up),
                _pn(nc, _ip), _pn(cid, _ip), cstride)
        tail = (_pn(used, _up), _pn(Ht), _pn(rs), _pn(G), ldg if out else 0, rep)
        more = {}
        if iterated:
            irep = (IterReport * B)() if out else None
            trace = np.zeros((max(max_lin, 1), B, stride, 3)) if want_trace else None
            _check(lib().eqf_observe_landmarks_iterated(*head, max_lin, float(tol), *tail, _pn(trace), irep), "eqf_observe_landmarks_iterated")
            if out:
                more.update(n_lin=np.array([s.n_lin for s in irep], dtype=np.int32), status=np.array([s.status for s in irep], dtype=np.int32),
                            last_step=np.array([s.last_step for s in irep]))
        else:
            _check(lib().eqf_observe_landmarks(*head, *tail), "eqf_observe_landmarks")
        if not out:
            return None
        if want_rows:
            more.update(Ht=Ht, resid=rs)
        if want_trace:
            more.update(g_trace=trace)
        return self._report(rep, used=used, gamma=G, **more)

    @staticmethod
    def _members(idx, w):
        ii = np.ascontiguousarray(np.atleast_1d(idx), dtype=np.int32)
        ww = np.ascontiguousarray(np.atleast_1d(w), dtype=np.float64)
        if ii.ndim != 1 or ii.shape != ww.shape or len(ii) == 0:
            raise ValueError("idx and w must be one-dimensional, of one length and not empty")
        return ii, ww

    @staticmethod
    def _mixture_report(r):
        return dict(n_eff=r.n_eff, spread_trace=r.spread_trace, total_trace=r.total_trace, n=r.n, info=r.info)

    def mixture_moments(self, idx, w, ref, centred=True):
        """Mean and covariance of the weighted members idx of this handle in the chart of filter ref's estimate, the spread between the
        members included, on the device (include/eqf_vio_amd.h: eqf_get_mixture_moments; consistency.mixture_moments_host is its numpy
        statement, consistency.mixture_weights turns log-likelihoods into w).  Returns a dict with mean (11 + 3N,), P (11 + 3N, 11 + 3N)
        in the reference's index map -- NaN where info != 0 -- and n_eff, spread_trace, total_trace, n, info."""
        ii, ww = self._members(idx, w)
        n = 11 + 3 * self.num_landmarks(int(ref)) if 0 <= int(ref) < self.B else 11
        mean, P, rep = np.zeros(n), np.zeros((n, n)), MixtureReport()
        _check(lib().eqf_get_mixture_moments(self._h, len(ii), ii.ctypes.data_as(_ip), _p(ww), int(ref), int(bool(centred)), _p(mean), _p(P), n,
                                             C.byref(rep)), "eqf_get_mixture_moments")
        return dict(mean=mean, P=P, **self._mixture_report(rep))

    def merge(self, idx, w, ref, dst, report=True):
        """Filter dst becomes ONE filter that matches the first two moments of the weighted members idx: origin = the merged state, X =
        identity, Sigma = the members' mean-square error about it (include/eqf_vio_amd.h: eqf_merge_filters; consistency.merge_host).
        dst may be a member.  report: wait for the device and return n_eff, spread_trace, total_trace, n, info (info != 0: nothing was
        written); otherwise enqueue and return None."""
        ii, ww = self._members(idx, w)
        rep = MixtureReport() if report else None
        _check(lib().eqf_merge_filters(self._h, len(ii), ii.ctypes.data_as(_ip), _p(ww), int(ref), int(dst), C.byref(rep) if report else None),
               "eqf_merge_filters")
        return self._mixture_report(rep) if report else None

    def split_filters(self, a, dst_idx, src_idx, shift, shrink, local=True, want_gamma=False, report=True):
        """The deterministic split on the device (include/eqf_vio_amd.h: eqf_split_filters; consistency.split_host is its numpy statement):
        child k makes filter dst_idx[k] what copy_filters(src_idx[k] -> dst_idx[k]) leaves, with Sigma - shrink[k] u u^T and the state
        moved by shift[k] u, u = Sigma Ht^T / sqrt(Ht Sigma Ht^T) of the source.  a: array (B, >= n_max), row b the functional of filter b
        (rows of filters that are no child's source are not read), or a list of per-filter rows (None for the others); local: the rows are
        written against sigma_local()'s error around the estimate (a J is formed on the device), else against sigma()'s.  dst == src is the
        child that stays in place; a filter named as a dst may be a source only of itself.  consistency.split_components gives
        moment-matched (weights, shift, shrink).  Returns None (want_gamma and report both false: enqueues and returns, unless a dst's
        ids, clock or flags change) or a dict with S (n,), info (n,) per child -- info != 0: nothing of that source's children was written --
        and, with want_gamma, gamma (n, n_max), child k's increment in the reference index map."""
        B = self.B
        di = np.ascontiguousarray(np.atleast_1d(dst_idx), dtype=np.int32)
        si = np.ascontiguousarray(np.atleast_1d(src_idx), dtype=np.int32)
        n = int(di.size)
        if si.size != n:
            raise ValueError("split_filters: dst_idx and src_idx differ in length")
        sh = np.ascontiguousarray(np.broadcast_to(np.asarray(shift, dtype=np.float64), (n,)))
        sk = np.ascontiguousarray(np.broadcast_to(np.asarray(shrink, dtype=np.float64), (n,)))
        if n == 0:  # (an empty numpy array may have no address: the C ABI wants its arrays also for n = 0)
            di = si = np.zeros(1, dtype=np.int32)
            sh = sk = np.zeros(1)
        nmax = 11 + 3 * max([self.num_landmarks(b) for b in range(B)] + [0])
        if isinstance(a, np.ndarray) and a.ndim == 2:
            A = np.ascontiguousarray(a, dtype=np.float64)
            if A.shape[0] != B:
                raise ValueError("split_filters: one row per filter of the handle")
        else:
            A = np.zeros((B, nmax))
            for b, row in enumerate(a):
                if row is not None:
                    r = np.asarray(row, dtype=np.float64).ravel()
                    if r.size > nmax:
                        raise ValueError("split_filters: a row longer than the largest filter's order")
                    A[b, :r.size] = r
        G = np.zeros((n, nmax)) if want_gamma else None
        rep = (SplitReport * max(n, 1))() if report else None
        _check(lib().eqf_split_filters(self._h, int(bool(local)), _p(A), int(A.shape[1]), n, di.ctypes.data_as(_ip), si.ctypes.data_as(_ip),
                                       _p(sh), _p(sk), None if G is None else _p(G), nmax, rep), "eqf_split_filters")
        if not want_gamma and not report:
            return None
        out = {}
        if report:
            out["S"] = np.array([rep[k].S for k in range(n)])
            out["info"] = np.array([rep[k].info for k in range(n)], dtype=np.int32)
        if want_gamma:
            out["gamma"] = G
        return out

    def merge_costs(self, idx, w, ref=None, kind="runnalls", first=0, pairs=None):
        """Pairwise merge costs of the weighted members idx of this handle, on the device (include/eqf_vio_amd.h: eqf_get_merge_costs;
        consistency.merge_costs_host is its numpy statement).  ref: the member whose estimate is the chart centre (default: the heaviest,
        the first of them).  kind: "runnalls" or "bhattacharyya"; first: 0, 6 or 11.  pairs: (npairs, 2) POSITIONS in idx, or None: all
        i < j in lexicographic order.  Returns a dict: pairs (npairs, 2) as asked, cost, logdet_pair, maha, info (npairs,), member_logdet,
        member_min_pivot, member_dof, member_info (n,), ref, and with pairs=None the symmetric (n, n) matrix of costs, zero diagonal."""
        ii, ww = self._members(idx, w)
        n = len(ii)
        if ref is None:
            ref = int(ii[int(np.argmax(ww))])
        if pairs is None:
            pp = np.array([(i, j) for i in range(n) for j in range(i + 1, n)], dtype=np.int32).reshape(-1, 2)
        else:
            pp = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        npairs = len(pp)
        out = (PairCost * max(npairs, 1))()
        mem = (SigmaStats * n)()
        _check(lib().eqf_get_merge_costs(self._h, n, ii.ctypes.data_as(_ip), _p(ww), int(ref), COST_KINDS[kind], int(first), npairs,
                                         None if pairs is None or npairs == 0 else pp.ctypes.data_as(_ip), out, mem), "eqf_get_merge_costs")
        res = dict(pairs=pp, cost=np.array([out[k].cost for k in range(npairs)]), logdet_pair=np.array([out[k].logdet_pair for k in range(npairs)]),
                   maha=np.array([out[k].maha for k in range(npairs)]), info=np.array([out[k].info for k in range(npairs)], dtype=np.int32),
                   member_logdet=np.array([s.logdet for s in mem]), member_min_pivot=np.array([s.min_pivot for s in mem]),
                   member_dof=np.array([s.dof for s in mem], dtype=np.int32), member_info=np.array([s.info for s in mem], dtype=np.int32),
                   ref=int(ref))
        if pairs is None:
            M = np.zeros((n, n))
            for k in range(npairs):
                M[pp[k, 0], pp[k, 1]] = M[pp[k, 1], pp[k, 0]] = res["cost"][k]
            res["matrix"] = M
        return res

    def score_vision(self, ids, bearings, mask=None, want_lm=False, nb=None, stride=None):
        """How likely candidate vision frames are under every filter of the handle, WITHOUT applying any of them (include/eqf_vio_amd.h:
        eqf_score_vision; consistency.score_vision_host is its numpy statement, consistency.joint_compatible the chi-square test on the
        result).  ids[b][c]: the strictly ascending ids of candidate c of filter b, bearings[b][c] (n, 3) its bearings -- ragged lists, every
        filter with the same number of candidates -- or padded arrays (B, ncand, stride) / (B, ncand, stride, 3) with nb (B, ncand) the
        entries that count (default: all).  A single-filter handle also takes the candidates themselves.  mask (B,): 0 leaves a filter out
        (info = 3).  stride: the entries per candidate the arrays handed to the library are laid out for (default: the longest list).
        Returns a FrameScores: nis, logdet_S, loglik, dof, info (B, ncand), and with want_lm nis_lm and used (B, ncand, stride) at the
        caller's entry positions.  The handle is only read."""
        B = self.B
        if isinstance(ids, np.ndarray) and ids.ndim == 3:
            idm = np.ascontiguousarray(ids, dtype=np.int32)
            ncand, st = idm.shape[1], idm.shape[2]
            ys = np.ascontiguousarray(bearings, dtype=np.float64).reshape(idm.shape[0], ncand, st, 3)
            nbv = np.full((idm.shape[0], ncand), st, dtype=np.int32) if nb is None else np.ascontiguousarray(nb, dtype=np.int32).reshape(-1, ncand)
            if stride is not None and int(stride) != st:
                raise ValueError("score_vision: stride differs from the padded arrays'")
        else:
            def flat(x):  # one candidate's ids, not a list of candidates
                return (isinstance(x, np.ndarray) and x.ndim == 1) or (isinstance(x, (list, tuple)) and all(np.isscalar(e) for e in x))

            if B == 1 and len(ids) > 0 and flat(ids[0]):
                ids, bearings = [ids], [bearings]
            ncand = len(ids[0]) if len(ids) else 0
            if len(ids) != B or len(bearings) != B or any(len(i) != ncand or len(y) != ncand for i, y in zip(ids, bearings)):
                raise ValueError("score_vision: one list of candidates per filter, of one length")
            idl = [[np.asarray(x, dtype=np.int32).reshape(-1) for x in row] for row in ids]
            longest = max([1] + [len(x) for row in idl for x in row])
            st = longest if stride is None else int(stride)
            if st < longest:
                raise ValueError("score_vision: stride is shorter than the longest list")
            nbv = np.array([[len(x) for x in row] for row in idl], dtype=np.int32).reshape(B, ncand)
            idm = np.zeros((B, ncand, st), dtype=np.int32)
            ys = np.zeros((B, ncand, st, 3))
            for b in range(B):
                for c in range(ncand):
                    k = int(nbv[b, c])
                    if k:
                        idm[b, c, :k] = idl[b][c]
                        ys[b, c, :k] = np.asarray(bearings[b][c], dtype=np.float64).reshape(k, 3)
        if idm.shape[0] != B or nbv.shape != (B, ncand):
            raise ValueError("score_vision: one row of candidates per filter")
        mk = None if mask is None else np.ascontiguousarray(np.broadcast_to(np.asarray(mask), (B,)) != 0, dtype=np.uint8)
        up = C.POINTER(C.c_ubyte)
        out = (FrameScore * max(B * ncand, 1))()
        lm = np.zeros((B, ncand, st)) if want_lm else None
        used = np.zeros((B, ncand, st), dtype=np.uint8) if want_lm else None
        _check(lib().eqf_score_vision(self._h, int(ncand), nbv.ctypes.data_as(_ip), idm.ctypes.data_as(_ip), _p(ys), int(st),
                                      None if mk is None else mk.ctypes.data_as(up), out, None if lm is None else _p(lm),
                                      None if used is None else used.ctypes.data_as(up)), "eqf_score_vision")
        rec = [out[k] for k in range(B * ncand)]
        res = FrameScores(nis=np.array([r.nis for r in rec]).reshape(B, ncand), logdet_S=np.array([r.logdet_S for r in rec]).reshape(B, ncand),
                          loglik=np.array([r.loglik for r in rec]).reshape(B, ncand),
                          dof=np.array([r.dof for r in rec], dtype=np.int32).reshape(B, ncand),
                          info=np.array([r.info for r in rec], dtype=np.int32).reshape(B, ncand))
        if want_lm:
            res.nis_lm, res.used = lm, used
        return res

    def reduce_mixture(self, idx, w, target, max_cost=float("inf"), kind="runnalls"):
        """Greedy mixture reduction on the device: while more than `target` members are left, the pair of least merge cost (ties: the
        lower pair in lexicographic order of positions) is merged with merge() into the slot of the lower position -- into the centre's
        slot if the higher position holds the chart centre, the heaviest member at the start, so that it stays valid --, the weights are
        added and the other slot is dropped; only the pairs that involve the merged slot are asked for again.  Stops early when the
        cheapest cost exceeds max_cost.  Returns (surviving indices, their weights, log) with log a list of ((position kept, position
        dropped), cost), positions in idx.  consistency.reduce_mixture_host is its numpy statement."""
        ii, ww = self._members(idx, w)
        ww = ww / ww.sum()
        alive = list(range(len(ii)))
        wt = {k: float(ww[k]) for k in alive}
        centre = int(np.argmax(ww))
        log = []

        def ask(pairs_pos):  # (every member left is named, so that the weights are normalised as a whole; `pairs` picks what is factored)
            loc = {p: k for k, p in enumerate(alive)}
            r = self.merge_costs(ii[alive], [wt[p] for p in alive], ref=int(ii[centre]), kind=kind,
                                 pairs=[(loc[a], loc[b]) for a, b in pairs_pos])
            return {pr: (float(c) if i == 0 else float("inf")) for pr, c, i in zip(pairs_pos, r["cost"], r["info"])}

        cache = {}
        if len(alive) > 1:
            cache = ask([(a, b) for x, a in enumerate(alive) for b in alive[x + 1:]])
        while len(alive) > max(int(target), 1):
            (a, b), c = min(cache.items(), key=lambda kv: (kv[1], kv[0]))
            if not c <= max_cost:
                break
            keep, drop = (b, a) if b == centre else (a, b)
            s = wt[a] + wt[b]
            rep = self.merge([ii[a], ii[b]], [wt[a], wt[b]], ref=int(ii[keep]), dst=int(ii[keep]))
            if rep["info"] != 0:
                raise RuntimeError(f"reduce_mixture: merge of {(a, b)} reported info {rep['info']}")
            log.append(((keep, drop), c))
            wt[keep] = s
            del wt[drop]
            alive.remove(drop)
            cache = {pr: v for pr, v in cache.items() if a not in pr and b not in pr}
            fresh = [tuple(sorted((keep, o))) for o in alive if o != keep]
            if fresh:
                cache.update(ask(fresh))
        return ii[alive].copy(), np.array([wt[k] for k in alive]), log

    def debug_mixture_launches(self):
        """Kernel launches of the most recent merge() (include/eqf_vio_amd_debug.h)."""
        return _check(lib().eqf_debug_mixture_launches(self._h), "eqf_debug_mixture_launches")

    def debug_iterate_launches(self):
        """Kernel launches the most recent iterated observe_landmarks added to the one-shot call's (include/eqf_vio_amd_debug.h)."""
        return _check(lib().eqf_debug_iterate_launches(self._h), "eqf_debug_iterate_launches")

    def debug_sigma_pad(self, b=0, image=0):
        """Largest |entry| of the pad row and column of filter b's internal covariance (image 0) or of slot b of the scratch image, where
        mixture_moments leaves P in slot ref (image 1) (include/eqf_vio_amd_debug.h)."""
        out = C.c_double()
        _check(lib().eqf_debug_sigma_pad(self._h, int(b), int(image), C.byref(out)), "eqf_debug_sigma_pad")
        return out.value

    def debug_sigma_local_all(self):
        """k_sigma_local for every filter of the handle in one launch, nothing copied (include/eqf_vio_amd_debug.h)."""
        _check(lib().eqf_debug_sigma_local_all(self._h), "eqf_debug_sigma_local_all")

    def set_sigma(self, S, b=0):
        S = np.ascontiguousarray(S, dtype=np.float64)
        n = 11 + 3 * self.num_landmarks(b)
        assert S.shape == (n, n)
        _check(lib().eqf_set_sigma(self._h, b, _p(S), n), "eqf_set_sigma")

    def dump_state(self, b=0):
        """Lossless snapshot of filter b (everything eqf_set_state needs)."""
        cv, av, at, ini = np.zeros(6), np.zeros(6), np.zeros(1), np.zeros(1, dtype=np.int32)
        _check(lib().eqf_get_integrator(self._h, b, _p(cv), _p(av), _p(at), ini.ctypes.data_as(_ip)), "eqf_get_integrator")
        return dict(ids=self.ids(b), origin=self.origin(b), group=self.group(b), bias=self.bias(b), sigma=self.sigma(b),
                    time=float(self.get_time()[b]), currentVelocity=cv, accumulatedVelocity=av, accumulatedTime=float(at[0]),
                    initialised=int(ini[0]))

    def restore_state(self, st, b=0):
        """Inverse of dump_state (checkpoint / resume, cross-backend state injection)."""
        ids = np.ascontiguousarray(st["ids"], dtype=np.int32)
        N = len(ids)
        o, g = st["origin"], st["group"]

        def arr(a, shape):
            out = np.zeros(shape)
            if N:
                out[...] = np.asarray(a, dtype=np.float64).reshape(shape)
            return np.ascontiguousarray(out)

        p0, Qq, Qa = arr(o["p"], (max(N, 1), 3)), arr(g["Qq"], (max(N, 1), 4)), arr(g["Qa"], (max(N, 1),))
        S = np.ascontiguousarray(st["sigma"], dtype=np.float64)
        cv = np.ascontiguousarray(st["currentVelocity"], dtype=np.float64)
        av = np.ascontiguousarray(st["accumulatedVelocity"], dtype=np.float64)
        arrs = [np.ascontiguousarray(x, dtype=np.float64) for x in (o["q"], o["x"], o["v"], p0, g["Aq"], g["Ax"], g["w"], Qq, Qa, st["bias"], S)]
        _check(
            lib().eqf_set_state(self._h, b, N, ids.ctypes.data_as(_ip), *[_p(a) for a in arrs], S.shape[0], float(st["time"]), _p(cv), _p(av),
                                float(st["accumulatedTime"]), int(st["initialised"])),
            "eqf_set_state",
        )

    def copy_filters(self, src, dst_idx, src_idx):
        """Filter dst_idx[k] of this handle becomes what filter src_idx[k] of `src` (another FilterBatch, or this one) was before the call,
        on the device (include/eqf_vio_amd.h: eqf_copy_filters).  The state is copied, settings and capacity stay this handle's; filters that
        are not named are untouched.  dst_idx must not repeat, src_idx may (fan-out)."""
        di = np.ascontiguousarray(np.atleast_1d(dst_idx), dtype=np.int32)
        si = np.ascontiguousarray(np.atleast_1d(src_idx), dtype=np.int32)
        if di.ndim != 1 or di.shape != si.shape:
            raise ValueError("dst_idx and src_idx must be one-dimensional and of one length")
        n = len(di)
        if n == 0:  # (an empty numpy array may have no address: the C ABI wants two arrays also for n = 0)
            di = si = np.zeros(1, dtype=np.int32)
        _check(lib().eqf_copy_filters(self._h, src._h, n, di.ctypes.data_as(_ip), si.ctypes.data_as(_ip)), "eqf_copy_filters")

    def edit_landmarks(self, remove=None, insert=None):
        """Explicit landmark removal and insertion with priors for EVERY filter of the handle in one call, on the device
        (include/eqf_vio_amd.h: eqf_edit_landmarks).  remove: a list with one array of ids per filter (strictly ascending; may be empty or None), or
        None.  insert: a list with one (ids, p, P) per filter -- ids (K_b,) strictly ascending, p (K_b, 3) camera-frame positions, P
        (K_b, 3, 3) their covariances (lower triangles read; consistency.depth_prior / triangulation_prior write the usual ones) -- or None
        per filter or altogether.  A single-filter handle also takes the id array and the triple themselves.  Per filter the removals come
        first, then the insertions are appended in the order given; an id in both lists is replaced.
        Returns (removed, inserted): lists with one uint8 array per filter -- removed 1 gone, 0 not in the state; inserted 1 done, 0 already
        in the state after the removals, 2 values rejected (not finite, p = 0, P not positive definite).  The verdicts are the host's: the
        call does not wait for the device."""
        B = self.B
        if remove is not None and B == 1 and not (isinstance(remove, (list, tuple)) and len(remove) == 1 and np.ndim(remove[0]) == 1):
            remove = [remove]
        if insert is not None and B == 1 and isinstance(insert, tuple) and len(insert) == 3 and np.ndim(insert[0]) <= 1:
            insert = [insert]
        rem = [np.zeros(0, dtype=np.int32)] * B if remove is None else [
            np.zeros(0, dtype=np.int32) if r is None else np.asarray(r, dtype=np.int32).reshape(-1) for r in remove]
        insl = [None] * B if insert is None else list(insert)
        if len(rem) != B or len(insl) != B:
            raise ValueError("edit_landmarks: one item per filter")
        insl = [(np.zeros(0, dtype=np.int32), np.zeros((0, 3)), np.zeros((0, 3, 3))) if t is None else
                (np.asarray(t[0], dtype=np.int32).reshape(-1), np.asarray(t[1], dtype=np.float64).reshape(-1, 3),
                 np.asarray(t[2], dtype=np.float64).reshape(-1, 3, 3)) for t in insl]
        for i, p, P in insl:
            if not (len(i) == len(p) == len(P)):
                raise ValueError("edit_landmarks: ids, p and P of a filter differ in length")
        rs, istr = max(1, max(len(r) for r in rem)), max(1, max(len(t[0]) for t in insl))
        nr = np.array([len(r) for r in rem], dtype=np.int32)
        ni = np.array([len(t[0]) for t in insl], dtype=np.int32)
        rid, iid = np.zeros((B, rs), dtype=np.int32), np.zeros((B, istr), dtype=np.int32)
        pp, PP = np.zeros((B, istr, 3)), np.zeros((B, istr, 3, 3))
        for b in range(B):
            rid[b, :nr[b]] = rem[b]
            iid[b, :ni[b]], pp[b, :ni[b]], PP[b, :ni[b]] = insl[b]
        removed, inserted = np.zeros((B, rs), dtype=np.uint8), np.zeros((B, istr), dtype=np.uint8)
        up = C.POINTER(C.c_ubyte)
        _check(lib().eqf_edit_landmarks(self._h, nr.ctypes.data_as(_ip), rid.ctypes.data_as(_ip), rs, ni.ctypes.data_as(_ip),
                                        iid.ctypes.data_as(_ip), istr, _p(pp), _p(PP), removed.ctypes.data_as(up), inserted.ctypes.data_as(up)),
               "eqf_edit_landmarks")
        return [removed[b, :nr[b]].copy() for b in range(B)], [inserted[b, :ni[b]].copy() for b in range(B)]

    def remove_landmarks(self, ids):
        """edit_landmarks(remove=ids): the verdicts per filter (1 gone, 0 not in the state)."""
        return self.edit_landmarks(remove=ids)[0]

    def insert_landmarks(self, insert):
        """edit_landmarks(insert=insert): the verdicts per filter (1 done, 0 already in the state, 2 values rejected)."""
        return self.edit_landmarks(insert=insert)[1]

    def resample(self, parents):
        """In place: filter b continues from what filter parents[b] was before the call (consistency.systematic_resample gives parents
        from the log-likelihoods of innovation_stats())."""
        parents = np.ascontiguousarray(parents, dtype=np.int32)
        if parents.shape != (self.B,):
            raise ValueError(f"parents must have shape ({self.B},)")
        self.copy_filters(self, np.arange(self.B, dtype=np.int32), parents)

    def set_camera_offset(self, q, x):
        q, x = np.ascontiguousarray(q, dtype=np.float64), np.ascontiguousarray(x, dtype=np.float64)
        _check(lib().eqf_set_camera_offset(self._h, _p(q), _p(x)), "eqf_set_camera_offset")

    def last_update(self, b=0):
        N = self.num_landmarks(b)
        delta, gamma, Gamma = np.zeros(max(2 * N, 1)), np.zeros(11 + 3 * N), np.zeros(9 + 3 * N)
        _check(lib().eqf_get_last_update(self._h, b, _p(delta), _p(gamma), _p(Gamma)), "eqf_get_last_update")
        return dict(delta=delta[: 2 * N], gamma=gamma, Gamma=Gamma)

    def debug_blocks(self, b=0):
        """Linearisation blocks of the last single-step split-path launch + the C0i blocks (include/eqf_vio_amd.h)."""
        N = self.num_landmarks(b)
        common, rec, c0 = np.zeros(31), np.zeros((max(N, 1), 27)), np.zeros((max(N, 1), 6))
        _check(lib().eqf_debug_get_blocks(self._h, b, _p(common), _p(rec), _p(c0)), "eqf_debug_get_blocks")
        return dict(T=common[0], Bg=common[1:7].reshape(2, 3), Bvw=common[7:16].reshape(3, 3), RA=common[16:25].reshape(3, 3),
                    Avg=common[25:31].reshape(3, 2), D=rec[:N, 0:9].reshape(N, 3, 3), Lw=rec[:N, 9:18].reshape(N, 3, 3),
                    Lv=rec[:N, 18:27].reshape(N, 3, 3), C0=c0[:N].reshape(N, 2, 3))

    def device_error(self):
        return lib().eqf_device_error(self._h)

    def debug_drop_role(self, kind, role=0, R=0, C_=0):
        """Fault injection (tests): one role of the update launch leaves without publishing (kind < 0: off); include/eqf_vio_amd_debug.h."""
        _check(lib().eqf_debug_drop_role(self._h, int(kind), int(role), int(R), int(C_)), "eqf_debug_drop_role")

    def debug_option(self, name, value):
        """Developer toggle by name (include/eqf_vio_amd_debug.h: eqf_debug_option), e.g. ``"cs_in_burst"``."""
        _check(lib().eqf_debug_option(self._h, name.encode(), int(value)), "eqf_debug_option")

    def launch_shape(self):
        """Shape of the most recent IMU burst (include/eqf_vio_amd_debug.h: eqf_debug_launch_shape)."""
        a = (C.c_int * 8)()
        _check(lib().eqf_debug_launch_shape(self._h, a), "eqf_debug_launch_shape")
        return dict(builder_landmarks=a[0], rows_per_wave=a[1], fused=bool(a[2]), cs_out=bool(a[3]), builder_workgroups=a[4],
                    block_workgroups=a[5], steps=a[6])

    # ---- profiling
    def profile_enable(self, on=True):
        _check(lib().eqf_profile_enable(self._h, int(bool(on))), "eqf_profile_enable")

    def profile(self):
        out = {}
        for c in range(PROF_CLASSES):
            n = C.c_longlong()
            ms = C.c_double()
            _check(lib().eqf_profile_get(self._h, c, C.byref(n), C.byref(ms)), "eqf_profile_get")
            out[lib().eqf_profile_class_name(c).decode()] = (n.value, ms.value)
        return out
