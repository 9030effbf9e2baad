"""ctypes binding of the C-ABI in include/tray.h (libtray_amd.so, built in-tree).

This is the only way the Python host reaches the renderer: there is no Python,
PyTorch or CPU fallback for the hot path. If the shared library is missing the
import fails loudly with the build command to run.
"""
from __future__ import annotations

import ctypes
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# TRAY_LIB points the binding at another build of the same ABI (A/B tooling only).
LIB_PATH = os.environ.get("TRAY_LIB") or os.path.join(_HERE, "libtray_amd.so")

# include/tray.h enums
TRAY_OK = 0
TRAY_ERR_INVALID_ARGUMENT = -1
TRAY_ERR_UNSUPPORTED = -2
TRAY_ERR_DEVICE = -3
TRAY_ERR_NO_DEVICE = -4
TRAY_ERR_TOO_LARGE = -5
LAMBERTIAN, METAL, DIELECTRIC = 1, 2, 3
OUT_RGB_F64, OUT_RGB_F32, OUT_RGBA8 = 0, 1, 2
BYTES_PER_PIXEL = {OUT_RGB_F64: 24, OUT_RGB_F32: 12, OUT_RGBA8: 4}

# tray_sphere as a numpy structured dtype (72 bytes, C layout).
SPHERE_DTYPE = np.dtype(
    [
        ("center", "<f8", (3,)),
        ("radius", "<f8"),
        ("albedo", "<f8", (3,)),
        ("param", "<f8"),
        ("material", "<i4"),
        ("reserved", "<i4"),
    ]
)
assert SPHERE_DTYPE.itemsize == 72

_d3 = ctypes.c_double * 3


class Background(ctypes.Structure):
    _fields_ = [("color_a", _d3), ("color_b", _d3)]


class CameraSetup(ctypes.Structure):
    _fields_ = [
        ("position", _d3),
        ("look_at", _d3),
        ("up", _d3),
        ("vertical_fov", ctypes.c_double),
        ("focal_length", ctypes.c_double),
        ("focus_distance", ctypes.c_double),
        ("aperture", ctypes.c_double),
    ]


class CameraState(ctypes.Structure):
    _fields_ = [
        ("position", _d3),
        ("pixel00", _d3),
        ("pixel_x", _d3),
        ("pixel_y", _d3),
        ("defocus_u", _d3),
        ("defocus_v", _d3),
        ("aperture", ctypes.c_double),
        ("focus_distance", ctypes.c_double),
        ("focal_length", ctypes.c_double),
    ]

    def as_array(self) -> np.ndarray:
        """The 21 doubles in declaration order (the oracle's camera layout)."""
        return np.frombuffer(bytes(self), dtype=np.float64).copy()


assert ctypes.sizeof(CameraState) == 21 * 8


class Params(ctypes.Structure):
    _fields_ = [
        ("width", ctypes.c_int32),
        ("height", ctypes.c_int32),
        ("max_depth", ctypes.c_int32),
        ("rays_per_pixel", ctypes.c_int32),
        ("ray_radius", ctypes.c_double),
        ("seed", ctypes.c_uint64),
        ("y_start", ctypes.c_int32),
        ("y_end", ctypes.c_int32),
        ("tile_rows", ctypes.c_int32),
        ("tile_count", ctypes.c_int32),
        ("tile_index", ctypes.c_int32),
        ("output", ctypes.c_int32),
        ("flags", ctypes.c_int32),
        ("pass_", ctypes.c_int32),  # tray_params.pass (progressive pass)
    ]


FLAG_LINEAR_SCAN = 1  # TRAY_FLAG_LINEAR_SCAN
FLAG_ORDERED_SUM = 2  # TRAY_FLAG_ORDERED_SUM: Go's FP64 pixel sum in sample order (include/tray.h)


class SceneInfo(ctypes.Structure):
    """tray_scene_info: how an uploaded scene is traversed."""
    _fields_ = [("n_spheres", ctypes.c_int32), ("has_bvh", ctypes.c_int32), ("leaf_max", ctypes.c_int32),
                ("n_nodes", ctypes.c_int32), ("n_leaves", ctypes.c_int32), ("stack_depth", ctypes.c_int32),
                ("lds_resident", ctypes.c_int32), ("n_global", ctypes.c_int32), ("bound", ctypes.c_double)]


class RenderPlan(ctypes.Structure):
    """tray_render_plan: how a render would run (pixel sums, kernel, LDS, workspace)."""
    _fields_ = [("fixed_point_shift", ctypes.c_int32), ("acc_slots", ctypes.c_int32), ("bvh", ctypes.c_int32),
                ("lds_layout", ctypes.c_int32), ("stack_lds", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("lds_bytes", ctypes.c_int64), ("buffer_bytes", ctypes.c_int64)]

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name, _ in self._fields_ if name != "reserved"}


class TrayError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"tray error {code}: {message}")
        self.code = code


# Every symbol include/tray.h declares (tests check the library exports all of them).
EXPORTS = (
    "tray_abi_version",
    "tray_last_error",
    "tray_device_count",
    "tray_shutdown",
    "tray_camera_initialize",
    "tray_rich_scene_camera",
    "tray_default_background",
    "tray_default_scene",
    "tray_rich_scene",
    "tray_rich_scene_capacity",
    "tray_render",
    "tray_render_progress",
    "tray_render_devices",
    "tray_render_devices_progress",
    "tray_release_cache",
    "tray_scale_rgba",
    "tray_scale_rgba_async",
    "tray_scene_upload",
    "tray_scene_release",
    "tray_scene_get_info",
    "tray_render_plan_get",
    "tray_render_async",
    "tray_render_passes_async",
    "tray_render_stats_async",
    "tray_params_rows",
    "tray_to_srgba",
    "tray_linear_to_srgba_async",
)

# Every symbol include/tray_query.h declares (batched ray queries; not in EXPORTS).
QUERY_EXPORTS = (
    "tray_query_version",
    "tray_camera_rays_async",
    "tray_scene_hit_async",
    "tray_ray_color_async",
)

# tray_ray / tray_hit (include/tray_query.h) as numpy structured dtypes, C layout.
RAY_DTYPE = np.dtype([("origin", "<f8", (3,)), ("direction", "<f8", (3,))])
HIT_DTYPE = np.dtype([("point", "<f8", (3,)), ("normal", "<f8", (3,)), ("t", "<f8"), ("index", "<i4"),
                      ("front_face", "<i4")])
assert RAY_DTYPE.itemsize == 48 and HIT_DTYPE.itemsize == 64


class Ray(ctypes.Structure):
    """tray_ray."""
    _fields_ = [("origin", _d3), ("direction", _d3)]


class Hit(ctypes.Structure):
    """tray_hit."""
    _fields_ = [("point", _d3), ("normal", _d3), ("t", ctypes.c_double), ("index", ctypes.c_int32),
                ("front_face", ctypes.c_int32)]


assert ctypes.sizeof(Ray) == 48 and ctypes.sizeof(Hit) == 64

# Every symbol include/tray_shade.h declares (Material.Scatter, AmbientLight.Hit and the
# occlusion query; in neither EXPORTS nor QUERY_EXPORTS).
SHADE_EXPORTS = (
    "tray_shade_version",
    "tray_scatter_async",
    "tray_background_hit_async",
    "tray_scene_occluded_async",
)

# tray_scatter (include/tray_shade.h) as a numpy structured dtype, C layout.
SCATTER_DTYPE = np.dtype([("attenuation", "<f8", (3,)), ("ray", RAY_DTYPE), ("scattered", "<i4"), ("reserved", "<i4")])
assert SCATTER_DTYPE.itemsize == 80 and SCATTER_DTYPE.fields["scattered"][1] == 72


class Scatter(ctypes.Structure):
    """tray_scatter."""
    _fields_ = [("attenuation", _d3), ("ray", Ray), ("scattered", ctypes.c_int32), ("reserved", ctypes.c_int32)]


assert ctypes.sizeof(Scatter) == 80 and Scatter.scattered.offset == 72

# Every symbol include/tray_aov.h declares (the first-hit feature buffers; in none of the
# three lists above).
AOV_EXPORTS = (
    "tray_aov_version",
    "tray_render_aov_async",
)

# The buffers of tray_aov_buffers in declaration order: (name, channels, numpy dtype).
AOV_BUFFERS = (("albedo", 3, np.float64), ("normal", 3, np.float64), ("depth", 1, np.float64),
               ("coverage", 1, np.float64), ("index", 1, np.int32))


class AovBuffers(ctypes.Structure):
    """tray_aov_buffers: device pointers, each nullable."""
    _fields_ = [(name, ctypes.c_void_p) for name, _, _ in AOV_BUFFERS]


assert ctypes.sizeof(AovBuffers) == 40

# Every symbol include/tray_denoise.h declares (the a-trous denoiser guided by the feature
# buffers; in none of the four lists above).
DENOISE_EXPORTS = (
    "tray_denoise_version",
    "tray_denoise_default_params",
    "tray_denoise_workspace_bytes",
    "tray_denoise_async",
)
DENOISE_DEMODULATE = 1  # TRAY_DENOISE_DEMODULATE


class DenoiseGuides(ctypes.Structure):
    """tray_denoise_guides: device pointers, each nullable."""
    _fields_ = [("albedo", ctypes.c_void_p), ("normal", ctypes.c_void_p), ("depth", ctypes.c_void_p)]


class DenoiseParams(ctypes.Structure):
    """tray_denoise_params."""
    _fields_ = [("width", ctypes.c_int32), ("rows", ctypes.c_int32), ("iterations", ctypes.c_int32),
                ("flags", ctypes.c_int32), ("sigma_color", ctypes.c_double), ("sigma_normal", ctypes.c_double),
                ("sigma_depth", ctypes.c_double)]


assert ctypes.sizeof(DenoiseGuides) == 24 and ctypes.sizeof(DenoiseParams) == 40

# Every symbol include/tray_progressive.h declares (the pass accumulator, its convergence
# metric and the variance-guided filter; in none of the five lists above).
PROGRESSIVE_EXPORTS = (
    "tray_progressive_version",
    "tray_accum_metric_default_params",
    "tray_accum_fold_async",
    "tray_accum_fold_metric_async",
    "tray_denoise_variance_default_params",
    "tray_denoise_variance_workspace_bytes",
    "tray_denoise_variance_async",
)


class Accum(ctypes.Structure):
    """tray_accum: the device state (mean, m2) and the host-side frame count."""
    _fields_ = [("mean", ctypes.c_void_p), ("m2", ctypes.c_void_p), ("width", ctypes.c_int32),
                ("rows", ctypes.c_int32), ("count", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class AccumMetricParams(ctypes.Structure):
    """tray_accum_metric_params."""
    _fields_ = [("tolerance", ctypes.c_double), ("floor", ctypes.c_double)]


class AccumMetric(ctypes.Structure):
    """tray_accum_metric: the 16-byte device record."""
    _fields_ = [("unconverged", ctypes.c_uint64), ("max_ratio", ctypes.c_double)]


# tray_accum_metric as a numpy structured dtype, for reading the record back.
ACCUM_METRIC_DTYPE = np.dtype([("unconverged", "<u8"), ("max_ratio", "<f8")])


class DenoiseVarianceParams(ctypes.Structure):
    """tray_denoise_variance_params."""
    _fields_ = [("width", ctypes.c_int32), ("rows", ctypes.c_int32), ("iterations", ctypes.c_int32),
                ("flags", ctypes.c_int32), ("sigma_variance", ctypes.c_double), ("sigma_normal", ctypes.c_double),
                ("sigma_depth", ctypes.c_double), ("epsilon", ctypes.c_double)]


assert ctypes.sizeof(Accum) == 32 and ctypes.sizeof(AccumMetricParams) == 16 and ctypes.sizeof(AccumMetric) == 16
assert ctypes.sizeof(DenoiseVarianceParams) == 48 and ACCUM_METRIC_DTYPE.itemsize == 16

# Every symbol include/tray_adaptive.h declares (the renderer over a pixel list, the fold with
# per-pixel counts and the selection step; in none of the six lists above).
ADAPTIVE_EXPORTS = (
    "tray_adaptive_version",
    "tray_adaptive_default_params",
    "tray_render_pixels_async",
    "tray_adaptive_fold_async",
    "tray_adaptive_workspace_bytes",
    "tray_adaptive_select_async",
)


class AdaptiveState(ctypes.Structure):
    """tray_adaptive_state: the device state (mean, m2, count) of a width x rows image."""
    _fields_ = [("mean", ctypes.c_void_p), ("m2", ctypes.c_void_p), ("count", ctypes.c_void_p),
                ("width", ctypes.c_int32), ("rows", ctypes.c_int32)]


class AdaptiveParams(ctypes.Structure):
    """tray_adaptive_params."""
    _fields_ = [("tolerance", ctypes.c_double), ("floor", ctypes.c_double), ("min_passes", ctypes.c_int32),
                ("max_passes", ctypes.c_int32), ("dilate", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class AdaptiveRecord(ctypes.Structure):
    """tray_adaptive_record: the 32-byte device record."""
    _fields_ = [("n_active", ctypes.c_uint64), ("unconverged", ctypes.c_uint64), ("max_ratio", ctypes.c_double),
                ("pixel_passes", ctypes.c_uint64)]


# tray_adaptive_record as a numpy structured dtype, for reading the record back.
ADAPTIVE_RECORD_DTYPE = np.dtype([("n_active", "<u8"), ("unconverged", "<u8"), ("max_ratio", "<f8"),
                                  ("pixel_passes", "<u8")])
assert ctypes.sizeof(AdaptiveState) == 32 and ctypes.sizeof(AdaptiveParams) == 32
assert ctypes.sizeof(AdaptiveRecord) == 32 and ADAPTIVE_RECORD_DTYPE.itemsize == 32

# Every symbol include/tray_temporal.h declares (the temporal reprojection step; in none of the
# seven lists above).
TEMPORAL_EXPORTS = (
    "tray_temporal_version",
    "tray_temporal_default_params",
    "tray_temporal_step_async",
)


class TemporalState(ctypes.Structure):
    """tray_temporal_state: the device planes (colour, age, index, depth) of a width x height frame."""
    _fields_ = [("colour", ctypes.c_void_p), ("age", ctypes.c_void_p), ("index", ctypes.c_void_p),
                ("depth", ctypes.c_void_p), ("width", ctypes.c_int32), ("height", ctypes.c_int32)]


class TemporalParams(ctypes.Structure):
    """tray_temporal_params."""
    _fields_ = [("max_history", ctypes.c_int32), ("flags", ctypes.c_int32), ("depth_tolerance", ctypes.c_double),
                ("snap", ctypes.c_double), ("reserved", ctypes.c_int64)]


class TemporalRecord(ctypes.Structure):
    """tray_temporal_record: the 16-byte device record."""
    _fields_ = [("fresh", ctypes.c_uint64), ("age_sum", ctypes.c_uint64)]


# tray_temporal_record as a numpy structured dtype, for reading the record back.
TEMPORAL_RECORD_DTYPE = np.dtype([("fresh", "<u8"), ("age_sum", "<u8")])
assert ctypes.sizeof(TemporalState) == 40 and ctypes.sizeof(TemporalParams) == 32
assert ctypes.sizeof(TemporalRecord) == 16 and TEMPORAL_RECORD_DTYPE.itemsize == 16

# Every symbol include/tray_temporal_variance.h declares (the reprojection step that carries M2 and
# the variance of listed pixels; in none of the eight lists above).
TEMPORAL_VARIANCE_EXPORTS = (
    "tray_temporal_var_version",
    "tray_temporal_var_step_async",
    "tray_temporal_var_variance_async",
)


class TemporalVarState(ctypes.Structure):
    """tray_temporal_var_state: a TemporalState's planes plus m2 (height x width x 3 f64)."""
    _fields_ = [("colour", ctypes.c_void_p), ("m2", ctypes.c_void_p), ("age", ctypes.c_void_p),
                ("index", ctypes.c_void_p), ("depth", ctypes.c_void_p), ("width", ctypes.c_int32),
                ("height", ctypes.c_int32)]

    def adaptive(self) -> "AdaptiveState":
        """The same planes as a tray_adaptive_state {mean = colour, m2, count = age, width, rows = height}."""
        return AdaptiveState(self.colour, self.m2, self.age, self.width, self.height)


assert ctypes.sizeof(TemporalVarState) == 48

# Every symbol include/tray_temporal_motion.h declares (the reprojection step across a scene update:
# history follows the moved spheres; in none of the lists above).
TEMPORAL_MOTION_EXPORTS = (
    "tray_temporal_motion_version",
    "tray_temporal_motion_step_async",
)

# include/tray_scene_update.h: new centres and radii for an uploaded scene, its BVH refitted on the
# device (in none of the lists above).
SCENE_UPDATE_EXPORTS = ("tray_scene_update_async", "tray_scene_update")


class SceneUpdateRecord(ctypes.Structure):
    _fields_ = [("applied", ctypes.c_int32), ("n_refused", ctypes.c_int32), ("first_refused", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("extent", ctypes.c_double), ("bound", ctypes.c_double)]


assert ctypes.sizeof(SceneUpdateRecord) == 32
SCENE_UPDATE_RECORD_DTYPE = np.dtype([("applied", "<i4"), ("n_refused", "<i4"), ("first_refused", "<i4"),
                                      ("reserved", "<i4"), ("extent", "<f8"), ("bound", "<f8")])
assert SCENE_UPDATE_RECORD_DTYPE.itemsize == 32
# tray_debug_scene_nodes: Bvh4Node of tray_amd/csrc/bvh.hpp, [axis][low, high][child slot].
NODE_DTYPE = np.dtype([("box", "<f4", (3, 2, 4)), ("ref", "<u4", (4,)), ("pad", "<u4", (4,))])
assert NODE_DTYPE.itemsize == 128

# include/tray_debug.h: test / A-B hooks outside the stable ABI (not in EXPORTS).
DEBUG_EXPORTS = ("tray_debug_set", "tray_debug_clear", "tray_debug_progress_counts", "tray_debug_plain_instance",
                 "tray_debug_plain_launches", "tray_debug_phase_trigger", "tray_debug_query_traversal",
                 "tray_debug_scene_nodes", "tray_debug_scene_leaves")
# tray_debug_phase_trigger's phases.
TRIGGER_PHASES = {"leaf": 0, "shade": 1, "refill": 2}
DEBUG_KNOBS = ("acc_slots", "band_samples", "bvh_leaf", "bvh_lds_mode", "stack_lds_slots", "node_deep",
               "primary_candidates", "resolve_staged", "wave_chunks", "scene_contexts", "grid_reserve",
               "work_order", "coop_lanes", "plain_instance")
# tray_debug_plain_instance's `facts` bits (TRAY_PLAIN_FACT_*).
PLAIN_FACTS = {"bvh": 1, "stats": 2, "progress": 4, "stack_spill": 8, "segments": 16, "counting": 32,
               "candidates": 64, "work_order": 128}
# tray_debug_query_traversal's kinds (TRAY_QUERY_KIND_*).
QUERY_KINDS = {"plain": 0, "pixels": 1, "temporal": 2}

# tray_progress_fn: void (*)(int32_t rows, void *user)
PROGRESS_FN = ctypes.CFUNCTYPE(None, ctypes.c_int32, ctypes.c_void_p)

_libs: dict = {}


def _torch_first() -> None:
    """Load torch (when it is installed) before the library. Both link a HIP
    runtime with the same soname (libamdhip64.so.7): torch bundles its own, the
    library was linked against /opt/rocm's. Whichever is mapped first serves
    both, and torch does not work on /opt/rocm's (it then sees no GPU), while
    the library's C-ABI works on either. Importing torch here makes the import
    order of `tray_amd` and `torch` irrelevant to the caller."""
    import importlib.util

    if "torch" in sys.modules or importlib.util.find_spec("torch") is None:
        return
    import torch  # noqa: F401


def lib(path: str | None = None) -> ctypes.CDLL:
    """The C-ABI library (default: the in-tree build). `path` loads another build
    of the same ABI (used by tools/ab_bench.py to compare kernel variants)."""
    path = path or LIB_PATH
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: the HIP renderer is not built. Run `make -C tray_amd` "
            "(or __graft_entry__.build()). There is no CPU fallback."
        )
    _torch_first()
    L = ctypes.CDLL(path)
    vp, i32, u32p = ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_uint32)
    L.tray_abi_version.restype = i32
    L.tray_last_error.restype = ctypes.c_char_p
    L.tray_device_count.argtypes = [ctypes.POINTER(i32)]
    L.tray_camera_initialize.argtypes = [ctypes.POINTER(CameraSetup), i32, i32, ctypes.POINTER(CameraState)]
    L.tray_rich_scene_camera.argtypes = [ctypes.POINTER(CameraSetup)]
    L.tray_default_background.argtypes = [ctypes.POINTER(Background)]
    L.tray_default_scene.argtypes = [vp, i32, ctypes.POINTER(i32)]
    L.tray_rich_scene.argtypes = [ctypes.c_uint64, i32, vp, i32, ctypes.POINTER(i32)]
    L.tray_rich_scene_capacity.argtypes = [i32]
    L.tray_rich_scene_capacity.restype = i32
    L.tray_render.argtypes = [vp, i32, ctypes.POINTER(Background), ctypes.POINTER(CameraState),
                              ctypes.POINTER(Params), i32, vp, u32p]
    if hasattr(L, "tray_render_progress"):  # absent from older builds (A/B tools)
        L.tray_render_progress.argtypes = L.tray_render.argtypes + [PROGRESS_FN, vp]
    if hasattr(L, "tray_render_devices"):
        L.tray_render_devices.argtypes = [vp, i32, ctypes.POINTER(Background), ctypes.POINTER(CameraState),
                                          ctypes.POINTER(Params), ctypes.POINTER(i32), i32, vp, u32p]
    if hasattr(L, "tray_render_devices_progress"):
        L.tray_render_devices_progress.argtypes = L.tray_render_devices.argtypes + [PROGRESS_FN, vp]
    if hasattr(L, "tray_release_cache"):
        L.tray_release_cache.argtypes = [i32]
    if hasattr(L, "tray_scale_rgba"):
        L.tray_scale_rgba.argtypes = [vp, i32, i32, vp, i32, i32, i32, i32]
        L.tray_scale_rgba_async.argtypes = [vp, i32, i32, vp, i32, i32, i32, i32, vp]
    if hasattr(L, "tray_linear_to_srgba_async"):
        L.tray_linear_to_srgba_async.argtypes = [vp, ctypes.c_size_t, vp, i32, vp]
    L.tray_scene_upload.argtypes = [vp, i32, ctypes.POINTER(Background), i32, ctypes.POINTER(vp)]
    L.tray_scene_release.argtypes = [vp]
    if hasattr(L, "tray_scene_get_info"):  # absent from builds older than this binding (A/B tools)
        L.tray_scene_get_info.argtypes = [vp, ctypes.POINTER(SceneInfo)]
    if hasattr(L, "tray_render_plan_get"):
        L.tray_render_plan_get.argtypes = [vp, ctypes.POINTER(CameraState), ctypes.POINTER(Params), i32,
                                           ctypes.POINTER(RenderPlan)]
    L.tray_render_async.argtypes = [vp, ctypes.POINTER(CameraState), ctypes.POINTER(Params), vp, vp, vp]
    L.tray_render_stats_async.argtypes = [vp, ctypes.POINTER(CameraState), ctypes.POINTER(Params), vp, vp, vp]
    if hasattr(L, "tray_render_passes_async"):  # absent from older builds (A/B tools)
        L.tray_render_passes_async.argtypes = [vp, ctypes.POINTER(CameraState), ctypes.POINTER(Params), i32, vp, vp]
    L.tray_params_rows.argtypes = [ctypes.POINTER(Params)]
    L.tray_params_rows.restype = i32
    L.tray_to_srgba.argtypes = [vp, ctypes.c_size_t, vp]
    if hasattr(L, "tray_query_version"):  # include/tray_query.h; absent from older builds (A/B tools)
        L.tray_query_version.restype = i32
        L.tray_camera_rays_async.argtypes = [ctypes.POINTER(CameraState), ctypes.POINTER(Params), i32, vp, vp, vp]
        L.tray_scene_hit_async.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_double, i32, vp, vp]
        L.tray_ray_color_async.argtypes = [vp, vp, vp, ctypes.c_int64, i32, ctypes.c_uint64, i32, vp, vp, vp]
    if hasattr(L, "tray_shade_version"):  # include/tray_shade.h; absent from older builds (A/B tools)
        L.tray_shade_version.restype = i32
        L.tray_scatter_async.argtypes = [vp, vp, vp, vp, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64, vp, vp]
        L.tray_background_hit_async.argtypes = [ctypes.POINTER(Background), vp, ctypes.c_int64, vp, i32, vp]
        L.tray_scene_occluded_async.argtypes = [vp, vp, vp, ctypes.c_int64, ctypes.c_double, i32, vp, vp]
    if hasattr(L, "tray_aov_version"):  # include/tray_aov.h; absent from older builds (A/B tools)
        L.tray_aov_version.restype = i32
        L.tray_render_aov_async.argtypes = [vp, ctypes.POINTER(CameraState), ctypes.POINTER(Params),
                                            ctypes.POINTER(AovBuffers), vp]
    if hasattr(L, "tray_denoise_version"):  # include/tray_denoise.h; absent from older builds (A/B tools)
        L.tray_denoise_version.restype = i32
        L.tray_denoise_default_params.argtypes = [i32, i32, ctypes.POINTER(DenoiseParams)]
        L.tray_denoise_workspace_bytes.argtypes = [ctypes.POINTER(DenoiseParams), ctypes.POINTER(ctypes.c_size_t)]
        L.tray_denoise_async.argtypes = [vp, ctypes.POINTER(DenoiseGuides), ctypes.POINTER(DenoiseParams), vp, vp,
                                         ctypes.c_size_t, i32, vp]
    if hasattr(L, "tray_progressive_version"):  # include/tray_progressive.h; absent from older builds (A/B tools)
        L.tray_progressive_version.restype = i32
        L.tray_accum_metric_default_params.argtypes = [ctypes.POINTER(AccumMetricParams)]
        L.tray_accum_fold_async.argtypes = [ctypes.POINTER(Accum), vp, i32, i32, vp]
        L.tray_accum_fold_metric_async.argtypes = [ctypes.POINTER(Accum), vp, i32, ctypes.POINTER(AccumMetricParams),
                                                   vp, vp, i32, vp]
        L.tray_denoise_variance_default_params.argtypes = [i32, i32, ctypes.POINTER(DenoiseVarianceParams)]
        L.tray_denoise_variance_workspace_bytes.argtypes = [ctypes.POINTER(DenoiseVarianceParams),
                                                            ctypes.POINTER(ctypes.c_size_t)]
        L.tray_denoise_variance_async.argtypes = [vp, vp, ctypes.POINTER(DenoiseGuides),
                                                  ctypes.POINTER(DenoiseVarianceParams), vp, vp, vp, ctypes.c_size_t,
                                                  i32, vp]
    if hasattr(L, "tray_adaptive_version"):  # include/tray_adaptive.h; absent from older builds (A/B tools)
        L.tray_adaptive_version.restype = i32
        L.tray_adaptive_default_params.argtypes = [ctypes.POINTER(AdaptiveParams)]
        L.tray_render_pixels_async.argtypes = [vp, ctypes.POINTER(CameraState), ctypes.POINTER(Params), vp,
                                               ctypes.c_int64, vp, i32, vp, vp, vp]
        L.tray_adaptive_fold_async.argtypes = [ctypes.POINTER(AdaptiveState), vp, ctypes.c_int64, vp, i32, i32, vp]
        L.tray_adaptive_workspace_bytes.argtypes = [i32, i32, ctypes.POINTER(ctypes.c_size_t)]
        L.tray_adaptive_select_async.argtypes = [ctypes.POINTER(AdaptiveState), ctypes.POINTER(AdaptiveParams), vp, vp,
                                                 vp, vp, ctypes.c_size_t, i32, vp]
    if hasattr(L, "tray_temporal_version"):  # include/tray_temporal.h; absent from older builds (A/B tools)
        L.tray_temporal_version.restype = i32
        L.tray_temporal_default_params.argtypes = [ctypes.POINTER(TemporalParams)]
        L.tray_temporal_step_async.argtypes = [vp, ctypes.POINTER(CameraState), ctypes.POINTER(CameraState),
                                               ctypes.POINTER(TemporalParams), vp, ctypes.POINTER(TemporalState),
                                               ctypes.POINTER(TemporalState), vp, vp]
    if hasattr(L, "tray_temporal_var_version"):  # include/tray_temporal_variance.h; absent from older builds
        L.tray_temporal_var_version.restype = i32
        L.tray_temporal_var_step_async.argtypes = [vp, ctypes.POINTER(CameraState), ctypes.POINTER(CameraState),
                                                   ctypes.POINTER(TemporalParams), vp,
                                                   ctypes.POINTER(TemporalVarState),
                                                   ctypes.POINTER(TemporalVarState), vp, vp, vp]
        L.tray_temporal_var_variance_async.argtypes = [ctypes.POINTER(TemporalVarState), vp, ctypes.c_int64, vp, i32,
                                                       vp]
    if hasattr(L, "tray_temporal_motion_version"):  # include/tray_temporal_motion.h; absent from older builds
        L.tray_temporal_motion_version.restype = i32
        L.tray_temporal_motion_step_async.argtypes = [vp, ctypes.POINTER(CameraState), ctypes.POINTER(CameraState),
                                                      vp, i32, ctypes.POINTER(TemporalParams), vp,
                                                      ctypes.POINTER(TemporalVarState),
                                                      ctypes.POINTER(TemporalVarState), vp, vp, vp, vp]
    if hasattr(L, "tray_scene_update_async"):  # include/tray_scene_update.h; absent from older builds (A/B tools)
        L.tray_scene_update_async.argtypes = [vp, vp, i32, vp, vp]
        L.tray_scene_update.argtypes = [vp, vp, i32, ctypes.POINTER(SceneUpdateRecord)]
    if hasattr(L, "tray_debug_scene_nodes"):
        L.tray_debug_scene_nodes.argtypes = [vp, vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
        L.tray_debug_scene_leaves.argtypes = [vp, vp, i32, vp, i32, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    if hasattr(L, "tray_debug_set"):  # absent from older builds (A/B tools)
        L.tray_debug_set.argtypes = [ctypes.c_char_p, ctypes.c_int64]
        L.tray_debug_clear.argtypes = [ctypes.c_char_p]
    if hasattr(L, "tray_debug_progress_counts"):
        L.tray_debug_progress_counts.argtypes = [ctypes.c_int32, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int32,
                                                 ctypes.POINTER(ctypes.c_int32)]
    if hasattr(L, "tray_debug_plain_instance"):  # absent from older builds (A/B tools)
        L.tray_debug_plain_instance.argtypes = [ctypes.c_uint32] + [i32] * 7 + [ctypes.POINTER(i32)]
        L.tray_debug_plain_launches.argtypes = [ctypes.POINTER(ctypes.c_uint64)]
    if hasattr(L, "tray_debug_phase_trigger"):  # absent from older builds (A/B tools)
        L.tray_debug_phase_trigger.argtypes = [i32, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(i32)]
    if hasattr(L, "tray_debug_query_traversal"):  # absent from older builds (A/B tools)
        L.tray_debug_query_traversal.argtypes = [i32, i32, ctypes.POINTER(i32)]
    _libs[path] = L
    return L


def check(rc: int) -> None:
    if rc != TRAY_OK:
        msg = lib().tray_last_error()
        raise TrayError(rc, msg.decode() if msg else "")


_knobs_now: dict = {}  # the knobs this process has set (they are process-wide in the library)


def set_debug_knobs(lib_path: str | None = None, **knobs) -> dict:
    """Sets include/tray_debug.h knobs (None unsets one) and returns their
    previous values. Test and A/B use only: the library never reads the
    environment, so this is the one way to reach them."""
    unknown = set(knobs) - set(DEBUG_KNOBS)
    if unknown:
        raise ValueError(f"unknown debug knobs {sorted(unknown)}")
    L = lib(lib_path)
    before = {k: _knobs_now.get(k) for k in knobs}
    for name, value in knobs.items():
        if value is None:
            rc = L.tray_debug_clear(name.encode())
            _knobs_now.pop(name, None)
        else:
            rc = L.tray_debug_set(name.encode(), int(value))
            _knobs_now[name] = int(value)
        if rc != TRAY_OK:
            raise TrayError(rc, L.tray_last_error().decode())
    return before


def progress_counts(device: int = 0) -> np.ndarray:
    """tray_debug_progress_counts: finished samples per 8-row tile row as the kernel counted them
    during the last render(..., progress=...) on `device`."""
    n = ctypes.c_int32(0)
    check(lib().tray_debug_progress_counts(device, None, 0, ctypes.byref(n)))
    counts = np.zeros(n.value, dtype=np.uint64)
    if n.value:
        check(lib().tray_debug_progress_counts(device, counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), n.value,
                                               ctypes.byref(n)))
    return counts


def plain_instance(facts, rays_per_pixel: int, tile_rows: int, n_global: int, n_nodes: int, leaf_max: int, acc: int,
                   lds_mode: int) -> bool:
    """tray_debug_plain_instance: whether a launch with these properties (`facts`: names of
    PLAIN_FACTS) takes the megakernel's plain-frame instance. Host only."""
    bits = 0
    for name in facts:
        bits |= PLAIN_FACTS[name]
    out = ctypes.c_int32(-1)
    check(lib().tray_debug_plain_instance(bits, rays_per_pixel, tile_rows, n_global, n_nodes, leaf_max, acc,
                                          lds_mode, ctypes.byref(out)))
    return out.value == 1


def plain_launches() -> int:
    """tray_debug_plain_launches: launches that took the plain-frame instance so far."""
    n = ctypes.c_uint64(0)
    check(lib().tray_debug_plain_launches(ctypes.byref(n)))
    return int(n.value)


def phase_trigger(phase: str, waiting: int, traversing: int) -> bool:
    """tray_debug_phase_trigger: whether the plain-frame instance runs `phase` (a name of
    TRIGGER_PHASES) with `waiting` lanes gathered and `traversing` lanes in flight. Host only."""
    out = ctypes.c_int32(-1)
    check(lib().tray_debug_phase_trigger(TRIGGER_PHASES[phase], waiting, traversing, ctypes.byref(out)))
    return out.value == 1


def query_traversal(kind: str, stack_depth: int) -> bool:
    """tray_debug_query_traversal: whether a launch of `kind` (a name of QUERY_KINDS) on a scene with
    a BVH of tray_scene_info's `stack_depth` traverses the tree (True) or scans. Host only."""
    out = ctypes.c_int32(-1)
    check(lib().tray_debug_query_traversal(QUERY_KINDS[kind], stack_depth, ctypes.byref(out)))
    return out.value == 1


def clear_debug_knobs(lib_path: str | None = None) -> None:
    check(lib(lib_path).tray_debug_clear(None))
    _knobs_now.clear()


class debug_knobs:
    """`with debug_knobs(acc_slots=0): ...` sets knobs for the block and restores
    the previous values on exit."""

    def __init__(self, lib_path: str | None = None, **knobs):
        unknown = set(knobs) - set(DEBUG_KNOBS)
        if unknown:
            raise ValueError(f"unknown debug knobs {sorted(unknown)}")
        self.lib_path, self.knobs, self.saved = lib_path, knobs, {}

    def __enter__(self):
        self.saved = set_debug_knobs(self.lib_path, **self.knobs)
        return self

    def __exit__(self, et, ev, tb):
        set_debug_knobs(self.lib_path, **self.saved)
        return False


def code_object_sha256(path: str | None = None) -> str | None:
    """sha256 of the device code (the ELF section .hip_fatbin: every gfx950 kernel
    of the library) of a libtray_amd.so build. Profile records carry it
    (tools/pmc_summary.py, tools/pmc_mix.py) so that bench.py reuses counter
    figures only for the device code they were measured on; host-only changes
    leave it unchanged. None when the file has no such section."""
    import hashlib
    import struct

    with open(path or LIB_PATH, "rb") as f:
        data = f.read()
    if data[:4] != b"\x7fELF" or data[4] != 2 or data[5] != 1:  # ELF64, little endian
        return None
    shoff = struct.unpack_from("<Q", data, 0x28)[0]
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", data, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    names = secs[shstrndx][4]
    for name_off, _type, _flags, _addr, off, size, *_ in secs:
        end = data.index(b"\0", names + name_off)
        if data[names + name_off:end] == b".hip_fatbin":
            return hashlib.sha256(data[off:off + size]).hexdigest()
    return None


def device_count() -> int:
    n = ctypes.c_int32(0)
    check(lib().tray_device_count(ctypes.byref(n)))
    return n.value


def spheres_array(spheres) -> np.ndarray:
    a = np.ascontiguousarray(spheres if spheres is not None else np.zeros(0, SPHERE_DTYPE))
    if a.dtype != SPHERE_DTYPE:
        raise TypeError("spheres must use tray_amd._lib.SPHERE_DTYPE")
    return a


def make_params(width, height, max_depth, rays_per_pixel, ray_radius, seed, y_start=0, y_end=None,
                tile_rows=0, tile_count=1, tile_index=0, output=OUT_RGB_F64, flags=0, pass_=0) -> Params:
    return Params(width, height, max_depth, rays_per_pixel, float(ray_radius), int(seed) & (2**64 - 1), y_start,
                  height if y_end is None else y_end, tile_rows, tile_count, tile_index, output, flags, pass_)


def params_rows(p: Params) -> int:
    return int(lib().tray_params_rows(ctypes.byref(p)))


def render(spheres, background: Background, camera: CameraState, params: Params, device: int = 0,
           segments: bool = False, progress=None):
    """Synchronous tray_render into host memory. Returns (pixels, segments-or-None);
    pixels is (rows, W, 3) f64 / (rows, W, 3) f32 / (rows, W, 4) u8 by params.output.
    progress(rows): called (tray_render_progress) as rows finish while the device renders."""
    s = spheres_array(spheres)
    rows = params_rows(params)
    shape = {OUT_RGB_F64: (rows, params.width, 3), OUT_RGB_F32: (rows, params.width, 3),
             OUT_RGBA8: (rows, params.width, 4)}[params.output]
    dtype = {OUT_RGB_F64: np.float64, OUT_RGB_F32: np.float32, OUT_RGBA8: np.uint8}[params.output]
    out = np.zeros(shape, dtype=dtype)
    seg = np.zeros((rows, params.width), dtype=np.uint32) if segments else None
    args = (s.ctypes.data if len(s) else None, len(s), ctypes.byref(background), ctypes.byref(camera),
            ctypes.byref(params), device, out.ctypes.data,
            seg.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) if seg is not None else None)
    if progress is None:
        check(lib().tray_render(*args))
    else:
        with _Progress(progress) as cb:
            check(lib().tray_render_progress(*args, cb.fn, None))
    return out, seg


class _Progress:
    """A Python progress callback behind tray_progress_fn. ctypes swallows an
    exception raised inside a callback; this keeps the first one, stops calling
    the function after it, and re-raises it when the render returns."""

    def __init__(self, fn):
        self.user, self.error = fn, None
        self.fn = PROGRESS_FN(self._call)  # kept alive for the call

    def _call(self, rows, _user):
        if self.error is not None:
            return
        try:
            self.user(int(rows))
        except BaseException as e:  # noqa: BLE001 - re-raised after the render
            self.error = e

    def __enter__(self):
        return self

    def __exit__(self, et, ev, tb):
        if et is None and self.error is not None:
            raise self.error
        return False


def render_devices(spheres, background: Background, camera: CameraState, params: Params, devices,
                   segments: bool = False, progress=None):
    """tray_render_devices: the row set split over `devices` (interleaved 1-row
    tiles, a device may repeat), rows returned in image order like render().
    progress(rows): tray_render_devices_progress, called as rows finish on any device."""
    s = spheres_array(spheres)
    rows = params_rows(params)
    ch = 4 if params.output == OUT_RGBA8 else 3
    dtype = {OUT_RGB_F64: np.float64, OUT_RGB_F32: np.float32, OUT_RGBA8: np.uint8}[params.output]
    out = np.zeros((rows, params.width, ch), dtype=dtype)
    seg = np.zeros((rows, params.width), dtype=np.uint32) if segments else None
    devs = (ctypes.c_int32 * len(devices))(*devices)
    args = (s.ctypes.data if len(s) else None, len(s), ctypes.byref(background), ctypes.byref(camera),
            ctypes.byref(params), devs, len(devices), out.ctypes.data,
            seg.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) if seg is not None else None)
    if progress is None:
        check(lib().tray_render_devices(*args))
    else:
        with _Progress(progress) as cb:
            check(lib().tray_render_devices_progress(*args, cb.fn, None))
    return out, seg


SCALE_NEAREST, SCALE_BILINEAR = 0, 1  # tray_scale_filter


def scale_rgba(src: np.ndarray, dw: int, dh: int, bilinear: bool, dst: np.ndarray | None = None,
               device: int = 0) -> np.ndarray:
    """tray_scale_rgba: x/image/draw BiLinear / NearestNeighbor .Scale of an [H, W, 4]
    uint8 image onto dst (a fresh zero image by default, as main.go:123), on the device."""
    a = np.ascontiguousarray(src, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError("src must be [H, W, 4] uint8")
    out = np.zeros((dh, dw, 4), dtype=np.uint8) if dst is None else np.array(dst, dtype=np.uint8, copy=True)
    if out.shape != (dh, dw, 4):
        raise ValueError("dst must be [dh, dw, 4] uint8")
    check(lib().tray_scale_rgba(a.ctypes.data, a.shape[1], a.shape[0], out.ctypes.data, dw, dh,
                                SCALE_BILINEAR if bilinear else SCALE_NEAREST, device))
    return out


def release_cache(device: int = -1) -> None:
    """tray_release_cache: free what the synchronous renders keep on `device` (all: -1)."""
    check(lib().tray_release_cache(int(device)))


def linear_to_srgba_async(rgb_ptr: int, n_pixels: int, rgba_ptr: int, device: int = 0, stream: int | None = None):
    """tray_linear_to_srgba_async: ColorF.ToSRGBA over device buffers (n x 3 f64 -> n x 4 u8)."""
    check(lib().tray_linear_to_srgba_async(rgb_ptr, n_pixels, rgba_ptr, device, stream))


def _raise(L, rc: int) -> None:
    if rc != TRAY_OK:
        raise TrayError(rc, L.tray_last_error().decode())


def _override(p, overrides: dict, noun: str):
    """The parameter struct `p` with fields set by name; ValueError for a name it does not have."""
    for name, value in overrides.items():
        if name not in dict(type(p)._fields_):
            raise ValueError(f"unknown {noun} parameter {name!r}")
        setattr(p, name, value)
    return p


def denoise_params(width: int, rows: int, lib_path: str | None = None, **overrides) -> DenoiseParams:
    """tray_denoise_default_params for a width x rows image, with fields overridden by name."""
    p = DenoiseParams()
    L = lib(lib_path)
    _raise(L, L.tray_denoise_default_params(int(width), int(rows), ctypes.byref(p)))
    return _override(p, overrides, "denoise")


def denoise_workspace_bytes(params: DenoiseParams, lib_path: str | None = None) -> int:
    n = ctypes.c_size_t(0)
    L = lib(lib_path)
    _raise(L, L.tray_denoise_workspace_bytes(ctypes.byref(params), ctypes.byref(n)))
    return int(n.value)


def denoise_async(colour_ptr: int, params: DenoiseParams, out_ptr: int, workspace_ptr: int | None,
                  workspace_bytes: int, albedo_ptr: int | None = None, normal_ptr: int | None = None,
                  depth_ptr: int | None = None, device: int = 0, stream: int | None = None,
                  lib_path: str | None = None) -> None:
    """tray_denoise_async: the guided a-trous filter of include/tray_denoise.h over device buffers
    (rows x width x 3 f64 in and out; a None guide drops its term). Only enqueues on `stream`."""
    guides = DenoiseGuides(albedo_ptr, normal_ptr, depth_ptr)
    L = lib(lib_path)
    _raise(L, L.tray_denoise_async(colour_ptr, ctypes.byref(guides), ctypes.byref(params), out_ptr, workspace_ptr,
                                   int(workspace_bytes), int(device), stream))


def accum_metric_params(lib_path: str | None = None, **overrides) -> AccumMetricParams:
    """tray_accum_metric_default_params, with fields (tolerance, floor) overridden by name."""
    p = AccumMetricParams()
    L = lib(lib_path)
    _raise(L, L.tray_accum_metric_default_params(ctypes.byref(p)))
    return _override(p, overrides, "metric")


def accum_fold_async(acc: Accum, frames_ptr: int | None, n_frames: int, device: int = 0, stream: int | None = None,
                     lib_path: str | None = None) -> None:
    """tray_accum_fold_async: folds n_frames device frames (rows x width x 3 f64 each, consecutive)
    into acc's running mean and M2 in one launch; acc.count is updated. Only enqueues on `stream`."""
    L = lib(lib_path)
    _raise(L, L.tray_accum_fold_async(ctypes.byref(acc), frames_ptr, int(n_frames), int(device), stream))


def accum_fold_metric_async(acc: Accum, frames_ptr: int | None, n_frames: int, metric_params: AccumMetricParams,
                            variance_ptr: int | None = None, metric_ptr: int | None = None, device: int = 0,
                            stream: int | None = None, lib_path: str | None = None) -> None:
    """tray_accum_fold_metric_async: the fold with the variance of the mean (rows x width x 3 f64) and
    the 16-byte convergence record (ACCUM_METRIC_DTYPE) of the state after it, in the same launch."""
    L = lib(lib_path)
    _raise(L, L.tray_accum_fold_metric_async(ctypes.byref(acc), frames_ptr, int(n_frames),
                                             ctypes.byref(metric_params), variance_ptr, metric_ptr, int(device),
                                             stream))


def denoise_variance_params(width: int, rows: int, lib_path: str | None = None, **overrides) -> DenoiseVarianceParams:
    """tray_denoise_variance_default_params for a width x rows image, with fields overridden by name."""
    p = DenoiseVarianceParams()
    L = lib(lib_path)
    _raise(L, L.tray_denoise_variance_default_params(int(width), int(rows), ctypes.byref(p)))
    return _override(p, overrides, "variance-guided denoise")


def denoise_variance_workspace_bytes(params: DenoiseVarianceParams, lib_path: str | None = None) -> int:
    n = ctypes.c_size_t(0)
    L = lib(lib_path)
    _raise(L, L.tray_denoise_variance_workspace_bytes(ctypes.byref(params), ctypes.byref(n)))
    return int(n.value)


def denoise_variance_async(colour_ptr: int, variance_ptr: int, params: DenoiseVarianceParams, out_ptr: int,
                           workspace_ptr: int | None, workspace_bytes: int, albedo_ptr: int | None = None,
                           normal_ptr: int | None = None, depth_ptr: int | None = None,
                           variance_out_ptr: int | None = None, device: int = 0, stream: int | None = None,
                           lib_path: str | None = None) -> None:
    """tray_denoise_variance_async: the a-trous filter with its colour bandwidth set per pixel from
    the variance of the mean (rows x width x 3 f64); variance_out: rows x width f64, the last level's
    noise plane. Only enqueues on `stream`."""
    guides = DenoiseGuides(albedo_ptr, normal_ptr, depth_ptr)
    L = lib(lib_path)
    _raise(L, L.tray_denoise_variance_async(colour_ptr, variance_ptr, ctypes.byref(guides), ctypes.byref(params),
                                            out_ptr, variance_out_ptr, workspace_ptr, int(workspace_bytes),
                                            int(device), stream))


def adaptive_params(lib_path: str | None = None, **overrides) -> AdaptiveParams:
    """tray_adaptive_default_params, with fields overridden by name."""
    p = AdaptiveParams()
    L = lib(lib_path)
    _raise(L, L.tray_adaptive_default_params(ctypes.byref(p)))
    return _override(p, overrides, "adaptive")


def adaptive_workspace_bytes(width: int, rows: int, lib_path: str | None = None) -> int:
    n = ctypes.c_size_t(0)
    L = lib(lib_path)
    _raise(L, L.tray_adaptive_workspace_bytes(int(width), int(rows), ctypes.byref(n)))
    return int(n.value)


def adaptive_fold_async(state: AdaptiveState, pixels_ptr: int | None, n_pixels: int, values_ptr: int | None,
                        n_passes: int, device: int = 0, stream: int | None = None,
                        lib_path: str | None = None) -> None:
    """tray_adaptive_fold_async: folds n_passes values (n_passes x n_pixels x 3 f64, pass-major) of the
    listed (distinct) compact pixels into the state, each at its own count. Only enqueues on `stream`."""
    L = lib(lib_path)
    _raise(L, L.tray_adaptive_fold_async(ctypes.byref(state), pixels_ptr, int(n_pixels), values_ptr, int(n_passes),
                                         int(device), stream))


def adaptive_select_async(state: AdaptiveState, params: AdaptiveParams, pixels_ptr: int, record_ptr: int,
                          workspace_ptr: int | None, workspace_bytes: int, variance_ptr: int | None = None,
                          device: int = 0, stream: int | None = None, lib_path: str | None = None) -> None:
    """tray_adaptive_select_async: the per-pixel metric, the dilation and the ascending list of the
    active pixels (rows x width u32), with the 32-byte record (ADAPTIVE_RECORD_DTYPE) and, when
    asked for, the variance of the mean (rows x width x 3 f64). Only enqueues on `stream`."""
    L = lib(lib_path)
    _raise(L, L.tray_adaptive_select_async(ctypes.byref(state), ctypes.byref(params), variance_ptr, pixels_ptr,
                                           record_ptr, workspace_ptr, int(workspace_bytes), int(device), stream))


def temporal_params(lib_path: str | None = None, **overrides) -> TemporalParams:
    """tray_temporal_default_params, with fields overridden by name."""
    p = TemporalParams()
    L = lib(lib_path)
    _raise(L, L.tray_temporal_default_params(ctypes.byref(p)))
    return _override(p, overrides, "temporal")


def temporal_step_async(scene_handle: int | None, camera: CameraState | None, prev_camera: CameraState | None,
                        params: TemporalParams, frame_ptr: int | None, history: TemporalState | None,
                        out: TemporalState, record_ptr: int | None = None, stream: int | None = None,
                        lib_path: str | None = None) -> None:
    """tray_temporal_step_async on an uploaded scene's handle: reprojects `history` (a frame of
    prev_camera; both None: the first frame) into `camera`, folds the new frame (height x width x 3
    f64) into it and writes `out` and the 16-byte record (TEMPORAL_RECORD_DTYPE). Only enqueues
    on `stream`."""
    L = lib(lib_path)
    _raise(L, L.tray_temporal_step_async(scene_handle, ctypes.byref(camera) if camera is not None else None,
                                         ctypes.byref(prev_camera) if prev_camera is not None else None,
                                         ctypes.byref(params), frame_ptr,
                                         ctypes.byref(history) if history is not None else None, ctypes.byref(out),
                                         record_ptr, stream))


def temporal_var_step_async(scene_handle: int | None, camera: CameraState | None, prev_camera: CameraState | None,
                            params: TemporalParams, frame_ptr: int | None, history: TemporalVarState | None,
                            out: TemporalVarState, variance_ptr: int | None = None, record_ptr: int | None = None,
                            stream: int | None = None, lib_path: str | None = None) -> None:
    """tray_temporal_var_step_async: temporal_step_async on states that carry m2, with the variance of
    the mean (height x width x 3 f64, nullable) written in the same launch. Only enqueues on `stream`."""
    L = lib(lib_path)
    _raise(L, L.tray_temporal_var_step_async(scene_handle, ctypes.byref(camera) if camera is not None else None,
                                             ctypes.byref(prev_camera) if prev_camera is not None else None,
                                             ctypes.byref(params), frame_ptr,
                                             ctypes.byref(history) if history is not None else None,
                                             ctypes.byref(out), variance_ptr, record_ptr, stream))


def temporal_motion_step_async(scene_handle: int | None, camera: CameraState | None, prev_camera: CameraState | None,
                               prev_geometry_ptr: int | None, n_spheres: int, params: TemporalParams,
                               frame_ptr: int | None, history: TemporalVarState | None, out: TemporalVarState,
                               variance_ptr: int | None = None, motion_ptr: int | None = None,
                               record_ptr: int | None = None, stream: int | None = None,
                               lib_path: str | None = None) -> None:
    """tray_temporal_motion_step_async: the temporal step on a scene whose spheres moved since `history`
    was made. The scene holds the current geometry; prev_geometry_ptr -> n_spheres x {cx, cy, cz, radius}
    f64 on the device, what it held then. States with m2 (all or none of them) take the step of
    temporal_var_step_async, states without (m2 None) that of temporal_step_async; motion_ptr
    (height x width x 2 f64, nullable) receives the screen-space motion vectors. Only enqueues on
    `stream`."""
    L = lib(lib_path)
    _raise(L, L.tray_temporal_motion_step_async(scene_handle, ctypes.byref(camera) if camera is not None else None,
                                                ctypes.byref(prev_camera) if prev_camera is not None else None,
                                                prev_geometry_ptr, int(n_spheres), ctypes.byref(params), frame_ptr,
                                                ctypes.byref(history) if history is not None else None,
                                                ctypes.byref(out), variance_ptr, motion_ptr, record_ptr, stream))


def temporal_var_variance_async(state: TemporalVarState, pixels_ptr: int | None, n_pixels: int,
                                variance_ptr: int | None, device: int = 0, stream: int | None = None,
                                lib_path: str | None = None) -> None:
    """tray_temporal_var_variance_async: the variance of the mean of the listed pixels (n_pixels u32;
    None: every pixel) from the state's m2 and age; unlisted pixels keep their bytes. Only enqueues
    on `stream`."""
    L = lib(lib_path)
    _raise(L, L.tray_temporal_var_variance_async(ctypes.byref(state), pixels_ptr, int(n_pixels), variance_ptr,
                                                 int(device), stream))


def camera_rays_count(params: Params) -> int:
    """Rays tray_camera_rays_async writes for `params`: rows x width x rays_per_pixel."""
    return params_rows(params) * params.width * params.rays_per_pixel


def camera_rays_async(camera: CameraState, params: Params, rays_ptr: int, ids_ptr: int | None = None,
                      device: int = 0, stream: int | None = None) -> None:
    """tray_camera_rays_async: Camera.GetRay for every sample of params' row set into
    device buffers (camera_rays_count(params) x tray_ray; ids: 2 x uint32 per ray)."""
    check(lib().tray_camera_rays_async(ctypes.byref(camera), ctypes.byref(params), device, rays_ptr, ids_ptr, stream))


def background_hit_async(background: Background, rays_ptr: int, n: int, rgb_ptr: int, device: int = 0,
                         stream: int | None = None) -> None:
    """tray_background_hit_async: AmbientLight.Hit for n device rays -> n x 3 f64. Needs no scene."""
    check(lib().tray_background_hit_async(ctypes.byref(background), rays_ptr, int(n), rgb_ptr, device, stream))


class DeviceScene:
    """A scene uploaded once to one device (tray_scene_upload); render many times,
    from any thread and on any streams: each render runs in a launch context of
    its own (work queue, sample buffer, candidate records; include/tray.h)."""

    def __init__(self, spheres, background: Background, device: int = 0, lib_path: str | None = None):
        self.L = lib(lib_path)
        s = spheres_array(spheres)
        h = ctypes.c_void_p()
        rc = self.L.tray_scene_upload(s.ctypes.data if len(s) else None, len(s), ctypes.byref(background), device,
                                      ctypes.byref(h))
        if rc != TRAY_OK:
            raise TrayError(rc, self.L.tray_last_error().decode())
        self.handle = h
        self.device = device
        self.n = len(s)

    def render_async(self, camera: CameraState, params: Params, out_ptr: int, segments_ptr: int | None = None,
                     stream: int | None = None) -> None:
        rc = self.L.tray_render_async(self.handle, ctypes.byref(camera), ctypes.byref(params), out_ptr, segments_ptr,
                                      stream)
        if rc != TRAY_OK:
            raise TrayError(rc, self.L.tray_last_error().decode())

    def render_passes_async(self, camera: CameraState, params: Params, n_passes: int, out_ptr: int,
                            stream: int | None = None) -> None:
        """Progressive passes params.pass_ .. + n_passes - 1 in one persistent launch;
        frame k at out_ptr + k * rows * width * bytes-per-pixel."""
        rc = self.L.tray_render_passes_async(self.handle, ctypes.byref(camera), ctypes.byref(params), int(n_passes),
                                             out_ptr, stream)
        if rc != TRAY_OK:
            raise TrayError(rc, self.L.tray_last_error().decode())

    def render_stats_async(self, camera: CameraState, params: Params, out_ptr: int, stats_ptr: int,
                           stream: int | None = None) -> None:
        """Instrumented render (f32 output); stats_ptr -> 3 x uint64: segments, sphere tests, box tests."""
        rc = self.L.tray_render_stats_async(self.handle, ctypes.byref(camera), ctypes.byref(params), out_ptr,
                                            stats_ptr, stream)
        if rc != TRAY_OK:
            raise TrayError(rc, self.L.tray_last_error().decode())

    def hit_async(self, rays_ptr: int, n: int, hits_ptr: int, t_end: float = float("inf"), flags: int = 0,
                  stream: int | None = None) -> None:
        """tray_scene_hit_async: Scene.Hit(r, Interval{1e-6, t_end}) for n device rays -> n x tray_hit."""
        rc = self.L.tray_scene_hit_async(self.handle, rays_ptr, int(n), float(t_end), int(flags), hits_ptr, stream)
        if rc != TRAY_OK:
            raise TrayError(rc, self.L.tray_last_error().decode())

    def ray_color_async(self, rays_ptr: int, n: int, max_depth: int, seed: int, rgb_ptr: int,
                        ids_ptr: int | None = None, segments_ptr: int | None = None, flags: int = 0,
                        stream: int | None = None) -> None:
        """tray_ray_color_async: Scene.RayColor(r, max_depth) for n device rays -> n x 3 f64
        (+ n x uint32 Scene.Hit counts); ids: the (pixel, sample word) pair of each ray's draws."""
        rc = self.L.tray_ray_color_async(self.handle, rays_ptr, ids_ptr, int(n), int(max_depth),
                                         int(seed) & (2**64 - 1), int(flags), rgb_ptr, segments_ptr, stream)
        if rc != TRAY_OK:
            raise TrayError(rc, self.L.tray_last_error().decode())

    def scatter_async(self, rays_ptr: int, hits_ptr: int, n: int, seed: int, out_ptr: int,
                      ids_ptr: int | None = None, bounce: int = 0, stream: int | None = None) -> None:
        """tray_scatter_async: hits[i].Mat.Scatter(rays[i], hits[i]) for n device (ray, record) pairs
        -> n x tray_scatter; ids: the (pixel, sample word) pair of each ray's draws at `bounce`."""
        rc = self.L.tray_scatter_async(self.handle, rays_ptr, hits_ptr, ids_ptr, int(n), int(bounce),
                                       int(seed) & (2**64 - 1), out_ptr, stream)
        if rc != TRAY_OK:
            raise TrayError(rc, self.L.tray_last_error().decode())

    def occluded_async(self, rays_ptr: int, n: int, out_ptr: int, t_end: float = float("inf"),
                       t_ends_ptr: int | None = None, flags: int = 0, stream: int | None = None) -> None:
        """tray_scene_occluded_async: one byte per device ray, 1 iff a root lies in (1e-6, end);
        end = t_ends_ptr[i] (n x f64) when given, else t_end."""
        rc = self.L.tray_scene_occluded_async(self.handle, rays_ptr, t_ends_ptr, int(n), float(t_end), int(flags),
                                              out_ptr, stream)
        if rc != TRAY_OK:
            raise TrayError(rc, self.L.tray_last_error().decode())

    def render_aov_async(self, camera: CameraState, params: Params, albedo_ptr: int | None = None,
                         normal_ptr: int | None = None, depth_ptr: int | None = None,
                         coverage_ptr: int | None = None, index_ptr: int | None = None,
                         stream: int | None = None) -> None:
        """tray_render_aov_async: the first-hit feature buffers of params' row set into device
        buffers (rows x width x 3 f64, x 3 f64, f64, f64, i32); a None buffer is not written."""
        out = AovBuffers(albedo_ptr, normal_ptr, depth_ptr, coverage_ptr, index_ptr)
        rc = self.L.tray_render_aov_async(self.handle, ctypes.byref(camera), ctypes.byref(params), ctypes.byref(out),
                                          stream)
        if rc != TRAY_OK:
            raise TrayError(rc, self.L.tray_last_error().decode())

    def render_pixels_async(self, camera: CameraState, params: Params, pixels_ptr: int | None, n_pixels: int,
                            out_ptr: int | None, n_passes: int = 1, pass_plane_ptr: int | None = None,
                            segments_ptr: int | None = None, stream: int | None = None) -> None:
        """tray_render_pixels_async: the ordered-sum means of n_pixels listed compact pixels (u32) of
        params' row set, passes params.pass_ + plane[pixel] + k for k < n_passes, into out
        (n_passes x n_pixels x 3 f64; segments: n_passes x n_pixels u32)."""
        rc = self.L.tray_render_pixels_async(self.handle, ctypes.byref(camera), ctypes.byref(params), pixels_ptr,
                                             int(n_pixels), pass_plane_ptr, int(n_passes), out_ptr, segments_ptr,
                                             stream)
        if rc != TRAY_OK:
            raise TrayError(rc, self.L.tray_last_error().decode())

    def plan(self, camera: CameraState, params: Params, n_passes: int = 1) -> RenderPlan:
        """tray_render_plan_get: how render_async / render_passes_async would run."""
        out = RenderPlan()
        rc = self.L.tray_render_plan_get(self.handle, ctypes.byref(camera), ctypes.byref(params), int(n_passes),
                                         ctypes.byref(out))
        if rc != TRAY_OK:
            raise TrayError(rc, self.L.tray_last_error().decode())
        return out

    def info(self) -> SceneInfo:
        out = SceneInfo()
        rc = self.L.tray_scene_get_info(self.handle, ctypes.byref(out))
        if rc != TRAY_OK:
            raise TrayError(rc, self.L.tray_last_error().decode())
        return out

    def update_async(self, geometry_ptr: int, n: int, record_ptr: int, stream: int | None = None) -> None:
        """tray_scene_update_async: new centres and radii, n x {cx, cy, cz, radius} f64 on the device, and
        the BVH refitted to them, enqueued on `stream`; record_ptr -> a 32-byte tray_scene_update_record
        (SCENE_UPDATE_RECORD_DTYPE) on the device, whose `applied` is 0 when the update was refused."""
        rc = self.L.tray_scene_update_async(self.handle, geometry_ptr, int(n), record_ptr, stream)
        if rc != TRAY_OK:
            raise TrayError(rc, self.L.tray_last_error().decode())

    def update(self, geometry) -> SceneUpdateRecord:
        """tray_scene_update: the same from a host (n, 4) array {cx, cy, cz, radius}, synchronous."""
        g = np.ascontiguousarray(geometry, dtype=np.float64)
        if g.ndim != 2 or g.shape[1] != 4:
            raise ValueError("geometry must be (n, 4): cx, cy, cz, radius")
        rec = SceneUpdateRecord()
        rc = self.L.tray_scene_update(self.handle, g.ctypes.data if len(g) else None, len(g), ctypes.byref(rec))
        if rc != TRAY_OK:
            raise TrayError(rc, self.L.tray_last_error().decode())
        return rec

    def nodes(self) -> np.ndarray:
        """tray_debug_scene_nodes: the scene's BVH nodes as they are on the device, a NODE_DTYPE
        array (empty without a tree). Waits for the scene's enqueued renders and updates."""
        size = ctypes.c_size_t(0)
        rc = self.L.tray_debug_scene_nodes(self.handle, None, 0, ctypes.byref(size))
        if rc != TRAY_OK:
            raise TrayError(rc, self.L.tray_last_error().decode())
        out = np.zeros(size.value // NODE_DTYPE.itemsize, dtype=NODE_DTYPE)
        if size.value:
            rc = self.L.tray_debug_scene_nodes(self.handle, out.ctypes.data, out.nbytes, ctypes.byref(size))
            if rc != TRAY_OK:
                raise TrayError(rc, self.L.tray_last_error().decode())
        return out

    def leaves(self):
        """tray_debug_scene_leaves: (leaves, slots), int32 arrays: per leaf (first slot << 3) | count,
        per slot of the tree the list index of its sphere. Both empty without a tree."""
        nl, ns = ctypes.c_int32(0), ctypes.c_int32(0)
        rc = self.L.tray_debug_scene_leaves(self.handle, None, 0, None, 0, ctypes.byref(nl), ctypes.byref(ns))
        if rc != TRAY_OK:
            raise TrayError(rc, self.L.tray_last_error().decode())
        leaves, slots = np.zeros(nl.value, dtype=np.int32), np.zeros(ns.value, dtype=np.int32)
        rc = self.L.tray_debug_scene_leaves(self.handle, leaves.ctypes.data, len(leaves), slots.ctypes.data, len(slots),
                                            ctypes.byref(nl), ctypes.byref(ns))
        if rc != TRAY_OK:
            raise TrayError(rc, self.L.tray_last_error().decode())
        return leaves, slots

    def release(self) -> None:
        if self.handle:
            self.L.tray_scene_release(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass
