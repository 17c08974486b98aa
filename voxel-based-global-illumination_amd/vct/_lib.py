"""ctypes binding of include/vct.h (the C-ABI of the HIP path).

This module only loads the in-tree ``libvct_hip.so`` built by
``voxel-based-global-illumination_amd/Makefile``.  There is deliberately no
CPU fallback: if the library (or a HIP device) is missing, calls fail loudly.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VCT_LIB") or os.path.join(_HERE, "libvct_hip.so")

# every symbol include/vct.h declares (checked by tests/test_abi.py)
EXPORTS = (
    "vct_create", "vct_destroy", "vct_last_error", "vct_status_string", "vct_abi_version",
    "vct_get_config", "vct_set_stream", "vct_synchronize", "vct_create_multi", "vct_num_devices", "vct_trace_form", "vct_voxelize", "vct_voxelize_device",
    "vct_set_textures", "vct_voxelize_textured", "vct_voxelize_textured_device",
    "vct_inject_directional", "vct_build_mips", "vct_trace", "vct_trace_device",
    "vct_tiles_for_rank", "vct_untile_device", "vct_untile_planes_device", "vct_untile_planes_packed_device",
    "vct_tile_offset", "vct_comm_get_id", "vct_comm_init", "vct_comm_rank", "vct_comm_broadcast_level0",
    "vct_comm_trace_frame", "vct_comm_destroy", "vct_comm_set_timeout", "vct_comm_synchronize",
    "vct_comm_frame_layout", "vct_gbuffer_raycast_device", "vct_gbuffer_raster_device",
    "vct_composite_device",
    "vct_num_levels", "vct_level_dims", "vct_download_level", "vct_upload_level0",
    "vct_level0_device", "vct_copy_level0_to_device", "vct_set_level0_from_device",
    "vct_download_voxels", "vct_download_accum", "vct_device_alloc", "vct_device_free", "vct_memcpy",
    "vct_save_grid", "vct_load_grid", "vct_dump_info",
)

# include/vct_bounce.h: the additive part of the boundary that only the HIP library
# implements.  Bound on first use (bind_extension), so that a library without these
# symbols -- the CPU oracle backend -- still loads and binds.
EXTENSIONS = ("vct_inject_bounces", "vct_bounce_sources")

# include/vct_lights.h: point and spot lights, likewise HIP only (bind_light_extension)
LIGHT_EXTENSIONS = ("vct_inject_lights", "vct_composite_lights_device")
VCT_LIGHT_DIRECTIONAL, VCT_LIGHT_POINT, VCT_LIGHT_SPOT = 0, 1, 2
VCT_MAX_LIGHTS = 64

# include/vct_shadow.h: cone-traced soft shadows, likewise HIP only (bind_shadow_extension)
SHADOW_EXTENSIONS = ("vct_shadow_cones_device", "vct_composite_shadowed_device")

# include/vct_emission.h: emissive surfaces, likewise HIP only (bind_emission_extension)
EMISSION_EXTENSIONS = ("vct_voxelize_emission", "vct_voxelize_emission_device", "vct_emission_voxels",
                       "vct_download_emission", "vct_inject_emission", "vct_composite_emissive_device")
VCT_EMISSION_SCALE_LIMIT = 2.0 ** 111

# include/vct_sky.h: sky light, likewise HIP only (bind_sky_extension)
SKY_EXTENSIONS = ("vct_sky_cones_device", "vct_inject_sky")

# include/vct_dynamic.h: the dynamic layer, likewise HIP only (bind_dynamic_extension)
DYNAMIC_EXTENSIONS = ("vct_voxelize_dynamic", "vct_voxelize_dynamic_device", "vct_dynamic_voxels")

# include/vct_objects.h: dynamic objects, likewise HIP only (bind_objects_extension)
OBJECTS_EXTENSIONS = ("vct_objects_define", "vct_objects_update", "vct_objects_update_device", "vct_objects_get_stats")
VCT_MAX_OBJECTS = 4096

# include/vct_mixed.h: the mixed-resolution trace, likewise HIP only (bind_mixed_extension)
MIXED_EXTENSIONS = ("vct_mixed_default_params", "vct_trace_cones_device", "vct_mixed_pick_device",
                    "vct_mixed_upsample_device", "vct_mixed_scatter_device", "vct_trace_mixed_device")
VCT_CONES_DIFFUSE, VCT_CONES_SPECULAR = 1, 2
VCT_MIXED_NORMAL_COS = 0.9
VCT_MIXED_HOLE_WIDTH = 64
VCT_MIXED_NO_SOURCE = 0xFFFFFFFF

# include/vct_fog.h: volumetric fog, likewise HIP only (bind_fog_extension)
FOG_EXTENSIONS = ("vct_build_fog", "vct_fog_dims", "vct_download_fog", "vct_fog_rays_device", "vct_fog_march_device",
                  "vct_fog_apply_device")
VCT_FOG_DENSITY_LIMIT = 2.0 ** 20
VCT_FOG_DEFAULT_ALBEDO, VCT_FOG_DEFAULT_LEVEL, VCT_FOG_DEFAULT_STEP, VCT_FOG_DEFAULT_TAN = 0.9, 2, 1.0, 0.1

# include/vct_temporal.h: temporal accumulation, likewise HIP only (bind_temporal_extension)
TEMPORAL_EXTENSIONS = ("vct_temporal_default_params", "vct_temporal_accumulate_device")
VCT_TEMPORAL_DEFAULT_LEN, VCT_TEMPORAL_MAX_LEN = 8, 1024

# include/vct_sky_view.h: the sky in view, likewise HIP only (bind_sky_view_extension)
SKY_VIEW_EXTENSIONS = ("vct_sky_specular_device", "vct_sky_background_device")

# include/vct_query.h: cone queries and the probe grid, likewise HIP only (bind_query_extension)
QUERY_EXTENSIONS = ("vct_cone_query_device", "vct_probe_build_device", "vct_probe_sample_device")
VCT_QUERY_MAX_STEPS, VCT_PROBE_MAX_DIM = 4096, 256

# include/vct_voxview.h: the voxel view and ray picking, likewise HIP only (bind_voxview_extension)
VOXVIEW_EXTENSIONS = ("vct_voxel_pick_device", "vct_voxel_view_device")
VCT_VOXPICK_OCCUPANCY, VCT_VOXPICK_ALPHA = 0, 1
VCT_VOXVIEW_RADIANCE, VCT_VOXVIEW_ALPHA, VCT_VOXVIEW_ALBEDO, VCT_VOXVIEW_NORMAL = 0, 1, 2, 3
VCT_VOXVIEW_MODES = {"radiance": 0, "alpha": 1, "albedo": 2, "normal": 3}
VCT_VOXHIT_FACE_INSIDE, VCT_VOXHIT_FACE_MISS, VCT_VOXHIT_CELL_MISS = 6, 7, 0xFFFFFFFF
VCT_VOXVIEW_SHADE = (0.8, 1.0, 0.6)          # VCT_VOXVIEW_SHADE_X / _Y / _Z (include/vct_spec.h)
VCT_VOXVIEW_STEPS_PER_CELL = 3

# include/vct_env.h: the environment-map sky, likewise HIP only (bind_env_extension)
ENV_EXTENSIONS = ("vct_set_env", "vct_env_size", "vct_env_download_level", "vct_env_lookup_device",
                  "vct_env_cones_device", "vct_inject_env", "vct_env_specular_device", "vct_env_background_device")
VCT_ENV_MAX_DIM = 2048
VCT_ENV_TEXEL_LIMIT = 2.0 ** 52

# include/vct_shading.h: the shading G-buffer, likewise HIP only (bind_shading_extension)
SHADING_EXTENSIONS = ("vct_set_shading", "vct_gbuffer_shaded_device", "vct_specular_tint_device")
VCT_SHADING_NO_ATTR = 0xFFFFFFFF
VCT_SHADING_FLIP_GREEN = 1

# include/vct_cutout.h: alpha-cutout materials, likewise HIP only (bind_cutout_extension)
CUTOUT_EXTENSIONS = ("vct_voxelize_cutout", "vct_voxelize_cutout_device", "vct_gbuffer_cutout_device",
                     "vct_cutout_materials")

# include/vct_motion.h: object motion, likewise HIP only (bind_motion_extension)
MOTION_EXTENSIONS = ("vct_objects_poses_device", "vct_objects_motion_device")

# include/vct_present.h: the HDR present, likewise HIP only (bind_present_extension)
PRESENT_EXTENSIONS = ("vct_luminance_meter_device", "vct_exposure_update_device", "vct_bloom_scratch_bytes",
                      "vct_bloom_device", "vct_present_device")
VCT_PRESENT_BINS, VCT_PRESENT_KEY0, VCT_PRESENT_MAX_DIM, VCT_BLOOM_MAX_LEVELS = 512, (127 - 16) << 4, 16384, 8
VCT_CURVE_REINHARD, VCT_CURVE_REINHARD_WHITE, VCT_CURVE_ACES, VCT_CURVE_CLAMP = 0, 1, 2, 3
VCT_CURVES = {"reinhard": 0, "white": 1, "aces": 2, "clamp": 3}
VCT_TRANSFER_GAMMA22, VCT_TRANSFER_SRGB = 0, 1
VCT_EXPOSURE_LIMIT = 2.0 ** 64

STATUS = {0: "VCT_OK", 1: "VCT_EINVAL", 2: "VCT_ENOMEM", 3: "VCT_EDEVICE", 4: "VCT_ECOMM", 5: "VCT_ESTATE"}


class VctConfig(C.Structure):
    _fields_ = [
        ("n", C.c_uint32),
        ("aabb_min", C.c_float * 3),
        ("extent", C.c_float),
        ("aniso", C.c_uint32),
        ("n_diffuse", C.c_uint32),
        ("specular", C.c_uint32),
        ("device", C.c_int32),
    ]


class VctCamera(C.Structure):
    _fields_ = [
        ("position", C.c_float * 3),
        ("front", C.c_float * 3),
        ("up", C.c_float * 3),
        ("right", C.c_float * 3),
        ("zoom_deg", C.c_float),
        ("near_plane", C.c_float),
        ("far_plane", C.c_float),
    ]


class VctTexture(C.Structure):
    _fields_ = [("rgba8", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32)]


class VctLight(C.Structure):          # vct_light, 60 bytes
    _fields_ = [
        ("type", C.c_uint32),
        ("position", C.c_float * 3),
        ("direction", C.c_float * 3),
        ("color", C.c_float * 3),
        ("range", C.c_float),
        ("cos_inner", C.c_float),
        ("cos_outer", C.c_float),
        ("reserved", C.c_uint32 * 2),
    ]


class VctSky(C.Structure):            # vct_sky, 48 bytes
    _fields_ = [
        ("up", C.c_float * 3),
        ("zenith", C.c_float * 3),
        ("horizon", C.c_float * 3),
        ("ground", C.c_float * 3),
    ]


class VctEnvSky(C.Structure):         # vct_env_sky, 40 bytes
    _fields_ = [
        ("frame", (C.c_float * 3) * 3),
        ("scale", C.c_float),
    ]


class VctFog(C.Structure):            # vct_fog, 28 bytes
    _fields_ = [
        ("density", C.c_float),
        ("albedo", C.c_float * 3),
        ("ambient", C.c_float),
        ("level", C.c_uint32),
        ("step", C.c_float),
    ]


def check_fog(density, albedo, ambient, level, step, n, extent):
    """The input rule of include/vct_fog.h (vct_spec.h "volumetric fog") for a grid of n^3
    voxels and edge `extent`, in float32 as the library tests it: None, or what is wrong.
    The binding and the tests share it; the library applies the same rule itself."""
    import numpy as np
    F = np.float32
    with np.errstate(all="ignore"):
        d = F(density)
        if not np.isfinite(d) or np.signbit(d):
            return "density must be finite with a clear sign bit"
        if d > F(VCT_FOG_DENSITY_LIMIT):
            return "density above VCT_FOG_DENSITY_LIMIT"
        if len(albedo) != 3:
            return "albedo must have three components"
        for a in albedo:
            a = F(a)
            if not np.isfinite(a) or np.signbit(a) or a > F(1.0):
                return "albedo must be finite and in [0, 1] (-0.0f is refused)"
        am = F(ambient)
        if not np.isfinite(am) or not am >= F(0.0):
            return "ambient must be finite and >= 0"
        if int(level) != level or not 1 <= int(level) <= 31 or (int(n) >> int(level)) < 4:
            return "level must satisfy 1 <= level and (n >> level) >= 4"
        st = F(step)
        if not (st >= F(0.25) and st <= F(4.0)):
            return "step must be in [0.25, 4]"
        if not np.isfinite((d * F(extent)) / F(n)):
            return "density * extent overflows"
    return None


class VctMixedParams(C.Structure):    # vct_mixed_params, 16 bytes
    _fields_ = [
        ("normal_cos", C.c_float),
        ("plane_eps", C.c_float),
        ("max_holes", C.c_uint32),
        ("factor", C.c_uint32),
    ]


class VctMixedHoles(C.Structure):     # vct_mixed_holes
    _fields_ = [
        ("pos4", C.c_void_p),
        ("nrm4", C.c_void_p),
        ("alb4", C.c_void_p),
        ("px", C.c_void_p),
        ("count", C.c_void_p),
        ("stats", C.c_void_p),
        ("max_holes", C.c_uint32),
    ]


class VctTemporalParams(C.Structure):    # vct_temporal_params, 12 bytes
    _fields_ = [
        ("normal_cos", C.c_float),
        ("plane_eps", C.c_float),
        ("max_len", C.c_uint32),
    ]


class VctTemporalArgs(C.Structure):      # vct_temporal_args
    _fields_ = [
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("pos4", C.c_void_p),
        ("nrm4", C.c_void_p),
        ("motion4", C.c_void_p),
        ("prev_cam", C.POINTER(VctCamera)),
        ("prev_pos4", C.c_void_p),
        ("prev_nrm4", C.c_void_p),
        ("n_planes", C.c_uint32),
        ("cur4", C.c_void_p * 4),
        ("hist4", C.c_void_p * 4),
        ("out4", C.c_void_p * 4),
        ("hist_len", C.c_void_p),
        ("out_len", C.c_void_p),
        ("stats", C.c_void_p),
    ]


class VctCone(C.Structure):              # vct_cone, 48 bytes
    _fields_ = [
        ("p", C.c_float * 3),
        ("tau", C.c_float),
        ("d", C.c_float * 3),
        ("t_lim", C.c_float),
        ("off", C.c_float * 3),
        ("valid", C.c_float),
    ]


class VctConeQueryArgs(C.Structure):     # vct_cone_query_args
    _fields_ = [
        ("cones", C.c_void_p),
        ("count", C.c_uint32),
        ("out4", C.c_void_p),
        ("steps", C.c_void_p),
        ("cone_steps", C.c_void_p),
    ]


class VctProbeGrid(C.Structure):         # vct_probe_grid, 28 bytes
    _fields_ = [
        ("origin", C.c_float * 3),
        ("spacing", C.c_float),
        ("dims", C.c_uint32 * 3),
    ]


class VctVoxelPickArgs(C.Structure):    # vct_voxel_pick_args
    _fields_ = [
        ("org4", C.c_void_p),
        ("dir4", C.c_void_p),
        ("count", C.c_uint32),
        ("level", C.c_uint32),
        ("solid", C.c_uint32),
        ("hit4", C.c_void_p),
        ("cells", C.c_void_p),
    ]


class VctVoxelViewArgs(C.Structure):    # vct_voxel_view_args
    _fields_ = [
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("level", C.c_uint32),
        ("mode", C.c_uint32),
        ("shade", C.c_uint32),
        ("linear4", C.c_void_p),
        ("rgba8", C.c_void_p),
        ("hit4", C.c_void_p),
        ("cells", C.c_void_p),
    ]


class VctShadingMaterial(C.Structure):  # vct_shading_material, 32 bytes
    _fields_ = [
        ("ks", C.c_float * 3),
        ("roughness", C.c_float),
        ("normal_map", C.c_int32),
        ("specular_map", C.c_int32),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class VctShadingDesc(C.Structure):      # vct_shading_desc
    _fields_ = [
        ("verts", C.c_void_p),
        ("vertex_stride", C.c_uint32),
        ("n_verts", C.c_uint32),
        ("idx", C.c_void_p),
        ("n_idx", C.c_uint32),
        ("tri_material", C.c_void_p),
        ("normal_offset", C.c_uint32),
        ("uv_offset", C.c_uint32),
        ("tangent_offset", C.c_uint32),
        ("bitangent_offset", C.c_uint32),
        ("materials", C.c_void_p),
        ("n_materials", C.c_uint32),
    ]


class VctCutout(C.Structure):           # vct_cutout, 16 bytes
    _fields_ = [
        ("map", C.c_int32),
        ("channel", C.c_uint32),
        ("cutoff", C.c_float),
        ("reserved", C.c_uint32),
    ]


class VctExposureState(C.Structure):   # vct_exposure_state, 16 bytes (a device record)
    _fields_ = [
        ("exposure", C.c_float),
        ("target", C.c_float),
        ("mean_luminance", C.c_float),
        ("counted", C.c_uint32),
    ]


class VctExposureParams(C.Structure):  # vct_exposure_params, 32 bytes
    _fields_ = [
        ("key_value", C.c_float),
        ("min_exposure", C.c_float),
        ("max_exposure", C.c_float),
        ("low_permille", C.c_uint32),
        ("high_permille", C.c_uint32),
        ("rate_up", C.c_float),
        ("rate_down", C.c_float),
        ("reserved", C.c_uint32),
    ]


class VctBloomParams(C.Structure):     # vct_bloom_params, 16 bytes
    _fields_ = [
        ("threshold", C.c_float),
        ("levels", C.c_uint32),
        ("exposure", C.c_float),
        ("reserved", C.c_uint32),
    ]


class VctPresentParams(C.Structure):   # vct_present_params, 32 bytes
    _fields_ = [
        ("curve", C.c_uint32),
        ("transfer", C.c_uint32),
        ("dither", C.c_uint32),
        ("exposure", C.c_float),
        ("white", C.c_float),
        ("bloom_intensity", C.c_float),
        ("reserved", C.c_uint32 * 2),
    ]


class VctCommId(C.Structure):
    _fields_ = [("internal", C.c_char * 128)]


VCT_ALL_RANKS = -1


class VctCommLayout(C.Structure):
    _fields_ = [("buffer_tiles", C.c_uint64), ("diffuse_tile", C.c_uint64), ("spec_tile", C.c_uint64),
                ("tiles", C.c_uint32), ("exchange_tiles", C.c_uint32)]


class VctTraceArgs(C.Structure):
    _fields_ = [
        ("pos4", C.c_void_p),
        ("nrm4", C.c_void_p),
        ("alb4", C.c_void_p),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("eye", C.c_float * 3),
        ("diffuse4", C.c_void_p),
        ("spec4", C.c_void_p),
        ("steps_px", C.c_void_p),
        ("cone_steps", C.c_void_p),
        ("texel_fetches", C.c_void_p),
        ("tile_rank", C.c_uint32),
        ("tile_world", C.c_uint32),
        ("tile_compact", C.c_uint32),
        ("variant", C.c_uint32),
    ]


_lib = None


def load() -> C.CDLL:
    """Load libvct_hip.so once; raises FileNotFoundError if it was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(
            f"{LIB_PATH} is missing: build it with `make -C voxel-based-global-illumination_amd` "
            "(the VCT path has no CPU fallback)")
    _lib = bind(C.CDLL(LIB_PATH))
    return _lib


def bind(lib: C.CDLL) -> C.CDLL:
    """Declare the include/vct.h signatures on a loaded implementation of the
    header (the HIP library; tests also bind the CPU oracle backend,
    oracle/_build/libvct_cpu.so, explicitly -- the product never does)."""
    P = C.c_void_p
    u32, i32, f32 = C.c_uint32, C.c_int32, C.c_float
    sig = {
        "vct_create": (i32, [C.POINTER(VctConfig), C.POINTER(P)]),
        "vct_destroy": (None, [P]),
        "vct_last_error": (C.c_char_p, [P]),
        "vct_status_string": (C.c_char_p, [i32]),
        "vct_abi_version": (u32, []),
        "vct_get_config": (i32, [P, C.POINTER(VctConfig)]),
        "vct_set_stream": (i32, [P, P]),
        "vct_synchronize": (i32, [P]),
        "vct_create_multi": (i32, [C.POINTER(VctConfig), u32, C.POINTER(P)]),
        "vct_num_devices": (u32, [P]),
        "vct_trace_form": (C.c_int32, [P]),
        "vct_voxelize": (i32, [P, P, u32, u32, P, u32, P, P, u32]),
        "vct_voxelize_device": (i32, [P, P, u32, u32, P, u32, P, P, u32]),
        "vct_set_textures": (i32, [P, P, u32]),
        "vct_voxelize_textured": (i32, [P, P, u32, u32, P, u32, P, P, P, u32, u32]),
        "vct_voxelize_textured_device": (i32, [P, P, u32, u32, P, u32, P, P, P, u32, u32]),
        "vct_inject_directional": (i32, [P, C.POINTER(f32), C.POINTER(f32)]),
        "vct_build_mips": (i32, [P]),
        "vct_trace": (i32, [P, P, P, P, u32, u32, C.POINTER(f32), P, P, P, P]),
        "vct_trace_device": (i32, [P, C.POINTER(VctTraceArgs)]),
        "vct_tiles_for_rank": (u32, [u32, u32, u32, u32]),
        "vct_untile_device": (i32, [P, P, u32, u32, u32, P]),
        "vct_untile_planes_device": (i32, [P, P, u32, u32, u32, u32, P]),
        "vct_untile_planes_packed_device": (i32, [P, P, u32, u32, u32, u32, P]),
        "vct_tile_offset": (u32, [u32, u32, u32, u32]),
        "vct_comm_get_id": (i32, [P]),
        "vct_comm_init": (i32, [P, P, u32, u32]),
        "vct_comm_rank": (i32, [P, C.POINTER(u32), C.POINTER(u32)]),
        "vct_comm_broadcast_level0": (i32, [P, u32]),
        "vct_comm_trace_frame": (i32, [P, C.POINTER(VctTraceArgs), i32]),
        "vct_comm_destroy": (i32, [P]),
        "vct_comm_set_timeout": (i32, [P, u32]),
        "vct_comm_synchronize": (i32, [P]),
        "vct_comm_frame_layout": (i32, [u32, u32, u32, u32, i32, C.POINTER(VctCommLayout)]),
        "vct_gbuffer_raycast_device": (i32, [P, C.POINTER(VctCamera), u32, u32, f32, P, P, P]),
        "vct_gbuffer_raster_device": (i32, [P, C.POINTER(VctCamera), u32, u32, f32, P, P, P]),
        "vct_composite_device": (i32, [P, P, P, P, P, P, u32, u32, C.POINTER(f32), C.POINTER(f32), P, P]),
        "vct_num_levels": (u32, [P]),
        "vct_level_dims": (i32, [P, u32, C.POINTER(u32), C.POINTER(u32)]),
        "vct_download_level": (i32, [P, u32, u32, P]),
        "vct_upload_level0": (i32, [P, P]),
        "vct_level0_device": (i32, [P, C.POINTER(P), C.POINTER(C.c_size_t)]),
        "vct_copy_level0_to_device": (i32, [P, P]),
        "vct_set_level0_from_device": (i32, [P, P]),
        "vct_download_voxels": (i32, [P, P, P]),
        "vct_download_accum": (i32, [P, P, P]),
        "vct_device_alloc": (i32, [P, C.c_size_t, C.POINTER(P)]),
        "vct_device_free": (i32, [P, P]),
        "vct_memcpy": (i32, [P, P, P, C.c_size_t, C.c_int]),
        "vct_save_grid": (i32, [P, C.c_char_p, u32]),
        "vct_load_grid": (i32, [P, C.c_char_p]),
        "vct_dump_info": (i32, [C.c_char_p, C.POINTER(VctConfig), C.POINTER(u32)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


def bind_extension(lib: C.CDLL, name: str):
    """The include/vct_bounce.h function `name` of `lib`, with its signature declared;
    AttributeError (naming the library) if this implementation does not export it."""
    P, u32, i32 = C.c_void_p, C.c_uint32, C.c_int32
    sig = {
        "vct_inject_bounces": (i32, [P, u32]),
        "vct_bounce_sources": (i32, [P, C.POINTER(u32)]),
    }
    res, args = sig[name]
    try:
        fn = getattr(lib, name)
    except AttributeError:
        raise AttributeError(f"{getattr(lib, '_name', lib)} does not export {name} "
                             "(include/vct_bounce.h is implemented by the HIP library only)") from None
    fn.restype = res
    fn.argtypes = args
    return fn


def bind_light_extension(lib: C.CDLL, name: str):
    """The include/vct_lights.h function `name` of `lib`, with its signature declared;
    AttributeError (naming the library) if this implementation does not export it."""
    P, u32, i32 = C.c_void_p, C.c_uint32, C.c_int32
    sig = {
        "vct_inject_lights": (i32, [P, C.POINTER(VctLight), u32]),
        "vct_composite_lights_device": (i32, [P, P, P, P, P, P, u32, u32, C.POINTER(VctLight), u32, P, P]),
    }
    res, args = sig[name]
    try:
        fn = getattr(lib, name)
    except AttributeError:
        raise AttributeError(f"{getattr(lib, '_name', lib)} does not export {name} "
                             "(include/vct_lights.h is implemented by the HIP library only)") from None
    fn.restype = res
    fn.argtypes = args
    return fn


def bind_shadow_extension(lib: C.CDLL, name: str):
    """The include/vct_shadow.h function `name` of `lib`, with its signature declared;
    AttributeError (naming the library) if this implementation does not export it."""
    P, u32, i32 = C.c_void_p, C.c_uint32, C.c_int32
    sig = {
        "vct_shadow_cones_device": (i32, [P, P, P, u32, u32, C.POINTER(VctLight), u32, C.POINTER(C.c_float), P, P]),
        "vct_composite_shadowed_device": (i32, [P, P, P, P, P, P, u32, u32, C.POINTER(VctLight), u32, P, P, P]),
    }
    res, args = sig[name]
    try:
        fn = getattr(lib, name)
    except AttributeError:
        raise AttributeError(f"{getattr(lib, '_name', lib)} does not export {name} "
                             "(include/vct_shadow.h is implemented by the HIP library only)") from None
    fn.restype = res
    fn.argtypes = args
    return fn


def bind_emission_extension(lib: C.CDLL, name: str):
    """The include/vct_emission.h function `name` of `lib`, with its signature declared;
    AttributeError (naming the library) if this implementation does not export it."""
    P, u32, i32, f32 = C.c_void_p, C.c_uint32, C.c_int32, C.c_float
    sig = {
        "vct_voxelize_emission": (i32, [P, P, u32, u32, P, u32, P, P, u32]),
        "vct_voxelize_emission_device": (i32, [P, P, u32, u32, P, u32, P, P, u32]),
        "vct_emission_voxels": (i32, [P, C.POINTER(u32)]),
        "vct_download_emission": (i32, [P, P]),
        "vct_inject_emission": (i32, [P, f32]),
        "vct_composite_emissive_device": (i32, [P, P, P, P, P, P, u32, u32, C.POINTER(VctLight), u32, P, f32, P, P]),
    }
    res, args = sig[name]
    try:
        fn = getattr(lib, name)
    except AttributeError:
        raise AttributeError(f"{getattr(lib, '_name', lib)} does not export {name} "
                             "(include/vct_emission.h is implemented by the HIP library only)") from None
    fn.restype = res
    fn.argtypes = args
    return fn


def bind_fog_extension(lib: C.CDLL, name: str):
    """The include/vct_fog.h function `name` of `lib`, with its signature declared;
    AttributeError (naming the library) if this implementation does not export it."""
    P, u32, i32 = C.c_void_p, C.c_uint32, C.c_int32
    F3 = C.POINTER(C.c_float)
    sig = {
        "vct_build_fog": (i32, [P, C.POINTER(VctFog), C.POINTER(VctLight), u32, F3]),
        "vct_fog_dims": (i32, [P, C.POINTER(u32)]),
        "vct_download_fog": (i32, [P, P]),
        "vct_fog_rays_device": (i32, [P, C.POINTER(VctCamera), F3, P, u32, u32, P]),
        "vct_fog_march_device": (i32, [P, C.POINTER(VctFog), F3, P, u32, u32, P, P]),
        "vct_fog_apply_device": (i32, [P, P, u32, u32, P, P]),
    }
    res, args = sig[name]
    try:
        fn = getattr(lib, name)
    except AttributeError:
        raise AttributeError(f"{getattr(lib, '_name', lib)} does not export {name} "
                             "(include/vct_fog.h is implemented by the HIP library only)") from None
    fn.restype = res
    fn.argtypes = args
    return fn


def debug_fog(lib: C.CDLL, handle=None, force64: int = -1, counters=None) -> int:
    """Test hook (vct_debug_fog, not part of the headers).  force64 >= 0, process-wide: nonzero
    sends the light cones of every fog build through the 64-bit-address path (the one 1024^3
    takes).  counters: None, or (light_steps, ambient_steps) device pointers (ints, 0: none) of
    8-byte counters the context's following builds add their light-cone and ambient K4 steps
    to.  -> the address path of the context's last build: 32, 64, 0 before any."""
    fn = lib.vct_debug_fog
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    a, b = counters if counters is not None else (0, 0)
    return int(fn(handle, int(force64), 0 if counters is None else 1, a or None, b or None))


def bind_sky_extension(lib: C.CDLL, name: str):
    """The include/vct_sky.h function `name` of `lib`, with its signature declared;
    AttributeError (naming the library) if this implementation does not export it."""
    P, u32, i32 = C.c_void_p, C.c_uint32, C.c_int32
    sig = {
        "vct_sky_cones_device": (i32, [P, P, P, u32, u32, C.POINTER(VctSky), P, P, P]),
        "vct_inject_sky": (i32, [P, C.POINTER(VctSky)]),
    }
    res, args = sig[name]
    try:
        fn = getattr(lib, name)
    except AttributeError:
        raise AttributeError(f"{getattr(lib, '_name', lib)} does not export {name} "
                             "(include/vct_sky.h is implemented by the HIP library only)") from None
    fn.restype = res
    fn.argtypes = args
    return fn


def bind_sky_view_extension(lib: C.CDLL, name: str):
    """The include/vct_sky_view.h function `name` of `lib`, with its signature declared;
    AttributeError (naming the library) if this implementation does not export it."""
    P, u32, i32 = C.c_void_p, C.c_uint32, C.c_int32
    F3 = C.POINTER(C.c_float)
    sig = {
        "vct_sky_specular_device": (i32, [P, P, P, P, u32, u32, F3, C.POINTER(VctSky), P, P, P]),
        "vct_sky_background_device": (i32, [P, C.POINTER(VctCamera), P, u32, u32, C.POINTER(VctSky), P, P]),
    }
    res, args = sig[name]
    try:
        fn = getattr(lib, name)
    except AttributeError:
        raise AttributeError(f"{getattr(lib, '_name', lib)} does not export {name} "
                             "(include/vct_sky_view.h is implemented by the HIP library only)") from None
    fn.restype = res
    fn.argtypes = args
    return fn


def bind_env_extension(lib: C.CDLL, name: str):
    """The include/vct_env.h function `name` of `lib`, with its signature declared;
    AttributeError (naming the library) if this implementation does not export it."""
    P, u32, i32 = C.c_void_p, C.c_uint32, C.c_int32
    F3, E = C.POINTER(C.c_float), C.POINTER(VctEnvSky)
    sig = {
        "vct_set_env": (i32, [P, P, u32]),
        "vct_env_size": (u32, [P]),
        "vct_env_download_level": (i32, [P, u32, P]),
        "vct_env_lookup_device": (i32, [P, E, P, u32, P]),
        "vct_env_cones_device": (i32, [P, P, P, u32, u32, E, P, P, P]),
        "vct_inject_env": (i32, [P, E]),
        "vct_env_specular_device": (i32, [P, P, P, P, u32, u32, F3, E, P, P, P]),
        "vct_env_background_device": (i32, [P, C.POINTER(VctCamera), P, u32, u32, E, P, P]),
    }
    res, args = sig[name]
    try:
        fn = getattr(lib, name)
    except AttributeError:
        raise AttributeError(f"{getattr(lib, '_name', lib)} does not export {name} "
                             "(include/vct_env.h is implemented by the HIP library only)") from None
    fn.restype = res
    fn.argtypes = args
    return fn


def bind_query_extension(lib: C.CDLL, name: str):
    """The include/vct_query.h function `name` of `lib`, with its signature declared;
    AttributeError (naming the library) if this implementation does not export it."""
    P, u32, i32 = C.c_void_p, C.c_uint32, C.c_int32
    PG = C.POINTER(VctProbeGrid)
    sig = {
        "vct_cone_query_device": (i32, [P, C.POINTER(VctConeQueryArgs)]),
        "vct_probe_build_device": (i32, [P, PG, P, P, P]),
        "vct_probe_sample_device": (i32, [P, PG, P, P, P, P, u32, P, P]),
    }
    res, args = sig[name]
    try:
        fn = getattr(lib, name)
    except AttributeError:
        raise AttributeError(f"{getattr(lib, '_name', lib)} does not export {name} "
                             "(include/vct_query.h is implemented by the HIP library only)") from None
    fn.restype = res
    fn.argtypes = args
    return fn


def bind_voxview_extension(lib: C.CDLL, name: str):
    """The include/vct_voxview.h function `name` of `lib`, with its signature declared;
    AttributeError (naming the library) if this implementation does not export it."""
    P, i32 = C.c_void_p, C.c_int32
    sig = {
        "vct_voxel_pick_device": (i32, [P, C.POINTER(VctVoxelPickArgs)]),
        "vct_voxel_view_device": (i32, [P, C.POINTER(VctCamera), C.POINTER(VctVoxelViewArgs)]),
    }
    res, args = sig[name]
    try:
        fn = getattr(lib, name)
    except AttributeError:
        raise AttributeError(f"{getattr(lib, '_name', lib)} does not export {name} "
                             "(include/vct_voxview.h is implemented by the HIP library only)") from None
    fn.restype = res
    fn.argtypes = args
    return fn


def bind_shading_extension(lib: C.CDLL, name: str):
    """The include/vct_shading.h function `name` of `lib`, with its signature declared;
    AttributeError (naming the library) if this implementation does not export it."""
    P, u32, i32, f32 = C.c_void_p, C.c_uint32, C.c_int32, C.c_float
    sig = {
        "vct_set_shading": (i32, [P, C.POINTER(VctShadingDesc)]),
        "vct_gbuffer_shaded_device": (i32, [P, C.POINTER(VctCamera), u32, u32, f32, P, P, P, P, P, P, P]),
        "vct_specular_tint_device": (i32, [P, P, P, u32, u32, P]),
    }
    res, args = sig[name]
    try:
        fn = getattr(lib, name)
    except AttributeError:
        raise AttributeError(f"{getattr(lib, '_name', lib)} does not export {name} "
                             "(include/vct_shading.h is implemented by the HIP library only)") from None
    fn.restype = res
    fn.argtypes = args
    return fn


def bind_cutout_extension(lib: C.CDLL, name: str):
    """The include/vct_cutout.h function `name` of `lib`, with its signature declared;
    AttributeError (naming the library) if this implementation does not export it."""
    P, u32, i32, f32 = C.c_void_p, C.c_uint32, C.c_int32, C.c_float
    vox = (i32, [P, P, u32, u32, P, u32, P, P, P, C.POINTER(VctCutout), u32, u32])
    sig = {
        "vct_voxelize_cutout": vox,
        "vct_voxelize_cutout_device": vox,
        "vct_gbuffer_cutout_device": (i32, [P, C.POINTER(VctCamera), u32, u32, f32, P, P, P, P, P, P, P]),
        "vct_cutout_materials": (u32, [P]),
    }
    res, args = sig[name]
    try:
        fn = getattr(lib, name)
    except AttributeError:
        raise AttributeError(f"{getattr(lib, '_name', lib)} does not export {name} "
                             "(include/vct_cutout.h is implemented by the HIP library only)") from None
    fn.restype = res
    fn.argtypes = args
    return fn


def bind_present_extension(lib: C.CDLL, name: str):
    """The include/vct_present.h function `name` of `lib`, with its signature declared;
    AttributeError (naming the library) if this implementation does not export it."""
    P, u32, i32 = C.c_void_p, C.c_uint32, C.c_int32
    sig = {
        "vct_luminance_meter_device": (i32, [P, P, u32, u32, P, P]),
        "vct_exposure_update_device": (i32, [P, P, P, C.POINTER(VctExposureParams), P, P]),
        "vct_bloom_scratch_bytes": (i32, [u32, u32, u32, C.POINTER(C.c_size_t)]),
        "vct_bloom_device": (i32, [P, P, u32, u32, C.POINTER(VctBloomParams), P, P, C.c_size_t]),
        "vct_present_device": (i32, [P, P, u32, u32, C.POINTER(VctPresentParams), P, P, P, P]),
    }
    res, args = sig[name]
    try:
        fn = getattr(lib, name)
    except AttributeError:
        raise AttributeError(f"{getattr(lib, '_name', lib)} does not export {name} "
                             "(include/vct_present.h is implemented by the HIP library only)") from None
    fn.restype = res
    fn.argtypes = args
    return fn


def debug_present(lib: C.CDLL, agg: int = -1) -> int:
    """Tool hook (vct_debug_present, not part of the headers).  agg >= 0, process-wide: 0 (the
    default) makes the luminance meter send one LDS atomic per lane, 1 folds the lanes that share
    the wave's first live key into one add.  -> the form in force."""
    fn = lib.vct_debug_present
    fn.restype = C.c_int
    fn.argtypes = [C.c_int]
    return int(fn(int(agg)))


def bind_dynamic_extension(lib: C.CDLL, name: str):
    """The include/vct_dynamic.h function `name` of `lib`, with its signature declared;
    AttributeError (naming the library) if this implementation does not export it."""
    P, u32, i32 = C.c_void_p, C.c_uint32, C.c_int32
    sig = {
        "vct_voxelize_dynamic": (i32, [P, P, u32, u32, P, u32, P, P, u32]),
        "vct_voxelize_dynamic_device": (i32, [P, P, u32, u32, P, u32, P, P, u32]),
        "vct_dynamic_voxels": (i32, [P, C.POINTER(u32)]),
    }
    res, args = sig[name]
    try:
        fn = getattr(lib, name)
    except AttributeError:
        raise AttributeError(f"{getattr(lib, '_name', lib)} does not export {name} "
                             "(include/vct_dynamic.h is implemented by the HIP library only)") from None
    fn.restype = res
    fn.argtypes = args
    return fn


class VctObjectMesh(C.Structure):     # vct_object_mesh: host arrays
    _fields_ = [
        ("verts", C.c_void_p),
        ("vertex_stride", C.c_uint32),
        ("n_verts", C.c_uint32),
        ("idx", C.c_void_p),
        ("n_idx", C.c_uint32),
        ("tri_material", C.c_void_p),
    ]


class VctObjectPose(C.Structure):     # vct_object_pose, 80 bytes
    _fields_ = [("m", C.c_float * 16), ("visible", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class VctObjectsStats(C.Structure):   # vct_objects_stats, 32 bytes
    _fields_ = [
        ("n_objects", C.c_uint32),
        ("n_triangles", C.c_uint32),
        ("n_visible", C.c_uint32),
        ("last_moved_triangles", C.c_uint32),
        ("last_candidates", C.c_uint64),
        ("last_touched_voxels", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


def bind_objects_extension(lib: C.CDLL, name: str):
    """The include/vct_objects.h function `name` of `lib`, with its signature declared;
    AttributeError (naming the library) if this implementation does not export it."""
    P, u32, i32 = C.c_void_p, C.c_uint32, C.c_int32
    sig = {
        "vct_objects_define": (i32, [P, C.POINTER(VctObjectMesh), u32, P, u32]),
        "vct_objects_update": (i32, [P, P, P, u32]),
        "vct_objects_update_device": (i32, [P, P, P, u32]),
        "vct_objects_get_stats": (i32, [P, C.POINTER(VctObjectsStats)]),
    }
    res, args = sig[name]
    try:
        fn = getattr(lib, name)
    except AttributeError:
        raise AttributeError(f"{getattr(lib, '_name', lib)} does not export {name} "
                             "(include/vct_objects.h is implemented by the HIP library only)") from None
    fn.restype = res
    fn.argtypes = args
    return fn


def bind_mixed_extension(lib: C.CDLL, name: str):
    """The include/vct_mixed.h function `name` of `lib`, with its signature declared;
    AttributeError (naming the library) if this implementation does not export it."""
    P, u32, i32 = C.c_void_p, C.c_uint32, C.c_int32
    MP, MH = C.POINTER(VctMixedParams), C.POINTER(VctMixedHoles)
    sig = {
        "vct_mixed_default_params": (i32, [P, u32, MP]),
        "vct_trace_cones_device": (i32, [P, C.POINTER(VctTraceArgs), u32]),
        "vct_mixed_pick_device": (i32, [P, P, P, P, u32, u32, C.POINTER(C.c_float * 3), u32, P, P, P, P]),
        "vct_mixed_upsample_device": (i32, [P, P, P, P, u32, u32, u32, P, P, P, P, MP, P, MH]),
        "vct_mixed_scatter_device": (i32, [P, P, MH, P]),
        "vct_trace_mixed_device": (i32, [P, C.POINTER(VctTraceArgs), MP]),
    }
    res, args = sig[name]
    try:
        fn = getattr(lib, name)
    except AttributeError:
        raise AttributeError(f"{getattr(lib, '_name', lib)} does not export {name} "
                             "(include/vct_mixed.h is implemented by the HIP library only)") from None
    fn.restype = res
    fn.argtypes = args
    return fn


def bind_temporal_extension(lib: C.CDLL, name: str):
    """The include/vct_temporal.h function `name` of `lib`, with its signature declared;
    AttributeError (naming the library) if this implementation does not export it."""
    P, i32 = C.c_void_p, C.c_int32
    TP = C.POINTER(VctTemporalParams)
    sig = {
        "vct_temporal_default_params": (i32, [P, TP]),
        "vct_temporal_accumulate_device": (i32, [P, C.POINTER(VctTemporalArgs), TP]),
    }
    res, args = sig[name]
    try:
        fn = getattr(lib, name)
    except AttributeError:
        raise AttributeError(f"{getattr(lib, '_name', lib)} does not export {name} "
                             "(include/vct_temporal.h is implemented by the HIP library only)") from None
    fn.restype = res
    fn.argtypes = args
    return fn


class VctMotionArgs(C.Structure):        # vct_motion_args
    _fields_ = [
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("pos4", C.c_void_p),
        ("nrm4", C.c_void_p),
        ("tri_id", C.c_void_p),
        ("bary2", C.c_void_p),
        ("prev_poses", C.c_void_p),
        ("n_prev", C.c_uint32),
        ("motion4", C.c_void_p),
        ("prev_nrm4", C.c_void_p),
        ("stats", C.c_void_p),
    ]


def bind_motion_extension(lib: C.CDLL, name: str):
    """The include/vct_motion.h function `name` of `lib`, with its signature declared;
    AttributeError (naming the library) if this implementation does not export it."""
    P, u32, i32 = C.c_void_p, C.c_uint32, C.c_int32
    sig = {
        "vct_objects_poses_device": (i32, [P, P, u32]),
        "vct_objects_motion_device": (i32, [P, C.POINTER(VctMotionArgs)]),
    }
    res, args = sig[name]
    try:
        fn = getattr(lib, name)
    except AttributeError:
        raise AttributeError(f"{getattr(lib, '_name', lib)} does not export {name} "
                             "(include/vct_motion.h is implemented by the HIP library only)") from None
    fn.restype = res
    fn.argtypes = args
    return fn


def debug_accum_packed(lib: C.CDLL, handle) -> bool:
    """Test hook (vct_debug_accum_packed, not part of the headers): K1's records hold two sums
    per word (the packed layout) rather than one."""
    fn = lib.vct_debug_accum_packed
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p]
    return bool(fn(handle))


def debug_sky(lib: C.CDLL, handle=None, force64: int = -1, profile: int = -1):
    """Test and tool hook (vct_debug_sky, not part of the headers).  force64 >= 0, process-wide:
    nonzero sends every grid's sky march through the 64-bit-address path (the one 1024^3
    takes).  profile >= 0: nonzero times the stages of the context's following inject_sky
    calls.  -> (march, add, K3) ms of the last timed inject_sky."""
    fn = lib.vct_debug_sky
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float)]
    ms = (C.c_float * 3)()
    fn(handle, int(force64), int(profile), ms)
    return tuple(float(v) for v in ms)


def debug_sky_path(lib: C.CDLL, handle) -> int:
    """Test hook (vct_debug_sky_path): the address path the context's last sky march was
    launched with -- 32 (buffer resources), 64 (64-bit addresses), 0 before any."""
    fn = lib.vct_debug_sky_path
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p]
    return int(fn(handle))


def debug_sky_view(lib: C.CDLL, force64: int = -1) -> None:
    """Test and tool hook (vct_debug_sky_view, not part of the headers).  force64 >= 0,
    process-wide: nonzero sends every grid's specular sky march through the 64-bit-address path
    (the one 1024^3 takes)."""
    fn = lib.vct_debug_sky_view
    fn.restype = C.c_int
    fn.argtypes = [C.c_int]
    fn(int(force64))


def debug_sky_view_path(lib: C.CDLL, handle) -> int:
    """Test hook (vct_debug_sky_view_path): the address path the context's last specular sky
    march was launched with -- 32 (buffer resources), 64 (64-bit addresses), 0 before any."""
    fn = lib.vct_debug_sky_view_path
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p]
    return int(fn(handle))


def debug_env(lib: C.CDLL, force64: int = -1) -> None:
    """Test and tool hook (vct_debug_env, not part of the headers).  force64 >= 0, process-wide:
    nonzero sends every grid's env marches through the 64-bit-address path (the one 1024^3 takes)."""
    fn = lib.vct_debug_env
    fn.restype = C.c_int
    fn.argtypes = [C.c_int]
    fn(int(force64))


def debug_env_mips(lib: C.CDLL, handle, profile: int = -1) -> float:
    """Tool hook (vct_debug_env_mips).  profile >= 0: nonzero times the mip kernels of the
    context's following set_env calls with events.  -> ms of the last timed build."""
    fn = lib.vct_debug_env_mips
    fn.restype = C.c_float
    fn.argtypes = [C.c_void_p, C.c_int]
    return float(fn(handle, int(profile)))


def debug_env_path(lib: C.CDLL, handle) -> int:
    """Test hook (vct_debug_env_path): the address path the context's last env march was
    launched with: 32, 64, or 0 before the first one."""
    fn = lib.vct_debug_env_path
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p]
    return int(fn(handle))


def debug_shadow(lib: C.CDLL, force64: bool = False):
    """Test hook (vct_debug_shadow, not part of the headers), process-wide: send every grid
    through the 64-bit-address path of the shadow cones (the one 1024^3 takes)."""
    fn = lib.vct_debug_shadow
    fn.restype = None
    fn.argtypes = [C.c_int]
    fn(1 if force64 else 0)


def debug_shadow_path(lib: C.CDLL, handle) -> int:
    """Test hook (vct_debug_shadow_path): the address path the context's last shadow-cone
    march was launched with -- 32 (buffer resources), 64 (64-bit addresses), 0 before any."""
    fn = lib.vct_debug_shadow_path
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p]
    return int(fn(handle))


def debug_lights(lib: C.CDLL, form: int = -1, pair_cap: int = 0, count: bool = False, route: bool = True):
    """Tool / test hook (vct_debug_lights, not part of the headers), process-wide: the form
    vct_inject_lights runs (-1 the shipped one, 0 one light per pass, 1 batched pairs), a cap
    on the pair list in entries (0: the default), cell counting, and whether a list of one
    directional light goes to vct_inject_directional's kernels."""
    fn = lib.vct_debug_lights
    fn.restype = None
    fn.argtypes = [C.c_int, C.c_uint32, C.c_int, C.c_int]
    fn(form, pair_cap, 1 if count else 0, 1 if route else 0)


def debug_lights_stats(lib: C.CDLL, handle):
    """(pairs walked, cells stepped) of the context's last vct_inject_lights (cells only
    with counting on, debug_lights); waits for the ctx stream."""
    fn = lib.vct_debug_lights_stats
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 2)()
    if fn(handle, out) != 0:
        return None
    return int(out[0]), int(out[1])


def debug_zmap(lib: C.CDLL, handle, m: int):
    """Test hook (vct_debug_zmap, not part of include/vct.h): K4's empty-space map m of the
    last build_mips as a uint32 array [dim, dim, rw] (z, y, row dwords), or None when the
    context has no such map or its maps are not current."""
    import numpy as np
    fn = lib.vct_debug_zmap
    fn.restype = C.c_longlong
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    cfg = VctConfig()
    if lib.vct_get_config(handle, C.byref(cfg)) != 0:
        return None
    dim_max = cfg.n + 1
    out = np.zeros(dim_max * dim_max * ((dim_max + 31) // 32), np.uint32)
    dim, rw = C.c_uint32(), C.c_uint32()
    words = fn(handle, m, out.ctypes.data, out.size, C.byref(dim), C.byref(rw))
    if words < 0:
        return None
    return out[:words].reshape(dim.value, dim.value, rw.value).copy()
