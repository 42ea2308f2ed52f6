"""MI355X-native per-pixel hot path of the Chaos course ray tracer -- Python-side loader.

The product is the shared library `libcrt_hip.so` (HIP kernels for gfx950 + the C ABI of
include/crt_hip.h and include/crt_host.h + the C++ host mirror of the reference's
SceneParser / RayTracer).  This module only loads it with ctypes and wraps the handles; it holds
no rendering logic and has NO fallback: if the library is missing, or no GPU is present when a
tracer is created, it raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import scenes  # noqa: F401  (synthetic workload generators)

HERE = os.path.dirname(os.path.abspath(__file__))
# libcrt_hip.so is the product; libcrt_hip_test.so is the same objects plus the unit-test hooks (TEST_HOOK_SYMBOLS below), which the
# test suite loads (tests/conftest.py sets CRT_TEST_HOOKS; this package reads the variable, the library itself reads none)
LIB_PATH = os.path.join(HERE, "libcrt_hip_test.so" if os.environ.get("CRT_TEST_HOOKS") else "libcrt_hip.so")

CRT_OK, CRT_ERR_INVALID, CRT_ERR_NO_DEVICE, CRT_ERR_HIP, CRT_ERR_NOMEM, CRT_ERR_IO, CRT_ERR_PARSE = range(7)
OPT_NONE, OPT_REGIONS, OPT_BUCKETS_POOL, OPT_BUCKETS_QUEUE, OPT_AABB, OPT_BUCKETS_POOL_AABB, \
    OPT_BUCKETS_QUEUE_AABB, OPT_BVH, OPT_BVH_BUCKETS_POOL, OPT_BVH_BUCKETS_QUEUE = range(10)
LINK_END, LINK_LEAF, ENTRY_LAST = 0xFFFFFFFF, 0x80000000, 0x80000000


class CrtError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("crt error %d: %s" % (code, message))
        self.code = code


class Node(C.Structure):
    _fields_ = [("lo", C.c_float * 3), ("miss", C.c_uint32), ("hi", C.c_float * 3), ("link", C.c_uint32)]


class Triangle(C.Structure):
    _fields_ = [("v0", C.c_float * 3), ("nx", C.c_float), ("v1", C.c_float * 3), ("ny", C.c_float),
                ("v2", C.c_float * 3), ("nz", C.c_float), ("plane", C.c_float), ("pad", C.c_uint32 * 3)]


class MeshRec(C.Structure):
    _fields_ = [("root", C.c_uint32), ("material", C.c_uint32), ("flags", C.c_uint32), ("pad", C.c_uint32)]


class MaterialRec(C.Structure):
    _fields_ = [("albedo", C.c_float * 3), ("ior", C.c_float), ("type", C.c_uint32), ("smooth", C.c_uint32),
                ("texture", C.c_int32), ("pad", C.c_uint32)]


class TextureRec(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("color_a", C.c_float * 3), ("color_b", C.c_float * 3), ("scalar", C.c_float),
                ("width", C.c_uint32), ("height", C.c_uint32), ("texel_offset", C.c_uint64)]


class LightRec(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("intensity", C.c_uint32)]


class SceneDesc(C.Structure):
    _fields_ = [
        ("width", C.c_uint32), ("height", C.c_uint32), ("background", C.c_float * 3),
        ("nodes", C.POINTER(Node)), ("n_nodes", C.c_uint32), ("top_root", C.c_uint32),
        ("leaf_triangles", C.POINTER(C.c_uint32)), ("n_leaf_triangles", C.c_uint64),
        ("leaf_meshes", C.POINTER(C.c_uint32)), ("n_leaf_meshes", C.c_uint32),
        ("triangles", C.POINTER(Triangle)), ("n_triangles", C.c_uint32),
        ("triangle_vertices", C.POINTER(C.c_uint32)),
        ("vertex_normals", C.POINTER(C.c_float)), ("vertex_uvs", C.POINTER(C.c_float)), ("n_vertices", C.c_uint32),
        ("meshes", C.POINTER(MeshRec)), ("n_meshes", C.c_uint32),
        ("materials", C.POINTER(MaterialRec)), ("n_materials", C.c_uint32),
        ("textures", C.POINTER(TextureRec)), ("n_textures", C.c_uint32),
        ("texels", C.POINTER(C.c_uint8)), ("n_texels", C.c_uint64),
        ("lights", C.POINTER(LightRec)), ("n_lights", C.c_uint32),
    ]


class Options(C.Structure):
    _fields_ = [("max_depth", C.c_uint32), ("shadow_bias", C.c_float), ("reflection_bias", C.c_float),
                ("refraction_bias", C.c_float), ("use_gi", C.c_uint32), ("collect_counters", C.c_uint32),
                ("gi_sample_size", C.c_uint32), ("rays_per_pixel", C.c_uint32), ("monte_carlo_bias", C.c_float), ("gi_seed", C.c_uint32)]


class Rect(C.Structure):
    _fields_ = [("row", C.c_uint32), ("col", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("total_ms", C.c_double), ("box_tests", C.c_uint64),
                ("tri_tests", C.c_uint64), ("leaf_index_reads", C.c_uint64), ("shaded_hits", C.c_uint64),
                ("light_evals", C.c_uint64), ("texel_fetches", C.c_uint64), ("primary_rays", C.c_uint64),
                ("secondary_rays", C.c_uint64), ("shadow_rays", C.c_uint64), ("pixels", C.c_uint64),
                ("counters_valid", C.c_uint32), ("fallback_frames", C.c_uint32), ("queue_bytes", C.c_uint64),
                ("queue_regrows", C.c_uint64)]

    def counters(self):
        return {k: int(getattr(self, k)) for k in ("box_tests", "tri_tests", "leaf_index_reads", "shaded_hits",
                                                   "light_evals", "texel_fetches", "primary_rays", "secondary_rays",
                                                   "shadow_rays")}


# ---- ray queries (include/crt_hip.h: crt_trace_rays*, crt_occluded_rays*, crt_camera_rays_device)
RAY_PRIMARY, RAY_SHADOW, RAY_REFLECTION, RAY_REFRACTION = range(4)   # enum RayType, Ray.h:14


class Ray(C.Structure):
    """crt_ray, 24 bytes"""
    _fields_ = [("origin", C.c_float * 3), ("direction", C.c_float * 3)]


class Hit(C.Structure):
    """crt_hit, 48 bytes"""
    _fields_ = [("t", C.c_float), ("point", C.c_float * 3), ("normal", C.c_float * 3), ("u", C.c_float), ("v", C.c_float),
                ("mesh", C.c_uint32), ("triangle", C.c_uint32), ("hit", C.c_uint32)]


class QueryStats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("hits", C.c_uint64), ("rerouted", C.c_uint64), ("kernel_ms", C.c_double)]


class ShootStats(C.Structure):
    """crt_shoot_stats: the last radiance query (Tracer.shoot_rays*)"""
    _fields_ = [("rays", C.c_uint64), ("levels", C.c_uint32), ("pad", C.c_uint32), ("level_rays", C.c_uint64 * 64),
                ("shadow_records", C.c_uint64), ("rerouted", C.c_uint64), ("kernel_ms", C.c_double)]


class ShootReport(C.Structure):
    """crt_shoot_report: what the device writes for a Tracer.shoot_rays*_enqueue call"""
    _fields_ = [("levels", C.c_uint32), ("overflow", C.c_uint32), ("dropped", C.c_uint64), ("level_rays", C.c_uint64 * 64),
                ("hits", C.c_uint64), ("shadow_records", C.c_uint64), ("rerouted", C.c_uint64)]


class Adaptive(C.Structure):
    """crt_adaptive: the stopping rule's settings of an adaptively sampled GI frame (make_adaptive fills it)"""
    _fields_ = [("size", C.c_uint32), ("min_samples", C.c_uint32), ("max_samples", C.c_uint32), ("threshold", C.c_float), ("floor", C.c_float)]


def _make_settings(kind, name, fields, reserved=("size",), cast=None):
    """a `kind` structure as crt_<name>_defaults fills it, with the given fields replaced"""
    s = kind()
    getattr(lib(), "crt_%s_defaults" % name)(C.byref(s))
    for k, v in fields.items():
        if k not in dict(kind._fields_) or k in reserved:
            raise KeyError("crt_%s has no field %r" % (name, k))
        setattr(s, k, cast(v) if cast else v)
    return s


def make_adaptive(**fields):
    """crt_adaptive_defaults (4, 64, 0.05, 1e-4) with the given fields replaced, e.g. make_adaptive(min_samples=2, max_samples=8)."""
    return _make_settings(Adaptive, "adaptive", fields)


class Denoise(C.Structure):
    """crt_denoise: the settings of the GI frames' denoiser (make_denoise fills it)"""
    _fields_ = [("size", C.c_uint32), ("iterations", C.c_uint32), ("normal_squarings", C.c_uint32), ("sigma_colour", C.c_float),
                ("sigma_plane", C.c_float), ("floor", C.c_float)]


def make_denoise(**fields):
    """crt_denoise_defaults (4, 5, 2.0, 0.02, 1e-6) with the given fields replaced, e.g. make_denoise(iterations=3)."""
    return _make_settings(Denoise, "denoise", fields)


class Temporal(C.Structure):
    """crt_temporal: the settings of the GI frames' temporal accumulation (make_temporal fills it)"""
    _fields_ = [("size", C.c_uint32), ("max_history", C.c_float), ("normal_min", C.c_float), ("sigma_plane", C.c_float)]


class CameraPose(C.Structure):
    """crt_camera_pose: what crt_set_camera takes"""
    _fields_ = [("position", C.c_float * 3), ("matrix", C.c_float * 9)]


def make_temporal(**fields):
    """crt_temporal_defaults (64.0, 0.9, 0.02) with the given fields replaced, e.g. make_temporal(max_history=16.0)."""
    return _make_settings(Temporal, "temporal", fields)


class VarianceEstimate(C.Structure):
    """crt_variance_estimate: the settings of the GI frames' variance estimate (make_variance_estimate fills it)"""
    _fields_ = [("size", C.c_uint32), ("min_history", C.c_float), ("normal_squarings", C.c_uint32), ("sigma_plane", C.c_float)]


def make_variance_estimate(**fields):
    """crt_variance_estimate_defaults (4.0, 5, 0.02) with the given fields replaced, e.g. make_variance_estimate(min_history=2.0)."""
    return _make_settings(VarianceEstimate, "variance_estimate", fields)


class Bake(C.Structure):
    """crt_bake, 28 bytes: what is baked (make_bake fills it)"""
    _fields_ = [("mesh", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("samples", C.c_uint32), ("dilate", C.c_uint32),
                ("check_probes", C.c_uint32), ("probe_offset", C.c_float)]


class BakeStats(C.Structure):
    """crt_bake_stats: the last Tracer.bake_lightmap call"""
    _fields_ = [("texels", C.c_uint64), ("covered", C.c_uint64), ("dilated", C.c_uint64), ("probe_self", C.c_uint64),
                ("raster_ms", C.c_double), ("shoot_ms", C.c_double), ("total_ms", C.c_double)]


def make_bake(**fields):
    """crt_bake_defaults (mesh 0, 256 x 256, 1 sample, dilate 2, check_probes 0, probe_offset 1e-3) with the given fields replaced."""
    return _make_settings(Bake, "bake", fields, reserved=())


# crt_bake_texel as a numpy record (48 bytes; the layout of a torch.uint8 [n, 48] tensor)
BAKE_TEXEL_DTYPE = np.dtype([("point", np.float32, 3), ("u", np.float32), ("normal", np.float32, 3), ("v", np.float32), ("triangle", np.uint32),
                             ("mesh", np.uint32), ("status", np.uint32), ("pad", np.uint32)])
BAKE_EMPTY, BAKE_COVERED, BAKE_DILATED = range(3)


class ProbeVolume(C.Structure):
    """crt_probe_volume, 48 bytes: where the probes stand and how many rays each shoots (make_probe_volume fills it)"""
    _fields_ = [("origin", C.c_float * 3), ("spacing", C.c_float * 3), ("nx", C.c_uint32), ("ny", C.c_uint32), ("nz", C.c_uint32), ("rays", C.c_uint32),
                ("gi_seed", C.c_uint32), ("backface_limit", C.c_float)]


class ProbeStats(C.Structure):
    """crt_probe_stats: the last Tracer.bake_probes call"""
    _fields_ = [("probes", C.c_uint64), ("invalid", C.c_uint64), ("rays", C.c_uint64), ("shoot_ms", C.c_double), ("project_ms", C.c_double),
                ("total_ms", C.c_double)]


class ProbeLitStats(C.Structure):
    """crt_probe_lit_stats: the DIFFUSE records of the last probe-lit query that took light from the volume, and those that found no probe"""
    _fields_ = [("lit", C.c_uint64), ("unlit", C.c_uint64)]


def make_probe_volume(**fields):
    """crt_probe_volume_defaults (origin 0, spacing 1, 1 x 1 x 1, 64 rays, gi_seed 0, backface_limit 1.0) with the given fields replaced;
    origin and spacing take three numbers each."""
    v = ProbeVolume()
    lib().crt_probe_volume_defaults(C.byref(v))
    for k, val in fields.items():
        if k not in dict(ProbeVolume._fields_):
            raise KeyError("crt_probe_volume has no field %r" % (k,))
        setattr(v, k, (C.c_float * 3)(*[float(x) for x in val]) if k in ("origin", "spacing") else val)
    return v


# crt_probe as a numpy record (128 bytes; the layout of a torch.uint8 [n, 128] tensor)
PROBE_DTYPE = np.dtype([("coef", np.float32, (9, 3)), ("rays", np.uint32), ("back", np.uint32), ("miss", np.uint32), ("state", np.uint32),
                        ("pad", np.uint32)])
PROBE_INVALID, PROBE_VALID = range(2)


class ProbeVisibility(C.Structure):
    """crt_probe_visibility, 20 bytes: the parameters of the Chebyshev-weighted lookup (make_probe_visibility fills it from a volume)"""
    _fields_ = [("size", C.c_uint32), ("max_distance", C.c_float), ("normal_bias", C.c_float), ("variance_floor", C.c_float), ("min_weight", C.c_float)]


def make_probe_visibility(volume, **fields):
    """crt_probe_visibility_defaults of the volume (max_distance 1.5 x the cell diagonal, normal_bias 0.02 x the smallest spacing,
    variance_floor 1e-6 x max_distance^2, min_weight 0.01) with the given fields replaced."""
    p = ProbeVisibility()
    if lib().crt_probe_visibility_defaults(C.byref(volume), C.byref(p)) != CRT_OK:
        raise ValueError("make_probe_visibility: the volume is not valid")
    for k, val in fields.items():
        if k not in dict(ProbeVisibility._fields_):
            raise KeyError("crt_probe_visibility has no field %r" % (k,))
        setattr(p, k, val)
    return p


# crt_probe_depth as a numpy record (512 bytes: (mean, mean2) of the 64 texels of a probe's 8 x 8 octahedral map)
PROBE_DEPTH_DTYPE = np.dtype([("moments", np.float32, (64, 2))])


def make_pose(position, matrix):
    """a crt_camera_pose of 3 and 9 floats"""
    pose = CameraPose()
    pose.position[:] = [float(v) for v in np.asarray(position, dtype=np.float32).reshape(3)]
    pose.matrix[:] = [float(v) for v in np.asarray(matrix, dtype=np.float32).reshape(9)]
    return pose


# crt_history_pixel as a numpy record (64 bytes; the layout of a torch.uint8 [n, 64] tensor)
HISTORY_DTYPE = np.dtype([("n", np.float32, 3), ("t", np.float32), ("x", np.float32, 3), ("mesh", np.uint32), ("c", np.float32, 3),
                          ("m2", np.float32), ("weight", np.float32), ("pad", np.float32, 3)])


# crt_hit as a numpy record (what Tracer.trace_rays returns, and the layout of a torch.uint8 [n, 48] output tensor)
HIT_DTYPE = np.dtype([("t", np.float32), ("point", np.float32, 3), ("normal", np.float32, 3), ("u", np.float32), ("v", np.float32),
                      ("mesh", np.uint32), ("triangle", np.uint32), ("hit", np.uint32)])

# direct lighting of the caller's records (include/crt_hip.h: crt_shade_hits*, crt_light_points*): the status of a record
SHADE_BACKGROUND, SHADE_DIFFUSE, SHADE_RECURSES, SHADE_INVALID = range(4)

MODE_STREAM, MODE_LANES = range(2)


class Tuning(C.Structure):
    """crt_tuning (include/crt_hip.h): kernel selection and sizing; no setting changes a pixel."""
    _fields_ = [(n, C.c_uint32) for n in (
        "size", "mode", "step_budget", "shadow_budget", "level0_budget", "heavy_level", "side_blocks",
        "node_cap", "ray_cap", "shadow_cap", "bvh", "level_queue", "fetch_chunk")]


def make_tuning(**fields):
    """Default tuning (crt_tuning_defaults) with the given fields replaced, e.g. make_tuning(mode=MODE_LANES)."""
    return _make_settings(Tuning, "tuning", fields, reserved=("size", "reserved"), cast=int)


def tuning_from_string(text):
    """'quad=0 heavy_level=0' -> make_tuning(quad=0, heavy_level=0); '' -> None.  Used by the development tools
    (tools/*.py read it from their command line or from the CRT_TUNING variable); the library itself reads no
    environment variables."""
    text = (text or "").strip()
    if not text:
        return None
    return make_tuning(**{k: int(v, 0) for k, v in (kv.split("=") for kv in text.split())})


# every symbol include/crt_hip.h and include/crt_host.h declare; the test hooks are exported by libcrt_hip_test.so only
TEST_HOOK_SYMBOLS = ["crt_bvh_selftest", "crt_bvh_census", "crt_debug_set_filter_stack", "crt_debug_set_query_chunks", "crt_test_pow5", "crt_test_gi",
                     "crt_debug_multi_force_staged", "crt_debug_multi_fail_next_alloc", "crt_debug_set_probe_chunk"]
DEVICE_SYMBOLS = ["crt_bvh_selftest", "crt_bvh_census", "crt_debug_set_filter_stack", "crt_debug_set_query_chunks", "crt_tuning_defaults", "crt_create_tuned", "crt_create", "crt_set_camera", "crt_render", "crt_render_tiles_device", "crt_packed_tile_count",
                  "crt_unpack_tiles_device", "crt_quantize_device", "crt_read_quantized", "crt_kernel_elapsed_ms", "crt_kernel_times_ms",
                  "crt_get_stats", "crt_get_kernel_counters", "crt_synchronize", "crt_destroy", "crt_last_error", "crt_device_count", "crt_test_pow5", "crt_test_gi",
                  "crt_describe_kernels", "crt_debug_stream_counts", "crt_get_executed_counters", "crt_get_executed_plan_tests",
                  "crt_render_async", "crt_wait", "crt_alloc_pinned", "crt_free_pinned",
                  "crt_trace_rays", "crt_trace_rays_device", "crt_occluded_rays", "crt_occluded_rays_device", "crt_camera_rays_device",
                  "crt_get_query_stats", "crt_shade_hits", "crt_shade_hits_device", "crt_light_points", "crt_light_points_device",
                  "crt_shoot_rays", "crt_shoot_rays_device", "crt_get_shoot_stats", "crt_shoot_rays_gi", "crt_shoot_rays_gi_device",
                  "crt_shoot_rays_enqueue", "crt_shoot_rays_gi_enqueue", "crt_get_shoot_report", "crt_query_scratch_generation",
                  "crt_camera_sample_rays_device", "crt_accumulate_samples_device", "crt_render_progressive", "crt_progressive_samples",
                  "crt_adaptive_defaults", "crt_adaptive_work_bytes", "crt_adaptive_step_device", "crt_render_adaptive", "crt_progressive_active",
                  "crt_denoise_defaults", "crt_denoise_work_bytes", "crt_sample_variance_device", "crt_denoise_device", "crt_render_denoised",
                  "crt_temporal_defaults", "crt_temporal_device", "crt_render_accumulated", "crt_history_reset", "crt_history_frames",
                  "crt_shoot_rays_gi_split", "crt_shoot_rays_gi_split_device", "crt_split_fold_device", "crt_split_recombine_device",
                  "crt_render_adaptive_split", "crt_read_split_state", "crt_render_denoised_split", "crt_render_accumulated_split", "crt_history_frames_split",
                  "crt_guide_work_bytes", "crt_guide_rays", "crt_guide_rays_device", "crt_set_guide_bounces", "crt_guide_bounces",
                  "crt_variance_estimate_defaults", "crt_variance_estimate_device", "crt_set_variance_estimate", "crt_get_variance_estimate",
                  "crt_bake_defaults", "crt_bake_work_bytes", "crt_bake_texels_device", "crt_bake_dilate_device", "crt_bake_lightmap", "crt_get_bake_stats",
                  "crt_probe_volume_defaults", "crt_probe_rays_device", "crt_probe_project_device", "crt_probe_validity_device", "crt_probe_irradiance_device",
                  "crt_bake_probes", "crt_probe_irradiance", "crt_get_probe_stats", "crt_debug_set_probe_chunk",
                  "crt_probe_visibility_defaults", "crt_probe_depth_device", "crt_probe_irradiance_visible_device", "crt_probe_irradiance_visible",
                  "crt_bake_probes_visible",
                  "crt_probe_light_hits_device", "crt_shoot_rays_lit", "crt_shoot_rays_lit_device", "crt_render_probe_lit", "crt_render_probe_lit_host", "crt_get_probe_lit_stats",
                  "crt_build_tree_device", "crt_built_tree_node_count", "crt_built_tree_index_total", "crt_built_tree_boxes",
                  "crt_built_tree_links", "crt_built_tree_indexes", "crt_built_tree_free", "crt_build_last_error",
                  "crt_multi_create", "crt_multi_set_camera", "crt_multi_render", "crt_multi_read_quantized", "crt_multi_get_stats",
                  "crt_multi_device_count", "crt_multi_context", "crt_multi_last_error", "crt_multi_destroy",
                  "crt_multi_staged_parts", "crt_multi_peer_note", "crt_debug_multi_force_staged", "crt_debug_multi_fail_next_alloc"]
HOST_SYMBOLS = ["crt_host_tracer_note", "crt_host_scene_parse_file", "crt_host_scene_parse_text", "crt_host_scene_parse_text_ex",
                "crt_host_scene_build_seconds", "crt_host_scene_free", "crt_host_scene_desc",
                "crt_host_scene_settings", "crt_host_scene_camera", "crt_host_scene_mesh_count",
                "crt_host_tree_node_count", "crt_host_tree_index_total", "crt_host_tree_dump", "crt_host_mesh_sizes",
                "crt_host_mesh_normals", "crt_host_bucket_rects", "crt_host_camera_apply", "crt_host_tracer_create", "crt_host_tracer_create_tuned",
                "crt_host_tracer_create_multi", "crt_host_tracer_stats",
                "crt_host_tracer_free", "crt_host_tracer_set_camera", "crt_host_tracer_render", "crt_host_tracer_ctx", "crt_host_tracer_multi",
                "crt_host_export_ppm", "crt_host_last_error", "crt_host_shoot_stats_layout"]

_lib = None


def lib():
    """Load libcrt_hip.so (built by `make -C course-assignment-danielhalachev_amd` / __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("the library is not built (%s): run __graft_entry__.build(); there is no fallback path"
                          % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int
    L.crt_create.argtypes = [C.POINTER(SceneDesc), i32, C.POINTER(vp)]
    L.crt_set_camera.argtypes = [vp, vp, vp]
    L.crt_render.argtypes = [vp, C.POINTER(Options), C.POINTER(Rect), u32, vp]
    L.crt_render_tiles_device.argtypes = [vp, C.POINTER(Options), u32, u32, vp, vp]
    L.crt_render_async.argtypes = [vp, C.POINTER(Options), C.POINTER(Rect), u32, vp, vp]
    L.crt_wait.argtypes = [vp]
    L.crt_alloc_pinned.restype = vp
    L.crt_alloc_pinned.argtypes = [C.c_size_t]
    L.crt_free_pinned.restype = None
    L.crt_free_pinned.argtypes = [vp]
    L.crt_packed_tile_count.restype = u32
    L.crt_packed_tile_count.argtypes = [vp, u32, u32]
    L.crt_unpack_tiles_device.argtypes = [vp, vp, u32, C.c_uint64, vp, vp]
    L.crt_quantize_device.argtypes = [vp, vp, C.c_uint64, vp, vp]
    L.crt_read_quantized.argtypes = [vp, vp]
    L.crt_kernel_elapsed_ms.argtypes = [vp, C.POINTER(C.c_double)]
    L.crt_kernel_times_ms.argtypes = [vp, C.POINTER(C.c_double), u32, C.POINTER(u32)]
    L.crt_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.crt_trace_rays.argtypes = [vp, vp, C.c_uint64, u32, vp]
    L.crt_trace_rays_device.argtypes = [vp, vp, C.c_uint64, u32, vp, vp]
    L.crt_occluded_rays.argtypes = [vp, vp, vp, C.c_uint64, vp]
    L.crt_occluded_rays_device.argtypes = [vp, vp, vp, C.c_uint64, vp, vp]
    L.crt_camera_rays_device.argtypes = [vp, vp, vp]
    L.crt_get_query_stats.argtypes = [vp, C.POINTER(QueryStats)]
    L.crt_shade_hits.argtypes = [vp, vp, C.c_uint64, C.POINTER(Options), vp, vp]
    L.crt_shade_hits_device.argtypes = [vp, vp, C.c_uint64, C.POINTER(Options), vp, vp, vp]
    L.crt_light_points.argtypes = [vp, vp, vp, C.c_uint64, C.c_float, vp]
    L.crt_light_points_device.argtypes = [vp, vp, vp, C.c_uint64, C.c_float, vp, vp]
    L.crt_shoot_rays.argtypes = [vp, vp, C.c_uint64, u32, C.POINTER(Options), vp]
    L.crt_shoot_rays_device.argtypes = [vp, vp, C.c_uint64, u32, C.POINTER(Options), vp, vp]
    L.crt_get_shoot_stats.argtypes = [vp, C.POINTER(ShootStats)]
    L.crt_shoot_rays_gi.argtypes = [vp, vp, vp, C.c_uint64, u32, C.POINTER(Options), vp]
    L.crt_shoot_rays_gi_device.argtypes = [vp, vp, vp, C.c_uint64, u32, C.POINTER(Options), vp, vp]
    L.crt_shoot_rays_enqueue.argtypes = [vp, vp, C.c_uint64, u32, C.POINTER(Options), vp, vp, vp, vp]
    L.crt_shoot_rays_gi_enqueue.argtypes = [vp, vp, vp, C.c_uint64, u32, C.POINTER(Options), vp, vp, vp, vp]
    L.crt_get_shoot_report.argtypes = [vp, C.POINTER(ShootReport)]
    L.crt_query_scratch_generation.argtypes = [vp]
    L.crt_query_scratch_generation.restype = C.c_uint64
    L.crt_camera_sample_rays_device.argtypes = [vp, u32, u32, vp, C.c_uint64, vp, vp, vp]
    L.crt_accumulate_samples_device.argtypes = [vp, vp, vp, C.c_uint64, u32, vp, vp, vp]
    L.crt_render_progressive.argtypes = [vp, C.POINTER(Options), u32, u32, vp]
    L.crt_progressive_samples.argtypes = [vp]
    L.crt_progressive_samples.restype = u32
    L.crt_adaptive_defaults.argtypes = [C.POINTER(Adaptive)]
    L.crt_adaptive_defaults.restype = None
    L.crt_adaptive_work_bytes.argtypes = [C.c_uint64]
    L.crt_adaptive_work_bytes.restype = C.c_size_t
    L.crt_adaptive_step_device.argtypes = [vp, vp, vp, C.c_uint64, u32, C.POINTER(Adaptive), vp, vp, vp, vp, vp, vp, vp, vp]
    L.crt_render_adaptive.argtypes = [vp, C.POINTER(Options), C.POINTER(Adaptive), u32, u32, vp, vp]
    L.crt_progressive_active.argtypes = [vp]
    L.crt_progressive_active.restype = C.c_uint64
    L.crt_denoise_defaults.argtypes = [C.POINTER(Denoise)]
    L.crt_denoise_defaults.restype = None
    L.crt_denoise_work_bytes.argtypes = [u32, u32]
    L.crt_denoise_work_bytes.restype = C.c_size_t
    L.crt_sample_variance_device.argtypes = [vp, vp, vp, vp, C.c_uint64, vp, vp, vp]
    L.crt_denoise_device.argtypes = [vp, C.POINTER(Denoise), u32, u32, vp, vp, vp, vp, vp, vp, vp]
    L.crt_render_denoised.argtypes = [vp, C.POINTER(Denoise), vp, vp]
    L.crt_temporal_defaults.argtypes = [C.POINTER(Temporal)]
    L.crt_temporal_defaults.restype = None
    L.crt_temporal_device.argtypes = [vp, C.POINTER(Temporal), u32, u32, C.POINTER(CameraPose)] + [vp] * 10
    L.crt_render_accumulated.argtypes = [vp, C.POINTER(Temporal), C.POINTER(Denoise), vp, vp, vp]
    L.crt_history_reset.argtypes = [vp]
    L.crt_history_frames.argtypes = [vp]
    L.crt_history_frames.restype = u32
    L.crt_shoot_rays_gi_split.argtypes = [vp, vp, vp, C.c_uint64, u32, C.POINTER(Options), vp, vp]
    L.crt_shoot_rays_gi_split_device.argtypes = [vp, vp, vp, C.c_uint64, u32, C.POINTER(Options), vp, vp, vp]
    L.crt_split_fold_device.argtypes = [vp, vp, vp, vp, C.c_uint64, u32, vp, vp, vp, vp]
    L.crt_split_recombine_device.argtypes = [vp, vp, vp, vp, C.c_uint64, vp, vp]
    L.crt_render_adaptive_split.argtypes = [vp, C.POINTER(Options), C.POINTER(Adaptive), u32, u32, vp, vp]
    L.crt_render_denoised_split.argtypes = [vp, C.POINTER(Denoise), vp, vp]
    L.crt_read_split_state.argtypes = [vp, vp, vp, vp]
    L.crt_render_accumulated_split.argtypes = [vp, C.POINTER(Temporal), C.POINTER(Denoise), vp, vp, vp]
    L.crt_history_frames_split.argtypes = [vp]
    L.crt_guide_work_bytes.restype = C.c_size_t
    L.crt_guide_work_bytes.argtypes = [C.c_uint64]
    L.crt_guide_rays.argtypes = [vp, vp, C.c_uint64, u32, C.POINTER(Options), u32, vp, vp, vp]
    L.crt_guide_rays_device.argtypes = [vp, vp, C.c_uint64, u32, C.POINTER(Options), u32, vp, vp, vp, vp, vp]
    L.crt_set_guide_bounces.argtypes = [vp, u32]
    L.crt_guide_bounces.restype = u32
    L.crt_guide_bounces.argtypes = [vp]
    L.crt_variance_estimate_defaults.argtypes = [C.POINTER(VarianceEstimate)]
    L.crt_variance_estimate_defaults.restype = None
    L.crt_variance_estimate_device.argtypes = [vp, C.POINTER(VarianceEstimate), u32, u32, vp, vp, vp, vp, vp]
    L.crt_set_variance_estimate.argtypes = [vp, C.POINTER(VarianceEstimate)]
    L.crt_get_variance_estimate.argtypes = [vp, C.POINTER(VarianceEstimate)]
    L.crt_history_frames_split.restype = u32
    L.crt_bake_defaults.argtypes = [C.POINTER(Bake)]
    L.crt_bake_defaults.restype = None
    L.crt_bake_work_bytes.argtypes = [u32, u32]
    L.crt_bake_work_bytes.restype = C.c_size_t
    L.crt_bake_texels_device.argtypes = [vp, C.POINTER(Bake), vp, vp, vp, vp]
    L.crt_bake_dilate_device.argtypes = [vp, u32, u32, u32, vp, vp, vp, vp]
    L.crt_bake_lightmap.argtypes = [vp, C.POINTER(Bake), C.POINTER(Options), vp, vp, vp, vp]
    L.crt_get_bake_stats.argtypes = [vp, C.POINTER(BakeStats)]
    L.crt_probe_volume_defaults.argtypes = [C.POINTER(ProbeVolume)]
    L.crt_probe_volume_defaults.restype = None
    L.crt_probe_rays_device.argtypes = [vp, C.POINTER(ProbeVolume), u32, u32, vp, vp, vp]
    L.crt_probe_project_device.argtypes = [vp, vp, vp, u32, u32, vp, vp]
    L.crt_probe_validity_device.argtypes = [vp, vp, vp, u32, u32, C.c_float, vp, vp]
    L.crt_probe_irradiance_device.argtypes = [vp, C.POINTER(ProbeVolume), vp, vp, vp, C.c_uint64, vp, vp, vp]
    L.crt_bake_probes.argtypes = [vp, C.POINTER(ProbeVolume), C.POINTER(Options), vp, vp]
    L.crt_probe_irradiance.argtypes = [vp, C.POINTER(ProbeVolume), vp, vp, vp, C.c_uint64, vp, vp]
    L.crt_get_probe_stats.argtypes = [vp, C.POINTER(ProbeStats)]
    L.crt_probe_visibility_defaults.argtypes = [C.POINTER(ProbeVolume), C.POINTER(ProbeVisibility)]
    L.crt_probe_depth_device.argtypes = [vp, vp, vp, u32, u32, C.c_float, vp, vp]
    L.crt_probe_irradiance_visible_device.argtypes = [vp, C.POINTER(ProbeVolume), C.POINTER(ProbeVisibility), vp, vp, vp, vp, C.c_uint64, vp, vp, vp]
    L.crt_probe_irradiance_visible.argtypes = [vp, C.POINTER(ProbeVolume), C.POINTER(ProbeVisibility), vp, vp, vp, vp, C.c_uint64, vp, vp]
    L.crt_bake_probes_visible.argtypes = [vp, C.POINTER(ProbeVolume), C.POINTER(ProbeVisibility), C.POINTER(Options), vp, vp, vp, vp]
    L.crt_probe_light_hits_device.argtypes = [vp, C.POINTER(ProbeVolume), C.POINTER(ProbeVisibility), vp, vp, vp, vp, C.c_uint64, u32, vp, vp, vp]
    L.crt_shoot_rays_lit_device.argtypes = [vp, vp, C.c_uint64, u32, C.POINTER(Options), C.POINTER(ProbeVolume), C.POINTER(ProbeVisibility), vp, vp, vp, vp]
    L.crt_shoot_rays_lit.argtypes = [vp, vp, C.c_uint64, u32, C.POINTER(Options), C.POINTER(ProbeVolume), C.POINTER(ProbeVisibility), vp, vp, vp]
    L.crt_render_probe_lit.argtypes = [vp, C.POINTER(ProbeVolume), C.POINTER(ProbeVisibility), vp, vp, C.POINTER(Options), vp, vp]
    L.crt_render_probe_lit_host.argtypes = [vp, C.POINTER(ProbeVolume), C.POINTER(ProbeVisibility), vp, vp, C.POINTER(Options), vp, vp]
    L.crt_get_probe_lit_stats.argtypes = [vp, C.POINTER(ProbeLitStats)]
    L.crt_host_shoot_stats_layout.argtypes = [C.POINTER(u32), u32]
    L.crt_host_shoot_stats_layout.restype = u32
    L.crt_get_kernel_counters.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.crt_synchronize.argtypes = [vp]
    L.crt_destroy.argtypes = [vp]
    L.crt_destroy.restype = None
    L.crt_last_error.restype = C.c_char_p
    L.crt_last_error.argtypes = [vp]
    L.crt_host_scene_parse_file.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(vp)]
    L.crt_host_scene_parse_text.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.POINTER(vp)]
    L.crt_host_scene_parse_text_ex.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, i32, C.POINTER(vp)]
    L.crt_host_scene_build_seconds.restype = C.c_double
    L.crt_host_scene_build_seconds.argtypes = [vp]
    L.crt_host_scene_free.argtypes = [vp]
    L.crt_host_scene_free.restype = None
    L.crt_host_scene_desc.restype = C.POINTER(SceneDesc)
    L.crt_host_scene_desc.argtypes = [vp]
    L.crt_host_scene_settings.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
    L.crt_host_scene_settings.restype = None
    L.crt_host_scene_camera.argtypes = [vp, vp, vp]
    L.crt_host_scene_camera.restype = None
    L.crt_host_scene_mesh_count.restype = u32
    L.crt_host_scene_mesh_count.argtypes = [vp]
    L.crt_host_tree_node_count.restype = u32
    L.crt_host_tree_node_count.argtypes = [vp, i32]
    L.crt_host_tree_index_total.restype = C.c_uint64
    L.crt_host_tree_index_total.argtypes = [vp, i32]
    L.crt_host_tree_dump.argtypes = [vp, i32, vp, vp, vp]
    L.crt_host_tree_dump.restype = None
    L.crt_host_mesh_sizes.argtypes = [vp, u32, C.POINTER(u32), C.POINTER(u32)]
    L.crt_host_mesh_sizes.restype = None
    L.crt_host_mesh_normals.argtypes = [vp, u32, vp, vp]
    L.crt_host_mesh_normals.restype = None
    L.crt_host_bucket_rects.restype = u32
    L.crt_host_bucket_rects.argtypes = [u32, u32, u32, i32, u32, C.POINTER(Rect), u32]
    L.crt_host_camera_apply.argtypes = [vp, vp, i32, vp]
    L.crt_host_tracer_create.argtypes = [vp, i32, C.POINTER(vp)]
    L.crt_host_tracer_create_tuned.argtypes = [vp, i32, C.POINTER(Tuning), C.POINTER(vp)]
    L.crt_host_tracer_create_multi.argtypes = [vp, C.POINTER(C.c_int), u32, C.POINTER(Tuning), C.POINTER(vp)]
    L.crt_host_tracer_stats.argtypes = [vp, C.POINTER(Stats)]
    L.crt_tuning_defaults.argtypes = [C.POINTER(Tuning)]
    L.crt_tuning_defaults.restype = None
    L.crt_create_tuned.argtypes = [C.POINTER(SceneDesc), i32, C.POINTER(Tuning), C.POINTER(vp)]
    L.crt_host_tracer_free.argtypes = [vp]
    L.crt_host_tracer_free.restype = None
    L.crt_host_tracer_set_camera.argtypes = [vp, vp, vp]
    L.crt_host_tracer_render.argtypes = [vp, C.c_char_p, i32, C.POINTER(Options), vp]
    L.crt_host_tracer_note.argtypes = [vp]
    L.crt_host_tracer_note.restype = C.c_char_p
    L.crt_host_tracer_ctx.restype = vp
    L.crt_host_tracer_ctx.argtypes = [vp]
    L.crt_host_export_ppm.argtypes = [C.c_char_p, vp, u32, u32]
    L.crt_host_last_error.restype = C.c_char_p
    _lib = L
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def make_options(max_depth=5, shadow_bias=1e-4, reflection_bias=1e-4, refraction_bias=1e-4, counters=False, use_gi=False,
                 gi_sample_size=2, rays_per_pixel=1, monte_carlo_bias=1e-4, gi_seed=0):
    # counters: False / True (the counting build, reference semantics) / 2 (production kernels tallying executed tests)
    # use_gi: the reference's GI / multi-sample mode (RayTracer.h:27-30) with the counter-based generator of csrc/gi_random.h
    return Options(max_depth, shadow_bias, reflection_bias, refraction_bias, int(bool(use_gi)), int(counters), gi_sample_size,
                   rays_per_pixel, monte_carlo_bias, gi_seed)


def _host_check(rc):
    if rc != CRT_OK:
        raise CrtError(rc, lib().crt_host_last_error().decode(errors="replace"))


class Scene:
    """A parsed `.crtscene` with its tree built and flattened (host side only; no GPU needed)."""

    def __init__(self, json_text=None, path=None, folder="", build_device=-1):
        """build_device >= 0: the big meshes' trees are built on that GPU (same trees, node for node)."""
        L = lib()
        h = C.c_void_p()
        if json_text is not None:
            data = json_text.encode() if isinstance(json_text, str) else json_text
            _host_check(L.crt_host_scene_parse_text_ex(data, len(data), folder.encode(), build_device, C.byref(h)))
        else:
            _host_check(L.crt_host_scene_parse_file(path.encode(), folder.encode(), C.byref(h)))
        self._h = h
        w, hh, b = C.c_uint32(), C.c_uint32(), C.c_uint32()
        L.crt_host_scene_settings(h, C.byref(w), C.byref(hh), C.byref(b))
        self.width, self.height, self.bucket_size = w.value, hh.value, b.value
        self.build_seconds = L.crt_host_scene_build_seconds(h)

    def close(self):
        if getattr(self, "_h", None):
            lib().crt_host_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def desc(self):
        return lib().crt_host_scene_desc(self._h).contents

    @property
    def mesh_count(self):
        return lib().crt_host_scene_mesh_count(self._h)

    def camera(self):
        pos = np.zeros(3, dtype=np.float32)
        mat = np.zeros(9, dtype=np.float32)
        lib().crt_host_scene_camera(self._h, _p(pos), _p(mat))
        return pos, mat

    def tree(self, mesh=-1):
        """Tree in the reference's node numbering: (boxes [n,6], links [n,4], indexes [total])."""
        L = lib()
        n = L.crt_host_tree_node_count(self._h, mesh)
        total = L.crt_host_tree_index_total(self._h, mesh)
        boxes = np.zeros((n, 6), dtype=np.float32)
        links = np.zeros((n, 4), dtype=np.uint32)
        idx = np.zeros(max(total, 1), dtype=np.uint32)
        L.crt_host_tree_dump(self._h, mesh, _p(boxes), _p(links), _p(idx))
        return boxes, links, idx[:total]

    def mesh_normals(self, mesh):
        nv, nt = C.c_uint32(), C.c_uint32()
        lib().crt_host_mesh_sizes(self._h, mesh, C.byref(nv), C.byref(nt))
        fn = np.zeros((nt.value, 3), dtype=np.float32)
        vn = np.zeros((nv.value, 3), dtype=np.float32)
        lib().crt_host_mesh_normals(self._h, mesh, _p(fn), _p(vn))
        return fn, vn

    def flat_nodes(self):
        d = self.desc
        return np.ctypeslib.as_array(C.cast(d.nodes, C.POINTER(C.c_uint32)), shape=(d.n_nodes, 8)).copy()

    def flat_leaf_triangles(self):
        d = self.desc
        if d.n_leaf_triangles == 0:
            return np.zeros(0, dtype=np.uint32)
        return np.ctypeslib.as_array(d.leaf_triangles, shape=(d.n_leaf_triangles,)).copy()

    def flat_leaf_meshes(self):
        d = self.desc
        if d.n_leaf_meshes == 0:
            return np.zeros(0, dtype=np.uint32)
        return np.ctypeslib.as_array(d.leaf_meshes, shape=(d.n_leaf_meshes,)).copy()


def bucket_rects(width, height, bucket_size, optimization=OPT_BVH_BUCKETS_POOL, hardware_concurrency=8):
    out = (Rect * 65536)()
    n = lib().crt_host_bucket_rects(width, height, bucket_size, optimization, hardware_concurrency, out, 65536)
    return np.array([[r.row, r.col, r.width, r.height] for r in out[:min(n, 65536)]], dtype=np.uint32).reshape(-1, 4)


def camera_apply(position, matrix, op, v):
    pos = np.ascontiguousarray(position, dtype=np.float32).copy()
    mat = np.ascontiguousarray(matrix, dtype=np.float32).reshape(9).copy()
    vv = np.zeros(3, dtype=np.float32)
    vv[:len(np.atleast_1d(v))] = np.atleast_1d(v)
    _host_check(lib().crt_host_camera_apply(_p(pos), _p(mat), {"truck": 0, "pan": 1, "tilt": 2, "roll": 3}[op], _p(vv)))
    return pos, mat


def export_ppm(path, rgb):
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    _host_check(lib().crt_host_export_ppm(path.encode(), _p(rgb), rgb.shape[1], rgb.shape[0]))


class Tracer:
    """crt::RayTracer on one GPU: scene + tree resident in HBM, re-renderable with a new camera."""

    def __init__(self, scene: Scene, device=0, tuning: Tuning = None, devices=None):
        """devices: a list of GPU indices -> the frame's tiles are dealt over them (crt_multi), devices[0] gathers."""
        L = lib()
        self.scene = scene
        h = C.c_void_p()
        tp = C.byref(tuning) if tuning is not None else None
        if devices:
            arr = (C.c_int * len(devices))(*devices)
            _host_check(L.crt_host_tracer_create_multi(scene._h, arr, len(devices), tp, C.byref(h)))
        else:
            _host_check(L.crt_host_tracer_create_tuned(scene._h, device, tp, C.byref(h)))
        self.devices = list(devices) if devices else [device]
        self._h = h
        self.ctx = C.c_void_p(L.crt_host_tracer_ctx(h))
        self.width, self.height = scene.width, scene.height

    def close(self):
        if getattr(self, "_h", None):
            lib().crt_host_tracer_free(self._h)
            self._h = None

    # ---- several devices: which parts reach devices[0] over xGMI, which are staged through pinned host memory
    def _multi(self):
        L = lib()
        L.crt_host_tracer_multi.restype = C.c_void_p
        L.crt_host_tracer_multi.argtypes = [C.c_void_p]
        m = L.crt_host_tracer_multi(self._h)
        if not m:
            raise RuntimeError("not a multi-device tracer")
        return C.c_void_p(m)

    def staged_parts(self):
        L = lib()
        L.crt_multi_staged_parts.restype = C.c_uint32
        L.crt_multi_staged_parts.argtypes = [C.c_void_p]
        return int(L.crt_multi_staged_parts(self._multi()))

    def peer_note(self):
        L = lib()
        L.crt_multi_peer_note.restype = C.c_char_p
        L.crt_multi_peer_note.argtypes = [C.c_void_p]
        return L.crt_multi_peer_note(self._multi()).decode()

    def fail_next_alloc(self):
        """Tests: the next re-partition of a multi-device tracer stops half-way with CRT_ERR_NOMEM."""
        L = lib()
        L.crt_debug_multi_fail_next_alloc.argtypes = [C.c_void_p]
        self._check(L.crt_debug_multi_fail_next_alloc(self._multi()))

    def force_staged(self, on=True):
        """Tests: every part but the first copies its tiles through pinned host memory, as if no device had peer access."""
        L = lib()
        L.crt_debug_multi_force_staged.argtypes = [C.c_void_p, C.c_int]
        self._check(L.crt_debug_multi_force_staged(self._multi(), 1 if on else 0))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_camera(self, position, matrix):
        p = np.ascontiguousarray(position, dtype=np.float32)
        m = np.ascontiguousarray(matrix, dtype=np.float32).reshape(9)
        _host_check(lib().crt_host_tracer_set_camera(self._h, _p(p), _p(m)))

    def render(self, max_depth=5, optimization=OPT_BVH_BUCKETS_POOL, ppm_path=None, counters=False, out=None,
               options=None):
        """RayTracer::render: returns the H x W x 3 float32 colour buffer (and writes a PPM if asked)."""
        o = options or make_options(max_depth, counters=counters)
        rgb = out if out is not None else np.zeros((self.height, self.width, 3), dtype=np.float32)
        _host_check(lib().crt_host_tracer_render(self._h, ppm_path.encode() if ppm_path else None, optimization,
                                                 C.byref(o), _p(rgb)))
        return rgb

    def note(self) -> str:
        """What the last render did differently from the reference ("" when nothing): a non-tree RenderOptimization renders with the
        tree modes' semantics (crt_host.h: crt_host_tracer_note)."""
        return (lib().crt_host_tracer_note(self._h) or b"").decode()

    def synchronize(self):
        """crt_synchronize on the first context: waits for everything enqueued on its device; afterwards stats() reflects the
        last frame (fallback_frames included)."""
        self._check(lib().crt_synchronize(self.ctx))

    def stats(self) -> Stats:
        s = Stats()
        lib().crt_host_tracer_stats(self._h, C.byref(s))
        return s

    def executed_counters(self):
        """{box_tests, tri_tests} the production kernels executed in the last render made with counters=2."""
        a = (C.c_uint64 * 4)()
        self._check(lib().crt_get_executed_counters(self.ctx, a))
        b = (C.c_uint64 * 2)()
        L = lib()
        L.crt_get_executed_plan_tests.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        self._check(L.crt_get_executed_plan_tests(self.ctx, b))
        return {"box_tests": int(a[0]), "tri_tests": int(a[1]), "shadow_pass0_box_tests": int(a[2]), "shadow_pass0_tri_tests": int(a[3]),
                "plan_tests": int(b[0]), "shadow_pass0_plan_tests": int(b[1])}

    def kernel_counters(self):
        """(recursion levels' counters, bulk shadow pass's counters) of the last counted render, as dicts."""
        names = ("box_tests", "tri_tests", "leaf_index_reads", "shaded_hits", "light_evals", "texel_fetches",
                 "primary_rays", "secondary_rays", "shadow_rays")
        a = (C.c_uint64 * 9)()
        b = (C.c_uint64 * 9)()
        self._check(lib().crt_get_kernel_counters(self.ctx, a, b))
        return ({k: int(a[i]) for i, k in enumerate(names)}, {k: int(b[i]) for i, k in enumerate(names)})

    def _check(self, rc):
        if rc != CRT_OK:
            raise CrtError(rc, lib().crt_last_error(self.ctx).decode(errors="replace"))

    # ---- device-resident API (multi-GPU tile partition, bench)
    def packed_tile_count(self, first, stride):
        return lib().crt_packed_tile_count(self.ctx, first, stride)

    def render_tiles_device(self, options, first, stride, d_packed_ptr, stream_ptr=None):
        self._check(lib().crt_render_tiles_device(self.ctx, C.byref(options), first, stride, C.c_void_p(d_packed_ptr),
                                                  C.c_void_p(stream_ptr or 0)))

    def unpack_tiles_device(self, d_packed_all_ptr, n_parts, part_stride_floats, d_frame_ptr, stream_ptr=None):
        self._check(lib().crt_unpack_tiles_device(self.ctx, C.c_void_p(d_packed_all_ptr), n_parts, part_stride_floats,
                                                  C.c_void_p(d_frame_ptr), C.c_void_p(stream_ptr or 0)))

    def quantize_device(self, d_rgb_ptr, n_values, d_out_ptr, stream_ptr=None):
        self._check(lib().crt_quantize_device(self.ctx, C.c_void_p(d_rgb_ptr), n_values, C.c_void_p(d_out_ptr),
                                              C.c_void_p(stream_ptr or 0)))

    def kernel_elapsed_ms(self):
        ms = C.c_double()
        self._check(lib().crt_kernel_elapsed_ms(self.ctx, C.byref(ms)))
        return ms.value

    def kernel_times_ms(self, max_count=64):
        """[(total, recursion levels, shadow pass 0 [overlapped], shadow pass 1 + heavy, resolve)] in ms of the
        most recent renders, oldest first."""
        a = (C.c_double * (5 * max_count))()
        n = C.c_uint32()
        self._check(lib().crt_kernel_times_ms(self.ctx, a, max_count, C.byref(n)))
        return [tuple(a[5 * i + j] for j in range(5)) for i in range(n.value)]

    # ---- a frame without waiting for it (crt_render_async / crt_wait), through the device-level ABI of the first context
    def render_async(self, options, rgb=None, rgb8=None, optimization=OPT_BVH_BUCKETS_POOL):
        """Enqueue a frame (coverage: the reference's bucket rectangles); rgb / rgb8 are numpy arrays the copies land in
        once wait() has returned."""
        r = bucket_rects(self.width, self.height, self.scene.bucket_size, optimization)
        rects = (Rect * len(r))(*[Rect(*map(int, x)) for x in r])
        self._check(lib().crt_render_async(self.ctx, C.byref(options), rects, len(r), _p(rgb) if rgb is not None else None,
                                           _p(rgb8) if rgb8 is not None else None))

    def wait(self):
        self._check(lib().crt_wait(self.ctx))

    # ---- ray queries: closest hit / occlusion for the caller's rays (include/crt_hip.h has the contract)
    def _single(self, what):
        if len(self.devices) > 1:
            raise RuntimeError("%s: ray queries are not available on a multi-device tracer (devices=...); create a Tracer on one device"
                               % what)

    @staticmethod
    def _rays_array(rays):
        rays = np.ascontiguousarray(rays, dtype=np.float32)
        if rays.ndim != 2 or rays.shape[1] != 6:
            raise ValueError("rays: expected shape [n, 6] (origin xyz, direction xyz), got %r" % (rays.shape,))
        return rays

    def trace_rays(self, rays, ray_type=RAY_REFLECTION):
        """Closest hit of each ray (AccelerationStructure::intersect): rays float32 [n, 6] = origin, direction (used as given, not
        normalised) -> numpy record array of crt_hit (HIT_DTYPE)."""
        self._single("trace_rays")
        rays = self._rays_array(rays)
        out = np.zeros(len(rays), dtype=HIT_DTYPE)
        self._check(lib().crt_trace_rays(self.ctx, _p(rays), len(rays), ray_type, _p(out)))
        return out

    def occluded_rays(self, rays, max_distance):
        """checkForIntersection(ray, max_distance) of each (shadow) ray -> bool [n]; max_distance: a number or an array [n]."""
        self._single("occluded_rays")
        rays = self._rays_array(rays)
        dist = np.ascontiguousarray(np.broadcast_to(np.asarray(max_distance, dtype=np.float32), (len(rays),)))
        out = np.zeros(len(rays), dtype=np.uint8)
        self._check(lib().crt_occluded_rays(self.ctx, _p(rays), _p(dist), len(rays), _p(out)))
        return out.astype(bool)

    def trace_rays_device(self, d_rays_ptr, n, ray_type, d_hits_ptr, stream_ptr=None):
        """The same on device memory (e.g. torch tensors' data_ptr(): rays float32 [n, 6], hits uint8 [n, 48]), asynchronous on the stream."""
        self._single("trace_rays_device")
        self._check(lib().crt_trace_rays_device(self.ctx, C.c_void_p(d_rays_ptr), n, ray_type, C.c_void_p(d_hits_ptr),
                                                C.c_void_p(stream_ptr or 0)))

    def occluded_rays_device(self, d_rays_ptr, d_max_distance_ptr, n, d_out_ptr, stream_ptr=None):
        """rays float32 [n, 6], max_distance float32 [n], out uint8 [n]; asynchronous on the stream."""
        self._single("occluded_rays_device")
        self._check(lib().crt_occluded_rays_device(self.ctx, C.c_void_p(d_rays_ptr), C.c_void_p(d_max_distance_ptr), n,
                                                   C.c_void_p(d_out_ptr), C.c_void_p(stream_ptr or 0)))

    def camera_rays_device(self, d_rays_ptr, stream_ptr=None):
        """RayTracer::getRay at every pixel centre with the current camera: float32 [H * W, 6], row-major, into device memory."""
        self._single("camera_rays_device")
        self._check(lib().crt_camera_rays_device(self.ctx, C.c_void_p(d_rays_ptr), C.c_void_p(stream_ptr or 0)))

    # ---- direct lighting for the caller's hit records and points (RayTracer::calculateDiffusion; include/crt_hip.h has the contract)
    def shade_hits(self, hits, shadow_bias=1e-4):
        """The colour shootRay returns for a ray whose closest hit is hits[i] (records as trace_rays returns them, HIT_DTYPE), wherever
        it does not recurse -> (rgb float32 [n, 3], status uint8 [n] of SHADE_*)."""
        self._single("shade_hits")
        hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE).reshape(-1)
        rgb = np.zeros((len(hits), 3), dtype=np.float32)
        status = np.zeros(len(hits), dtype=np.uint8)
        self._check(lib().crt_shade_hits(self.ctx, _p(hits), len(hits), C.byref(make_options(0, shadow_bias)), _p(rgb), _p(status)))
        return rgb, status

    def light_points(self, points, normals, shadow_bias=1e-4):
        """The sum of the unoccluded lights' factors intensity / (4 r^2 pi) * max(0, l . n) at each point: points, normals float32 [n, 3]
        -> float32 [n] (what a white diffuse surface there is lit with)."""
        self._single("light_points")
        points = np.ascontiguousarray(points, dtype=np.float32)
        normals = np.ascontiguousarray(normals, dtype=np.float32)
        if points.ndim != 2 or points.shape[1] != 3 or normals.shape != points.shape:
            raise ValueError("points, normals: expected two arrays of shape [n, 3], got %r and %r" % (points.shape, normals.shape))
        out = np.zeros(len(points), dtype=np.float32)
        self._check(lib().crt_light_points(self.ctx, _p(points), _p(normals), len(points), shadow_bias, _p(out)))
        return out

    def shade_hits_device(self, d_hits_ptr, n, d_rgb_ptr, d_status_ptr=None, shadow_bias=1e-4, stream_ptr=None):
        """The same on device memory (data_ptr() of: hits uint8 [n, 48], rgb float32 [n, 3], status uint8 [n] or None), asynchronous."""
        self._single("shade_hits_device")
        self._check(lib().crt_shade_hits_device(self.ctx, C.c_void_p(d_hits_ptr), n, C.byref(make_options(0, shadow_bias)), C.c_void_p(d_rgb_ptr),
                                                C.c_void_p(d_status_ptr or 0), C.c_void_p(stream_ptr or 0)))

    def light_points_device(self, d_points_ptr, d_normals_ptr, n, d_out_ptr, shadow_bias=1e-4, stream_ptr=None):
        """points, normals float32 [n, 3], out float32 [n]; asynchronous on the stream."""
        self._single("light_points_device")
        self._check(lib().crt_light_points_device(self.ctx, C.c_void_p(d_points_ptr), C.c_void_p(d_normals_ptr), n, shadow_bias,
                                                  C.c_void_p(d_out_ptr), C.c_void_p(stream_ptr or 0)))

    # ---- radiance queries: shootRay for the caller's rays (include/crt_hip.h has the contract)
    def shoot_rays(self, rays, ray_type=RAY_REFLECTION, max_depth=5, shadow_bias=1e-4, reflection_bias=1e-4, refraction_bias=1e-4):
        """The colour RayTracer::shootRay returns for each ray (direction normalised on entry; reflections, refractions and the Fresnel
        mix down to max_depth): rays float32 [n, 6] -> float32 [n, 3]."""
        self._single("shoot_rays")
        rays = self._rays_array(rays)
        rgb = np.zeros((len(rays), 3), dtype=np.float32)
        o = make_options(max_depth, shadow_bias, reflection_bias, refraction_bias)
        self._check(lib().crt_shoot_rays(self.ctx, _p(rays), len(rays), ray_type, C.byref(o), _p(rgb)))
        return rgb

    def shoot_rays_device(self, d_rays_ptr, n, d_rgb_ptr, ray_type=RAY_REFLECTION, max_depth=5, shadow_bias=1e-4, reflection_bias=1e-4,
                          refraction_bias=1e-4, stream_ptr=None):
        """The same on device memory (data_ptr() of: rays float32 [n, 6], rgb float32 [n, 3]) on the stream; the call waits for the
        stream once per recursion level, so it cannot be captured into a graph."""
        self._single("shoot_rays_device")
        o = make_options(max_depth, shadow_bias, reflection_bias, refraction_bias)
        self._check(lib().crt_shoot_rays_device(self.ctx, C.c_void_p(d_rays_ptr), n, ray_type, C.byref(o), C.c_void_p(d_rgb_ptr),
                                                C.c_void_p(stream_ptr or 0)))

    # ---- radiance queries in the GI mode (include/crt_hip.h: crt_shoot_rays_gi*)
    @staticmethod
    def _gi_options(options, option_fields):
        """`options` (an Options with use_gi set) or make_options(use_gi=True, **option_fields): one of the two"""
        if options is not None:
            if option_fields:
                raise TypeError("shoot_rays_gi: pass either options or option fields, not both (%s)" % ", ".join(sorted(option_fields)))
            return options
        return make_options(**dict(option_fields, use_gi=True))

    def shoot_rays_gi(self, rays, keys=None, ray_type=RAY_REFLECTION, options=None, **option_fields):
        """The colour shootRay of the GI build returns for each ray: rays float32 [n, 6], keys uint32 [n] (the key of each ray's shootRay
        invocation, csrc/gi_random.h) or None for the keys of a frame's pixels 0 .. n - 1, sample 0, under options.gi_seed -> float32
        [n, 3].  options: an Options with use_gi set, or make_options' fields by name (max_depth, gi_sample_size, gi_seed, ...).
        split=True (by name, beside the option fields; the default is False): -> (rgb, direct), the same colours and each one's direct
        part float32 [n, 3] (include/crt_hip.h: "Split GI frames")."""
        self._single("shoot_rays_gi")
        split = bool(option_fields.pop("split", False))
        rays = self._rays_array(rays)
        if keys is not None:
            keys = np.ascontiguousarray(keys, dtype=np.uint32)
            if keys.shape != (len(rays),):
                raise ValueError("keys: expected shape [%d], got %r" % (len(rays), keys.shape))
        rgb = np.zeros((len(rays), 3), dtype=np.float32)
        o = self._gi_options(options, option_fields)
        if split:
            direct = np.zeros((len(rays), 3), dtype=np.float32)
            self._check(lib().crt_shoot_rays_gi_split(self.ctx, _p(rays), _p(keys) if keys is not None else None, len(rays), ray_type, C.byref(o),
                                                      _p(rgb), _p(direct)))
            return rgb, direct
        self._check(lib().crt_shoot_rays_gi(self.ctx, _p(rays), _p(keys) if keys is not None else None, len(rays), ray_type, C.byref(o), _p(rgb)))
        return rgb

    def shoot_rays_gi_device(self, d_rays_ptr, n, d_rgb_ptr, d_keys_ptr=None, ray_type=RAY_REFLECTION, options=None, stream_ptr=None,
                             d_direct_ptr=None, **option_fields):
        """The same on device memory (data_ptr() of: rays float32 [n, 6], rgb float32 [n, 3], keys uint32 [n] or None) on the stream; the
        call waits for the stream once per recursion level, so it cannot be captured into a graph.  d_direct_ptr (float32 [n, 3]): the
        split call, which also writes each colour's direct part."""
        self._single("shoot_rays_gi_device")
        o = self._gi_options(options, option_fields)
        if d_direct_ptr is not None:
            self._check(lib().crt_shoot_rays_gi_split_device(self.ctx, C.c_void_p(d_rays_ptr), C.c_void_p(d_keys_ptr or 0), n, ray_type, C.byref(o),
                                                             C.c_void_p(d_rgb_ptr), C.c_void_p(d_direct_ptr), C.c_void_p(stream_ptr or 0)))
            return
        self._check(lib().crt_shoot_rays_gi_device(self.ctx, C.c_void_p(d_rays_ptr), C.c_void_p(d_keys_ptr or 0), n, ray_type, C.byref(o),
                                                   C.c_void_p(d_rgb_ptr), C.c_void_p(stream_ptr or 0)))

    # ---- radiance queries with no host wait (include/crt_hip.h: crt_shoot_rays*_enqueue)
    @staticmethod
    def _level_cap(level_cap, max_depth):
        """None, or the capacities as the uint32 array of max_depth + 1 entries the call reads ([0] is ignored)"""
        if level_cap is None:
            return None
        caps = np.ascontiguousarray(level_cap, dtype=np.uint32)
        if caps.shape != (max_depth + 1,):
            raise ValueError("level_cap: expected %d entries (levels 0 .. max_depth), got shape %r" % (max_depth + 1, caps.shape))
        return caps

    def shoot_rays_enqueue(self, d_rays_ptr, n, d_rgb_ptr, ray_type=RAY_REFLECTION, max_depth=5, shadow_bias=1e-4, reflection_bias=1e-4,
                           refraction_bias=1e-4, level_cap=None, d_report_ptr=None, stream_ptr=None):
        """shoot_rays_device's colours from a call that only enqueues on the stream -- no wait, so it can be captured into a graph.
        level_cap: rays each level may hold (max_depth + 1 entries), or None for what the context's level arrays hold now (size them
        with one shoot_rays_device call); d_report_ptr: device memory for a ShootReport, or None.  A child that does not fit is the
        background, and the report says so (overflow, dropped)."""
        self._single("shoot_rays_enqueue")
        o = make_options(max_depth, shadow_bias, reflection_bias, refraction_bias)
        caps = self._level_cap(level_cap, max_depth)
        self._check(lib().crt_shoot_rays_enqueue(self.ctx, C.c_void_p(d_rays_ptr), n, ray_type, C.byref(o), C.c_void_p(d_rgb_ptr),
                                                 _p(caps) if caps is not None else None, C.c_void_p(d_report_ptr or 0),
                                                 C.c_void_p(stream_ptr or 0)))

    def shoot_rays_gi_enqueue(self, d_rays_ptr, n, d_rgb_ptr, d_keys_ptr=None, ray_type=RAY_REFLECTION, options=None, level_cap=None,
                              d_report_ptr=None, stream_ptr=None, **option_fields):
        """shoot_rays_gi_device's colours from a call that only enqueues (see shoot_rays_enqueue)."""
        self._single("shoot_rays_gi_enqueue")
        o = self._gi_options(options, option_fields)
        caps = self._level_cap(level_cap, o.max_depth)
        self._check(lib().crt_shoot_rays_gi_enqueue(self.ctx, C.c_void_p(d_rays_ptr), C.c_void_p(d_keys_ptr or 0), n, ray_type, C.byref(o),
                                                    C.c_void_p(d_rgb_ptr), _p(caps) if caps is not None else None,
                                                    C.c_void_p(d_report_ptr or 0), C.c_void_p(stream_ptr or 0)))

    def shoot_report(self) -> ShootReport:
        """The report of the last shoot_rays*_enqueue call outside a capture (waits for it)."""
        self._single("shoot_report")
        r = ShootReport()
        self._check(lib().crt_get_shoot_report(self.ctx, C.byref(r)))
        return r

    def query_scratch_generation(self) -> int:
        """Changes whenever a query scratch array is reallocated: a graph captured from an enqueue call is valid while it stays."""
        self._single("query_scratch_generation")
        return int(lib().crt_query_scratch_generation(self.ctx))

    # ---- progressive GI frames (include/crt_hip.h: crt_camera_sample_rays_device, crt_accumulate_samples_device, crt_render_progressive)
    def camera_sample_rays_device(self, gi_seed, sample, d_rays_ptr, n=None, d_keys_ptr=None, d_pixels_ptr=None, stream_ptr=None):
        """The rays (float32 [n, 6]) and keys (uint32 [n], or None) of sample `sample` of the pixels listed in d_pixels_ptr (uint32 [n],
        row-major indices) or, without a list, of every pixel of the frame (n = H * W): sample 0 through the pixel centre, the others
        jittered by the key's numbers.  Enqueues on the stream and returns."""
        self._single("camera_sample_rays_device")
        n = self.width * self.height if n is None else n
        self._check(lib().crt_camera_sample_rays_device(self.ctx, int(gi_seed), int(sample), C.c_void_p(d_pixels_ptr or 0), n,
                                                        C.c_void_p(d_rays_ptr), C.c_void_p(d_keys_ptr or 0), C.c_void_p(stream_ptr or 0)))

    def accumulate_samples_device(self, d_rgb_ptr, sample, d_sum_ptr, d_mean_ptr=None, n=None, d_pixels_ptr=None, stream_ptr=None):
        """One step of the frame's fold: sum[p] = (0 if sample == 0 else sum[p]) + rgb[i], mean[p] = sum[p] * (1 / (sample + 1)) for the
        listed pixels (distinct!) or all of them; sum and mean are float32 [H * W * 3] device arrays of the caller's.  Enqueues and returns."""
        self._single("accumulate_samples_device")
        n = self.width * self.height if n is None else n
        self._check(lib().crt_accumulate_samples_device(self.ctx, C.c_void_p(d_rgb_ptr), C.c_void_p(d_pixels_ptr or 0), n, int(sample),
                                                        C.c_void_p(d_sum_ptr), C.c_void_p(d_mean_ptr or 0), C.c_void_p(stream_ptr or 0)))

    def progressive_samples(self) -> int:
        """Samples folded into the context's progressive frame so far (0 after set_camera or a render)."""
        self._single("progressive_samples")
        return int(lib().crt_progressive_samples(self.ctx))

    def render_progressive(self, options, samples, per_call=1, on_pass=None, first_sample=0):
        """The GI frame of `options` (use_gi set; rays_per_pixel is not read) with `samples` rays per pixel, per_call samples a call: every
        pixel of the frame, bit for bit the one-shot frame when the last call is in.  on_pass(samples_done, mean) is called after every
        call with the frame so far (float32 [H, W, 3], the caller's to keep) and may return False to stop.  first_sample > 0 continues
        the context's frame (it must equal progressive_samples()).  Returns the last mean."""
        self._single("render_progressive")
        if per_call < 1:
            raise ValueError("per_call: at least one sample a call")
        rgb = np.zeros((self.height, self.width, 3), dtype=np.float32)
        done = int(first_sample)
        while done < samples:
            k = min(int(per_call), samples - done)
            self._check(lib().crt_render_progressive(self.ctx, C.byref(options), done, k, _p(rgb)))
            done += k
            if on_pass is not None and on_pass(done, rgb.copy()) is False:
                break
        return rgb

    # ---- adaptive sampling (include/crt_hip.h: crt_adaptive_step_device, crt_render_adaptive, crt_progressive_active)
    @staticmethod
    def adaptive_work_bytes(n) -> int:
        """Bytes of the work area adaptive_step_device needs for a list of n entries."""
        return int(lib().crt_adaptive_work_bytes(int(n)))

    def adaptive_step_device(self, d_rgb_ptr, sample, adaptive, d_sum_ptr, d_sq_ptr, d_counts_ptr, d_next_pixels_ptr, d_next_n_ptr, d_work_ptr,
                             d_mean_ptr=None, n=None, d_pixels_ptr=None, stream_ptr=None):
        """One step of the fold and of the stopping rule for the listed pixels (distinct!) or all of them, and the next pass's list: sum
        and mean float32 [H * W * 3], sq float32 [H * W], counts uint32 [H * W], next_pixels uint32 [>= n] (the kept pixels in the order
        they had), next_n uint32 [1], work adaptive_work_bytes(n) bytes -- device arrays of the caller's.  Enqueues and returns."""
        self._single("adaptive_step_device")
        n = self.width * self.height if n is None else n
        self._check(lib().crt_adaptive_step_device(self.ctx, C.c_void_p(d_rgb_ptr), C.c_void_p(d_pixels_ptr or 0), n, int(sample), C.byref(adaptive),
                                                   C.c_void_p(d_sum_ptr), C.c_void_p(d_sq_ptr), C.c_void_p(d_mean_ptr or 0), C.c_void_p(d_counts_ptr),
                                                   C.c_void_p(d_next_pixels_ptr), C.c_void_p(d_next_n_ptr), C.c_void_p(d_work_ptr),
                                                   C.c_void_p(stream_ptr or 0)))

    def progressive_active(self) -> int:
        """Pixels the next pass of the context's progressive or adaptive frame would shoot (0: the frame is done, or none is under way)."""
        self._single("progressive_active")
        return int(lib().crt_progressive_active(self.ctx))

    def render_adaptive(self, options, adaptive, per_call=1, on_pass=None, split=False):
        """The GI frame of `options` (use_gi set; rays_per_pixel is not read) sampled adaptively: every pixel is shot until the rule of
        `adaptive` (make_adaptive) stops it, at most adaptive.max_samples times, per_call passes a call.  on_pass(passes_done, mean, counts)
        is called after every call and may return False to stop.  Returns (rgb float32 [H, W, 3], counts uint32 [H, W]): a pixel with
        count k holds the one-shot frame of rays_per_pixel = k.  split: the same frame, bit for bit, that also keeps every sample's
        direct part, for render_denoised(split=True) and render_accumulated(split=True)."""
        self._single("render_adaptive")
        call = lib().crt_render_adaptive_split if split else lib().crt_render_adaptive
        if per_call < 1:
            raise ValueError("per_call: at least one pass a call")
        rgb = np.zeros((self.height, self.width, 3), dtype=np.float32)
        counts = np.zeros((self.height, self.width), dtype=np.uint32)
        done = 0
        while done == 0 or (done < adaptive.max_samples and self.progressive_active()):
            k = min(int(per_call), adaptive.max_samples - done)
            self._check(call(self.ctx, C.byref(options), C.byref(adaptive), done, k, _p(rgb), _p(counts)))
            done += k
            if on_pass is not None and on_pass(done, rgb.copy(), counts.copy()) is False:
                break
        return rgb, counts

    # ---- denoising (include/crt_hip.h: crt_sample_variance_device, crt_denoise_device, crt_render_denoised)
    @staticmethod
    def denoise_work_bytes(width, height) -> int:
        """Bytes of the work area denoise_device needs for a width x height image."""
        return int(lib().crt_denoise_work_bytes(int(width), int(height)))

    def sample_variance_device(self, d_sum_ptr, d_sq_ptr, d_counts_ptr, n_pixels, d_mean_ptr, d_var_ptr, stream_ptr=None):
        """The mean and the variance of the mean of the adaptive fold's state: sum float32 [n * 3], sq float32 [n], counts uint32 [n] ->
        mean float32 [n * 3], var float32 [n]; device arrays of the caller's.  Enqueues and returns."""
        self._single("sample_variance_device")
        self._check(lib().crt_sample_variance_device(self.ctx, C.c_void_p(d_sum_ptr), C.c_void_p(d_sq_ptr), C.c_void_p(d_counts_ptr), int(n_pixels),
                                                     C.c_void_p(d_mean_ptr), C.c_void_p(d_var_ptr), C.c_void_p(stream_ptr or 0)))

    def denoise_device(self, denoise, width, height, d_rgb_ptr, d_var_ptr, d_hits_ptr, d_out_rgb_ptr, d_work_ptr, d_out_var_ptr=None,
                       stream_ptr=None):
        """The a-trous filter on a width x height image of the caller's: rgb float32 [H * W * 3], var float32 [H * W], hits uint8 [H * W, 48]
        (crt_hit records, e.g. trace_rays_device's) -> out_rgb (may be rgb), out_var (or None); work denoise_work_bytes(width, height)
        bytes, 16-byte aligned.  Enqueues and returns."""
        self._single("denoise_device")
        self._check(lib().crt_denoise_device(self.ctx, C.byref(denoise), int(width), int(height), C.c_void_p(d_rgb_ptr), C.c_void_p(d_var_ptr),
                                             C.c_void_p(d_hits_ptr), C.c_void_p(d_out_rgb_ptr), C.c_void_p(d_out_var_ptr or 0),
                                             C.c_void_p(d_work_ptr), C.c_void_p(stream_ptr or 0)))

    def render_denoised(self, denoise=None, rgb8=False, split=False):
        """The context's adaptive frame, under way or finished (render_adaptive), denoised with `denoise` (make_denoise; None: the
        defaults) -> rgb float32 [H, W, 3]; with rgb8 also the PPMColor quantisation, (rgb, uint8 [H, W, 3]).  The frame itself is left
        exactly as it was and can be continued.  split (a frame of render_adaptive(split=True)): only the indirect light is filtered, and
        the direct light, which carries the texels, is added back untouched."""
        self._single("render_denoised")
        d = denoise if denoise is not None else make_denoise()
        rgb = np.zeros((self.height, self.width, 3), dtype=np.float32)
        q8 = np.zeros((self.height, self.width, 3), dtype=np.uint8) if rgb8 else None
        call = lib().crt_render_denoised_split if split else lib().crt_render_denoised
        self._check(call(self.ctx, C.byref(d), _p(rgb), _p(q8) if rgb8 else None))
        return (rgb, q8) if rgb8 else rgb

    # ---- temporal accumulation (include/crt_hip.h: crt_temporal_device, crt_render_accumulated, crt_history_reset, crt_history_frames)
    def temporal_device(self, temporal, width, height, prev_pose, d_prev_ptr, d_sum_ptr, d_sq_ptr, d_counts_ptr, d_hits_ptr, d_next_ptr, d_out_rgb_ptr,
                        d_out_var_ptr=None, d_out_valid_ptr=None, stream_ptr=None):
        """The previous frame's history (prev uint8 [H * W, 64], crt_history_pixel records, with its pose: make_pose; or None and None)
        reprojected and merged with the fold's state sum float32 [H * W * 3], sq float32 [H * W], counts uint32 [H * W] under the guides of
        hits uint8 [H * W, 48] -> next uint8 [H * W, 64], out_rgb float32 [H * W * 3], out_var float32 [H * W] (or None), out_valid uint8
        [H * W] (or None); device arrays of the caller's, prev and next aligned to 16 bytes.  Enqueues and returns."""
        self._single("temporal_device")
        self._check(lib().crt_temporal_device(self.ctx, C.byref(temporal), int(width), int(height), C.byref(prev_pose) if prev_pose is not None else None,
                                              C.c_void_p(d_prev_ptr or 0), C.c_void_p(d_sum_ptr), C.c_void_p(d_sq_ptr), C.c_void_p(d_counts_ptr),
                                              C.c_void_p(d_hits_ptr), C.c_void_p(d_next_ptr), C.c_void_p(d_out_rgb_ptr), C.c_void_p(d_out_var_ptr or 0),
                                              C.c_void_p(d_out_valid_ptr or 0), C.c_void_p(stream_ptr or 0)))

    def render_accumulated(self, temporal=None, denoise=None, rgb8=False, valid=False, split=False):
        """The context's adaptive frame, under way or finished (render_adaptive), merged with the last frame's history with `temporal`
        (make_temporal; None: the defaults) and then filtered with `denoise` (make_denoise; None: no spatial filter) -> rgb float32
        [H, W, 3]; with rgb8 also the PPMColor quantisation uint8 [H, W, 3], with valid also the valid taps per pixel uint8 [H, W], as a
        tuple in that order.  The frame itself is left exactly as it was and can be continued; the history survives set_camera.  Give
        consecutive frames different gi_seed values.  split (a frame of render_adaptive(split=True)): only the indirect light is merged and
        filtered, in a history of its own (history_frames(split=True))."""
        self._single("render_accumulated")
        call = lib().crt_render_accumulated_split if split else lib().crt_render_accumulated
        t = temporal if temporal is not None else make_temporal()
        rgb = np.zeros((self.height, self.width, 3), dtype=np.float32)
        q8 = np.zeros((self.height, self.width, 3), dtype=np.uint8) if rgb8 else None
        taps = np.zeros((self.height, self.width), dtype=np.uint8) if valid else None
        self._check(call(self.ctx, C.byref(t), C.byref(denoise) if denoise is not None else None, _p(rgb), _p(q8) if rgb8 else None,
                         _p(taps) if valid else None))
        out = (rgb,) + ((q8,) if rgb8 else ()) + ((taps,) if valid else ())
        return out if len(out) > 1 else rgb

    def history_reset(self):
        """Drops the accumulated history: the next render_accumulated is a first frame again."""
        self._single("history_reset")
        self._check(lib().crt_history_reset(self.ctx))

    def history_frames(self, split=False) -> int:
        """The frames merged into the history (split: into the split calls' history) since the last history_reset."""
        self._single("history_frames")
        return int((lib().crt_history_frames_split if split else lib().crt_history_frames)(self.ctx))

    # ---- lightmap baking (include/crt_hip.h: crt_bake_texels_device, crt_bake_dilate_device, crt_bake_lightmap, crt_get_bake_stats)
    @staticmethod
    def bake_work_bytes(width, height) -> int:
        return int(lib().crt_bake_work_bytes(int(width), int(height)))

    def bake_texels_device(self, bake, d_texels_ptr, d_rays_ptr, d_work_ptr, stream_ptr=None):
        """The records of every texel of the bake's map -> texels uint8 [H * W, 48] (BAKE_TEXEL_DTYPE, aligned to 16 bytes) and the probe
        rays of the covered ones -> rays float32 [H * W, 6] (an empty texel's ray is not written); work: bake_work_bytes(W, H) bytes,
        aligned to 16.  Enqueues and returns (the first call for a mesh reads the scene's trees back once)."""
        self._single("bake_texels_device")
        self._check(lib().crt_bake_texels_device(self.ctx, C.byref(bake), C.c_void_p(d_texels_ptr), C.c_void_p(d_rays_ptr), C.c_void_p(d_work_ptr),
                                                 C.c_void_p(stream_ptr or 0)))

    def bake_dilate_device(self, width, height, passes, d_rgb_ptr, d_status_ptr, d_work_ptr, stream_ptr=None):
        """`passes` dilation passes on rgb float32 [H * W * 3] and status uint8 [H * W], in place; work: bake_work_bytes(W, H) bytes, aligned
        to 16.  Enqueues and returns."""
        self._single("bake_dilate_device")
        self._check(lib().crt_bake_dilate_device(self.ctx, int(width), int(height), int(passes), C.c_void_p(d_rgb_ptr), C.c_void_p(d_status_ptr),
                                                 C.c_void_p(d_work_ptr), C.c_void_p(stream_ptr or 0)))

    def bake_lightmap(self, mesh, width, height, options=None, samples=1, dilate=2, probe_offset=1e-3, check_probes=False, rgb8=False):
        """The lightmap of `mesh`'s UV layout, width x height texels, row 0 the top: every covered texel is what shootRay returns for its
        probe ray (options: make_options; None: the defaults; with use_gi the mean of `samples` GI samples), the texels beside a chart are
        filled by `dilate` dilation passes -> (rgb float32 [H, W, 3], status uint8 [H, W] of BAKE_EMPTY / BAKE_COVERED / BAKE_DILATED,
        texels BAKE_TEXEL_DTYPE [H, W]); with rgb8 the PPMColor quantisation uint8 [H, W, 3] as a fourth.  bake_stats() describes the call."""
        self._single("bake_lightmap")
        b = make_bake(mesh=int(mesh), width=int(width), height=int(height), samples=int(samples), dilate=int(dilate), check_probes=int(bool(check_probes)),
                      probe_offset=float(probe_offset))
        o = options if options is not None else make_options()
        shape = (max(int(height), 0), max(int(width), 0))
        rgb = np.zeros(shape + (3,), dtype=np.float32)
        status = np.zeros(shape, dtype=np.uint8)
        texels = np.zeros(shape, dtype=BAKE_TEXEL_DTYPE)
        q8 = np.zeros(shape + (3,), dtype=np.uint8) if rgb8 else None
        self._check(lib().crt_bake_lightmap(self.ctx, C.byref(b), C.byref(o), _p(rgb), _p(q8) if rgb8 else None, _p(status), _p(texels)))
        return (rgb, status, texels) + ((q8,) if rgb8 else ())

    def bake_stats(self) -> BakeStats:
        self._single("bake_stats")
        st = BakeStats()
        self._check(lib().crt_get_bake_stats(self.ctx, C.byref(st)))
        return st

    # ---- irradiance probes (include/crt_hip.h: "Irradiance probes")
    def probe_rays_device(self, volume, first, count, d_rays_ptr, d_keys_ptr=None, stream_ptr=None):
        """The rays of the probes [first, first + count) of the volume -> rays float32 [count * rays, 6] (aligned to 16 bytes) and, unless
        d_keys_ptr is None, their GI keys uint32 [count * rays].  Enqueues and returns."""
        self._single("probe_rays_device")
        self._check(lib().crt_probe_rays_device(self.ctx, C.byref(volume), int(first), int(count), C.c_void_p(d_rays_ptr), C.c_void_p(d_keys_ptr or 0),
                                                C.c_void_p(stream_ptr or 0)))

    def probe_project_device(self, d_rays_ptr, d_rgb_ptr, count, rays, d_probes_ptr, stream_ptr=None):
        """The SH9 records of `count` probes of `rays` rays each from rays float32 [count * rays, 6] and their colours float32
        [count * rays, 3] -> probes uint8 [count, 128] (PROBE_DTYPE, aligned to 16 bytes).  Enqueues and returns."""
        self._single("probe_project_device")
        self._check(lib().crt_probe_project_device(self.ctx, C.c_void_p(d_rays_ptr), C.c_void_p(d_rgb_ptr), int(count), int(rays), C.c_void_p(d_probes_ptr),
                                                   C.c_void_p(stream_ptr or 0)))

    def probe_validity_device(self, d_rays_ptr, d_hits_ptr, count, rays, backface_limit, d_probes_ptr, stream_ptr=None):
        """back, miss and state of `count` records from the rays and the hits uint8 [count * rays, 48] trace_rays_device wrote for them.
        Enqueues and returns."""
        self._single("probe_validity_device")
        self._check(lib().crt_probe_validity_device(self.ctx, C.c_void_p(d_rays_ptr), C.c_void_p(d_hits_ptr), int(count), int(rays), float(backface_limit),
                                                    C.c_void_p(d_probes_ptr), C.c_void_p(stream_ptr or 0)))

    def probe_irradiance_device(self, volume, d_probes_ptr, d_points_ptr, d_normals_ptr, n, d_rgb_ptr, d_status_ptr=None, stream_ptr=None):
        """The lookup at n points in the volume's records: points, normals float32 [n, 3] -> rgb float32 [n, 3], status uint8 [n] (the
        corners used, 0: no light) or None.  Enqueues and returns."""
        self._single("probe_irradiance_device")
        self._check(lib().crt_probe_irradiance_device(self.ctx, C.byref(volume), C.c_void_p(d_probes_ptr), C.c_void_p(d_points_ptr), C.c_void_p(d_normals_ptr),
                                                      int(n), C.c_void_p(d_rgb_ptr), C.c_void_p(d_status_ptr or 0), C.c_void_p(stream_ptr or 0)))

    def bake_probes(self, volume, options=None, d_probes_ptr=None):
        """The volume's probes (make_probe_volume), each the SH9 projection of what shootRay returns for its rays (options: make_options;
        None: the defaults; with use_gi the GI mode under the volume's gi_seed) -> PROBE_DTYPE [nz, ny, nx]; d_probes_ptr: device memory
        that takes the records too.  probe_stats() describes the call."""
        self._single("bake_probes")
        o = options if options is not None else make_options()
        out = np.zeros((max(int(volume.nz), 0), max(int(volume.ny), 0), max(int(volume.nx), 0)), dtype=PROBE_DTYPE)
        self._check(lib().crt_bake_probes(self.ctx, C.byref(volume), C.byref(o), _p(out) if out.size else None, C.c_void_p(d_probes_ptr or 0)))
        return out

    def probe_irradiance(self, volume, probes, points, normals):
        """The diffuse light a white Lambertian surface shows at points float32 [n, 3] with normals float32 [n, 3] (used as given) in the
        volume's records `probes` (as bake_probes returns them) -> (rgb float32 [n, 3], status uint8 [n]: the corners used, 0: no light)."""
        self._single("probe_irradiance")
        probes = np.ascontiguousarray(probes, dtype=PROBE_DTYPE).reshape(-1)
        points = np.ascontiguousarray(points, dtype=np.float32)
        normals = np.ascontiguousarray(normals, dtype=np.float32)
        if points.ndim != 2 or points.shape[1] != 3 or normals.shape != points.shape:
            raise ValueError("points, normals: expected two arrays of shape [n, 3], got %r and %r" % (points.shape, normals.shape))
        if len(probes) != int(volume.nx) * int(volume.ny) * int(volume.nz):
            raise ValueError("probes: expected %d x %d x %d records, got %d" % (volume.nz, volume.ny, volume.nx, len(probes)))
        rgb = np.zeros((len(points), 3), dtype=np.float32)
        status = np.zeros(len(points), dtype=np.uint8)
        self._check(lib().crt_probe_irradiance(self.ctx, C.byref(volume), _p(probes), _p(points), _p(normals), len(points), _p(rgb), _p(status)))
        return rgb, status

    # ---- probe visibility (include/crt_hip.h: "Probe visibility")
    def probe_depth_device(self, d_rays_ptr, d_hits_ptr, count, rays, max_distance, d_depth_ptr, stream_ptr=None):
        """The depth records of `count` probes of `rays` rays each from rays float32 [count * rays, 6] and the hits uint8 [count * rays, 48]
        trace_rays_device wrote for them -> depth uint8 [count, 512] (PROBE_DEPTH_DTYPE, aligned to 16 bytes).  Enqueues and returns."""
        self._single("probe_depth_device")
        self._check(lib().crt_probe_depth_device(self.ctx, C.c_void_p(d_rays_ptr), C.c_void_p(d_hits_ptr), int(count), int(rays), float(max_distance),
                                                 C.c_void_p(d_depth_ptr), C.c_void_p(stream_ptr or 0)))

    def probe_irradiance_visible_device(self, volume, visibility, d_probes_ptr, d_depth_ptr, d_points_ptr, d_normals_ptr, n, d_rgb_ptr, d_status_ptr=None,
                                        stream_ptr=None):
        """probe_irradiance_device with every corner weighted by the Chebyshev bound of its depth record (visibility: make_probe_visibility).
        Enqueues and returns."""
        self._single("probe_irradiance_visible_device")
        self._check(lib().crt_probe_irradiance_visible_device(self.ctx, C.byref(volume), C.byref(visibility), C.c_void_p(d_probes_ptr), C.c_void_p(d_depth_ptr),
                                                              C.c_void_p(d_points_ptr), C.c_void_p(d_normals_ptr), int(n), C.c_void_p(d_rgb_ptr),
                                                              C.c_void_p(d_status_ptr or 0), C.c_void_p(stream_ptr or 0)))

    def bake_probes_visible(self, volume, visibility=None, options=None, d_probes_ptr=None, d_depth_ptr=None):
        """bake_probes with the depth pass -> (PROBE_DTYPE [nz, ny, nx], PROBE_DEPTH_DTYPE [nz, ny, nx]); visibility: make_probe_visibility
        (None: the volume's defaults); d_probes_ptr, d_depth_ptr: device memory that takes the records too.  probe_stats() describes the call."""
        self._single("bake_probes_visible")
        o = options if options is not None else make_options()
        vis = visibility if visibility is not None else make_probe_visibility(volume)
        shape = (max(int(volume.nz), 0), max(int(volume.ny), 0), max(int(volume.nx), 0))
        out, depth = np.zeros(shape, dtype=PROBE_DTYPE), np.zeros(shape, dtype=PROBE_DEPTH_DTYPE)
        self._check(lib().crt_bake_probes_visible(self.ctx, C.byref(volume), C.byref(vis), C.byref(o), _p(out) if out.size else None,
                                                  C.c_void_p(d_probes_ptr or 0), _p(depth) if depth.size else None, C.c_void_p(d_depth_ptr or 0)))
        return out, depth

    def probe_irradiance_visible(self, volume, visibility, probes, depth, points, normals):
        """probe_irradiance with the visibility term: `depth` are the volume's depth records as bake_probes_visible returns them
        -> (rgb float32 [n, 3], status uint8 [n])."""
        self._single("probe_irradiance_visible")
        probes = np.ascontiguousarray(probes, dtype=PROBE_DTYPE).reshape(-1)
        depth = np.asarray(depth)
        if depth.dtype != PROBE_DEPTH_DTYPE:                               # the moments themselves, float32 [..., 64, 2]
            depth = np.ascontiguousarray(depth, dtype=np.float32).reshape(-1, 128).view(PROBE_DEPTH_DTYPE)
        depth = np.ascontiguousarray(depth).reshape(-1)
        points = np.ascontiguousarray(points, dtype=np.float32)
        normals = np.ascontiguousarray(normals, dtype=np.float32)
        if points.ndim != 2 or points.shape[1] != 3 or normals.shape != points.shape:
            raise ValueError("points, normals: expected two arrays of shape [n, 3], got %r and %r" % (points.shape, normals.shape))
        total = int(volume.nx) * int(volume.ny) * int(volume.nz)
        if len(probes) != total or len(depth) != total:
            raise ValueError("probes, depth: expected %d x %d x %d records each, got %d and %d" % (volume.nz, volume.ny, volume.nx, len(probes), len(depth)))
        rgb = np.zeros((len(points), 3), dtype=np.float32)
        status = np.zeros(len(points), dtype=np.uint8)
        self._check(lib().crt_probe_irradiance_visible(self.ctx, C.byref(volume), C.byref(visibility), _p(probes), _p(depth), _p(points), _p(normals),
                                                       len(points), _p(rgb), _p(status)))
        return rgb, status

    # ---- probe-lit radiance (include/crt_hip.h: "Probe-lit radiance"): diffuse hits take their bounce light from a probe volume
    @staticmethod
    def _vis_ref(visibility):
        return C.byref(visibility) if visibility is not None else None

    def probe_light_hits_device(self, volume, visibility, d_probes_ptr, d_depth_ptr, d_hits_ptr, d_status_ptr, n, gi_sample_size, d_rgb_ptr,
                                d_counts_ptr=None, stream_ptr=None):
        """For each of n records whose status byte is SHADE_DIFFUSE: rgb = (rgb + S * Lbar) * (1 / (S + 1)), Lbar the zonal lookup of the
        record's point and normal in the volume (visibility None: the plain lookup; otherwise the Chebyshev-weighted one, with depth records).
        hits uint8 [n, 48], status uint8 [n], rgb float32 [n, 3] in place, counts uint64 [2] or None ([0] += lit, [1] += unlit).  Enqueues
        and returns."""
        self._single("probe_light_hits_device")
        self._check(lib().crt_probe_light_hits_device(self.ctx, C.byref(volume), self._vis_ref(visibility), C.c_void_p(d_probes_ptr),
                                                      C.c_void_p(d_depth_ptr or 0), C.c_void_p(d_hits_ptr), C.c_void_p(d_status_ptr), int(n),
                                                      int(gi_sample_size), C.c_void_p(d_rgb_ptr), C.c_void_p(d_counts_ptr or 0), C.c_void_p(stream_ptr or 0)))

    @staticmethod
    def _probe_records(volume, probes, depth, need_depth):
        probes = np.ascontiguousarray(probes, dtype=PROBE_DTYPE).reshape(-1)
        total = int(volume.nx) * int(volume.ny) * int(volume.nz)
        if len(probes) != total:
            raise ValueError("probes: expected %d x %d x %d records, got %d" % (volume.nz, volume.ny, volume.nx, len(probes)))
        if not need_depth:
            return probes, None
        depth = np.asarray(depth)
        if depth.dtype != PROBE_DEPTH_DTYPE:                               # the moments themselves, float32 [..., 64, 2]
            depth = np.ascontiguousarray(depth, dtype=np.float32).reshape(-1, 128).view(PROBE_DEPTH_DTYPE)
        depth = np.ascontiguousarray(depth).reshape(-1)
        if len(depth) != total:
            raise ValueError("depth: expected %d x %d x %d records, got %d" % (volume.nz, volume.ny, volume.nx, len(depth)))
        return probes, depth

    def shoot_rays_lit(self, rays, volume, probes, visibility=None, depth=None, ray_type=RAY_REFLECTION, options=None, **option_fields):
        """The GI build's colours with the probe volume in place of the sample rays: rays float32 [n, 6], probes (and, with a visibility,
        depth) the volume's records as bake_probes / bake_probes_visible return them -> float32 [n, 3].  options: an Options with use_gi set
        (its gi_sample_size is the rule's S), or make_options' fields by name."""
        self._single("shoot_rays_lit")
        rays = self._rays_array(rays)
        if visibility is not None and depth is None:
            raise ValueError("shoot_rays_lit: a visibility needs the volume's depth records")
        probes, depth = self._probe_records(volume, probes, depth, visibility is not None)
        rgb = np.zeros((len(rays), 3), dtype=np.float32)
        o = self._gi_options(options, option_fields)
        self._check(lib().crt_shoot_rays_lit(self.ctx, _p(rays), len(rays), ray_type, C.byref(o), C.byref(volume), self._vis_ref(visibility), _p(probes),
                                             _p(depth) if depth is not None else None, _p(rgb)))
        return rgb

    def shoot_rays_lit_device(self, d_rays_ptr, n, d_rgb_ptr, volume, d_probes_ptr, visibility=None, d_depth_ptr=None, ray_type=RAY_REFLECTION,
                              options=None, stream_ptr=None, **option_fields):
        """The same on device memory (data_ptr() of: rays float32 [n, 6], rgb float32 [n, 3], probes uint8 [count, 128], depth uint8
        [count, 512]) on the stream; the call waits for the stream once per recursion level, so it cannot be captured into a graph."""
        self._single("shoot_rays_lit_device")
        o = self._gi_options(options, option_fields)
        self._check(lib().crt_shoot_rays_lit_device(self.ctx, C.c_void_p(d_rays_ptr), int(n), ray_type, C.byref(o), C.byref(volume),
                                                    self._vis_ref(visibility), C.c_void_p(d_probes_ptr), C.c_void_p(d_depth_ptr or 0),
                                                    C.c_void_p(d_rgb_ptr), C.c_void_p(stream_ptr or 0)))

    def render_probe_lit(self, volume, d_probes_ptr, visibility=None, d_depth_ptr=None, options=None, quantized=False, **option_fields):
        """The probe-lit frame: the camera's rays of every pixel through shoot_rays_lit_device -> float32 [H, W, 3], or, quantized=True,
        (that, uint8 [H, W, 3] from the quantiser).  d_probes_ptr and d_depth_ptr are device memory."""
        self._single("render_probe_lit")
        o = self._gi_options(options, option_fields)
        rgb = np.zeros((self.height, self.width, 3), dtype=np.float32)
        rgb8 = np.zeros((self.height, self.width, 3), dtype=np.uint8) if quantized else None
        self._check(lib().crt_render_probe_lit(self.ctx, C.byref(volume), self._vis_ref(visibility), C.c_void_p(d_probes_ptr), C.c_void_p(d_depth_ptr or 0),
                                               C.byref(o), _p(rgb), _p(rgb8) if quantized else None))
        return (rgb, rgb8) if quantized else rgb

    def probe_lit_stats(self) -> ProbeLitStats:
        """lit / unlit: the DIFFUSE records of the last probe-lit query or frame, over all its levels (waits for it)."""
        self._single("probe_lit_stats")
        st = ProbeLitStats()
        self._check(lib().crt_get_probe_lit_stats(self.ctx, C.byref(st)))
        return st

    def probe_stats(self) -> ProbeStats:
        self._single("probe_stats")
        st = ProbeStats()
        self._check(lib().crt_get_probe_stats(self.ctx, C.byref(st)))
        return st

    def set_probe_chunk(self, probes=0):
        """Test hook (libcrt_hip_test.so): bake_probes takes `probes` probes per chunk from now on; 0 restores the default."""
        self._single("set_probe_chunk")
        L = lib()
        L.crt_debug_set_probe_chunk.argtypes = [C.c_void_p, C.c_uint32]
        self._check(L.crt_debug_set_probe_chunk(self.ctx, int(probes)))

    # ---- chain guides (include/crt_hip.h: crt_guide_rays*, crt_set_guide_bounces): filter guides that follow mirrors and glass
    def guide_work_bytes(self, n) -> int:
        return int(lib().crt_guide_work_bytes(int(n)))

    def guide_rays(self, rays, ray_type=RAY_PRIMARY, max_bounces=4, reflection_bias=1e-4, refraction_bias=1e-4):
        """The chain guide of each ray: the record of the first diffuse or constant surface it reaches through mirrors and glass, with
        the path length as t and a tagged mesh; rays float32 [n, 6] (used as given) -> (records HIT_DTYPE [n], status uint8 [n]: bits 0-5
        the bounces, bit 7 cut at max_bounces, last_rays float32 [n, 6]: the terminal segment's ray)."""
        self._single("guide_rays")
        rays = self._rays_array(rays)
        hits = np.zeros(len(rays), dtype=HIT_DTYPE)
        status = np.zeros(len(rays), dtype=np.uint8)
        last = np.zeros((len(rays), 6), dtype=np.float32)
        o = make_options(0, 1e-4, reflection_bias, refraction_bias)
        self._check(lib().crt_guide_rays(self.ctx, _p(rays), len(rays), ray_type, C.byref(o), int(max_bounces), _p(hits), _p(status), _p(last)))
        return hits, status, last

    def guide_rays_device(self, d_rays_ptr, n, ray_type, max_bounces, d_hits_ptr, d_work_ptr, d_status_ptr=None, d_last_rays_ptr=None,
                          reflection_bias=1e-4, refraction_bias=1e-4, stream_ptr=None):
        """The same on device memory (rays float32 [n, 6], hits uint8 [n, 48], status uint8 [n] or None, last_rays float32 [n, 6] or None,
        work guide_work_bytes(n) bytes, 16-byte aligned).  Enqueues and returns."""
        self._single("guide_rays_device")
        o = make_options(0, 1e-4, reflection_bias, refraction_bias)
        self._check(lib().crt_guide_rays_device(self.ctx, C.c_void_p(d_rays_ptr), int(n), ray_type, C.byref(o), int(max_bounces), C.c_void_p(d_hits_ptr),
                                                C.c_void_p(d_status_ptr or 0), C.c_void_p(d_last_rays_ptr or 0), C.c_void_p(d_work_ptr),
                                                C.c_void_p(stream_ptr or 0)))

    def set_guide_bounces(self, max_bounces):
        """0 (the default): the frame calls filter under first-hit guides.  Above 0: render_denoised's and render_accumulated's spatial
        filter runs under the chain guides of the camera's centre rays; the temporal stage keeps the first hits."""
        self._single("set_guide_bounces")
        self._check(lib().crt_set_guide_bounces(self.ctx, int(max_bounces)))

    def guide_bounces(self) -> int:
        return int(lib().crt_guide_bounces(self.ctx))

    # ---- variance estimate (include/crt_hip.h: crt_variance_estimate_device, crt_set_variance_estimate)
    def variance_estimate_device(self, estimate, width, height, d_moments_ptr, d_hits_ptr, d_var_ptr, d_out_var_ptr, stream_ptr=None):
        """Where a pixel's record stands for fewer than estimate.min_history samples, its variance of the mean is replaced by a 7x7
        cross-bilateral estimate from its neighbours' moments: moments uint8 [H * W, 64] (crt_history_pixel records, e.g. temporal_device's
        next; aligned to 16 bytes), hits uint8 [H * W, 48], var float32 [H * W] -> out_var float32 [H * W] (may be var); device arrays of
        the caller's.  Enqueues and returns."""
        self._single("variance_estimate_device")
        self._check(lib().crt_variance_estimate_device(self.ctx, C.byref(estimate), int(width), int(height), C.c_void_p(d_moments_ptr),
                                                       C.c_void_p(d_hits_ptr), C.c_void_p(d_var_ptr), C.c_void_p(d_out_var_ptr),
                                                       C.c_void_p(stream_ptr or 0)))

    def set_variance_estimate(self, estimate=None):
        """None (the default): off.  A make_variance_estimate(): render_denoised and render_accumulated (with a filter) run the variance
        estimate between the stage that produces colour and variance and the a-trous filter.  Nothing is dropped by changing it."""
        self._single("set_variance_estimate")
        self._check(lib().crt_set_variance_estimate(self.ctx, C.byref(estimate) if estimate is not None else None))

    def variance_estimate(self):
        """The setting: a VarianceEstimate, or None when it is off."""
        self._single("variance_estimate")
        e = VarianceEstimate()
        return e if lib().crt_get_variance_estimate(self.ctx, C.byref(e)) else None

    # ---- split GI frames (include/crt_hip.h: crt_split_fold_device, crt_split_recombine_device)
    def split_fold_device(self, d_rgb_ptr, d_direct_ptr, sample, d_dsum_ptr, d_rsum_ptr, d_rsq_ptr, n=None, d_pixels_ptr=None, stream_ptr=None):
        """One step of the split's fold for the listed pixels (distinct!) or all of them: rgb and direct float32 [n, 3] (shoot_rays_gi_device
        with d_direct_ptr) into dsum and rsum float32 [H * W * 3] and rsq float32 [H * W], device arrays of the caller's.  Enqueues and
        returns."""
        self._single("split_fold_device")
        n = self.width * self.height if n is None else n
        self._check(lib().crt_split_fold_device(self.ctx, C.c_void_p(d_rgb_ptr), C.c_void_p(d_direct_ptr), C.c_void_p(d_pixels_ptr or 0), n, int(sample),
                                                C.c_void_p(d_dsum_ptr), C.c_void_p(d_rsum_ptr), C.c_void_p(d_rsq_ptr), C.c_void_p(stream_ptr or 0)))

    def read_split_state(self):
        """The split frame under way or finished: (dsum float32 [H, W, 3], rsum float32 [H, W, 3], rsq float32 [H, W]) -- the sums of the
        samples' direct parts and the first and second moment of the rest; dsum / counts is the frame's direct-light layer."""
        self._single("read_split_state")
        dsum, rsum = (np.zeros((self.height, self.width, 3), dtype=np.float32) for _ in range(2))
        rsq = np.zeros((self.height, self.width), dtype=np.float32)
        self._check(lib().crt_read_split_state(self.ctx, _p(dsum), _p(rsum), _p(rsq)))
        return dsum, rsum, rsq

    def split_recombine_device(self, d_filtered_ptr, d_dsum_ptr, d_counts_ptr, n_pixels, d_out_ptr, stream_ptr=None):
        """out = filtered + dsum / count (count 0: filtered) for n_pixels pixels: filtered, dsum and out float32 [n * 3], counts uint32 [n],
        device arrays of the caller's; out may be filtered.  Enqueues and returns."""
        self._single("split_recombine_device")
        self._check(lib().crt_split_recombine_device(self.ctx, C.c_void_p(d_filtered_ptr), C.c_void_p(d_dsum_ptr), C.c_void_p(d_counts_ptr),
                                                     int(n_pixels), C.c_void_p(d_out_ptr), C.c_void_p(stream_ptr or 0)))

    def shoot_stats(self) -> ShootStats:
        """rays / levels / level_rays / shadow_records / rerouted / kernel_ms of the last radiance query (waits for it)."""
        self._single("shoot_stats")
        s = ShootStats()
        self._check(lib().crt_get_shoot_stats(self.ctx, C.byref(s)))
        return s

    def query_stats(self) -> QueryStats:
        """rays / hits / rerouted / kernel_ms of the last query call (waits for it)."""
        self._single("query_stats")
        s = QueryStats()
        self._check(lib().crt_get_query_stats(self.ctx, C.byref(s)))
        return s

    def kernels(self):
        """{'level0': ..., 'shadow0': ..., 'levels': ...}: the kernels a production frame runs (names as rocprofv3 prints them; shadow0 is what the last frame ran)."""
        buf = C.create_string_buffer(512)
        L = lib()
        L.crt_describe_kernels.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        self._check(L.crt_describe_kernels(self.ctx, buf, 512))
        return dict(kv.split("=", 1) for kv in buf.value.decode().split(";"))

    def set_filter_stack(self, entries):
        """Test hook (libcrt_hip_test.so): the filter walks may use `entries` stack entries from now on, clamped to [1, built size]."""
        self._single("set_filter_stack")
        L = lib()
        L.crt_debug_set_filter_stack.argtypes = [C.c_void_p, C.c_uint32]
        self._check(L.crt_debug_set_filter_stack(self.ctx, int(entries)))

    def set_query_chunks(self, host_rays=0, launch_rays=0, pass_rays=0):
        """Test hook (libcrt_hip_test.so): the queries' chunk sizes from now on -- rays per round trip of the host variants, per launch,
        per pass of a radiance query; 0 restores a default, other values are clamped to [64, the default]."""
        self._single("set_query_chunks")
        L = lib()
        L.crt_debug_set_query_chunks.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64]
        self._check(L.crt_debug_set_query_chunks(self.ctx, int(host_rays), int(launch_rays), int(pass_rays)))

    def stream_counts(self):
        """Diagnostics: the ray-stream pass's counter block of the last frame (SC_* layout of csrc/kernel_stream.h)."""
        out = (C.c_uint32 * 512)()
        L = lib()
        L.crt_debug_stream_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_uint32]
        self._check(L.crt_debug_stream_counts(self.ctx, out, 512))
        return np.array(out[:], dtype=np.uint32)

    def read_quantized(self):
        out = np.zeros((self.height, self.width, 3), dtype=np.uint8)
        self._check(lib().crt_read_quantized(self.ctx, _p(out)))
        return out


def test_pow5(x, device=0):
    """Device build of the restated glibc powf(x, 5) on a float32 array (unit-test hook)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.empty_like(x)
    L = lib()
    L.crt_test_pow5.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint64]
    rc = L.crt_test_pow5(device, _p(x), _p(out), x.size)
    if rc != CRT_OK:
        raise CrtError(rc, "crt_test_pow5 failed")
    return out


def csrc_sha256():
    """SHA-256 over the kernel sources (csrc/*, sorted by name): profiles/ records it at collection time and bench.py compares it
    with the running tree's, so that counters of other kernels are never passed off as this build's."""
    import hashlib
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
    h = hashlib.sha256()
    for name in sorted(os.listdir(d)):
        if name.endswith((".h", ".hip", ".cpp")):
            h.update(name.encode())
            with open(os.path.join(d, name), "rb") as f:
                h.update(f.read())
    return h.hexdigest()


def device_count():
    return lib().crt_device_count()
