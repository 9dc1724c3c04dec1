"""Loader for librenderbaby_hip.so (the C ABI of include/rb_abi.h).

The product path has no fallback: if the HIP library is missing or fails to
load, importing the engine raises.  ``torch`` is imported first on purpose: its
wheel bundles a HIP runtime with the same SONAME (libamdhip64.so.7), and a
process must not end up with two HIP runtimes if device pointers are to be
shared with torch.distributed (the RCCL gather).
"""
import ctypes as C
import os

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# RB_LIBRARY_PATH: an alternative build of the library (A/B experiments with compile-time knobs)
LIB_PATH = os.environ.get("RB_LIBRARY_PATH") or os.path.join(_HERE, "librenderbaby_hip.so")
_lib = None


# every entry point of include/rb_abi.h the package calls: name -> (restype, argtypes)
P = C.POINTER
vp, u32, i32, sz = C.c_void_p, C.c_uint32, C.c_int, C.c_size_t
SIGNATURES = {
    "rb_create": (vp, [P(abi.Config)]),
    "rb_create_ex": (vp, [P(abi.Config), P(abi.Options)]),
    "rb_create_multi": (vp, [P(abi.Config), P(abi.Options), P(C.c_int32), u32]),
    "rb_comm_unique_id": (i32, [vp]),
    "rb_comm_available": (i32, []),
    "rb_comm_init_rank": (i32, [vp, vp, u32, u32]),
    "rb_comm_info": (i32, [vp, P(u32), P(u32), P(C.c_float)]),
    "rb_destroy": (None, [vp]),
    "rb_update": (i32, [vp, P(abi.Config)]),
    "rb_render": (i32, [vp, vp]),
    "rb_render_config": (i32, [vp, P(abi.Config), vp]),
    "rb_iter_begin": (i32, [vp, P(abi.Config)]),
    "rb_iter_has_next": (i32, [vp]),
    "rb_iter_next": (i32, [vp, vp]),
    "rb_iter_destroy": (None, [vp]),
    "rb_iter_set_passes_per_frame": (i32, [vp, u32]),
    "rb_last_error": (C.c_char_p, [vp]),
    "rb_get_size": (i32, [vp, P(u32), P(u32)]),
    "rb_clear": (i32, [vp]),
    "rb_dispatch": (i32, [vp, u32, u32]),
    "rb_reserve": (i32, [vp, u32]),
    "rb_sync": (i32, [vp]),
    "rb_read_rgba": (i32, [vp, vp]),
    "rb_read_accumulation": (i32, [vp, vp]),
    "rb_device_rgba": (i32, [vp, P(vp), P(sz)]),
    "rb_host_alloc": (vp, [sz]),
    "rb_host_free": (None, [vp]),
    "rb_local_rows": (i32, [vp, P(u32), P(u32)]),
    "rb_global_row": (i32, [vp, u32, P(u32)]),
    "rb_shard_layout": (i32, [u32, u32, u32, u32, P(u32), P(u32)]),
    "rb_shard_global_row": (u32, [u32, u32, u32, u32]),
    "rb_get_stats": (i32, [vp, P(abi.Stats)]),
    "rb_reset_stats": (i32, [vp]),
    "rb_last_dispatch_ms": (i32, [vp, P(C.c_float)]),
    "rb_bvh_build": (i32, [vp, sz, vp, sz, P(sz), vp]),
    "rb_bvh_build_canonical": (i32, [vp, sz, vp, sz, P(sz), vp]),
    "rb_bvh_build_device": (i32, [i32, vp, sz, vp, sz, P(sz), vp]),
    "rb_engine_tree": (i32, [vp, vp, sz, P(sz), vp, sz, P(sz)]),
    "rb_tree_builder": (C.c_char_p, [vp, vp]),
    "rb_debug_chunk_tree": (i32, [vp, sz, vp, sz, vp, sz, vp]),
    "rb_measure_l1_gather": (i32, [i32, C.c_uint64, P(C.c_double)]),
    "rb_debug_math": (i32, [vp, vp, vp, u32]),
    "rb_debug_walk_profile": (i32, [vp, i32]),
    "rb_debug_rcp_exhaustive": (i32, [u32, vp]),
    "rb_debug_rcp_det_exhaustive": (i32, [u32, vp]),
    "rb_debug_rnd_pm1_exhaustive": (i32, [vp]),
    "rb_debug_triangle_trip": (i32, [u32, u32, vp]),
    "rb_debug_triangle_trip_flat": (i32, [u32, u32, vp]),
    "rb_debug_triangle_trip_vec": (i32, [u32, u32, u32, vp]),
    "rb_debug_tri_filter": (i32, [vp, vp, u32, vp, vp]),
    "rb_debug_trace_form": (u32, [vp]),
    "rb_debug_root_box": (i32, [vp, u32, vp, vp]),
    "rb_debug_normalize_sites": (i32, [vp, u32, u32, u32, u32, vp]),
    "rb_measure_salu_mix": (i32, [i32, u32, u32, P(C.c_double)]),
    "rb_debug_div_exhaustive": (i32, [u32, u32, u32, u32, u32, u32, vp]),
    "rb_last_kernel_name": (C.c_char_p, [vp]),
    "rb_cast_rays": (i32, [vp, vp, sz, vp, vp]),
    "rb_render_hits": (i32, [vp, vp, vp]),
    "rb_pick": (i32, [vp, u32, u32, vp, vp]),
    "rb_occluded": (i32, [vp, vp, vp, sz, u32, vp]),
    "rb_occluded_device": (i32, [vp, vp, vp, sz, u32, vp]),
    "rb_cast_rays_device": (i32, [vp, vp, sz, vp, vp]),
    "rb_trace_rays": (i32, [vp, vp, vp, sz, u32, u32, vp]),
    "rb_trace_rays_device": (i32, [vp, vp, vp, sz, u32, u32, vp]),
    "rb_camera_rays": (i32, [i32, vp, C.c_uint64, sz, u32, u32, vp, vp]),
    "rb_trace_camera": (i32, [vp, vp, C.c_uint64, sz, u32, u32, vp]),
    "rb_trace_camera_device": (i32, [vp, vp, C.c_uint64, sz, u32, u32, vp]),
    "rb_last_camera_rays_ms": (i32, [vp, P(C.c_float)]),
    "rb_hemisphere_rays": (i32, [i32, vp, vp, sz, vp, u32, u32, vp, vp]),
    "rb_trace_hemisphere": (i32, [vp, vp, vp, sz, vp, u32, u32, vp]),
    "rb_trace_hemisphere_device": (i32, [vp, vp, vp, sz, vp, u32, u32, vp]),
    "rb_openness_hemisphere": (i32, [vp, vp, vp, sz, vp, u32, u32, vp]),
    "rb_openness_hemisphere_device": (i32, [vp, vp, vp, sz, vp, u32, u32, vp]),
    "rb_scene_emitters": (i32, [vp, vp, sz, P(sz)]),
    "rb_scene_emitters_device": (i32, [vp, vp, sz, vp]),
    "rb_light_rays": (i32, [i32, vp, sz, vp, vp, sz, vp, u32, u32, vp, vp, vp]),
    "rb_direct_light": (i32, [vp, vp, sz, vp, vp, sz, vp, u32, u32, vp]),
    "rb_direct_light_device": (i32, [vp, vp, sz, vp, vp, sz, vp, u32, u32, vp]),
    "rb_emitter_cdf": (i32, [i32, vp, sz, vp]),
    "rb_scene_emitter_cdf": (i32, [vp, vp, sz, P(sz)]),
    "rb_scene_emitter_cdf_device": (i32, [vp, vp, sz, vp]),
    "rb_light_rays_cdf": (i32, [i32, vp, vp, sz, vp, vp, sz, vp, u32, u32, vp, vp, vp]),
    "rb_direct_light_cdf": (i32, [vp, vp, vp, sz, vp, vp, sz, vp, u32, u32, vp]),
    "rb_direct_light_cdf_device": (i32, [vp, vp, vp, sz, vp, vp, sz, vp, u32, u32, vp]),
    "rb_emitter_grid_cdf": (i32, [i32, vp, sz, vp, vp]),
    "rb_emitter_grid_cdf_device": (i32, [vp, vp, sz, vp, vp]),
    "rb_light_rays_grid": (i32, [i32, vp, vp, vp, sz, vp, vp, sz, vp, u32, u32, vp, vp, vp]),
    "rb_direct_light_grid": (i32, [vp, vp, vp, vp, sz, vp, vp, sz, vp, u32, u32, vp]),
    "rb_direct_light_grid_device": (i32, [vp, vp, vp, vp, sz, vp, vp, sz, vp, u32, u32, vp]),
    "rb_direct_light_grid_tally": (i32, [vp, vp, vp, vp, sz, vp, vp, sz, vp, u32, u32, vp, vp]),
    "rb_direct_light_grid_tally_device": (i32, [vp, vp, vp, vp, sz, vp, vp, sz, vp, u32, u32, vp, vp]),
    "rb_emitter_grid_learned": (i32, [i32, vp, sz, vp, vp, C.c_float, vp]),
    "rb_emitter_grid_learned_device": (i32, [vp, vp, sz, vp, vp, C.c_float, vp]),
    "rb_lightmap_surfels": (i32, [i32, vp, sz, vp, sz, vp, vp, vp]),
    "rb_lightmap_surfels_device": (i32, [vp, vp, vp, vp]),
    "rb_lightmap_resolve": (i32, [i32, u32, u32, vp, u32, vp]),
    "rb_bake_lightmap": (i32, [vp, vp, u32, u32, vp, vp]),
    "rb_bake_lightmap_device": (i32, [vp, vp, u32, u32, vp, vp]),
    "rb_last_lightmap_ms": (i32, [vp, P(C.c_float), P(C.c_float)]),
    "rb_probe_rays": (i32, [i32, vp, vp, sz, u32, u32, vp, vp]),
    "rb_bake_probes": (i32, [vp, vp, vp, sz, u32, u32, vp]),
    "rb_bake_probes_device": (i32, [vp, vp, vp, sz, u32, u32, vp]),
    "rb_last_probe_project_ms": (i32, [vp, P(C.c_float)]),
    "rb_probe_coefficients": (i32, [i32, vp, sz, vp]),
    "rb_probe_coefficients_device": (i32, [vp, vp, sz, vp]),
    "rb_light_points": (i32, [i32, vp, vp, vp, sz, vp]),
    "rb_light_points_device": (i32, [vp, vp, vp, vp, sz, vp]),
    "rb_bake_probe_depth": (i32, [vp, vp, vp, sz, u32, u32, C.c_float, vp]),
    "rb_bake_probe_depth_device": (i32, [vp, vp, vp, sz, u32, u32, C.c_float, vp]),
    "rb_last_probe_depth_project_ms": (i32, [vp, P(C.c_float)]),
    "rb_probe_moments": (i32, [i32, vp, sz, vp, vp]),
    "rb_probe_moments_device": (i32, [vp, vp, sz, vp, vp]),
    "rb_light_points_visible": (i32, [i32, vp, vp, vp, vp, sz, vp, vp]),
    "rb_light_points_visible_device": (i32, [vp, vp, vp, vp, vp, sz, vp, vp]),
    "rb_last_query_kernel_name": (C.c_char_p, [vp]),
    "rb_last_query_ms": (i32, [vp, P(C.c_float)]),
    "rb_denoise_default_params": (i32, [vp]),
    "rb_denoise_buffers": (i32, [i32, vp, u32, u32, vp, vp, vp, vp]),
    "rb_denoise": (i32, [vp, vp, vp, vp]),
    "rb_denoise_device": (i32, [vp, vp, vp, vp]),
    "rb_denoise_guides": (i32, [vp, vp]),
    "rb_last_denoise_ms": (i32, [vp, P(C.c_float), P(C.c_float)]),
    "rb_view_from_camera": (i32, [vp, u32, u32, vp]),
    "rb_reproject_default_params": (i32, [vp]),
    "rb_reproject_buffers": (i32, [i32, vp, u32, u32, vp, vp, vp, vp, vp, vp]),
    "rb_reproject_device": (i32, [vp, vp, u32, u32, vp, vp, vp, vp, vp, vp]),
    "rb_denoise_history": (i32, [vp, vp, vp, vp, vp]),
    "rb_denoise_history_device": (i32, [vp, vp, vp, vp, vp]),
    "rb_history_read": (i32, [vp, vp]),
    "rb_history_reset": (i32, [vp]),
    "rb_last_reproject_ms": (i32, [vp, P(C.c_float)]),
    "rb_fast_bvh_builder": (C.c_char_p, [vp, vp]),
    "rb_sphere_tree_builder": (C.c_char_p, [vp, vp]),
    "rb_chunk_tree_builder": (C.c_char_p, [vp, vp]),
    "rb_debug_engine_chunk_tree": (i32, [vp, vp]),
    "rb_debug_own_tree": (i32, [vp, sz, vp, sz, vp, sz, vp, sz, vp, sz, vp, sz, vp, vp, vp]),
    "rb_debug_engine_own_tree": (i32, [vp, vp, sz, vp, sz, vp, sz, vp, vp, vp]),
    "rb_debug_sphere_tree": (i32, [vp, sz, vp, sz, vp, vp, sz, vp, vp]),
    "rb_debug_engine_sphere_tree": (i32, [vp, vp, sz, vp, vp, sz, vp, vp]),
    "rb_version": (C.c_char_p, []),
    "rb_device_name": (i32, [i32, C.c_char_p, sz]),
}
EXPORTS = list(SIGNATURES)


class LibraryMissing(RuntimeError):
    pass


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LibraryMissing(
            f"{LIB_PATH} not found: build it with `make` (or __graft_entry__.build()). "
            "There is no CPU fallback for the render path.")
    try:
        import torch  # noqa: F401  (see module docstring)
    except Exception:  # pragma: no cover - torch is optional for pure C-ABI use
        pass
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError = header/library mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def source_fingerprint():
    """Short hash of the library's sources (csrc/ + the ABI header): profiles are stamped with it so that a
    number measured on another build is never quoted for this one."""
    import hashlib
    h = hashlib.sha256()
    files = sorted(os.listdir(os.path.join(_HERE, "csrc")))
    for name in files:
        with open(os.path.join(_HERE, "csrc", name), "rb") as f:
            h.update(name.encode() + b"\0" + f.read())
    with open(os.path.join(os.path.dirname(_HERE), "include", "rb_abi.h"), "rb") as f:
        h.update(f.read())
    return h.hexdigest()[:16]
