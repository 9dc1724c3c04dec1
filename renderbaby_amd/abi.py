"""Byte layouts of the C ABI (include/rb_abi.h) as numpy dtypes and ctypes structs.

The numpy dtypes are the host-side mirror of the reference's ``#[repr(C)]`` PODs
(crates/engine-config/src/{uniforms,camera,material,sphere,mesh,point_lights}.rs,
crates/engine-bvh/src/{bvh,triangle}.rs); sizes and offsets are asserted below
and again in tests/test_abi.py.
"""
import ctypes as C

import numpy as np

f4, u4, i4 = np.float32, np.uint32, np.int32

CAMERA = np.dtype([
    ("pane_distance", f4), ("pane_width", f4), ("_pad0", f4, (2,)),
    ("pos", f4, (3,)), ("_pad1", f4), ("dir", f4, (3,)), ("_pad2", f4)])

UNIFORMS = np.dtype([
    ("width", u4), ("height", u4), ("total_samples", u4), ("color_hash_enabled", u4),
    ("camera", CAMERA),
    ("spheres_count", u4), ("triangles_count", u4), ("bvh_node_count", u4),
    ("bvh_triangle_count", u4), ("bvh_root", u4), ("ground_height", f4),
    ("ground_enabled", u4), ("checkerboard_enabled", u4),
    ("sky_color", f4, (3,)), ("max_depth", u4),
    ("checkerboard_color_1", f4, (3,)), ("_pad1", u4),
    ("checkerboard_color_2", f4, (3,)), ("_pad2", u4)])

MATERIAL = np.dtype([
    ("ambient", f4, (3,)), ("_pad0", f4), ("diffuse", f4, (3,)), ("_pad1", f4),
    ("specular", f4, (3,)), ("shininess", f4), ("emissive", f4, (3,)), ("ior", f4),
    ("opacity", f4), ("illum", u4), ("texture_index", i4), ("_pad2", u4)])

SPHERE = np.dtype([("center", f4, (3,)), ("radius", f4), ("material", MATERIAL)])
POINT_LIGHT = np.dtype([("center", f4, (3,)), ("radius", f4), ("material", MATERIAL)])
MESH = np.dtype([("triangle_index_start", u4), ("triangle_count", u4), ("_pad", u4, (2,)),
                 ("material", MATERIAL)])
BVH_NODE = np.dtype([("aabb_min", f4, (3,)), ("_pad0", u4), ("aabb_max", f4, (3,)), ("_pad1", u4),
                     ("left", u4), ("right", u4), ("first_primitive", u4), ("primitive_count", u4)])
GPU_TRIANGLE = np.dtype([("v0", f4, (3,)), ("v0_index", u4), ("v1", f4, (3,)), ("v1_index", u4),
                         ("v2", f4, (3,)), ("v2_index", u4), ("mesh_index", u4),
                         ("_pad0", u4), ("_pad1", u4), ("_pad2", u4)])

# closest-hit queries (rb_cast_rays / rb_render_hits / rb_pick)
RAY = np.dtype([("origin", f4, (3,)), ("_pad0", f4), ("dir", f4, (3,)), ("_pad1", f4)])
HIT = np.dtype([("t", f4), ("kind", u4), ("prim", u4), ("mesh", u4), ("u", f4), ("v", f4), ("_pad", u4, (2,)),
                ("normal", f4, (3,)), ("_pad1", f4)])
SURFACE = np.dtype([("albedo", f4, (3,)), ("flags", u4), ("emissive", f4, (3,)), ("texture_index", i4),
                    ("uv", f4, (2,)), ("_pad", f4, (2,))])
HIT_NONE, HIT_GROUND, HIT_TRIANGLE, HIT_SPHERE, HIT_LIGHT, HIT_INVALID = 0, 1, 2, 3, 4, 0xFFFFFFFF
SURFACE_IS_METAL, SURFACE_USE_TEXTURE = 1, 2
NO_INDEX = 0xFFFFFFFF
# path-traced radiance along given rays (rb_trace_rays): the per-ray sum and the items of one launch
RADIANCE = np.dtype([("sum", f4, (3,)), ("weight", f4)])
TRACE_PIECE_ITEMS = 1 << 24
# camera rays made on the device (rb_camera_rays / rb_trace_camera): the camera record, kinds and flags
CAMERA_EX = np.dtype([("kind", u4), ("width", u4), ("height", u4), ("flags", u4),
                      ("pos", f4, (3,)), ("tan_half_fov", f4), ("right", f4, (3,)), ("half_width", f4),
                      ("up", f4, (3,)), ("half_height", f4), ("forward", f4, (3,)), ("lens_radius", f4),
                      ("focus_distance", f4), ("_reserved", u4, (3,))])
CAM_PERSPECTIVE, CAM_ORTHO, CAM_EQUIRECT = 1, 2, 3
CAM_NO_JITTER = 1
CAMERA_PIECE_ITEMS = 1 << 23
# hemisphere rays made on the device (rb_hemisphere_rays / rb_trace_hemisphere / rb_openness_hemisphere):
# a surface point with its normal, the parameters of a call and the counts of a surfel's samples
SURFEL = np.dtype([("pos", f4, (3,)), ("_pad0", f4), ("normal", f4, (3,)), ("_pad1", f4)])
HEMI_PARAMS = np.dtype([("offset", f4), ("radius", f4), ("mask", u4), ("flags", u4), ("_reserved", u4, (4,))])
OPENNESS = np.dtype([("open", u4), ("valid", u4)])
HEMI_PIECE_ITEMS = 1 << 23
# lightmap texels made on the device (rb_lightmap_surfels / rb_lightmap_resolve / rb_bake_lightmap)
LIGHTMAP_PARAMS = np.dtype([("width", u4), ("height", u4), ("mesh", u4), ("flags", u4), ("offset", f4), ("dilate", u4),
                            ("_reserved", u4, (2,))])
LIGHTMAP_ALL_MESHES, LIGHTMAP_NO_OWNER, LIGHTMAP_FLIP = 0xFFFFFFFF, 0xFFFFFFFF, 1
LIGHTMAP_MAX_SIDE, LIGHTMAP_MAX_DILATE = 16384, 64
# irradiance probes made on the device (rb_probe_rays / rb_bake_probes): a point in free space and the
# ordered SH9 sums of its samples, sum[j][channel], with the number of valid samples behind
PROBE = np.dtype([("pos", f4, (3,)), ("_pad", f4)])
SH9 = np.dtype([("sum", f4, (9, 3)), ("weight", f4)])
PROBE_PIECE_ITEMS = 1 << 23
# light points from a baked probe grid (rb_probe_coefficients / rb_light_points): the regular grid the
# coefficient records (abi.SH9's layout, the weight 1 or 0) belong to, x fastest, and a point's lit value with its blend weight
PROBE_GRID = np.dtype([("origin", f4, (3,)), ("_pad0", u4), ("step", f4, (3,)), ("_pad1", u4), ("counts", u4, (3,)), ("flags", u4)])
LIT = np.dtype([("value", f4, (3,)), ("weight", f4)])
LIGHT_PIECE_POINTS = 1 << 22
# probe visibility (rb_bake_probe_depth / rb_probe_moments / rb_light_points_visible): a probe's 8 x 8
# octahedral map, texel ty * 8 + tx = {sum_r, sum_r2, count, back} (sums) or {mean, mean2, valid, back share} (moments), and
# the blend's parameters
PROBE_DEPTH = np.dtype([("texel", f4, (64, 4))])
LIGHT_VISIBILITY = np.dtype([("normal_bias", f4), ("min_visibility", f4), ("flags", u4), ("_pad", u4)])
VIS_NO_WRAP, VIS_NO_DEPTH = 1, 2
# direct light at surface points (rb_scene_emitters / rb_light_rays / rb_direct_light): an emitter of the
# table -- a triangle as {v0, e1, e2}, a sphere or light as {centre, (radius, 0, 0), 0} --, the parameters of a call and the most
# emitters a table may hold
EMITTER = np.dtype([("a", f4, (3,)), ("kind", u4), ("b", f4, (3,)), ("prim", u4), ("c", f4, (3,)), ("area", f4),
                    ("emissive", f4, (3,)), ("_pad", f4)])
LIGHT_PARAMS = np.dtype([("offset", f4), ("shorten", f4), ("mask", u4), ("flags", u4), ("_reserved", u4, (4,))])
MAX_EMITTERS = 1 << 24
MAX_GRID_ENTRIES = 1 << 26   # cells times emitters of the pick per grid cell
# the tally of shadow rays tried and seen per (cell, emitter), record r * n + j, and the largest prior
GRID_TALLY = np.dtype([("tried", u4), ("seen", u4)])
MAX_PRIOR = 16777216.0
# any-hit occlusion (rb_occluded): result bytes and stage masks
OCCL_VISIBLE, OCCL_OCCLUDED, OCCL_INVALID = 0, 1, 255
MASK_GROUND, MASK_TRIANGLES, MASK_SPHERES, MASK_LIGHTS, MASK_ALL = 1, 2, 4, 8, 15
# the denoiser (rb_denoise*): the guide record of a pixel and the filter's parameters
GUIDE = np.dtype([("normal", f4, (3,)), ("t", f4), ("pos", f4, (3,)), ("cls", u4), ("albedo", f4, (3,)), ("_pad", f4)])
DENOISE_PARAMS = np.dtype([("iterations", u4), ("normal_power_log2", u4), ("sigma_depth", f4), ("sigma_color", f4),
                           ("albedo_floor", f4), ("flags", u4), ("_reserved", u4, (2,))])
# temporal reprojection (rb_reproject* / rb_denoise_history): a render camera as the inverse of the
# pixel-centre ray needs it, the parameters, and a frame record {mean r, g, b, count}
VIEW = np.dtype([("pos", f4, (3,)), ("cx", f4), ("right", f4, (3,)), ("cy", f4), ("up", f4, (3,)), ("sx", f4), ("fwd", f4, (3,)), ("sy", f4)])
REPROJECT_PARAMS = np.dtype([("sigma_depth", f4), ("normal_min", f4), ("albedo_floor", f4), ("max_history", f4), ("flags", u4),
                             ("_reserved", u4, (3,))])
FRAME_RECORD = np.dtype([("mean", f4, (3,)), ("count", f4)])
# test aids (rb_debug_*own_tree / rb_debug_*sphere_tree): a node of the library's own triangle tree and of its sphere tree
OWN_NODE = np.dtype([("lmin", f4, (3,)), ("left", u4), ("lmax", f4, (3,)), ("right", u4),
                     ("rmin", f4, (3,)), ("left_fa", f4), ("rmax", f4, (3,)), ("right_fa", f4)])
SPHERE_NODE = np.dtype([("cx", f4, (4,)), ("cy", f4, (4,)), ("cz", f4, (4,)), ("hx", f4, (4,)), ("hy", f4, (4,)), ("hz", f4, (4,)),
                        ("ref", u4, (4,)), ("axes", u4), ("_pad", u4, (3,))])

SIZES = {"camera": (CAMERA, 48), "uniforms": (UNIFORMS, 144), "material": (MATERIAL, 80),
         "sphere": (SPHERE, 96), "point_light": (POINT_LIGHT, 96), "mesh": (MESH, 96),
         "bvh_node": (BVH_NODE, 48), "gpu_triangle": (GPU_TRIANGLE, 64),
         "ray": (RAY, 32), "hit": (HIT, 48), "surface": (SURFACE, 48),
         "guide": (GUIDE, 48), "denoise_params": (DENOISE_PARAMS, 32), "view": (VIEW, 64),
         "reproject_params": (REPROJECT_PARAMS, 32), "frame_record": (FRAME_RECORD, 16), "camera_ex": (CAMERA_EX, 96),
         "surfel": (SURFEL, 32), "hemi_params": (HEMI_PARAMS, 32), "openness": (OPENNESS, 8),
         "lightmap_params": (LIGHTMAP_PARAMS, 32), "probe": (PROBE, 16), "sh9": (SH9, 112),
         "probe_grid": (PROBE_GRID, 48), "lit": (LIT, 16),
         "probe_depth": (PROBE_DEPTH, 1024), "light_visibility": (LIGHT_VISIBILITY, 16),
         "emitter": (EMITTER, 64), "light_params": (LIGHT_PARAMS, 32),
         "own_node": (OWN_NODE, 64), "sphere_node": (SPHERE_NODE, 128)}
for _n, (_dt, _sz) in SIZES.items():
    assert _dt.itemsize == _sz, (_n, _dt.itemsize, _sz)

# Change<T> discriminants (render_config.rs:99-109)
KEEP, CREATE, UPDATE, DELETE = 0, 1, 2, 3

# status codes (rb_abi.h)
RB_OK = 0
ERR = {
    1: "PaneDistanceOutOfBounds", 2: "PaneWidthOutOfBounds", 3: "InvalidCameraDirection",
    4: "InvalidUniforms", 5: "InvalidSpheres", 6: "InvalidUVs", 7: "InvalidMeshes",
    8: "InvalidLights", 9: "InvalidTextures", 10: "CannotDeleteNonexistent",
    11: "UniformsNotInitialized", 12: "NoMoreFrames", 13: "InvalidBVH", 14: "UnsupportedDelete",
    15: "NullArgument", 16: "Device", 17: "NotInitialized", 18: "InvalidOptions"}
RB_ERR_NO_MORE_FRAMES = 12
RB_ERR_DEVICE = 16   # HIP runtime failure

KERNEL_DEFAULT, KERNEL_PIXEL, KERNEL_QUEUE, KERNEL_STREAM = 0, 1, 2, 3
# rb_debug_trace_form: which instantiation of "k_trace" ran
TRACE_FORM_FLAT, TRACE_FORM_BIG, TRACE_FORM_STAGED, TRACE_FORM_MULTI = 1, 4, 8, 16
TRACE_FORM_SIFT = 2
FLAG_STATS = 1
FLAG_NO_SPHERE_BVH = 2
FLAG_FAST_BVH = 4
FLAG_DEVICE_BVH = 8
FLAG_DEVICE_LBVH = 16
FLAG_REFERENCE_WALK = 32
FLAG_HOST_BVH = 64
FLAG_GATHER_PEER_COPY = 128
FLAG_NO_RUN_AHEAD = 256
FLAG_SKIP_NEAR_DEGENERATE = 512
FLAG_CHUNK_WALK = 1024
FLAG_SPHERE_TREE_HOST = 2048
FLAG_SPHERE_TREE_DEVICE = 4096
FLAG_CHUNK_TREE_HOST = 8192
FLAG_CHUNK_TREE_DEVICE = 16384
FLAG_BUILD_TREE = 32768        # the engine builds the reference-layout tree from the triangles (on the device)
FLAG_BUILD_TREE_HOST = 65536   # ... on the host
COMM_ID_BYTES = 128


class Field(C.Structure):
    _fields_ = [("change", C.c_uint32), ("ptr", C.c_void_p), ("count", C.c_size_t)]


class Config(C.Structure):
    _fields_ = [(n, Field) for n in ("uniforms", "spheres", "uvs", "meshes", "lights", "bvh_nodes",
                                      "bvh_indices", "bvh_triangles", "textures")]


class Texture(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("rgba_data", C.c_void_p)]


class Options(C.Structure):
    _fields_ = [("device", C.c_int32), ("shard_rank", C.c_uint32), ("shard_count", C.c_uint32),
                ("stripe_rows", C.c_uint32), ("passes_per_launch", C.c_uint32), ("kernel", C.c_uint32),
                ("flags", C.c_uint32), ("_reserved", C.c_uint32 * 5)]


class Ray(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("_pad0", C.c_float), ("dir", C.c_float * 3), ("_pad1", C.c_float)]


class Hit(C.Structure):
    _fields_ = [("t", C.c_float), ("kind", C.c_uint32), ("prim", C.c_uint32), ("mesh", C.c_uint32), ("u", C.c_float),
                ("v", C.c_float), ("_pad", C.c_uint32 * 2), ("normal", C.c_float * 3), ("_pad1", C.c_float)]


class Surface(C.Structure):
    _fields_ = [("albedo", C.c_float * 3), ("flags", C.c_uint32), ("emissive", C.c_float * 3),
                ("texture_index", C.c_int32), ("uv", C.c_float * 2), ("_pad", C.c_float * 2)]


class Stats(C.Structure):
    _fields_ = [("segments", C.c_uint64), ("paths", C.c_uint64), ("nodes_popped", C.c_uint64),
                ("tris_tested", C.c_uint64), ("spheres_tested", C.c_uint64),
                ("lights_tested", C.c_uint64), ("mesh_hits", C.c_uint64), ("launches", C.c_uint64),
                ("kernel_ms", C.c_double), ("trace_ms", C.c_double), ("accumulate_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


def algorithmic_bytes(stats, pixels_written, resumed=False):
    """logical bytes the traversal algorithm consumes.

    48 B per node popped, 68 B per triangle tested (64 B triangle + 4 B index),
    96 B per sphere / light tested, 96 + 24 B per accepted mesh hit (Mesh +
    three UV pairs), plus 20 B per pixel per launch (16 B accumulation store +
    4 B RGBA store; +16 B load when a launch resumes an accumulation).
    """
    s = stats if isinstance(stats, dict) else stats.as_dict()
    scene = (48 * s["nodes_popped"] + 68 * s["tris_tested"] + 96 * s["spheres_tested"]
             + 96 * s["lights_tested"] + 120 * s["mesh_hits"])
    frame = pixels_written * (36 if resumed else 20)
    return scene + frame
