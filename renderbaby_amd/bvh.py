"""BVH build through the library's host-side restatement of ``BVH::new``
(crates/engine-bvh/src/bvh.rs:87-150) -- rb_bvh_build in include/rb_abi.h."""
import ctypes as C

import numpy as np

from . import abi
from ._lib import load


def build(tris):
    """tris: abi.GPU_TRIANGLE[] -> (abi.BVH_NODE[], uint32[] indices)."""
    lib = load()
    tris = np.ascontiguousarray(tris, dtype=abi.GPU_TRIANGLE)
    n = len(tris)
    n_nodes = C.c_size_t(0)
    rc = lib.rb_bvh_build(tris.ctypes.data, n, None, 0, C.byref(n_nodes), None)
    if rc:
        raise RuntimeError(f"rb_bvh_build failed: {rc}")
    nodes = np.zeros(n_nodes.value, dtype=abi.BVH_NODE)
    indices = np.zeros(n, dtype=np.uint32)
    rc = lib.rb_bvh_build(tris.ctypes.data, n, nodes.ctypes.data, len(nodes), C.byref(n_nodes), indices.ctypes.data)
    if rc:
        raise RuntimeError(f"rb_bvh_build failed: {rc}")
    return nodes, indices


def _two_call(fn, prefix, tris):
    from .engine import RenderError
    lib = load()
    tris = np.ascontiguousarray(tris, dtype=abi.GPU_TRIANGLE)
    n = len(tris)
    n_nodes = C.c_size_t(0)
    rc = fn(*prefix, tris.ctypes.data, n, None, 0, C.byref(n_nodes), None)
    if rc:
        raise RenderError(rc, (lib.rb_last_error(None) or b"").decode())
    nodes = np.zeros(n_nodes.value, dtype=abi.BVH_NODE)
    indices = np.zeros(n, dtype=np.uint32)
    rc = fn(*prefix, tris.ctypes.data, n, nodes.ctypes.data, len(nodes), C.byref(n_nodes), indices.ctypes.data)
    if rc:
        raise RenderError(rc, (lib.rb_last_error(None) or b"").decode())
    return nodes, indices


def build_canonical(tris):
    """The canonical reference-layout tree (rb_bvh_build_canonical): ``build``'s topology with every open choice fixed --
    (centroid, index) order, leaves in ascending index, boxes with -0 < +0.  Non-finite vertices raise RenderError
    (InvalidBVH).  tris: abi.GPU_TRIANGLE[] -> (abi.BVH_NODE[], uint32[] indices)."""
    return _two_call(load().rb_bvh_build_canonical, (), tris)


def build_device(tris, device=-1):
    """The same bytes as ``build_canonical``, built on HIP device ``device`` (rb_bvh_build_device)."""
    return _two_call(load().rb_bvh_build_device, (int(device),), tris)


def own_tree_readback(check, fn, *prefix):
    """The two calls of rb_debug_own_tree / rb_debug_engine_own_tree (`prefix`: the arguments before the out arrays): dict of
    nodes (abi.OWN_NODE[]), slots, slot_meta, root, depth, bmin, bmax -- or None when there is no such tree."""
    counts, rd, b6 = (C.c_uint64 * 3)(), (C.c_uint32 * 2)(), (C.c_float * 6)()
    check(fn(*prefix, None, 0, None, 0, None, 0, counts, rd, b6))
    if not counts[1]:
        return None
    nodes = np.zeros(counts[0], dtype=abi.OWN_NODE)
    slots, meta = np.zeros(counts[1], dtype=np.uint32), np.zeros(counts[2], dtype=np.uint32)
    check(fn(*prefix, nodes.ctypes.data, len(nodes), slots.ctypes.data, len(slots), meta.ctypes.data, len(meta), counts, rd, b6))
    assert (counts[0], counts[1], counts[2]) == (len(nodes), len(slots), len(meta)), "the tree changed between the two calls"
    b = np.array(list(b6), dtype=np.float32)
    return dict(nodes=nodes, slots=slots, slot_meta=meta, root=int(rd[0]), depth=int(rd[1]), bmin=b[:3], bmax=b[3:])


def sphere_tree_readback(check, fn, *prefix):
    """The two calls of rb_debug_sphere_tree / rb_debug_engine_sphere_tree: dict of nodes (abi.SPHERE_NODE[]), leaf
    (float32[n, 4]: centre, radius in leaf order), ids, root, depth (stack entries) -- or None when there is no tree."""
    counts, rd = (C.c_uint64 * 2)(), (C.c_uint32 * 2)()
    check(fn(*prefix, None, 0, None, None, 0, counts, rd))
    if not counts[1]:
        return None
    nodes = np.zeros(counts[0], dtype=abi.SPHERE_NODE)
    leaf, ids = np.zeros((counts[1], 4), dtype=np.float32), np.zeros(counts[1], dtype=np.uint32)
    check(fn(*prefix, nodes.ctypes.data, len(nodes), leaf.ctypes.data, ids.ctypes.data, len(ids), counts, rd))
    assert (counts[0], counts[1]) == (len(nodes), len(ids)), "the tree changed between the two calls"
    return dict(nodes=nodes, leaf=leaf, ids=ids, root=int(rd[0]), depth=int(rd[1]))


def _check_global(rc):
    from .engine import RenderError
    if rc:
        raise RenderError(rc, (load().rb_last_error(None) or b"").decode())


def debug_own_tree(tris, nodes, indices):
    """Test aid, host only (rb_debug_own_tree): the host builder's own triangle tree over this mesh and caller tree, unchecked."""
    tris = np.ascontiguousarray(tris, dtype=abi.GPU_TRIANGLE)
    nodes = np.ascontiguousarray(nodes, dtype=abi.BVH_NODE)
    indices = np.ascontiguousarray(indices, dtype=np.uint32)
    return own_tree_readback(_check_global, load().rb_debug_own_tree, tris.ctypes.data, len(tris), nodes.ctypes.data, len(nodes),
                             indices.ctypes.data, len(indices))


def debug_sphere_tree(spheres):
    """Test aid, host only (rb_debug_sphere_tree): the host builder's sphere tree over abi.SPHERE[], unchecked."""
    spheres = np.ascontiguousarray(spheres, dtype=abi.SPHERE)
    return sphere_tree_readback(_check_global, load().rb_debug_sphere_tree, spheres.ctypes.data, len(spheres))


def node_count(n_tris):
    """Nodes of the reference-layout tree over n_tris triangles (follows from the count alone; touches no device)."""
    lib = load()
    n_nodes = C.c_size_t(0)
    rc = lib.rb_bvh_build_device(-1, None, int(n_tris), None, 0, C.byref(n_nodes), None)
    if rc:
        raise RuntimeError(f"rb_bvh_build_device size query failed: {rc}")
    return n_nodes.value
