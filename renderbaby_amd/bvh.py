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


def node_count(n_tris):
    """Nodes of the reference-layout tree over n_tris triangles (follows from the count alone; touches no device)."""
    lib = load()
    n_nodes = C.c_size_t(0)
    rc = lib.rb_bvh_build_device(-1, None, int(n_tris), None, 0, C.byref(n_nodes), None)
    if rc:
        raise RuntimeError(f"rb_bvh_build_device size query failed: {rc}")
    return n_nodes.value
