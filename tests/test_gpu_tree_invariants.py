"""The device-built own triangle tree (k_lbvh_* / k_ploc_*) and sphere tree (k_ms_*, section 4.3) read back
from the engine and held to tests/_tree_model.py's invariants, at the sizes and degeneracies where a builder goes wrong.  The
structure is checked before anything walks it (rb_reserve prepares without tracing); only a tree that passed is rendered, 16 x 16,
1 spp, depth 2, and the frame, the accumulation and the segment count are the oracle's, exactly.  Every case asserts the builder
that ran.  (tests/test_tree_invariants.py shows, without a GPU, that the checker rejects each single corruption.)"""
import dataclasses
import functools

import numpy as np
import pytest

from renderbaby_amd import Engine, RenderConfig, abi
from tests import _oracle
from tests import _tree_cases as K
from tests import _tree_model as M

pytestmark = pytest.mark.gpu

OWN_BUILDERS = {"ploc": (dict(device_bvh=True), "device-ploc"), "lbvh": (dict(device_lbvh=True), "device-lbvh"),
                "host": (dict(host_bvh=True), "host-sah")}
SPHERE_BUILDERS = {"device": "device-median", "host": "host-median"}


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def mesh_reference(case):
    scene = K.mesh_scene(case)
    acc, _, rgba, st = _oracle.render(scene)
    assert st["segments"] > 256, (case, "the camera sees no geometry")
    return scene, _u32(acc), rgba, st["segments"]


@functools.lru_cache(maxsize=None)
def sphere_reference(layout, n):
    scene = K.sphere_scene(layout, n)
    acc, _, rgba, st = _oracle.render(scene)                       # the reference's linear scan
    if layout != "radius_zero":                                     # (a sphere of radius 0 is never hit: that frame is the sky)
        assert st["segments"] > 256, (layout, n, "the camera sees no sphere")
    return scene, _u32(acc), rgba, st["segments"]


def check_frame(eng, want, where):
    _, acc, rgba, segments = want
    eng.reset_stats()
    px = eng.render_current().pixels
    assert np.array_equal(px, rgba), (where, "pixels differ from the oracle's", int((px != rgba).any(-1).sum()))
    assert np.array_equal(_u32(eng.read_accumulation()), acc), (where, "accumulation differs from the oracle's")
    assert eng.stats()["segments"] == segments, (where, "segments")


def own_structure(eng, scene, named, where):
    """the own tree read back and checked against the scene's mesh; returns the read-back"""
    eng.reserve(1)                                                  # ensure_prepared: the tree is built, nothing walks it
    assert eng.fast_bvh_builder()[0] == named, (where, eng.fast_bvh_builder())
    t = eng.debug_own_tree()
    assert t is not None, where
    report = {}
    why = M.check_own_tree(t["nodes"], t["slots"], t["slot_meta"], t["root"], t["depth"], t["bmin"], t["bmax"], scene.bvh_triangles,
                           scene.bvh_indices, len(scene.bvh_triangles), report)
    assert why is None, (where, why)
    print(f"{where}: {len(t['slots'])} slots, depth {t['depth']}, need {report['need']}, excess {report['excess']}")
    return t


# ------------------------------------------------------------------ the own tree ---
def own_engine(case, builder, **kw):
    flags, named = OWN_BUILDERS[builder]
    scene = K.mesh_scene(case)
    rc = RenderConfig.from_scene(scene)
    eng = Engine.new(rc, device=0, stats=True, **flags, **kw)
    eng.update(rc)
    return eng, scene, named


@pytest.mark.parametrize("builder", sorted(OWN_BUILDERS))
@pytest.mark.parametrize("case", K.MESH_CASES)
def test_own_tree_structure(case, builder):
    """the structure alone, nothing walks the tree: an under-reported depth shows here without a write past stack_overflow"""
    eng, scene, named = own_engine(case, builder)
    try:
        t = own_structure(eng, scene, named, (case, builder))
        if (case, builder) == ("deep", "lbvh"):
            assert t["depth"] > 32, ("the scene is no longer deep: the spill path below would not be reached", t["depth"])
    finally:
        eng.close()


@pytest.mark.parametrize("builder", sorted(OWN_BUILDERS))
@pytest.mark.parametrize("case", [c for c in K.MESH_CASES if c != "deep"])
def test_own_tree_checked_then_rendered(case, builder):
    want = mesh_reference(case)
    eng, scene, named = own_engine(case, builder)
    try:
        own_structure(eng, scene, named, (case, builder))
        check_frame(eng, want, (case, builder))
        assert eng.last_kernel_name() == "k_trace_fast", (case, builder, eng.last_kernel_name())
    finally:
        eng.close()


@pytest.mark.parametrize("kernel", ["stream", "queue"])
def test_deep_lbvh_tree_checked_then_spills(kernel):
    """LBVH, deeper than the LDS stack: the walk spills to stack_overflow (FastWalk::spill), under both persistent kernels"""
    want = mesh_reference("deep")
    rc = RenderConfig.from_scene(want[0])
    eng = Engine.new(rc, device=0, stats=True, device_lbvh=True, kernel={"stream": abi.KERNEL_STREAM, "queue": abi.KERNEL_QUEUE}[kernel])
    try:
        eng.update(rc)
        t = own_structure(eng, want[0], "device-lbvh", ("deep", kernel))
        assert t["depth"] > 32, ("the scene is no longer deep: nothing would spill", t["depth"])
        check_frame(eng, want, ("deep", kernel))
    finally:
        eng.close()


def test_deep_tree_under_the_pixel_kernel_is_the_hosts():
    """no bounded grid, no spill column: the depth-limited host builder takes a tree the device made too deep"""
    want = mesh_reference("deep")
    rc = RenderConfig.from_scene(want[0])
    eng = Engine.new(rc, device=0, stats=True, device_lbvh=True, kernel=abi.KERNEL_PIXEL)
    try:
        eng.update(rc)
        t = own_structure(eng, want[0], "host-sah", ("deep", "pixel"))
        assert t["depth"] <= 32
        check_frame(eng, want, ("deep", "pixel"))
    finally:
        eng.close()


@pytest.mark.parametrize("builder", ["ploc", "lbvh"])
def test_own_tree_follows_updates(builder):
    """one engine, 2049 -> 1025 -> 2049 triangles with the matching trees: after each step the read-back is the current mesh's"""
    kw, named = OWN_BUILDERS[builder]
    first = mesh_reference("count_2049")
    eng = Engine.new(RenderConfig.from_scene(first[0]), device=0, stats=True, **kw)
    try:
        for step, case in enumerate(["count_2049", "count_1025", "count_2049"]):
            want = mesh_reference(case)
            eng.update(RenderConfig.from_scene(want[0], create=step == 0))
            own_structure(eng, want[0], named, (builder, step, case))
            check_frame(eng, want, (builder, step, case))
    finally:
        eng.close()


# --------------------------------------------------------------- the sphere tree ---
def sphere_structure(eng, scene, builder, where):
    assert eng.sphere_tree_builder()[0] == SPHERE_BUILDERS[builder], (where, eng.sphere_tree_builder())
    t = eng.debug_sphere_tree()
    assert t is not None, where
    why = M.check_sphere_tree(t["nodes"], t["leaf"], t["ids"], t["root"], t["depth"], scene.spheres)
    assert why is None, (where, why)


def sphere_engine(layout, n, builder):
    scene = K.sphere_scene(layout, n)
    rc = RenderConfig.from_scene(scene)
    eng = Engine.new(rc, device=0, stats=True, sphere_tree=builder)
    eng.update(rc)                                                  # the sphere tree is built with the update
    return eng, scene


@pytest.mark.parametrize("builder", sorted(SPHERE_BUILDERS))
@pytest.mark.parametrize("layout,n", K.SPHERE_CASES)
def test_sphere_tree_structure(layout, n, builder):
    eng, scene = sphere_engine(layout, n, builder)
    try:
        sphere_structure(eng, scene, builder, (layout, n, builder))
    finally:
        eng.close()


@pytest.mark.parametrize("builder", sorted(SPHERE_BUILDERS))
@pytest.mark.parametrize("layout,n", K.SPHERE_CASES)
def test_sphere_tree_checked_then_rendered(layout, n, builder):
    want = sphere_reference(layout, n)
    eng, scene = sphere_engine(layout, n, builder)
    try:
        sphere_structure(eng, scene, builder, (layout, n, builder))
        check_frame(eng, want, (layout, n, builder))
    finally:
        eng.close()


def test_no_tree_reads_back_as_none():
    scene = K.sphere_scene("random", 65)
    scene = dataclasses.replace(scene, spheres=scene.spheres[:64].copy())
    scene.uniforms = scene.uniforms.copy()
    scene.uniforms["spheres_count"] = 64
    rc = RenderConfig.from_scene(scene)
    eng = Engine.new(rc, device=0)
    try:
        eng.update(rc)
        eng.reserve(1)
        assert eng.debug_sphere_tree() is None and eng.debug_own_tree() is None      # 64 spheres are scanned; no mesh
    finally:
        eng.close()
