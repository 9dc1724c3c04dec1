"""tests/_update_model.py on the CPU: the model against a reading of gpu_wrapper.rs on hand-written sequences, and the
condition that keeps tests/test_gpu_update_sequences.py honest -- every accepted step of every script it runs changes what
the ORACLE sees, so that an engine which ignored the update could not pass.  No device."""
import ctypes as C

import numpy as np
import pytest

from renderbaby_amd import bvh, scenes
from renderbaby_amd.engine import Change, RenderConfig
from tests import _oracle
from tests import _update_model as M

f32 = np.float32
SCRIPTS = [("fixed", None), ("random", 1), ("random", 2), ("random", 3)]
VARIANTS = {"caller": dict(own_tree=False, large=False), "caller-large": dict(own_tree=False, large=True), "own": dict(own_tree=True, large=False)}


def script_names(kind, seed, own_tree):
    return M.fixed_script(own_tree) if kind == "fixed" else M.random_script(seed, 10, own_tree)


def script_id(kind, seed):
    return "fixed" if kind == "fixed" else f"random{seed}"


# ------------------------------------------------------- the model, rule by rule ---
def _started(own=False):
    m = M.Model(bvh.build_canonical if own else None)
    s = M.base_scene()
    assert m.apply(M.create_config(s, with_tree=not own)) is None
    return m, s


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def test_first_update_only_create_acts():
    s = M.base_scene()
    m = M.Model()
    rc = M.create_config(s)
    rc.lights = Change.update(s.lights)
    assert "lights" in m.apply(rc) and m.scene is None and not m.initialized          # validate_init
    rc = M.create_config(s)
    rc.bvh_triangles = Change.update(s.bvh_triangles)                                   # not checked by validate_init, and not acted on
    rc.bvh_nodes, rc.bvh_indices = Change.keep(), Change.keep()
    assert m.apply(rc) is None
    assert len(m.scene.bvh_triangles) == 0 and len(m.scene.bvh_nodes) == 0 and _same(m.scene.spheres, s.spheres)
    # Keep nodes: the caller's count.  The Update was not acted on, yet update_uniforms takes its vector's length (:490): a count
    # that the (empty) buffer does not back, which the model marks as kept
    assert m.kept == M.KEPT_NODES | M.KEPT_TRIANGLES
    assert int(m.scene.uniforms["bvh_triangle_count"][0]) == len(s.bvh_triangles)


def test_later_update_acts_and_keep_leaves_buffer_and_count():
    m, s = _started()
    assert m.kept == 0 and _same(m.scene.meshes, s.meshes)
    sp = M.make_spheres(12, 3)
    u = s.uniforms.copy()
    u["spheres_count"], u["bvh_triangle_count"] = 999, 17
    assert m.apply(RenderConfig(uniforms=Change.update(u), spheres=Change.update(sp))) is None
    assert _same(m.scene.spheres, sp) and int(m.scene.uniforms["spheres_count"][0]) == 12          # Update: the vector's length
    assert m.kept == M.KEPT_NODES | M.KEPT_TRIANGLES and int(m.scene.uniforms["bvh_triangle_count"][0]) == 17   # Keep: the caller's
    assert _same(m.scene.bvh_triangles, s.bvh_triangles) and _same(m.scene.lights, s.lights)
    # three steps: the next config's Keep of spheres puts the caller's count in force again, the buffer stays
    u2 = s.uniforms.copy()
    u2["spheres_count"] = 5
    assert m.apply(RenderConfig(uniforms=Change.update(u2), lights=Change.update(s.lights[:1]))) is None
    assert len(m.scene.spheres) == 12 and m.kept == 7 and int(m.scene.uniforms["spheres_count"][0]) == 5 and len(m.scene.lights) == 1


def test_later_create_acts_for_the_bvh_fields_only():
    m, s = _started()
    t = s.bvh_triangles[:100].copy()
    nodes, idx = bvh.build(t)
    other = M.make_spheres(7, 9)
    rc = RenderConfig(uniforms=Change.update(s.uniforms), spheres=Change.create(other), meshes=Change.create(s.meshes[:1]),
                      lights=Change.create(s.lights[:1]), uvs=Change.create(s.uvs[:2]), textures=Change.create([]),
                      bvh_nodes=Change.create(nodes), bvh_indices=Change.create(idx), bvh_triangles=Change.create(t))
    # (meshes[:1] is ignored, so the four meshes still cover the triangles' mesh indices)
    assert m.apply(rc) is None
    for f in ("spheres", "meshes", "lights", "uvs"):
        assert _same(getattr(m.scene, f), getattr(s, f)), f
    assert len(m.scene.textures) == 3
    assert _same(m.scene.bvh_triangles, t) and _same(m.scene.bvh_nodes, nodes) and _same(m.scene.bvh_indices, idx)
    # gpu_wrapper.rs:476: the count is the ignored vector's length; the buffer is the old one
    assert int(m.scene.uniforms["spheres_count"][0]) == 7 and m.kept == M.KEPT_SPHERES
    assert int(m.scene.uniforms["bvh_triangle_count"][0]) == 100 and int(m.scene.uniforms["bvh_node_count"][0]) == len(nodes)


def test_delete_empties_spheres_and_the_bvh_fields():
    m, s = _started()
    assert m.apply(RenderConfig(uniforms=Change.update(s.uniforms), spheres=Change.delete())) is None
    assert len(m.scene.spheres) == 0 and int(m.scene.uniforms["spheres_count"][0]) == 0 and m.kept == M.KEPT_NODES | M.KEPT_TRIANGLES
    assert m.apply(RenderConfig(uniforms=Change.update(s.uniforms), bvh_nodes=Change.delete(), bvh_indices=Change.delete(),
                                bvh_triangles=Change.delete())) is None
    assert len(m.scene.bvh_nodes) == len(m.scene.bvh_indices) == len(m.scene.bvh_triangles) == 0
    assert m.kept == M.KEPT_SPHERES and int(m.scene.uniforms["bvh_node_count"][0]) == 0 and int(m.scene.uniforms["bvh_triangle_count"][0]) == 0
    assert len(m.scene.spheres) == 0 and _same(m.scene.meshes, s.meshes)


@pytest.mark.parametrize("field", M.NO_DELETE)
def test_delete_of_the_other_fields_is_refused(field):
    m, s = _started()
    before, scene, kept = M.scene_bytes(m.scene, m.kept), m.scene, m.kept
    why = m.apply(RenderConfig(uniforms=Change.update(s.with_params(width=8).uniforms), **{field: Change.delete()}))
    assert why and field in why
    assert M.scene_bytes(m.scene, m.kept) == before and m.scene is scene and m.kept == kept       # not even the uniforms were taken


def test_an_engine_that_builds_the_tree_follows_the_triangles():
    m, s = _started(own=True)
    nodes, idx = bvh.build_canonical(s.bvh_triangles)
    assert _same(m.scene.bvh_nodes, nodes) and _same(m.scene.bvh_indices, idx) and m.kept == 0
    assert "Keep" in m.apply(RenderConfig(uniforms=Change.update(s.uniforms), bvh_nodes=Change.update(s.bvh_nodes)))
    t = s.bvh_triangles[:100].copy()
    assert m.apply(RenderConfig(uniforms=Change.update(s.uniforms), bvh_triangles=Change.update(t))) is None
    assert len(m.scene.bvh_nodes) == 1 and m.kept == M.KEPT_SPHERES and int(m.scene.uniforms["bvh_node_count"][0]) == 1
    assert m.apply(RenderConfig(uniforms=Change.update(s.uniforms), bvh_triangles=Change.delete())) is None
    assert len(m.scene.bvh_nodes) == 0 and len(m.scene.bvh_indices) == 0 and int(m.scene.uniforms["bvh_node_count"][0]) == 0


# --------------------------------------------------------------- what the oracle sees ---
def primary_rays(scene):
    """[y, x] in the accumulation's order -> (origin, direction) of the pixel centres"""
    w, h = scene.width, scene.height
    O, D = np.zeros((h, w, 3), f32), np.zeros((h, w, 3), f32)
    L = _oracle.lib()
    u = np.ascontiguousarray(scene.uniforms)
    o, d = np.zeros(3, f32), np.zeros(3, f32)
    for y in range(h):
        for x in range(w):
            L.rbo_primary_ray(u.ctypes.data, x, y, f32(0), f32(0), o.ctypes.data, d.ctypes.data)
            O[y, x], D[y, x] = o, d
    return O, D


def traced(scene, kept, O, D):
    """per ray, everything rbo_trace_ray reports: the radiance's three words and its seven counters"""
    os_ = _oracle.OracleScene(scene, 1, kept)
    L = _oracle.lib()
    h, w = O.shape[:2]
    out = np.zeros((h, w, 3 + len(_oracle.STAT_KEYS)), np.uint64)
    rgb = np.zeros(3, f32)
    for y in range(h):
        for x in range(w):
            st = _oracle.Stats()
            o, d = np.ascontiguousarray(O[y, x]), np.ascontiguousarray(D[y, x])
            L.rbo_trace_ray(C.byref(os_.c), o.ctypes.data, d.ctypes.data, 1 + y * w + x, rgb.ctypes.data, C.byref(st))
            out[y, x, :3] = rgb.view(np.uint32)
            out[y, x, 3:] = [st.as_dict()[k] for k in _oracle.STAT_KEYS]
    return out


def first_hit_is_triangle(scene, kept, O, D):
    """rbo_trace_ray with max_depth 1 returns the winner's emissive: 1 for every mesh, 0 for everything else"""
    t = scenes.Scene(scene.uniforms.copy(), scene.spheres.copy(), scene.lights.copy(), scene.meshes.copy(), scene.bvh_nodes, scene.bvh_indices,
                     scene.bvh_triangles, scene.uvs, scene.textures)
    for arr, v in ((t.spheres, 0.0), (t.lights, 0.0), (t.meshes, 1.0)):
        arr["material"]["emissive"] = v
    t.uniforms["sky_color"], t.uniforms["max_depth"], t.uniforms["color_hash_enabled"] = (0, 0, 0), 1, 0
    return traced(t, kept, O, D)[..., 0] == np.float32(1.0).view(np.uint32)


def oracle_view(scene, kept):
    acc = _oracle.render(scene, counts_kept=kept)[0]
    O, D = primary_rays(scene)
    return acc.view(np.uint32), traced(scene, kept, O, D), (O, D)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("kind, seed", SCRIPTS)
def test_every_step_bites(kind, seed, variant):
    """After each accepted step that changes a byte of the model's scene, the oracle's frame or its per-ray trace of the pixel
    centres differs from the step before; for the uvs / textures / meshes steps in a pixel whose first hit is a triangle.
    Refused steps leave the model byte-identical; steps that change no byte (a Create that is ignored) leave the frame."""
    kw = VARIANTS[variant]
    names = script_names(kind, seed, kw["own_tree"])
    first = M.Model(bvh.build_canonical if kw["own_tree"] else None)
    first.apply(M.create_config(M.base_scene(kw["large"]), with_tree=not kw["own_tree"]))
    prev_bytes, prev = M.scene_bytes(first.scene, first.kept), oracle_view(first.scene, first.kept)
    prev_scene, prev_kept = None, 0
    assert len(first.scene.bvh_nodes) > 1 and len(first.scene.bvh_triangles) >= (1024 if kw["large"] else 258)
    for i, name, rc, why, model in M.run_script(names, script_id(kind, seed), tree_builder=bvh.build_canonical, **kw):
        where = (variant, i, name)
        if why is not None:
            assert model.scene is prev_scene and model.kept == prev_kept, where     # not a byte, not a count
        prev_scene, prev_kept = model.scene, model.kept
        now_bytes = M.scene_bytes(model.scene, model.kept)
        assert (why is not None) == (name in M.REFUSED), (where, why)
        if why is not None:
            assert now_bytes == prev_bytes, where
            continue
        now = oracle_view(model.scene, model.kept)
        if now_bytes == prev_bytes:
            assert np.array_equal(now[0], prev[0]), where
            continue
        if now[0].shape != prev[0].shape:
            differs = np.ones(now[0].shape[:2], bool)            # another resolution: another frame
        else:
            differs = (now[0] != prev[0]).any(-1) | (now[1] != prev[1]).any(-1)
        assert differs.any(), (where, "the step changes nothing the oracle sees")
        if name in M.TRIANGLE_FIRST:
            assert (differs & first_hit_is_triangle(model.scene, model.kept, *now[2])).any(), (where, "no differing pixel shows a triangle first")
        if name.startswith("uniforms_") and name.endswith("_below") or name == "create_spheres_shorter":
            full = _oracle.render(model.scene, counts_kept=0)[0].view(np.uint32)
            assert not np.array_equal(full, now[0]), (where, "the kept count changes nothing")
        prev_bytes, prev = now_bytes, now


def test_random_scripts_are_legal_and_reach_every_kind():
    for own in (False, True):
        drawn = set()
        for seed in (1, 2, 3):
            names = M.random_script(seed, 10, own)
            assert len(names) == 10 and set(names) <= set(M.LEGAL[own])
            assert names == M.random_script(seed, 10, own)
            drawn |= set(names)
        assert len(drawn) >= 15
    assert not set(M.LEGAL[True]) & {"tree_swap", "tree_create_taken", "indices_reverse_leaves", "nodes_cyclic", "nodes_leaf_past_indices"}
    assert set(M.fixed_script(False)) | set(M.fixed_script(True)) == set(M.STEPS)   # the fixed script runs every step there is


def test_a_kept_count_above_the_buffer_is_the_buffers_length_for_the_oracle():
    """The reference leaves a Keep count above the length to WGSL's robust access (the elements beyond read as zero and are
    never hit); the oracle clamps it, and so does the engine (patch_count).  Pinned here for the oracle, in
    test_gpu_update_sequences.py for the engine."""
    m, s = _started()
    u = s.uniforms.copy()
    u["spheres_count"], u["bvh_node_count"], u["bvh_triangle_count"] = len(s.spheres) + 7, len(s.bvh_nodes) + 3, len(s.bvh_triangles) + 100
    assert m.apply(RenderConfig(uniforms=Change.update(u))) is None and m.kept == 7
    assert np.array_equal(_oracle.render(m.scene, counts_kept=7)[0].view(np.uint32), _oracle.render(s)[0].view(np.uint32))
