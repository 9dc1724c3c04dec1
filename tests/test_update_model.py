"""tests/_update_model.py on the CPU: the model against a reading of gpu_wrapper.rs on hand-written sequences, and the
condition that keeps tests/test_gpu_update_sequences.py honest -- every accepted step of every script it runs changes what
the ORACLE sees, so that an engine which ignored the update could not pass.  For the caches script, whose subject the frame
does not show, the conditions are on the model's emitter table (renderbaby_amd/direct.py) as well.  No device."""
import ctypes as C

import numpy as np
import pytest

from renderbaby_amd import abi, bvh, direct, scenes
from renderbaby_amd.engine import Change, RenderConfig
from tests import _oracle
from tests import _update_model as M

f32 = np.float32
SCRIPTS = [("fixed", None), ("random", 1), ("random", 2), ("random", 3), ("caches", None)]
VARIANTS = {"caller": dict(own_tree=False, large=False), "caller-large": dict(own_tree=False, large=True), "own": dict(own_tree=True, large=False)}


def script_names(kind, seed, own_tree):
    if kind == "caches":
        return M.caches_script(own_tree)
    return M.fixed_script(own_tree) if kind == "fixed" else M.random_script(seed, 10, own_tree)


def script_id(kind, seed):
    return kind if kind in ("fixed", "caches") else f"random{seed}"


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
    caches_only = {f.__name__ for f in M._CACHES_ONLY}
    assert set(M.fixed_script(False)) | set(M.fixed_script(True)) == set(M.STEPS) - caches_only   # the fixed script runs every step there is ...
    assert caches_only <= set(M.caches_script(False)) and caches_only <= set(M.caches_script(True))   # ... but the caches script's own
    assert not caches_only & (set(M.LEGAL[False]) | set(M.LEGAL[True]))


def test_a_kept_count_above_the_buffer_is_the_buffers_length_for_the_oracle():
    """The reference leaves a Keep count above the length to WGSL's robust access (the elements beyond read as zero and are
    never hit); the oracle clamps it, and so does the engine (patch_count).  Pinned here for the oracle, in
    test_gpu_update_sequences.py for the engine."""
    m, s = _started()
    u = s.uniforms.copy()
    u["spheres_count"], u["bvh_node_count"], u["bvh_triangle_count"] = len(s.spheres) + 7, len(s.bvh_nodes) + 3, len(s.bvh_triangles) + 100
    assert m.apply(RenderConfig(uniforms=Change.update(u))) is None and m.kept == 7
    assert np.array_equal(_oracle.render(m.scene, counts_kept=7)[0].view(np.uint32), _oracle.render(s)[0].view(np.uint32))


# ------------------------------------------- the caches script: what it must show ---
def model_table(scene, kept, **counts):
    """direct.scene_emitters of the model's scene under the counts in force (`counts` overrides one of them)"""
    ns, _, nt = M.effective_counts(scene, kept)
    kw = dict(triangle_count=nt, spheres_count=ns)
    kw.update(counts)
    return direct.scene_emitters(scene, **kw)


def _prims(table, kind):
    return set(int(p) for p in table["prim"][table["kind"] == kind])


@pytest.mark.parametrize("own_tree", [False, True], ids=["caller", "own"])
def test_caches_script_moves_the_emitter_table(own_tree):
    """Conditions on tests/test_gpu_update_sequences.py::test_caches_sequence's input, from the model and direct.py alone: the
    table takes every kind, changes often, changes under counts that are cut short, loses emitters to a kept count alone, loses
    its triangles to the colour hash, and stands across every refused step."""
    names = M.caches_script(own_tree)
    first = M.Model(bvh.build_canonical if own_tree else None)
    first.apply(M.create_config(M.base_scene(), with_tree=not own_tree))
    prev, prev_scene = model_table(first.scene, first.kept), first.scene
    all_kinds = changes = changes_cut_short = sphere_by_count = triangle_by_count = emptied_by_hash = refused = 0
    for i, name, rc, why, model in M.run_script(names, "caches", own_tree=own_tree, tree_builder=bvh.build_canonical):
        s, kept = model.scene, model.kept
        now = model_table(s, kept)
        if why is not None:
            refused += 1
            assert s is prev_scene and now.tobytes() == prev.tobytes(), (i, name)
            continue
        ns, _, nt = M.effective_counts(s, kept)
        all_kinds += set(int(k) for k in now["kind"]) == {abi.HIT_TRIANGLE, abi.HIT_SPHERE, abi.HIT_LIGHT}
        if now.tobytes() != prev.tobytes():
            changes += 1
            changes_cut_short += (ns, nt) != (len(s.spheres), len(s.bvh_triangles))
        uniforms_only = all(getattr(rc, f).tag == abi.KEEP for f in M.FIELDS[1:])
        lost_s = _prims(prev, abi.HIT_SPHERE) - _prims(now, abi.HIT_SPHERE)
        lost_t = _prims(prev, abi.HIT_TRIANGLE) - _prims(now, abi.HIT_TRIANGLE)
        # "alone": the step sent the uniforms only, and with the whole buffer counted the emitter would still be there
        if uniforms_only and lost_s and lost_s <= _prims(model_table(s, kept, spheres_count=None), abi.HIT_SPHERE):
            assert min(lost_s) >= ns
            sphere_by_count += 1
        if uniforms_only and lost_t and lost_t <= _prims(model_table(s, kept, triangle_count=None), abi.HIT_TRIANGLE):
            assert min(lost_t) >= nt
            triangle_by_count += 1
        if uniforms_only and lost_t and not _prims(now, abi.HIT_TRIANGLE) and int(s.uniforms["color_hash_enabled"][0]) \
                and int(prev_scene.uniforms["color_hash_enabled"][0]) == 0 and nt == len(s.bvh_triangles):
            emptied_by_hash += 1
        prev, prev_scene = now, s
    got = dict(all_kinds=all_kinds, changes=changes, changes_cut_short=changes_cut_short, sphere_by_count=sphere_by_count,
               triangle_by_count=triangle_by_count, emptied_by_hash=emptied_by_hash, refused=refused)
    print(got)
    assert all_kinds >= 1 and changes >= 12 and changes_cut_short >= 2, got
    assert sphere_by_count >= 1 and triangle_by_count >= 1 and emptied_by_hash >= 1 and refused >= 2, got


def test_caches_script_has_the_steps_in_the_places_the_history_chain_needs():
    for own in (False, True):
        names = M.caches_script(own)
        assert 20 <= len(names) <= 28
        assert {"spheres_emissive", "uniforms_spheres_below", "uniforms_counts_above", "spheres_65", "spheres_emissive_edge", "spheres_moved",
                "create_spheres_shorter", "spheres_delete", "lights_one_dark", "lights_none", "lights_more", "uniforms_triangles_below",
                "triangles_permute_meshes", "triangles_shrink"} <= set(names)
        pairs = list(zip(names, names[1:]))
        assert names.count("uniforms_color_hash") == 2
        on, off = (i for i, n in enumerate(names) if n == "uniforms_color_hash")
        assert off - on >= 2                                             # a step, and with it a table query, between on and off
        assert any(b in M.REFUSED for a, b in pairs if a == "spheres_emissive")                       # refused after a table change
        assert any(b in M.REFUSED for a, b in pairs if a == "uniforms_camera_small")                  # refused after a camera move
        assert ("uniforms_camera_small", "uniforms_camera_small") in pairs
        k = names.index("uniforms_resolution")
        assert k > 0 and names[k + 1:k + 3] == ["uniforms_camera_small", "uniforms_resolution"]
        assert any(n.startswith(("triangles_", "own_triangles_")) for n in names[1:-1])


def test_the_scripts_that_existed_are_unchanged():
    """the fixed and the random scripts, step for step, as they stood before the caches steps were added"""
    materials = ["meshes_swap_metal", "meshes_shininess", "meshes_too_short", "meshes_texture_none", "meshes_texture_valid", "uvs_new_values",
                 "uvs_odd", "meshes_texture_past_end", "meshes_swap_metal", "meshes_texture_valid", "textures_other", "textures_empty",
                 "uvs_shorter", "textures_none", "textures_other", "lights_more", "lights_fewer", "lights_none", "create_ignored", "lights_more"]
    spheres = ["spheres_64", "spheres_65", "uniforms_spheres_below", "spheres_64", "spheres_moved", "spheres_empty", "spheres_delete",
               "spheres_70", "create_spheres_shorter", "uniforms_resolution", "uniforms_color_hash", "uniforms_camera", "uniforms_nodes_below",
               "uniforms_triangles_below", "uniforms_all_below", "uniforms_counts_above", "uniforms_color_hash", "uniforms_resolution",
               "spheres_40"]
    assert M.fixed_script(False) == materials + spheres + [
        "triangles_shrink", "nodes_cyclic", "triangles_permute_meshes", "triangles_bad_mesh", "tree_swap", "nodes_leaf_past_indices",
        "indices_reverse_leaves", "triangles_create_taken", "tree_create_taken", "uvs_new_values", "indices_reverse_leaves", "tree_swap"]
    assert M.fixed_script(True) == materials + spheres + [
        "triangles_shrink", "own_with_nodes", "own_triangles_100", "triangles_permute_meshes", "own_triangles_128", "triangles_bad_mesh",
        "own_triangles_129", "uniforms_nodes_below", "own_triangles_delete", "own_triangles_578", "triangles_create_taken", "uvs_new_values"]
    assert M.random_script(1, 10, False) == ["spheres_empty", "spheres_delete", "uniforms_nodes_below", "indices_reverse_leaves", "meshes_shininess",
                                             "meshes_too_short", "uniforms_counts_above", "indices_reverse_leaves", "lights_more",
                                             "create_spheres_shorter"]
    assert M.random_script(1, 10, True) == ["spheres_empty", "spheres_moved", "uniforms_triangles_below", "own_triangles_578", "meshes_shininess",
                                            "create_ignored", "own_triangles_578", "lights_fewer", "own_triangles_100", "spheres_65"]
    assert M.random_script(2, 10, False) == ["create_ignored", "textures_none", "lights_more", "spheres_64", "uniforms_counts_above", "spheres_70",
                                             "lights_fewer", "triangles_bad_mesh", "uniforms_counts_above", "uniforms_spheres_below"]
    assert M.random_script(2, 10, True) == ["create_spheres_shorter", "textures_none", "lights_more", "spheres_65", "create_ignored", "spheres_70",
                                            "lights_none", "triangles_create_taken", "create_ignored", "uniforms_nodes_below"]
    assert M.random_script(3, 10, False) == ["uniforms_counts_above", "meshes_texture_valid", "uvs_shorter", "textures_other", "uvs_shorter",
                                             "uniforms_all_below", "create_spheres_shorter", "triangles_permute_meshes", "meshes_shininess",
                                             "meshes_texture_valid"]
    assert M.random_script(3, 10, True) == ["create_ignored", "meshes_texture_valid", "uvs_shorter", "textures_other", "uvs_shorter",
                                            "uniforms_counts_above", "own_triangles_100", "triangles_bad_mesh", "meshes_shininess",
                                            "meshes_texture_valid"]
