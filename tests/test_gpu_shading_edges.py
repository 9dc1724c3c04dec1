"""What happens AFTER the winner is known -- texture lookup (offsets, every entry of the sRGB table, shapes, clamps, wrap),
uv interpolation and its guards, the checkerboard where i32 saturates and wraps, the per-material prep at its thresholds,
texture updates -- against the oracle, bit for bit on uint32 views, no ray left out.  The scenes and rays are those of
tests/_edge_scenes.py; tests/test_shading_edges_scene.py shows on the oracle alone that they reach these edges, and its
coverage conditions are asserted here again beside every comparison.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from renderbaby_amd import Engine, RenderConfig, abi
from renderbaby_amd.engine import Change, RenderError
from tests import _edge_scenes as es
from tests import _oracle
from tests.conftest import has_gpu
from tests.test_gpu_parity import KERNELS
from tests.test_gpu_query import (_copy, _engine, _normalize, check_records, check_winner_ids, id_scene, is_metal, oracle_emissive,
                                  pixel_centre_rays, sample_texture)
from tests.test_shading_edges_scene import (INHERITED_LIGHTS, INHERITED_SPHERES, assert_edge_conditions, assert_far_conditions,
                                            edge_conditions, far_conditions)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

f32 = np.float32
WALKS = [pytest.param(dict(), "k_query_chunk", id="chunk"), pytest.param(dict(reference_walk=True), "k_query_bvh", id="reference"),
         pytest.param(dict(host_bvh=True), "k_query_bvh", id="host_bvh")]
INVALID_TEXTURES = {v: k for k, v in abi.ERR.items()}["InvalidTextures"]   # RB_ERR_INVALID_TEXTURES
STAT_KEYS = ("segments", "paths", "nodes_popped", "tris_tested", "spheres_tested", "lights_tested", "mesh_hits")


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _aimed():
    s = es.texture_edges_scene()
    O, D, Q = es.aimed_rays(s)
    return O, D, Q, edge_conditions(s, O, D, Q)


def _cast_and_check(scene, O, D, kw, kernel, label):
    """ways 1 and 2 of tests/test_gpu_query.py for the rays (O, D): every record against the shader's arithmetic on the
    primitive it names, and the named primitive against the oracle's own walk on the identification scene"""
    Dn = _normalize(D)
    e = _engine(scene, **kw)
    try:
        hits, surf = e.cast_rays(O, D, surfaces=True)
        assert e.last_query_kernel_name() == kernel
    finally:
        e.close()
    assert (hits["kind"] != abi.HIT_INVALID).all()
    inherited = check_records(scene, O, Dn, hits, surf, label)
    ids = id_scene(scene)
    ei = _engine(ids, **kw)
    try:
        hits_i, surf_i = ei.cast_rays(O, D, surfaces=True)
    finally:
        ei.close()
    em = oracle_emissive(ids, O, Dn)
    assert np.array_equal(_u32(surf_i["emissive"]), _u32(em)), label
    check_winner_ids(ids, hits_i, em)
    for f in ("t", "kind", "prim", "u", "v", "normal"):
        assert np.array_equal(_u32(hits_i[f]), _u32(hits[f])), f
    return hits, surf, inherited


@pytest.mark.parametrize("color_hash", [0, 1])
@pytest.mark.parametrize("kw,kernel", WALKS)
def test_aimed_rays(kw, kernel, color_hash):
    """one ray at every texel of every texture, grids with corners and edge midpoints on the tiled / integer / offset /
    below-zero / v = 0 quads, the out-of-range texture indices and uv indices, the spheres and lights in front"""
    O, D, Q, cond = _aimed()
    assert_edge_conditions(cond)
    s = es.texture_edges_scene(color_hash=color_hash)
    hits, surf, inherited = _cast_and_check(s, O, D, kw, kernel, f"aimed hash={color_hash}")
    assert inherited >= INHERITED_SPHERES + INHERITED_LIGHTS, inherited
    if not color_hash:   # the device's own records name every texture and the tail quads too
        tri = hits["kind"] == abi.HIT_TRIANGLE
        assert set(range(es.N_TEX)) <= set(surf["texture_index"][tri].tolist())
        for name in ("uv_straddle", "uv_beyond", "oob_max"):
            assert np.isin(hits["prim"][tri], es.quad_triangles(s, name)).any(), name


@pytest.mark.parametrize("kw,kernel", WALKS)
def test_far_ground(kw, kernel):
    """the checkerboard where floor(uv * 10) saturates i32, where the sum of the two wraps, where it is negative and odd, where
    uv * 10 is infinite; and the ground test's |d.y| threshold from both sides"""
    s = es.texture_edges_scene()
    O, D = es.far_ground_rays()
    cond = far_conditions(s, O, _normalize(D))
    assert_far_conditions(cond)
    hits, surf, _ = _cast_and_check(s, O, D, kw, kernel, "far ground")
    assert (hits["kind"] == abi.HIT_GROUND).sum() == len(O) - cond["dy_refused"] == sum(cond[k] for k in ("plain", "saturated", "beyond", "infinite"))


@pytest.mark.parametrize("color_hash", [0, 1])
def test_material_prep_at_the_thresholds(color_hash):
    """k_prep_materials: one ray at each threshold sphere; SURFACE_IS_METAL is the numpy-float32 predicate, the albedo is the
    specular colour, or diffuse * texture at the inherited uv"""
    s = es.texture_edges_scene(color_hash=color_hash)
    O, D, idx = es.threshold_rays(s)
    hits, surf, _ = _cast_and_check(s, O, D, dict(), "k_query_chunk", "thresholds")
    os_ = _oracle.OracleScene(s)
    names = [n for n, _ in es.threshold_materials()]
    seen = set()
    for k, (name, h, sf) in enumerate(zip(names, hits, surf)):
        assert int(h["kind"]) == abi.HIT_SPHERE and int(h["prim"]) == int(idx[k]), name
        m = s.spheres[int(idx[k])]["material"]
        metal = is_metal(m)
        assert bool(int(sf["flags"]) & abi.SURFACE_IS_METAL) == metal, name
        exp = m["specular"].astype(f32) if metal else (m["diffuse"].astype(f32) * sample_texture(os_, int(m["texture_index"]), sf["uv"])).astype(f32)
        assert sf["uv"].any() and np.array_equal(_u32(sf["albedo"]), _u32(exp)), (name, sf["albedo"], exp)
        seen.add((name.split("_")[0], name.rsplit("_", 1)[-1], metal))
    # both sides of both comparisons, and 0.01f itself: `>` false, `<` false
    assert {("spec", "below", False), ("spec", "above", True), ("spec", "equal", False),
            ("diff", "below", True), ("diff", "above", False), ("diff", "equal", False)} <= seen, seen


def _render(scene, **kw):
    rc = RenderConfig.from_scene(scene)
    e = Engine.new(rc, stats=True, **kw)
    try:
        frame = e.render(rc)
        return frame.pixels, e.read_accumulation(), e.stats(), e.last_kernel_name()
    finally:
        e.close()


@pytest.mark.parametrize("color_hash", [0, 1])
@pytest.mark.parametrize("size,camera", [((64, 48), "main"), ((37, 23), "main"), ((37, 23), "low")])
def test_whole_frames(size, camera, color_hash):
    """3 spp, depth 6: the only place the fuzz of k_prep_materials and the metal branch's absorption run (the query does not
    report fuzz).  Every entry of KERNELS under the reference walk with all seven counters, the chunked walk and the
    library's own tree with the counters that do not depend on the walk."""
    s = es.texture_edges_scene(size[0], size[1], 3, 6, color_hash=color_hash, camera=camera)
    assert len(s.bvh_nodes) > 1
    o_acc, _, o_rgba, o_st = _oracle.render(s)
    assert np.isfinite(o_acc).all()   # NaN payloads are outside the numerics contract
    for kernel in KERNELS:
        pixels, acc, st, _ = _render(s, kernel=kernel, reference_walk=True)
        assert np.array_equal(_u32(acc), _u32(o_acc)), kernel
        assert np.array_equal(pixels, o_rgba), kernel
        for k in STAT_KEYS:
            assert st[k] == o_st[k], (kernel, k, st[k], o_st[k])
    for kw, name in ((dict(), "k_trace_chunk"), (dict(host_bvh=True), "k_trace_fast")):
        pixels, acc, st, kname = _render(s, **kw)
        assert kname == name
        assert np.array_equal(_u32(acc), _u32(o_acc)), name
        assert np.array_equal(pixels, o_rgba), name
        assert st["segments"] == o_st["segments"] and st["paths"] == o_st["paths"], name


def test_texture_updates_leave_nothing_stale():
    """Change::update of the textures to fewer (3: indices 3..6 of the scene are now out of range, every offset moves), then to
    more (9, other sizes), then an update of the uniforms alone (textures are Keep): records and a 2-spp frame equal a fresh
    engine's on the resulting scene, and the oracle's."""
    cur = es.texture_edges_scene(64, 48, 2, 4)
    e = _engine(cur)
    try:
        for step, (texs, size) in enumerate([(es.other_textures(3), (64, 48)), (es.other_textures(9), (64, 48)), (None, (48, 40))]):
            u = cur.uniforms.copy()
            u["width"], u["height"] = size
            if texs is not None:
                cur = _copy(cur, uniforms=u, textures=texs)
                e.update(RenderConfig(uniforms=Change.update(u), textures=Change.update(texs)))
            else:
                cur = _copy(cur, uniforms=u)
                e.update(RenderConfig(uniforms=Change.update(u)))
            hits, surf = e.render_hits(surfaces=True)
            pixels, acc = e.render_current().pixels, e.read_accumulation()
            fresh = _engine(cur)
            try:
                hits_f, surf_f = fresh.render_hits(surfaces=True)
                pixels_f, acc_f = fresh.render_current().pixels, fresh.read_accumulation()
            finally:
                fresh.close()
            assert np.array_equal(hits.view(np.uint32), hits_f.view(np.uint32)) and np.array_equal(surf.view(np.uint32), surf_f.view(np.uint32)), step
            assert np.array_equal(pixels, pixels_f) and np.array_equal(_u32(acc), _u32(acc_f)), step
            o_acc, _, o_rgba, _ = _oracle.render(cur)
            assert np.isfinite(o_acc).all()
            assert np.array_equal(_u32(acc), _u32(o_acc)) and np.array_equal(pixels, o_rgba), step
            O, D = pixel_centre_rays(cur)
            check_records(cur, O, D, hits, surf, f"update step {step}")
            tri = hits["kind"] == abi.HIT_TRIANGLE
            # the frame sees textured triangles whose index is in range and (with three textures) ones whose index no longer is
            tex = surf["texture_index"][tri]
            assert ((tex >= 0) & (tex < len(cur.textures))).sum() > 20 and (step != 0 or (tex >= 3).sum() > 50)
    finally:
        e.close()


def test_empty_and_null_textures_are_refused_before_any_launch():
    """width 0, height 0, null rgba_data: RB_ERR_INVALID_TEXTURES from validation, as the first update and as a later one; the
    engine then still answers for the scene it holds.  (Such a texture is never rendered: that is the point.)"""
    from renderbaby_amd._lib import load
    lib = load()
    s = es.texture_edges_scene(32, 24, 1, 3)
    e = _engine(s)
    try:
        before = e.render_hits(surfaces=True)
        st0 = e.stats()
        for field, value in (("width", 0), ("height", 0), ("rgba_data", None)):
            for which in (0, 2):
                rc = RenderConfig(uniforms=Change.update(s.uniforms), textures=Change.update(es.other_textures(3)))
                cfg, keep = rc.to_c()
                arr = C.cast(cfg.textures.ptr, C.POINTER(abi.Texture))
                setattr(arr[which], field, value)
                assert lib.rb_update(e._h, C.byref(cfg)) == INVALID_TEXTURES, (field, which)
                assert b"texture" in lib.rb_last_error(e._h)
                del keep
        assert e.stats() == st0
        after = e.render_hits(surfaces=True)
        assert np.array_equal(before[0].view(np.uint32), after[0].view(np.uint32)) and np.array_equal(before[1].view(np.uint32), after[1].view(np.uint32))
        o_acc, _, o_rgba, _ = _oracle.render(s)
        assert np.array_equal(e.render_current().pixels, o_rgba) and np.array_equal(_u32(e.read_accumulation()), _u32(o_acc))
    finally:
        e.close()
    # as the engine's first scene: rb_create_ex refuses it
    bad = _copy(s, textures=[(0, 4, np.zeros(4, np.uint32))] + list(s.textures[1:]))
    with pytest.raises(RenderError, match="texture 0 is empty") as ei:
        _engine(bad)
    assert ei.value.code == INVALID_TEXTURES
