"""The flat kernels of k_trace's plain walk, k_trace_flat and k_trace_flat_direct ("Scenes that carry no
u, v"): a scene whose mesh and sphere materials have no texture -- and, with the ground on, whose lights have none either --
runs kernels that carry {t, slot} through the triangle loop and have no tri_uv and no texel lookup.  Held here, bit for bit:
 * the debug sweep: the flat trip against the compiler-laid triangle test on seeded and constructed triples;
 * frames against the oracle and against the kernels with u, v of the same build (RB_TRACE_UV=1): the direct form, the staged
   form, and one launch of 3 * 2^23 items for the 8-wave instantiation;
 * the edges of the fact, each against the oracle with the kernel that ran asserted: the ground's checkerboard without a
   texture, the colour hash, a textured sphere in front of an untextured wall, a textured light with and without the
   ground, a mesh material whose index is past the textures;
 * updates on one engine that move the scene across the fact and back, against a fresh engine at each step."""
import contextlib
import dataclasses
import os

import numpy as np
import pytest

from renderbaby_amd import Change, Engine, RenderConfig, _lib, abi, scenes
from tests import _oracle

pytestmark = pytest.mark.gpu

FLAT, BIG, STAGED = abi.TRACE_FORM_FLAT, abi.TRACE_FORM_BIG, abi.TRACE_FORM_STAGED


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


@contextlib.contextmanager
def _forced_uv(on):
    """RB_TRACE_UV=1 while an engine is made: that engine keeps the kernels with u, v"""
    old = os.environ.get("RB_TRACE_UV")
    if on:
        os.environ["RB_TRACE_UV"] = "1"
    try:
        yield
    finally:
        if on:
            if old is None:
                del os.environ["RB_TRACE_UV"]
            else:
                os.environ["RB_TRACE_UV"] = old


def _render(scene, forced=False, **kw):
    rc = RenderConfig.from_scene(scene)
    with _forced_uv(forced):
        e = Engine.new(rc, **kw)
    try:
        px = e.render(rc).pixels
        st = e.stats()
        assert e.last_kernel_name() == "k_trace"
        return _u32(e.read_accumulation()), px, (st["segments"], st["paths"]), e.trace_form()
    finally:
        e.close()


def _against_oracle(scene, form, mask=FLAT, rows=None, **kw):
    """the frame of `scene` is the oracle's, and the kernel that ran has `form` among the bits of `mask`"""
    acc, px, counts, got = _render(scene, **kw)
    assert got & mask == form, (got, form)
    o_acc, _, o_rgba, o_st = _oracle.render(scene, rows=rows)
    r0, r1 = rows if rows else (0, scene.height)
    assert np.array_equal(acc[r0:r1], _u32(o_acc)[r0:r1]), "accumulation"
    assert np.array_equal(px[r0:r1], o_rgba[r0:r1]), "frame"
    if rows is None:
        assert counts == (o_st["segments"], o_st["paths"])
    return acc, px, counts, o_st


# ------------------------------------------------------------------------------------ the sweep ---
@pytest.mark.parametrize("seed", [1, 20240917, 0xFFFFFFFF])
def test_flat_trip_equals_the_compiler_laid_form(seed):
    # the edges tests/test_gpu_triangle_trip.py sweeps (rb_debug.hip, trip_case): det at and beside 1e-6 and 2^100 and with the low
    # half all ones, u, v, u + v, t at and next to their bounds, t == hit.t, NaN and infinity in o and d, lanes off on entry
    out = np.zeros(32, dtype=np.uint32)
    assert _lib.load().rb_debug_triangle_trip_flat(1 << 20, seed, out.ctypes.data) == 0
    assert out[0] == 0, ("triples that differ", int(out[0]), "one of them", int(out[1]), out[2:18].view(np.float32),
                         "trip", out[18:22], "accept_slot", out[22:26])


# ------------------------------------------------------- frames: the oracle, and the kernels with u, v ---
def _both(scene, form, rows=None, **kw):
    acc, px, counts, _ = _against_oracle(scene, form, mask=FLAT | BIG | STAGED, rows=rows, **kw)
    f_acc, f_px, f_counts, f_form = _render(scene, forced=True, **kw)
    assert f_form == form & (BIG | STAGED), (f_form, form)          # the same shape of launch, the kernels with u, v
    assert np.array_equal(acc, f_acc) and np.array_equal(px, f_px) and counts == f_counts


def test_direct_form_six_waves():
    _both(scenes.cornell(40, 24, 3, 8), FLAT)


def test_staged_form_six_waves():
    _both(scenes.cornell(203, 77, 6, 5), FLAT | STAGED, queue_batch=256)


def test_eight_wave_instantiation():
    w, h, spp, depth = 256, 192, 512, 2
    assert (w // 8) * (h // 8) * 64 * spp >= 3 << 23
    _both(scenes.cornell(w, h, spp, depth), FLAT | BIG | STAGED, rows=(92, 100))


def test_forced_engines_do_not_leak_the_variable():
    assert "RB_TRACE_UV" not in os.environ
    assert _render(scenes.cornell(16, 8, 1, 2))[3] & FLAT


# ---------------------------------------------------------------------------- the edges of the fact ---
W, H, SPP, DEPTH = 40, 24, 3, 5


def _feature(mesh_tex=-1, sphere_tex=-1, light_tex=-1, **kw):
    """scenes.feature_scene -- ground with the checkerboard, a quad with uvs, five spheres, two lights, one 8 x 4 texture -- with
    the three texture indices of its materials set"""
    s = scenes.feature_scene(W, H, SPP, DEPTH, **kw)
    meshes, spheres, lights = s.meshes.copy(), s.spheres.copy(), s.lights.copy()
    meshes["material"]["texture_index"][0] = mesh_tex
    spheres["material"]["texture_index"][3] = sphere_tex
    lights["material"]["texture_index"][0] = light_tex
    return dataclasses.replace(s, meshes=meshes, spheres=spheres, lights=lights)


def _with_uniforms(s, **kw):
    u = s.uniforms.copy()
    for k, v in kw.items():
        u[k] = v
    return dataclasses.replace(s, uniforms=u)


def test_ground_checkerboard_without_a_texture():
    s = _feature()
    acc = _against_oracle(s, FLAT)[0]
    plain = _u32(_oracle.render(_with_uniforms(s, checkerboard_enabled=0))[0])
    assert (acc != plain).any(-1).mean() > 0.1, "the ground's uv is not used"


def test_colour_hash():
    _against_oracle(_feature(color_hash=1), FLAT)


def test_textured_sphere_in_front_of_an_untextured_wall():
    # a wall with uvs and no texture behind a textured lambert sphere: where the sphere wins, the walk hit the wall first, and
    # the sphere's texture is sampled at the wall's uv (shader.wgsl: a sphere does not reset closest_hit.uv)
    wall = scenes._quad((-3.0, 0.0, -4.0), (3.0, 0.0, -4.0), (3.0, 6.0, -4.0), (-3.0, 6.0, -4.0))

    def make(uv):
        sp = np.zeros(1, dtype=abi.SPHERE)
        sp[0]["center"], sp[0]["radius"] = (0.0, 3.0, -1.0), 1.5
        sp[0]["material"] = scenes.material(diffuse=(0.9, 0.9, 0.9), texture_index=0)
        u = scenes.make_uniforms(W, H, SPP, 2, cam_pos=(0, 3, 5), cam_dir=(0, 0, -1), ground_enabled=0, sky=(0.5, 0.7, 1.0))
        return scenes._finish("wall", u, sp, np.zeros(0, dtype=abi.POINT_LIGHT), [(scenes.material(diffuse=(0.6, 0.6, 0.6)), wall)],
                              [uv], [scenes.checker_texture()])
    s = make([[(0, 0), (1, 0), (1, 1)], [(0, 0), (1, 1), (0, 1)]])
    acc = _against_oracle(s, 0)[0]
    other = _u32(_oracle.render(make([[(0.5, 0.5), (0.25, 0), (0, 0.75)], [(0.5, 0.5), (0, 0.75), (0.75, 1)]]))[0])
    assert (acc != other).any(-1).mean() > 0.05, "the wall's uv does not reach the sphere's texture"


@pytest.mark.parametrize("ground", [1, 0])
def test_textured_light_only(ground):
    # a light's own index is sampled where a ground hit has left use_texture set: with the ground on the lights are part of the fact
    s = _with_uniforms(_feature(light_tex=0), ground_enabled=ground)
    _against_oracle(s, 0 if ground else FLAT)


def test_mesh_index_past_the_textures():
    s = _feature(mesh_tex=5)
    assert len(s.textures) == 1
    _against_oracle(s, 0)


def test_empty_lights_leave_a_textured_phantom():
    # no lights: the buffer's one zero-filled light has texture index 0; it counts with the ground on only
    s = dataclasses.replace(_feature(), lights=np.zeros(0, dtype=abi.POINT_LIGHT))
    _against_oracle(s, 0)
    _against_oracle(_with_uniforms(s, ground_enabled=0), FLAT)


# ------------------------------------------------------------------------- updates on one engine ---
def test_updates_across_the_fact():
    base = _feature()
    textured = _feature(sphere_tex=0)
    huge = scenes._quad((-1e17, 30.0, 1e17), (1e17, 30.0, 1e17), (1e17, 30.0, -1e17), (-1e17, 30.0, -1e17))   # a lid over the scene, on the division path of the trip's reciprocal
    tris = np.concatenate([base.bvh_triangles, scenes.build_mesh_arrays([(scenes.material(), huge)])[1]])
    tris["mesh_index"][-2:] = 2
    nodes = base.bvh_nodes.copy()
    assert len(nodes) == 1
    nodes["primitive_count"][0] = len(tris)
    nodes["aabb_min"][0], nodes["aabb_max"][0] = (-1e17, -3.0, -1e17), (1e17, 30.0, 1e17)
    u = base.uniforms.copy()
    u["bvh_triangle_count"] = len(tris)
    big = dataclasses.replace(base, uniforms=u, bvh_triangles=tris, bvh_nodes=nodes, bvh_indices=np.arange(len(tris), dtype=np.uint32))
    steps = [(base, FLAT), (textured, 0), (base, FLAT), (big, FLAT), (textured, 0), (base, FLAT)]
    fresh = {}
    e = None
    try:
        for k, (s, form) in enumerate(steps):
            if id(s) not in fresh:
                fresh[id(s)] = _render(s)
                assert fresh[id(s)][3] & FLAT == form, (k, "fresh", fresh[id(s)][3])
            rc = RenderConfig.from_scene(s, create=(k == 0))
            if e is None:
                e = Engine.new(rc)
            e.reset_stats()
            px = e.render(rc).pixels
            st = e.stats()
            assert e.trace_form() & FLAT == form, (k, e.trace_form())
            want = fresh[id(s)]
            assert np.array_equal(_u32(e.read_accumulation()), want[0]) and np.array_equal(px, want[1]), k
            assert (st["segments"], st["paths"]) == want[2], k
        # a sphere material alone (with the uniforms every config carries): the other fields are kept
        sp = base.spheres.copy()
        sp["material"]["texture_index"][1] = 0
        e.update(RenderConfig(uniforms=Change.update(base.uniforms), spheres=Change.update(sp)))
        e.render_current()
        assert e.trace_form() & FLAT == 0
        e.update(RenderConfig(uniforms=Change.update(base.uniforms), spheres=Change.update(base.spheres)))
        e.render_current()
        assert e.trace_form() & FLAT == FLAT
        assert np.array_equal(_u32(e.read_accumulation()), fresh[id(base)][0])
    finally:
        if e is not None:
            e.close()
    assert len({f[0].tobytes() for f in fresh.values()}) == 3
