"""The once-per-iteration half of a segment in the single-node kernels (segment_post<.., TRIM> in rb_device_shade.hpp), whose four
normalizes -- the unit vector, the sphere or light normal, the scatter's operand, the new direction -- go through normalize_trim.
Per lane these are the operations they were, so everything below is bit for bit against the oracle: accumulation words, RGBA8,
segment and path counts.  16 x 16 and 24 x 16 frames of the one-node Cornell box under a blue sky, 4 samples, depth 8, each through
the staged k_trace (reservations of 256 items) and through k_trace_direct (reservations of 64), and on the same engine again
after an rb_update that hands every sphere, mesh and light the material of its neighbour:
 * one sphere, then 8 (plastic, metal and mirror lanes in one wave);
 * metal spheres only, fuzz 0 and fuzz 1 in turn (shininess 1000 and 0);
 * a point light that wins: the light's normal site, which no other scene here enters;
 * a point light with the centre and radius of a sphere: equal t, the sphere stays the winner;
 * the box's triangles with a texture (the other scenes have them without one);
 * colour-hash mode;
 * max_depth 1.
test_the_frames_hold_the_cases shows from the oracle alone that the frames reach those cases.

Not here: a scatter whose normal + ruv is near zero (every |component| < 1e-8).  No frame reaches it: a unit vector's components
are quotients of coordinates on a 2^-24 grid, so one below 1e-8 in magnitude is exactly 0 or has a coordinate of at most 6e-8
times its length, and cancelling an axis-aligned normal takes two zero coordinates in one try, cancelling a sphere's normal a
match to 1e-8 in two components -- neither occurs in frames of this size.  The normalize of vectors down there is held by
tests/test_gpu_normalize_sites.py."""
import dataclasses

import numpy as np
import pytest

from renderbaby_amd import Engine, RenderConfig, abi, scenes
from tests import _oracle

pytestmark = pytest.mark.gpu

SKY = (0.5, 0.7, 1.0)
FRAMES = {"16x16": (16, 16), "24x16": (24, 16)}
DISPATCH = {"staged": dict(queue_batch=256), "direct": dict(queue_batch=64)}
SPP, DEPTH = 4, 8
CASES = ("one", "eight", "metal", "light", "equal_t", "textured", "hash", "depth1")

_cache = {}


def _light(center, radius, emissive=(2.0, 3.0, 4.0)):
    lt = np.zeros(1, dtype=abi.POINT_LIGHT)
    lt[0]["center"], lt[0]["radius"] = center, radius
    lt[0]["material"] = scenes.material(diffuse=(0.7, 0.6, 0.5), emissive=emissive)
    return lt


def _scene(case, w, h, swapped=False, without=None, emissive=(2.0, 3.0, 4.0)):
    s = scenes.cornell(w, h, SPP, 1 if case == "depth1" else DEPTH)
    u = s.uniforms.copy()
    u["sky_color"] = SKY
    sph, lights, meshes, uvs, textures = s.spheres.copy(), s.lights, s.meshes.copy(), s.uvs, s.textures
    if case == "one":
        sph = sph[:1]
    elif case == "metal":
        for k in range(len(sph)):
            col = np.array([0.4 + 0.07 * k, 0.9 - 0.06 * k, 0.6], np.float32)
            sph[k]["material"] = scenes.material(diffuse=(0, 0, 0), specular=col, shininess=1000.0 if k % 2 else 0.0)
    elif case == "light":
        lights = _light((0.9, 3.4, -2.6), 0.45, emissive)
    elif case == "equal_t":
        lights = _light(tuple(sph[0]["center"]), float(sph[0]["radius"]), emissive)
    elif case == "textured":
        textures = [scenes.checker_texture()]
        uvs = np.random.default_rng(27).uniform(-1.5, 2.5, len(s.uvs)).astype(np.float32)
        meshes["material"]["texture_index"] = 0
    elif case == "hash":
        u["color_hash_enabled"] = 1
    if without == "spheres":
        sph = sph[:0]
    elif without == "sphere0":
        sph = sph[1:]
    elif without == "lights":
        lights = lights[:0]
    if swapped:   # everything takes its neighbour's material; a light trades its emission's channels
        sph["material"] = np.roll(sph["material"], 1)
        tex = meshes["material"]["texture_index"].copy()
        meshes["material"] = np.roll(meshes["material"], 1)
        meshes["material"]["texture_index"] = tex
        if len(lights):
            lights = lights.copy()
            lights["material"]["emissive"] = lights["material"]["emissive"][:, ::-1]
    u["spheres_count"] = len(sph)
    return dataclasses.replace(s, uniforms=u, spheres=sph, lights=lights, meshes=meshes, uvs=uvs, textures=textures)


def _want(case, frame, **kw):
    """the oracle's frame, rendered once per module and never written to"""
    key = (case, frame, tuple(sorted(kw.items())))
    if key not in _cache:
        s = _scene(case, *FRAMES[frame], **kw)
        acc, _, rgba, st = _oracle.render(s)
        for a in (acc, rgba):
            a.setflags(write=False)
        _cache[key] = (s, acc, rgba, st)
    return _cache[key]


def _same(e, rc, want, what):
    _, o_acc, o_rgba, o_st = want
    e.reset_stats()
    px = e.render(rc).pixels
    acc, st = e.read_accumulation(), e.stats()
    assert e.last_kernel_name() == "k_trace", what
    assert np.array_equal(acc.view(np.uint32), o_acc.view(np.uint32)), what
    assert np.array_equal(px, o_rgba), what
    assert st["segments"] == o_st["segments"] and st["paths"] == o_st["paths"], (what, st, o_st)


@pytest.mark.parametrize("dispatch", list(DISPATCH))
@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("case", CASES)
def test_frame_and_counters_before_and_after_an_update(case, frame, dispatch):
    first, second = _want(case, frame), _want(case, frame, swapped=True)
    rc = RenderConfig.from_scene(first[0])
    e = Engine.new(rc, **DISPATCH[dispatch])
    try:
        _same(e, rc, first, (case, frame, dispatch, "first upload"))
        _same(e, RenderConfig.from_scene(second[0], create=False), second, (case, frame, dispatch, "after the update"))
    finally:
        e.close()


def test_the_frames_hold_the_cases():
    for frame in FRAMES:
        rgba = lambda case, **kw: _want(case, frame, **kw)[2]
        stats = lambda case, **kw: _want(case, frame, **kw)[3]
        # sphere winners, one and eight; the update changes what they look like
        assert not np.array_equal(rgba("one"), rgba("one", without="spheres"))
        assert not np.array_equal(rgba("eight"), rgba("one"))
        for case in CASES:
            assert not np.array_equal(rgba(case), rgba(case, swapped=True)), (case, frame)
        # metal scatters: fuzz enters only there, and the metal set absorbs paths the seeded set keeps
        assert stats("metal")["paths"] == stats("eight")["paths"] and stats("metal")["segments"] != stats("eight")["segments"]
        # the light wins somewhere: its emission shows
        assert not np.array_equal(rgba("light"), rgba("light", emissive=(4.0, 2.0, 1.0)))
        # equal t: the sphere in front of the light's copy of it stays the winner -- the light changes nothing, the sphere does
        assert np.array_equal(rgba("equal_t"), rgba("equal_t", without="lights"))
        assert np.array_equal(rgba("equal_t"), rgba("equal_t", emissive=(4.0, 2.0, 1.0)))
        assert not np.array_equal(rgba("equal_t"), rgba("equal_t", without="sphere0"))
        # the texture and the colour hash reach the triangles' albedo
        assert not np.array_equal(rgba("textured"), rgba("eight")) and not np.array_equal(rgba("hash"), rgba("eight"))
        assert stats("eight")["mesh_hits"] > 0
        # max_depth 1: one segment a path
        assert stats("depth1")["segments"] == stats("depth1")["paths"]
