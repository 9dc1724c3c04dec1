"""The scatter of a segment (segment_post in rb_device_shade.hpp) after its two normalize sites were folded into one: the metal
branch normalized d, the lambert branch normal + ruv, a lane takes one of them and the wave paid for both; now one
normalize of the lane's own operand stands in front of the branch.  Per lane these are the same operations on the same
values, so everything below is bit for bit against the oracle -- accumulation words, RGBA8, segment and path counts:
 * the frames of tests/test_gpu_path_state.py -- 64 x 40 with reservations of 256 items for the staged k_trace, 9 x 7 for
   k_trace_direct -- at max_depth 1, 2, 8 and 1 and 3 samples under a blue sky, with four sphere sets: the seeded one (metal,
   mirror and plastic lanes in one wave, so the shared normalize selects per lane), all metal, none metal, and the seeded
   one with a point light in the box, so that K_LIGHT loads a material and scatters;
 * test_the_frames_hold_the_cases proves from the oracle alone that those frames hold what they are meant to: metal
   scatters that go on, paths absorbed on metal, sphere, triangle and light winners;
 * one small frame through every other kernel that shades through segment_post -- the chunked walk, the reference walk
   (from LDS and through L2), the library's own tree, the per-segment ablation, on the 578-triangle mesh of the golden set;
   the sphere walk on 66 spheres; k_queue and k_pixel -- plain and counting: some instantiations keep the two sites
   (rb_kernels.hip says which), the frame is the same either way;
 * the 8-wave instantiations of k_trace and k_trace_direct, which only launches of 3 * 2^23 items or more take (the
   flagship's): one such frame each, 1024 x 768 at 32 samples -- about 10^8 segments, under a tenth of a second on an
   MI355X with the engine's set-up -- of which the oracle renders two small windows (10 000 paths).
The ground, colour-hash and texture paths through the same code are held by tests/test_gpu_shading_edges.py."""
import dataclasses
import os

import numpy as np
import pytest

from renderbaby_amd import Engine, RenderConfig, abi, scenes
from tests import _oracle

pytestmark = pytest.mark.gpu

SKY = (0.5, 0.7, 1.0)
FRAMES = {"staged-64x40": (64, 40, dict(queue_batch=256)), "direct-9x7": (9, 7, {})}
DEPTHS = (1, 2, 8)
SPPS = (1, 3)
SETS = ("seeded", "metal", "plastic", "light")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mesh578_32x20_2spp.npz")

_cache = {}


def _scene(w, h, spp, depth, spheres="seeded", tint=1.0, light_emissive=(2.0, 3.0, 4.0), no_spheres=False):
    s = scenes.cornell(w, h, spp, depth)
    u = s.uniforms.copy()
    u["sky_color"] = SKY
    sph = s.spheres.copy()
    for k in range(len(sph)):
        col = np.float32(tint) * np.array([0.3 + 0.08 * k, 0.9 - 0.07 * k, 0.5], dtype=np.float32)
        if spheres == "metal":
            sph[k]["material"] = scenes.sphere_material("metal" if k % 2 else "mirror", col)
        elif spheres == "plastic":
            sph[k]["material"] = scenes.sphere_material("plastic", col)
        elif tint != 1.0 and k % 4 in (1, 2):   # the seeded set's metal and mirror spheres in another colour
            sph[k]["material"]["specular"] = np.float32(tint) * sph[k]["material"]["specular"]
    if no_spheres:
        sph = sph[:0]
    lights = s.lights
    if spheres == "light":
        lights = np.zeros(1, dtype=abi.POINT_LIGHT)
        lights[0]["center"] = (0.9, 3.4, -2.6)
        lights[0]["radius"] = 0.45
        lights[0]["material"] = scenes.material(diffuse=(0.7, 0.6, 0.5), emissive=light_emissive)
    u["spheres_count"] = len(sph)
    return dataclasses.replace(s, uniforms=u, spheres=sph, lights=lights)


def _want(w, h, spp, depth, **kw):
    """the oracle's frame, rendered once per module and never written to"""
    key = (w, h, spp, depth, tuple(sorted(kw.items())))
    if key not in _cache:
        s = _scene(w, h, spp, depth, **kw)
        acc, _, rgba, st = _oracle.render(s)
        for a in (acc, rgba):
            a.setflags(write=False)
        _cache[key] = (s, acc, rgba, st)
    return _cache[key]


def _render(s, **engine_kw):
    rc = RenderConfig.from_scene(s)
    e = Engine.new(rc, **engine_kw)
    try:
        f = e.render(rc)
        return e.read_accumulation(), f.pixels, e.stats(), e.last_kernel_name()
    finally:
        e.close()


def _same(got, want, what):
    acc, px, st, _ = got
    o_acc, o_rgba, o_st = want
    assert np.array_equal(acc.view(np.uint32), o_acc.view(np.uint32)), what
    assert np.array_equal(px, o_rgba), what
    assert st["segments"] == o_st["segments"] and st["paths"] == o_st["paths"], (what, st, o_st)


@pytest.mark.parametrize("spp", SPPS)
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("spheres", SETS)
@pytest.mark.parametrize("frame", list(FRAMES))
def test_frame_and_counters(frame, spheres, depth, spp):
    w, h, kw = FRAMES[frame]
    s, *want = _want(w, h, spp, depth, spheres=spheres)
    got = _render(s, **kw)
    assert got[3] == "k_trace"
    _same(got, want, (frame, spheres, depth, spp))


@pytest.mark.parametrize("spheres", ("seeded", "light"))
@pytest.mark.parametrize("frame", list(FRAMES))
def test_counting_instantiation(frame, spheres):
    w, h, kw = FRAMES[frame]
    s, *want = _want(w, h, 3, 8, spheres=spheres)
    _same(_render(s, stats=True, **kw), want, (frame, spheres))


def test_the_frames_hold_the_cases():
    for w, h, _ in FRAMES.values():
        seeded = _want(w, h, 3, 8, spheres="seeded")
        # triangle winners: the box's triangles are hit
        assert seeded[3]["mesh_hits"] > 0
        # sphere winners: without the spheres the same rays give another frame
        assert not np.array_equal(seeded[1], _want(w, h, 3, 8, spheres="seeded", no_spheres=True)[1]), (w, h)
        # metal scatters that go on: the specular colour only enters a path's attenuation when the metal branch scatters
        # (an absorbed path returns before), and only shows if the path then reaches the sky or the lamp
        assert not np.array_equal(seeded[1], _want(w, h, 3, 8, spheres="seeded", tint=0.5)[1]), (w, h)
        # light winners: the light's emission is added only where the light is the closest hit
        lit = _want(w, h, 3, 8, spheres="light")
        assert not np.array_equal(lit[1], _want(w, h, 3, 8, spheres="light", light_emissive=(4.0, 2.0, 1.0))[1]), (w, h)
        assert lit[3]["lights_tested"] == lit[3]["segments"]
    # absorbed on metal: the first segments of a frame do not depend on the materials, so at depth 2 the plastic set ends
    # in its first segment only on the sky; the metal sets lose more paths there
    w, h, _ = FRAMES["staged-64x40"]
    plastic = _want(w, h, 3, 2, spheres="plastic")[3]
    for name in ("seeded", "metal"):
        st = _want(w, h, 3, 2, spheres=name)[3]
        assert st["paths"] == plastic["paths"] and st["segments"] < plastic["segments"], (name, st, plastic)
    # ... and the all-metal set more than the seeded one, whose plastic spheres absorb nothing
    assert _want(w, h, 3, 2, spheres="metal")[3]["segments"] < _want(w, h, 3, 2, spheres="seeded")[3]["segments"]


MESH_WALKS = [(dict(), "k_trace_chunk"), (dict(reference_walk=True), "k_trace_bvh_lds"), (dict(reference_walk=True, lds_mode=1), "k_trace_bvh"),
              (dict(host_bvh=True), "k_trace_fast"), (dict(no_leaf_stepping=True), "k_trace")]


@pytest.mark.parametrize("stats", (False, True), ids=("plain", "counting"))
@pytest.mark.parametrize("kw,name", MESH_WALKS, ids=[n + ("" if i != 4 else "_multi") for i, (_, n) in enumerate(MESH_WALKS)])
def test_mesh_walks(kw, name, stats):
    s, acc, rgba, st = _oracle.load_golden(GOLDEN)
    got = _render(s, stats=stats, **kw)
    assert got[3] == name
    _same(got, (acc, rgba, st), (name, stats))


@pytest.mark.parametrize("stats", (False, True), ids=("plain", "counting"))
@pytest.mark.parametrize("tree", (None, "host"))
def test_sphere_walk(tree, stats):
    key = "balls"
    if key not in _cache:
        s = scenes.spheres_scene(n=66, width=32, height=24, spp=2, max_depth=5, extent=4.0)
        acc, _, rgba, st = _oracle.render(s)
        _cache[key] = (s, acc, rgba, st)
    s, *want = _cache[key]
    got = _render(s, stats=stats, **({} if tree is None else dict(sphere_tree=tree)))
    assert got[3] == "k_trace_sph"
    _same(got, want, (tree, stats))


@pytest.mark.parametrize("stats", (False, True), ids=("plain", "counting"))
@pytest.mark.parametrize("spheres", ("seeded", "light"))
@pytest.mark.parametrize("kernel,name", [(abi.KERNEL_QUEUE, "k_queue"), (abi.KERNEL_PIXEL, "k_pixel")], ids=("k_queue", "k_pixel"))
def test_queue_and_pixel_kernels(kernel, name, spheres, stats):
    w, h, _ = FRAMES["staged-64x40"]
    s, *want = _want(w, h, 3, 8, spheres=spheres)
    got = _render(s, kernel=kernel, stats=stats)
    assert got[3] == name
    _same(got, want, (name, spheres, stats))


@pytest.mark.parametrize("batch", (256, 64), ids=("staged", "direct"))
def test_eight_wave_instantiations(batch):
    # 1024 x 768 pixels at 32 samples are 128 x 96 tiles x 64 x 32 = 3 * 2^23 items in one launch: the 8-wave instantiation.  The
    # oracle renders two windows of it (pixels do not depend on one another): one over the spheres, one in a corner
    w, h, spp = 1024, 768, 32
    assert (w // 8) * (h // 8) * 64 * spp >= 3 << 23
    s = _scene(w, h, spp, 8, spheres="light")
    rc = RenderConfig.from_scene(s)
    e = Engine.new(rc, queue_batch=batch)
    try:
        e.render(rc)
        acc = e.read_accumulation()
        assert e.last_kernel_name() == "k_trace"
    finally:
        e.close()
    for (r0, r1), (c0, c1) in (((440, 444), (380, 444)), ((0, 2), (0, 32))):
        o_acc = _oracle.render(s, rows=(r0, r1), cols=(c0, c1))[0]
        assert np.array_equal(acc[r0:r1, c0:c1].view(np.uint32), o_acc[r0:r1, c0:c1].view(np.uint32)), (batch, r0, c0)
