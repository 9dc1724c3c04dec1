"""The linear sphere scan of the single-node kernels (segment_spheres<.., LEAN> in rb_device_shade.hpp): pass 1 walks a
32-sphere block from its last sphere to its first, shifts each sphere's bit in at the bottom of the lane's mask and reads
{centre, radius^2} from 16-byte scan records that rb_update makes; pass 2 walks the mask upwards as before.  Per lane these
are the operations of the ascending scan, so everything below is bit for bit against the oracle -- accumulation words,
RGBA8, segment and path counts:
 * 16 x 16 frames at 3 samples and depth 4 with 1, 2, 31, 32, 33 and 64 spheres -- the ends of the scan's blocks and the
   kernel's limit -- under a sky alone and inside the one-node Cornell box, in two layouts: `spread`, a grid of spheres of
   distinct colours, and `pairs`, the same grid with the spheres at indices 1, 32 and n - 1 moved onto their predecessors
   (same centre, same radius, another colour), through the staged k_trace and through k_trace_direct;
 * test_the_frames_hold_the_cases proves from the oracle alone that in `spread` every index is some pixel's winner (the
   frame changes when that sphere is taken away), and that in `pairs` the lower index of a coincident pair wins (taking
   the upper one away changes nothing, taking the lower one away does);
 * after an rb_update that moves a sphere and changes a radius the frame is the oracle's frame of the new scene, which a
   scan record left over from the first upload would not give;
 * the 8-wave instantiations, which only launches of 3 * 2^23 items or more take: one 1024 x 768 frame at 32 samples with
   the 64 spheres of `pairs` in the box through each, of which the oracle renders two windows;
 * rcp_det, the reciprocal of the single-node triangle test with its two-compare guard, against 1.0f / x on all 2^23
   significands and both signs at the biased exponents 107 (the reference's 1e-6 rejection sits there), 127, 226 and 227
   (either side of the guard's 2^100), 254 and 255 (infinities and NaNs; a NaN equals a NaN)."""
import dataclasses

import numpy as np
import pytest

from renderbaby_amd import Engine, RenderConfig, _lib, abi, scenes
from tests import _oracle

pytestmark = pytest.mark.gpu

SKY = (0.5, 0.7, 1.0)
COUNTS = (1, 2, 31, 32, 33, 64)
LAYOUTS = ("spread", "pairs")
DISPATCH = {"staged": dict(queue_batch=256), "direct": {}}
W = H = 16
SPP, DEPTH = 3, 4

_cache = {}


def _pairs(n):
    """upper indices of the coincident pairs (0, 1), (31, 32), (n - 2, n - 1) that exist among n spheres"""
    return sorted({j for j in (1, 32, n - 1) if 1 <= j < n})


def _spheres(n, layout):
    """n spheres on a g x g grid (g = ceil(sqrt(n))) in the plane z = -3, which the camera of the Cornell scenes sees whole
    inside the box; radius 0.42 of the pitch, every third one a little nearer so that the mask's bits do not arrive in
    depth order; plastic, metal and mirror in turn, a colour per index"""
    g = int(np.ceil(np.sqrt(n)))
    pitch = 4.4 / g
    sph = np.zeros(n, dtype=abi.SPHERE)
    for k in range(n):
        i, j = k % g, k // g
        sph[k]["center"] = (-2.2 + (i + 0.5) * pitch, 0.8 + (j + 0.5) * pitch, -3.0 + 0.3 * (k % 3))
        sph[k]["radius"] = 0.42 * pitch
        col = (0.25 + 0.7 * ((k * 37) % 64) / 63.0, 0.25 + 0.7 * ((k * 11) % 64) / 63.0, 0.25 + 0.7 * ((k * 23) % 64) / 63.0)
        sph[k]["material"] = scenes.sphere_material(("plastic", "plastic", "metal", "mirror")[k % 4], col)
    if layout == "pairs":
        for j in _pairs(n):
            sph[j]["center"] = sph[j - 1]["center"]
            sph[j]["radius"] = sph[j - 1]["radius"]
    return sph


def _scene(n, layout, mesh, w=W, h=H, spp=SPP, depth=DEPTH, without=None, moved=False):
    s = scenes.cornell(w, h, spp, depth)
    u = s.uniforms.copy()
    u["sky_color"] = SKY
    u["camera"]["pane_width"] = 21.0   # at the grid's depth the frame is 4.8 wide: a sphere of the 8 x 8 grid covers a pixel and a half of 16
    sph = _spheres(n, layout)
    if moved:   # what the rb_update of test_update_remakes_the_scan_records changes: one centre, one radius
        sph[0]["center"] = sph[0]["center"] + np.array((0.35, -0.3, 0.4), dtype=np.float32)
        sph[n - 1]["radius"] = sph[n - 1]["radius"] * np.float32(1.6)
    if without is not None:
        sph = np.delete(sph, without)
    u["spheres_count"] = len(sph)
    if not mesh:
        u["bvh_node_count"] = u["bvh_triangle_count"] = 0
        return dataclasses.replace(s, uniforms=u, spheres=sph, meshes=s.meshes[:0], bvh_nodes=s.bvh_nodes[:0], bvh_indices=s.bvh_indices[:0],
                                   bvh_triangles=s.bvh_triangles[:0], uvs=s.uvs[:0])
    return dataclasses.replace(s, uniforms=u, spheres=sph)


def _want(n, layout, mesh, **kw):
    """the oracle's frame, rendered once per module and never written to"""
    key = (n, layout, mesh, tuple(sorted(kw.items())))
    if key not in _cache:
        s = _scene(n, layout, mesh, **kw)
        acc, _, rgba, st = _oracle.render(s)
        for a in (acc, rgba):
            a.setflags(write=False)
        _cache[key] = (s, acc, rgba, st)
    return _cache[key]


def _same(e, frame, want, what):
    o_acc, o_rgba, o_st = want
    st = e.stats()
    assert e.last_kernel_name() == "k_trace", what
    assert np.array_equal(e.read_accumulation().view(np.uint32), o_acc.view(np.uint32)), what
    assert np.array_equal(frame.pixels, o_rgba), what
    assert st["segments"] == o_st["segments"] and st["paths"] == o_st["paths"], (what, st, o_st)


@pytest.mark.parametrize("dispatch", list(DISPATCH))
@pytest.mark.parametrize("mesh", (False, True), ids=("sky", "box"))
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", COUNTS)
def test_frame_and_counters(n, layout, mesh, dispatch):
    s, *want = _want(n, layout, mesh)
    rc = RenderConfig.from_scene(s)
    e = Engine.new(rc, **DISPATCH[dispatch])
    try:
        _same(e, e.render(rc), want, (n, layout, mesh, dispatch))
    finally:
        e.close()


@pytest.mark.parametrize("mesh", (False, True), ids=("sky", "box"))
@pytest.mark.parametrize("n", (2, 33))
def test_counting_instantiation(n, mesh):
    s, *want = _want(n, "pairs", mesh)
    rc = RenderConfig.from_scene(s)
    e = Engine.new(rc, stats=True, **DISPATCH["staged"])
    try:
        _same(e, e.render(rc), want, (n, mesh))
        assert e.stats()["spheres_tested"] == want[2]["spheres_tested"]
    finally:
        e.close()


@pytest.mark.parametrize("mesh", (False, True), ids=("sky", "box"))
@pytest.mark.parametrize("n", COUNTS)
def test_the_frames_hold_the_cases(n, mesh):
    whole = _want(n, "spread", mesh)[1]
    for k in range(n):   # every index wins somewhere: without it the frame is another one
        assert not np.array_equal(whole, _oracle.render(_scene(n, "spread", mesh, without=k))[0]), (n, mesh, k)
    whole = _want(n, "pairs", mesh)[1]
    for j in _pairs(n):
        # the upper sphere of a coincident pair is never the winner (a strict `<` in ascending order) ...
        assert np.array_equal(whole, _oracle.render(_scene(n, "pairs", mesh, without=j))[0]), (n, mesh, j)
        # ... and the lower one is: its twin's colour shows once it is gone
        assert not np.array_equal(whole, _oracle.render(_scene(n, "pairs", mesh, without=j - 1))[0]), (n, mesh, j - 1)


@pytest.mark.parametrize("dispatch", list(DISPATCH))
@pytest.mark.parametrize("n", (2, 33, 64))
def test_update_remakes_the_scan_records(n, dispatch):
    first, after = _want(n, "spread", True), _want(n, "spread", True, moved=True)
    assert not np.array_equal(first[1], after[1])
    rc = RenderConfig.from_scene(first[0])
    e = Engine.new(rc, **DISPATCH[dispatch])
    try:
        _same(e, e.render(rc), first[1:], (n, dispatch, "first"))
        e.reset_stats()
        _same(e, e.render(RenderConfig.from_scene(after[0], create=False)), after[1:], (n, dispatch, "updated"))
    finally:
        e.close()


@pytest.mark.parametrize("batch", (256, 64), ids=("staged", "direct"))
def test_eight_wave_instantiations(batch):
    # 1024 x 768 pixels at 32 samples are 128 x 96 tiles x 64 x 32 = 3 * 2^23 items in one launch: the 8-wave instantiation.  The
    # oracle renders two windows of it (pixels do not depend on one another): one over the grid's middle, where spheres 31 and
    # 32 lie, one in a corner
    w, h, spp = 1024, 768, 32
    assert (w // 8) * (h // 8) * 64 * spp >= 3 << 23
    s = _scene(64, "pairs", True, w=w, h=h, spp=spp)
    rc = RenderConfig.from_scene(s)
    e = Engine.new(rc, queue_batch=batch)
    try:
        e.render(rc)
        acc = e.read_accumulation()
        assert e.last_kernel_name() == "k_trace"
    finally:
        e.close()
    for (r0, r1), (c0, c1) in (((380, 384), (480, 544)), ((0, 2), (0, 32))):
        o_acc = _oracle.render(s, rows=(r0, r1), cols=(c0, c1))[0]
        assert np.array_equal(acc[r0:r1, c0:c1].view(np.uint32), o_acc[r0:r1, c0:c1].view(np.uint32)), (batch, r0, c0)


@pytest.mark.parametrize("expo", (107, 127, 226, 227, 254, 255))
def test_rcp_det_exhaustive(expo):
    out = np.zeros(16, dtype=np.uint32)
    assert _lib.load().rb_debug_rcp_det_exhaustive(expo, out.ctypes.data) == 0
    assert out[0] == 0, (expo, [hex(int(x)) for x in out[1:1 + min(int(out[0]), 15)]])
