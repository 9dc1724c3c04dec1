"""The triangle trip of k_trace / k_trace_direct on single-node trees (intersect_bvh<.., TRIP = true> in rb_device_intersect.hpp:
the record loaded at the top of its own trip, one latch, and accept_trip, the triangle test with its exec flow laid out by
hand).  Frames, accumulation words and segment counts are the oracle's, bit for bit, where the trip could go wrong: a trip count
of one, odd and even counts, the leaf limit and the last record of the table; dead records at the first, a middle and the last
position; lanes that enter the loop switched off; an early-out that no lane passes; determinants on the division path and
below the reference's 1e-6; a table that grows and shrinks under one engine.  rb_debug_triangle_trip holds the trip to the
compiler-laid form on seeded and constructed (ray, triangle, incoming hit) triples."""
import dataclasses

import numpy as np
import pytest

from renderbaby_amd import Engine, RenderConfig, _lib, abi, scenes
from tests import _oracle

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH = 64, 32, 4, 4
STAGED, DIRECT = 256, 64          # queue_batch: whole multiples of 256 items start rows in one pass (k_trace), others are k_trace_direct
NO_SPHERES = np.zeros(0, dtype=abi.SPHERE)
NO_LIGHTS = np.zeros(0, dtype=abi.POINT_LIGHT)


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _one_node(tris):
    """every triangle in the root: the tree the single-node walk takes, whatever the count"""
    nodes = np.zeros(1, dtype=abi.BVH_NODE)
    pts = np.concatenate([tris["v0"], tris["v1"], tris["v2"]]).astype(np.float32)
    nodes["aabb_min"][0], nodes["aabb_max"][0] = pts.min(0), pts.max(0)
    nodes["left"], nodes["right"] = abi.NO_INDEX, abi.NO_INDEX
    nodes["first_primitive"], nodes["primitive_count"] = 0, len(tris)
    return nodes, np.arange(len(tris), dtype=np.uint32)


def _box_groups(n, seed=5):
    """the Cornell box's 12 triangles in their order, cut to n or filled up to n with seeded small triangles inside the box"""
    flat = [(mat, t) for mat, tl in scenes.cornell_groups() for t in tl][:n]
    groups = []
    for mat, t in flat:
        if groups and groups[-1][0] is mat:
            groups[-1][1].append(t)
        else:
            groups.append((mat, [t]))
    if n > 12:
        rng = np.random.default_rng(seed)
        c = rng.uniform((-2.2, 0.8, -5.2), (2.2, 5.0, -0.8), (n - 12, 1, 3))
        extra = (c + rng.uniform(-0.45, 0.45, (n - 12, 3, 3))).astype(np.float32)
        groups.append((scenes.material(diffuse=(0.3, 0.5, 0.9)), [tuple(map(tuple, t)) for t in extra]))
    return groups


def _scene(groups, spheres, cam_pos=(0, 3, 5), cam_dir=(0, 0, -1), sky=(0, 0, 0), depth=DEPTH):
    u = scenes.make_uniforms(W, H, SPP, depth, cam_pos=cam_pos, cam_dir=cam_dir, ground_enabled=0, sky=sky)
    s = scenes._finish("trip", u, spheres, NO_LIGHTS, groups, bvh_builder=_one_node)
    assert len(s.bvh_nodes) == 1
    return s


def _spheres(n):
    return scenes.cornell_spheres(n=n) if n else NO_SPHERES


_cache = {}


def _want(key, make):
    """(scene, oracle accumulation words, oracle RGBA, oracle stats) of make(), rendered once and never written to"""
    if key not in _cache:
        s = make()
        acc, _, rgba, st = _oracle.render(s)
        acc, rgba = _u32(acc), np.ascontiguousarray(rgba)
        for a in (acc, rgba):
            a.setflags(write=False)
        _cache[key] = (s, acc, rgba, st)
    return _cache[key]


def _check(want, batch, where):
    s, o_acc, o_rgba, o_st = want
    rc = RenderConfig.from_scene(s)
    e = Engine.new(rc, queue_batch=batch)
    try:
        px = e.render(rc).pixels
        # the single-node kernel; which of its two forms follows from the forced batch alone (launch_render: the staged k_trace iff the
        # batch is a whole multiple of 256 items, k_trace_direct otherwise) -- the engine reports one name for both
        assert e.last_kernel_name() == "k_trace", (where, e.last_kernel_name())
        assert np.array_equal(_u32(e.read_accumulation()), o_acc), (where, batch, "accumulation")
        assert np.array_equal(px, o_rgba), (where, batch, "frame")
        assert e.stats()["segments"] == o_st["segments"], (where, batch, "segments")
    finally:
        e.close()


BATCHES = pytest.mark.parametrize("batch", [STAGED, DIRECT], ids=["k_trace", "k_trace_direct"])


@BATCHES
@pytest.mark.parametrize("n_spheres", [0, 8])
@pytest.mark.parametrize("n", [1, 2, 3, 12, 13, 127, 128])
def test_triangle_counts(n, n_spheres, batch):
    want = _want(("count", n, n_spheres), lambda: _scene(_box_groups(n), _spheres(n_spheres)))
    assert want[3]["segments"] > want[3]["paths"] == W * H * SPP      # the floor is triangle 0: paths bounce in every scene
    _check(want, batch, ("count", n, n_spheres))


@BATCHES
@pytest.mark.parametrize("dead", [(0,), (6,), (11,), (0, 6, 11)], ids=["first", "middle", "last", "all_three"])
def test_dead_records(dead, batch):
    def make():
        s = _scene(_box_groups(12), _spheres(8))
        idx = s.bvh_indices.copy()
        idx[list(dead)] = abi.NO_INDEX                                   # no such triangle: the record's `live` word is 0
        return dataclasses.replace(s, bvh_indices=idx)
    want = _want(("dead", dead), make)
    whole = _want(("count", 12, 8), lambda: _scene(_box_groups(12), _spheres(8)))
    assert not np.array_equal(want[1], whole[1]), "the dead records are seen by no ray"
    _check(want, batch, ("dead", dead))


@BATCHES
def test_lanes_outside_the_nodes_box(batch):
    # from further back and off to the side the box fills only part of the frame: the other lanes enter the loop switched off
    want = _want("aside", lambda: _scene(_box_groups(12), _spheres(8), cam_pos=(5, 3, 14), sky=(0.25, 0.5, 0.75)))
    sky = (want[2][..., :3] == want[2][0, -1, :3]).all(-1)
    assert 0.2 < sky.mean() < 0.8, sky.mean()                            # (the top right pixel looks past the box)
    _check(want, batch, "aside")


@BATCHES
@pytest.mark.parametrize("depth", [1, DEPTH])
def test_an_early_out_no_lane_passes(depth, batch):
    # A 13th triangle in the plane x = 1000 beside the camera, edge1 along z.  A primary ray leaves (0, 3, 5) within the pane,
    # |dz / dx| >= 35 / 18, so its line meets that plane at |z - 5| >= 1000 * 35 / 18: u, the coordinate along edge1 = (0, 0, 1)
    # from v0.z = 4, is beyond 1900 in magnitude for every lane, and a ray with dx = 0 fails the determinant before it.  With
    # depth 1 there are only primary rays, so every trip of this record runs past the u test with an empty mask.
    assert 1000.0 * 35.0 / 18.0 - 1.0 > 1900.0
    far = (scenes.material(diffuse=(0.9, 0.1, 0.9)), [((1000.0, 2.0, 4.0), (1000.0, 2.0, 5.0), (1000.0, 3.0, 4.0))])
    want = _want(("far", depth), lambda: _scene(_box_groups(12) + [far], _spheres(8), depth=depth))
    box = _want(("box", depth), lambda: _scene(_box_groups(12), _spheres(8), depth=depth))
    if depth == 1:
        assert np.array_equal(want[1], box[1]), "a primary ray hits the far triangle"
    _check(want, batch, ("far", depth))


def _floor(half, y=0.0):
    return scenes._quad((-half, y, half), (half, y, half), (half, y, -half), (-half, y, -half))


def _bare(s):
    """the scene without its triangles, for the oracle: what the frame is when no triangle is ever hit"""
    u = s.uniforms.copy()
    u["bvh_node_count"] = 0
    u["bvh_triangle_count"] = 0
    return dataclasses.replace(s, uniforms=u, bvh_nodes=s.bvh_nodes[:0], bvh_indices=s.bvh_indices[:0], bvh_triangles=s.bvh_triangles[:0],
                               meshes=s.meshes[:0])


@BATCHES
def test_determinants_on_the_division_path(batch):
    # a floor with edges of 2e17: |det| = |edge1 x edge2 . d| is 4e34 |d.y|, at or above 2^100 = 1.3e30 for all but grazing rays
    grey = scenes.material(diffuse=(0.7, 0.7, 0.7))
    want = _want("huge", lambda: _scene([(grey, _floor(1e17))], _spheres(8), sky=(0.25, 0.5, 0.75)))
    bare = _want("huge_bare", lambda: _bare(_scene([(grey, _floor(1e17))], _spheres(8), sky=(0.25, 0.5, 0.75))))
    assert (want[1] != bare[1]).any(-1).mean() > 0.25, "the oracle hits the huge floor in too few pixels"
    _check(want, batch, "huge")


@BATCHES
def test_determinants_below_the_reference_bound(batch):
    # triangles with edges of 1e-4 in front of the camera: |det| <= 1e-8 |d| < 1e-6, every one rejected by the first early-out
    rng = np.random.default_rng(11)
    c = rng.uniform((-1.0, 2.0, 1.0), (1.0, 4.0, 3.0), (12, 1, 3))
    tiny = (c + rng.uniform(-1e-4, 1e-4, (12, 3, 3)) / 2).astype(np.float32)
    groups = [(scenes.material(diffuse=(0.9, 0.9, 0.1)), [tuple(map(tuple, t)) for t in tiny])]
    want = _want("tiny", lambda: _scene(groups, _spheres(8), sky=(0.25, 0.5, 0.75)))
    bare = _want("tiny_bare", lambda: _bare(_scene(groups, _spheres(8), sky=(0.25, 0.5, 0.75))))
    assert np.array_equal(want[1], bare[1]) and want[3]["segments"] == bare[3]["segments"], "the oracle hits a tiny triangle"
    assert want[3]["segments"] > want[3]["paths"]                        # the spheres are there to be hit
    _check(want, batch, "tiny")


@BATCHES
def test_updates_grow_and_shrink_the_table(batch):
    # one engine, 12 -> 13 -> 11 triangles: the trip count and the end of the table follow every update
    wants = [_want(("count", n, 8), lambda n=n: _scene(_box_groups(n), _spheres(8))) for n in (12, 13, 11)]
    assert len({w[1].tobytes() for w in wants}) == 3
    e = None
    try:
        for k, (s, o_acc, o_rgba, o_st) in enumerate(wants):
            rc = RenderConfig.from_scene(s, create=(k == 0))
            if e is None:
                e = Engine.new(rc, queue_batch=batch)
            e.reset_stats()
            px = e.render(rc).pixels
            assert e.last_kernel_name() == "k_trace"
            assert np.array_equal(_u32(e.read_accumulation()), o_acc), (k, "accumulation")
            assert np.array_equal(px, o_rgba), (k, "frame")
            assert e.stats()["segments"] == o_st["segments"], (k, "segments")
    finally:
        if e is not None:
            e.close()


@pytest.mark.parametrize("seed", [1, 20240917, 0xFFFFFFFF])
def test_trip_equals_the_compiler_laid_form(seed):
    out = np.zeros(32, dtype=np.uint32)
    assert _lib.load().rb_debug_triangle_trip(1 << 20, seed, out.ctypes.data) == 0
    assert out[0] == 0, ("triples that differ", int(out[0]), "one of them", int(out[1]), out[2:18].view(np.float32),
                         "trip", out[18:22], "accept_slot", out[22:26])


@pytest.mark.parametrize("branch", [0, 1])
def test_scalar_mix_measures(branch):
    import ctypes as C
    for scalar in (0, 16):
        v = (C.c_double * 3)()
        assert _lib.load().rb_measure_salu_mix(0, scalar, branch, v) == 0
        print("scalar per 16 vector", scalar, "branch", branch, "-> clocks per vector instruction", v[0], "GHz", v[1], "ms", v[2])
        assert all(np.isfinite(x) and x > 0 for x in v)
