"""The rejection loop of random_unit_vector on the device (rb_device_math.hpp): one fma per coordinate, and a lane that
has its vector searches on and parks its seed in front of its next accepting try.  Every path must draw the vectors it
always drew, so everything below is bit for bit against the oracle, which keeps the shader's loop -- accumulation words
as uint32, RGBA8, segment and path counts:
 * depth 1 (every parked seed is thrown away), 2 (each is used exactly once), 8 and 40 (long chains of parked seeds),
   with staged (k_trace) and direct (k_trace_direct) starts;
 * all eight spheres metal at fuzz 0 and at fuzz 1: the exit of a path absorbed after its draw, the branch that scales
   the vector;
 * a multi-node mesh through k_trace_chunk, and rb_trace_rays on a few thousand rays;
 * the fused coordinate against the three operations on all 2^32 seeds."""
import dataclasses

import numpy as np
import pytest

from renderbaby_amd import Engine, RenderConfig, _lib, scenes
from tests import _oracle
from tests.conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

W, H, SPP = 64, 40, 8
_cache = {}


def _frozen(scene):
    acc, _, rgba, st = _oracle.render(scene)
    for a in (acc, rgba):
        a.setflags(write=False)
    return scene, acc, rgba, st


def _want(key, make):
    """the oracle's frame of a scene, rendered once per module and never written to"""
    if key not in _cache:
        _cache[key] = _frozen(make())
    return _cache[key]


def _render(scene, **kw):
    rc = RenderConfig.from_scene(scene)
    e = Engine.new(rc, device=0, **kw)
    try:
        f = e.render(rc)
        return e.read_accumulation(), f.pixels, e.stats(), e.last_kernel_name()
    finally:
        e.close()


def _same(scene, want, kernel, **kw):
    _, o_acc, o_rgba, o_st = want
    acc, px, st, name = _render(scene, **kw)
    assert name == kernel, name
    assert np.array_equal(acc.view(np.uint32), o_acc.view(np.uint32)), kw
    assert np.array_equal(px, o_rgba), kw
    assert st["segments"] == o_st["segments"] and st["paths"] == o_st["paths"], (st, o_st)


@pytest.mark.parametrize("batch", [256, 64], ids=["staged", "direct"])
@pytest.mark.parametrize("depth", [1, 2, 8, 40])
def test_cornell_depths(depth, batch):
    want = _want(("cornell", depth), lambda: scenes.cornell(W, H, SPP, depth))
    st = want[3]
    # nothing vacuous: every path is there, and paths scatter wherever the depth lets them
    assert st["paths"] == W * H * SPP and (st["segments"] > st["paths"] if depth > 1 else st["segments"] == st["paths"]), st
    _same(want[0], want, "k_trace", queue_batch=batch)


def _all_metal(shininess):
    s = scenes.cornell(W, H, SPP, 8)
    sp = s.spheres.copy()
    for k in range(len(sp)):
        sp[k]["material"] = scenes.material(diffuse=(0, 0, 0), specular=(0.9, 0.8, 0.7), shininess=shininess)
    return dataclasses.replace(s, spheres=sp)


@pytest.mark.parametrize("batch", [256, 64], ids=["staged", "direct"])
@pytest.mark.parametrize("fuzz", [0, 1])
def test_metal_spheres(fuzz, batch):
    # fuzz = clamp(1 - shininess / 1000, 0, 1): 0 leaves the vector out of the direction (it is drawn all the same),
    # 1 adds all of it, and a path whose scattered direction points into the sphere ends after the draw
    want = _want(("metal", fuzz), lambda: _all_metal(1000.0 * (1 - fuzz)))
    _same(want[0], want, "k_trace", queue_batch=batch)


def test_mesh_through_the_chunked_walk():
    # the scene of tests/golden/mesh578_32x20_2spp.npz (tests/golden/make_golden.py), at depth 6
    want = _want("mesh578", lambda: scenes.mesh_scene(12, 12, 32, 20, 2, 6, seed=7, bvh_builder=_oracle.bvh_build))
    assert len(want[0].bvh_nodes) > 1
    _same(want[0], want, "k_trace_chunk")


def test_trace_rays():
    from tests.test_gpu_query import _engine, pixel_centre_rays
    from tests.test_gpu_radiance import _u32, oracle_radiance
    scene = scenes.cornell(W, H, 1, 6)
    O, D = pixel_centre_rays(scene)
    O, D = O.reshape(-1, 3), D.reshape(-1, 3)
    assert len(O) == W * H
    e = _engine(scene)
    try:
        out = e.trace_rays(O, D, samples=2, first_sample=3)
        assert e.last_query_kernel_name() == "k_rad"
    finally:
        e.close()
    want = oracle_radiance(scene, O, D, None, 2, 3)
    assert (want["sum"] != 0).any()
    bad = np.nonzero((_u32(out).reshape(-1, 4) != _u32(want).reshape(-1, 4)).any(1))[0]
    assert len(bad) == 0, (len(bad), bad[:5], out[bad[:5]], want[bad[:5]])


def test_fused_coordinate_on_every_seed():
    out = np.full(16, 0xFFFFFFFF, np.uint32)
    assert _lib.load().rb_debug_rnd_pm1_exhaustive(out.ctypes.data) == 0
    assert out[0] == 0, [hex(int(x)) for x in out[:16]]
