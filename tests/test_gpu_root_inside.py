"""The root box of the single-node walk without its slab test (rb_device_intersect.hpp, RB_ROOT_INSIDE), on the device.
 * rb_debug_root_box runs the walk's own slab test (isect_aabb on rcp_exact's reciprocals) and the rule k_trace skips it by over
   the cases of tests/test_root_inside_model.py: both answers bit for bit the numpy model's, and "known" never without "true".
 * Frames against the oracle, byte for byte, where the rule's premises change from ray to ray: the camera outside the box (C2's),
   strictly inside it and exactly on the plane z = bmax.z; a small mesh whose box the spheres and the ground lie outside of, so
   that secondary rays start outside, re-enter and miss; a sphere resting on the floor (the offset origin under it falls below
   the floor).  40 x 24 and 37 x 19 (padding pixels), 3 samples, depth 8, through the staged kernel and through k_trace_direct."""
import dataclasses

import numpy as np
import pytest

from renderbaby_amd import Engine, RenderConfig, _lib, abi, scenes
from tests import _oracle
from tests import _root_box_cases as rb

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(rb.BOXES))
def test_device_slab_and_rule_are_the_model_s(name):
    o, d, bmin, bmax = rb.cases(name)
    rays = np.ascontiguousarray(np.concatenate([o, d], axis=1), dtype=np.float32)
    box = np.ascontiguousarray(np.concatenate([bmin, bmax]), dtype=np.float32)
    out = np.full(len(rays), 0xFFFFFFFF, dtype=np.uint32)
    assert _lib.load().rb_debug_root_box(rays.ctypes.data, len(rays), box.ctypes.data, out.ctypes.data) == 0
    assert out.max() <= 3
    slab, known = (out & 1) != 0, (out & 2) != 0
    want_slab, want_known = rb.slab(o, d, bmin, bmax), rb.known(o, d, bmin, bmax)
    bad = np.flatnonzero(slab != want_slab)
    assert bad.size == 0, (name, "slab", o[bad[:4]], d[bad[:4]])
    bad = np.flatnonzero(known != want_known)
    assert bad.size == 0, (name, "rule", o[bad[:4]], d[bad[:4]])
    assert not (known & ~slab).any()
    print(name, len(rays), "rays,", int(known.sum()), "known,", int(slab.sum()), "pass the slab test")


def _camera(scene, pos, direction=(0, 0, -1)):
    u = scene.uniforms.copy()
    u["camera"]["pos"] = pos
    u["camera"]["dir"] = direction
    return dataclasses.replace(scene, uniforms=u)


def _spheres(specs):
    s = np.zeros(len(specs), dtype=abi.SPHERE)
    for k, (c, r, preset, col) in enumerate(specs):
        s[k]["center"] = c
        s[k]["radius"] = r
        s[k]["material"] = scenes.sphere_material(preset, np.array(col, dtype=np.float32))
    return s


def _outside(w, h, spp, depth):
    # two small quads (a lit one and a grey one, one node) above a checkered ground, spheres to both sides and behind: nothing
    # but the quads is inside the tree's root box, and whatever scatters off ground or spheres starts outside of it
    u = scenes.make_uniforms(w, h, spp, depth, cam_pos=(0, 3.0, 2.5), cam_dir=(0, -0.55, -1), ground_enabled=1, ground_height=0.0,
                             sky=(0.6, 0.7, 0.9), cb1=(0.9, 0.9, 0.9), cb2=(0.3, 0.3, 0.3))
    lit = scenes._quad((-0.5, 1.0, -3.0), (0.5, 1.0, -3.0), (0.5, 2.0, -3.2), (-0.5, 2.0, -3.2))
    grey = scenes._quad((-0.6, 0.4, -2.6), (0.6, 0.4, -2.6), (0.6, 0.4, -3.4), (-0.6, 0.4, -3.4))
    groups = [(scenes.material(**scenes.LIGHT), lit), (scenes.material(**scenes.KHAKI), grey)]
    sph = _spheres([((-1.6, 0.7, -3.0), 0.7, "mirror", (0.9, 0.9, 0.9)), ((1.7, 0.6, -2.8), 0.6, "metal", (0.9, 0.6, 0.3)),
                    ((0.0, 0.9, -5.0), 0.9, "plastic", (0.3, 0.5, 0.9))])
    s = scenes._finish("outside", u, sph, np.zeros(0, dtype=abi.POINT_LIGHT), groups)
    assert len(s.bvh_nodes) == 1
    return s


def _resting(w, h, spp, depth):
    # one large sphere resting on the Cornell floor: centre.y = floor + radius
    u = scenes.make_uniforms(w, h, spp, depth, cam_pos=(0, 3, 5), cam_dir=(0, 0, -1))
    y0 = np.float32(scenes.BOX["y0"])
    sph = _spheres([((0.0, float(y0 + np.float32(1.25)), -3.0), 1.25, "plastic", (0.8, 0.4, 0.3))])
    return scenes._finish("resting", u, sph, np.zeros(0, dtype=abi.POINT_LIGHT), scenes.cornell_groups())


SCENES = {
    "camera_outside": lambda w, h: scenes.cornell(w, h, 3, 8),
    "camera_inside": lambda w, h: _camera(scenes.cornell(w, h, 3, 8), (0.3, 3.0, -1.0)),
    "camera_on_plane": lambda w, h: _camera(scenes.cornell(w, h, 3, 8), (0.0, 3.0, scenes.BOX["z1"])),
    "mesh_box_outside": lambda w, h: _outside(w, h, 3, 8),
    "resting_sphere": lambda w, h: _resting(w, h, 3, 8),
}
_frames = {}


def _want(name, size):
    """the oracle's frame, rendered once per module and never written to"""
    if (name, size) not in _frames:
        s = SCENES[name](*size)
        acc, _, rgba, st = _oracle.render(s)
        assert st["paths"] == size[0] * size[1] * 3 and st["segments"] >= 2 * st["paths"] and st["mesh_hits"] > 0, st   # the paths do bounce
        for a in (acc, rgba):
            a.setflags(write=False)
        _frames[(name, size)] = (s, acc, rgba, st)
    return _frames[(name, size)]


@pytest.mark.parametrize("batch", [256, 64], ids=["staged", "direct"])
@pytest.mark.parametrize("size", [(40, 24), (37, 19)], ids=["40x24", "37x19"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_frames_are_the_oracle_s(name, size, batch):
    s, o_acc, o_rgba, o_st = _want(name, size)
    rc = RenderConfig.from_scene(s)
    e = Engine.new(rc, queue_batch=batch)
    try:
        f = e.render(rc)
        acc, px, st, kernel = e.read_accumulation(), f.pixels, e.stats(), e.last_kernel_name()
    finally:
        e.close()
    assert kernel == "k_trace"
    assert np.array_equal(acc.view(np.uint32), o_acc.view(np.uint32)), (name, size, batch)
    assert np.array_equal(px, o_rgba), (name, size, batch)
    assert st["segments"] == o_st["segments"] and st["paths"] == o_st["paths"], (st, o_st)
