"""The triangle sift of the single-node kernels, k_trace_sift ("The triangle sift"): pass 1 is a conservative
box test per group of triangles, pass 2 the hand-laid trip on each lane's own survivors.  Conservative means exact here: the
frame is the one the unsifted kernel draws.  Held, bit for bit -- accumulation, pixels, segment and path counts -- at 64 x 48 and
33 x 17, 4 spp, depth 8, every scene three ways: this build sifting, this build with RB_TRI_FILTER=0 (k_trace_flat, the parent's
kernel), and the oracle.  Which kernel ran is asserted every time (rb_debug_trace_form).

The scenes: the Cornell box; single nodes of 1, 2, 3, 4, 31, 32, 33, 64 and 128 triangles (the fall-back below four live
triangles, the edges of the 32-slot blocks); a node whose groups all always pass (degenerate, NaN-vertex and 1e30 triangles) and
one that mixes them with ordinary ones; the ground on, whose hits start rays outside the origin region; the camera outside and
inside the root box.  The staged form is the one that sifts, so every launch reserves 256 items at a time (queue_batch).

Beside the frames: the trip of pass 2, which takes the record in vector registers, against the compiler-laid triangle test on the
triples of tests/test_gpu_triangle_trip.py, every word; and pass 1 on the device (rb_debug_tri_filter) against the float32 reference
test -- no accepted slot may be missing from a ray's mask -- and against the numpy model, whose masks may differ in at most 1 % of
the bits (the approximate reciprocal is not the model's), or the model is not the kernel.  That comparison runs on the Cornell
table and on the named tables of tests/_tri_filter_cases.py (groups of 1 to 4, bent groups, open groups between closed ones, dead
slots, a list from slot 7, 2 to 4 blocks, scenes far away, small and large), there under rays aimed at the triangles' edges and
vertices on grazing rays; each of those scenes is also rendered three ways at 33 x 17."""
import contextlib
import dataclasses
import os

import numpy as np
import pytest

from renderbaby_amd import Engine, RenderConfig, _lib, abi, scenes
from tests import _oracle
from tests import _tri_filter_cases as T   # the model's scene tables and the float32 reference test

pytestmark = pytest.mark.gpu

FLAT, SIFT, STAGED = abi.TRACE_FORM_FLAT, abi.TRACE_FORM_SIFT, abi.TRACE_FORM_STAGED
SIZES = [(64, 48), (33, 17)]
SPP, DEPTH = T.SPP, T.DEPTH


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


@contextlib.contextmanager
def _unsifted(on):
    """RB_TRI_FILTER=0 while an engine is made: that engine keeps k_trace_flat"""
    old = os.environ.get("RB_TRI_FILTER")
    if on:
        os.environ["RB_TRI_FILTER"] = "0"
    try:
        yield
    finally:
        if on:
            if old is None:
                del os.environ["RB_TRI_FILTER"]
            else:
                os.environ["RB_TRI_FILTER"] = old


def _render(scene, forced):
    rc = RenderConfig.from_scene(scene)
    with _unsifted(forced):
        e = Engine.new(rc, queue_batch=256)
    try:
        px = e.render(rc).pixels
        st = e.stats()
        assert e.last_kernel_name() == "k_trace"
        return _u32(e.read_accumulation()), px, (st["segments"], st["paths"]), e.trace_form()
    finally:
        e.close()


def _three_ways(scene, sifts):
    acc, px, counts, form = _render(scene, False)
    assert form & (FLAT | STAGED) == FLAT | STAGED, form
    assert bool(form & SIFT) == sifts, (form, sifts)
    f_acc, f_px, f_counts, f_form = _render(scene, True)
    assert f_form == form & ~SIFT, (f_form, form)
    assert np.array_equal(acc, f_acc), "accumulation against the unsifted kernel"
    assert np.array_equal(px, f_px) and counts == f_counts
    o_acc, _, o_rgba, o_st = _oracle.render(scene)
    assert np.array_equal(acc, _u32(o_acc)), "accumulation against the oracle"
    assert np.array_equal(px, o_rgba) and counts == (o_st["segments"], o_st["paths"])


# ----------------------------------------------------------------------------------- the scenes ---
_soup, ODD = T._soup, T.ODD      # (tests/_tri_filter_cases.py: the CPU tests build their tables from the same scenes)


@pytest.mark.parametrize("w,h", SIZES)
def test_cornell(w, h):
    _three_ways(scenes.cornell(w, h, SPP, DEPTH), True)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("n", [1, 2, 3, 4, 31, 32, 33, 64, 128])
def test_single_nodes(n, w, h):
    _three_ways(_soup(n, w, h), n >= 4)


@pytest.mark.parametrize("w,h", SIZES)
def test_groups_that_always_pass(w, h):
    _three_ways(_soup(0, w, h, extra=ODD), False)            # nothing can reject: the unsifted kernel
    _three_ways(_soup(9, w, h, extra=ODD), True)             # ordinary triangles beside them


@pytest.mark.parametrize("w,h", SIZES)
def test_ground_on(w, h):
    s = scenes.cornell(w, h, SPP, DEPTH)
    u = s.uniforms.copy()
    u["ground_enabled"], u["ground_height"], u["sky_color"] = 1, -1.0, (0.5, 0.7, 1.0)
    lights = np.zeros(1, dtype=abi.POINT_LIGHT)
    lights[0]["center"], lights[0]["radius"] = (0.0, 9.0, 3.0), 0.5
    lights[0]["material"] = scenes.material(diffuse=(0, 0, 0), emissive=(40, 40, 40))
    _three_ways(dataclasses.replace(s, uniforms=u, lights=lights), True)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("cam", [(0.0, 3.0, 5.0), (0.0, 3.0, -3.0), (40.0, 30.0, 60.0)])
def test_camera_outside_and_inside_the_root_box(cam, w, h):
    s = scenes.cornell(w, h, SPP, DEPTH)
    u = s.uniforms.copy()
    u["camera"]["pos"] = cam
    if cam[0] > 10:
        d = -np.asarray(cam, dtype=np.float64) + (0, 3, -3)
        u["camera"]["dir"] = d / np.linalg.norm(d)
    _three_ways(dataclasses.replace(s, uniforms=u), True)


def test_forced_engines_do_not_leak_the_variable():
    assert "RB_TRI_FILTER" not in os.environ


# ------------------------------------------------------------------------- the trip of pass 2 ---
@pytest.mark.parametrize("uv", [0, 1])
@pytest.mark.parametrize("seed", [1, 20240917, 0xFFFFFFFF])
def test_vector_operand_trip_equals_the_compiler_laid_form(seed, uv):
    # the triples and constructed edges of tests/test_gpu_triangle_trip.py, the record handed over in vector registers
    out = np.zeros(32, dtype=np.uint32)
    assert _lib.load().rb_debug_triangle_trip_vec(1 << 20, seed, uv, out.ctypes.data) == 0
    assert out[0] == 0, ("triples that differ", int(out[0]), "one of them", int(out[1]), out[2:18].view(np.float32),
                         "trip", out[18:22], "accept_slot", out[22:26])


# ------------------------------------------------------------------- pass 1 against its model ---
def _mask_families():
    from tests import _root_box_cases
    rng = np.random.default_rng(5)
    b, n = scenes.BOX, 40_000
    lo, hi = np.array([b["x0"], b["y0"], b["z0"]]), np.array([b["x1"], b["y1"], b["z1"]])
    inside = (lo + rng.random((n, 3)) * (hi - lo)).astype(np.float32)
    on = inside.copy()
    axis, side = rng.integers(0, 3, n), rng.integers(0, 2, n)
    on[np.arange(n), axis] = np.where(side == 0, lo[axis], hi[axis]).astype(np.float32)
    under = np.column_stack([rng.uniform(-1.2, 1.2, n), rng.uniform(0.3, 5.7399, n), rng.uniform(-4.2, -1.8, n)]).astype(np.float32)
    up = np.column_stack([rng.normal(size=n) * 0.3, np.abs(rng.normal(size=n)) + 0.05, rng.normal(size=n) * 0.3])
    yield "inside the box", inside, T._unit(rng.normal(size=(n, 3)))
    yield "from the walls", on, T._unit(rng.normal(size=(n, 3)))
    yield "under the light", under, T._unit(up)
    yield "outside the region", inside * np.float32(40.0), T._unit(rng.normal(size=(n, 3)))
    o, d, _, _ = _root_box_cases.cases("cornell")
    yield "root box cases", o, d
    yield "the three rays of a review", np.array([[0, 5, -3], [0, 5, -3], [0.5, 5.5, -3]], np.float32), \
        np.array([[1, 1.2e-38, 0], [1, -1.2e-38, 0], [0, 1.2e-38, -1]], np.float32)
    o, d = T.tiny_component_rays()
    yield "tiny direction components", o, d
    yield "tiny direction components, normalised", o, T._unit(d)


def test_device_masks_hold_every_accepted_hit_and_are_the_models():
    scene = scenes.cornell(64, 48, SPP, DEPTH)
    groups, reg, tri = T._scene_table(scene)
    rc = RenderConfig.from_scene(scene)
    e = Engine.new(rc, queue_batch=256)
    try:
        e.update(rc)
        for what, o, d in _mask_families():
            dev, first = e.tri_filter_masks(o, d)
            assert first == 0 and dev.shape == (12, len(o))
            o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
            ot, dt = np.ascontiguousarray(o.T), np.ascontiguousarray(d.T)
            acc, model = T._accepted(tri, ot, dt), T.M.candidate_mask(groups, reg, ot, dt)
            assert not (acc & ~dev).any(), (what, "accepted hits missing from the device's mask", int((acc & ~dev).sum()))
            share = float((dev != model).mean())
            print(f"{what}: {len(o)} rays, {int(acc.sum())} accepted, device candidates per ray {dev.sum(0).mean():.2f}, "
                  f"device and model differ in {share:.5%} of the bits")
            assert share <= 0.01, (what, share)
    finally:
        e.close()


@pytest.mark.parametrize("name", T.tables())
def test_device_masks_on_other_tables(name):
    scene = T.table_scene(name)
    (groups, reg, tri), (list_first, list_end) = T.table_of(name)
    rng = np.random.default_rng([36, T.tables().index(name)])       # (tests/test_tri_filter_model.py holds the model on the same rays)
    aimed = T.aimed_rays(tri, reg, rng)[:2]
    families = [("aimed", aimed, False), ("inside the region", T.region_rays(reg, 20_000, rng), True),
                ("from the triangles", T.surface_rays(tri, 20_000, rng), True),
                # held to the model like the random families, for the same reason -- one rule, two reciprocals: on the bent table
                # these rays are where the cone's s decides (tests/test_tri_filter_model.py shows how much of the mask hangs on it)
                ("along the edges", T.edge_rays(tri, reg, 10_000, rng), True)]
    rc = RenderConfig.from_scene(scene)
    e = Engine.new(rc, queue_batch=256)
    try:
        e.render(rc)
        assert e.trace_form() & SIFT, (name, e.trace_form())
        for what, (o, d), like_the_model in families:
            dev, first = e.tri_filter_masks(o, d)
            assert first == list_first == int(scene.bvh_nodes["first_primitive"][0])
            assert dev.shape == (list_end - list_first, len(o))
            ot, dt = np.ascontiguousarray(o.T), np.ascontiguousarray(d.T)
            acc, model = T._accepted(tri, ot, dt), T.M.candidate_mask(groups, reg, ot, dt)
            assert not acc[~tri[3]].any()                            # a dead slot accepts nothing; its candidate bit is free: pass 2 skips it
            assert not (acc & ~dev).any(), (name, what, "accepted hits missing from the device's mask", int((acc & ~dev).sum()))
            share = float((dev != model)[tri[3]].mean())
            print(f"{name}, {what}: {len(o)} rays, {int(acc.sum())} accepted, device candidates per ray {dev.sum(0).mean():.2f}, "
                  f"device and model differ in {share:.5%} of the live slots' bits")
            assert not dev.all(), (name, what, "pass 1 rejects nothing")
            if like_the_model:
                assert share <= 0.01, (name, what, share)
    finally:
        e.close()


@pytest.mark.parametrize("name", [n for n in T.tables() if n not in ("soup33", "soup64", "soup128")])   # (those: test_single_nodes)
def test_other_tables_three_ways(name):
    scene = T.table_scene(name)
    assert (scene.width, scene.height) == (33, 17)
    _three_ways(scene, True)                           # (for `offset` and `mixed` the oracle is the judge of what the list is)


def test_scenes_that_do_not_sift_say_so():
    scene = _soup(3, 64, 48)
    rc = RenderConfig.from_scene(scene)
    e = Engine.new(rc, queue_batch=256)
    try:
        e.update(rc)
        with pytest.raises(Exception, match="does not sift"):
            e.tri_filter_masks(np.zeros((1, 3), np.float32), np.ones((1, 3), np.float32))
    finally:
        e.close()
