"""RB_FLAG_BUILD_TREE on the MI355X: the device builder of the canonical reference-layout tree gives rb_bvh_build_canonical's
bytes, and an engine that builds its own tree renders what the oracle renders with that tree, under every walk."""
import dataclasses

import numpy as np
import pytest

from renderbaby_amd import Engine, RenderConfig, abi, bvh, refscenes, scenes
from renderbaby_amd.engine import Change, RenderError
from tests import _oracle
from tests.test_build_tree import _soup, model_sets

pytestmark = pytest.mark.gpu


def _same_bytes(tris):
    h_nodes, h_idx = bvh.build_canonical(tris)
    d_nodes, d_idx = bvh.build_device(tris, device=0)
    assert d_nodes.tobytes() == h_nodes.tobytes()
    assert np.array_equal(d_idx, h_idx)
    return d_nodes, d_idx


@pytest.mark.parametrize("name", sorted(model_sets()))
def test_device_matches_host_on_the_model_sets(name):
    _same_bytes(model_sets()[name])


@pytest.mark.parametrize("n", [1, 2, 128, 129, 255, 256, 257, 4097, 65_537])
def test_device_matches_host_by_count(n):
    _same_bytes(_soup(n, 1000 + n))


@pytest.mark.parametrize("which", ["c3", "lamp", "c5"])
def test_device_matches_host_on_the_baseline_meshes(which):
    tris = {"c3": lambda: scenes.mesh_scene(112, 112, 16, 16, 1, 2, seed=7).bvh_triangles,
            "lamp": lambda: refscenes.ref_lamp(width=16, height=16, spp=1).bvh_triangles,
            "c5": lambda: scenes.mesh_scene(1024, 512, 16, 16, 1, 2, seed=11, with_blob=False).bvh_triangles}[which]()
    first = _same_bytes(tris)
    again = bvh.build_device(tris, device=0)
    assert again[0].tobytes() == first[0].tobytes() and np.array_equal(again[1], first[1])


# ---- the engine's own tree
def _scenes():
    return {
        "cornell": scenes.cornell(32, 24, 2, 4),
        "feature": scenes.feature_scene(24, 16, 2, 5),
        "c3": scenes.mesh_scene(112, 112, 24, 16, 2, 4, seed=7),
        "lamp": refscenes.ref_lamp(width=20, height=20, spp=2, max_depth=4),
    }


WALKS = {
    "chunk-device": dict(chunk_tree="device"),
    "chunk-host": dict(chunk_tree="host"),
    "reference": dict(reference_walk=True),
    "own": dict(own_tree=True),
    "queue": dict(kernel=abi.KERNEL_QUEUE),
    "pixel": dict(kernel=abi.KERNEL_PIXEL),
}


@pytest.fixture(scope="module")
def scene_set():
    return _scenes()


def _with_tree(scene, nodes, idx):
    s = dataclasses.replace(scene, bvh_nodes=nodes, bvh_indices=idx)
    s.uniforms = scene.uniforms.copy()
    s.uniforms["bvh_node_count"] = len(nodes)
    return s


def _render(eng, rc):
    frame = eng.render(rc)
    return frame.pixels, eng.read_accumulation(), eng.stats()


def _render_current(eng):
    frame = eng.render_current()
    return frame.pixels, eng.read_accumulation(), eng.stats()


@pytest.mark.parametrize("builder", ["device", "host"])
@pytest.mark.parametrize("walk", sorted(WALKS))
@pytest.mark.parametrize("name", ["cornell", "feature", "c3", "lamp"])
def test_engine_tree_against_the_oracle(scene_set, name, walk, builder):
    sc = scene_set[name]
    rc = RenderConfig.from_scene(sc, with_tree=False)
    eng = Engine.new(rc, device=0, build_tree=builder, **WALKS[walk])
    try:
        px, acc, st = _render(eng, rc)
        nodes, idx = eng.tree()
        assert eng.tree_builder()[0] == builder
    finally:
        eng.close()
    h_nodes, h_idx = bvh.build_canonical(sc.bvh_triangles)
    assert nodes.tobytes() == h_nodes.tobytes() and np.array_equal(idx, h_idx)
    o_acc, _, o_rgba, o_st = _oracle.render(_with_tree(sc, nodes, idx))
    assert np.array_equal(acc.view(np.uint32), o_acc.view(np.uint32))
    assert np.array_equal(px, o_rgba)
    assert st["segments"] == o_st["segments"]


@pytest.mark.parametrize("builder", ["device", "host"])
def test_engine_tree_equals_a_caller_canonical_tree(scene_set, builder):
    sc = scene_set["c3"]
    nodes, idx = bvh.build_canonical(sc.bvh_triangles)
    caller = Engine.new(RenderConfig.from_scene(_with_tree(sc, nodes, idx)), device=0)
    own_rc = RenderConfig.from_scene(sc, with_tree=False)
    own = Engine.new(own_rc, device=0, build_tree=builder)
    try:
        a = _render(caller, RenderConfig.from_scene(_with_tree(sc, nodes, idx)))
        b = _render(own, own_rc)
        assert caller.tree_builder()[0] == "caller" and own.tree_builder()[0] == builder
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
        t_nodes, t_idx = caller.tree()
        assert t_nodes.tobytes() == nodes.tobytes() and np.array_equal(t_idx, idx)
    finally:
        caller.close()
        own.close()


def test_both_builder_flags_are_refused(scene_set):
    from renderbaby_amd._lib import load
    import ctypes as C
    rc = RenderConfig.from_scene(scene_set["cornell"], with_tree=False)
    cfg, keep = rc.to_c()
    opt = abi.Options()
    opt.device = 0
    opt.flags = abi.FLAG_BUILD_TREE | abi.FLAG_BUILD_TREE_HOST
    lib = load()
    h = lib.rb_create_ex(C.byref(cfg), C.byref(opt))
    assert not h
    assert b"RB_FLAG_BUILD_TREE" in lib.rb_last_error(None)


def test_updates_follow_the_triangles(scene_set):
    sc = scene_set["c3"]
    rc = RenderConfig.from_scene(sc, with_tree=False)
    eng = Engine.new(rc, device=0, build_tree="device")
    try:
        before = _render(eng, rc)
        # moved triangles: the frame of a fresh engine
        tris = sc.bvh_triangles.copy()
        for f in ("v0", "v1", "v2"):
            tris[f][:, 1] += np.float32(0.25)
        moved = dataclasses.replace(sc, bvh_triangles=tris)
        eng.update(RenderConfig(uniforms=Change.update(sc.uniforms), bvh_triangles=Change.update(tris)))
        got = _render_current(eng)
        fresh_rc = RenderConfig.from_scene(moved, with_tree=False)
        fresh = Engine.new(fresh_rc, device=0, build_tree="device")
        want = _render(fresh, fresh_rc)
        fresh.close()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
        assert not np.array_equal(got[0], before[0])
        # a config that carries bvh_nodes is refused, and the scene stays as it was
        with pytest.raises(RenderError) as ei:
            eng.update(RenderConfig(uniforms=Change.update(sc.uniforms), bvh_nodes=Change.update(sc.bvh_nodes)))
        assert ei.value.code == 13
        again = _render_current(eng)
        assert np.array_equal(again[0], got[0])
        # deleted triangles: an empty tree
        eng.update(RenderConfig(uniforms=Change.update(sc.uniforms), bvh_triangles=Change.delete()))
        nodes, idx = eng.tree()
        assert len(nodes) == 0 and len(idx) == 0
        assert eng.tree_builder()[0] == ""
        empty = _render_current(eng)
        o_acc, _, o_rgba, _ = _oracle.render(dataclasses.replace(sc, bvh_nodes=nodes, bvh_indices=idx, bvh_triangles=tris[:0]))
        assert np.array_equal(empty[0], o_rgba)
    finally:
        eng.close()


def test_iterator_with_the_flag(scene_set):
    sc = scene_set["c3"]
    rc = RenderConfig.from_scene(sc, with_tree=False)
    eng = Engine.new(rc, device=0, build_tree="device")
    try:
        it = eng.frame_iterator(rc)
        last = None
        for fr in it:
            last = fr
        nodes, idx = eng.tree()
    finally:
        eng.close()
    _, _, o_rgba, _ = _oracle.render(_with_tree(sc, nodes, idx))
    assert np.array_equal(last.pixels, o_rgba)


def test_multi_part_handle(scene_set):
    sc = scene_set["lamp"]
    rc = RenderConfig.from_scene(sc, with_tree=False)
    single = Engine.new(rc, device=0, build_tree="device")
    multi = Engine.new(rc, devices=[0, 0], gather_peer_copy=True, build_tree="device")
    try:
        a = single.render(rc).pixels
        b = multi.render(rc).pixels
        assert np.array_equal(a, b)
        assert multi.tree_builder()[0] == "device"
        m_nodes, m_idx = multi.tree()
        s_nodes, s_idx = single.tree()
        assert m_nodes.tobytes() == s_nodes.tobytes() and np.array_equal(m_idx, s_idx)
    finally:
        single.close()
        multi.close()
