"""Differential fuzzing (tools/fuzz_parity.py) in a small dose: random scenes with nasty geometry, every
kernel variant that applies, bit for bit against the oracle."""
import importlib.util
import os

import numpy as np
import pytest

from renderbaby_amd import Engine, RenderConfig
from tests import _oracle

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location(
    "fuzz_parity", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "fuzz_parity.py"))
fuzz = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fuzz)


@pytest.mark.parametrize("first", [0, 1000, 2000])
def test_random_scenes_all_variants(first):
    for seed in range(first, first + 25):
        s = fuzz.random_scene(seed)
        o_acc, _, o_rgba, o_st = _oracle.render(s)
        rc = RenderConfig.from_scene(s)
        for name, kw in fuzz.variants(s):
            e = Engine.new(rc, stats=True, **kw)
            frame = e.render(rc)
            acc, st = e.read_accumulation(), e.stats()
            e.close()
            assert np.array_equal(acc.view(np.uint32), o_acc.view(np.uint32)), (seed, name)
            assert np.array_equal(frame.pixels, o_rgba), (seed, name)
            assert st["segments"] == o_st["segments"] and st["paths"] == o_st["paths"], (seed, name)


def _every_variant_matches_the_oracle(s, label):
    o_acc, _, o_rgba, o_st = _oracle.render(s)
    rc = RenderConfig.from_scene(s)
    for name, kw in fuzz.variants(s):
        e = Engine.new(rc, stats=True, **kw)
        frame = e.render(rc)
        acc, st = e.read_accumulation(), e.stats()
        e.close()
        assert np.array_equal(acc.view(np.uint32), o_acc.view(np.uint32)), (label, name)
        assert np.array_equal(frame.pixels, o_rgba), (label, name)
        assert st["segments"] == o_st["segments"] and st["paths"] == o_st["paths"], (label, name)


@pytest.mark.parametrize("first", [3000, 3020])
def test_random_scenes_with_several_textures(first):
    # 40 small scenes with 2 to 5 textures of odd shapes (1 to 17 texels a side), a texture index per mesh group and per sphere from
    # -1 to n_tex (one past the end: black) and uv scales of 1, -3 and 1000: the texture offsets, the clamps and the wrap of
    # sample_texture under every variant
    textured = 0
    for seed in range(first, first + 20):
        s = fuzz.random_scene(seed, rich_textures=True)
        assert 2 <= len(s.textures) <= 5
        textured += int((s.meshes["material"]["texture_index"] > 0).any() or (s.spheres["material"]["texture_index"] > 0).any())
        _every_variant_matches_the_oracle(s, seed)
    assert textured >= 10, textured   # a texture other than the first is in use


@pytest.mark.parametrize("first", [500180, 603375, 700000])
def test_random_large_frames_all_variants(first, monkeypatch):
    # Both parity bugs of r02 (a tie between a sphere and an earlier category, seed 500188; large triangles behind a
    # zero-area one in the second pass of the library's walk, seed 603382) showed only on LARGE frames -- several queue
    # reservations per wave, up to 300 x 200 pixels and 9 spp -- which the small dose above never makes.  Fifteen such
    # scenes per range, the two seeds included, every variant.
    monkeypatch.setenv("FUZZ_BIG", "1")
    for seed in range(first, first + 15):
        s = fuzz.random_scene(seed)
        o_acc, _, o_rgba, o_st = _oracle.render(s)
        rc = RenderConfig.from_scene(s)
        for name, kw in fuzz.variants(s):
            e = Engine.new(rc, **kw)
            frame = e.render(rc)
            acc, st = e.read_accumulation(), e.stats()
            e.close()
            assert np.array_equal(acc.view(np.uint32), o_acc.view(np.uint32)), (seed, name)
            assert np.array_equal(frame.pixels, o_rgba), (seed, name)
            assert st["segments"] == o_st["segments"] and st["paths"] == o_st["paths"], (seed, name)


def test_sphere_at_exactly_the_t_of_an_earlier_category(monkeypatch):
    # Found by the r02 fuzzer (FUZZ_BIG, seed 500188, pixel (54, 38)): a triangle and a sphere (of 90, so the
    # library's sphere tree is in use) are hit at exactly the same t.  The reference's scan accepts a sphere only
    # if t < closest.t, so the triangle stays; the tree's tie rule (lower index wins among spheres) used to let the
    # first sphere displace it.  Whole frame, every variant.
    monkeypatch.setenv("FUZZ_BIG", "1")
    s = fuzz.random_scene(500188)
    assert len(s.spheres) > 64 and (s.width, s.height) == (283, 199)
    o_acc, _, o_rgba, o_st = _oracle.render(s)
    rc = RenderConfig.from_scene(s)
    for name, kw in fuzz.variants(s):
        e = Engine.new(rc, **kw)
        frame = e.render(rc)
        acc, st = e.read_accumulation(), e.stats()
        e.close()
        assert np.array_equal(acc.view(np.uint32), o_acc.view(np.uint32)), name
        assert np.array_equal(frame.pixels, o_rgba), name
        assert st["segments"] == o_st["segments"], name


def test_second_pass_keeps_the_triangles_behind_a_degenerate_one(monkeypatch):
    # Found by the r02 fuzzer (FUZZ_BIG, seed 603382, six pixels): the eye lies in the plane of a huge triangle, so the
    # reference reports hits from a near-zero determinant that only the second pass of the library's walk can find.
    # The list of a reference leaf's large triangles used to END at the first triangle without a normal (zero area),
    # so every large triangle after it in the leaf was invisible to that pass.
    monkeypatch.setenv("FUZZ_BIG", "1")
    s = fuzz.random_scene(603382)
    assert len(s.bvh_nodes) > 1
    o_acc, _, o_rgba, o_st = _oracle.render(s)
    rc = RenderConfig.from_scene(s)
    for name, kw in fuzz.variants(s):
        e = Engine.new(rc, **kw)
        frame = e.render(rc)
        acc, st = e.read_accumulation(), e.stats()
        e.close()
        assert np.array_equal(acc.view(np.uint32), o_acc.view(np.uint32)), name
        assert np.array_equal(frame.pixels, o_rgba), name
