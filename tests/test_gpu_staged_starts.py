"""k_trace's staged row starts (ColorRing::stage_row in rb_kernels.hip): with reservations of whole multiples of 256 items
the wave starts all 64 paths of a row in one full-width pass when it opens the row, parks direction and seed in the colour
ring and hands them out from there.  Everything below is bit for bit against the oracle -- accumulation words, RGBA8,
segment and path counts -- at the places where a staged entry could be lost, started twice or taken for radiance:
padding pixels, rows that turn over every iteration, the zero-depth arm, the sample wrap to the next tile, paths that
outlive their slice, the slow-divide camera, sharded rows, the 8-wave instantiation, and staged against direct starts."""
import dataclasses

import numpy as np
import pytest

from renderbaby_amd import Engine, RenderConfig, scenes
from renderbaby_amd import dist as rdist
from tests import _oracle

pytestmark = pytest.mark.gpu

_oracle_cache = {}


def _want(w, h, spp, depth):
    """the oracle's frame of cornell(w, h, spp, depth), rendered once per module and never written to"""
    key = (w, h, spp, depth)
    if key not in _oracle_cache:
        s = scenes.cornell(w, h, spp, depth)
        acc, _, rgba, st = _oracle.render(s)
        # nothing vacuous: every pixel's paths are there, and they bounce wherever the depth lets them
        assert st["paths"] == w * h * spp and st["segments"] >= (2 * st["paths"] if depth > 1 else depth * st["paths"]), st
        for a in (acc, rgba):
            a.setflags(write=False)
        _oracle_cache[key] = (s, acc, rgba, st)
    return _oracle_cache[key]


def _render(scene, **kw):
    rc = RenderConfig.from_scene(scene)
    e = Engine.new(rc, **kw)
    try:
        f = e.render(rc)
        return e.read_accumulation(), f.pixels, e.stats(), e.last_kernel_name()
    finally:
        e.close()


def _check(w, h, spp, depth, batch):
    s, o_acc, o_rgba, o_st = _want(w, h, spp, depth)
    acc, px, st, name = _render(s, queue_batch=batch)
    assert name == "k_trace"
    assert np.array_equal(acc.view(np.uint32), o_acc.view(np.uint32)), (w, h, spp, depth, batch)
    assert np.array_equal(px, o_rgba), (w, h, spp, depth, batch)
    assert st["segments"] == o_st["segments"] and st["paths"] == o_st["paths"], (st, o_st)
    return acc


@pytest.mark.parametrize("batch", [256, 512])
@pytest.mark.parametrize("size", [(203, 77), (9, 9)], ids=["203x77", "9x9"])
def test_padding_is_staged_but_never_started(size, batch):
    # edge tiles: 203 = 25 tiles + 3 pixels, 77 = 9 tiles + 5 rows; 9 x 9: three of four tiles are mostly padding
    _check(size[0], size[1], 6, 5, batch)


@pytest.mark.parametrize("depth", [1, 0])
def test_depth_one_and_depth_zero(depth):
    # depth 1: every lane is idle again after one segment, so a row turns over in every iteration and the takes straddle
    # two rows all the time; depth 0: the arm that stores zeros and never becomes active, with the ring on
    _check(64, 40, 8, depth, 256)


@pytest.mark.parametrize("spp", [1, 3])
def test_sample_wrap_to_the_next_tile(spp):
    # 24 x 16 = 3 x 2 tiles: with 1 (3) samples the row after a tile's last sample is the next tile's first, the
    # third tile's the first of the next tile row
    _check(24, 16, spp, 6, 256)


def test_deep_paths_outlive_their_slice():
    # depth 40: lanes still tracing when their slice is restaged are marked to store directly; the slice is retaken meanwhile
    _check(64, 40, 16, 40, 256)


@pytest.mark.parametrize("size", [(2, 2), (1, 4)], ids=["2x2", "1x4"])
def test_slow_divide_camera(size):
    # w - 1 or h - 1 outside the exact-reciprocal division's range: the camera arm with the compiler's division, from the
    # staged start; the forced batch is larger than the frame.  (1 x 4: w - 1 = 0, the quotient is not finite and every
    # path is its primary segment -- the words must still be the oracle's)
    pos, direction = (0, 9, 0.5), (0.01, -1.0, -0.02)
    s = scenes.cornell(size[0], size[1], 4, 4)
    u = s.uniforms.copy()
    u["camera"]["pos"] = pos
    u["camera"]["dir"] = direction
    s = dataclasses.replace(s, uniforms=u)
    o_acc, _, o_rgba, o_st = _oracle.render(s)
    assert o_st["paths"] == size[0] * size[1] * 4 and o_st["segments"] >= o_st["paths"]
    acc, px, st, name = _render(s, queue_batch=256)
    assert name == "k_trace"
    assert np.array_equal(acc.view(np.uint32), o_acc.view(np.uint32))
    assert np.array_equal(px, o_rgba)
    assert st["segments"] == o_st["segments"] and st["paths"] == o_st["paths"]


@pytest.mark.parametrize("stripe_rows", [1, 8])
def test_sharded_rows(stripe_rows):
    # two ranks on one device: a rank's local rows are every other stripe of the frame (global_row in the staged pass),
    # 24 rows in stripes of 8 leave rank 1 a padded stripe
    w, h = 40, 24
    s, o_acc, o_rgba, o_st = _want(w, h, 4, 5)
    parts, segments, paths = [], 0, 0
    for rank in range(2):
        sr = rdist.ShardedRenderer(s, rank=rank, world=2, device=0, stripe_rows=stripe_rows, queue_batch=256)
        try:
            sr.render_local()
            assert sr.engine.last_kernel_name() == "k_trace"
            acc = sr.engine.read_accumulation()
            rows = rdist.global_rows(h, rank, 2, stripe_rows)
            own = rows < h
            assert own.sum() == sr.owned
            assert np.array_equal(acc[own].view(np.uint32), o_acc[rows[own]].view(np.uint32)), rank
            st = sr.engine.stats()
            segments, paths = segments + st["segments"], paths + st["paths"]
            parts.append(sr.local.cpu().clone())
        finally:
            sr.close()
    assert np.array_equal(rdist.assemble(parts, h, stripe_rows).numpy(), o_rgba)
    assert segments == o_st["segments"] and paths == o_st["paths"]


def test_eight_wave_instantiation():
    # one launch of 3 * 2^23 items takes the instantiation built for 8 waves per SIMD (64 registers): 1024 x 768 at 32
    # samples; the oracle renders a window of rows across a tile boundary and the frame's last rows
    w, h, spp, depth = 1024, 768, 32, 4
    assert (w // 8) * (h // 8) * 64 * spp >= 3 << 23
    s = scenes.cornell(w, h, spp, depth)
    acc, px, _, name = _render(s)
    assert name == "k_trace"
    for r0, r1 in ((381, 387), (766, 768)):
        o_acc, _, o_rgba, o_st = _oracle.render(s, rows=(r0, r1))
        assert o_st["paths"] == w * (r1 - r0) * spp and o_st["segments"] > o_st["paths"]
        assert np.array_equal(acc[r0:r1].view(np.uint32), o_acc[r0:r1].view(np.uint32)), (r0, r1)
        assert np.array_equal(px[r0:r1], o_rgba[r0:r1]), (r0, r1)


def test_staged_and_direct_starts_agree():
    # batch 64: every lane starts its own path (k_trace_direct); batch 256: the staged form
    staged = _check(203, 77, 6, 5, 256)
    direct = _check(203, 77, 6, 5, 64)
    assert np.array_equal(staged.view(np.uint32), direct.view(np.uint32))
