"""A launch group of the stream kernels that does not fit one launch alternates between two colour parts: k_accumulate of
launch i runs on a stream of its own underneath k_trace of launch i + 1 (dispatch in rb_runtime.cpp, rb_color_plan.hpp).
The hazards are about launch counts and ordering, not frame size, so the frames are small; everything is bit for bit
against the oracle -- accumulation words, RGBA8, segments and paths -- and every test asserts its launch count, so that
none can pass on a single launch.

The budget rule cannot give two launches: a group that does not fit the budget runs in halves of it, and what does not fit
the whole takes at least three halves.  Two launches are reached with passes_per_launch instead."""
import ctypes as C

import numpy as np
import pytest

from renderbaby_amd import Engine, RenderConfig, abi, denoise, scenes
from renderbaby_amd.engine import PinnedFrame
from tests import _oracle

pytestmark = pytest.mark.gpu

W, H, DEPTH = 64, 40, 4          # 8 x 5 tiles: 2560 items per pass; 1 MiB holds 25 passes, half of it 12
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _cornell(spp, w=W, h=H):
    return scenes.cornell_c1().with_params(width=w, height=h, spp=spp, max_depth=DEPTH)


def _mesh(spp=5):
    # the scene of tests/golden/mesh578_32x20_2spp.npz (tests/golden/make_golden.py)
    return scenes.mesh_scene(12, 12, 32, 20, spp, 6, seed=7, bvh_builder=_oracle.bvh_build)


def _want(key, make, **kw):
    """(scene, oracle accumulation, oracle RGBA8, oracle stats), rendered once per module and never written to"""
    if key not in _cache:
        s = make()
        acc, _, rgba, st = _oracle.render(s, **kw)
        assert st["paths"] > 0 and st["segments"] > st["paths"], st   # nothing vacuous
        for a in (acc, rgba):
            a.setflags(write=False)
        _cache[key] = (s, acc, rgba, st)
    return _cache[key]


def _check_engine(e, want, launches, frame=None, also=()):
    """the engine's committed frame and its counters since the last reset: `want`, and the groups of `also` traced before it"""
    _, o_acc, o_rgba, o_st = want
    px = e.read_rgba() if frame is None else frame
    acc, st = e.read_accumulation(), e.stats()
    assert st["launches"] == launches, st
    assert np.array_equal(_bits(acc), _bits(o_acc))
    assert np.array_equal(px, o_rgba)
    for k in ("segments", "paths"):
        assert st[k] == o_st[k] + sum(w[3][k] for w in also), (k, st, o_st)
    return st


def _render(want, launches, **kw):
    rc = RenderConfig.from_scene(want[0])
    e = Engine.new(rc, **kw)
    try:
        f = e.render(rc)
        st = _check_engine(e, want, launches, f.pixels)
        return st, e.last_kernel_name(), e.last_dispatch_ms()
    finally:
        e.close()


@pytest.mark.parametrize("spp,kw,launches", [(25, {}, 1), (24, dict(passes_per_launch=12), 2), (36, {}, 3), (37, {}, 4), (60, {}, 5)],
                         ids=["1", "2", "3", "4-short-last", "5"])
def test_cornell_launch_counts(spp, kw, launches):
    # 36: three whole halves; 37: a last launch of one pass; 60: five, both parts reused twice
    want = _want(("cornell", spp), lambda: _cornell(spp))
    st, name, ms = _render(want, launches, color_budget_mib=1, **kw)
    assert name == "k_trace"    # (reservations of 64 items: the direct starts)
    assert st["trace_ms"] > 0 and st["accumulate_ms"] > 0
    # the group's time spans the join, so no trace launch is longer than it.  stats() has the launches' sum only: one launch
    # is compared as it is, several (their tails overlap, so the sum may exceed the group's time) through their mean
    assert ms >= st["trace_ms"] / launches


def test_staged_trace_three_launches():
    # reservations of 256 items give the staged k_trace (tests/test_gpu_staged_starts.py); 9 x 9 is its smallest frame there
    for (w, h, spp) in ((9, 9, 7), (W, H, 40)):
        want = _want(("cornell", spp, w, h), lambda: _cornell(spp, w, h))
        kw = dict(passes_per_launch=3) if w == 9 else dict(color_budget_mib=1)
        st, name, _ = _render(want, 3 if w == 9 else 4, queue_batch=256, **kw)
        assert name == "k_trace"


def test_one_pass_per_launch():
    want = _want(("cornell", 5), lambda: _cornell(5))
    _render(want, 5, passes_per_launch=1)


def test_mesh_through_the_chunked_walk():
    want = _want("mesh", _mesh)
    _, name, _ = _render(want, 3, passes_per_launch=2)
    assert name == "k_trace_chunk"


def test_stats_builds_count_what_the_oracle_counts():
    want = _want("mesh", _mesh)
    st, name, _ = _render(want, 3, passes_per_launch=2, stats=True)
    assert name == "k_trace_chunk"
    st, _, _ = _render(want, 3, passes_per_launch=2, stats=True, reference_walk=True)   # every counter is the reference walk's
    assert {k: st[k] for k in _oracle.STAT_KEYS} == want[3]
    want = _want(("cornell", 36), lambda: _cornell(36))
    _render(want, 3, color_budget_mib=1, stats=True)


@pytest.mark.parametrize("kernel", [abi.KERNEL_QUEUE, abi.KERNEL_PIXEL], ids=["k_queue", "k_pixel"])
def test_kernels_without_a_colour_buffer(kernel):
    want = _want(("cornell", 5), lambda: _cornell(5))
    st, _, _ = _render(want, 3, kernel=kernel, passes_per_launch=2, color_budget_mib=1)
    assert st["trace_ms"] > 0


def _async_engine(want, **kw):
    """an engine holding the scene, nothing rendered: what follows is queued without a host synchronisation in between"""
    rc = RenderConfig.from_scene(want[0])
    e = Engine.new(rc, color_budget_mib=1, **kw)
    e.update(rc)
    return e


def test_queries_and_the_denoiser_follow_the_join():
    want = _want(("cornell", 36), lambda: _cornell(36))
    e = _async_engine(want)
    try:
        e.clear()
        e.dispatch(0, 36)
        hits = e.render_hits()                 # a query queued behind the group
        filtered = e.denoise(linear=True)      # reads the accumulation the last accumulate writes
        guides = e.denoise_guides()
        model = denoise.filter(denoise.mean_radiance(np.array(want[1])), guides)
        assert np.array_equal(_bits(filtered), _bits(model))
        assert hits.shape == (H, W)
        _check_engine(e, want, 3)
    finally:
        e.close()


def test_clear_and_back_to_back_groups():
    want = _want(("cornell", 60), lambda: _cornell(60))
    first = _want(("cornell", 60, "first 37"), lambda: _cornell(60), n_passes=37)
    dropped = _want(("cornell", 60, "first 36"), lambda: _cornell(60), n_passes=36)
    e = _async_engine(want)
    try:
        e.clear()
        e.dispatch(0, 36)      # thrown away by the clear that follows it
        e.clear()
        e.dispatch(0, 37)      # 4 launches, the last of one pass
        e.dispatch(37, 23)     # 1 launch: its accumulate reads what the other stream has just written
        _check_engine(e, want, 3 + 4 + 1, also=[dropped])
        e.reset_stats()
        e.clear()
        e.dispatch(0, 37)
        st = _check_engine(e, first, 4)
        assert st["trace_ms"] > 0 and st["accumulate_ms"] > 0
    finally:
        e.close()


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "page-locked"])
def test_iterator_runs_a_group_ahead_on_both_slots(pinned):
    # 90 passes in frames of 30: every group is 3 launches, started ahead on the other slot while this frame is read
    spp, per = 90, 30
    s = _cornell(spp)
    rc = RenderConfig.from_scene(s)
    e = Engine.new(rc, color_budget_mib=1)
    pf = PinnedFrame(W, H) if pinned else None
    try:
        it = e.frame_iterator(rc, passes_per_frame=per)
        for k in range(3):
            want = _want(("cornell", spp, "first", (k + 1) * per), lambda: _cornell(spp), n_passes=(k + 1) * per)
            if pinned:    # the copy-stream path, behind the slot's event
                e._check(e._lib.rb_iter_next(e._h, pf.array.ctypes.data))
                px = pf.array
            else:
                px = it.next().pixels
            assert np.array_equal(px, want[2]), k
            assert np.array_equal(_bits(e.read_accumulation()), _bits(want[1])), k
        assert not it.has_next()
        assert e.stats()["launches"] == 9
        if pinned:
            e._check(e._lib.rb_render(e._h, pf.array.ctypes.data))
            assert np.array_equal(pf.array, want[2])
    finally:
        e.close()
        if pf is not None:
            pf.free()


def test_sharded_engine():
    want = _want(("cornell", 36), lambda: _cornell(36))
    s, o_acc, o_rgba, _ = want
    rc = RenderConfig.from_scene(s)
    e = Engine.new(rc, shard_rank=1, shard_count=3, stripe_rows=8, passes_per_launch=8)
    try:
        f = e.render(rc)
        assert e.stats()["launches"] == 5
        acc = e.read_accumulation()
        owned, padded = e.local_rows()
        assert owned == 16 and padded == 16      # stripes 1 and 4 of five
        rows = np.array([e.global_row(r) for r in range(padded)])
        assert np.array_equal(_bits(acc), _bits(o_acc[rows]))
        assert np.array_equal(f.pixels, o_rgba[rows])
    finally:
        e.close()


def test_update_to_a_larger_frame_behind_a_group():
    small = _want(("cornell", 36), lambda: _cornell(36))
    large = _want(("cornell", 30, 96, 64), lambda: _cornell(30, 96, 64))    # 6144 items per pass: 10 fit, 5 per half
    e = _async_engine(small)
    try:
        e.clear()
        e.dispatch(0, 36)                                     # 3 launches queued, nothing waited for
        f = e.render(RenderConfig.from_scene(large[0], create=False))   # new frame buffers, a larger colour buffer
        _check_engine(e, large, 3 + 6, f.pixels, also=[small])
        f = e.render(RenderConfig.from_scene(small[0], create=False))   # and back
        assert np.array_equal(f.pixels, small[2]) and np.array_equal(_bits(e.read_accumulation()), _bits(small[1]))
    finally:
        e.close()
