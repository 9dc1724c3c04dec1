"""The path state of k_trace across the joins of its persistent loop (trace_body in rb_kernels.hip): a lane's Path, its
item and its active flag live in one set of registers from the refill rounds through the three exits of a segment (sky,
absorbed, scattered) to the loop's back edge, every exit updating its own fields in place.  Everything below is bit for
bit against the oracle -- accumulation words, RGBA8, segment and path counts -- on the smallest frames at which a join
could hand a lane another lane's or a stale field:
 * a 64 x 40 Cornell frame with reservations of 256 items, which launch_render gives the staged k_trace (the shape and
   the forced batch of tests/test_gpu_staged_starts.py), and an 8 x 8 and a 9 x 7 frame, whose 64-item reservations run
   k_trace_direct (Engine.last_kernel_name() says "k_trace" for both: the form follows from the batch alone);
 * max_depth 0 (no lane ever becomes active), 1 (every lane ends in its first segment, whichever exit it takes), 2 and 8;
   1 and 3 samples; the sky is blue here, not the Cornell scene's black, so that a sky exit adds att * sky to the colour
   and a wrong att or colour at that exit shows in the words;
 * test_the_cases_cover_the_exits proves from the oracle alone that the frames hold what they are meant to: paths that
   end on the sky through the open front, paths absorbed on a metal sphere, paths cut at max_depth, padding pixels;
 * one STATS render per frame: same words, same counters.
A lane that is refilled in the SECOND round of one iteration cannot be shown from the oracle: it depends on how the
device's waves drain their reservations.  On the frames above it never happens (every wave's only reservation is its own
first one; the second round runs there, finds the queue empty and ends the refill).  test_second_refill_round adds the
smallest frames on which arithmetic forces it -- one block per CU and several reservations per wave, so that a wave
comes to the end of a partly used reservation with more idle lanes than items -- and checks them like the others; that
the round was taken is reasoned there, not asserted."""
import dataclasses

import numpy as np
import pytest

from renderbaby_amd import Engine, RenderConfig, scenes
from tests import _oracle

pytestmark = pytest.mark.gpu

SKY = (0.5, 0.7, 1.0)
FRAMES = {"staged-64x40": (64, 40, dict(queue_batch=256)), "direct-8x8": (8, 8, {}), "direct-9x7": (9, 7, {})}
DEPTHS = (0, 1, 2, 8)
SPPS = (1, 3)

_cache = {}


def _scene(w, h, spp, depth, sky=SKY, plastic=False):
    s = scenes.cornell(w, h, spp, depth)
    u = s.uniforms.copy()
    u["sky_color"] = sky
    spheres = s.spheres
    if plastic:   # the same spheres, none of them metal: nothing absorbs
        spheres = s.spheres.copy()
        for k in range(len(spheres)):
            spheres[k]["material"] = scenes.sphere_material("plastic", (0.5, 0.5, 0.5))
    return dataclasses.replace(s, uniforms=u, spheres=spheres)


def _want(w, h, spp, depth, **kw):
    """the oracle's frame, rendered once per module and never written to"""
    key = (w, h, spp, depth, tuple(sorted(kw.items())))
    if key not in _cache:
        s = _scene(w, h, spp, depth, **kw)
        acc, _, rgba, st = _oracle.render(s)
        assert st["paths"] == w * h * spp, st
        for a in (acc, rgba):
            a.setflags(write=False)
        _cache[key] = (s, acc, rgba, st)
    return _cache[key]


def _check(w, h, spp, depth, **engine_kw):
    s, o_acc, o_rgba, o_st = _want(w, h, spp, depth)
    rc = RenderConfig.from_scene(s)
    e = Engine.new(rc, **engine_kw)
    try:
        f = e.render(rc)
        acc, px, st, name = e.read_accumulation(), f.pixels, e.stats(), e.last_kernel_name()
    finally:
        e.close()
    assert name == "k_trace"
    assert np.array_equal(acc.view(np.uint32), o_acc.view(np.uint32)), (w, h, spp, depth, engine_kw)
    assert np.array_equal(px, o_rgba), (w, h, spp, depth, engine_kw)
    assert st["segments"] == o_st["segments"] and st["paths"] == o_st["paths"], (st, o_st)


@pytest.mark.parametrize("spp", SPPS)
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("frame", list(FRAMES))
def test_frame_and_counters(frame, depth, spp):
    w, h, kw = FRAMES[frame]
    _check(w, h, spp, depth, **kw)


@pytest.mark.parametrize("frame", list(FRAMES))
def test_stats_instantiation(frame):
    # the counting instantiations share the loop: same frame, same counters
    w, h, kw = FRAMES[frame]
    _check(w, h, 3, 8, stats=True, **kw)


def test_the_cases_cover_the_exits():
    for w, h, _ in FRAMES.values():
        # sky: with a black sky the same paths give another frame, so some path ended on the sky and added att * sky
        blue, black = _want(w, h, 3, 8), _want(w, h, 3, 8, sky=(0.0, 0.0, 0.0))
        assert blue[3] == black[3] and not np.array_equal(blue[1], black[1]), (w, h)
        # (after a bounce, through the open front: every primary ray of these frames meets the box)
        # cut at max_depth: one more bounce allowed gives more segments, so some path was alive when depth 8 cut it;
        # and at depth 2 some path scattered into a second segment while some other ended in its first
        assert _want(w, h, 3, 9)[3]["segments"] > blue[3]["segments"], (w, h)
        d2 = _want(w, h, 3, 2)[3]
        assert d2["paths"] < d2["segments"] < 2 * d2["paths"], d2
    # absorbed on a metal sphere: the first segments of a frame do not depend on the materials, so with the same spheres
    # in plastic the paths that end in their first segment are the sky's alone; the metal frame loses more
    w, h, _ = FRAMES["staged-64x40"]
    metal, plastic = _want(w, h, 3, 2)[3], _want(w, h, 3, 2, plastic=True)[3]
    assert metal["paths"] == plastic["paths"] and metal["segments"] < plastic["segments"], (metal, plastic)
    # padding: 9 x 7 is two 8 x 8 tiles, 128 items per sample for 63 pixels
    w, h, _ = FRAMES["direct-9x7"]
    assert _want(w, h, 3, 8)[3]["paths"] == 63 * 3 < 128 * 3


@pytest.mark.parametrize("batch,spp", [(64, 32), (256, 96)], ids=["direct", "staged"])
def test_second_refill_round(batch, spp):
    # one block of four waves per CU: at most 4 * 304 waves on any device of this family, 256 * 4 on MI355X.  128 x 64 pixels
    # at 32 (96) samples are 262 144 (786 432) items: four (three) reservations of 64 (256) for each of 1 024 waves.  Lanes
    # end at different depths, so a wave reaches the end of a reservation with fewer items left than idle lanes: the first
    # round hands out the rest, the second reserves again and serves the others in the same iteration.
    w, h = 128, 64
    assert (w // 8) * (h // 8) * 64 * spp >= 2 * batch * 4 * 304
    _check(w, h, spp, 8, queue_batch=batch, blocks_per_cu=1)
