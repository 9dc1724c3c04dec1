"""The numpy model of the denoiser (renderbaby_amd/denoise.py) against a second, independent restatement of DESIGN.md section
13.1: the per-pixel loops of tests/_denoise_scalar.py.  The model is one vectorisation (shifted arrays, `take` masks, np.where)
of the text; a misreading that the model and the kernels share would pass every device test, and is caught here.  No device.

Every comparison is on the uint32 words of the linear vec4.  The inputs are the well-behaved frames of
tests/test_gpu_denoise.py and the frames with degenerate values that tests/test_gpu_denoise_edges.py gives the device
(DESIGN.md section 13.5), small enough for the loops; the loops' counters prove that each frame met what it was made for.
"""
import numpy as np
import pytest

from renderbaby_amd import abi, denoise
from tests import _denoise_scalar as S
from tests.test_gpu_denoise import synthetic

f32 = np.float32
ITERATIONS, SIGMA_COLOR, NORMAL_POWER = (0, 1, 3), (0.0, 2.0), (0, 3, 10)

_runs = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def both(key, c, g, **kw):
    """(model, loops, counters) of one frame and parameter set; each pair is computed once per session and never written to"""
    k = (key, tuple(sorted(kw.items())))
    if k not in _runs:
        p = denoise.params(**kw)
        want = denoise.filter(c, g, p)
        got, counters = S.filter_scalar(c, g, p)
        for a in (want, got):
            a.setflags(write=False)
        _runs[k] = (want, got, counters)
    return _runs[k]


def same(key, c, g, **kw):
    want, got, counters = both(key, c, g, **kw)
    bad = np.nonzero((bits(want) != bits(got)).any(-1))
    assert len(bad[0]) == 0, (key, kw, len(bad[0]), bad[0][:4], bad[1][:4], want[bad][:4], got[bad][:4])
    return want, counters


def live_of(c, g):
    return (g["cls"] != 0) & np.isfinite(c).all(-1)


def total(counters, name):
    return sum(k[name] for k in counters["iterations"])


# ---- the counters themselves, on a frame small enough to count by hand
def test_the_counters_count():
    """1 x 3, classes TRIANGLE TRIANGLE SPHERE, one iteration: of a pixel's 25 taps only those of its own row can be inside the
    frame; pixel 0 has taps at x = 0, 1, 2, pixel 1 at 0, 1, 2, pixel 2 at 0, 1, 2 -- 9 inside, 66 outside, and 4 of the 9 look at
    the other class.  The middle normal is zero: its own taps weigh nothing (fallback), and the tap pixel 0 takes from it is 0."""
    c = np.ones((1, 3, 3), f32)
    g = np.zeros((1, 3), abi.GUIDE)
    g["cls"] = [[abi.HIT_TRIANGLE, abi.HIT_TRIANGLE, abi.HIT_SPHERE]]
    g["normal"] = [[(0, 1, 0), (0, 0, 0), (0, 1, 0)]]
    g["t"], g["albedo"] = 1, 0.5
    out, k = S.filter_scalar(c, g, denoise.params(iterations=1))
    k = k["iterations"][0]
    assert (k["frame_skipped"], k["class_skipped"]) == (66, 4)
    assert (k["fallback"], k["fallback_at"], k["zero_w"]) == (1, [(0, 1)], 3)
    assert (k["subnormal_w"], k["subnormal_results"], k["nan_generated"]) == (0, 0, 0)
    assert np.array_equal(bits(out), bits(denoise.filter(c, g, denoise.params(iterations=1))))


# ---- 1. well-behaved frames
# (the largest frame with one normal power and 0 and 3 iterations only: the loops take a second there)
SYNTHETIC_CASES = [(h, w, i, sc, n) for h, w in ((14, 19), (1, 9), (7, 1), (20, 24)) for i in ITERATIONS for sc in SIGMA_COLOR for n in NORMAL_POWER
                   if (h, w) != (20, 24) or (n == 3 and i != 1)]


@pytest.mark.parametrize("h,w,iterations,sigma_color,npow", SYNTHETIC_CASES)
def test_model_equals_the_loops_on_synthetic_frames(h, w, iterations, sigma_color, npow):
    c, g = synthetic(h, w, 500 + h * w)
    _, k = same(("synthetic", h, w), c, g, iterations=iterations, sigma_color=sigma_color, normal_power_log2=npow)
    assert len(k["iterations"]) == iterations
    if iterations:
        assert total(k, "frame_skipped") > 0 and total(k, "fallback") == 0
        assert h * w < 100 or total(k, "class_skipped") > 0


# ---- 2. every quiet hazard at once: the full grid of parameters
@pytest.mark.parametrize("iterations", ITERATIONS)
@pytest.mark.parametrize("sigma_color", SIGMA_COLOR)
@pytest.mark.parametrize("npow", NORMAL_POWER)
def test_model_equals_the_loops_with_every_quiet_hazard_together(iterations, sigma_color, npow):
    c, g, planted = S.frame_with_everything(14, 19)
    want, k = same("everything", c, g, iterations=iterations, sigma_color=sigma_color, normal_power_log2=npow)
    live = live_of(c, g)
    assert all((planted[f] & live).any() for f in ("normal", "t", "pos", "albedo", "cls")), "a field was planted at no live pixel"
    assert np.isfinite(want[live]).all(), "the quiet values are not quiet together"
    assert np.array_equal(bits(want[..., :3])[~live], bits(c)[~live])
    if iterations:
        assert total(k, "fallback") > 0 and total(k, "zero_w") > 0 and total(k, "class_skipped") > 0 and total(k, "frame_skipped") > 0


# ---- 3. each quiet value alone
FALLS_BACK = {"normal": S.QUIET["normal"], "t": (0.0, S.NAN), "pos": (S.NAN, S.INF, -S.INF)}   # the planted pixel's every w is 0
QUIET_CASES = [(f, v) for f, vs in S.QUIET.items() for v in vs]


def _falls_back(field, value):
    return any(value == v or (value != value and v != v) for v in FALLS_BACK.get(field, ()))


@pytest.mark.parametrize("field,value", QUIET_CASES, ids=[f"{f}={v!r}" for f, v in QUIET_CASES])
def test_model_equals_the_loops_for_each_quiet_value(field, value):
    c, g, at = S.frame_with(field, value, 12, 13, seed=21)
    c0, g0 = S.benign(12, 13, 21)
    live = live_of(c, g)
    assert (at & live).any()
    for kw in (dict(iterations=3, sigma_color=2.0), dict(iterations=1, normal_power_log2=10)):
        want, k = same((field, repr(value)), c, g, **kw)
        assert np.isfinite(want[live]).all(), "a quiet value produced a non-finite word"
        assert all(i["nan_generated"] == 0 for i in (k["prepare"], k["finish"]))
        first = k["iterations"][0]
        if _falls_back(field, value):
            ys, xs = np.nonzero(at & live)
            assert set(zip(ys.tolist(), xs.tolist())) <= set(first["fallback_at"]), "a planted pixel found a weight"
            if field == "normal":
                assert first["zero_w"] > 0
        if field == "cls":
            k0 = both(("benign", 21), c0, g0, **kw)[2]
            assert first["class_skipped"] > k0["iterations"][0]["class_skipped"], "the planted class words separated nothing"
            assert first["fallback"] == 0, "a pixel of a planted class is live and has at least its own tap"
        changed = (bits(want) != bits(both(("benign", 21), c0, g0, **kw)[0])).any(-1)
        assert changed.any(), "the value changed nothing: the case tests nothing"


@pytest.mark.parametrize("value", S.PASS_THROUGH, ids=repr)
def test_a_non_finite_colour_makes_its_pixel_class_zero(value):
    c, g, at = S.frame_with("color", value, 12, 13, seed=22)
    assert (at & (g["cls"] != 0)).any()
    want, k = same(("pass", repr(value)), c, g, iterations=3, sigma_color=2.0)
    assert np.array_equal(bits(want[..., :3])[at], bits(c)[at]), "a non-finite pixel is copied bit for bit"
    live = live_of(c, g)
    assert not (live & at).any() and np.isfinite(want[live]).all()
    g0 = g.copy()
    g0["cls"][at] = 0   # the same frame with the class word cleared by hand: the same output everywhere else
    assert np.array_equal(bits(denoise.filter(c, g0, denoise.params(iterations=3, sigma_color=2.0)))[~at], bits(want)[~at])
    assert all(i["nan_generated"] == 0 for i in k["iterations"]), "a class 0 pixel was read by a tap"


# ---- 4. the loud values: the loops and the model agree on every word here too (both are numpy on one host)
@pytest.mark.parametrize("field,value", S.LOUD, ids=[f"{f}={v!r}" for f, v in S.LOUD])
@pytest.mark.parametrize("iterations", [1, 2])
def test_model_equals_the_loops_for_each_loud_value(field, value, iterations):
    c, g, (y, x) = S.loud_frame(field, value, 13, 15)
    for kw in (dict(), dict(sigma_color=2.0), dict(normal_power_log2=10)):
        want, k = same(("loud", field, repr(value)), c, g, iterations=iterations, **kw)
        made = sum(i["nan_generated"] for i in k["iterations"]) + k["prepare"]["nan_generated"] + k["finish"]["nan_generated"]
        assert not np.isfinite(want[..., :3]).all(), "a loud value left every word finite"
        assert made > 0 or not np.isnan(want).any(), "NaN words in the output of a frame that holds none, and none was generated"


# ---- 5. subnormal weights, subnormal colours
def test_model_equals_the_loops_on_subnormal_weights():
    c, g = S.subnormal_weight_frame(12, 13)
    want, k = same("subnormal-w", c, g, iterations=3, normal_power_log2=10)
    first = k["iterations"][0]
    assert first["subnormal_w"] > 100 and first["zero_w"] > 0 and first["nan_generated"] == 0
    assert np.isfinite(want).all()
    # without its small weights the frame comes out differently: they are not lost beside a large centre weight
    flushed = g.copy()
    flushed["normal"] *= f32(0.5)   # every dot a quarter: every w_n underflows to 0, every pixel falls back
    assert not np.array_equal(bits(denoise.filter(c, flushed, denoise.params(iterations=3, normal_power_log2=10))), bits(want))


def test_model_equals_the_loops_on_subnormal_colours():
    c, g = S.subnormal_color_frame(12, 13)
    for kw in (dict(iterations=3), dict(iterations=3, sigma_color=2.0)):
        want, k = same("subnormal-c", c, g, **kw)
        assert total(k, "subnormal_results") > 100 and total(k, "nan_generated") == 0
        a = np.abs(want[..., :3])
        assert ((a > 0) & (a < S.TINY)).sum() > 100, "no subnormal word in the output"
