"""The denoiser's kernels (csrc/rb_denoise.hip) at degenerate inputs and awkward frames, where tests/test_gpu_denoise.py stops:
guide and colour values no renderer should produce but one can (zero normals of zero-area triangles, t <= 0, NaN, inf, class
words of the caller's invention), subnormal weights and colours, values at which the filter itself generates NaN, engine
frames of odd width, and a frame large enough for the guide build's second piece.  DESIGN.md section 13.5 has the tables.

The reference is the numpy model (renderbaby_amd/denoise.py), itself held to the per-pixel loops of tests/_denoise_scalar.py
by tests/test_denoise_scalar.py.  Sections 1 and 2 compare every word and byte with no exception; what allows that -- no
non-finite word at a live pixel of finite colour -- is asserted from the model.  Section 3 is the one place with an
exception, the one section 13.1 names: a NaN the filter generates has no specified sign or payload.
"""
import time

import numpy as np
import pytest

from renderbaby_amd import Engine, RenderConfig, abi, denoise, engine, scenes
from tests import _denoise_scalar as S
from tests.conftest import has_gpu
from tests.test_gpu_denoise import bits, engine_frames
from tests.test_gpu_query import _engine

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

f32 = np.float32
VARIANTS = ("plain", "lds")
# 5 iterations: the plain kernel (the only one from step 4 up) also at steps 4, 8 and 16
GRID = [dict(iterations=i, sigma_color=sc, normal_power_log2=n) for i in (3, 5) for sc in (0.0, 2.0) for n in (0, 3, 10)]

_model = {}


def model(key, c, g, kw):
    """(linear, rgba) of the numpy model, computed once per frame and parameter set and never written to"""
    k = (key, tuple(sorted(kw.items())))
    if k not in _model:
        _model[k] = denoise.filter(c, g, denoise.params(**kw), rgba=True)
        for a in _model[k]:
            a.setflags(write=False)
    return _model[k]


def live_of(c, g):
    return (g["cls"] != 0) & np.isfinite(c).all(-1)


def exact(key, c, g, kw, want_finite=True):
    """the device against the model: every word, every byte"""
    want_lin, want_img = model(key, c, g, kw)
    if want_finite:   # (from the model alone: what makes "every bit" a fair demand)
        assert np.isfinite(want_lin[live_of(c, g)]).all(), (key, kw, "the model has a non-finite word at a live pixel of finite colour")
    lin, img = engine.denoise_buffers(c, g, denoise.params(**kw), device=0)
    bad = np.nonzero((bits(lin) != bits(want_lin)).any(-1))
    assert len(bad[0]) == 0, (key, kw, len(bad[0]), bad[0][:4], bad[1][:4], lin[bad][:4], want_lin[bad][:4])
    assert np.array_equal(img, want_img), (key, kw)
    return want_lin


def falls_back(c, g, y, x, kw):
    """whether pixel (y, x), at least 2 from every border, takes the wsum == 0 fallback in iteration 0: the loops of
    tests/_denoise_scalar.py on the 5 x 5 pixels its taps read"""
    crop = (slice(y - 2, y + 3), slice(x - 2, x + 3))
    _, k = S.filter_scalar(c[crop], g[crop], denoise.params(**dict(kw, iterations=1)))
    return (2, 2) in k["iterations"][0]["fallback_at"]   # (normal_power_log2 = 3 in the callers: at 0 a normal of 1e-39 keeps a subnormal weight)


def inner(at, live):
    """the planted live pixels at least 2 from every border"""
    m = at & live
    m[:2], m[-2:], m[:, :2], m[:, -2:] = False, False, False, False
    return list(zip(*np.nonzero(m)))


# ---- 1. quiet hazards: bit for bit, no exception
FALLS_BACK = {"normal": S.QUIET["normal"], "t": (0.0, S.NAN), "pos": (S.NAN, S.INF, -S.INF)}   # every w of the planted pixel is 0
QUIET_CASES = [(f, v) for f, vs in S.QUIET.items() for v in vs]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("field,value", QUIET_CASES, ids=[f"{f}={v!r}" for f, v in QUIET_CASES])
def test_each_quiet_value_equals_the_model(field, value, variant, monkeypatch):
    """one value of one field at 1 % of a 37 x 53 frame"""
    monkeypatch.setenv("RB_DENOISE_VARIANT", variant)
    c, g, at = S.frame_with(field, value)
    live = live_of(c, g)
    assert (at & live).sum() >= 10
    for kw in GRID:
        exact((field, repr(value)), c, g, kw)
    if any(value == v or (value != value and v != v) for v in FALLS_BACK.get(field, ())):
        spots = inner(at, live)
        assert spots and all(falls_back(c, g, y, x, GRID[1]) for y, x in spots[:3]), "no planted pixel took the wsum == 0 fallback"


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("value", S.PASS_THROUGH, ids=repr)
def test_a_non_finite_colour_passes_through(value, variant, monkeypatch):
    monkeypatch.setenv("RB_DENOISE_VARIANT", variant)
    c, g, at = S.frame_with("color", value)
    assert (at & (g["cls"] != 0)).sum() >= 10
    for kw in GRID:
        want = exact(("pass", repr(value)), c, g, kw)
        assert np.array_equal(bits(want[..., :3])[at], bits(c)[at])   # class 0 now: copied, and (by the finiteness above) read by no tap


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("h,w", [(37, 53), (15, 15), (16, 16), (17, 31), (31, 17), (1, 64), (64, 1), (3, 130)])
def test_every_quiet_value_together_equals_the_model(h, w, variant, monkeypatch):
    """tile remainders of 15, 0 and 1 for the 16 x 16 tiles, of 1 and 2 columns and 1 and 3 rows for the 64 x 4 ones; with 5
    iterations the steps pass the frame's size in every one but the first"""
    monkeypatch.setenv("RB_DENOISE_VARIANT", variant)
    c, g, planted = S.frame_with_everything(h, w)
    live = live_of(c, g)
    for kw in GRID:
        exact(("everything", h, w), c, g, kw)
    if (h, w) == (37, 53):
        assert all((planted[f] & live).sum() >= 10 for f in planted if f != "color")
        spots = inner(planted["normal"], live)
        assert spots and any(falls_back(c, g, y, x, GRID[1]) for y, x in spots[:6])


@pytest.mark.parametrize("variant", VARIANTS)
def test_subnormal_weights_equal_the_model(variant, monkeypatch):
    """w_n = dot^1024 in and under the subnormal range at every tap, the centre's too (S.subnormal_weight_frame): wsum is
    subnormal or 0 at many pixels, the quotients sum / wsum have subnormal operands.  A translation unit that flushed them
    (or a division that does not take them) gives other words, or falls back where the model does not."""
    monkeypatch.setenv("RB_DENOISE_VARIANT", variant)
    c, g = S.subnormal_weight_frame()
    _, k = S.filter_scalar(c[:12, :12], g[:12, :12], denoise.params(iterations=1, normal_power_log2=10))
    k = k["iterations"][0]
    print("subnormal weights, 12 x 12 corner, iteration 0:", {a: v for a, v in k.items() if a != "fallback_at"})
    assert k["subnormal_w"] > 1000 and k["zero_w"] > 0 and k["nan_generated"] == 0
    for kw in (dict(iterations=3, normal_power_log2=10), dict(iterations=5, normal_power_log2=10, sigma_color=2.0)):
        want = exact("subnormal-w", c, g, kw)
        assert not np.array_equal(bits(want[..., :3]), bits(c)), "every pixel fell back: the small weights decided nothing"


@pytest.mark.parametrize("variant", VARIANTS)
def test_subnormal_colours_equal_the_model(variant, monkeypatch):
    """colours scaled by 2^-130: demodulation, w * r_q, the sums, sum / wsum and remodulation have subnormal operands and
    results"""
    monkeypatch.setenv("RB_DENOISE_VARIANT", variant)
    c, g = S.subnormal_color_frame()
    _, k = S.filter_scalar(c[:12, :12], g[:12, :12], denoise.params(iterations=1))
    print("subnormal colours, 12 x 12 corner, iteration 0:", {a: v for a, v in k["iterations"][0].items() if a != "fallback_at"})
    assert k["iterations"][0]["subnormal_results"] > 100
    for kw in GRID:
        want = exact("subnormal-c", c, g, kw)
        a = np.abs(want[..., :3])
        assert ((a > 0) & (a < S.TINY)).sum() > 1000, "the model's output has no subnormal words"


# ---- 2. loud hazards: which words are NaN is specified, their sign and payload are not
LOUD_PARAMS = (dict(), dict(sigma_color=2.0), dict(normal_power_log2=10))


def spreads(field, iterations):
    """whether one pixel with a loud value of `field` can make a NaN at ANOTHER pixel within `iterations`: normal and colour are
    read by every tap that looks at the pixel; t enters only the pixel's own den, so its NaN needs a second iteration to be
    read by a neighbour; albedo enters only the pixel's own m, after the last iteration, and never reaches anyone"""
    return field in ("normal", "color") or (field == "t" and iterations >= 2)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("iterations", [1, 2])
@pytest.mark.parametrize("field,value", S.LOUD, ids=[f"{f}={v!r}" for f, v in S.LOUD])
def test_each_loud_value_equals_the_model_up_to_the_bits_of_a_generated_nan(field, value, iterations, variant, monkeypatch):
    """33 x 35, one pixel near the middle.  Where the model's word is a NaN the device's is a NaN, of any sign and payload;
    every other word is equal, and so is every byte (a NaN channel maps to 0 on both sides).  The frame holds no NaN, so every
    NaN of the output is generated.  With the colour term off, colour +-3e38 only makes inf words (compared exactly): its NaN
    condition is asserted with the term on."""
    monkeypatch.setenv("RB_DENOISE_VARIANT", variant)
    c, g, (y, x) = S.loud_frame(field, value)
    assert not np.isnan(c).any() and not any(np.isnan(g[f]).any() for f in ("normal", "t", "pos", "albedo"))
    live = g["cls"] != 0
    for extra in LOUD_PARAMS:
        kw = dict(extra, iterations=iterations)
        want_lin, want_img = model(("loud", field, repr(value)), c, g, kw)
        nan = np.isnan(want_lin)
        # -- the conditions, from the model alone
        assert nan.sum() * 4 <= live.sum() * 3, "NaN words are more than a quarter of the live words"
        if extra == (dict(sigma_color=2.0) if field == "color" else dict()):
            elsewhere = nan.any(-1) & live
            elsewhere[y, x] = False
            if spreads(field, iterations):
                assert elsewhere.any(), "no generated NaN at a live pixel other than the planted one: the case tests nothing"
            else:
                assert not elsewhere.any() and not np.isfinite(want_lin[y, x, :3]).all()
        # -- the device
        lin, img = engine.denoise_buffers(c, g, denoise.params(**kw), device=0)
        assert np.array_equal(np.isnan(lin), nan), (field, value, kw, "other words are NaN")
        assert np.array_equal(bits(lin)[~nan], bits(want_lin)[~nan]), (field, value, kw)
        assert np.array_equal(img, want_img), (field, value, kw)
        assert (want_img[..., :3][nan[..., :3]] == 0).all()


# ---- 3. the engine path at odd shapes
ODD_SHAPES = [(1, 1), (17, 9), (65, 5), (131, 3)]
ODD_SCENES = {"cornell": lambda w, h: scenes.cornell(w, h, 2, 4), "feature": lambda w, h: scenes.feature_scene(width=w, height=h, spp=2)}


@pytest.mark.parametrize("w,h", ODD_SHAPES)
@pytest.mark.parametrize("name", ODD_SCENES)
def test_engine_denoise_equals_the_model_at_odd_shapes(name, w, h):
    """widths that are odd and no multiple of 16 or 64, through the mirrored read of the accumulation (k_dn_prepare) and the
    mirrored ray of k_guide_pack"""
    for p in (denoise.default_params(), denoise.params(iterations=5, sigma_color=4.0, normal_power_log2=5)):
        want_lin, want_img, lin, img, d_lin, d_img, g, _, _ = engine_frames(lambda: ODD_SCENES[name](w, h), dict(), p)
        assert w * h == 1 or (g["cls"] != 0).any(), "the scene must have something to filter"
        assert np.array_equal(bits(lin), bits(want_lin)), (name, w, h)
        assert np.array_equal(img, want_img), (name, w, h)
        assert np.array_equal(bits(d_lin), bits(lin)) and np.array_equal(d_img, img), "host and device forms differ"


@pytest.mark.parametrize("w,h", ODD_SHAPES)
@pytest.mark.parametrize("name", ODD_SCENES)
def test_guides_against_the_records_at_odd_shapes(name, w, h):
    s = ODD_SCENES[name](w, h)
    e = _engine(s)
    try:
        hits, surf = e.render_hits(surfaces=True)
        g = e.denoise_guides()
    finally:
        e.close()
    assert np.array_equal(bits(g["normal"]), bits(hits["normal"])) and np.array_equal(bits(g["t"]), bits(hits["t"]))
    assert np.array_equal(bits(g["albedo"]), bits(surf["albedo"]))
    k = hits["kind"]
    filterable = np.isin(k, (abi.HIT_GROUND, abi.HIT_TRIANGLE, abi.HIT_SPHERE)) & ~(surf["emissive"] > 0).any(-1)
    assert np.array_equal(g["cls"], np.where(filterable, k, 0))
    hit = (k != abi.HIT_NONE) & (k != abi.HIT_INVALID)
    if hit.any():
        cam = np.asarray(s.uniforms["camera"]["pos"], np.float64).reshape(3)
        t = hits["t"][hit].astype(np.float64)
        assert (np.abs(np.sqrt(((g["pos"][hit].astype(np.float64) - cam) ** 2).sum(-1)) - t) / t <= 1e-5).all()
    m = denoise.guides_from_records(s.uniforms, hits, surf)   # (its pos mirrors x by itself: an odd width has a middle column)
    for f in ("normal", "t", "albedo", "cls"):
        assert np.array_equal(bits(m[f]), bits(g[f])), f
    if hit.any():
        assert (np.abs(m["pos"][hit].astype(np.float64) - g["pos"][hit]).max(-1) <= 1e-5 * t).all()


def test_a_zero_weight_accumulation_denoises_to_black():
    """after the first update and before any dispatch acc.w is 0 everywhere: c = 0 by the mean-radiance rule, and every step
    keeps +0 -- (0, 0, 0, 1), and (0, 0, 0, 255) in bytes"""
    for w, h in ((17, 9), (64, 48)):
        e = _engine(scenes.feature_scene(width=w, height=h, spp=2))
        try:
            assert not e.read_accumulation().any()
            for p in (denoise.default_params(), denoise.params(iterations=0), denoise.params(iterations=5, sigma_color=4.0)):
                lin, img = e.denoise(p, linear=True), e.denoise(p)
                assert np.array_equal(bits(lin), bits(np.broadcast_to(np.array([0, 0, 0, 1], f32), (h, w, 4))))
                assert np.array_equal(img, np.broadcast_to(np.array([0, 0, 0, 255], np.uint8), (h, w, 4)))
        finally:
            e.close()


def test_guides_of_a_second_piece():
    """2048 x 2056 is the smallest frame whose guide build (ensure_guides) takes a second piece: 2^22 rays are 2048 rows of
    2048, the last 8 rows come from a second launch.  The guides at 64 pixels -- both sides of the seam, the corners, the last
    row -- against rb_pick, a single-ray launch that shares no piece loop with the build; and denoise(iterations = 0) of the
    whole frame against the render's own.  The numpy model is not run at this size.  Measured on one MI355X: 0.03 s for the
    whole test, engine and render included (under 0.1 s by pytest's own clock), so the whole-frame comparison stays."""
    w, h = 2048, 2056
    s = scenes.feature_scene(width=w, height=h, spp=1, max_depth=2)
    rc = RenderConfig.from_scene(s)
    t0 = time.perf_counter()
    e = Engine.new(rc, device=0)
    try:
        frame = e.render(rc).pixels
        t1 = time.perf_counter()
        g = e.denoise_guides()
        t2 = time.perf_counter()
        assert e.last_denoise_ms()[1] > 0.0, "the guides were not built by this call"
        where = [(y, x) for y in (2046, 2047, 2048, 2049) for x in (0, 1, 1023, 2046, 2047)]
        where += [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)] + [(h - 1, int(x)) for x in np.linspace(1, w - 2, 40)]
        assert len(set(where)) == 64
        classes = set()
        for y, x in where:
            hit, surf = e.pick(x, y)
            for f, rec in (("normal", hit["normal"]), ("t", hit["t"]), ("albedo", surf["albedo"])):
                assert np.array_equal(bits(g[f][y, x]), bits(rec)), (y, x, f, g[f][y, x], rec)
            k = int(hit["kind"])
            cls = k if k in (abi.HIT_GROUND, abi.HIT_TRIANGLE, abi.HIT_SPHERE) and not (surf["emissive"] > 0).any() else 0
            assert int(g["cls"][y, x]) == cls, (y, x)
            classes.add(cls)
        assert len(classes) >= 2, "the 64 pixels all look at one thing"
        assert np.array_equal(e.denoise(denoise.params(iterations=0)), frame)
    finally:
        e.close()
    t3 = time.perf_counter()
    print(f"second guide piece, {w} x {h}: {t3 - t0:.2f} s (engine and render {t1 - t0:.2f}, guides {t2 - t1:.2f}, picks and frame {t3 - t2:.2f})")
