"""The numpy model of the temporal reprojection (renderbaby_amd/temporal.py) against things that are not
the model: the pixel-centre rays it has to invert, expectations written by hand on inputs whose arithmetic is exact
(tests/_reproject_cases.py), and the statistics of accumulated noise.  No device, no library."""
import numpy as np
import pytest

from renderbaby_amd import abi, aov, scenes, temporal
from tests import _reproject_cases as cases
from tests._reproject_cases import bits

f32 = np.float32
EPS = 2.0 ** -24   # the unit roundoff of binary32: one operation's relative error


# ---- the inverse of the pixel-centre ray
@pytest.mark.parametrize("make", [scenes.cornell, scenes.feature_scene], ids=["cornell", "feature"])
@pytest.mark.parametrize("w,h", [(33, 17), (64, 48)])
@pytest.mark.parametrize("t", [0.5, 3.0, 40.0])
def test_projection_inverts_the_pixel_centre_ray(make, w, h, t):
    """P = pos + t d for the direction d of every pixel centre lands on the pixel's own displayed column and row.

    The bound, from the rounding of the steps (EPS per operation), with A = |a / z|, B = |b / z|:
      * P is rounded to binary32 once per component (it is worked out in binary64 here), e = P - pos once more:
        |delta e_k| <= EPS (|P_k| + |e_k|) =: eta_k.
      * z, a, b are dot products of e with unit vectors: three products and two sums, each EPS of at most |e|, on top of
        |eta|:  D = |eta| + 3 EPS |e|.
      * a / z inherits D / z from a and A D / z from z, and rounds once:  (D / z)(1 + A) + EPS A.
      * the direction itself is not exact: the model's d went through about a dozen rounded operations (two products and two
        sums per component, the normalisation's length, root and quotient), and the basis is orthonormal only to a few EPS
        (two normalisations and two cross products).  Each of these at most K = 16 steps moves a / z by at most
        EPS (1 + A + B).
      * the product with sx rounds once, EPS A sx, and the subtraction from cx once, EPS |X| <= EPS w.
    Together: sx ((D / z)(1 + A) + (K + 2) EPS (1 + A + B)) + EPS w -- of the order of 1e-4 px at these sizes."""
    u = np.asarray(make(width=w, height=h).uniforms, dtype=abi.UNIFORMS).reshape(-1)[0]
    view = temporal.view_from_camera(u)
    d = aov.pixel_centre_dirs(u).astype(np.float64)
    pos = np.asarray(u["camera"]["pos"], np.float64)
    P = (pos + t * d).astype(f32)
    X, Y, on = temporal.project(P, view, w, h)
    assert on.all()
    e = P.astype(np.float64) - pos
    z = e @ np.asarray(view["fwd"], np.float64)
    A = np.abs(e @ np.asarray(view["right"], np.float64)) / z
    B = np.abs(e @ np.asarray(view["up"], np.float64)) / z
    eta = np.sqrt(((EPS * (np.abs(P.astype(np.float64)) + np.abs(e))) ** 2).sum(-1))
    D = eta + 3 * EPS * np.sqrt((e * e).sum(-1))
    K = 16
    yy, xx = np.mgrid[0:h, 0:w]
    for got, want, s, n, R in ((X, xx, float(view["sx"]), w, A), (Y, yy, float(view["sy"]), h, B)):
        bound = s * ((D / z) * (1 + R) + (K + 2) * EPS * (1 + A + B)) + EPS * n
        err = np.abs(got.astype(np.float64) - want)
        print(f"{w} x {h}, t = {t}: error at most {err.max():.3g} px, bound at least {bound.min():.3g} and at most {bound.max():.3g} px")
        assert bound.max() < 2e-3, "the bound itself must stay a small fraction of a pixel"
        assert (err <= bound).all(), (err.max(), bound[err > bound][:4])


def test_view_of_a_scene_is_the_camera_the_rays_are_made_with():
    u = np.asarray(scenes.cornell(width=64, height=48).uniforms, dtype=abi.UNIFORMS).reshape(-1)[0]
    v = temporal.view_from_camera(u)
    assert v.dtype == abi.VIEW and np.array_equal(v["pos"], u["camera"]["pos"])
    assert v["cx"] == f32(31.5) and v["cy"] == f32(23.5)
    assert v.tobytes() == temporal.view_from_camera(u["camera"], 64, 48).tobytes()
    for a, b in (("right", "up"), ("right", "fwd"), ("up", "fwd")):
        assert abs(float(np.dot(v[a].astype(np.float64), v[b]))) < 1e-6
    # a camera that looks along y has no basis: the view is not finite, and nothing has history under it
    u["camera"]["dir"] = (0, 1, 0)
    bad = temporal.view_from_camera(u)
    assert not np.isfinite(bad["right"]).all()
    g = cases.flat_guides(cases.flat_view())
    assert not temporal.reproject(cases.prev_frame(), g, bad, g).any()


# ---- exact cases, bit for bit against hand-written expectations
EXACT = cases.exact_cases()
REJECT = cases.rejection_cases()


@pytest.mark.parametrize("case", EXACT, ids=[c[0] for c in EXACT])
def test_exact_cases(case):
    _, prev, pg, view, cg, p, want = case
    got = temporal.reproject(prev, pg, view, cg, p)
    assert got.dtype == f32 and np.array_equal(bits(got), bits(want)), (got[..., 0], want[..., 0])


def test_rejection_one_tap_at_a_time():
    """a rejected tap changes the result exactly as if it lay outside the frame: the expectation sums the other three"""
    assert len(REJECT) > 80
    _, prev, pg, view, cg, p, _ = REJECT[0]
    full = cases.tap_expectation(cases.prev_frame(), list(cases.TAPS))
    assert np.array_equal(bits(temporal.reproject(cases.prev_frame(), cases.flat_guides(view), view, cg, p)[cases.PIXEL]), bits(full))
    for name, prev, pg, view, cg, p, want in REJECT:
        got = temporal.reproject(prev, pg, view, cg, p)[cases.PIXEL]
        assert np.array_equal(bits(got), bits(want)), (name, got, want)
        if "at normal_min" in name or "at den" in name or "at -den" in name:
            assert np.array_equal(bits(want), bits(full)), name   # the edge itself is accepted


def test_a_tap_outside_the_frame_is_the_same_as_a_rejected_one():
    """the frame cut so that taps 1 and 3 of the pixel lie outside it, against the whole frame with those taps' class changed"""
    view = cases.flat_view()
    p = temporal.params(max_history=64.0)
    prev, pg, cg = cases.prev_frame(), cases.flat_guides(view), cases.flat_guides(view, shift_x=0.5, shift_y=0.5)
    for t in (cases.TAPS[1], cases.TAPS[3]):
        pg["cls"][t] = abi.HIT_SPHERE
    whole = temporal.reproject(prev, pg, view, cg, p)[cases.PIXEL]
    cut = 3   # columns 0 .. 2: the pixel's column is the last one (cx, sx stay the 8-wide frame's: the same projection)
    part = temporal.reproject(prev[:, :cut], cases.flat_guides(view)[:, :cut], view, cg[:, :cut], p)[cases.PIXEL]
    assert np.array_equal(bits(whole), bits(part)) and whole[3] > 0


def test_merge_cases_keep_bits_where_they_pass_through():
    hst, g, cur, want = cases.merge_cases()
    got = temporal.merge(hst, g, cur)
    assert np.array_equal(bits(got), bits(want)), (got, want)
    assert bits(got)[0, 3, 0] == 0x7FC12345 and bits(got)[0, 5, 3] == 0x7FC12345


def test_check_params_refuses_what_the_library_refuses():
    temporal.check_params(temporal.default_params())
    d = temporal.default_params()
    assert (float(d["sigma_depth"]), float(d["albedo_floor"])) == (float(f32(0.02)), float(f32(0.01)))
    for kw in (dict(sigma_depth=0.0), dict(sigma_depth=-1.0), dict(sigma_depth=np.nan), dict(sigma_depth=np.inf), dict(normal_min=1.5),
               dict(normal_min=-1.5), dict(normal_min=np.nan), dict(albedo_floor=0.0), dict(albedo_floor=np.inf), dict(max_history=0.5),
               dict(max_history=np.inf), dict(max_history=np.nan), dict(flags=1), dict(_reserved=(0, 0, 1))):
        with pytest.raises(ValueError):
            temporal.check_params(temporal.params(**kw))
    for kw in (dict(normal_min=-1.0), dict(normal_min=1.0), dict(max_history=1.0), dict(sigma_depth=1e-30)):
        temporal.check_params(temporal.params(**kw))
    with pytest.raises(ValueError):
        g = cases.flat_guides(cases.flat_view())
        temporal.reproject(cases.prev_frame()[:, :4], g, cases.flat_view(), g)


# ---- noise
def test_accumulated_noise_falls_as_one_over_the_count():
    """Two planes, the upper half of the frame one unit in front of the camera and the lower half two units, under a camera that
    moves 1 / 16 to the right per frame: the near plane moves two whole pixels per frame and the far plane one, so every
    projection is exact and a pixel with full history is the mean of 16 independent samples of its surface point.  Its noise
    variance is then sigma^2 / 16.  The estimate over N values (pixels x channels, independent) has the relative standard
    deviation sqrt(2 / (N - 1)); five of them is the margin."""
    w, h, frames, sigma = 64, 32, 16, 0.5
    rng = np.random.Generator(np.random.PCG64(2025))
    signal = np.array([[0.75, 0.5, 0.25], [0.25, 1.0, 0.5]], f32)
    near = (np.arange(h) < h // 2)[:, None] & np.ones((1, w), bool)

    def guides(view):
        a, b = cases.flat_guides(view, w, h, depth=1.0, cls=abi.HIT_TRIANGLE, albedo=0.5), cases.flat_guides(view, w, h, depth=2.0, cls=abi.HIT_GROUND, albedo=0.25)
        return np.where(near, a, b)

    p = temporal.default_params()
    F = g_prev = v_prev = None
    for k in range(frames):
        view = cases.flat_view(w, h, cam_x=k / 16)
        g = guides(view)
        cur = np.empty((h, w, 4), f32)
        cur[..., :3] = np.where(near[..., None], signal[0], signal[1]) + rng.normal(0, sigma, (h, w, 3)).astype(f32)
        cur[..., 3] = 1
        hist = np.zeros_like(cur) if F is None else temporal.reproject(F, g_prev, v_prev, g, p)
        F, g_prev, v_prev = temporal.merge(hist, g, cur), g, view
    count = F[..., 3]
    assert set(np.unique(count)) <= set(float(c) for c in range(1, frames + 1)), "exact shifts: whole counts only"
    full = count == frames
    # the near plane loses 2 x 15 columns of 64, the far plane 15
    assert full[near].sum() == (h // 2) * (w - 30) and full[~near].sum() == (h // 2) * (w - 15)
    noise = (F[..., :3] - np.where(near[..., None], signal[0], signal[1])).astype(np.float64)
    for c in (frames, frames // 2):
        m = count == c
        n = int(m.sum()) * 3
        var = float((noise[m] ** 2).mean())
        margin = 5 * np.sqrt(2 / (n - 1))
        print(f"count {c}: variance {var:.5f} over {n} values, sigma^2 / count {sigma * sigma / c:.5f}, margin {margin:.3f}")
        assert abs(var / (sigma * sigma / c) - 1) <= margin, (c, var, n)
