"""The numpy model of the pick per grid cell (renderbaby_amd/direct.py: emitter_bounds, grid_weights, emitter_grid_cdf, grid_cell,
rays(grid=...)) held to its definition: the bounds against float64, the quantised rows and what is
weighable in them, the weight at its edges, the cell of a position against exact rational arithmetic, the two identities that
tie the new pick to section 23's bit for bit, malformed rows, and the factor float(Q) / float(q) as the estimator sees it --
the same integral as a sum over every emitter alone, with less noise than the pick by power where the lights are many."""
from fractions import Fraction

import numpy as np
import pytest

from renderbaby_amd import abi, direct, hemisphere, scenes
from tests.test_direct_cdf_model import FLT_MAX, GARBAGE, TOP, feature_surfels, same_bits, scalar_search, steps, table
from tests.test_direct_model import _u32

f32, u32 = np.float32, np.uint32
TRI, SPH, LGT = abi.HIT_TRIANGLE, abi.HIT_SPHERE, abi.HIT_LIGHT
GRIDS = {"1x1x1": (1, 1, 1), "2x1x1": (2, 1, 1), "3x2x2": (3, 2, 2)}


def cells(lo, hi, counts):
    """the abi.PROBE_GRID of `counts` cells over the box lo .. hi"""
    g = np.zeros(1, dtype=abi.PROBE_GRID)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    g["origin"], g["step"], g["counts"] = lo, (hi - lo) / np.asarray(counts, np.float64), counts
    return g[0]


def spread(n, rng, lo=-3.0, hi=3.0):
    """n weighable records of all three kinds, seeded, their places spread over -10 .. 10 and their powers over 10^lo .. 10^hi"""
    e = table(n, rng, lo, hi)
    e["kind"] = np.array([SPH, TRI, LGT], u32)[rng.integers(0, 3, n)]
    e["a"] = rng.uniform(-10, 10, (n, 3))
    e["b"] = rng.uniform(0.1, 1.5, (n, 3))
    e["c"] = np.where((e["kind"] == TRI)[:, None], rng.uniform(-1.5, 1.5, (n, 3)), 0)
    return e


# ---- 1. the bounds
@pytest.mark.parametrize("name", ["feature", "cornell"])
def test_bounds_hold_the_record_within_a_few_ulp(name):
    s = scenes.feature_scene() if name == "feature" else scenes.cornell(32, 32, 1, 4)
    e = direct.scene_emitters(s)
    assert len(e) > 0
    ce, re = direct.emitter_bounds(e)
    assert ce.dtype == f32 and re.dtype == f32 and ce.shape == (len(e), 3) and re.shape == (len(e),)
    a, b, c = (e[k].astype(np.float64) for k in "abc")
    tri = e["kind"] == TRI
    want_ce = np.where(tri[:, None], a + (b + c) / 3.0, a)
    corners = np.stack([a, a + b, a + c], axis=1)
    want_re = np.where(tri, np.sqrt(((corners - want_ce[:, None, :]) ** 2).sum(2)).max(1), np.abs(b[:, 0]))
    scale = np.abs(corners).max((1, 2)) + want_re
    assert (np.abs(ce - want_ce).max(1) <= 4 * np.spacing(scale.astype(f32))).all()
    assert (np.abs(re - want_re) <= 8 * np.spacing(scale.astype(f32))).all()
    # a sphere's bound is the sphere, bit for bit
    assert np.array_equal(_u32(ce[~tri]), _u32(e["a"][~tri])) and np.array_equal(_u32(re[~tri]), _u32(np.abs(e["b"][~tri, 0])))


# ---- 2. the quantised rows
@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 257])
def test_quantised_rows(n, grid):
    rng = np.random.default_rng(1000 + n)
    e = spread(n, rng)
    dead = rng.random(n) < 0.15
    dead[n // 2] = False
    e["area"][dead] = 0
    g = cells((-8, -8, -8), (8, 8, 8), GRIDS[grid])
    rows = int(np.prod(GRIDS[grid]))
    tabs = direct.emitter_grid_cdf(e, g)
    assert tabs.dtype == u32 and tabs.shape == (rows * n,)
    w = direct.grid_weights(e, g)
    assert w.dtype == f32 and w.shape == (rows, n) and not np.isnan(w).any() and (w >= 0).all() and (w <= FLT_MAX).all()
    S = direct.cdf_scale(n)
    for r, row in enumerate(tabs.reshape(rows, n)):
        q = steps(row)
        assert int(row[-1]) <= TOP and (q >= 0).all()                       # Q_r <= 2^24; non-decreasing
        assert (q[~dead] >= 1).all() and (q[dead] == 0).all() and (q <= S).all()   # q >= 1 exactly on the weighable records
        assert q[np.argmax(w[r])] == S                                       # the largest weight sits at S
        ratio = w[r].astype(np.float64) / float(w[r].max()) * S
        big = q > 1
        assert (np.abs(q[big] - ratio[big]) <= 1.0 + ratio[big] * 2.0 ** -22).all()
    # the weight is the power over the squared distance to the cell, no nearer than the radii together (float64, a few ulp)
    p = direct.emitter_weights(e).astype(np.float64)
    ce, re = direct.emitter_bounds(e)
    cc = direct.grid_centres(g).astype(np.float64)
    hd = 0.5 * np.sqrt((g["step"].astype(np.float64) ** 2).sum())
    d2 = ((ce.astype(np.float64)[None] - cc[:, None]) ** 2).sum(2)
    want = p[None] / np.maximum(d2, (re.astype(np.float64) + hd)[None] ** 2)
    assert np.allclose(w, want, rtol=1e-5, atol=0)
    # rows differ where the cells do: the grid matters
    if rows > 1 and n > 2:
        assert not np.array_equal(tabs[:n], tabs[-n:])


def test_cell_centres_and_row_order():
    g = cells((0, 10, 100), (3, 12, 102), (3, 2, 2))
    cc = direct.grid_centres(g)
    assert cc.shape == (12, 3)
    want = [(ix + 0.5, 10.5 + iy, 100.5 + iz) for iz in range(2) for iy in range(2) for ix in range(3)]   # row = (iz ny + iy) nx + ix
    assert np.array_equal(cc, f32(want))


# ---- 3. the weight at its edges
def one_sphere(a, power=6.0, radius=1.0):
    e = table(1)
    e["a"], e["b"] = a, (radius, 0, 0)
    e["area"], e["emissive"] = power / 3.0, (3, 1, 2)
    return e


def test_an_emitter_on_a_cell_centre():
    g = cells((0, 0, 0), (2, 2, 2), (1, 1, 1))
    e = np.concatenate([one_sphere((1, 1, 1)), one_sphere((1, 1, 5))])
    w = direct.grid_weights(e, g)[0]
    hd = np.sqrt(f32(0.25) * f32(12.0))
    assert w[0] == f32(6.0) / ((f32(1.0) + hd) * (f32(1.0) + hd))   # d2 = 0: the floor decides
    assert w[1] == f32(6.0) / f32(16.0)                               # d2 = 16 above the floor (1 + sqrt 3)^2 = 7.46
    assert list(steps(direct.emitter_grid_cdf(e, g))) == [TOP >> 1, int((w[1] / w[0]) * f32(TOP >> 1))]


def test_a_step_so_small_that_hd_underflows():
    g = cells((0, 0, 0), (1e-30, 1e-30, 1e-30), (1, 1, 1))
    e = np.concatenate([one_sphere((0, 0, 2), radius=0.5), one_sphere((0, 0, 0), radius=0.0)])
    e["area"][1] = 2.0   # a record of radius 0 that is weighable all the same: the area is the table's word, not b.x's
    w = direct.grid_weights(e, g)[0]
    assert w[0] == f32(6.0) / f32(4.0)
    assert w[1] == FLT_MAX          # d2, re and hd are all 0 to single precision: p / 0, clamped
    assert list(steps(direct.emitter_grid_cdf(e, g))) == [1, TOP >> 1]


def test_far_emitters_keep_the_floor_of_one():
    g = cells((0, 0, 0), (2, 2, 2), (2, 1, 1))
    e = np.concatenate([one_sphere((1, 1, 1)), one_sphere((1e30, 0, 0)), one_sphere((0, -3e38, 0))])
    w = direct.grid_weights(e, g)
    assert (w[:, 0] > 0).all() and (w[:, 1:] == 0).all()    # d2 overflows: w = 0 ...
    q = direct.emitter_grid_cdf(e, g).reshape(2, 3)
    assert [list(steps(r)) for r in q] == [[TOP >> 2, 1, 1]] * 2    # ... and q = 1: reachable
    # a row in which every weight underflows: every weighable q is 1, the others 0
    e = np.concatenate([one_sphere((1e30, 0, 0), power=1e-20), one_sphere((0, 1e30, 0), power=1e-20), one_sphere((5, 5, 5))])
    e["area"][2] = 0
    assert (direct.grid_weights(e, g) == 0).all()
    assert [list(r) for r in direct.emitter_grid_cdf(e, g).reshape(2, 3)] == [[1, 2, 2]] * 2
    # a grid so coarse that the floor itself overflows
    big = cells((-3e19, -3e19, -3e19), (3e19, 3e19, 3e19), (1, 1, 1))
    assert list(direct.emitter_grid_cdf(np.concatenate([one_sphere((1, 1, 1)), one_sphere((2, 2, 2))]), big)) == [1, 2]


def test_an_overflowing_power_and_a_table_without_power():
    g = cells((0, 0, 0), (4, 4, 4), (2, 1, 1))
    e = np.concatenate([one_sphere((1, 2, 2)), one_sphere((3, 2, 2)), one_sphere((3, 2, 2))])
    e["emissive"][1], e["area"][1] = (3e38, 1, 1), 10.0
    assert direct.emitter_weights(e)[1] == FLT_MAX
    w = direct.grid_weights(e, g)
    assert np.isfinite(w).all() and (w[:, 1] > 1e36).all()
    q = direct.emitter_grid_cdf(e, g).reshape(2, 3)
    assert [list(steps(r)) for r in q] == [[1, TOP >> 2, 1]] * 2
    e["emissive"] = 0
    assert not direct.emitter_grid_cdf(e, g).any() and not direct.grid_weights(e, g).any()
    surf = hemisphere.surfels([(1.0, 0.0, 1.0)] * 2, [(0, 1, 0)] * 2)
    o, d, tmax, contrib = direct.rays(e, surf, 0, 8, grid=g)
    assert not tmax.any() and not _u32(contrib[:, :3]).any() and not _u32(d).any() and (contrib[:, 3] == 1).all()
    assert len(direct.emitter_grid_cdf(e[:0], g)) == 0
    with pytest.raises(ValueError):
        direct.emitter_grid_cdf(np.zeros(3, abi.EMITTER), cells((0, 0, 0), (1, 1, 1), (1 << 10, 1 << 10, 1 << 5)))   # the entry cap


def edge_cases():
    """name -> (table, grid) of the edge cases above and a few beside them, for the device to be held to as well"""
    unit, two = cells((0, 0, 0), (2, 2, 2), (1, 1, 1)), cells((0, 0, 0), (2, 2, 2), (2, 1, 1))
    tiny = one_sphere((0, 0, 0), radius=0.0)
    tiny["area"] = 2.0
    dark = np.concatenate([one_sphere((1e30, 0, 0), power=1e-20), one_sphere((0, 1e30, 0), power=1e-20), one_sphere((5, 5, 5))])
    dark["area"][2] = 0
    hot = np.concatenate([one_sphere((1, 2, 2)), one_sphere((3, 2, 2)), one_sphere((3, 2, 2))])
    hot["emissive"][1], hot["area"][1] = (3e38, 1, 1), 10.0
    none = hot.copy()
    none["emissive"] = 0
    odd = spread(9, np.random.default_rng(9))
    odd["a"][0], odd["b"][1], odd["c"][2] = (np.nan, 0, 0), (np.inf, 0, 0), (0, -np.inf, 0)   # not good: p = 0 whatever the bound is
    odd["a"][3], odd["b"][3], odd["c"][3], odd["kind"][3] = (3e38, 3e38, 3e38), (3e38, 0, 0), (0, 3e38, 0), TRI   # good, its bound overflows
    return {"on a cell centre": (np.concatenate([one_sphere((1, 1, 1)), one_sphere((1, 1, 5))]), unit),
            "hd underflows": (np.concatenate([one_sphere((0, 0, 2), radius=0.5), tiny]), cells((0, 0, 0), (1e-30, 1e-30, 1e-30), (1, 1, 1))),
            "d2 overflows": (np.concatenate([one_sphere((1, 1, 1)), one_sphere((1e30, 0, 0)), one_sphere((0, -3e38, 0))]), two),
            "every w underflows": (dark, two),
            "the floor overflows": (np.concatenate([one_sphere((1, 1, 1)), one_sphere((2, 2, 2))]), cells((-3e19,) * 3, (3e19,) * 3, (1, 1, 1))),
            "an overflowing p": (hot, cells((0, 0, 0), (4, 4, 4), (2, 1, 1))), "no power": (none, two),
            "bad and overflowing bounds": (odd, cells((-8, -8, -8), (8, 8, 8), (3, 2, 2))),
            "cells at the end of the range": (spread(5, np.random.default_rng(2)), cells((3e38, -3e38, 0), (3.3e38, -2.7e38, 1), (2, 2, 1)))}


def test_edge_cases_keep_the_rows_properties():
    for name, (e, g) in edge_cases().items():
        n, p = len(e), direct.emitter_weights(e)
        w = direct.grid_weights(e, g)
        assert not np.isnan(w).any() and (w >= 0).all() and (w <= FLT_MAX).all(), name
        for row in direct.emitter_grid_cdf(e, g).reshape(-1, n):
            q = steps(row)
            assert int(row[-1]) <= TOP and ((q >= 1) == (p > 0)).all() and (q <= direct.cdf_scale(n)).all(), name


# ---- 4. the cell of a position, against exact rational arithmetic
def round_f32(x):
    """the binary32 nearest the Fraction x, ties to even, as a Fraction; +-inf as float"""
    if x == 0:
        return Fraction(0)
    s, x = (-1 if x < 0 else 1), abs(x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    quantum = Fraction(2) ** (max(e, -126) - 23)
    n = x / quantum
    k = n.numerator // n.denominator
    rest = n - k
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and k % 2 == 1):
        k += 1
    r = k * quantum
    return s * float("inf") if r >= Fraction(2) ** 128 else s * r


def exact_axis(pos, origin, step, count):
    d = round_f32(Fraction(float(pos)) - Fraction(float(origin)))
    if isinstance(d, float):
        return count - 1 if d > 0 else 0
    f = round_f32(d / Fraction(float(step)))
    if isinstance(f, float):
        return count - 1 if f > 0 else 0
    return min(max(int(f), 0) if f > 0 else 0, count - 1)


CELL_GRIDS = [((-2.0, 0.0, 1.0), (0.5, 0.25, 2.0), (4, 3, 2)), ((0.3, -0.7, 1e-3), (0.1, 0.3, 1e-4), (7, 1, 5)),
              ((-1e30, 0.0, 3e38), (1e29, 1e-30, 1e37), (5, 2, 3)), ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (1, 1, 1))]


@pytest.mark.parametrize("origin,step,counts", CELL_GRIDS, ids=[str(g[2]) for g in CELL_GRIDS])
def test_cells_against_exact_arithmetic(origin, step, counts):
    g = np.zeros(1, dtype=abi.PROBE_GRID)
    g["origin"], g["step"], g["counts"] = origin, step, counts
    o, s = g["origin"][0], g["step"][0]
    rng = np.random.default_rng(5)
    per_axis = []
    for a in range(3):
        with np.errstate(over="ignore"):
            faces = [f32(o[a] + f32(k) * s[a]) for k in range(counts[a] + 2)]   # on the faces, the last and one past it included
            near = [np.nextafter(v, f32(d)) for v in faces for d in (-np.inf, np.inf)]
            outside = [f32(o[a] - s[a]), f32(o[a] - f32(1e6) * s[a]), f32(o[a] + f32(counts[a] + 1) * s[a]), f32(-3e38), f32(3e38), f32(0.0), f32(-0.0)]
            inside = list((o[a] + rng.uniform(0, counts[a], 20).astype(f32) * s[a]).astype(f32))
            per_axis.append(np.array([v for v in faces + near + outside + inside if np.isfinite(v)], f32))
    m = max(len(v) for v in per_axis)
    pos = np.stack([np.resize(v, m) for v in per_axis], axis=1)
    pos = np.concatenate([pos, np.stack([np.roll(np.resize(v, m), k) for k, v in enumerate(per_axis)], axis=1)])
    row = direct.grid_cell(pos, g[0])
    want = [[exact_axis(p[a], o[a], s[a], counts[a]) for a in range(3)] for p in pos]
    want_row = [(iz * counts[1] + iy) * counts[0] + ix for ix, iy, iz in want]
    assert np.array_equal(row, want_row)
    assert ((row >= 0) & (row < int(np.prod(counts)))).all()
    if counts[0] > 1:
        assert len(set(row)) > 1


def test_a_point_outside_takes_the_nearest_cell():
    g = cells((0, 0, 0), (3, 2, 2), (3, 2, 2))
    pos = f32([(-5, -5, -5), (9, 9, 9), (1.5, -1, 9), (-3e38, 3e38, 0.5), (3.0, 2.0, 2.0), (1.0, 1.0, 1.0), (0.999, 0.999, 0.999)])
    assert list(direct.grid_cell(pos, g)) == [0, 11, 7, 3, 11, 10, 0]


# ---- 5. the two identities
def test_equal_rows_are_section_23s_pick_bit_for_bit():
    e, surf = feature_surfels()
    T = direct.emitter_cdf(e)
    own = np.cumsum([3, 0, 7, 1, 0], dtype=np.uint64).astype(u32)
    for name, counts in GRIDS.items():
        g = cells((-2, -2, -3), (1, 0, 0), counts)   # the surfels fall into several cells
        rows = int(np.prod(counts))
        assert rows == 1 or len(set(direct.grid_cell(surf["pos"], g))) > 1
        for tab in (T, own):
            assert same_bits(direct.rays(e, surf, 5, 64, grid=g, tables=np.tile(tab, rows)), direct.rays(e, surf, 5, 64, cdf=tab)), name
        # ... so rows of j + 1 are the uniform pick
        ramp = np.arange(1, len(e) + 1, dtype=u32)
        ids = np.arange(100, 108, dtype=u32)
        kw = dict(seeds=ids, offset=0.0, shorten=0.25)
        assert same_bits(direct.rays(e, surf, 0, 64, grid=g, tables=np.tile(ramp, rows), **kw), direct.rays(e, surf, 0, 64, **kw)), name
    # the 1 x 1 x 1 grid's own table searches one row: its result is section 23's with that row
    g = cells((-2, -2, -3), (1, 0, 0), (1, 1, 1))
    assert same_bits(direct.rays(e, surf, 0, 64, grid=g), direct.rays(e, surf, 0, 64, cdf=direct.emitter_grid_cdf(e, g)))


def test_every_item_searches_its_own_row_and_invalid_surfels_pick_nothing():
    e, surf = feature_surfels()
    g = cells((-2, -2, -3), (1, 0, 0), (3, 2, 2))
    tabs = direct.emitter_grid_cdf(e, g)
    surf = np.concatenate([surf, surf[:3]])
    surf["pos"][-3] = (np.nan, 0, 0)
    surf["normal"][-2] = (0, 0, 0)
    surf["pos"][-1] = (np.inf, 0, 0)
    got = direct.rays(e, surf, 3, 16, grid=g, tables=tabs)
    row = direct.grid_cell(surf["pos"][:-3], g)
    for i in range(len(surf) - 3):
        want = direct.rays(e, surf[i:i + 1], 3, 16, seeds=[i], cdf=tabs.reshape(12, -1)[row[i]])
        assert same_bits([x[i * 16:(i + 1) * 16] for x in got], want), i
    tail = slice((len(surf) - 3) * 16, None)
    assert not got[2][tail].any() and not _u32(got[3][tail]).any() and not _u32(got[1][tail]).any()
    assert np.array_equal(_u32(got[0][tail]), _u32(np.repeat(surf["pos"][-3:], 16, axis=0)))


# ---- 6. malformed rows
@pytest.mark.parametrize("name,cdf", [g for g in GARBAGE if len(g[1]) == 5], ids=[g[0] for g in GARBAGE if len(g[1]) == 5])
def test_malformed_rows_stay_in_range_and_are_dark_where_the_definition_says(name, cdf):
    e, surf = feature_surfels()
    g = cells((-2, -2, -3), (1, 0, 0), (2, 1, 1))
    good = direct.emitter_cdf(e)
    row = direct.grid_cell(surf["pos"], g)
    assert set(row) == {0, 1}
    for bad_row in (0, 1):
        tabs = np.concatenate([good, good]).astype(u32)
        tabs[bad_row * 5:bad_row * 5 + 5] = cdf
        got = direct.rays(e, surf, 0, 32, grid=g, tables=tabs)   # search_cdf raises if an index leaves its row
        assert np.isfinite(got[3]).all() and (got[3][:, 3] == 1).all()
        for i in range(len(surf)):
            sl = slice(i * 32, (i + 1) * 32)
            want = direct.rays(e, surf[i:i + 1], 0, 32, seeds=[i], cdf=tabs[row[i] * 5:row[i] * 5 + 5])
            assert same_bits([x[sl] for x in got], want), (name, i)
            Q = int(np.array(cdf, u32)[-1])
            if row[i] == bad_row and (Q == 0 or Q > TOP):
                assert not got[2][sl].any() and not _u32(got[3][sl, :3]).any() and not _u32(got[1][sl]).any()
    u0 = direct.draws(4, 0, 64)["u0"]
    j, q, Q = direct.pick_grid(u0, np.repeat([0, 1, -1, 1], 64), np.concatenate([np.array(cdf, u32), good]), 5)
    assert ((j >= 0) & (j < 5)).all() and (q[128:192] == 0).all()
    if 0 < int(np.array(cdf, u32)[-1]) <= TOP:
        t = np.minimum((u0[:64] * f32(Q[0])).astype(f32).astype(u32), u32(Q[0] - 1))
        assert np.array_equal(j[:64], [scalar_search(int(x), np.array(cdf, u32)) for x in t])


# ---- 7. the factor
def test_the_grid_pick_estimates_the_sum_over_every_emitter_with_less_noise_than_power():
    """spheres_scene(n=20000): 197 emitters, 12 seeded ground points, an 8 x 1 x 8 grid over the emitters' and the points' box,
    unoccluded contributions.  One side is the grid pick at 131072 samples per point; the other has no pick at all: every
    emitter alone (a table of one record, factor 1), summed, at 4096 samples per point.  The pooled means are at most 5
    combined standard errors apart and that error is below 3 % of the mean (section 21.5's two numbers); the pooled variance
    of the grid pick is below the pick by power's on the same points; a factor float(N) kept in place of float(Q) / float(q)
    -- the mutant -- misses the reference by more than 5 standard errors.
    Measured with this model: grid 0.04500 +- 0.00015 against 0.04473 +- 0.00021, 1.05 standard errors apart, a combined
    error of 0.57 % of the mean (the reference alone 0.46 %); pooled variance power / grid 6.87; the mutant 776 % off."""
    s = scenes.spheres_scene(n=20000)
    e = direct.scene_emitters(s)
    N = len(e)
    assert N == 197
    rng = np.random.default_rng(24)
    ce, re = direct.emitter_bounds(e)
    lo, hi = (ce - re[:, None]).min(0), (ce + re[:, None]).max(0)
    pts = np.stack([rng.uniform(lo[0], hi[0], 12), np.zeros(12), rng.uniform(lo[2], hi[2], 12)], axis=1).astype(f32)
    surf = hemisphere.surfels(pts, np.tile(f32([0, 1, 0]), (12, 1)))
    g = cells(np.minimum(lo, pts.min(0)), np.maximum(hi, pts.max(0)), (8, 1, 8))
    tabs = direct.emitter_grid_cdf(e, g)
    SG, SR, SP = 131072, 4096, 32768
    grid = direct.rays(e, surf, 0, SG, grid=g, tables=tabs)[3]
    assert (grid[:, 3] == 1).all()
    gv = grid[:, :3].astype(np.float64).mean(1)
    ref = np.zeros(12 * SR)
    for j in range(N):
        ref += direct.rays(e[j:j + 1], surf, 0, SR)[3][:, :3].astype(np.float64).mean(1)
    pw = direct.rays(e, surf, 0, SP, cdf=direct.emitter_cdf(e))[3][:, :3].astype(np.float64).mean(1)
    mg, mr = gv.mean(), ref.mean()
    seg, ser = gv.std(ddof=1) / np.sqrt(len(gv)), ref.std(ddof=1) / np.sqrt(len(ref))
    se = np.hypot(seg, ser)
    pooled = 0.5 * (mg + mr)
    print(f"grid {mg:.5f} +- {seg:.5f}, every emitter alone {mr:.5f} +- {ser:.5f}: {abs(mg - mr) / se:.2f} combined standard errors, "
          f"{100 * se / pooled:.2f} % of the mean (the reference alone {100 * ser / mr:.2f} %)")
    print(f"pooled variance: power {pw.var(ddof=1):.4g}, grid {gv.var(ddof=1):.4g}, power / grid {pw.var(ddof=1) / gv.var(ddof=1):.2f}; "
          f"power's mean {pw.mean():.5f}")
    assert mg > 0 and mr > 0
    assert se < 0.03 * pooled, (se, pooled)
    assert abs(mg - mr) <= 5.0 * se, (mg, mr, se)
    assert gv.var(ddof=1) < pw.var(ddof=1)
    # the mutant: the grid pick's records with the uniform pick's factor
    row = np.repeat(direct.grid_cell(surf["pos"], g), SG)
    j, q, Q = direct.pick_grid(direct.draws(12, 0, SG)["u0"], row, tabs, N)
    mutant = gv * (N / (Q.astype(np.float64) / q.astype(np.float64)))
    sem = np.hypot(mutant.std(ddof=1) / np.sqrt(len(mutant)), ser)
    print(f"mutant (factor N): {mutant.mean():.5f}, {100 * (mutant.mean() / mr - 1):.0f} % off, {abs(mutant.mean() - mr) / sem:.1f} standard errors")
    assert abs(mutant.mean() - mr) > 5.0 * sem
