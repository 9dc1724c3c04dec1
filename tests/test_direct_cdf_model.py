"""The numpy model of the weighted pick (renderbaby_amd/direct.py: emitter_weights, emitter_cdf, search_cdf, pick_cdf,
rays(cdf=...)) held to its definition: the quantised table and what is weighable, the search on good and
on malformed tables, the two identities that tie the weighted pick to the uniform one bit for bit, and the factor float(Q) /
float(q) as the estimator sees it -- the same integral by both picks, with less noise by power where the powers differ."""
import numpy as np
import pytest

from renderbaby_amd import abi, direct, hemisphere, scenes
from tests.test_direct_model import M32, _u32, seeds_drawing

f32, u32 = np.float32, np.uint32
TRI, SPH, LGT = abi.HIT_TRIANGLE, abi.HIT_SPHERE, abi.HIT_LIGHT
FLT_MAX = f32(3.4028235e38)
TOP = 1 << 24


def table(n, rng=None, lo=-30.0, hi=38.0):
    """n sphere records whose powers m area span 10^lo .. 10^hi (seeded), the exponent split between emission and area"""
    e = np.zeros(n, dtype=abi.EMITTER)
    e["kind"], e["a"], e["b"] = SPH, (0, 5, 0), (1, 0, 0)
    if rng is None:
        e["area"], e["emissive"] = 2.0, (3, 1, 2)
        return e
    ex = rng.uniform(lo, hi, n)
    part = rng.uniform(0.3, 0.7, n)
    e["area"] = (10.0 ** (ex * part)).astype(f32)
    m = (10.0 ** (ex * (1 - part))).astype(f32)
    e["emissive"] = np.stack([m, m * f32(0.5), np.zeros(n, f32)], axis=1)
    return e


def steps(cdf):
    cdf = np.asarray(cdf, np.int64)
    return np.diff(np.concatenate([[0], cdf]))


# ---- 1. the quantisation
@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 4097, 10 ** 4])
def test_quantised_table(n):
    rng = np.random.default_rng(n)
    e = table(n, rng)
    dead = rng.random(n) < 0.1
    dead[n // 2] = False   # one at least stays
    e["area"][dead] = 0
    p = direct.emitter_weights(e)
    assert p.dtype == f32 and ((p > 0) == ~dead).all() and np.isfinite(p).all()
    # the weight is the product, one rounding (float64 holds the exact product of two floats)
    exact = e["emissive"].max(1).astype(np.float64) * e["area"].astype(np.float64)
    assert np.array_equal(p[~dead], np.minimum(exact[~dead].astype(f32), FLT_MAX))
    cdf = direct.emitter_cdf(e)
    q = steps(cdf)
    S = direct.cdf_scale(n)
    assert cdf.dtype == u32 and len(cdf) == n
    assert S == 1 << (24 - int(np.ceil(np.log2(n)))) and S * n >= TOP // 2 * (n > 1) and S * n <= TOP
    assert int(cdf[-1]) <= TOP and (q >= 0).all()                   # Q <= 2^24; non-decreasing
    assert (q[~dead] >= 1).all() and (q[dead] == 0).all() and (q <= S).all()
    assert q[np.argmax(p)] == S                                     # the largest power has the whole scale
    # the quantised weight is the floor of the scaled ratio: within one of it, except under the floor of 1
    ratio = p.astype(np.float64) / float(p.max()) * S
    big = q > 1
    assert (np.abs(q[big] - ratio[big]) <= 1.0 + ratio[big] * 2.0 ** -22).all()
    assert (ratio[(q == 1) & ~dead] < 2.0 + 2.0 ** -20).all()


def test_scale_of_every_size():
    assert [direct.cdf_scale(n) for n in (1, 2, 3, 4, 5, 64, 65, 4096, 4097, TOP - 1, TOP)] == \
        [TOP, TOP >> 1, TOP >> 2, TOP >> 2, TOP >> 3, TOP >> 6, TOP >> 7, TOP >> 12, TOP >> 13, 1, 1]
    with pytest.raises(ValueError):
        direct.emitter_cdf(np.zeros(TOP + 1, dtype=abi.EMITTER))
    assert len(direct.emitter_cdf(np.zeros(0, dtype=abi.EMITTER))) == 0


def test_an_overflowing_power_is_clamped_not_dropped():
    e = table(3)
    e["emissive"][1] = (3e38, 1, 1)
    e["area"][1] = 10.0
    p = direct.emitter_weights(e)
    assert p[1] == FLT_MAX and p[0] == 6.0 and p[2] == 6.0
    q = steps(direct.emitter_cdf(e))
    assert list(q) == [1, TOP >> 2, 1]   # the dim ones keep the floor of 1: reachable at any dynamic range
    # two that overflow share the top
    e["emissive"][2], e["area"][2] = (1e30, 0, 0), 1e30
    assert list(steps(direct.emitter_cdf(e))) == [1, TOP >> 2, TOP >> 2]


def test_a_power_that_underflows_to_zero_is_not_weighable():
    e = table(2)
    e["emissive"][0], e["area"][0] = (1e-30, 0, 0), 1e-30
    assert list(direct.emitter_weights(e)) == [0.0, 6.0]
    assert list(direct.emitter_cdf(e)) == [0, TOP >> 1]


def test_no_power_at_all_gives_zeros():
    e = table(5)
    e["emissive"] = 0
    assert (direct.emitter_weights(e) == 0).all() and (direct.emitter_cdf(e) == 0).all()
    j, q, Q = direct.pick_cdf(f32([0.0, 0.5, 1.0]), direct.emitter_cdf(e))
    assert Q == 0 and (q == 0).all()


NOT_WEIGHABLE = [("area", v) for v in (np.nan, np.inf, -np.inf, -1.0, 0.0, -0.0)] + [("kind", v) for v in (0, 1, 5, 0xFFFFFFFF)] + \
    [("emissive", v) for v in ((0, 0, 0), (-1, -2, -3), (0, -1, 0), (np.nan, 1, 1), (1, np.inf, 1), (1, 1, -np.inf), (-0.0, -0.0, -0.0))] + \
    [(f, v) for f in "abc" for v in ((np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf))]


@pytest.mark.parametrize("field,value", NOT_WEIGHABLE, ids=[f"{f}={v}" for f, v in NOT_WEIGHABLE])
def test_not_weighable_one_field_at_a_time(field, value):
    e = table(3)
    assert (direct.emitter_weights(e) == 6.0).all()
    e[field][1] = value
    assert list(direct.emitter_weights(e)) == [6.0, 0.0, 6.0]
    assert list(steps(direct.emitter_cdf(e))) == [TOP >> 2, 0, TOP >> 2]


def test_weighable_at_the_edges():
    e = table(4)
    e["emissive"][0] = (-5, 1e-45, -1)      # the largest component decides, a denormal included ...
    e["area"][0] = 1e10                      # ... as long as the product stays above 0
    e["kind"] = (SPH, TRI, LGT, SPH)
    p = direct.emitter_weights(e)
    assert (p > 0).all() and p[0] == f32(1e-45) * f32(1e10)


# ---- 2. the search
def scalar_search(t, cdf):
    """section 23.1's loop on Python integers; every index is checked"""
    lo, ln, reads = 0, len(cdf), 0
    while ln > 1:
        half = ln >> 1
        assert 0 <= lo + half - 1 < len(cdf)
        reads += 1
        if int(cdf[lo + half - 1]) <= t:
            lo, ln = lo + half, ln - half
        else:
            ln = half
    assert 0 <= lo < len(cdf) and reads <= 24
    return lo


SMALL = [[1], [7], [1, 2], [0, 3], [3, 3], [1, 2, 3], [0, 0, 4], [2, 2, 2, 5], [0, 1, 1, 1, 6], [4, 4, 9, 9, 9, 9, 11], [0, 0, 0, 0, 0, 0, 0, 1],
         list(np.cumsum(np.random.default_rng(3).integers(0, 4, 37)) + 1)]


@pytest.mark.parametrize("cdf", SMALL, ids=[f"N={len(c)}" + ("" if i < 11 else " seeded") for i, c in enumerate(SMALL)])
def test_search_lands_on_the_first_entry_above_t(cdf):
    cdf = np.array(cdf, u32)
    Q = int(cdf[-1])
    t = np.arange(Q, dtype=u32)
    j = direct.search_cdf(t, cdf)
    want = np.searchsorted(cdf, t, side="right")
    assert np.array_equal(j, want) and np.array_equal(j, [scalar_search(int(x), cdf) for x in t])
    assert (steps(cdf)[j] > 0).all()   # a zero step is never picked
    # through the draw: u0 = (t + 1/2) / Q picks t's record, with its step and the total
    u0 = ((t.astype(np.float64) + 0.5) / Q).astype(f32)
    jj, q, QQ = direct.pick_cdf(u0, cdf)
    assert QQ == Q and np.array_equal(jj, want) and np.array_equal(q, steps(cdf)[want])


def test_search_on_a_long_table():
    rng = np.random.default_rng(11)
    for n in (4097, 10 ** 4):
        e = table(n, rng, -3.0, 3.0)
        e["area"][rng.random(n) < 0.2] = 0
        cdf = direct.emitter_cdf(e)
        t = np.concatenate([rng.integers(0, int(cdf[-1]), 2000), [0, int(cdf[-1]) - 1]]).astype(u32)
        j = direct.search_cdf(t, cdf)
        assert np.array_equal(j, np.searchsorted(cdf, t, side="right"))
        assert (direct.emitter_weights(e)[j] > 0).all()


def test_u0_of_exactly_one_picks_the_last_weighable_record():
    e = direct.scene_emitters(scenes.feature_scene())
    e = np.concatenate([e, e[:2]])
    e["area"][-2:] = 0   # the table ends in two records without weight
    cdf = direct.emitter_cdf(e)
    ids = np.array([seeds_drawing(w, 7, 0) for w in (M32, M32 - 127, M32 - 128)], u32)
    dr = direct.draws(3, 7, 1, seeds=ids)
    assert dr["u0"][0] == 1.0 and dr["u0"][1] == 1.0 and dr["u0"][2] < 1.0
    j, q, Q = direct.pick_cdf(dr["u0"], cdf)
    last = len(e) - 3
    assert list(j) == [last] * 3 and Q == int(cdf[-1]) and (q == steps(cdf)[last]).all() and q[0] > 0
    # t = min(uint(u0 Q), Q - 1) is Q - 1 for all three
    assert (f32(dr["u0"][2]) * f32(Q)).astype(u32) >= Q - 1
    surf = hemisphere.surfels([(0.0, 0.0, 0.0)] * 3, [(0, 1, 0)] * 3)
    o, d, tmax, contrib = direct.rays(e, surf, 7, 1, seeds=ids, cdf=cdf)
    want = direct.rays(e[last:last + 1], surf, 7, 1, seeds=ids)
    assert np.array_equal(_u32(d), _u32(want[1])) and np.array_equal(_u32(tmax), _u32(want[2])) and (tmax > 0).any()
    w = f32(Q) / f32(q[0])
    assert np.allclose(contrib[:, :3], want[3][:, :3] * w, rtol=1e-6)


GARBAGE = [("decreasing", [9, 7, 5, 3, 1]), ("decreasing to 0", [4, 3, 2, 1, 0]), ("all equal", [6, 6, 6, 6, 6]), ("all zero", [0, 0, 0, 0, 0]),
           ("total above 2^24", [1, 2, 3, 4, TOP + 1]), ("total far above", [5, 5, 5, 5, M32]), ("a dip", [3, 1, 8, 2, 9]),
           ("wrapping step", [M32, M32, 1, 2, 3]), ("one entry of 0", [0]), ("one entry above", [TOP + 1]), ("two, decreasing", [8, 2])]


@pytest.mark.parametrize("name,cdf", GARBAGE, ids=[g[0] for g in GARBAGE])
def test_malformed_tables_stay_in_range_and_are_dark_where_the_definition_says(name, cdf):
    cdf = np.array(cdf, u32)
    n = len(cdf)
    e = direct.scene_emitters(scenes.feature_scene())[:n]
    assert len(e) == n
    pts = np.array([(-1.5, -1, -2), (0.5, -1, -1), (0.5, -1, 0)], f32)
    surf = hemisphere.surfels(pts, np.tile(f32([0, 1, 0]), (3, 1)))
    dr = direct.draws(3, 0, 64)
    j, q, Q = direct.pick_cdf(dr["u0"], cdf)   # search_cdf raises if an index leaves the table
    assert ((j >= 0) & (j < n)).all() and Q == int(cdf[-1])
    o, d, tmax, contrib = direct.rays(e, surf, 0, 64, cdf=cdf)
    assert np.isfinite(contrib).all() and (contrib[:, 3] == 1).all()   # dark or not, an item of a valid surfel is valid
    if Q == 0 or Q > TOP:
        assert (q == 0).all() and (j == 0).all()
        assert (tmax == 0).all() and (_u32(contrib[:, :3]) == 0).all() and (_u32(d) == 0).all()
        return
    t = np.minimum((dr["u0"] * f32(Q)).astype(f32).astype(u32), u32(Q - 1))
    assert np.array_equal(j, [scalar_search(int(x), cdf) for x in t])
    step = (cdf[j].astype(np.int64) - np.where(j > 0, cdf[np.maximum(j - 1, 0)], 0).astype(np.int64)) & M32
    assert np.array_equal(q, step)
    dark = q == 0
    assert (tmax[dark] == 0).all() and (_u32(contrib[dark, :3]) == 0).all() and (_u32(d[dark]) == 0).all()
    # the others are the items of their records with the factor float(Q) / float(q), whatever that is
    for k in np.nonzero(~dark)[0][:16]:
        one = direct.rays(e[j[k]:j[k] + 1], surf[k // 64:k // 64 + 1], k % 64, 1, seeds=[k // 64])
        assert np.array_equal(_u32(d[k]), _u32(one[1][0]))
        if one[2][0] > 0 and tmax[k] > 0:
            w = f32(Q) / f32(q[k])
            assert np.allclose(contrib[k, :3], one[3][0, :3] * w, rtol=1e-6)


# ---- 3. the two identities
def feature_surfels():
    s = scenes.feature_scene()
    e = direct.scene_emitters(s)
    pts = np.array([(x, -1.0, z) for x in (-1.5, 0.5) for z in (-3.0, -2.0, -1.0, 0.0)], f32)
    return e, hemisphere.surfels(pts, np.tile(f32([0, 1, 0]), (len(pts), 1)))


def same_bits(got, want):
    return all(np.array_equal(_u32(g), _u32(w)) for g, w in zip(got, want))


def test_the_ramp_is_the_uniform_pick_bit_for_bit():
    e, surf = feature_surfels()
    for n in (len(e), 3, 1):
        ramp = np.arange(1, n + 1, dtype=u32)
        assert same_bits(direct.rays(e[:n], surf, 5, 256, cdf=ramp), direct.rays(e[:n], surf, 5, 256))
    ids = np.arange(100, 108, dtype=u32)
    assert same_bits(direct.rays(e, surf, 0, 64, seeds=ids, offset=0.0, shorten=0.25, cdf=np.arange(1, len(e) + 1, dtype=u32)),
                     direct.rays(e, surf, 0, 64, seeds=ids, offset=0.0, shorten=0.25))


def test_equal_powers_are_the_uniform_pick_bit_for_bit():
    e, surf = feature_surfels()
    assert len(e) == 5
    e = e.copy()
    e["area"], e["emissive"] = 2.0, (3, 1, 2)      # five records of one power where they are
    cdf = direct.emitter_cdf(e)
    assert list(steps(cdf)) == [TOP >> 3] * 5       # q = S, a power of two: w = N exactly
    assert same_bits(direct.rays(e, surf, 5, 256, cdf=cdf), direct.rays(e, surf, 5, 256))
    for n in (3, 4, 1):
        assert same_bits(direct.rays(e[:n], surf, 0, 64, cdf=direct.emitter_cdf(e[:n])), direct.rays(e[:n], surf, 0, 64))
    # ... and the draws that sit on an edge of the uniform pick: u0 N a whole number, and u0 == 1
    ids = np.array([seeds_drawing(w, 0, 0) for w in (M32, M32 - 128, 0, 0x33333333, 0x33333400, 0x66666600, 0x99999980, 0xCCCCCC00, 0xCCCCCD00)], u32)
    one = hemisphere.surfels([(0.5, -1.0, -1.0)] * len(ids), [(0, 1, 0)] * len(ids))
    assert same_bits(direct.rays(e, one, 0, 1, seeds=ids, cdf=cdf), direct.rays(e, one, 0, 1, seeds=ids))


# ---- 4. the factor
def test_both_picks_estimate_the_same_integral_and_power_with_less_noise():
    """Unoccluded contributions of 8 floor points of the feature scene, 4096 samples each, its table's powers 75, 75, 226, 188
    and 94: the pooled means differ by at most 5 combined standard errors, that error is below 3 % of the mean (section
    21.5's two numbers), and the pooled variance by power is below the uniform pick's.  A factor float(N) kept in place of
    float(Q) / float(q) -- the mutant -- misses by far more."""
    e, surf = feature_surfels()
    power = direct.emitter_weights(e)
    print("powers", power)
    assert power.min() > 50 and power.max() / power.min() > 2.5
    cdf = direct.emitter_cdf(e)
    S = 4096
    uni = direct.rays(e, surf, 0, S)[3]
    pw = direct.rays(e, surf, 0, S, cdf=cdf)[3]
    assert (uni[:, 3] == 1).all() and (pw[:, 3] == 1).all()
    u = uni[:, :3].astype(np.float64).mean(1)
    p = pw[:, :3].astype(np.float64).mean(1)
    mu, mp = u.mean(), p.mean()
    seu, sep = u.std(ddof=1) / np.sqrt(len(u)), p.std(ddof=1) / np.sqrt(len(p))
    se = np.hypot(seu, sep)
    pooled = 0.5 * (mu + mp)
    per_u, per_p = u.reshape(8, S), p.reshape(8, S)
    print(f"uniform {mu:.5f} +- {seu:.5f}, power {mp:.5f} +- {sep:.5f}: {abs(mu - mp) / se:.2f} combined standard errors, {100 * se / pooled:.2f} % of the mean")
    print("per point, relative deviation per sample: uniform", np.round(per_u.std(1) / per_u.mean(1), 2), "power", np.round(per_p.std(1) / per_p.mean(1), 2))
    print("per point, means power / uniform", np.round(per_p.mean(1) / per_u.mean(1), 3), "; pooled variance uniform / power", u.var() / p.var())
    assert mu > 0 and mp > 0
    assert se < 0.03 * pooled, (se, pooled)
    assert abs(mu - mp) <= 5.0 * se, (mu, mp, se)
    assert p.var(ddof=1) < u.var(ddof=1)
    # the mutant: the power pick's records with the uniform pick's factor
    j, q, Q = direct.pick_cdf(direct.draws(8, 0, S)["u0"], cdf)
    mutant = p * (len(e) / (float(Q) / q.astype(np.float64)))
    print(f"mutant (factor N): {mutant.mean():.5f}, {100 * (mutant.mean() / mu - 1):.0f} % off")
    assert abs(mutant.mean() - mu) > 5.0 * se and abs(mutant.mean() / mu - 1) > 0.1
