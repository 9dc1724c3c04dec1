"""The numpy model of the per-cell tables that learn visibility (renderbaby_amd/direct.py: seen_share, grid_weights(tally=...),
emitter_grid_cdf(tally=...), count, tally) held to its definition: the factor f against exact rational
arithmetic and the rows against float64, the two identities with section 24 bit for bit, the tally at its edges, the count on
hand-made items and against a loop over the items, and the estimator under an analytic occluder -- the same integral as a sum
over every emitter alone, with less noise than section 24's tables, and a factor taken from the wrong row found out."""
from fractions import Fraction

import numpy as np
import pytest

from renderbaby_amd import abi, direct, hemisphere
from tests.test_direct_cdf_model import FLT_MAX, TOP, feature_surfels, steps
from tests.test_direct_grid_model import GRIDS, cells, one_sphere, round_f32, spread

f32, u32 = np.float32, np.uint32
TALLY = abi.GRID_TALLY
BOX = ((-8, -8, -8), (8, 8, 8))
TINY = np.float32(1e-45)   # the smallest binary32 above 0
PRIORS = (TINY, 0.5, 1.0, 3.0, abi.MAX_PRIOR)


def records(tried, seen):
    t = np.zeros(len(np.atleast_1d(tried)), dtype=TALLY)
    t["tried"], t["seen"] = tried, seen
    return t


def random_tally(n, rng):
    """n records of every sort: empty, small, seen above tried, at and near the counters' end"""
    tried = rng.integers(0, 200, n).astype(np.uint64)
    seen = (tried * rng.random(n)).astype(np.uint64)
    kind = rng.integers(0, 8, n)
    tried = np.where(kind == 0, 0, np.where(kind == 1, 2 ** 32 - 1, np.where(kind == 2, rng.integers(1 << 24, 1 << 32, n), tried)))
    seen = np.where(kind == 0, 0, np.where(kind == 3, seen + 500, np.where(kind == 2, tried // 3, seen)))
    return records(tried.astype(u32), np.minimum(seen, 2 ** 32 - 1).astype(u32))


# ---- 1. the factor and the rows
def exact_share(tried, seen, a):
    s, t, a = Fraction(min(int(seen), int(tried))), Fraction(int(tried)), Fraction(float(a))
    return round_f32(round_f32(round_f32(s) + a) / round_f32(round_f32(t) + a))


@pytest.mark.parametrize("prior", PRIORS)
def test_the_factor_against_exact_arithmetic(prior):
    rng = np.random.default_rng(7)
    t = np.concatenate([random_tally(120, rng), records([0, 1, 2, 2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1, 16777217, 5],
                                                        [0, 0, 0, 0, 2 ** 32 - 1, 2 ** 31, 16777217, 2 ** 32 - 1])])
    f = direct.seen_share(t, prior)
    assert f.dtype == f32 and not np.isnan(f).any() and (f >= 0).all() and (f <= 1).all()
    want = [exact_share(r["tried"], r["seen"], f32(prior)) for r in t]
    assert [Fraction(float(x)) for x in f] == want
    if f32(prior) >= f32(2.0) ** -117:
        assert (f > 0).all()   # (below that the quotient can underflow: the floor of 1, not f, keeps an emitter reachable)
    s = np.minimum(t["seen"], t["tried"]).astype(np.float64)
    assert np.allclose(f, (s + float(f32(prior))) / (t["tried"].astype(np.float64) + float(f32(prior))), rtol=3e-7, atol=1e-45)


@pytest.mark.parametrize("bad", [0.0, -1.0, np.nan, np.inf, 3.0e7, -0.0])
def test_a_bad_prior_is_refused(bad):
    with pytest.raises(ValueError, match="prior"):
        direct.seen_share(records([1], [1]), bad)
    with pytest.raises(ValueError, match="prior"):
        direct.emitter_grid_cdf(one_sphere((1, 1, 1)), cells((0, 0, 0), (2, 2, 2), (1, 1, 1)), records([1], [1]), bad)


@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 257])
def test_learned_rows(n, grid):
    rng = np.random.default_rng(2500 + n)
    e = spread(n, rng)
    dead = rng.random(n) < 0.15
    dead[n // 2] = False
    e["area"][dead] = 0
    g = cells(*BOX, GRIDS[grid])
    rows = int(np.prod(GRIDS[grid]))
    t = random_tally(rows * n, rng)
    w0 = direct.grid_weights(e, g)
    S = direct.cdf_scale(n)
    for prior in (0.5, 1.0, abi.MAX_PRIOR):
        w = direct.grid_weights(e, g, t, prior)
        f = direct.seen_share(t, prior).reshape(rows, n)
        assert w.dtype == f32 and w.shape == (rows, n) and not np.isnan(w).any() and (w >= 0).all() and (w <= w0).all()
        assert np.array_equal(w.view(u32), (w0 * f).astype(f32).view(u32))   # one multiply
        s64 = np.minimum(t["seen"], t["tried"]).astype(np.float64).reshape(rows, n)
        f64 = (s64 + prior) / (t["tried"].astype(np.float64).reshape(rows, n) + prior)
        assert np.allclose(w, w0.astype(np.float64) * f64, rtol=1e-6, atol=1e-44)
        tabs = direct.emitter_grid_cdf(e, g, t, prior)
        assert tabs.dtype == u32 and tabs.shape == (rows * n,)
        for r, row in enumerate(tabs.reshape(rows, n)):
            q = steps(row)
            assert int(row[-1]) <= TOP and (q[~dead] >= 1).all() and (q[dead] == 0).all() and (q <= S).all()
            assert q[np.argmax(w[r])] == S
            ratio = w[r].astype(np.float64) / float(w[r].max()) * S
            big = q > 1
            assert (np.abs(q[big] - ratio[big]) <= 1.0 + ratio[big] * 2.0 ** -22).all()
    if n > 3:
        assert not np.array_equal(direct.emitter_grid_cdf(e, g, t, 1.0), direct.emitter_grid_cdf(e, g))   # the tally matters
    with pytest.raises(ValueError):
        direct.emitter_grid_cdf(e, g, t[:-1], 1.0)


# ---- 2. the identities
@pytest.mark.parametrize("grid", list(GRIDS))
def test_an_empty_and_a_saturated_tally_give_section_24s_rows(grid):
    rng = np.random.default_rng(3)
    for n in (1, 3, 65):
        e = spread(n, rng)
        e["area"][n // 3] = 0
        g = cells(*BOX, GRIDS[grid])
        rows = int(np.prod(GRIDS[grid]))
        want = direct.emitter_grid_cdf(e, g)
        tried = rng.integers(0, 1 << 32, rows * n).astype(u32)
        for prior in PRIORS:
            assert np.array_equal(direct.emitter_grid_cdf(e, g, np.zeros(rows * n, TALLY), prior), want), (n, prior)
            assert np.array_equal(direct.emitter_grid_cdf(e, g, records(tried, tried), prior), want), (n, prior)
            above = records(tried, np.maximum(tried, rng.integers(0, 1 << 32, rows * n).astype(u32)))
            assert np.array_equal(direct.emitter_grid_cdf(e, g, above, prior), want), (n, prior)
        assert np.array_equal(direct.grid_weights(e, g, records(tried, tried), 1.0).view(u32), direct.grid_weights(e, g).view(u32))
    assert len(direct.emitter_grid_cdf(e[:0], g, np.zeros(0, TALLY), 1.0)) == 0


# ---- 3. the tally at its edges
def test_edges_of_the_tally():
    g = cells((0, 0, 0), (2, 2, 2), (1, 1, 1))
    e = np.concatenate([one_sphere((1, 1, 1)), one_sphere((1, 1, 1)), one_sphere((1, 1, 1)), one_sphere((1, 1, 1))])
    half = TOP >> 2   # S for four records
    # seen above tried counts as tried; a record never seen keeps the prior's share
    assert list(steps(direct.emitter_grid_cdf(e, g, records([4, 4, 4, 0], [9, 4, 0, 0]), 1.0))) == [half, half, int(f32(0.2) * f32(half)), half]
    # the counters' end: (2^32 - 1) rounds to 2^32 and nothing overflows
    q = steps(direct.emitter_grid_cdf(e, g, records([2 ** 32 - 1] * 4, [2 ** 32 - 1, 2 ** 31, 0, 1]), 1.0))
    assert list(q) == [half, half >> 1, 1, 1]
    # the prior at both ends of its range
    top = steps(direct.emitter_grid_cdf(e, g, records([100, 100, 0, 2 ** 32 - 1], [0, 50, 0, 0]), abi.MAX_PRIOR))
    for k, (s, t) in enumerate(((0, 100), (50, 100), (0, 0), (0, 2 ** 32))):   # the largest prior still learns, slowly
        assert abs(int(top[k]) - (s + 2.0 ** 24) / (t + 2.0 ** 24) * half) <= 1, k
    assert top[2] == half and top[0] < top[1] < half and top[3] < half >> 7
    low = steps(direct.emitter_grid_cdf(e, g, records([1, 2, 0, 7], [0, 0, 0, 7]), TINY))
    assert list(low) == [1, 1, half, half]   # f = 1e-45 and, for tried = 2, an f that underflows to 0: the floor holds both
    assert direct.seen_share(records([2], [0]), TINY)[0] == 0 and direct.seen_share(records([1], [0]), TINY)[0] == TINY


def test_a_row_whose_every_weight_underflows_and_records_without_power():
    g = cells((0, 0, 0), (2, 2, 2), (2, 1, 1))
    e = np.concatenate([one_sphere((1, 1, 1), power=1e-37), one_sphere((1, 1, 1), power=1e-37), one_sphere((5, 5, 5))])
    e["area"][2] = 0
    t = records([2 ** 32 - 1] * 6, [0] * 6)
    assert (direct.grid_weights(e, g) > 0)[:, :2].all() and (direct.grid_weights(e, g, t, TINY) == 0).all()
    assert [list(r) for r in direct.emitter_grid_cdf(e, g, t, TINY).reshape(2, 3)] == [[1, 2, 2]] * 2


def test_every_record_with_power_stays_reachable_whatever_the_tally():
    rng = np.random.default_rng(11)
    for n, counts in ((5, (2, 1, 1)), (64, (3, 2, 2)), (257, (1, 1, 1))):
        e = spread(n, rng)
        e["area"][::7] = (0.0, np.nan, -1.0, np.inf)[n % 4]
        p = direct.emitter_weights(e)
        g = cells(*BOX, counts)
        rows = int(np.prod(counts))
        for trial in range(4):
            t = random_tally(rows * n, rng)
            if trial == 3:
                t = records(np.full(rows * n, 2 ** 32 - 1, u32), np.zeros(rows * n, u32))
            for prior in PRIORS:
                w = direct.grid_weights(e, g, t, prior)
                assert not np.isnan(w).any() and (w >= 0).all() and (w <= FLT_MAX).all()
                for row in direct.emitter_grid_cdf(e, g, t, prior).reshape(rows, n):
                    q = steps(row)
                    assert int(row[-1]) <= TOP and ((q >= 1) == (p > 0)).all()


# ---- 4. the count
V, O, I = abi.OCCL_VISIBLE, abi.OCCL_OCCLUDED, abi.OCCL_INVALID


def test_the_count_on_hand_made_items():
    #        record   bound  byte
    items = [(0, 1.5, V), (0, 2.0, O), (0, 0.0, V),      # a seen ray, a blocked one, an unlit item whose byte says visible
             (3, 0.5, V), (3, 0.5, V), (3, 0.0, I),      # two seen, an invalid item
             (5, 0.0, O), (5, -1.0, V), (5, np.nan, V),  # no pick; bounds that are not above 0 count nothing
             (2, 1e-45, O), (2, 3e38, I)]                # the smallest bound counts; a counted item with any other byte is tried only
    idx, bound, byte = (np.array(c) for c in zip(*items))
    got = direct.count(6, idx, bound.astype(f32), byte.astype(np.uint8))
    assert got.dtype == TALLY
    assert list(got["tried"]) == [2, 0, 2, 2, 0, 0] and list(got["seen"]) == [1, 0, 0, 2, 0, 0]
    # on top of a tally, which is left as it was; a call split in two is the sum of its halves
    start = records([7, 0, 1, 0, 9, 2 ** 32 - 1], [3, 0, 5, 0, 0, 1])
    keep = start.copy()
    whole = direct.count(6, idx, bound, byte, into=start)
    assert np.array_equal(start, keep)
    assert list(whole["tried"]) == [9, 0, 3, 2, 9, 2 ** 32 - 1] and list(whole["seen"]) == [4, 0, 5, 2, 0, 1]
    for cut in (0, 1, 4, 7, len(items)):
        first = direct.count(6, idx[:cut], bound[:cut], byte[:cut], into=start)
        assert np.array_equal(direct.count(6, idx[cut:], bound[cut:], byte[cut:], into=first), whole), cut
    # the counters wrap
    end = records([2 ** 32 - 1, 2 ** 32 - 2, 0, 0, 0, 0], [2 ** 32 - 1, 0, 0, 0, 0, 0])
    got = direct.count(6, [0, 0, 1, 1, 1], f32([1, 1, 1, 1, 1]), np.uint8([V, V, V, O, V]), into=end)
    assert list(got["tried"][:2]) == [1, 1] and list(got["seen"][:2]) == [1, 2]
    assert len(direct.count(0, [], [], [])) == 0
    with pytest.raises(ValueError):
        direct.count(6, [0, 1], f32([1]), np.uint8([V, V]))


def test_the_tally_of_a_call_against_a_loop_over_its_items():
    e, surf = feature_surfels()
    n = len(e)
    g = cells((-2, -2, -3), (1, 0, 0), (3, 2, 2))
    surf = np.concatenate([surf, surf[:3]])
    surf["pos"][-3] = (np.nan, 0, 0)       # invalid surfels count nothing
    surf["normal"][-2] = (0, 0, 0)
    surf["pos"][-1] = (np.inf, 0, 0)
    m, S = len(surf), 24
    ids = np.arange(50, 50 + m, dtype=u32)
    rng = np.random.default_rng(4)
    occl = rng.choice(np.uint8([V, O, O, I]), m * S)
    tabs = direct.emitter_grid_cdf(e, g)
    own = np.tile(np.cumsum([3, 0, 7, 1, 0], dtype=np.uint64).astype(u32), 12)   # rows that leave two records without a pick
    for tables in (tabs, own):
        got = direct.tally(e, surf, 5, S, g, occl, tables=tables, seeds=ids)
        bound = direct.rays(e, surf, 5, S, seeds=ids, grid=g, tables=tables)[2]
        u0 = direct.draws(m, 5, S, ids)["u0"]
        want = np.zeros(12 * n, dtype=TALLY)
        lit = 0
        for i in range(m):
            if not np.isfinite(surf["pos"][i]).all():
                assert not bound[i * S:(i + 1) * S].any()
                continue
            r = int(direct.grid_cell(surf["pos"][i:i + 1], g)[0])
            for k in range(S):
                if bound[i * S + k] > 0:
                    j = int(direct.pick_cdf(u0[i * S + k:i * S + k + 1], tables[r * n:(r + 1) * n])[0][0])
                    want["tried"][r * n + j] += 1
                    want["seen"][r * n + j] += occl[i * S + k] == V
                    lit += 1
        assert np.array_equal(got, want) and lit > 50 and 0 < want["seen"].sum() < want["tried"].sum() == lit
        assert not bound[-3 * S:].any()
        # a call split in two, the second half under its own ids, on top of the first
        cut = 5
        a = direct.tally(e, surf[:cut], 5, S, g, occl[:cut * S], tables=tables, seeds=ids[:cut])
        b = direct.tally(e, surf[cut:], 5, S, g, occl[cut * S:], tables=tables, seeds=ids[cut:], into=a)
        assert np.array_equal(b, want)
    assert (direct.tally(e, surf, 5, S, g, occl, tables=own, seeds=ids)["tried"].reshape(12, n)[:, [1, 4]] == 0).all()
    # nothing to count: no emitter, no surfel
    assert len(direct.tally(e[:0], surf, 0, 4, g, np.zeros(m * 4, np.uint8))) == 0
    assert not direct.tally(e, surf[:0], 0, 4, g, np.zeros(0, np.uint8)).view(u32).any()


# ---- 5. the estimator under an analytic occluder
def ring_and_wall():
    """16 equal lamps on a ring of radius 6, 3 above the ground, about 8 ground points within 0.5 of the ring's axis -- so every
    lamp is as far from every point as every other, to 10 % --, and the wall x = -0.75: in float64, a shadow ray is blocked when
    it starts on the points' side and ends beyond the wall.  The 8 lamps centred at x <= -1.17 (radius 0.3) are hidden whole, the
    other 8 seen whole."""
    K = 16
    ang = (np.arange(K) + 0.5) * (2 * np.pi / K)
    e = np.concatenate([one_sphere((6 * np.cos(a), 3.0, 6 * np.sin(a)), power=6.0, radius=0.3) for a in ang])
    rng = np.random.default_rng(25)
    r, th = 0.5 * np.sqrt(rng.random(8)), rng.random(8) * 2 * np.pi
    pts = np.stack([r * np.cos(th), np.zeros(8), r * np.sin(th)], axis=1).astype(f32)
    surf = hemisphere.surfels(pts, np.tile(f32([0, 1, 0]), (8, 1)))
    g = cells((-0.5, -1, -0.5), (0.5, 1, 0.5), (2, 1, 2))
    return e, surf, g


def behind_the_wall(o, d, tmax):
    """abi.OCCL_* bytes of shadow rays under the wall x = -0.75, in float64"""
    end = o[:, 0].astype(np.float64) + d[:, 0].astype(np.float64) * tmax.astype(np.float64)
    return np.where((o[:, 0] > -0.75) & (end < -0.75), O, V).astype(np.uint8)


def seen_light(e, surf, first, S, **kw):
    """(per-item value: the mean of the three channels of what the item saw, the rays' bytes, the bounds)"""
    o, d, tmax, contrib = direct.rays(e, surf, first, S, **kw)
    byte = behind_the_wall(o, d, tmax)
    return np.where(byte == V, contrib[:, :3].astype(np.float64).mean(1), 0.0), byte, tmax


def test_learned_tables_keep_the_mean_and_lose_noise_behind_a_wall():
    """Rendered: samples 0 .. 16383 of every point.  Trained: 2 rounds of 64 samples from 2^20 on, round 1 on section 24's
    tables, round 2 on round 1's, one running tally, prior 1 -- no trained sample is rendered.  Every emitter alone, summed
    (4096 samples each) is the reference.  The uniform pick and the learned pick must both lie within 4 combined standard
    errors of it, the pooled variance of section 24's tables over the learned ones must be above 1, and a factor Q / q read
    from the unlearned row -- the mutant -- must miss the reference by more than 4.
    Measured with this model: reference 0.02566 +- 0.00013; uniform 0.02561 +- 0.00015 (0.24 standard errors); learned
    0.02560 +- 0.00011 (0.36); pooled variance section 24 / learned 2.01 (uniform / learned 2.07); the mutant 0.04354, 70 %
    off, 80 standard errors."""
    e, surf, g = ring_and_wall()
    N, m = len(e), len(surf)
    SR, S, ST, T0 = 4096, 16384, 64, 1 << 20
    ref = np.zeros(m * SR)
    for j in range(N):
        ref += seen_light(e[j:j + 1], surf, 0, SR)[0]
    mr, ser = ref.mean(), ref.std(ddof=1) / np.sqrt(len(ref))
    assert sum(seen_light(e[j:j + 1], surf, 0, 64)[0].any() for j in range(N)) == 8   # half of the ring is hidden

    def against(v):
        se = np.hypot(v.std(ddof=1) / np.sqrt(len(v)), ser)
        return abs(v.mean() - mr) / se

    uni = seen_light(e, surf, 0, S)[0]
    base = direct.emitter_grid_cdf(e, g)
    plain = seen_light(e, surf, 0, S, grid=g, tables=base)[0]
    # training, on samples the render does not use
    tables, kept = base, np.zeros(4 * N, dtype=TALLY)
    for rnd in range(2):
        byte = seen_light(e, surf, T0 + rnd * ST, ST, grid=g, tables=tables)[1]
        kept = direct.tally(e, surf, T0 + rnd * ST, ST, g, byte, tables=tables, into=kept)
        tables = direct.emitter_grid_cdf(e, g, kept, 1.0)
    assert kept["tried"].sum() > 0.3 * 2 * m * ST and 0 < kept["seen"].sum() < kept["tried"].sum()
    hidden = e["a"][:, 0] < -1
    q0, q1 = (np.stack([steps(r) for r in t.reshape(4, N)]) for t in (base, tables))
    assert (q1[:, hidden].sum(1) < q0[:, hidden].sum(1)).all() and (q1[:, hidden] >= 1).all() and (q1[:, ~hidden].sum(1) >= q0[:, ~hidden].sum(1)).all()
    learned = seen_light(e, surf, 0, S, grid=g, tables=tables)[0]
    print(f"reference {mr:.5f} +- {ser:.5f}; uniform {uni.mean():.5f} +- {uni.std(ddof=1) / np.sqrt(len(uni)):.5f} ({against(uni):.2f} standard errors); "
          f"learned {learned.mean():.5f} +- {learned.std(ddof=1) / np.sqrt(len(learned)):.5f} ({against(learned):.2f})")
    print(f"pooled variance: section 24 / learned {plain.var(ddof=1) / learned.var(ddof=1):.2f}, uniform / learned {uni.var(ddof=1) / learned.var(ddof=1):.2f}")
    assert mr > 0 and against(uni) <= 4.0 and against(plain) <= 4.0
    assert against(learned) <= 4.0
    assert plain.var(ddof=1) / learned.var(ddof=1) > 1.0
    # the mutant: the learned tables' picks under the factor of the unlearned row
    row = np.repeat(direct.grid_cell(surf["pos"], g), S)
    u0 = direct.draws(m, 0, S)["u0"]
    j, q, Q = direct.pick_grid(u0, row, tables, N)
    qb = q0[row, j].astype(np.float64)
    Qb = base.reshape(4, N)[row, -1].astype(np.float64)
    mutant = learned * ((Qb / qb) / (Q.astype(np.float64) / q.astype(np.float64)))
    print(f"mutant (Q / q of the unlearned row): {mutant.mean():.5f}, {100 * (mutant.mean() / mr - 1):.0f} % off, {against(mutant):.0f} standard errors")
    assert against(mutant) > 4.0
