"""The numpy model of the lightmap stages (renderbaby_amd/lightmap.py) on the cases of
tests/_lightmap_edge_cases.py against exact arithmetic.  No device.

The reference.  Every finite binary32 number is an integer multiple of u = 2^-149, and a texel centre x + 1/2 is (2 x + 1) 2^148 u.
``exact_edge`` takes the corners ``lightmap.texel_space`` returns, as Python integers in that unit, and evaluates section 17.1's edge
function E* = (b.x - a.x) (P.y - a.y) - (b.y - a.y) (P.x - a.x) in integers, in units of u^2 = 2^-298: no float takes part, so the
values are exact at 1e30 texels as they are at 1.  (numpy carries the integers in object arrays; the arithmetic is Python's.)

The bound.  The model's binary32 E is seven operations.  The four differences b.x - a.x, P.y - a.y, b.y - a.y and P.x - a.x are off
by a relative 2^-24 each, each product adds a relative 2^-24 of its own, so a product is off by (1 + 2^-24)^3 - 1 of its exact value
p1 = |dx| |P.y - a.y| or p2 = |dy| |P.x - a.x|; the last subtraction adds 2^-24 |p1 - p2| <= 2^-24 (p1 + p2).  Together less than
4.01 2^-24 (p1 + p2), the 0.01 taking the second-order terms; a product that lands in the subnormal range is off by up to half of
2^-149 in place of its relative share, which the absolute term covers:

    |E - E*| <= B = 4.01 2^-24 (|dx| |P.y - a.y| + |dy| |P.x - a.x|) + 2^-148

as long as nothing overflows.  B is evaluated exactly as well; the code carries 100 2^24 E* and 100 2^24 B, both integers.

A (triangle, texel of its box) pair is in the band when some |E*| <= B: there the model may go either way and nothing is asserted.
The band's share of all pairs is asserted to stay at or below 1 % for the families a, b (the one-ulp neighbours), d and e -- a
condition on the cases, which keeps the assertions from going vacuous.

Barycentrics.  u = w1 / area with |w1 - w1*| <= B(w1) and |area - area*| <= B(area), derived the same way:
w1 / area - w1* / area* = (w1 - w1*) / area - u* (area - area*) / area, and the correctly rounded division adds 2^-24 |u|, so

    |u - u*| <= (B(w1) + |u*| B(area)) / |area*| + 2^-23 |u*|

(the 2^-23 takes the rounding and the difference between dividing by area and by area*), checked in integers after multiplying
through by area*^2; v likewise with w2.
"""
import functools
from fractions import Fraction

import numpy as np
import pytest

from renderbaby_amd import lightmap
from tests import _lightmap_edge_cases as lec
from tests._probe_edge_cases import mismatches

f32 = np.float32
NO = lightmap.NO_OWNER
UNIT = 149                      # coordinates in units of 2^-149
K = 100 << 24                   # E* and B are carried times 100 * 2^24 ...
ABSOLUTE = K << (2 * UNIT - 148)   # ... in units of 2^-298, where 2^-148 is 2^150
CAPPED = ("a slivers", "b tile corners", "d long lists", "e atlas shapes")


def to_int(x):
    """a finite binary32 number in units of 2^-149"""
    q = Fraction(float(x)) * (1 << UNIT)
    assert q.denominator == 1
    return q.numerator


def centres(lo, hi):
    return [(2 * k + 1) << (UNIT - 1) for k in range(lo, hi + 1)]


def exact_edge(S, T, px, py, sign=1):
    """(100 2^24 sign E*, 100 2^24 B) of the edge from S to T at the centres px x py, each an object array (len(py), len(px)) of
    Python integers.  The ends go into canonical order first, as section 17.1 has it."""
    ordered = S[0] < T[0] or (S[0] == T[0] and S[1] <= T[1])
    a, b = (S, T) if ordered else (T, S)
    dx, dy = b[0] - a[0], b[1] - a[1]
    if not ordered:
        sign = -sign
    row = np.array([dx * (y - a[1]) for y in py], dtype=object)
    col = np.array([dy * (x - a[0]) for x in px], dtype=object)
    e = (sign * K * row)[:, None] - (sign * K * col)[None, :]
    bound = (401 * np.abs(row) + ABSOLUTE)[:, None] + (401 * np.abs(col))[None, :]
    return e, bound


def exact_box(corners, width, height):
    """section 17.1's box in integers: (x0, x1, y0, y1) or None"""
    lo = [min(c[k] for c in corners) >> UNIT for k in (0, 1)]   # >> floors
    hi = [max(c[k] for c in corners) >> UNIT for k in (0, 1)]
    if hi[0] < 0 or hi[1] < 0 or lo[0] > width - 1 or lo[1] > height - 1:
        return None
    return max(lo[0], 0), min(hi[0], width - 1), max(lo[1], 0), min(hi[1], height - 1)


class Exact:
    """what exact arithmetic says of one triangle with finite corners: ``area`` and ``area_bound`` (scaled as above), ``box``,
    and over the box the three edge values turned to the triangle's side (positive inside) with their bounds"""

    def __init__(self, a, b, c, width, height):
        self.corners = [tuple(to_int(v) for v in p) for p in (a, b, c)]
        A, B, C = self.corners
        area, bound = exact_edge(A, B, [C[0]], [C[1]])
        self.area, self.area_bound = area[0, 0], bound[0, 0]
        self.box = exact_box(self.corners, width, height)
        self.side = 1 if self.area > 0 else -1

    def edges(self):
        x0, x1, y0, y1 = self.box
        px, py = centres(x0, x1), centres(y0, y1)
        A, B, C = self.corners
        return [exact_edge(S, T, px, py, self.side) for S, T in ((B, C), (C, A), (A, B))]   # w0, w1, w2

    def classify(self, edges=None):
        """(clearly inside, clearly outside, in the band), bool arrays over the box"""
        inside, outside, band = True, False, False
        for e, bound in edges or self.edges():
            inside = inside & (e > bound)
            outside = outside | (-e > bound)
            band = band | ((e <= bound) & (-e <= bound))
        return inside.astype(bool), outside.astype(bool), band.astype(bool)


def finite_corners(A, B, C, k):
    return bool(np.isfinite(A[k]).all() and np.isfinite(B[k]).all() and np.isfinite(C[k]).all())


def alone(tris, uvs, width, height, k):
    """the texels triangle k covers by the model, whatever the other triangles do"""
    return lightmap.owners(tris[k:k + 1], uvs, width, height) != NO


@functools.lru_cache(maxsize=None)
def audit(family):
    """One pass over every triangle of every case of a family: per case the pairs examined and those in the band, the centres
    clearly inside a triangle that are not owned by it or a lower index, the owned texels clearly outside their owner, and the
    barycentrics beyond their bound."""
    rows = []
    for index, (name, tris, uvs, width, height) in enumerate(lec.cases(family)):
        own = lec.model(family, index)[1].reshape(height, width)
        u, v = lightmap.barycentrics(tris, uvs, width, height, own)
        A, B, C = lightmap.texel_space(tris, uvs, width, height)
        r = dict(name=name, pairs=0, band=0, holes=0, strays=0, bary=0, bary_bad=0, owners_without_a_box=0, in_area_band=0)
        may_own = np.zeros(len(tris) + 1, bool)
        for k in range(len(tris)):
            if not finite_corners(A, B, C, k):
                continue
            t = Exact(A[k], B[k], C[k], width, height)
            if t.area == 0 or t.box is None:
                continue
            may_own[k] = True
            x0, x1, y0, y1 = t.box
            n = (x1 - x0 + 1) * (y1 - y0 + 1)
            r["pairs"] += n
            if abs(t.area) <= t.area_bound:   # the model's own area may have either sign: the whole triangle is band
                r["band"] += n
                r["in_area_band"] += 1
                continue
            edges = t.edges()
            inside, outside, band = t.classify(edges)
            mine = own[y0:y1 + 1, x0:x1 + 1]
            r["band"] += int(band.sum())
            r["holes"] += int((inside & (mine > k)).sum())          # NO_OWNER is the largest uint32
            r["strays"] += int((outside & (mine == k)).sum())
            if abs(t.area) >= (K << (2 * UNIT - 10)) and (mine == k).any():
                ys, xs = np.nonzero(mine == k)
                for got, (w, wb) in ((u, edges[1]), (v, edges[2])):
                    U = np.array([to_int(g) for g in got[y0 + ys, x0 + xs]], dtype=object)
                    w, wb, area = w[ys, xs] * t.side, wb[ys, xs], t.area
                    lhs = np.abs(U * area - w * (1 << UNIT)) * abs(area)
                    rhs = (wb * abs(area) + np.abs(w) * t.area_bound) * (1 << UNIT) + np.abs(w) * abs(area) * (1 << (UNIT - 23))
                    r["bary"] += len(U)
                    r["bary_bad"] += int((lhs > rhs).sum())
        may_own[-1] = True
        owners = np.unique(own)
        r["owners_without_a_box"] = int((~may_own[np.minimum(owners, len(tris))]).sum())
        rows.append(r)
    return rows


def share(rows):
    pairs, band = sum(r["pairs"] for r in rows), sum(r["band"] for r in rows)
    return pairs, band, band / max(pairs, 1)


@pytest.mark.parametrize("family", CAPPED)
def test_cover_against_exact_arithmetic(family):
    """no hole, no stray owner, and the band's share of the pairs at or below 1 %"""
    rows = audit(family)
    if family == "b tile corners":   # at the dyadic ones the edge passes through centres: |E*| = 0 there, and they are held exactly below
        rows = [r for r in rows if "dyadic" not in r["name"]]
    pairs, band, part = share(rows)
    print(f"{family}: {len(rows)} cases, {pairs} pairs examined, {band} in the band: {100 * part:.4f} %")
    for r in rows:
        assert r["holes"] == 0 and r["strays"] == 0 and r["owners_without_a_box"] == 0, r
    assert pairs > 0 and part <= 0.01, (family, pairs, band)


@pytest.mark.parametrize("family", CAPPED)
def test_barycentrics_against_exact_arithmetic(family):
    rows = audit(family)
    checked, bad = sum(r["bary"] for r in rows), sum(r["bary_bad"] for r in rows)
    print(f"{family}: {checked} values of u and v checked, {bad} beyond the bound")
    assert checked > 0 and bad == 0, [r for r in rows if r["bary_bad"]]


def shared_edge_pairs(tris, uvs, width, height):
    """(k, k + 1, S, T): neighbours in the list that have exactly two corners in common, bit for bit in texel space"""
    A, B, C = lightmap.texel_space(tris, uvs, width, height)
    out = []
    for k in range(len(tris) - 1):
        if not (finite_corners(A, B, C, k) and finite_corners(A, B, C, k + 1)):
            continue
        first = {p.tobytes(): p for p in (A[k], B[k], C[k])}
        common = [first[p.tobytes()] for p in (A[k + 1], B[k + 1], C[k + 1]) if p.tobytes() in first]
        if len(first) == 3 and len(common) == 2:
            out.append((k, k + 1, common[0], common[1]))
    return out


@pytest.mark.parametrize("family", ["a slivers", "e atlas shapes"])
def test_no_texel_is_owned_from_both_sides_of_a_shared_edge(family):
    pairs = doubles = on_edge = 0
    for name, tris, uvs, width, height in lec.cases(family):
        for k, m, s, t in shared_edge_pairs(tris, uvs, width, height):
            both = alone(tris, uvs, width, height, k) & alone(tris, uvs, width, height, m)
            pairs += 1
            for y, x in np.argwhere(both):
                e, _ = exact_edge(tuple(map(to_int, s)), tuple(map(to_int, t)), centres(x, x), centres(y, y))
                on_edge += 1
                doubles += int(e[0, 0] != 0)
    print(f"{family}: {pairs} pairs, {on_edge} texels owned from both sides with the edge's exact value 0, {doubles} with another")
    assert pairs >= 20 and doubles == 0


def test_dyadic_triangles_are_covered_exactly():
    """family b's dyadic triangles: the model's cover is the exact rule ``>= 0`` texel for texel -- no band"""
    cases = [c for c in lec.cases("b tile corners") if "dyadic" in c[0]]
    on_edge = covered = lone = 0
    for name, tris, uvs, width, height in cases:
        A, B, C = lightmap.texel_space(tris, uvs, width, height)
        for k in range(len(tris)):
            t = Exact(A[k], B[k], C[k], width, height)
            want = np.zeros((height, width), bool)
            x0, x1, y0, y1 = t.box
            edges = [e for e, _ in t.edges()]
            inside = (edges[0] >= 0) & (edges[1] >= 0) & (edges[2] >= 0)
            want[y0:y1 + 1, x0:x1 + 1] = inside.astype(bool)
            got = alone(tris, uvs, width, height, k)
            assert np.array_equal(got, want), (name, k, np.argwhere(got != want)[:5])
            zero = inside & ((edges[0] == 0) | (edges[1] == 0) | (edges[2] == 0))
            on_edge += int(zero.sum())
            covered += int(want.sum())
            # tiles of which a corner centre on the edge is the only covered texel: what the equality in lm_tile_outside decides
            full = np.zeros((height, width), bool)
            full[y0:y1 + 1, x0:x1 + 1] = zero.astype(bool)
            T = lec.TILE
            per_tile = want.reshape(height // T, T, width // T, T).sum((1, 3))
            lone += int(((per_tile == 1) & (full.reshape(height // T, T, width // T, T).sum((1, 3)) == 1)).sum())
    print(f"dyadic: {len(cases)} cases, {covered} covered texels, {on_edge} of them with an exact edge value of 0, {lone} tiles whose only covered texel is one")
    assert on_edge > 500 and lone > 50


def test_far_corners_cover_nothing_outside_the_exact_triangle():
    """Family c.  A triangle whose exact area is non-zero and whose binary32 area is finite and non-zero covers no texel outside
    the exact triangle by more than B; one with a non-finite corner, or whose area overflowed or is a NaN, covers nothing."""
    kept = dropped = covered = band = pairs = 0
    for name, tris, uvs, width, height in lec.cases("c far corners"):
        A, B, C = lightmap.texel_space(tris, uvs, width, height)
        for k in range(len(tris)):
            got = alone(tris, uvs, width, height, k)
            area = lightmap.edge(A[k], B[k], C[k]) if finite_corners(A, B, C, k) else f32(np.nan)
            if not np.isfinite(area):
                dropped += 1
                assert not got.any(), (name, k, "a triangle without a finite area covers", int(got.sum()))
                continue
            t = Exact(A[k], B[k], C[k], width, height)
            if area == 0 or t.area == 0 or t.box is None:
                assert area != 0 or not got.any(), (name, k)
                continue
            kept += 1
            x0, x1, y0, y1 = t.box
            inside, outside, in_band = t.classify()
            mine = got[y0:y1 + 1, x0:x1 + 1]
            assert int(got.sum()) == int(mine.sum()), (name, k, "covered outside its box")
            assert not (mine & outside).any(), (name, k, np.argwhere(mine & outside)[:5] + (y0, x0), float(area))
            covered, band, pairs = covered + int(mine.sum()), band + int(in_band.sum()), pairs + mine.size
    print(f"c far corners: {kept} triangles with a finite area ({covered} texels covered, {band} of {pairs} pairs in the band), {dropped} without")
    assert kept >= 40 and dropped >= 20 and covered > 1000


def test_the_cases_reach_what_they_are_there_for():
    """conditions on the inputs: the last tile column is reached, the long lists hold the runs they claim, family g makes NaNs"""
    name, tris, uvs, width, height = lec.cases("a slivers")[-1]
    own = lec.model("a slivers", len(lec.cases("a slivers")) - 1)[1].reshape(height, width)
    assert (width, height) == (257, 255) and set(own[:, 256][own[:, 256] != NO]) == {0, 1}
    boxes = [lightmap._box(a, b, c, 257, 255) for a, b, c in zip(*lightmap.texel_space(*lec.cases("a slivers")[4][1:3], 257, 255))]
    assert max((b[1] // 8 - b[0] // 8 + 1) * (b[3] // 8 - b[2] // 8 + 1) for b in boxes) >= 500, "no sliver's box has hundreds of tiles"
    for index, (name, tris, uvs, width, height) in enumerate(lec.cases("d long lists")):
        assert len(tris) == lec.LIST_LENGTH == 20001
        for mesh in (None, 0):
            units = np.array([k for k, *_ in lightmap._covering(tris, uvs, width, height, mesh, None)])
            has = np.zeros(len(tris), bool)
            has[units] = True
            runs = sorted(int(g) for g in np.diff(np.flatnonzero(np.concatenate([[True], has, [True]]))) - 1 if g > 0)
            if name == "the last alone has units":
                assert runs == [20000] and units.tolist() == [20000]
            elif mesh is None:
                assert runs == sorted(lec.RUNS), (name, runs)
                assert has[0] == (name == "ends with a run") and has[-1] == (name == "begins with a run")
            else:   # the stretches of the other mesh lengthen the runs and add new ones
                assert max(runs) >= 4097 and len(runs) > len(lec.RUNS)
    nans = 0
    for index in range(len(lec.cases("g surfels out of range"))):
        surf, own = lec.model("g surfels out of range", index)
        assert (own != NO).all()
        nans += int(np.isnan(surf["pos"]).sum())
    assert nans > 100
    for family in lec.NO_NAN_FAMILIES:
        for index in range(len(lec.cases(family))):
            surf, _ = lec.model(family, index)
            assert not np.isnan(surf.view(f32)).any(), (family, index)


# ---- the resolve
def scalar_resolve(sums, width, height, dilate):
    """Section 17.1's "Resolve" paragraph, one texel and one neighbour at a time.  Pass 0: a texel with ``sums.w > 0`` gets {r / w,
    g / w, b / w, 1}, every other {0, 0, 0, 0}.  Then ``dilate`` passes, each reading only the pass before: a texel whose fourth
    component is 0 looks at its neighbours in the order (-1,-1), (0,-1), (1,-1), (-1,0), (1,0), (-1,1), (0,1), (1,1) of (dx, dy),
    uses those inside the atlas -- no wrap -- with a non-zero fourth component, and with c > 0 of them becomes {sum r / float(c),
    sum g / float(c), sum b / float(c), 2}, each sum taken from +0.0f in that order."""
    zero = f32(0.0)
    cur = [[(zero, zero, zero, zero)] * width for _ in range(height)]
    with np.errstate(all="ignore"):
        for y in range(height):
            for x in range(width):
                s = sums[y * width + x]
                w = f32(s["weight"])
                if w > zero:
                    cur[y][x] = (f32(s["sum"][0]) / w, f32(s["sum"][1]) / w, f32(s["sum"][2]) / w, f32(1.0))
        for _ in range(dilate):
            nxt = [row[:] for row in cur]
            for y in range(height):
                for x in range(width):
                    if cur[y][x][3] != zero:
                        continue
                    r, g, b, c = zero, zero, zero, 0
                    for dx, dy in ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)):
                        nx, ny = x + dx, y + dy
                        if nx < 0 or nx >= width or ny < 0 or ny >= height:
                            continue
                        q = cur[ny][nx]
                        if q[3] != zero:
                            r, g, b, c = f32(r + q[0]), f32(g + q[1]), f32(b + q[2]), c + 1
                    if c > 0:
                        nxt[y][x] = (f32(r / f32(c)), f32(g / f32(c)), f32(b / f32(c)), f32(2.0))
            cur = nxt
    return np.array(cur, dtype=f32).reshape(height, width, 4)


@pytest.mark.parametrize("dilate", [0, 1, 2, 3, 5])
def test_resolve_matches_its_definition_on_the_records(dilate):
    """family f; a word that is a NaN by the definition is a NaN of any sign and payload in the model, every other word is equal
    in every bit"""
    nan_words = filled = 0
    for name, sums, width, height in lec.cases("f resolve records"):
        got = lightmap.resolve(sums, width, height, dilate)
        want = scalar_resolve(sums, width, height, dilate)
        assert got.dtype == f32 and got.shape == (height, width, 4)
        bad, nans = mismatches(got, want, 4, nan_rule=True)
        assert len(bad) == 0, (name, dilate, len(bad), bad[:5], got.reshape(-1, 4)[bad[:5]], want.reshape(-1, 4)[bad[:5]])
        nan_words += nans
        filled += int((want[..., 3] == 2).sum())
        if "one texel at" in name:   # the fill never crosses the border: after k passes the chart has grown k texels and no more
            x, y = (int(n) for n in name.split("(")[1].rstrip(")").split(","))
            ys, xs = np.mgrid[0:height, 0:width]
            reach = np.maximum(np.abs(xs - x), np.abs(ys - y))
            assert np.array_equal(want[..., 3] != 0, reach <= dilate), (name, dilate)
            assert (want[..., :3][reach <= dilate] == (1.0, 0.5, 0.25)).all()
    print(f"dilate {dilate}: {nan_words} NaN words compared under the rule, {filled} filled texels")
    assert nan_words > 0 and (filled > 0) == (dilate > 0)
