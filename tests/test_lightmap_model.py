"""The numpy model of the lightmap stages (renderbaby_amd/lightmap.py) against exact arithmetic: the cover
rule leaves no hole and no doubly owned texel on random convex quads, an owned texel's interpolated uv lands on the texel itself
through sample_texture's index formula, overlaps go to the lowest index, and the resolve is what its definition says."""
import numpy as np
import pytest

from renderbaby_amd import abi, lightmap
from tests._lightmap_scenes import convex_quad, quad_triangles, uv_triangles

f32 = np.float32
NO = lightmap.NO_OWNER


def exact_edge(s, t, px, py):
    """(t - s) x (P - s) in float64 on float32 corners and half-integer P: the differences are exact, the two products and their
    difference are off by less than 1e-11 at these sizes -- seven orders inside the margin the test asks for"""
    return (float(t[0]) - float(s[0])) * (py - float(s[1])) - (float(t[1]) - float(s[1])) * (px - float(s[0]))


def quad_cases():
    """(width, height, quad, diagonal, clockwise) -- 400 of them, atlases from 1 x 1 to 69 x 69"""
    rng = np.random.default_rng(17)
    sizes = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (7, 5), (8, 8), (9, 17), (64, 64), (65, 63), (69, 69), (69, 1), (1, 69)]
    out = []
    for k in range(400):
        w, h = sizes[k % len(sizes)] if k < 3 * len(sizes) else (int(rng.integers(1, 70)), int(rng.integers(1, 70)))
        out.append((w, h, convex_quad(rng), k % 2, (k // 2) % 2 == 1))
    return out


@pytest.fixture(scope="module")
def quads():
    res = []
    for w, h, q, diagonal, clockwise in quad_cases():
        t, shared = quad_triangles(q, diagonal, clockwise)
        tris, uvs = uv_triangles(t)
        res.append(dict(w=w, h=h, q=q, tris=tris, uvs=uvs, shared=shared, own=lightmap.owners(tris, uvs, w, h),
                        halves=[lightmap.owners(tris[k:k + 1], uvs, w, h) for k in (0, 1)]))
    return res


def test_no_hole_and_no_double_owner_on_convex_quads(quads):
    covered = holes = doubles = 0
    for c in quads:
        w, h = c["w"], c["h"]
        # the quad in texel space, by the model's own float32 corners: the atlas geometry is what those are
        A, B, C = lightmap.texel_space(*uv_triangles([tuple(c["q"][:3]), (c["q"][0], c["q"][2], c["q"][3])]), w, h)
        corners = [A[0], B[0], C[0], C[1]]   # q0 q1 q2 q3 in texels; v is flipped, so the winding there is clockwise
        ys, xs = np.mgrid[0:h, 0:w]
        px, py = xs + 0.5, ys + 0.5
        inside = np.ones((h, w), bool)
        for k in range(4):
            inside &= -exact_edge(corners[k], corners[(k + 1) % 4], px, py) > 1e-4
        covered += int(inside.sum())
        holes += int((inside & (c["own"] == NO)).sum())
        both = (c["halves"][0] != NO) & (c["halves"][1] != NO)
        if both.any():
            sa, sb = lightmap.texel_space(*uv_triangles([(c["shared"][0], c["shared"][1], c["shared"][0])]), w, h)[:2]
            P = np.stack([px[both].astype(f32), py[both].astype(f32)], axis=-1)
            doubles += int((lightmap.edge(sa[0], sb[0], P) != 0).sum())
    print(dict(covered=covered, holes=holes, doubles=doubles))
    assert covered > 40000, "the fixture covers too few texels to say anything"
    assert holes == 0 and doubles == 0


def test_an_owned_texels_uv_lands_on_the_texel(quads):
    """tri_uv's formula (shader.wgsl:353-361) on the model's (u, v), then sample_texture's index formula (:173-179)"""
    checked = misses = 0
    for c in quads:
        w, h, tris, uvs = c["w"], c["h"], c["tris"], c["uvs"]
        A, B, C = lightmap.texel_space(tris, uvs, w, h)
        areas = [abs(float(lightmap.edge(A[k], B[k], C[k]))) for k in (0, 1)]
        if min(areas) < 2.0:   # the fixture keeps to triangles of one texel^2 or more (the edge value is twice the area)
            continue
        own = c["own"]
        u, v = lightmap.barycentrics(tris, uvs, w, h, own)
        ys, xs = np.nonzero(own != NO)
        k = own[ys, xs].astype(np.int64)
        uu, vv = u[ys, xs], v[ys, xs]
        ww = ((f32(1.0) - uu).astype(f32) - vv).astype(f32)
        i0, i1, i2 = tris["v0_index"][k].astype(np.int64), tris["v1_index"][k].astype(np.int64), tris["v2_index"][k].astype(np.int64)
        uv = [(((ww * uvs[2 * i0 + a]).astype(f32) + (uu * uvs[2 * i1 + a]).astype(f32)).astype(f32) + (vv * uvs[2 * i2 + a]).astype(f32)).astype(f32)
              for a in (0, 1)]
        fu, fv = (uv[0] - np.floor(uv[0])).astype(f32), (uv[1] - np.floor(uv[1])).astype(f32)
        x = np.minimum((fu * f32(w)).astype(f32).astype(np.int64), w - 1)
        y = np.minimum(((f32(1.0) - fv).astype(f32) * f32(h)).astype(f32).astype(np.int64), h - 1)
        checked += len(xs)
        misses += int(((x != xs) | (y != ys)).sum())
    print(dict(checked=checked, misses=misses))
    assert checked > 30000
    assert misses == 0


def test_model_edge_is_exact_negation_across_a_shared_edge():
    rng = np.random.default_rng(3)
    P = (rng.integers(0, 64, (500, 2)) + 0.5).astype(f32)
    for _ in range(50):
        s, t = (rng.uniform(0, 64, 2)).astype(f32), (rng.uniform(0, 64, 2)).astype(f32)
        a, b = lightmap.edge(s, t, P), lightmap.edge(t, s, P)
        assert np.array_equal(a.view(np.uint32) ^ np.uint32(0x80000000), b.view(np.uint32))
        # and the sign is the exact one wherever the exact value is clear of the rounding
        e64 = exact_edge(s, t, P[:, 0].astype(np.float64), P[:, 1].astype(np.float64))
        clear = np.abs(e64) > 1e-2
        assert (np.sign(a[clear]) == np.sign(e64[clear])).all()


def test_the_lowest_index_owns_an_overlap():
    a = [(0.1, 0.1), (0.9, 0.1), (0.1, 0.9)]
    b = [(0.2, 0.05), (0.95, 0.8), (0.2, 0.95)]
    for order in ((a, b), (b, a)):
        tris, uvs = uv_triangles(list(order))
        own = lightmap.owners(tris, uvs, 33, 31)
        first = lightmap.owners(tris[:1], uvs, 33, 31)
        second = lightmap.owners(tris[1:], uvs, 33, 31)   # (its indices 3 .. 5 still point into uvs)
        assert ((first != NO) & (second != NO)).sum() > 50, "the triangles do not overlap"
        assert (own[first != NO] == 0).all()
        assert (own[(first == NO) & (second != NO)] == 1).all()
        assert (own[(first == NO) & (second == NO)] == NO).all()
    # the mesh filter and the short triangle count take a triangle out altogether
    tris, uvs = uv_triangles([a, b], meshes=[0, 1])
    assert set(np.unique(lightmap.owners(tris, uvs, 33, 31, mesh=1))) == {1, NO}
    assert set(np.unique(lightmap.owners(tris, uvs, 33, 31, tri_count=1))) == {0, NO}


def scalar_resolve(sums, w, h, dilate):
    """the definition of section 17's resolve, one texel at a time"""
    cur = np.zeros((h, w, 4), f32)
    for y in range(h):
        for x in range(w):
            s = sums[y * w + x]
            if s["weight"] > 0:
                cur[y, x] = [f32(s["sum"][0]) / f32(s["weight"]), f32(s["sum"][1]) / f32(s["weight"]), f32(s["sum"][2]) / f32(s["weight"]), 1]
    for _ in range(dilate):
        nxt = cur.copy()
        for y in range(h):
            for x in range(w):
                if cur[y, x, 3] != 0:
                    continue
                acc, c = [f32(0), f32(0), f32(0)], 0
                for dx, dy in ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)):
                    if 0 <= x + dx < w and 0 <= y + dy < h and cur[y + dy, x + dx, 3] != 0:
                        acc = [f32(acc[k] + cur[y + dy, x + dx, k]) for k in range(3)]
                        c += 1
                if c:
                    nxt[y, x] = [f32(acc[0] / f32(c)), f32(acc[1] / f32(c)), f32(acc[2] / f32(c)), 2]
        cur = nxt
    return cur


def hand_made_sums():
    """5 x 4: an isolated baked texel at (0, 0) -- a corner --, a chart of three at the right edge, an invalid weight"""
    s = np.zeros(20, dtype=abi.RADIANCE)
    s[0] = ((3.0, 1.5, 0.75), 3.0)
    s[1 * 5 + 3] = ((0.1, 0.2, 0.3), 7.0)
    s[1 * 5 + 4] = ((5.0, 6.0, 7.0), 2.0)
    s[2 * 5 + 4] = ((1e-3, 0.0, 9.0), 1.0)
    s[3 * 5 + 1] = ((4.0, 4.0, 4.0), 0.0)      # traced nothing: empty
    s[3 * 5 + 2] = ((4.0, 4.0, 4.0), -1.0)     # a weight that is not positive: empty
    return s


@pytest.mark.parametrize("dilate", [0, 1, 2, 3, 64])
def test_resolve_matches_its_definition(dilate):
    s = hand_made_sums()
    got = lightmap.resolve(s, 5, 4, dilate)
    want = scalar_resolve(s, 5, 4, dilate)
    assert got.dtype == f32 and got.shape == (4, 5, 4)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert tuple(got[0, 0]) == (1.0, 0.5, 0.25, 1.0)
    assert got[3, 1, 3] == (0 if dilate < 2 else 2) and got[3, 2, 3] == (0 if dilate < 2 else 2) and got[2, 3, 3] == (0 if dilate < 1 else 2)
    if dilate == 0:
        assert (got[..., 3] == 1).sum() == 4 and (got[..., 3] == 0).sum() == 16
    if dilate == 1:
        assert tuple(got[1, 1]) == (1.0, 0.5, 0.25, 2.0)    # the isolated texel's only neighbour value
    if dilate >= 3:   # larger than the map: everything is filled and nothing moves any more
        assert (got[..., 3] != 0).all()
        assert np.array_equal(got, lightmap.resolve(s, 5, 4, 3))
