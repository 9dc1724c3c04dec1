"""The degenerate inputs of the lightmap kernels, shared by tests/test_lightmap_edges_model.py (the numpy
model against exact integer arithmetic, no device) and tests/test_gpu_lightmap_edges.py (the device against the model).  No
device, no library.  Every input is one the ABI accepts; nothing aims at an index out of range.

Families a - e and g return (name, tris, uvs, width, height) tuples built with ``_lightmap_scenes.uv_triangles``; family f returns
(name, abi.RADIANCE sums, width, height).  ``FAMILIES`` names them, ``cases(family)`` builds a family once and ``model`` keeps
the model's answer to a case, so the two test files share one evaluation of it.
"""
import functools
import itertools

import numpy as np

from renderbaby_amd import abi, lightmap
from tests._lightmap_scenes import many_triangles, uv_triangles

f32, f64, u32 = np.float32, np.float64, np.uint32
TILE = 8   # kLmTile: the cover pass's units are 8 x 8-texel tiles


def bits(x):
    return np.array([x], u32).view(f32)[0]


SUB_MIN, FLT_MIN, FLT_MAX = bits(1), bits(0x00800000), bits(0x7F7FFFFF)
PAYLOAD_NAN = bits(0x7FA12345)
INF = f32(np.inf)
SLOPES = (1 / 64, 1 / 7, 1.0, 7.0, 64.0)
WIDTHS = (0.3, 1.0, 3.0)


def uv_of(points, width, height):
    """texel coordinates (x right, y down) -> the float32 uvs the atlas maps back to them: (x / width, 1 - y / height)"""
    p = np.asarray(points, f64)
    with np.errstate(all="ignore"):
        return np.stack([p[..., 0] / width, 1.0 - p[..., 1] / height], axis=-1).astype(f32)


def case(name, texel_tris, width, height, meshes=None):
    tris, uvs = uv_triangles(uv_of(texel_tris, width, height), meshes, shared=True)
    return name, tris, uvs, width, height


# ---- a. slivers
def _sliver_set(width, height, slope, outside):
    """Eight slivers along the direction (1, slope), side by side: the three ``WIDTHS`` in both windings, then a pair that
    shares its long edge.  Each runs from an apex to a short base of the given width, through a point near the middle of the
    atlas.  ``outside``: the ends lie four atlas sizes from the middle along the dominant axis, so the box is clamped; else the
    sliver is as long as fits between 2 % and 98 % of the atlas, at most the diagonal."""
    d = np.array([1.0, slope]) / np.hypot(1.0, slope)
    n = np.array([-d[1], d[0]])
    gap = max(min(width, height) / 10.0, 0.37)
    out = []
    for j, (wd, clockwise) in enumerate(list(itertools.product(WIDTHS, (False, True))) + [(1.7, None)]):
        c = np.array([width * 0.5037, height * 0.4971]) + (j - 3) * gap * n
        if outside:
            t0 = t1 = 4.0 * min(width / abs(d[0]), height / abs(d[1]))
        else:
            lo, hi = np.array([0.02 * width, 0.02 * height]), np.array([0.98 * width, 0.98 * height])
            c = np.clip(c, lo + 0.2 * (hi - lo), hi - 0.2 * (hi - lo))
            t1 = 0.98 * min(np.min((hi - c) / np.abs(d)), np.min((c - lo) / np.abs(d)), 0.5 * np.hypot(width, height))
            t0 = t1
        apex, base = c - t0 * d, c + t1 * d
        p1, p2 = base - 0.5 * wd * n, base + 0.5 * wd * n
        if clockwise is None:   # the pair: (apex, p1) is the edge both have, with the same uv bits
            out += [(apex, p1, p2), (p1, apex, base - 1.5 * wd * n)]
        else:
            out.append((apex, p2, p1) if clockwise else (apex, p1, p2))
    return out


def slivers():
    """Reaches ``lm_tile_outside`` where it does nearly all the work: triangles 0.3 to 3 texels wide and as long as the atlas'
    diagonal at the slopes 1/64, 1/7, 1, 7 and 64, whose boxes are up to 33 x 32 tiles of which the corner test keeps a few dozen.
    Atlases 257 x 255 (a last tile column one texel wide, a last tile row seven high) and 64 x 256; corners inside the atlas, and
    corners four atlas sizes outside so that the box is clamped; both windings; a pair per set that shares its long edge with the
    same uv bits; and one sliver whose base lies inside the one-texel-wide tile column 32 of the 257-wide atlas."""
    out = []
    for width, height in ((257, 255), (64, 256)):
        for slope, outside in itertools.product(SLOPES, (False, True)):
            name = f"{width}x{height} slope {slope:.4g} {'clamped' if outside else 'inside'}"
            out.append(case(name, _sliver_set(width, height, slope, outside), width, height))
    last = [((200.3, 100.2), (256.8, 107.1), (256.8, 108.9)), ((200.3, 120.2), (256.8, 128.9), (256.8, 127.1))]
    out.append(case("257x255 ends in the last tile column", last, 257, 255))
    return out


# ---- b. edges through tile corners
B_SIDE = 128   # a power of two: u * 128 and (1 - v) * 128 are exact for the dyadic corners below


def _corner_lines():
    """(name, S, T, third corner): edges S-T through texel centres that are corners of tiles, and a third corner that puts the
    triangle on the side where such a centre is the only texel of its tile that the edge leaves inside"""
    s = float(B_SIDE)
    return [
        # x + y = 129: through (8k + 0.5, 8m + 0.5) with 8k + 8m = 128; below it, only that corner of the tile is inside
        ("c0 on x+y=129", (-7.5, 136.5), (136.5, -7.5), (-7.25, -7.25)),
        # x + y = 127: through (8k + 7.5, 8m + 7.5) with 8k + 8m = 112; above it, only that corner
        ("c3 on x+y=127", (-9.5, 136.5), (136.5, -9.5), (s + 9.25, s + 9.25)),
        # y = x - 7: through (8k + 7.5, 8m + 0.5), k = m; right of and above it, only that corner
        ("c1 on y=x-7", (-0.5, -7.5), (135.5, 128.5), (s + 9.25, -9.25)),
        # y = x + 7: through (8k + 0.5, 8m + 7.5)
        ("c2 on y=x+7", (-7.5, -0.5), (128.5, 135.5), (-9.25, s + 9.25)),
        # the diagonal itself: through (8k + 0.5, 8k + 0.5) and (8k + 7.5, 8k + 7.5) alike
        ("both on y=x", (-7.5, -7.5), (135.5, 135.5), (-9.25, s + 3.25)),
        # slope 1/2 through (16j + 0.5, 8j + 0.5), and slope 2 through (8j + 7.5, 16j + 7.5)
        ("c0 on slope 1/2", (-15.5, -7.5), (144.5, 72.5), (20.25, s + 9.25)),
        ("c3 on slope 2", (-0.5, -8.5), (71.5, 135.5), (s + 9.25, 20.25)),
        # an axis-parallel edge along a column of tile corners, and one along a row
        ("c0 on x=64.5", (64.5, -3.5), (64.5, 131.5), (s + 5.25, 60.25)),
        ("c3 on y=63.5", (-3.5, 63.5), (131.5, 63.5), (60.25, -5.25)),
    ]


def tile_corner_edges():
    """Reaches the equality in ``lm_tile_outside``: a tile whose only covered texel is a corner centre at which the edge function
    is exactly zero, all the tile's other corners being outside.  Dyadic corners (multiples of 1/4 texel on a 128 x 128 atlas,
    every product in E exact, so coverage is known exactly) put an edge through the centres (8k + 0.5, 8m + 0.5), (8k + 7.5, 8m +
    7.5) and the two mixed kinds, in both windings; cases named ``dyadic``.  The cases named ``-1 ulp`` and ``+1 ulp`` are the
    same triangles with one end of that edge moved by one ulp of its u: the centres that lay on the edge now lie off it by less
    than the rounding of E."""
    out = []
    for name, s, t, c in _corner_lines():
        tri = [(s, t, c), (s, c, t)]
        out.append(case(f"{name} dyadic", tri, B_SIDE, B_SIDE))
        for step, label in ((-1, "-1 ulp"), (1, "+1 ulp")):
            uv = uv_of(tri, B_SIDE, B_SIDE)
            uv[:, 0, 0] = np.nextafter(uv[:, 0, 0], f32(step * np.inf))
            tris, uvs = uv_triangles(uv, shared=True)
            out.append((f"{name} {label}", tris, uvs, B_SIDE, B_SIDE))
    return out


# ---- c. far corners
def far_corners():
    """Reaches E where it rounds coarsely or overflows, in ``lm_setup``, ``lm_tile_outside`` and the cover test alike: one corner
    at 1e6, 1e12, 1e20, 1e30 and 3e38 texels (u = value / width) towards +u, -u, +u and -v, and -v, the other two corners inside
    the atlas, both windings; two far corners whose ``area`` overflows to inf, and two whose products make inf - inf; corners at
    +-FLT_MAX / width, which times width land on FLT_MAX or on inf; subnormal and -0.0f uvs."""
    out = []
    for width, height in ((64, 64), (65, 63)):
        inside = ((0.31 * width, 0.22 * height), (0.72 * width, 0.83 * height))
        for value in (1e6, 1e12, 1e20, 1e30, 3e38):
            tri = []
            for far in ((value, 0.4 * height), (-value, 0.6 * height), (value, value), (0.55 * width, value), (0.45 * width, -value)):
                tri += [(far, inside[0], inside[1]), (far, inside[1], inside[0])]
            out.append(case(f"{width}x{height} corner at {value:g}", tri, width, height))
        m = (0.5 * width, 0.5 * height)
        out.append(case(f"{width}x{height} area overflows", [((1e30, 3.0), (5.0, 1e30), m), ((1e30, 3.0), m, (5.0, 1e30)),
                                                               ((-1e38, -1e38), (1e38, 1e38), m), ((-1e38, -1e38), m, (1e38, 1e38)),
                                                               ((-1e25, -1e25), (1e25, 1e25), m), ((-1e19, -1e19), (1e19, 1.0000001e19), m)],
                        width, height))
        # uvs given directly: +-FLT_MAX / width, subnormals, -0.0
        big = f32(FLT_MAX / f32(width))
        uv = [[(big, 0.5), (0.2, 0.2), (0.8, 0.7)], [(-big, 0.5), (0.8, 0.7), (0.2, 0.2)], [(0.5, big), (0.2, 0.2), (0.8, 0.7)],
              [(0.5, -big), (0.2, 0.2), (0.8, 0.7)], [(FLT_MAX, 0.5), (0.2, 0.2), (0.8, 0.7)], [(big, -big), (0.2, 0.2), (0.8, 0.7)],
              [(SUB_MIN, 1.0), (0.6, -0.0), (-0.0, -0.0)], [(-0.0, 1.0), (-0.0, SUB_MIN), (0.7, FLT_MIN)],
              [(-SUB_MIN, 0.5), (0.5, -SUB_MIN), (1.0, 1.0)]]
        tris, uvs = uv_triangles(np.array(uv, f32), shared=True)
        out.append((f"{width}x{height} FLT_MAX / width, subnormal and -0.0 uvs", tris, uvs, width, height))
    return out


# ---- d. long lists
RUNS = (1, 255, 256, 257, 4095, 4096, 4097)
LIST_LENGTH = 20001


def _small_triangles(m, seed):
    """``many_triangles`` drawn in about its centroid to a quarter: +-0.03 in uv, two texels of a 64 x 64 atlas; a centroid that
    lies off the atlas is moved onto it, so every one of them has a box"""
    t = many_triangles(m, seed).astype(f64)
    c = t.mean(1, keepdims=True)
    return (np.clip(c, 0.06, 0.94) + 0.25 * (t - c)).astype(f32)


def _zero_unit(m):
    """m triangles without units under any mesh filter: no uv area (one uv three times), a NaN uv, wholly outside the atlas"""
    kinds = np.array([[(0.3, 0.3), (0.3, 0.3), (0.3, 0.3)], [(np.nan, 0.5), (0.6, 0.5), (0.5, 0.6)], [(1.2, 1.3), (1.9, 1.2), (1.5, 1.8)]], f32)
    return kinds[np.arange(m) % 3]


def _list_case(name, parts):
    """parts: (uv triangles, is a run) in order; the triangles outside the runs belong to mesh 1 in stretches of 50 out of every
    250, so that under ``mesh = 0`` the runs grow and new ones appear, and to mesh 0 otherwise"""
    uv = np.concatenate([p for p, _ in parts])
    run = np.concatenate([np.full(len(p), r) for p, r in parts])
    meshes = np.where(~run & ((np.arange(len(uv)) // 50) % 5 == 4), 1, 0)
    assert len(uv) == LIST_LENGTH
    tris, uvs = uv_triangles(uv, meshes)
    return name, tris, uvs, 64, 64


def long_lists():
    """Reaches rocPRIM's multi-block scan with 64-bit counts and ``k_lm_cover``'s search of it.  gfx950 has no tuned entry in
    rocprim/device/detail/config/device_scan.hpp, so the scan runs ``default_scan_config_base``
    (rocprim/device/detail/device_config_helper.hpp): 256 threads with max(1, 16 / (sizeof(value) / 4)) = 8 items each for an
    8-byte count, 2048 items per block.  The 20 002 counts of these lists take ten blocks, and a run of 4095 or more zero counts
    spans at least one whole block.  Three lists of 20 001 triangles on a 64 x 64 atlas: two-texel triangles with runs of 1, 255,
    256, 257, 4095, 4096 and 4097 zero-unit triangles between them (no uv area, a NaN uv, wholly outside; and another mesh, which
    lengthens the runs under ``mesh = 0``), one list beginning with its longest run and one ending with it; and a list of which
    the last triangle alone has units."""
    real = _small_triangles(LIST_LENGTH - sum(RUNS), seed=23)
    cuts = np.linspace(0, len(real), len(RUNS) + 1).astype(int)
    segments = [real[cuts[k]:cuts[k + 1]] for k in range(len(RUNS))]
    order = (4097, 1, 255, 256, 257, 4095, 4096)
    begins = [p for r, s in zip(order, segments) for p in ((_zero_unit(r), True), (s, False))]
    ends = [p for r, s in zip(order[::-1], segments) for p in ((s, False), (_zero_unit(r), True))]
    alone = [(_zero_unit(LIST_LENGTH - 1), True), (real[:1], False)]
    return [_list_case("begins with a run", begins), _list_case("ends with a run", ends), _list_case("the last alone has units", alone)]


# ---- e. atlas shapes
SHAPES = ((1, 70001), (70001, 1), (1, 16384), (16384, 1), (8, 1), (9, 9), (263, 7))


def atlas_shapes():
    """Reaches the launch and box arithmetic at atlases that are one row or one column longer than any launch block (256 lanes,
    8 x 8 tiles), at one tile and one tile plus a texel, and at 263 x 7 with its last tile column seven wide under a single tile
    row: the slivers of family a scaled to the atlas, all five slopes inside and clamped, and behind them -- the highest index --
    a triangle over the whole atlas, which owns what they leave.  1 x 70001 and 70001 x 1 are past ``abi.LIGHTMAP_MAX_SIDE``:
    the model takes them and is held to exact arithmetic there, the entry points refuse them, and 1 x 16384 and 16384 x 1, the
    longest row and column the ABI accepts, stand beside them for the device."""
    out = []
    for width, height in SHAPES:
        tri = [t for slope, outside in itertools.product(SLOPES, (False, True)) for t in _sliver_set(width, height, slope, outside)]
        tri.append(((-1.0 * width, -1.0 * height), (-1.0 * width, 3.0 * height), (3.0 * width, -1.0 * height)))
        out.append(case(f"{width}x{height}", tri, width, height))
    return out


# ---- g. surfels out of range
def surfels_out_of_range():
    """Reaches ``k_lm_surfels`` where ``(v0 + u e1) + v e2`` leaves the finite range: positions of +-3e38 with mixed signs, so
    that the prepared e1 or e2 is infinite and u e1 is +-inf or, at u = 0, a NaN; a position component that is infinite; one that
    is a NaN.  The uvs are finite and plain: two triangles that tile a 9 x 9 and a 33 x 31 atlas."""
    uv = [[(0.0, 0.0), (1.0, 0.0), (0.0, 1.0)], [(1.0, 0.0), (1.0, 1.0), (0.0, 1.0)]]
    positions = {
        "3e38 of mixed sign": [((3e38, -3e38, 1.0), (-3e38, 3e38, 2.0), (3e38, 3e38, -3e38)), ((-3e38, 1.0, 3e38), (3e38, 2.0, -3e38), (1e38, -3e38, 3e38))],
        "3e38 of one sign": [((3e38, 3e38, 3e38), (3.4e38, 1e38, 3e38), (1e38, 3.4e38, 2e38)), ((-3e38, -3e38, -3e38), (-1e38, -3.4e38, -3e38), (-3.4e38, -1e38, -2e38))],
        "an infinite component": [((np.inf, 0.0, 1.0), (1.0, 2.0, 3.0), (2.0, 1.0, 0.5)), ((0.0, 1.0, 2.0), (1.0, -np.inf, 3.0), (2.0, 1.0, np.inf))],
        "a NaN component": [((np.nan, 0.0, 1.0), (1.0, 2.0, 3.0), (2.0, 1.0, 0.5)), ((0.0, 1.0, 2.0), (1.0, 2.0, 3.0), (2.0, np.nan, 0.5))],
    }
    out = []
    for (name, pos), (width, height) in itertools.product(positions.items(), ((9, 9), (33, 31))):
        tris, uvs = uv_triangles(np.array(uv, f32), shared=True)
        p = np.array(pos, f32)
        tris["v0"], tris["v1"], tris["v2"] = p[:, 0], p[:, 1], p[:, 2]
        out.append((f"{width}x{height} {name}", tris, uvs, width, height))
    return out


# ---- f. resolve records
WEIGHTS = np.array([PAYLOAD_NAN, INF, -INF, -1.0, -0.0, 0.0, SUB_MIN, FLT_MIN, 1.0, 2.0 ** 24, FLT_MAX], f32)
COLOURS = np.array([np.nan, INF, -INF, FLT_MAX, -FLT_MAX, -1.0, -0.0, SUB_MIN, 1.0], f32)
WEIGHTS.view(u32)[0] = 0x7FA12345   # (the list went through float64, which quiets a signalling payload)
RESOLVE_SHAPES = ((1, 1), (2, 2), (3, 3), (9, 1), (1, 9), (17, 13))


def _sums(width, height):
    return np.zeros(width * height, dtype=abi.RADIANCE)


def resolve_records():
    """(name, sums, width, height) for ``rb_lightmap_resolve``.  Reaches ``k_lm_resolve``'s ``w > 0`` at every kind of weight and
    the divisions at every kind of colour: all 99 pairs of ``WEIGHTS`` and ``COLOURS`` once, two texels apart on a 17 x 13 map, so
    that the fill adds what the pairs left (NaN, +-inf, -0.0).  Reaches ``k_lm_dilate``'s border: a one-texel chart in each corner
    and on each edge of an otherwise empty 1 x 1 ... 17 x 13 map -- every texel of column 0 computes ``x + (uint32_t)(-1)`` and
    must take nothing from the far side, where in these maps the only filled texel lies.  And the eight-neighbour sum past
    FLT_MAX: to +inf, to -inf, and back from it."""
    out = []
    s = _sums(17, 13)
    for k, (w, c) in enumerate(itertools.product(WEIGHTS, COLOURS)):
        s["weight"][2 * k] = w
        s["sum"][2 * k] = (c, f32(1.0), -c)
    out.append(("every pair of a weight and a colour", s, 17, 13))
    for width, height in RESOLVE_SHAPES:
        spots = sorted({(x, y) for x in {0, width // 2, width - 1} for y in {0, height // 2, height - 1}} - ({(width // 2, height // 2)} if min(width, height) > 2 else set()))
        for x, y in spots:
            s = _sums(width, height)
            s[y * width + x] = ((3.0, 1.5, 0.75), 3.0)
            out.append((f"{width}x{height} one texel at ({x}, {y})", s, width, height))
        out.append((f"{width}x{height} empty", _sums(width, height), width, height))
    for name, values in (("to +inf", [FLT_MAX / 2] * 8), ("to -inf", [-FLT_MAX / 2] * 8), ("from +inf by -FLT_MAX", [FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, 1, 1, 1, 1]),
                         ("inf - inf", [FLT_MAX, FLT_MAX, 1, -FLT_MAX, -FLT_MAX, -FLT_MAX, 1, 1])):
        s = _sums(3, 3)
        for (dx, dy), v in zip(lightmap.NEIGHBOURS, values):
            s[(1 + dy) * 3 + 1 + dx] = ((v, -f32(v), f32(v) / 4), 1.0)
        out.append((f"3x3 neighbours sum {name}", s, 3, 3))
    return out


FAMILIES = {"a slivers": slivers, "b tile corners": tile_corner_edges, "c far corners": far_corners, "d long lists": long_lists,
            "e atlas shapes": atlas_shapes, "g surfels out of range": surfels_out_of_range}
NO_NAN_FAMILIES = ("a slivers", "b tile corners", "d long lists", "e atlas shapes")


@functools.lru_cache(maxsize=None)
def cases(family):
    return FAMILIES[family]() if family != "f resolve records" else resolve_records()


@functools.lru_cache(maxsize=None)
def model(family, index, mesh=None, flip=False):
    """(abi.SURFEL[], owners) of case ``index`` of ``family`` from ``lightmap.surfels``; read-only, shared by every test"""
    _, tris, uvs, width, height = cases(family)[index]
    surf, own = lightmap.surfels(tris, uvs, width, height, mesh=mesh, flip=flip)
    surf.setflags(write=False)
    own.setflags(write=False)
    return surf, own
