"""The numpy model of direct light at surface points (csrc/rb_direct.hip): the same binary32 operations
in the same order, so ``scene_emitters`` equals ``rb_scene_emitters``, ``rays`` equals ``rb_light_rays`` and ``fold`` the sums
of ``rb_direct_light`` bit for bit.

``scene_emitters``  abi.EMITTER[] of a scene: its emissive triangles, then spheres, then lights, each in ascending order
``emitter_records`` the records of given triangles and spheres, whether or not they would qualify (a table of the caller's own)
``qualifies``       which of such records are emitters
``draws``           what the generator draws for every (surfel, sample) item: three numbers, always
``pick``            the emitter an item's first draw picks
``emitter_weights``, ``emitter_cdf``, ``pick_cdf``  the pick weighted by a table (section 23): the power of every record, the
                    quantised inclusive table ``rb_emitter_cdf`` makes of them, and the record an item's first draw picks from a table
``emitter_bounds``, ``grid_weights``, ``emitter_grid_cdf``, ``grid_cell``  the pick per grid cell (section 24): a sphere about
                    every record, its weight in every cell, the tables ``rb_emitter_grid_cdf`` makes -- one row per cell --, and
                    the row a surfel's position searches
``count``, ``tally``, ``seen_share``  the tables that learn visibility (section 25): the count of shadow rays tried and seen per
                    (cell, emitter) given the result bytes, and the factor a tally puts on a weight; ``grid_weights`` and
                    ``emitter_grid_cdf`` take a tally and a prior
``barycentrics``, ``points``  the point an item's second and third draws make on its emitter, and the emitter's normal there
``rays``          (origins, directions, bounds, contributions) of the items: what ``rb_light_rays`` returns -- with ``cdf``,
                    what ``rb_light_rays_cdf`` returns; with ``grid``, what ``rb_light_rays_grid`` returns
``fold``            abi.RADIANCE[m] from the contributions and the any-hit bytes of the items' shadow rays
"""
import numpy as np

from . import abi
from .camera import _unit, pcg, random_float, sincos_turn

f32, u32, u64 = np.float32, np.uint32, np.uint64
INV_PI = f32(0.318309886)
FOUR_PI = f32(12.566371)
KINDS = (abi.HIT_TRIANGLE, abi.HIT_SPHERE, abi.HIT_LIGHT)


def _dot(a, b):
    return ((a[..., 0] * b[..., 0]).astype(f32) + (a[..., 1] * b[..., 1]).astype(f32)).astype(f32) + (a[..., 2] * b[..., 2]).astype(f32)


def _cross(a, b):
    """each component two multiplies and one subtraction"""
    return np.stack([(a[..., 1] * b[..., 2]).astype(f32) - (a[..., 2] * b[..., 1]).astype(f32),
                     (a[..., 2] * b[..., 0]).astype(f32) - (a[..., 0] * b[..., 2]).astype(f32),
                     (a[..., 0] * b[..., 1]).astype(f32) - (a[..., 1] * b[..., 0]).astype(f32)], axis=-1).astype(f32)


def emitter_records(kind, prim, a, b, c, emissive):
    """abi.EMITTER[n] from per-record arrays; the area by the table's rule: half the length of cross(b, c) for a triangle,
    12.566371 (radius radius) with radius = b.x otherwise"""
    n = len(np.asarray(prim).reshape(-1))
    e = np.zeros(n, dtype=abi.EMITTER)
    e["kind"], e["prim"] = kind, prim
    e["a"], e["b"], e["c"], e["emissive"] = (np.asarray(x, f32).reshape(n, 3) for x in (a, b, c, emissive))
    with np.errstate(all="ignore"):
        cr = _cross(e["b"], e["c"])
        tri = (f32(0.5) * np.sqrt(_dot(cr, cr), dtype=f32)).astype(f32)
        sph = (FOUR_PI * (e["b"][:, 0] * e["b"][:, 0]).astype(f32)).astype(f32)
    e["area"] = np.where(e["kind"] == abi.HIT_TRIANGLE, tri, sph)
    return e


def qualifies(e):
    """which records of a table built by the table's rule are emitters (section 21.1); a sphere's radius is b.x"""
    with np.errstate(all="ignore"):
        fin = np.isfinite(e["emissive"]).all(1) & np.isfinite(e["a"]).all(1) & np.isfinite(e["b"]).all(1) & np.isfinite(e["c"]).all(1)
        ok = fin & (e["emissive"].max(1) > 0) & np.isfinite(e["area"]) & (e["area"] > 0)
        return ok & ((e["kind"] == abi.HIT_TRIANGLE) | (e["b"][:, 0] > 0))


def scene_emitters(scene, triangle_count=None, spheres_count=None):
    """abi.EMITTER[] of a scenes.Scene as an engine that has just taken it sees it.  ``triangle_count`` / ``spheres_count``:
    the counts of a later update that kept the arrays (uniforms.bvh_triangle_count / spheres_count, clamped to the arrays as the
    engine clamps them); by default every triangle and sphere counts."""
    tris, meshes = scene.bvh_triangles, scene.meshes
    nt = len(tris) if triangle_count is None else min(int(triangle_count), len(tris))
    ns = len(scene.spheres) if spheres_count is None else min(int(spheres_count), len(scene.spheres))
    t = tris[:nt]
    t = t[t["mesh_index"] < len(meshes)]
    prim_t = np.nonzero(tris[:nt]["mesh_index"] < len(meshes))[0]
    em_t = meshes["material"]["emissive"][t["mesh_index"]] if len(t) else np.zeros((0, 3), f32)
    if int(scene.uniforms["color_hash_enabled"][0]) != 0:
        em_t = np.zeros_like(em_t)   # a triangle hit under the colour hash reports no emission
    parts = [emitter_records(abi.HIT_TRIANGLE, prim_t, t["v0"], (t["v1"] - t["v0"]).astype(f32), (t["v2"] - t["v0"]).astype(f32), em_t)]
    for kind, rec in ((abi.HIT_SPHERE, scene.spheres[:ns]), (abi.HIT_LIGHT, scene.lights)):
        b = np.zeros((len(rec), 3), f32)
        b[:, 0] = rec["radius"]
        parts.append(emitter_records(kind, np.arange(len(rec)), rec["center"], b, np.zeros((len(rec), 3), f32), rec["material"]["emissive"]))
    e = np.concatenate(parts)
    return np.ascontiguousarray(e[qualifies(e)])


def draws(m, first_sample, samples, seeds=None):
    """What the generator draws for the items (surfel, sample) of ``m`` surfels, surfel-major: dict of ``u0``, ``u1``, ``u2``
    and ``surfel`` (the item's surfel).  ``seeds``: the surfels' ids, by default their indices -- rb_trace_rays' rule."""
    sid = np.arange(m, dtype=u64) if seeds is None else np.asarray(seeds, u32).reshape(-1).astype(u64)
    if len(sid) != m:
        raise ValueError("seeds: one id per surfel is needed")
    surfel = np.repeat(np.arange(m, dtype=np.int64), samples)
    k = np.tile(np.arange(samples, dtype=u64), m)
    hs = pcg((u64(first_sample) + k) & u64(0xFFFFFFFF))
    seed = pcg((sid[surfel] + hs.astype(u64)) & u64(0xFFFFFFFF))
    seed, u0 = random_float(seed)
    seed, u1 = random_float(seed)
    seed, u2 = random_float(seed)
    return dict(u0=u0, u1=u1, u2=u2, surfel=surfel)


def pick(u0, n_emit):
    """j = min(uint(u0 float(N)), N - 1)"""
    return np.minimum((np.asarray(u0, f32) * f32(n_emit)).astype(f32).astype(u32), u32(n_emit - 1)).astype(np.int64)


MAX_WEIGHT = f32(3.4028235e38)
MAX_CDF = 1 << 24


def emitter_weights(em):
    """p[n] float32, the pick weight of every record by its power (section 23.1): min(m area, 3.4028235e38) with m the largest
    component of ``emissive`` when the record is good in section 21.1's sense, m > 0 and the product is > 0; else 0"""
    e = np.asarray(em, dtype=abi.EMITTER).reshape(-1)
    with np.errstate(all="ignore"):
        good = (np.isfinite(e["a"]).all(1) & np.isfinite(e["b"]).all(1) & np.isfinite(e["c"]).all(1) & np.isfinite(e["emissive"]).all(1)
                & np.isfinite(e["area"]) & (e["area"] > 0) & np.isin(e["kind"], KINDS))
        m = np.where(good, e["emissive"].max(1), f32(0)).astype(f32)
        p = np.minimum((m * e["area"]).astype(f32), MAX_WEIGHT).astype(f32)
        return np.where(good & (m > 0) & (p > 0), p, f32(0)).astype(f32)


def cdf_scale(n):
    """S = 2^(24 - L), L the smallest integer with 2^L >= n"""
    return 1 << (24 - max(int(n) - 1, 0).bit_length())


def emitter_cdf(em):
    """uint32[n], the quantised inclusive table by power (section 23.1): q_j = max(1, uint((p_j / pmax) float(S))) for p_j > 0,
    else 0; cdf[j] = q_0 + ... + q_j.  What rb_emitter_cdf returns."""
    p = emitter_weights(em)
    if len(p) > abi.MAX_EMITTERS:
        raise ValueError("at most 2^24 emitters are taken")
    if len(p) == 0:
        return np.zeros(0, u32)
    pmax = p.max()
    with np.errstate(all="ignore"):
        r = ((p / pmax).astype(f32) * f32(cdf_scale(len(p)))).astype(f32)
        q = np.where(p > 0, np.maximum(np.where(p > 0, r, f32(0)).astype(u32), u32(1)), u32(0)).astype(u32)
    return np.cumsum(q, dtype=u64).astype(u32)


def search_cdf(t, cdf):
    """j of every t by the halving search of section 23.1, literally: lo = 0, len = N; while len > 1: half = len >> 1; if
    cdf[lo + half - 1] <= t: lo += half, len -= half; else len = half.  The first j with cdf[j] > t in a non-decreasing table;
    for any contents every index read is inside the table (checked here)."""
    cdf = np.asarray(cdf, u32).reshape(-1)
    t = np.asarray(t, u32).reshape(-1)
    n = len(cdf)
    lo = np.zeros(len(t), np.int64)
    ln = np.full(len(t), n, np.int64)
    while (ln > 1).any():
        go = ln > 1
        half = ln >> 1
        idx = np.where(go, lo + half - 1, 0)
        if not ((idx >= 0) & (idx < n)).all():
            raise IndexError("the search left the table")
        up = go & (cdf[idx] <= t)
        lo = np.where(up, lo + half, lo)
        ln = np.where(up, ln - half, np.where(go, half, ln))
    return lo


def pick_cdf(u0, cdf):
    """(j, q, Q) of the items' first draws and an inclusive table of any contents (section 23.1): Q = cdf[N - 1];
    t = min(uint(u0 float(Q)), Q - 1); j by the halving search, which reads inside the table whatever it holds;
    q = cdf[j] - cdf[j - 1], wrapping.  Q == 0 or Q > 2^24: no pick is made and every q is 0 (a dark item)."""
    cdf = np.asarray(cdf, u32).reshape(-1)
    u0 = np.asarray(u0, f32).reshape(-1)
    n = len(cdf)
    if n == 0:
        raise ValueError("an empty table picks nothing")
    Q = int(cdf[n - 1])
    j = np.zeros(len(u0), np.int64)
    if Q == 0 or Q > MAX_CDF:
        return j, np.zeros(len(u0), u32), Q
    t = np.minimum((u0 * f32(Q)).astype(f32).astype(u32), u32(Q - 1))
    j = search_cdf(t, cdf)
    below = np.where(j > 0, cdf[np.maximum(j - 1, 0)], u32(0)).astype(u32)
    q = (cdf[j].astype(u64) - below.astype(u64)).astype(u32)   # wrapping
    return j, q, Q


def _gt(x, y):
    """max(x, y) as section 24 has it: x > y ? x : y"""
    return np.where(x > y, x, y).astype(f32)


def _grid(grid):
    """(origin (3,) float32, step (3,) float32, counts (3,) int64, rows) of an abi.PROBE_GRID whose counts count cells"""
    g = np.asarray(grid, dtype=abi.PROBE_GRID).reshape(())
    cnt = g["counts"].astype(np.int64)
    return g["origin"].astype(f32), g["step"].astype(f32), cnt, int(cnt[0] * cnt[1] * cnt[2])


def emitter_bounds(em):
    """(ce (n, 3), re (n,)) float32, a sphere that holds every record (section 24).  A triangle: ce = a + ((b + c) 0.33333334),
    re = sqrt of the largest of |a - ce|^2, |(a + b) - ce|^2, |(a + c) - ce|^2; any other kind: ce = a, re = |b.x|."""
    e = np.asarray(em, dtype=abi.EMITTER).reshape(-1)
    a, b, c = e["a"].astype(f32), e["b"].astype(f32), e["c"].astype(f32)
    with np.errstate(all="ignore"):
        ce = (a + ((b + c).astype(f32) * f32(0.33333334)).astype(f32)).astype(f32)
        ls = []
        for corner in (a, (a + b).astype(f32), (a + c).astype(f32)):
            v = (corner - ce).astype(f32)
            ls.append(_dot(v, v).astype(f32))
        re = np.sqrt(_gt(_gt(ls[0], ls[1]), ls[2]), dtype=f32)
    tri = e["kind"] == abi.HIT_TRIANGLE
    return np.where(tri[:, None], ce, a).astype(f32), np.where(tri, re, np.abs(b[:, 0])).astype(f32)


def grid_centres(grid):
    """(rows, 3) float32: cc = origin + (float(i) + 0.5) step of every cell, row = (iz ny + iy) nx + ix"""
    org, step, cnt, rows = _grid(grid)
    r = np.arange(rows, dtype=np.int64)
    idx = np.stack([r % cnt[0], (r // cnt[0]) % cnt[1], r // (cnt[0] * cnt[1])], axis=1)
    with np.errstate(all="ignore"):
        return (org[None, :] + ((idx.astype(f32) + f32(0.5)).astype(f32) * step[None, :]).astype(f32)).astype(f32)


def _prior(prior):
    a = f32(prior)
    if not (np.isfinite(a) and 0 < a <= f32(abi.MAX_PRIOR)):
        raise ValueError("prior: finite, above 0 and at most 16777216")
    return a


def seen_share(tally, prior):
    """f float32 of every abi.GRID_TALLY record (section 25): t = tried, s = min(seen, tried), f = (float(s) + a) / (float(t) + a);
    in [0, 1] and never a NaN for a finite prior a with 0 < a <= 16777216"""
    t = np.asarray(tally, dtype=abi.GRID_TALLY)
    a = _prior(prior)
    s = np.minimum(t["seen"], t["tried"])
    with np.errstate(all="ignore"):
        return ((s.astype(f32) + a).astype(f32) / (t["tried"].astype(f32) + a).astype(f32)).astype(f32)


def grid_weights(em, grid, tally=None, prior=None):
    """w (rows, n) float32 of section 24: p_j / max(d2, (re + hd)^2), at most 3.4028235e38, and 0 where p_j is 0; never a NaN.
    ``tally`` (abi.GRID_TALLY[rows * n]) and ``prior``: w' = w f of section 25, f by ``seen_share``; None: section 24 untouched"""
    p = emitter_weights(em)
    ce, re = emitter_bounds(em)
    _, step, _, rows = _grid(grid)
    cc = grid_centres(grid)
    with np.errstate(all="ignore"):
        hd = np.sqrt((f32(0.25) * (((step[0] * step[0]).astype(f32) + (step[1] * step[1]).astype(f32)).astype(f32)
                                   + (step[2] * step[2]).astype(f32)).astype(f32)).astype(f32), dtype=f32)
        v = (ce[None, :, :] - cc[:, None, :]).astype(f32)
        d2 = _dot(v, v).astype(f32)
        r0 = (re + hd).astype(f32)
        fl = np.broadcast_to((r0 * r0).astype(f32)[None, :], d2.shape)
        x = (p[None, :] / _gt(d2, fl)).astype(f32)
        w = np.where(x < MAX_WEIGHT, x, MAX_WEIGHT).astype(f32)
    w = np.where(p[None, :] > 0, w, f32(0)).astype(f32).reshape(rows, len(p))
    if tally is None:
        return w
    t = np.asarray(tally, dtype=abi.GRID_TALLY).reshape(-1)
    if len(t) != rows * len(p):
        raise ValueError("tally: one record per cell and emitter is needed")
    with np.errstate(all="ignore"):
        return (w * seen_share(t, prior).reshape(rows, len(p))).astype(f32)


def emitter_grid_cdf(em, grid, tally=None, prior=1.0):
    """uint32[rows * n], the tables of section 24, row r at [r n, (r + 1) n): q = max(1, uint((w / wmax_r) float(S))) for
    p_j > 0 -- 1 where the row's largest weight is 0 --, else 0, summed inclusively along the row.  What rb_emitter_grid_cdf
    returns.  ``tally``: the learned tables of section 25 -- the same with w' = w f, what rb_emitter_grid_learned returns."""
    p = emitter_weights(em)
    n = len(p)
    rows = _grid(grid)[3]
    if n > abi.MAX_EMITTERS or rows * max(n, 1) > abi.MAX_GRID_ENTRIES:
        raise ValueError("at most 2^24 emitters and 2^26 entries are taken")
    if n == 0:
        return np.zeros(0, u32)
    w = grid_weights(em, grid) if tally is None else grid_weights(em, grid, tally, prior)
    wmax = w.max(axis=1)[:, None]
    with np.errstate(all="ignore"):
        r = ((w / wmax).astype(f32) * f32(cdf_scale(n))).astype(f32)
        some = np.broadcast_to(wmax > 0, w.shape)
        q = np.where(some, np.maximum(np.where(some, r, f32(0)).astype(u32), u32(1)), u32(1))
        q = np.where(p[None, :] > 0, q, u32(0)).astype(u32)
    return np.cumsum(q, axis=1, dtype=u64).astype(u32).reshape(-1)


def grid_cell(pos, grid):
    """row (m,) int64 of the cell each of (m, 3) finite positions searches (section 24): per axis f = (pos - origin) / step,
    i = min(uint(max(f, 0)), count - 1), truncating and saturating; the nearest cell for a point outside the grid"""
    org, step, cnt, _ = _grid(grid)
    pos = np.asarray(pos, f32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        f = ((pos - org[None, :]).astype(f32) / step[None, :]).astype(f32)
        f = np.where(f > 0, f, f32(0)).astype(f32)
        big = ~(f < f32(4294967296.0))
        i = np.minimum(np.where(big, f32(0), f).astype(np.int64), (cnt - 1)[None, :])
        i = np.where(big, (cnt - 1)[None, :], i)
    return (i[:, 2] * cnt[1] + i[:, 1]) * cnt[0] + i[:, 0]


def pick_grid(u0, rows, tables, n_emit):
    """(j, q, Q) per item of ``pick_cdf`` in the row each item searches; an item whose row is < 0 makes no pick (q = 0)"""
    tables = np.asarray(tables, u32).reshape(-1, n_emit)
    u0 = np.asarray(u0, f32).reshape(-1)
    j, q, Q = np.zeros(len(u0), np.int64), np.zeros(len(u0), u32), np.zeros(len(u0), np.int64)
    for r in np.unique(rows[rows >= 0]):
        sel = rows == r
        j[sel], q[sel], Q[sel] = pick_cdf(u0[sel], tables[r])
    return j, q, Q


def count(entries, index, bound, occl, into=None):
    """abi.GRID_TALLY[entries], the count of section 25 over items whose record is ``index`` (row n + j), whose stored bound is
    ``bound`` and whose result byte is ``occl``: an item with bound > 0 adds 1 to ``tried`` of its record, and 1 to ``seen`` if
    its byte is abi.OCCL_VISIBLE; any other item counts nothing.  uint32 sums that wrap, on top of ``into`` (not changed)."""
    out = np.zeros(entries, dtype=abi.GRID_TALLY) if into is None else np.array(into, dtype=abi.GRID_TALLY).reshape(-1)
    if len(out) != entries:
        raise ValueError("into: one record per cell and emitter is needed")
    index = np.asarray(index, np.int64).reshape(-1)
    counted = np.asarray(bound, f32).reshape(-1) > 0
    vis = np.asarray(occl, np.uint8).reshape(-1) == abi.OCCL_VISIBLE
    if not (len(index) == len(counted) == len(vis)):
        raise ValueError("index, bound, occl: one entry per item is needed")
    if entries == 0:
        return out
    tried = np.bincount(index[counted], minlength=entries).astype(u64)
    seen = np.bincount(index[counted & vis], minlength=entries).astype(u64)
    out["tried"] = ((out["tried"].astype(u64) + tried) & u64(0xFFFFFFFF)).astype(u32)
    out["seen"] = ((out["seen"].astype(u64) + seen) & u64(0xFFFFFFFF)).astype(u32)
    return out


def tally(emitters, surf, first_sample, samples, grid, occl, tables=None, seeds=None, offset=1e-3, shorten=1e-3, into=None):
    """abi.GRID_TALLY[rows * n] after a call of rb_direct_light_grid_tally whose shadow rays -- ``rays(grid=grid, tables=tables)``,
    surfel-major -- got the bytes ``occl`` from rb_occluded, on top of ``into`` (None: zeros): every item's row and pick as the
    generator has them, counted by ``count``"""
    em = np.asarray(emitters, dtype=abi.EMITTER).reshape(-1)
    surf = np.asarray(surf, dtype=abi.SURFEL).reshape(-1)
    n_emit, rows = len(em), _grid(grid)[3]
    if n_emit == 0 or len(surf) == 0:
        return count(rows * n_emit, np.zeros(0, np.int64), np.zeros(0, f32), np.zeros(0, np.uint8), into)
    tables = emitter_grid_cdf(em, grid) if tables is None else np.asarray(tables, u32).reshape(-1)
    bound = rays(em, surf, first_sample, samples, seeds, offset, shorten, grid=grid, tables=tables)[2]
    dr = draws(len(surf), first_sample, samples, seeds)
    pos = surf["pos"].astype(f32)
    fin = np.isfinite(pos).all(1)
    row = grid_cell(np.where(fin[:, None], pos, f32(0)), grid)[dr["surfel"]]
    j = pick_grid(dr["u0"], np.where(bound > 0, row, -1), tables, n_emit)[0]
    return count(rows * n_emit, row * n_emit + j, bound, occl, into)


def barycentrics(u1, u2):
    """(bu, bv) of a triangle's point: su = sqrt(u1), bv = u2 su, bu = su - bv; the point is (a + bu b) + bv c"""
    u1, u2 = np.asarray(u1, f32), np.asarray(u2, f32)
    su = np.sqrt(u1, dtype=f32)
    bv = (u2 * su).astype(f32)
    return (su - bv).astype(f32), bv


def points(E, u1, u2):
    """(Q, ne) of the emitters ``E`` (one record per item) and the items' second and third draws: the sampled point and the
    emitter's normal there -- a triangle's normalised as rb_cast_rays normalises, a sphere's as drawn"""
    a, b, c = E["a"], E["b"], E["c"]
    u1, u2 = np.asarray(u1, f32), np.asarray(u2, f32)
    with np.errstate(all="ignore"):
        bu, bv = barycentrics(u1, u2)
        q_tri = ((a + (bu[:, None] * b).astype(f32)).astype(f32) + (bv[:, None] * c).astype(f32)).astype(f32)
        ne_tri = _unit(_cross(b, c))
        # a sphere or a light: rb_probe_rays' lines
        s, cz = sincos_turn((u1 * f32(2.0) - f32(1.0)).astype(f32))
        z = (f32(1.0) - (u2 + u2).astype(f32)).astype(f32)
        r = np.sqrt((f32(1.0) - (z * z).astype(f32)).astype(f32), dtype=f32)
        ne_sph = np.stack([(r * cz).astype(f32), (r * s).astype(f32), z], axis=1)
        q_sph = (a + (b[:, 0:1] * ne_sph).astype(f32)).astype(f32)
    tri = (E["kind"] == abi.HIT_TRIANGLE)[:, None]
    return np.where(tri, q_tri, q_sph).astype(f32), np.where(tri, ne_tri, ne_sph).astype(f32)


def rays(emitters, surf, first_sample, samples, seeds=None, offset=1e-3, shorten=1e-3, cdf=None, grid=None, tables=None):
    """(origins (n, 3), directions (n, 3), bounds (n,), contributions (n, 4)) of the items (surfel, sample), surfel-major -- item
    i * samples + k is sample ``first_sample`` + k of ``surf[i]`` --: what rb_light_rays returns.  A lit item has a bound above
    0 and its unoccluded contribution; a dark one the bound 0 and +0 +0 +0; the fourth component is 1 for a valid item.  An
    invalid item (an invalid surfel, section 16.1) has its surfel's position as given and direction 0 0 0.
    ``cdf``: a uint32 table of pick weights, one inclusive entry per emitter (``emitter_cdf``, or any contents): what
    rb_light_rays_cdf returns (section 23) -- the pick by ``pick_cdf``, the factor float(Q) / float(q) in place of float(N); an
    item the table leaves without a pick is dark and has direction 0 0 0, as every item of an empty table.
    ``grid``: an abi.PROBE_GRID of cells: what rb_light_rays_grid returns (section 24) -- the same with every item searching the
    row of ``tables`` (uint32[rows * n_emit], any contents; None: ``emitter_grid_cdf``) that ``grid_cell`` gives its surfel."""
    em = np.asarray(emitters, dtype=abi.EMITTER).reshape(-1)
    n_emit = len(em)
    if n_emit > abi.MAX_EMITTERS:
        raise ValueError("at most 2^24 emitters are taken")
    surf = np.asarray(surf, dtype=abi.SURFEL).reshape(-1)
    pos = surf["pos"].astype(f32)
    dr = draws(len(surf), first_sample, samples, seeds)
    i = dr["surfel"]
    n = len(i)
    with np.errstate(all="ignore"):
        nrm = _unit(surf["normal"].astype(f32))
        px, py, pz = pos[:, 0], pos[:, 1], pos[:, 2]
        reach = np.sqrt((((px * px).astype(f32) + (py * py).astype(f32)).astype(f32) + (pz * pz).astype(f32)).astype(f32), dtype=f32)
        step = (f32(offset) * np.where(reach > f32(1.0), reach, f32(1.0)).astype(f32)).astype(f32)
        o = (pos + (step[:, None] * nrm).astype(f32)).astype(f32)
        ok = np.isfinite(pos).all(1) & np.isfinite(nrm).all(1) & (nrm != 0).any(1) & np.isfinite(o).all(1)
    valid = ok[i]
    org = o[i]
    org[~valid] = pos[i][~valid]
    d = np.zeros((n, 3), f32)
    tmax = np.zeros(n, f32)
    contrib = np.zeros((n, 4), f32)
    contrib[:, 3] = valid
    if n_emit == 0 or n == 0:
        return org, d, tmax, contrib
    with np.errstate(all="ignore"):
        if grid is not None:
            if cdf is not None:
                raise ValueError("cdf and grid: one pick at a time")
            tables = emitter_grid_cdf(em, grid) if tables is None else np.asarray(tables, u32).reshape(-1)
            if len(tables) != _grid(grid)[3] * n_emit:
                raise ValueError("tables: one entry per cell and emitter is needed")
            row = np.where(ok, grid_cell(np.where(ok[:, None], pos, f32(0)), grid), -1)[i]
            j, q, Q = pick_grid(dr["u0"], row, tables, n_emit)
            valid = valid & (q != 0)
            fn = (Q.astype(f32) / q.astype(f32)).astype(f32)
            E = em[j]
        elif cdf is None:
            fn = f32(n_emit)
            E = em[pick(dr["u0"], n_emit)]
        else:
            cdf = np.asarray(cdf, u32).reshape(-1)
            if len(cdf) != n_emit:
                raise ValueError("cdf: one entry per emitter is needed")
            j, q, Q = pick_cdf(dr["u0"], cdf)
            valid = valid & (q != 0)   # from here on: the items that have a pick
            fn = (f32(Q) / q.astype(f32)).astype(f32)
            E = em[j]
        area = E["area"]
        tri = E["kind"] == abi.HIT_TRIANGLE
        good = (np.isfinite(E["a"]).all(1) & np.isfinite(E["b"]).all(1) & np.isfinite(E["c"]).all(1) & np.isfinite(E["emissive"]).all(1)
                & np.isfinite(area) & (area > 0) & np.isin(E["kind"], KINDS))
        Q, ne = points(E, dr["u1"], dr["u2"])
        v = (Q - o[i]).astype(f32)
        d2 = _dot(v, v).astype(f32)
        dist = np.sqrt(d2, dtype=f32)
        dd = (v / dist[:, None]).astype(f32)
        cs = _dot(nrm[i], dd).astype(f32)
        ce = _dot(ne, dd).astype(f32)
        ce = np.where(tri, np.abs(ce), -ce).astype(f32)
        aimed = np.isfinite(dd).all(1) & (dd != 0).any(1)
        g = ((((cs * ce).astype(f32) * area).astype(f32) / d2).astype(f32) * fn).astype(f32)
        g = (g * INV_PI).astype(f32)
        lit3 = (E["emissive"] * g[:, None]).astype(f32)
        lit = valid & good & aimed & (cs > 0) & (ce > 0) & (d2 > 0) & np.isfinite(lit3).all(1)
        bound = (dist * (f32(1.0) - f32(shorten))).astype(f32)
    keep = valid & aimed
    d[keep] = dd[keep]
    tmax[lit] = bound[lit]
    contrib[lit, :3] = lit3[lit]
    return org, d, tmax, contrib


def fold(contrib, occl, samples):
    """abi.RADIANCE[m] of m * samples items, surfel-major: ``sum`` from +0, in ascending sample order, the contribution of
    every item whose byte is abi.OCCL_VISIBLE, one float32 add per component; ``weight`` the number of valid items."""
    c = np.asarray(contrib, f32).reshape(-1, samples, 4)
    seen = np.asarray(occl, np.uint8).reshape(-1, samples) == abi.OCCL_VISIBLE
    out = np.zeros(len(c), dtype=abi.RADIANCE)
    total = np.zeros((len(c), 3), f32)
    weight = np.zeros(len(c), f32)
    with np.errstate(all="ignore"):
        for k in range(samples):
            total = np.where(seen[:, k, None], (total + c[:, k, :3]).astype(f32), total)
            weight = (weight + c[:, k, 3]).astype(f32)
    out["sum"], out["weight"] = total, weight
    return out


def params(offset=1e-3, shorten=1e-3, mask=abi.MASK_ALL):
    """abi.LIGHT_PARAMS[1] of a call"""
    p = np.zeros(1, dtype=abi.LIGHT_PARAMS)
    p["offset"], p["shorten"], p["mask"] = offset, shorten, int(mask)
    return p
