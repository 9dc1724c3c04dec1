"""What the tests of the triangle sift share (tests/test_tri_filter_model.py on the CPU, tests/test_gpu_tri_filter.py and
tests/test_gpu_tri_filter_updates.py on the device): the float32 reference test of tools/margin_check.py, the table and region of
a node's list from the numpy model (renderbaby_amd/tri_filter_model.py), the accepted slots of a set of rays, the named
single-node scenes (`tables`) and the ray families, among them the rays aimed at where a conservative box test fails first
(`aimed_rays`)."""
import dataclasses
import functools
import importlib.util
import os

import numpy as np

from renderbaby_amd import abi, scenes
from renderbaby_amd import tri_filter_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SPP, DEPTH = 4, 8


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MC = _tool("margin_check")


def node_list(scene):
    """[first, end) of the list of a single-node scene's node, `end` clipped to the index array as prep_tri_filter clips it"""
    assert len(scene.bvh_nodes) == 1
    first, count = int(scene.bvh_nodes["first_primitive"][0]), int(scene.bvh_nodes["primitive_count"][0])
    return first, min(first + count, len(scene.bvh_indices))


def _list_of(scene, first, end, tri_count):
    end = len(scene.bvh_indices) if end is None else min(int(end), len(scene.bvh_indices))
    tri_count = len(scene.bvh_triangles) if tri_count is None else min(int(tri_count), len(scene.bvh_triangles))
    idx = np.asarray(scene.bvh_indices[first:end], np.int64)
    return idx, idx < tri_count


def _valid(scene, first=0, end=None, tri_count=None):
    """slot s of the list [first, end) is live iff bvh_indices[s] < bvh_triangle_count (shader.wgsl:336; k_prep_tris' `valid`)"""
    return _list_of(scene, first, end, tri_count)[1]


def _prepared(scene, first=0, end=None, tri_count=None):
    """the prepared triangles (v0, e1, e2 as k_prep_tris makes them) of the slots [first, end) of the index array, by default all
    of it; a dead slot's record is zero, as the device's is"""
    idx, valid = _list_of(scene, first, end, tri_count)
    t = scene.bvh_triangles[np.where(valid, idx, 0)] if len(scene.bvh_triangles) else np.zeros(len(idx), abi.GPU_TRIANGLE)
    live = valid[:, None]
    v0 = np.where(live, t["v0"].astype(F32), F32(0))
    return v0, np.where(live, t["v1"].astype(F32) - v0, F32(0)), np.where(live, t["v2"].astype(F32) - v0, F32(0))


def _scene_table(scene, origins=None, first=0, end=None, tri_count=None):
    """the table of the list [first, end) (by default the whole index array, every triangle the buffer holds live) and the region
    of a launch over it; `origins`: rays start there as if the camera did (their finite box joins).
    -> (groups, region, (v0, e1, e2, valid))"""
    v0, e1, e2 = _prepared(scene, first, end, tri_count)
    valid = _valid(scene, first, end, tri_count)
    assert len(v0) <= M.MAX_SLOTS
    groups, live, closed = M.build_table(v0, e1, e2, valid)
    cam = np.asarray(scene.uniforms["camera"]["pos"][0], np.float64)
    lo, hi = cam.copy(), cam.copy()
    for s in scene.spheres:
        r = abs(float(s["radius"])) * 1.0001
        lo, hi = np.minimum(lo, s["center"] - r), np.maximum(hi, s["center"] + r)
    if origins is not None:
        o = np.asarray(origins, np.float64)
        o = o[np.all(np.abs(o) < 1e6, axis=1)]
        lo, hi = np.minimum(lo, o.min(0)), np.maximum(hi, o.max(0))
    return groups, M.table_region(groups, lo, hi), (v0, e1, e2, valid)


def _accepted(tri, o, d):
    """bool [slots][rays]: the float32 reference test accepts; a dead slot (tri[3], where given) accepts nothing"""
    v0, e1, e2 = tri[:3]
    valid = tri[3] if len(tri) > 3 else np.ones(len(v0), bool)
    out = np.zeros((len(v0), o.shape[1]), bool)
    for k in range(len(v0)):
        if not valid[k]:
            continue
        with np.errstate(all="ignore"):   # (the families carry infinite and NaN components on purpose)
            ok, _, _ = MC.mt32(tuple(o), tuple(d), *(tuple(np.full(o.shape[1], a[k][i], F32) for i in range(3)) for a in (v0, e1, e2)))
        out[k] = ok
    return out


def _hold(scene_table, o, d, what):
    groups, reg, tri = scene_table
    o, d = np.ascontiguousarray(np.asarray(o, F32).T), np.ascontiguousarray(np.asarray(d, F32).T)
    cand, acc = M.candidate_mask(groups, reg, o, d), _accepted(tri, o, d)
    print(f"{what}: {o.shape[1]} rays, {int(acc.sum())} accepted hits, candidates per ray mean {cand.sum(0).mean():.2f} max {int(cand.sum(0).max())}")
    assert not (acc & ~cand).any(), (what, int((acc & ~cand).sum()))
    return cand, acc


def _unit(d):
    d = np.asarray(d, F32)
    with np.errstate(all="ignore"):
        return (d / np.sqrt((d * d).sum(1, dtype=F32))[:, None]).astype(F32)


def tiny_component_rays(n_per=24, seed=9):
    """Origins inside the Cornell box, directions with one or two components swept over the smallest normal exponents and the
    subnormals beside them (+-2^-149 .. 2^-100), the others of ordinary size -> (o [n][3], d [n][3]) float32.  1 / d_k is then
    finite and up to 2^126, or infinite."""
    rng = np.random.default_rng(seed)
    b = scenes.BOX
    lo, hi = np.array([b["x0"], b["y0"], b["z0"]]), np.array([b["x1"], b["y1"], b["z1"]])
    tiny = [s * m * 2.0 ** e for e in list(range(-149, -99, 2)) + [-127, -126, -125] for m in (1.0, 1.2, 1.9999999) for s in (1.0, -1.0)]
    O, D = [], []
    for t in tiny:
        for k in range(3):
            for two in (False, True):
                d = rng.normal(size=(n_per, 3))
                d[:, k] = t
                if two:
                    d[:, (k + 1) % 3] = -t
                O.append(lo + rng.random((n_per, 3)) * (hi - lo))
                D.append(d)
    o, d = np.concatenate(O).astype(F32), np.concatenate(D).astype(F32)
    keep = np.abs(d).max(1) > 0.05     # (an ordinary component beside the tiny ones)
    return o[keep], d[keep]


# ----------------------------------------------------------------------------------- the scenes ---
def _soup(n, w, h, seed=7, extra=(), scale=1.0, shift=(0.0, 0.0, 0.0)):
    """n ordinary triangles (pairs of them quads, the rest singles) scattered in front of the camera in one node, two spheres
    and a sky, so that paths bounce between triangles, spheres and nothing; `extra`: triangles appended as they are;
    `scale`, `shift`: triangles, spheres and camera scaled about the origin, then translated (in double, rounded once)"""
    rng = np.random.default_rng(seed + n)
    place = lambda p: tuple(np.asarray(p, np.float64) * scale + np.asarray(shift, np.float64))
    tris = []
    while len(tris) < n:
        c = rng.uniform((-3, 0.5, -7), (3, 5.5, -2))
        a, b = rng.normal(size=3), rng.normal(size=3)
        a *= rng.uniform(0.4, 1.6) / np.linalg.norm(a)
        b -= a * (a @ b) / (a @ a)
        b *= rng.uniform(0.4, 1.6) / np.linalg.norm(b)
        q = scenes._quad(place(c - a - b), place(c + a - b), place(c + a + b), place(c - a + b))
        tris += q if n - len(tris) >= 2 and rng.uniform() < 0.7 else q[:1]
    tris = tris[:n] + list(extra)
    sp = np.zeros(2, dtype=abi.SPHERE)
    sp[0]["center"], sp[0]["radius"] = place((-1.2, 1.0, -3.0)), 0.8 * scale
    sp[0]["material"] = scenes.sphere_material("mirror", (0.9, 0.9, 0.9))
    sp[1]["center"], sp[1]["radius"] = place((1.4, 2.5, -4.0)), 0.7 * scale
    sp[1]["material"] = scenes.sphere_material("plastic", (0.3, 0.6, 0.9))
    u = scenes.make_uniforms(w, h, SPP, DEPTH, cam_pos=place((0, 3, 5)), cam_dir=(0, 0, -1), ground_enabled=0, sky=(0.5, 0.7, 1.0))
    half = len(tris) // 2
    groups = [(scenes.material(**scenes.KHAKI), tris[:half]), (scenes.material(**scenes.GREEN), tris[half:])] if half else \
        [(scenes.material(**scenes.KHAKI), tris)]
    s = scenes._finish("soup", u, sp, np.zeros(0, dtype=abi.POINT_LIGHT), groups)
    assert len(s.bvh_nodes) == 1 and int(s.bvh_nodes["primitive_count"][0]) == len(tris)
    return s


NAN = float("nan")
ODD = [((0, 1, -4), (0, 1, -4), (0, 1, -4)),                     # a point
       ((-1, 1, -4), (0, 1, -4), (1, 1, -4)),                    # a segment: N = 0
       ((NAN, 1, -4), (1, 1, -4), (0, 2, -4)),                   # a NaN vertex
       ((-1e30, -1e30, -9), (1e30, -1e30, -9), (0, 1e30, -9)),   # beyond the range the bounds are claimed for
       ((0, 0, -5), (0, 0, -5), (1, 1, -5))]
SOUPS = ("soup33", "soup64", "soup97", "soup128")
W, H = 33, 17


def _with_list(scene, indices, first, count):
    nodes = scene.bvh_nodes.copy()
    nodes["first_primitive"][0], nodes["primitive_count"][0] = first, count
    return dataclasses.replace(scene, bvh_nodes=nodes, bvh_indices=np.asarray(indices, np.uint32))


def _mixed():
    """_soup(9) and the ODD triangles, those in the middle of the list with a dead slot beside them: open groups between closed ones"""
    s = _soup(9, W, H, extra=ODD)
    idx = [int(i) for i in s.bvh_indices]
    plain, odd = [i for i in idx if i < 9], [i for i in idx if i >= 9]
    dead = len(s.bvh_triangles) + 3
    return _with_list(s, plain[:5] + odd[:2] + [dead] + odd[2:] + plain[5:], 0, len(idx) + 1)


def _strip():
    """_soup(20) with two runs of coplanar triangles in its list, of 3 and of 4: an oblique quad whose in-plane edges a, b have
    a_k b_k >= 0 on every axis, so that the diagonal p0 p2 spans the quad's whole box, and triangles that all hold that diagonal --
    the union box is each member's own, the normals are one: groups of 3 and of 4, which the soups' quads do not give (the box of
    one half of an oblique quad is smaller than the quad's by more than kSiftBoxGrow allows)"""
    def run(c, a, b, thirds):
        c, a, b = (np.asarray(x, np.float64) for x in (c, a, b))
        assert (a * b >= 0).all()
        return [(tuple(c - a - b), tuple(c + s * a - s * b), tuple(c + a + b)) for s in thirds]
    extra = run((-1.0, 2.0, -4.5), (0.9, 0.5, 0.0), (0.0, 0.4, 0.7), (1.0, -1.0, 0.4)) + \
        run((1.5, 3.5, -5.5), (0.6, 0.0, 0.8), (0.3, 0.9, 0.2), (1.0, -1.0, 0.5, -0.3))
    s = _soup(20, W, H, extra=extra)
    idx = [int(i) for i in s.bvh_indices]
    plain, three, four = [i for i in idx if i < 20], list(range(20, 23)), list(range(23, 27))
    return _with_list(s, plain[:6] + three + plain[6:13] + four + plain[13:], 0, len(idx))


def _bent(tilt=1.8e-3):
    """the Cornell box with every wall's quad bent about its diagonal by `tilt`: groups of two whose cone is nearly as wide as
    kSiftAlphaMax allows (s about 0.9e-3 where a planar quad's is 2e-6), axis-aligned edges, thin boxes -- where lb = |d . n| - s
    decides and a ray along an edge can miss the group's box"""
    groups = []
    for mat, tl in scenes.cornell_groups():
        out = []
        for q in range(0, len(tl), 2):
            p0, p1, p2 = (np.asarray(v, np.float64) for v in tl[q])
            p3 = np.asarray(tl[q + 1][2], np.float64)
            n = np.cross(p1 - p0, p2 - p0)
            n /= np.linalg.norm(n)
            dg = (p2 - p0) / np.linalg.norm(p2 - p0)
            p3 = p3 + n * tilt * np.linalg.norm((p3 - p0) - ((p3 - p0) @ dg) * dg)
            out += [(tuple(p0), tuple(p1), tuple(p2)), (tuple(p0), tuple(p2), tuple(p3))]
        groups.append((mat, out))
    u = scenes.make_uniforms(W, H, SPP, DEPTH, cam_pos=(0, 3, 5), cam_dir=(0, 0, -1), ground_enabled=0, sky=(0, 0, 0))
    return scenes._finish("bent", u, scenes.cornell_spheres(), np.zeros(0, abi.POINT_LIGHT), groups)


def _offset():
    """40 triangles behind 7 leading index entries the node does not name; its list is a permutation, three of its slots dead"""
    s = _soup(40, W, H)
    rng = np.random.default_rng(40)
    perm = rng.permutation(np.asarray(s.bvh_indices, np.int64))
    perm[[3, 17, 36]] = [40, 0xFFFFFFFF, 41]        # >= bvh_triangle_count: dead (two in the list's first block of 32, one in its second)
    lead = rng.integers(0, 40, 7)
    return _with_list(s, np.concatenate([lead, perm]), 7, 40)


_BUILDERS = {
    "soup33": lambda: _soup(33, W, H), "soup64": lambda: _soup(64, W, H), "soup97": lambda: _soup(97, W, H), "soup128": lambda: _soup(128, W, H),
    "strip": _strip, "bent": _bent, "mixed": _mixed, "offset": _offset,
    "far": lambda: _soup(33, W, H, shift=(4096.0, -2048.0, 8192.0)),
    "small": lambda: _soup(33, W, H, scale=2.0 ** -10), "large": lambda: _soup(33, W, H, scale=2.0 ** 10),
}


def tables():
    """the names of the single-node scenes beside the Cornell box that pass 1 is held on; each sifts (table_scene, table_of)"""
    return list(_BUILDERS)


@functools.lru_cache(maxsize=None)
def table_scene(name):
    """the scene of that name at 33 x 17, 4 spp, depth 8 (shared: nobody writes to it)"""
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def table_of(name):
    """the model's (groups, region, (v0, e1, e2, valid)) of the scene's node's list, and [first, end)"""
    s = table_scene(name)
    first, end = node_list(s)
    return _scene_table(s, first=first, end=end), (first, end)


# ------------------------------------------------------------------------------- the ray families ---
MAX_AIMED = 20_000
OFFSETS = (0, 1, -1, 4, -4, 64, -64)                  # k: outward (+) and inward (-), units of 2^-23 max|coordinate of the triangle|
ANGLES = (0.5, 1e-1, 1e-2, 1e-3, 1e-4, 1e-5)          # grazing angles between the ray and the triangle's plane


def _aimable(tri):
    """the live slots a point can be aimed at: finite vertices of ordinary size, a normal"""
    v0, e1, e2, valid = tri
    with np.errstate(all="ignore"):
        n = np.cross(e1.astype(np.float64), e2.astype(np.float64))
        size = np.abs(np.concatenate([v0, v0 + e1, v0 + e2], 1).astype(np.float64)).max(1)
        ok = valid & np.isfinite(v0).all(1) & np.isfinite(e1).all(1) & np.isfinite(e2).all(1) & (np.linalg.norm(n, axis=1) > 0) & (size < 1e9)
    return np.flatnonzero(ok)


def _targets(tri, rng):
    """Points P in the plane of every aimable slot: the three vertices and two points on each edge (its middle and a random one),
    moved along the in-plane outward normal of the edge (at a vertex: away from the centroid) by k of OFFSETS.
    -> (P float64 [m][3], slot [m], k [m], plane normal [m][3], an in-plane unit vector [m][3])"""
    v0, e1, e2, _ = tri
    P, S, K, N, T = [], [], [], [], []
    for s in _aimable(tri):
        a = v0[s].astype(np.float64)
        v = np.stack([a, a + e1[s].astype(np.float64), a + e2[s].astype(np.float64)])
        nrm = np.cross(v[1] - v[0], v[2] - v[0])
        nrm /= np.linalg.norm(nrm)
        cen = v.mean(0)
        unit = 2.0 ** -23 * np.abs(v).max()
        base = []
        for i in range(3):
            out = v[i] - cen
            base.append((v[i], out / np.linalg.norm(out)))
            p, q = v[i], v[(i + 1) % 3]
            en = np.cross(q - p, nrm)
            en /= np.linalg.norm(en)
            if en @ (cen - p) > 0:
                en = -en
            for w in (0.5, rng.uniform(0.02, 0.98)):
                base.append((p + w * (q - p), en))
        tang = (v[1] - v[0]) / np.linalg.norm(v[1] - v[0])
        for point, out in base:
            for k in OFFSETS:
                P.append(point + k * unit * out), S.append(s), K.append(k), N.append(nrm), T.append(tang)
    return np.array(P), np.array(S), np.array(K), np.array(N), np.array(T)


def _on_triangles(tri, slots, rng, near=None, tries=8):
    """a point on triangle slots[i] each (float32, as a hit point is); `near` [n][3]: of `tries` draws the one closest to it"""
    v0, e1, e2, _ = tri
    n = len(slots)
    a, b = rng.random((tries, n)), rng.random((tries, n))
    a, b = np.where(a + b > 1, 1 - a, a), np.where(a + b > 1, 1 - b, b)
    q = v0[slots].astype(np.float64)[None] + a[..., None] * e1[slots].astype(np.float64)[None] + b[..., None] * e2[slots].astype(np.float64)[None]
    if near is None:
        return q[0].astype(F32)
    pick = np.linalg.norm(q - near[None], axis=2).argmin(0)
    return q[pick, np.arange(n)].astype(F32)


def aimed_rays(tri, region, rng):
    """Rays aimed at where pass 1 can be wrong: at points P on the edges and at the vertices of every live triangle of the list
    `tri` (v0, e1, e2, valid), moved outward and inward by a few units of the triangle's own rounding, on rays that graze the
    plane -- where the reference test's rounding accepts a point outside the exact triangle.  Two sets of origins, both inside
    `region` (the model's, M.table_region): o = P + r (cos a t + sin a n), t in the plane, a of ANGLES, r redrawn until o is
    inside; and points on another triangle of the list, as a bounce's origin is, half of them the closest of eight draws to P (a
    small t).  d = _unit(P - o).  At most MAX_AIMED rays.
    -> (o [n][3], d [n][3] float32, the aimed slot [n], P is outside the exact triangle [n])"""
    P, S, K, N, T = _targets(tri, rng)
    lo, hi = region["lo"][:, 0].astype(np.float64), region["hi"][:, 0].astype(np.float64)
    inside = ((P > lo) & (P < hi)).all(1)         # (a triangle no closed group holds need not lie in the region)
    P, S, K, N, T = P[inside], S[inside], K[inside], N[inside], T[inside]
    m = len(P)
    assert m > 0
    per = int(np.clip(MAX_AIMED // 2 // m, 1, len(ANGLES)))      # angles per target in the first set
    if 2 * m > MAX_AIMED:                                         # (128 slots: 8064 targets, one ray of each set)
        keep = np.sort(rng.permutation(m)[:MAX_AIMED // 2])
        P, S, K, N, T, m = P[keep], S[keep], K[keep], N[keep], T[keep], len(keep)
    # ---- the grazing origins
    rep = np.repeat(np.arange(m), per)
    ang = np.array(ANGLES)[(rep + np.tile(np.arange(per), m) + rng.integers(0, len(ANGLES))) % len(ANGLES)]
    # the reference refuses |a| < 1e-6 before anything else, a = e1 . (d x e2) = |e1 x e2| sin(angle): where a small triangle puts
    # an angle of ANGLES below that floor, three rays of four take the angle that puts |a| a twentieth above it instead (the flattest
    # ray the triangle accepts at all, where its rounding is largest); a triangle with |e1 x e2| below the floor keeps pi / 2
    cross = np.linalg.norm(np.cross(tri[1].astype(np.float64), tri[2].astype(np.float64)), axis=1)[S[rep]]
    at_floor = np.arcsin(np.minimum(1.0, 1.05e-6 / np.maximum(cross, 1e-300)))
    ang = np.where((cross * np.sin(ang) <= 1.05e-6) & (rng.random(len(rep)) < 0.75), at_floor, ang)
    p, size = P[rep], float((hi - lo).max())
    o = np.zeros_like(p)
    todo, top = np.ones(len(rep), bool), size
    for _ in range(400):      # a ray that leaves the region is drawn again, direction in the plane, side and distance
        k = int(todo.sum())
        phi = rng.uniform(0, 2 * np.pi, k)
        t = np.cos(phi)[:, None] * T[rep][todo] + np.sin(phi)[:, None] * np.cross(N[rep][todo], T[rep][todo])
        u = np.cos(ang[todo])[:, None] * t + (np.sin(ang[todo]) * rng.choice([-1.0, 1.0], k))[:, None] * N[rep][todo]
        # every scale of distance, and half of the rays from far away, where the reference's rounding is largest
        r = top * 10.0 ** np.where(rng.random(k) < 0.5, rng.uniform(-3.0, 0.0, k), rng.uniform(-0.5, 0.0, k))
        if top > 0.0011:   # the reference refuses t <= 0.001 whatever the scene's size: in a small scene most rays start beyond that
            r = np.where(rng.random(k) < 0.75, np.maximum(r, 0.0011), r)
        o[todo] = (p[todo] + r[:, None] * u).astype(F32)
        todo = ~((o > lo) & (o < hi)).all(1)
        if not todo.any():
            break
        top *= 0.98
    assert not todo.any(), "an origin could not be placed inside the region"
    O, D, slot, outside = [o.astype(F32)], [_unit(p - o.astype(F32).astype(np.float64))], [S[rep]], [K[rep] > 0]
    # ---- origins on another triangle of the list
    can = _aimable(tri)
    if len(can) > 1:
        other = can[(np.searchsorted(can, S) + rng.integers(1, len(can), m)) % len(can)]
        cen = (tri[0][can] + (tri[1][can] + tri[2][can]) / F32(3)).astype(np.float64)
        dist = np.linalg.norm(cen[None] - P[:, None], axis=2)
        dist[np.arange(m), np.searchsorted(can, S)] = np.inf
        close = rng.random(m) < 0.5
        other = np.where(close, can[dist.argmin(1)], other)
        q = np.where(close[:, None], _on_triangles(tri, other, rng, near=P), _on_triangles(tri, other, rng))
        O.append(q), D.append(_unit(P - q.astype(np.float64))), slot.append(S), outside.append(K > 0)
    o, d, slot, outside = np.concatenate(O), np.concatenate(D), np.concatenate(slot), np.concatenate(outside)
    assert len(o) <= MAX_AIMED
    return o, d, slot, outside


def aimed_census(tri, o, d, slot, outside):
    """of the (ray, aimed slot) pairs: (share the reference test accepts, share it refuses, share of the accepted whose P is outside
    the exact triangle) -- what keeps the aimed family from being empty; decided by the reference alone"""
    acc = _accepted(tri, np.ascontiguousarray(o.T), np.ascontiguousarray(d.T))[slot, np.arange(len(slot))]
    return float(acc.mean()), float((~acc).mean()), float(outside[acc].mean()) if acc.any() else 0.0


def region_rays(region, n, rng):
    """origins uniform inside the region's box, every direction"""
    lo, hi = region["lo"][:, 0].astype(np.float64), region["hi"][:, 0].astype(np.float64)
    return (lo + rng.random((n, 3)) * (hi - lo)).astype(F32), _unit(rng.normal(size=(n, 3)))


def surface_rays(tri, n, rng):
    """origins on the list's triangles (a bounce's), every direction"""
    can = _aimable(tri)
    return _on_triangles(tri, can[rng.integers(0, len(can), n)], rng), _unit(rng.normal(size=(n, 3)))


def face_rays(region, n, rng):
    """origins just inside and just outside the faces of the region's box (one or two float32 steps from a face's coordinate,
    the other two coordinates inside), every direction: the lanes that change between sifting and taking every slot"""
    o, d = region_rays(region, n, rng)
    lo, hi = region["lo"][:, 0], region["hi"][:, 0]
    axis, side, steps = rng.integers(0, 3, n), rng.integers(0, 2, n), rng.integers(-2, 3, n)
    face = np.where(side == 0, lo[axis], hi[axis]).astype(F32)
    for k in range(2):
        face = np.where(np.abs(steps) > k, np.nextafter(face, np.where(steps > 0, F32(np.inf), F32(-np.inf)).astype(F32)), face).astype(F32)
    o[np.arange(n), axis] = face
    return o, d


def edge_rays(tri, region, n, rng):
    """Rays that run along an edge of a triangle of the list, outside it by 10^-2.5 .. 10^-0.5 and 10^-6.5 .. 10^-3.5 off its plane,
    origins inside the region: far beyond what the reference test's rounding accepts, and flat enough that |d . n| is of the size
    of a bent group's s -- the rays on which the sign of s in lb = |d . n| - s shows in the masks (a planar group's s, 2e-6, shows
    on a few of them only).  -> (o, d) float32, fewer than n (an origin outside the region is dropped)"""
    v0, e1, e2, _ = tri
    can = _aimable(tri)
    s = can[rng.integers(0, len(can), n)]
    a = v0[s].astype(np.float64)
    v = np.stack([a, a + e1[s], a + e2[s]], 1)
    nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    i, k = rng.integers(0, 3, n), np.arange(n)
    p, q, cen = v[k, i], v[k, (i + 1) % 3], v.mean(1)
    ed = q - p
    length = np.linalg.norm(ed, axis=1)
    ed /= length[:, None]
    en = np.cross(ed, nrm)
    en *= np.where((en * (cen - p)).sum(1) > 0, -1.0, 1.0)[:, None]
    ang, delta, w = 10.0 ** rng.uniform(-6.5, -3.5, n), 10.0 ** rng.uniform(-2.5, -0.5, n), rng.uniform(0.02, 0.98, n)
    target = p + (w * length)[:, None] * ed + delta[:, None] * en
    u = (np.cos(ang) * rng.choice([-1.0, 1.0], n))[:, None] * ed + (np.sin(ang) * rng.choice([-1.0, 1.0], n))[:, None] * nrm
    o = (target - (length * 10.0 ** rng.uniform(-1.5, 0.0, n))[:, None] * u).astype(F32)
    ok = ((o > region["lo"][:, 0]) & (o < region["hi"][:, 0])).all(1)
    return o[ok], _unit(target[ok] - o[ok].astype(np.float64))
