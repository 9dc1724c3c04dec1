"""Closest-hit queries (rb_cast_rays / rb_render_hits / rb_pick) against the unmodified oracle, bit for bit on uint32 views,
no ray left out.

Way 1 -- the oracle's own walk decides the winner: rbo_trace_ray with max_depth = 1 returns exactly emissive(winner) (or the
sky colour), so on a copy of the scene whose emissive fields carry (kind, index + 1) as small integers the query's
rb_surface.emissive must equal the oracle's three floats for every ray.  Traversal, category order, ties and the phantom light
are the oracle's, nothing is restated here.  (The ground reads 0, and with colour hash a triangle does too.)
Way 2 -- the record is the shader's arithmetic on the reported primitive: t (u, v) from rbo_intersect_*, the normal and the
surface fields from numpy-float32 evaluation of shader.wgsl:351, :558, :582, :598, :615-651 with rbo_sample_texture /
rbo_hash_to_color.  For a sphere or light winner the uv and use_texture that the earlier stages left behind (the shader's
quirk: a beaten BVH hit keeps its uv, a light does not reset use_texture) come from the oracle too: rbo_trace_ray on the scene
without spheres and lights names the winner of the ground + BVH stage, on the scene without lights the winner of the sphere stage.
Way 3 -- every walk gives the same records.
"""
import ctypes as C

import numpy as np
import pytest

from renderbaby_amd import Engine, RenderConfig, abi, scenes
from renderbaby_amd.engine import Change
from tests import _oracle
from tests.conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

f32 = np.float32
SKY_ID = (9.0, 8.0, 7.0)


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _normalize(v):
    v = np.asarray(v, f32)
    return (v / np.sqrt((v[..., 0:1] * v[..., 0:1] + v[..., 1:2] * v[..., 1:2]) + v[..., 2:3] * v[..., 2:3])).astype(f32)


def _engine(scene, with_tree=True, **kw):
    """an engine holding `scene` (the first update: nothing is rendered)"""
    rc = RenderConfig.from_scene(scene, with_tree=with_tree)
    if "devices" not in kw:
        kw["device"] = 0
    e = Engine.new(rc, **kw)
    e.update(rc)
    return e


def _copy(s, **over):
    d = dict(uniforms=s.uniforms.copy(), spheres=s.spheres.copy(), lights=s.lights.copy(), meshes=s.meshes.copy(),
             bvh_nodes=s.bvh_nodes, bvh_indices=s.bvh_indices, bvh_triangles=s.bvh_triangles.copy(), uvs=s.uvs, textures=s.textures)
    d.update(over)
    return scenes.Scene(d["uniforms"], d["spheres"], d["lights"], d["meshes"], d["bvh_nodes"], d["bvh_indices"],
                        d["bvh_triangles"], d["uvs"], d["textures"], s.name)


def id_scene(s, per_triangle=False):
    """The scene with identification in the emissive fields: x = kind, y = index + 1 (positive integers: 0 + 1 * e is e bit
    for bit); per_triangle: one mesh per triangle (each with its triangle's material otherwise), so that y names the triangle."""
    t = _copy(s)
    if per_triangle and len(t.bvh_triangles):
        meshes = np.zeros(len(t.bvh_triangles), dtype=abi.MESH)
        for i, tri in enumerate(t.bvh_triangles):
            meshes[i] = s.meshes[int(tri["mesh_index"])]
        t.bvh_triangles["mesh_index"] = np.arange(len(t.bvh_triangles), dtype=np.uint32)
        t.meshes = meshes
    for arr, kind in ((t.spheres, abi.HIT_SPHERE), (t.lights, abi.HIT_LIGHT), (t.meshes, abi.HIT_TRIANGLE)):
        for i in range(len(arr)):
            arr["material"]["emissive"][i] = (kind, i + 1, 0)
    t.uniforms["sky_color"] = SKY_ID
    t.uniforms["max_depth"] = 1
    return t


def oracle_emissive(scene, O, D, counts_kept=0):
    os_ = _oracle.OracleScene(scene, 1, counts_kept)
    L = _oracle.lib()
    out = np.zeros((len(O), 3), f32)
    rgb = np.zeros(3, f32)
    st = _oracle.Stats()
    for i in range(len(O)):
        o, d = np.ascontiguousarray(O[i], f32), np.ascontiguousarray(D[i], f32)
        L.rbo_trace_ray(C.byref(os_.c), o.ctypes.data, d.ctypes.data, 12345, rgb.ctypes.data, C.byref(st))
        out[i] = rgb
    return out


def pixel_centre_rays(scene):
    """[row, displayed column] -> (origin, direction) of rbo_primary_ray(u, x, y, 0, 0), x = width - 1 - column."""
    w, h = scene.width, scene.height
    O, D = np.zeros((h, w, 3), f32), np.zeros((h, w, 3), f32)
    L = _oracle.lib()
    u = np.ascontiguousarray(scene.uniforms)
    o, d = np.zeros(3, f32), np.zeros(3, f32)
    for y in range(h):
        for xd in range(w):
            L.rbo_primary_ray(u.ctypes.data, w - 1 - xd, y, f32(0), f32(0), o.ctypes.data, d.ctypes.data)
            O[y, xd], D[y, xd] = o, d
    return O, D


def sample_texture(os_, index, uv):
    rgb = np.zeros(3, f32)
    uv = np.ascontiguousarray(uv, f32)
    _oracle.lib().rbo_sample_texture(C.byref(os_.c), int(index), uv.ctypes.data, rgb.ctypes.data)
    return rgb


def is_metal(m):
    s, d = m["specular"].astype(f32), m["diffuse"].astype(f32)
    return bool(((s[0] + s[1]) + s[2]) / f32(3.0) > f32(0.01) and ((d[0] + d[1]) + d[2]) / f32(3.0) < f32(0.01))


FAR_LIGHT = np.zeros(1, dtype=abi.POINT_LIGHT)
FAR_LIGHT["center"] = (1e30, 1e30, 1e30)   # |oc|^2 overflows: the discriminant is NaN, the returned root NaN, `t > 0.001` false: never hit


class Stages:
    """What the stages before the winner left in closest_hit, from the oracle's own walk: the scene with one mesh per triangle
    and identification in the emissive fields, colour hash off (it does not move the winner), (A) without spheres and lights,
    (B) without lights."""

    def __init__(self, scene, counts_kept):
        b = id_scene(scene, per_triangle=True)
        b.uniforms["color_hash_enabled"] = 0
        b = _copy(b, lights=FAR_LIGHT.copy())
        a = _copy(b, spheres=np.zeros(0, dtype=abi.SPHERE))
        a.uniforms["spheres_count"] = 0
        self.scene = scene
        self.a = _oracle.OracleScene(a, 1, counts_kept & ~_oracle.KEPT_SPHERES)
        self.b = _oracle.OracleScene(b, 1, counts_kept)
        self.hashed = int(scene.uniforms["color_hash_enabled"][0]) != 0

    def _trace(self, os_, o, d):
        rgb, st = np.zeros(3, f32), _oracle.Stats()
        o, d = np.ascontiguousarray(o, f32), np.ascontiguousarray(d, f32)
        _oracle.lib().rbo_trace_ray(C.byref(os_.c), o.ctypes.data, d.ctypes.data, 1, rgb.ctypes.data, C.byref(st))
        return rgb

    def after_bvh(self, o, d):
        """(uv, use_texture) after the ground and BVH stages, :552-571"""
        sc, e = self.scene, self._trace(self.a, o, d)
        if tuple(e) == SKY_ID:
            return np.zeros(2, f32), False
        if e[0] == 0:   # the ground
            t = f32(_oracle.isect_ground(o, d, float(sc.uniforms["ground_height"][0])))
            pos = (o + t * d).astype(f32)
            return np.array([pos[0], pos[2]], f32), True
        assert int(e[0]) == abi.HIT_TRIANGLE
        tri = sc.bvh_triangles[int(e[1]) - 1]
        _, u, v = _oracle.isect_triangle(o, d, tri["v0"], tri["v1"], tri["v2"])
        tex = int(sc.meshes[int(tri["mesh_index"])]["material"]["texture_index"])
        return tri_uv(sc, tri, f32(u), f32(v)), (False if self.hashed else tex >= 0)

    def after_spheres(self, o, d):
        """use_texture after the sphere stage, :574-586"""
        e = self._trace(self.b, o, d)
        if int(e[0]) == abi.HIT_SPHERE and tuple(e) != SKY_ID:
            return int(self.scene.spheres[int(e[1]) - 1]["material"]["texture_index"]) >= 0
        return self.after_bvh(o, d)[1]


def tri_uv(scene, tri, u, v):
    """:353-361"""
    uvs = scene.uvs

    def uv_of(k):
        return np.array([uvs[k * 2] if k * 2 < len(uvs) else 0, uvs[k * 2 + 1] if k * 2 + 1 < len(uvs) else 0], f32)
    w_ = f32(f32(1.0) - u) - v
    return ((w_ * uv_of(int(tri["v0_index"])) + u * uv_of(int(tri["v1_index"]))) + v * uv_of(int(tri["v2_index"]))).astype(f32)


def check_records(scene, O, D, hits, surf, label="", counts_kept=0):
    """Way 2 for every ray: the record against the shader's arithmetic on the primitive it names.  D is normalised.
    Returns how many sphere / light winners inherited a uv or use_texture from an earlier stage's hit."""
    os_ = _oracle.OracleScene(scene, 1, counts_kept)
    stages, inherited = Stages(scene, counts_kept), 0
    u = scene.uniforms[0]
    O, D = O.reshape(-1, 3), D.reshape(-1, 3)
    hits, surf = hits.reshape(-1), surf.reshape(-1)
    zero3 = np.zeros(3, f32)
    for i in range(len(O)):
        o, d, h, s = O[i], D[i], hits[i], surf[i]
        kind, where = int(h["kind"]), (label, i)
        exp_uv, exp_normal, exp_u, exp_v = None, zero3, f32(0), f32(0)
        mat, diffuse, tex, use_tex_known = None, None, -1, None
        if kind == abi.HIT_NONE:
            assert _u32(h["t"]) == _u32(f32(1e20)) and h["prim"] == abi.NO_INDEX and h["mesh"] == abi.NO_INDEX, where
            assert np.array_equal(_u32(s["emissive"]), _u32(u["sky_color"])), where
            assert np.array_equal(_u32(h["normal"]), _u32(zero3)) and np.array_equal(_u32(s["albedo"]), _u32(zero3)), where
            continue
        if kind == abi.HIT_GROUND:
            t = f32(_oracle.isect_ground(o, d, float(u["ground_height"])))
            pos = (o + t * d).astype(f32)
            exp_normal, exp_uv = np.array([0, 1, 0], f32), np.array([pos[0], pos[2]], f32)
            diffuse, emissive, metal, use_tex_known = np.full(3, 0.5, f32), zero3, False, True
            assert h["prim"] == abi.NO_INDEX and h["mesh"] == abi.NO_INDEX, where
        elif kind == abi.HIT_TRIANGLE:
            tri = scene.bvh_triangles[int(h["prim"])]
            t, exp_u, exp_v = _oracle.isect_triangle(o, d, tri["v0"], tri["v1"], tri["v2"])
            t, exp_u, exp_v = f32(t), f32(exp_u), f32(exp_v)
            e1, e2 = (tri["v1"] - tri["v0"]).astype(f32), (tri["v2"] - tri["v0"]).astype(f32)
            cr = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]], f32)
            exp_normal = _normalize(cr)
            assert int(h["mesh"]) == int(tri["mesh_index"]), where
            exp_uv = tri_uv(scene, tri, exp_u, exp_v)
            if int(u["color_hash_enabled"]):
                diffuse, emissive, metal, use_tex_known = _oracle.hash_to_color(int(h["prim"]) + 1), zero3, False, False
            else:
                mat = scene.meshes[int(tri["mesh_index"])]["material"]
        elif kind in (abi.HIT_SPHERE, abi.HIT_LIGHT):
            prims = scene.spheres if kind == abi.HIT_SPHERE else scene.lights
            if kind == abi.HIT_LIGHT and len(prims) == 0:
                prims = np.zeros(1, dtype=abi.POINT_LIGHT)   # the phantom light of an empty buffer
            p = prims[int(h["prim"])]
            t = f32(_oracle.isect_sphere(o, d, p["center"], float(p["radius"])))
            pos = (o + t * d).astype(f32)
            exp_normal = _normalize((pos - p["center"]).astype(f32))
            mat = p["material"]
            assert h["mesh"] == abi.NO_INDEX, where
            exp_uv, use_a = stages.after_bvh(o, d)   # nobody after the BVH stage writes uv
            use_tex_known = stages.after_spheres(o, d) if kind == abi.HIT_LIGHT else int(mat["texture_index"]) >= 0
            inherited += int(exp_uv.any() or (kind == abi.HIT_LIGHT and use_tex_known))
        else:
            raise AssertionError((where, "kind", kind))
        if mat is not None:
            diffuse, emissive, metal, tex = mat["diffuse"].astype(f32), mat["emissive"].astype(f32), is_metal(mat), int(mat["texture_index"])
            if kind == abi.HIT_TRIANGLE:
                use_tex_known = tex >= 0
        assert t > f32(0.001) and _u32(h["t"]) == _u32(t), (where, h["t"], t)
        assert _u32(h["u"]) == _u32(exp_u) and _u32(h["v"]) == _u32(exp_v), where
        assert np.array_equal(_u32(h["normal"]), _u32(exp_normal)), (where, h["normal"], exp_normal)
        assert np.array_equal(_u32(s["emissive"]), _u32(emissive)), where
        assert int(s["texture_index"]) == tex, where
        use_tex = bool(use_tex_known)
        assert bool(int(s["flags"]) & abi.SURFACE_USE_TEXTURE) == use_tex, (where, kind)
        assert bool(int(s["flags"]) & abi.SURFACE_IS_METAL) == metal, where
        assert np.array_equal(_u32(s["uv"]), _u32(exp_uv)), (where, kind, s["uv"], exp_uv)
        if metal:
            exp_albedo = mat["specular"].astype(f32)
        elif use_tex:
            exp_albedo = (diffuse * sample_texture(os_, tex, exp_uv)).astype(f32)
        else:
            exp_albedo = diffuse
        assert np.array_equal(_u32(s["albedo"]), _u32(exp_albedo)), (where, s["albedo"], exp_albedo)
    return inherited


def check_winner_ids(ids_scene, hits, em):
    """the record's (kind, prim / mesh) names the primitive the oracle's walk picked"""
    hits, em = hits.reshape(-1), em.reshape(-1, 3)
    hashed = int(ids_scene.uniforms["color_hash_enabled"][0]) != 0
    for i in range(len(hits)):
        k, e = int(hits[i]["kind"]), em[i]
        if tuple(e) == SKY_ID:
            assert k == abi.HIT_NONE, i
        elif e[0] == 0:
            assert k == abi.HIT_GROUND or (hashed and k == abi.HIT_TRIANGLE), (i, k)
        else:
            assert k == int(e[0]), (i, k, e)
            assert int(hits[i]["mesh" if k == abi.HIT_TRIANGLE else "prim"]) + 1 == int(e[1]), (i, k, e)


def random_rays(scene, n, seed):
    """origins inside and outside the scene box, random / axis-parallel / zero / non-finite directions, origins on a surface"""
    rng = np.random.default_rng(seed)
    pts = [scene.bvh_triangles["v0"].reshape(-1, 3), scene.spheres["center"].reshape(-1, 3), np.zeros((1, 3), f32)]
    pts = np.concatenate([p for p in pts if len(p)])
    lo, hi = pts.min(0) - 1.0, pts.max(0) + 1.0
    O = rng.uniform(lo - 3.0 * (hi - lo) * (rng.random((n, 1)) < 0.3), hi + 3.0 * (hi - lo) * (rng.random((n, 1)) < 0.3), (n, 3)).astype(f32)
    D = rng.normal(size=(n, 3)).astype(f32) * rng.choice([1.0, 3.0, 2.0 ** -20], size=(n, 1)).astype(f32)
    ax = np.eye(3, dtype=f32)
    for k in range(0, n, 11):
        D[k] = ax[k % 3] * (-1 if k % 2 else 1)          # axis-parallel
    for k in range(5, n, 97):
        D[k] = 0                                         # zero direction: INVALID
    for k in range(7, n, 101):
        D[k, k % 3] = [np.nan, np.inf, -np.inf][k % 3]   # INVALID (inf / inf)
    for k in range(9, n, 103):
        O[k, k % 3] = np.nan                             # INVALID
    for k in range(4, n, 89):
        D[k] = np.array([1e25, -3e24, 2e20], f32) * f32(-1 if k % 2 else 1)   # the squared length overflows: normalises to zero, INVALID
    for k in range(3, n, 13):                            # origins on a surface: the t > 0.001 rule
        if len(scene.bvh_triangles):
            tri = scene.bvh_triangles[k % len(scene.bvh_triangles)]
            O[k] = (tri["v0"] + tri["v1"] + tri["v2"]) / f32(3)
        elif len(scene.spheres):
            sp = scene.spheres[k % len(scene.spheres)]
            O[k] = sp["center"] + _normalize(D[k:k + 1])[0] * sp["radius"]
    return O, D


def plane_rays(scene, per_triangle=4, max_triangles=64):
    """Rays IN the plane of a triangle: origins v0 + a e1 + b e2 inside and outside the triangle, directions c e1 + g e2 along the
    plane -- the determinant of the triangle test is zero up to rounding, the case the culled walks' margins must survive.  For
    an axis-aligned triangle both are exactly in the plane.  Returns (origins, directions, how many are exactly in a y = const plane)."""
    tris = scene.bvh_triangles
    flat = [i for i in range(len(tris)) if tris["v0"][i][1] == tris["v1"][i][1] == tris["v2"][i][1]]
    pick = list(dict.fromkeys(flat + [int(i) for i in np.linspace(0, len(tris) - 1, max_triangles).astype(int)]))[:max_triangles]
    ab = [(0.3, 0.3, 1.0, 0.0), (0.25, 0.5, -0.4, 1.0), (1.5, -0.75, -1.0, 0.5), (-2.0, -1.0, 1.0, 1.0)][:per_triangle]
    O, D, exact = [], [], 0
    for i in pick:
        v0 = tris["v0"][i].astype(f32)
        e1, e2 = (tris["v1"][i] - v0).astype(f32), (tris["v2"][i] - v0).astype(f32)
        for a, b, c, g in ab:
            o = (v0 + f32(a) * e1 + f32(b) * e2).astype(f32)
            d = (f32(c) * e1 + f32(g) * e2).astype(f32)
            O.append(o)
            D.append(d)
            exact += int(i in flat and o[1] == v0[1] and d[1] == 0)
    return np.array(O, f32).reshape(-1, 3), np.array(D, f32).reshape(-1, 3), exact


def check_scene(scene, per_triangle=False, n_random=1500, counts_kept=0, mutate=None, min_plane_exact=0, min_inherited=0, **engine_kw):
    """ways 1 and 2 on every pixel centre (rb_render_hits, and the same rays through rb_cast_rays scaled) and on random rays"""
    ids = id_scene(scene, per_triangle)
    O, D = pixel_centre_rays(scene)
    e, ei = _engine(scene, **engine_kw), _engine(ids, **engine_kw)
    if mutate is not None:   # an update after the first: the scenes the engines now hold
        scene, ids = mutate(e, scene), mutate(ei, ids)
    try:
        st0 = e.stats()
        hits, surf = e.render_hits(surfaces=True)
        assert hits.shape == (scene.height, scene.width)
        inherited = check_records(scene, O, D, hits, surf, scene.name + " pixels", counts_kept)
        hits_i, surf_i = ei.render_hits(surfaces=True)
        em = oracle_emissive(ids, O.reshape(-1, 3), D.reshape(-1, 3), counts_kept)
        assert np.array_equal(_u32(surf_i["emissive"]).reshape(-1, 3), _u32(em)), scene.name
        check_winner_ids(ids, hits_i, em)
        for f in ("t", "kind", "prim", "u", "v", "normal"):   # the id scene differs in emissive and mesh numbering only
            assert np.array_equal(_u32(hits_i[f]), _u32(hits[f])), f
        # the same rays, un-normalised: scaled by 3 and by 2^-20; the device's normalize() is the contract's
        for scale in (f32(3.0), f32(2.0 ** -20)):
            Ds = (D.reshape(-1, 3) * scale).astype(f32)
            h2, s2 = e.cast_rays(O.reshape(-1, 3), Ds, surfaces=True)
            Dn = _normalize(Ds)
            check_records(scene, O.reshape(-1, 3), Dn, h2, s2, f"{scene.name} x{scale}", counts_kept)
            em2 = oracle_emissive(ids, O.reshape(-1, 3), Dn, counts_kept)
            assert np.array_equal(_u32(ei.cast_rays(O.reshape(-1, 3), Ds, surfaces=True)[1]["emissive"]), _u32(em2))
        h1 = e.cast_rays(O.reshape(-1, 3), D.reshape(-1, 3))   # scale 1: normalising a unit vector may move an ulp; only when it does not ...
        same = np.all(_u32(_normalize(D.reshape(-1, 3))) == _u32(D.reshape(-1, 3)), axis=1)
        assert np.array_equal(h1[same].view(np.uint32), hits.reshape(-1)[same].view(np.uint32))   # ... the records are rb_render_hits'
        # random rays
        Or, Dr = random_rays(scene, n_random, 11)
        hr, sr = e.cast_rays(Or, Dr, surfaces=True)
        Dn = _normalize(Dr)
        bad = ~(np.isfinite(Or).all(1) & np.isfinite(Dn).all(1) & (Dn != 0).any(1))
        huge = np.arange(4, n_random, 89)
        assert bad[huge].all() and (np.abs(Dr[huge]).max(1) > 1e19).all()
        assert bad.sum() >= 3 and (hr["kind"][bad] == abi.HIT_INVALID).all() and (hr["kind"][~bad] != abi.HIT_INVALID).all()
        assert (_u32(hr["t"][bad]) == _u32(f32(1e20))).all() and not _u32(sr["emissive"][bad]).any() and not _u32(hr["normal"][bad]).any()
        inherited += check_records(scene, Or[~bad], Dn[~bad], hr[~bad], sr[~bad], scene.name + " random", counts_kept)
        assert inherited >= min_inherited, inherited
        emr = oracle_emissive(ids, Or[~bad], Dn[~bad], counts_kept)
        hri, sri = ei.cast_rays(Or, Dr, surfaces=True)
        assert np.array_equal(_u32(sri["emissive"][~bad]), _u32(emr))
        check_winner_ids(ids, hri[~bad], emr)
        # rays in the plane of a triangle
        if len(scene.bvh_triangles):
            Op, Dp, exact = plane_rays(scene)
            assert len(Op) == 4 * min(64, len(scene.bvh_triangles)) and exact >= min_plane_exact, (len(Op), exact)
            Dpn = _normalize(Dp)
            assert np.isfinite(Dpn).all() and (Dpn != 0).any(1).all()
            hp, sp_ = e.cast_rays(Op, Dp, surfaces=True)
            check_records(scene, Op, Dpn, hp, sp_, scene.name + " in-plane", counts_kept)
            emp = oracle_emissive(ids, Op, Dpn, counts_kept)
            hpi, spi = ei.cast_rays(Op, Dp, surfaces=True)
            assert np.array_equal(_u32(spi["emissive"]), _u32(emp))
            check_winner_ids(ids, hpi, emp)
        assert e.stats() == st0, "queries moved rb_get_stats"
        return e.last_query_kernel_name()
    finally:
        e.close()
        ei.close()


@pytest.mark.parametrize("color_hash", [0, 1])
def test_feature_scene(color_hash):
    """ground + checkerboard, textured mesh and sphere, lambert / fuzzy metal / mirror, two lights, emissive quad"""
    # (min_inherited: the textured sphere and the lights stand in front of the ground and the textured quad)
    assert check_scene(scenes.feature_scene(width=48, height=32, color_hash=color_hash), min_inherited=20) in ("k_query", "k_query_bvh", "k_query_chunk")


@pytest.mark.parametrize("kw,kernel", [(dict(), "k_query_chunk"), (dict(reference_walk=True), "k_query_bvh"),
                                       (dict(host_bvh=True), "k_query_bvh")])
def test_multi_node_mesh_one_id_per_triangle(kw, kernel):
    s = scenes.mesh_scene(12, 12, 40, 30, 1, 4, seed=3)
    assert len(s.bvh_nodes) > 1
    assert check_scene(s, per_triangle=True, n_random=800, **kw) == kernel


def test_cornell_has_the_phantom_light():
    s = scenes.cornell(48, 36, 1, 4)
    assert len(s.lights) == 0
    assert check_scene(s, per_triangle=True) == "k_query"


def _identical_spheres():
    s = scenes.spheres_scene(n=300, width=40, height=40, spp=1, max_depth=4, extent=5.0)
    sp = s.spheres.copy()
    sp["center"][:150] = sp["center"][0]
    sp["radius"][:150] = f32(0.7)            # 150 identical spheres: equal t, the lowest index must win
    sp["center"][150:] = sp["center"][150]
    sp["radius"][150:] = np.linspace(0.2, 2.0, 150).astype(f32)
    return scenes.Scene(s.uniforms, sp, s.lights, s.meshes, s.bvh_nodes, s.bvh_indices, s.bvh_triangles, s.uvs, name="identical")


@pytest.mark.parametrize("kw", [dict(sphere_tree="device"), dict(sphere_tree="host"), dict(no_sphere_bvh=True)])
def test_identical_spheres_tie_to_the_lowest_index(kw):
    check_scene(_identical_spheres(), n_random=600, **kw)


def _coincident_triangles():
    """every quad of a small grid four times over (equal t: the reference's first-visited triangle wins) plus 16 triangles in
    the plane y = 0, which plane_rays takes first: 64 rays whose origin and direction lie exactly in that plane"""
    base = scenes.mesh_scene(6, 6, 32, 24, 1, 4, seed=5, with_blob=False)
    groups = []
    for rep in range(4):
        tl = [(t["v0"], t["v1"], t["v2"]) for t in base.bvh_triangles[:60]]
        groups.append((base.meshes[0]["material"], tl))
    flat = [((x, 0.0, z), (x + 1.0, 0.0, z), (x, 0.0, z + 1.0)) for x in range(-2, 2) for z in range(-8, -4)]
    groups.append((base.meshes[0]["material"], flat))
    return scenes._finish("coincident", base.uniforms.copy(), base.spheres, base.lights, groups)


@pytest.mark.parametrize("kw", [dict(), dict(reference_walk=True)])
def test_coincident_triangles_and_rays_in_a_triangles_plane(kw):
    check_scene(_coincident_triangles(), per_triangle=True, n_random=1200, min_plane_exact=64, **kw)


def _with_uniforms(**counts):
    """an update that carries new uniforms only: every array is Keep, so the three patched counts stay as the uniforms give
    them (gpu_wrapper.rs:475-495) -- the oracle's counts_kept"""
    def mutate(e, s):
        s2 = _copy(s)
        for k, v in counts.items():
            s2.uniforms[k] = v
        e.update(RenderConfig(uniforms=Change.update(s2.uniforms)))
        return s2
    return mutate


def test_kept_sphere_count():
    s = scenes.feature_scene(width=32, height=24)
    assert len(s.spheres) > 2
    check_scene(s, n_random=600, counts_kept=_oracle.KEPT_SPHERES, mutate=_with_uniforms(spheres_count=2))


@pytest.mark.parametrize("kw", [dict(), dict(reference_walk=True)])
def test_kept_triangle_and_node_counts(kw):
    s = scenes.mesh_scene(12, 12, 40, 30, 1, 4, seed=3)
    nt, nn = len(s.bvh_triangles), len(s.bvh_nodes)
    assert nn > 3
    # triangles with an id beyond the count are skipped (:336): the prepared triangles' `valid` word
    check_scene(s, per_triangle=True, n_random=500, counts_kept=_oracle.KEPT_TRIANGLES, mutate=_with_uniforms(bvh_triangle_count=nt // 2), **kw)
    # children beyond the node count are not pushed (:376-387): another tree than the one the chunked walk was built over
    check_scene(s, per_triangle=True, n_random=500, counts_kept=_oracle.KEPT_NODES | _oracle.KEPT_TRIANGLES,
                mutate=_with_uniforms(bvh_node_count=nn - 2, bvh_triangle_count=nt - 7), **kw)


def test_after_delete_of_spheres():
    def mutate(e, s):
        e.update(RenderConfig(uniforms=Change.update(s.uniforms), spheres=Change.delete()))
        gone = _copy(s, spheres=np.zeros(0, dtype=abi.SPHERE))
        gone.uniforms["spheres_count"] = 0
        return gone
    check_scene(scenes.feature_scene(width=32, height=24), n_random=600, mutate=mutate)


def test_null_outputs_and_too_many_rays_are_refused():
    from renderbaby_amd._lib import load
    lib = load()
    e = _engine(scenes.feature_scene(width=16, height=8))
    rays, hits = (abi.Ray * 1)(), (abi.Hit * 1)()
    try:
        assert lib.rb_render_hits(e._h, None, None) == 15
        assert lib.rb_pick(e._h, 0, 0, None, None) == 15
        assert lib.rb_cast_rays(e._h, rays, 1, None, None) == 15
        assert lib.rb_cast_rays(e._h, None, 1, hits, None) == 15
        assert lib.rb_cast_rays(e._h, rays, (1 << 31) - 63, hits, None) == 18
        assert lib.rb_cast_rays(e._h, None, 0, None, None) == 0
    finally:
        e.close()


def test_every_walk_gives_the_same_records():
    """C3 and the lamp fixture at their BASELINE frame sizes, and 20 000 spheres"""
    from renderbaby_amd import refscenes
    for s in (scenes.mesh_c3().with_params(spp=1), refscenes.ref_lamp(spp=1)):
        assert s.width * s.height >= 1920 * 1080
        ref = None
        for kw in (dict(), dict(reference_walk=True), dict(host_bvh=True), dict(chunk_tree="host")):
            e = _engine(s, **kw)
            h, sf = e.render_hits(surfaces=True)
            e.close()
            if ref is None:
                ref = (h, sf)
            assert np.array_equal(h.view(np.uint32), ref[0].view(np.uint32)) and np.array_equal(sf.view(np.uint32), ref[1].view(np.uint32)), (s.name, kw)
        got = []
        for bt in ("device", "host"):   # the engine's own tree: device and host builders against each other
            e = _engine(s, with_tree=False, build_tree=bt)
            got.append(e.render_hits(surfaces=True))
            e.close()
        assert np.array_equal(got[0][0].view(np.uint32), got[1][0].view(np.uint32)) and np.array_equal(got[0][1].view(np.uint32), got[1][1].view(np.uint32))
        # against the caller's tree: the canonical tree orders a leaf's triangles by index, so an exact-t tie inside a leaf may go
        # to another triangle -- t and kind are equal whatever the ties; everything else wherever the triangle is the same
        for f in ("t", "kind"):
            assert np.array_equal(_u32(got[0][0][f]), _u32(ref[0][f])), (s.name, f)
        same = got[0][0]["prim"] == ref[0]["prim"]
        assert np.array_equal(got[0][0][same].view(np.uint32), ref[0][same].view(np.uint32))
        assert np.array_equal(got[0][1][same].view(np.uint32), ref[1][same].view(np.uint32))
        assert (got[0][0]["kind"][~same] == abi.HIT_TRIANGLE).all() and (~same).mean() < 0.01, (~same).sum()
    s = scenes.spheres_scene(n=20_000, width=112, height=112, spp=1, max_depth=4, extent=30.0)
    ref = None
    for kw in (dict(sphere_tree="device"), dict(sphere_tree="host"), dict(no_sphere_bvh=True)):
        e = _engine(s, **kw)
        h, sf = e.render_hits(surfaces=True)
        e.close()
        if ref is None:
            ref = (h, sf)
        assert np.array_equal(h.view(np.uint32), ref[0].view(np.uint32)) and np.array_equal(sf.view(np.uint32), ref[1].view(np.uint32)), kw


def test_pieces_and_small_counts():
    s = scenes.mesh_scene(12, 12, 40, 30, 1, 4, seed=3)
    e = _engine(s)
    try:
        n = (1 << 22) * 2 + 77   # three pieces
        rng = np.random.default_rng(2)
        O = np.tile(np.asarray(s.uniforms["camera"]["pos"][0], f32), (n, 1))
        D = rng.normal(size=(n, 3)).astype(f32)
        D[:, 2] = -np.abs(D[:, 2]) - f32(1.0)
        hits, surf = e.cast_rays(O, D, surfaces=True)
        for m in (1, 63, 64, 65, 4097):
            for lo in (0, (1 << 22) - 30, n - m):
                h, sf = e.cast_rays(O[lo:lo + m], D[lo:lo + m], surfaces=True)
                assert np.array_equal(h.view(np.uint32), hits[lo:lo + m].view(np.uint32)), (m, lo)
                assert np.array_equal(sf.view(np.uint32), surf[lo:lo + m].view(np.uint32)), (m, lo)
        assert len(e.cast_rays(O[:0], D[:0])) == 0
        assert (hits["kind"] == abi.HIT_TRIANGLE).sum() > n // 10
    finally:
        e.close()


def test_pick_shards_and_the_multi_device_handle():
    s = scenes.feature_scene(width=40, height=36)
    e = _engine(s)
    whole_h, whole_s = e.render_hits(surfaces=True)
    for px, py in ((0, 0), (39, 35), (17, 20), (5, 30)):
        h, sf = e.pick(px, py)
        assert h.tobytes() == whole_h[py, px].tobytes() and sf.tobytes() == whole_s[py, px].tobytes()
    with pytest.raises(Exception) as ei:
        e.pick(40, 0)
    assert ei.value.code == 18
    e.close()
    for rank in range(3):
        p = _engine(s, shard_rank=rank, shard_count=3, stripe_rows=8)
        h, sf = p.render_hits(surfaces=True)
        owned, padded = p.local_rows()
        assert h.shape == (padded, 40)
        for lr in range(padded):
            y = p.global_row(lr)
            if y < 36:
                assert h[lr].tobytes() == whole_h[y].tobytes() and sf[lr].tobytes() == whole_s[y].tobytes(), (rank, lr)
            else:
                assert (h[lr]["kind"] == abi.HIT_INVALID).all()
        hp, _ = p.pick(17, 20)   # any global pixel
        assert hp.tobytes() == whole_h[20, 17].tobytes()
        p.close()
    g = _engine(s, devices=[0, 0], gather_peer_copy=True)
    h, sf = g.render_hits(surfaces=True)
    assert h.shape == (36, 40) and np.array_equal(h.view(np.uint32), whole_h.view(np.uint32)) and np.array_equal(sf.view(np.uint32), whole_s.view(np.uint32))
    assert g.pick(5, 30)[0].tobytes() == whole_h[30, 5].tobytes()
    g.close()


def test_a_query_between_iterator_frames_keeps_the_pass_run_ahead():
    s = scenes.feature_scene(width=48, height=32, spp=4)
    rc = RenderConfig.from_scene(s)

    def frames(query):
        e = Engine.new(rc, device=0)
        it = e.frame_iterator(rc)
        out, kernel = [], None
        while it.has_next():
            out.append(it.next().pixels.copy())
            if query:
                kernel = e.last_kernel_name()
                e.render_hits(surfaces=True)
                e.pick(3, 4)
                assert e.last_kernel_name() == kernel   # rb_last_kernel_name is the render's
        st = e.stats()
        e.close()
        return out, st
    plain, st0 = frames(False)
    asked, st1 = frames(True)
    assert len(plain) == len(asked) == 4
    for a, b in zip(plain, asked):
        assert np.array_equal(a, b)
    for k in ("segments", "paths", "launches"):   # the run-ahead pass was kept, not traced again; queries count nothing
        assert st0[k] == st1[k], k


def test_a_refused_update_leaves_queries_answering_for_the_previous_scene():
    s = scenes.feature_scene(width=32, height=24)
    e = _engine(s)
    try:
        before = e.render_hits(surfaces=True)
        bad = s.bvh_nodes.copy()
        bad["left"][0] = 0   # a cycle: refused by validation
        bad["right"][0] = 0
        bad["primitive_count"][0] = 0
        with pytest.raises(Exception):
            e.update(RenderConfig(bvh_nodes=Change.create(bad)))
        after = e.render_hits(surfaces=True)
        assert np.array_equal(before[0].view(np.uint32), after[0].view(np.uint32)) and np.array_equal(before[1].view(np.uint32), after[1].view(np.uint32))
    finally:
        e.close()


def test_page_locked_outputs():
    from renderbaby_amd._lib import load
    s = scenes.feature_scene(width=32, height=24)
    e = _engine(s)
    lib = load()
    n = 32 * 24
    p = lib.rb_host_alloc(n * 48)
    assert p
    try:
        pinned = np.ctypeslib.as_array((C.c_uint8 * (n * 48)).from_address(p)).view(abi.HIT)
        ref = e.render_hits()
        O, D = pixel_centre_rays(s)
        e.cast_rays(O.reshape(-1, 3), D.reshape(-1, 3) * f32(3), hits_out=pinned)
        pageable = e.cast_rays(O.reshape(-1, 3), D.reshape(-1, 3) * f32(3))
        assert np.array_equal(pinned.view(np.uint32), pageable.view(np.uint32))
        assert (pinned["kind"] == ref.reshape(-1)["kind"]).all()
    finally:
        e.close()
        lib.rb_host_free(p)
