"""The scenes and rays of tests/_edge_scenes.py on the oracle alone (no GPU): every edge the GPU comparison of
tests/test_gpu_shading_edges.py relies on is shown to be REACHED -- by the oracle's own walk, uv and texture sample --
before any device is asked.  The coverage conditions live here as functions; the GPU test asserts the same ones on
the same rays, so a silent miss cannot pass there as agreement.
"""
import ctypes as C

import numpy as np

from renderbaby_amd import abi
from tests import _edge_scenes as es
from tests import _oracle
from tests.test_gpu_query import SKY_ID, Stages, _normalize, id_scene, oracle_emissive, sample_texture, tri_uv

f32 = np.float32
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31
# sphere / light winners of aimed_rays() that inherit a uv from the quad behind them, as this module measures them on the
# oracle (test_aimed_rays_reach_every_edge asserts them exactly); the GPU test asks check_records for at least as many
INHERITED_SPHERES, INHERITED_LIGHTS = 207, 63


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def oracle_winners(scene, O, Dn):
    """What the oracle's walk picks for every ray and the uv / use_texture the shader then holds: a list of dicts
    (kind, prim, uv, tex, use_texture).  The winner comes from rbo_trace_ray on the identification scene (one mesh per
    triangle), t (u, v) from rbo_intersect_*, the inherited uv of a sphere or light from the staged walks of Stages."""
    ids = id_scene(scene, per_triangle=True)
    ids.uniforms["color_hash_enabled"] = 0   # (does not move the winner)
    em = oracle_emissive(ids, O, Dn)
    stages = Stages(scene, 0)
    hashed = int(scene.uniforms["color_hash_enabled"][0]) != 0
    gh = float(scene.uniforms["ground_height"][0])
    out = []
    for o, d, e in zip(O, Dn, em):
        if tuple(e) == SKY_ID:
            out.append(dict(kind=abi.HIT_NONE, prim=-1, uv=None, tex=-1, use_texture=False))
        elif e[0] == 0:
            t = f32(_oracle.isect_ground(o, d, gh))
            pos = (o + t * d).astype(f32)
            out.append(dict(kind=abi.HIT_GROUND, prim=-1, uv=np.array([pos[0], pos[2]], f32), tex=-1, use_texture=True, t=t))
        elif int(e[0]) == abi.HIT_TRIANGLE:
            i = int(e[1]) - 1
            tri = scene.bvh_triangles[i]
            _, u, v = _oracle.isect_triangle(o, d, tri["v0"], tri["v1"], tri["v2"])
            tex = int(scene.meshes[int(tri["mesh_index"])]["material"]["texture_index"])
            out.append(dict(kind=abi.HIT_TRIANGLE, prim=i, uv=tri_uv(scene, tri, f32(u), f32(v)), tex=-1 if hashed else tex,
                            use_texture=(tex >= 0 and not hashed)))
        else:
            kind, i = int(e[0]), int(e[1]) - 1
            mat = (scene.spheres if kind == abi.HIT_SPHERE else scene.lights)[i]["material"]
            uv, _ = stages.after_bvh(o, d)
            use = stages.after_spheres(o, d) if kind == abi.HIT_LIGHT else int(mat["texture_index"]) >= 0
            out.append(dict(kind=kind, prim=i, uv=uv, tex=int(mat["texture_index"]), use_texture=bool(use)))
    return out


def texel_of(tex, uv):
    """rb_oracle.c:121-126 in numpy binary32 -> (x, y, x before the clamp, y before the clamp)"""
    w, h, _ = tex
    u, v = f32(uv[0] - np.floor(uv[0])), f32(uv[1] - np.floor(uv[1]))
    x, y = int(f32(u * f32(w))), int(f32(f32(f32(1.0) - v) * f32(h)))
    return min(x, w - 1), min(y, h - 1), x, y


def oracle_pow_table(os_bytes):
    """the oracle's pow(k / 255, 2.2f) for k = 0..255: R of the all-bytes texture (texel k has R = k) at every texel's centre"""
    tab = np.zeros(256, f32)
    for k in range(256):
        tab[k] = sample_texture(os_bytes, es.ALL_BYTES, ((k % 16 + 0.5) / 16.0, 1.0 - (k // 16 + 0.5) / 16.0))[0]
    return tab


def edge_conditions(scene, O, Dn, Q):
    """The coverage of aimed_rays(), from the oracle alone.  -> dict of what was reached."""
    assert int(scene.uniforms["color_hash_enabled"][0]) == 0
    os_ = _oracle.OracleScene(scene)
    tab = oracle_pow_table(os_)
    win = oracle_winners(scene, O, Dn)
    quad_of_tri = {}
    for name in es.QUAD_INDEX:
        for t in es.quad_triangles(scene, name):
            quad_of_tri[t] = name
    c = dict(sampled=set(), bytes_texels=set(), wins={n: 0 for n in es.QUAD_INDEX}, x_clamp={n: 0 for n in es.QUAD_INDEX},
             y_clamp={n: 0 for n in es.QUAD_INDEX}, straddle_first=0, inherited_spheres=0, inherited_lights=0, kinds=set(),
             interior_integer=0, black=0)
    for w_ in win:
        c["kinds"].add(w_["kind"])
        if w_["kind"] == abi.HIT_SPHERE:
            c["inherited_spheres"] += int(w_["uv"].any())
        elif w_["kind"] == abi.HIT_LIGHT:
            c["inherited_lights"] += int(w_["uv"].any() and w_["use_texture"])
        if w_["kind"] != abi.HIT_TRIANGLE or w_["prim"] not in quad_of_tri:
            continue
        name = quad_of_tri[w_["prim"]]
        c["wins"][name] += 1
        c["straddle_first"] += int(w_["prim"] == es.quad_triangles(scene, "uv_straddle")[0] and bool(w_["uv"].any()))
        rgb = sample_texture(os_, w_["tex"], w_["uv"])
        if not 0 <= w_["tex"] < len(scene.textures):
            assert w_["tex"] >= len(scene.textures) and not rgb.any()   # the stand-in: black
            c["black"] += 1
            continue
        tex = scene.textures[w_["tex"]]
        x, y, xr, yr = texel_of(tex, w_["uv"])
        word = int(tex[2][y * tex[0] + x])
        # ties this module's texel arithmetic to what the oracle really sampled
        assert np.array_equal(_u32(rgb), _u32(np.array([tab[word & 255], tab[(word >> 8) & 255], tab[(word >> 16) & 255]], f32))), (name, x, y)
        c["sampled"].add(w_["tex"])
        if w_["tex"] == es.ALL_BYTES:
            c["bytes_texels"].add((x, y))
        c["x_clamp"][name] += int(xr >= tex[0])
        c["y_clamp"][name] += int(yr >= tex[1])
        c["interior_integer"] += int(name.startswith("integer_") and float(w_["uv"][0]) in (0.0, 1.0) and float(w_["uv"][1]) in (0.0, 1.0))
    return c


def assert_edge_conditions(c):
    assert c["sampled"] == set(range(es.N_TEX)), c["sampled"]                       # every texture, so every offset
    assert len(c["bytes_texels"]) == 256                                            # every entry of the table, three times over
    for name in ("oob_ntex", "oob_ntex5", "oob_max", "uv_beyond", "uv_straddle"):
        assert c["wins"][name] >= 1, name
    assert c["black"] >= 3 and c["straddle_first"] >= 1
    for name, (_, tex, uvr, _) in zip(es.QUAD_INDEX, es.ALL_QUADS):
        if not 0 <= tex < es.N_TEX:
            continue
        # fract(u) < 1 unless the subtraction rounds: the x clamp is reachable on the `below` quads only.  The y clamp wants
        # fract(v) == 0, an integer v exactly: every quad has it but tex0 (v in [0.25, 0.75]), below_* (v in [-1e-9, 0.5]: -1e-9
        # wraps to 1.0, row 0) and tiled_* (the range [-2.5, 3.25] puts integers at t = (4 n + 10) / 23, no binary fraction, so the
        # interpolated v only comes near them; integer_* carries exact integers on the same two textures).  uv_straddle reaches it
        # through its guard: the v of vertices 1 and 2 reads 0, so v = 0 along that edge.
        if name.startswith("below_"):
            assert c["x_clamp"][name] >= 1, name
        if not name.startswith(("tex0", "below_", "tiled_")):
            assert c["y_clamp"][name] >= 1, name
    assert c["interior_integer"] >= 2
    assert c["inherited_spheres"] >= INHERITED_SPHERES and c["inherited_lights"] >= INHERITED_LIGHTS, (c["inherited_spheres"], c["inherited_lights"])
    assert {abi.HIT_TRIANGLE, abi.HIT_SPHERE, abi.HIT_LIGHT} <= c["kinds"]


def _f2i(x):
    if np.isnan(x):
        return 0
    return I32_MAX if x >= 2147483648.0 else I32_MIN if x <= -2147483648.0 else int(x)


def far_conditions(scene, O, Dn):
    """The classes of far_ground_rays() by the oracle's own uv (shader.wgsl:160-166) -> dict of counts"""
    os_ = _oracle.OracleScene(scene)
    u = scene.uniforms[0]
    c = dict(plain=0, saturated=0, beyond=0, infinite=0, dy_exact=0, dy_refused=0, neg_odd=0, neg_even=0, wraps=0, colours=set())
    for o, d, w_ in zip(O, Dn, oracle_winners(scene, O, Dn)):
        at_threshold = abs(d[1]) == es.DY_MIN
        if w_["kind"] != abi.HIT_GROUND:
            assert abs(d[1]) == np.nextafter(es.DY_MIN, f32(0)), d   # nothing but the ground test's threshold turns a ray away
            c["dy_refused"] += 1
            continue
        c["dy_exact"] += int(at_threshold)
        uv = w_["uv"]
        with np.errstate(over="ignore"):
            s10 = [f32(uv[0] * f32(10.0)), f32(uv[1] * f32(10.0))]
        u2, v2 = _f2i(np.floor(s10[0])), _f2i(np.floor(s10[1]))
        total = u2 + v2
        s32 = (total + 2 ** 31) % 2 ** 32 - 2 ** 31
        odd = s32 % 2 != 0   # C: sum % 2 is -1 for a negative odd sum, so `== 0` is what decides
        exp = u["checkerboard_color_2"] if odd else u["checkerboard_color_1"]
        assert np.array_equal(_u32(sample_texture(os_, -1, uv)), _u32(exp)), (uv, u2, v2)
        c["colours"].add(bool(odd))
        big = float(np.abs(uv).max())
        c["infinite"] += int(np.isinf(s10).any())
        c["plain"] += int(big < 2 ** 31 / 10)
        c["saturated"] += int(2 ** 31 / 10 <= big < 2 ** 31)
        c["beyond"] += int(big >= 2 ** 31 and not np.isinf(s10).any())
        c["neg_odd"] += int(s32 < 0 and odd)
        c["neg_even"] += int(s32 < 0 and not odd)
        c["wraps"] += int(total != s32)
    return c


def assert_far_conditions(c):
    for k in ("plain", "saturated", "beyond", "infinite", "dy_exact", "dy_refused", "neg_odd", "neg_even", "wraps"):
        assert c[k] >= 2, (k, c)
    assert c["colours"] == {False, True}


# ------------------------------------------------------------------ tests ---
def test_scene_layout():
    s = es.texture_edges_scene()
    assert len(s.bvh_nodes) > 1 and len(s.textures) == es.N_TEX and len(s.lights) == 2
    assert [(w, h) for w, h, _ in s.textures] == [(1, 1), (1, 7), (5, 1), (3, 5), (16, 16), (8, 4), (257, 3)]
    offs = np.cumsum([0] + [w * h for w, h, _ in s.textures[:-1]])
    assert offs.tolist() == [0, 1, 8, 13, 28, 284, 316]
    for w, h, d in s.textures:
        assert len(d) == w * h and ((d >> 24) != 0).all()
    _, _, d = s.textures[es.ALL_BYTES]
    for sh in (0, 8, 16):
        assert sorted(((d >> sh) & 255).tolist()) == list(range(256))
    assert s.uvs[0] != 0 and s.uvs[1] != 0
    # the cut: of uv_straddle's first triangle vertex 0 and u of vertex 1 are inside, the rest of the tail is beyond the end
    t0 = es.quad_triangles(s, "uv_straddle")[0]
    i0, i1, i2 = (int(s.bvh_triangles[t0][k]) for k in ("v0_index", "v1_index", "v2_index"))
    assert i0 * 2 + 1 < len(s.uvs) and i1 * 2 < len(s.uvs) <= i1 * 2 + 1 and i2 * 2 >= len(s.uvs)
    for t in es.quad_triangles(s, "uv_beyond"):
        assert int(s.bvh_triangles[t]["v0_index"]) * 2 >= len(s.uvs)
    for name, (_, tex, _, _) in zip(es.QUAD_INDEX, es.ALL_QUADS):
        for t in es.quad_triangles(s, name):
            assert int(s.meshes[int(s.bvh_triangles[t]["mesh_index"])]["material"]["texture_index"]) == tex, name
    assert [int(s.meshes[es.QUAD_INDEX[n]]["material"]["texture_index"]) for n in ("oob_ntex", "oob_ntex5", "oob_max")] == [7, 12, 2 ** 31 - 1]


def test_threshold_materials_sit_on_both_sides():
    tr = es.threshold_triples()
    T = es.T
    for fam in ("aaa", "00x", "ab0"):
        lo, hi = es.strength(tr[fam + "_below"]), es.strength(tr[fam + "_above"])
        assert lo < T < hi and hi == np.nextafter(lo, f32(1)) or (fam + "_equal" in tr and np.nextafter(lo, f32(1)) == T == np.nextafter(hi, f32(0)))
    equal = [k for k in tr if k.endswith("_equal")]
    assert equal, "no family reaches 0.01f exactly: `>` and `>=` could not be told apart"
    for k in equal:
        assert es.strength(tr[k]) == T
    # (0, 0, x): x / 3 alone decides -- the sum adds nothing, the division's rounding is all there is
    assert tr["00x_below"][0] == 0 and tr["00x_below"][1] == 0
    names = [n for n, _ in es.threshold_materials()]
    assert len(names) == len(set(names)) == 2 * len(tr) + len(es.SHININESS)
    sh = np.array(es.SHININESS, f32)
    assert np.isnan(sh).sum() == 1 and np.isinf(sh).sum() == 1 and (sh < 0).any() and f32(999.99994) < f32(1000.0) < f32(1000.0001)


def test_aimed_rays_reach_every_edge(capsys):
    s = es.texture_edges_scene()
    O, D, Q = es.aimed_rays(s)
    assert np.array_equal(_u32(_normalize(D)), _u32(D))
    c = edge_conditions(s, O, D, Q)
    assert_edge_conditions(c)
    assert (c["inherited_spheres"], c["inherited_lights"]) == (INHERITED_SPHERES, INHERITED_LIGHTS)
    with capsys.disabled():
        print(f"\n[shading edges] {len(O)} aimed rays; inherited uv: {c['inherited_spheres']} sphere and {c['inherited_lights']} light winners; "
              f"x clamps {sum(c['x_clamp'].values())}, y clamps {sum(c['y_clamp'].values())}")


def test_threshold_rays_hit_their_spheres():
    s = es.texture_edges_scene()
    O, D, idx = es.threshold_rays(s)
    win = oracle_winners(s, O, D)
    assert [w["kind"] for w in win] == [abi.HIT_SPHERE] * len(O) and [w["prim"] for w in win] == idx.tolist()
    assert all(w["uv"].any() for w in win)   # the backdrop behind them: a textured non-metal has a texel to multiply with


def test_far_ground_rays_reach_every_class(capsys):
    s = es.texture_edges_scene()
    O, D = es.far_ground_rays()
    Dn = _normalize(D)
    assert np.isfinite(Dn).all()
    c = far_conditions(s, O, Dn)
    assert_far_conditions(c)
    with capsys.disabled():
        print(f"\n[shading edges] {len(O)} far-ground rays: {c}")


def test_oracle_pow_table_against_float64(capsys):
    """rbo_sample_texture's powf(c / 255, 2.2f) against numpy float64 pow rounded to binary32.  Where the two differ the ORACLE's
    value stands (it is what the shader's restatement computes with this libm); the count is printed.  Every entry must be
    within one binary32 step of the float64 value: a table that is off is caught here, without a GPU."""
    os_ = _oracle.OracleScene(es.texture_edges_scene())
    tab = oracle_pow_table(os_)
    c = (np.arange(256, dtype=f32) / f32(255.0)).astype(f32)
    ref = (c.astype(np.float64) ** np.float64(f32(2.2))).astype(f32)
    differ = int((_u32(tab) != _u32(ref)).sum())
    steps = np.abs(_u32(tab).astype(np.int64) - _u32(ref).astype(np.int64))
    assert steps.max() <= 1, steps.max()
    assert tab[0] == 0 and tab[255] == 1 and (np.diff(tab) > 0).all()
    # G and B of the same texels go through the same table
    for k in (0, 1, 77, 254, 255):
        rgb = sample_texture(os_, es.ALL_BYTES, ((k % 16 + 0.5) / 16.0, 1.0 - (k // 16 + 0.5) / 16.0))
        assert rgb[1] == tab[(k * 7 + 3) & 255] and rgb[2] == tab[255 - k]
    with capsys.disabled():
        print(f"\n[shading edges] powf vs float64 pow rounded to f32: {differ} of 256 entries differ (the oracle's stand)")


def test_frames_are_finite_and_see_the_scene():
    """the frames the GPU test compares: no NaN in the oracle's accumulation (NaN payloads are outside the numerics contract).  The
    64 x 48 frame is the one that runs fuzz and the metal branch: its primary rays alone meet the ground, the wall, the
    backdrop, the spheres in front and EVERY threshold sphere (each shininess, each metal).  (The 37 x 23 frames are there for an
    odd size and, with the low camera, for ground and sky to the horizon; they see few of the spheres or none.)"""
    for kw in (dict(width=64, height=48), dict(width=37, height=23), dict(width=37, height=23, camera="low")):
        for ch in (0, 1):
            s = es.texture_edges_scene(spp=3, depth=6, color_hash=ch, **kw)
            acc, _, rgba, st = _oracle.render(s)
            assert np.isfinite(acc).all() and st["segments"] > 3 * s.width * s.height
    from tests.test_gpu_query import is_metal, pixel_centre_rays
    s = es.texture_edges_scene(64, 48)
    O, D = pixel_centre_rays(s)
    win = oracle_winners(s, O.reshape(-1, 3), D.reshape(-1, 3))
    assert {abi.HIT_NONE, abi.HIT_GROUND, abi.HIT_TRIANGLE, abi.HIT_SPHERE} <= {w["kind"] for w in win}
    seen = {w["prim"] for w in win if w["kind"] == abi.HIT_SPHERE}
    metals = 0
    for k, (name, m) in enumerate(es.threshold_materials()):
        if name.startswith("shininess_") or is_metal(m):
            assert len(es.FRONT) + k in seen, name
            metals += int(is_metal(m))
    assert metals >= len(es.SHININESS) + 4, metals   # every shininess, and the metal side of each threshold family
