"""Lightmap texels made on the device (rb_lightmap_surfels / rb_lightmap_resolve / rb_bake_lightmap and their device forms;
DESIGN.md section 17), bit for bit on uint32 views:

  the generator = the numpy model renderbaby_amd/lightmap.py: the owner and all eight words of every surfel;
  the resolve   = the model, with empty texels inside charts;
  the bake      = rb_trace_hemisphere over the surfels rb_lightmap_surfels returned, then rb_lightmap_resolve of those sums;
  the forms and the pieces give the same answers, and a call has a query's side effects: none;
  a baked map handed back as a texture is what the engine then shades with.
"""

import numpy as np
import pytest

from renderbaby_amd import Change, Engine, RenderConfig, abi, bake, engine, lightmap, scenes
from tests import _lightmap_scenes as lms
from tests import _oracle
from tests.conftest import has_gpu
from tests.test_gpu_query import _engine
from tests.test_lightmap_abi import INVALID_OPTIONS, NULL_ARGUMENT, REFUSALS, _params

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

f32 = np.float32
NO = abi.LIGHTMAP_NO_OWNER
ATLASES = [(1, 1), (7, 5), (8, 8), (9, 17), (64, 64), (65, 63)]


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_surfels_equal(got, want, where):
    (gs, go), (ws, wo) = got, want
    assert go.dtype == np.uint32 and go.shape == wo.shape and gs.shape == ws.shape, where
    bad = np.nonzero(go != wo)[0]
    assert len(bad) == 0, (where, "owners", len(bad), bad[:5], go[bad[:5]], wo[bad[:5]])
    g, w = _u32(gs).reshape(-1, 8), _u32(ws).reshape(-1, 8)
    bad = np.nonzero((g != w).any(1))[0]
    assert len(bad) == 0, (where, "surfels", len(bad), bad[:5], gs[bad[:5]], ws[bad[:5]])


def special():
    names, tris, meshes = lms.special_triangles()
    return names, lms.uv_triangles(tris, meshes)


# ---- 1. the generator against the model
@pytest.mark.parametrize("width,height", ATLASES, ids=[f"{w}x{h}" for w, h in ATLASES])
def test_generator_equals_the_model(width, height):
    names, (tris, uvs) = special()
    owned = set()
    for mesh, flip in ((None, False), (0, False), (1, True)):
        got = engine.lightmap_surfels_device(tris, uvs, width, height, mesh=mesh, flip=flip, device=0)
        want = lightmap.surfels(tris, uvs, width, height, mesh=mesh, flip=flip)
        assert_surfels_equal(got, want, ("special", width, height, mesh, flip))
        assert (_u32(got[0]).reshape(-1, 8)[got[1] == NO] == 0).all()
        owned |= set(np.unique(got[1]).tolist())
        if mesh is not None:
            assert all(int(tris["mesh_index"][k]) == mesh for k in np.unique(got[1]) if k != NO)
    if (width, height) == (64, 64):   # the cases are laid out for this atlas: each does there what its name says
        own = engine.lightmap_surfels_device(tris, uvs, 64, 64, device=0)[1].reshape(64, 64)
        k = {n: i for i, n in enumerate(names)}
        never = ("wholly outside, uv > 1", "wholly outside, uv < 0", "zero uv area", "a NaN uv", "smaller than a texel, no centre inside")
        assert not any((own == k[n]).any() for n in never)
        assert (own != NO).all(), "the first triangle covers the whole atlas, so every texel has an owner"
        rest = engine.lightmap_surfels_device(tris[1:], uvs, 64, 64, device=0)[1].reshape(64, 64)   # without it: indices shift by one
        r = {n: i - 1 for n, i in k.items()}
        assert (rest == r["smaller than a texel, a centre inside"]).sum() == 1 and rest[50, 30] == r["smaller than a texel, a centre inside"]
        e, nb = r["centres on an edge and on vertices"], r["its neighbour across the diagonal"]
        assert rest[4, 40] == e and rest[4, 50] == e and rest[14, 40] == e     # centres exactly on its three vertices
        assert all(rest[4 + j, 50 - j] == e for j in range(11))                 # and on the shared diagonal: the lower index
        assert rest[14, 50] == nb and (rest == nb).sum() == 55
        assert (rest[36:60, 48:62] == r["overlapping, second"]).any() and rest[48, 50] == r["overlapping, first"]
        assert (rest == r["the other mesh"]).any()
        assert (rest[:, 63] == r["partly outside"]).any()
        alone = engine.lightmap_surfels_device(tris[1:], uvs, 64, 64, mesh=1, device=0)[1]   # what the lower indices took from it
        assert 0 < (rest == r["the other mesh, over the first"]).sum() < (alone == r["the other mesh, over the first"]).sum()
    # triangle counts round the wave and block edges of k_lm_count and the scan
    for m in (1, 63, 65, 130):
        t, u = lms.uv_triangles(lms.many_triangles(m))
        assert_surfels_equal(engine.lightmap_surfels_device(t, u, width, height, device=0), lightmap.surfels(t, u, width, height), ("many", m, width, height))


def test_uv_indices_shared_and_past_the_end():
    """an indexed mesh's shared uv pairs, and indices past the end of uvs, which read 0"""
    rng = np.random.default_rng(11)
    q = [lms.quad_triangles(lms.convex_quad(rng), k % 2, k % 4 >= 2)[0] for k in range(8)]
    tris, uvs = lms.uv_triangles([t for pair in q for t in pair], shared=True)
    assert_surfels_equal(engine.lightmap_surfels_device(tris, uvs, 33, 31, device=0), lightmap.surfels(tris, uvs, 33, 31), "shared")
    short = uvs[:len(uvs) // 2 + 1]   # an odd length: one index reads u and not v
    tris["v2_index"][3] = 0xFFFFFFFF   # 2 i wraps in uint32
    tris["v1_index"][5] = 0x80000001   # 2 i wraps to 2
    got = engine.lightmap_surfels_device(tris, short, 33, 31, device=0)
    assert_surfels_equal(got, lightmap.surfels(tris, short, 33, 31), "past the end")
    assert (got[1] != NO).any()
    none = engine.lightmap_surfels_device(tris, np.zeros(0, f32), 33, 31, device=0)   # no uvs at all: every corner is (0, height)
    assert (none[1] == NO).all() and (_u32(none[0]) == 0).all()


def test_cover_pieces(monkeypatch):
    """enough units to cross a cover piece boundary: equal to the model, and equal under a forced small piece size"""
    _, (tris, uvs) = special()
    t2, u2 = lms.uv_triangles(lms.many_triangles(130))
    t2["v0_index"] += len(uvs) // 2
    t2["v1_index"] += len(uvs) // 2
    t2["v2_index"] += len(uvs) // 2
    tris, uvs = np.concatenate([tris, t2]), np.concatenate([uvs, u2])
    want = lightmap.surfels(tris, uvs, 65, 63)
    whole = engine.lightmap_surfels_device(tris, uvs, 65, 63, device=0)
    assert_surfels_equal(whole, want, "default pieces")
    for units in ("1", "7", "64"):
        monkeypatch.setenv("RB_LIGHTMAP_PIECE_UNITS", units)
        assert_surfels_equal(engine.lightmap_surfels_device(tris, uvs, 65, 63, device=0), want, ("pieces of", units))
    monkeypatch.delenv("RB_LIGHTMAP_PIECE_UNITS")
    # a default piece boundary itself: 2^20 units is a 8192 x 8192 atlas under one triangle; its owners are all that triangle
    big, ub = lms.uv_triangles([[(-1.0, -1.0), (3.0, -1.0), (-1.0, 3.0)], [(0.25, 0.25), (0.5, 0.25), (0.25, 0.5)]])
    import torch
    e = _engine(lms.uv_scene(big, ub))
    try:
        n = 8200 * 8200
        surf, own = torch.empty((n, 8), dtype=torch.float32, device="cuda"), torch.empty((n,), dtype=torch.int32, device="cuda")
        e.lightmap_surfels(8200, 8200, out=(surf, own))
        assert (own == 0).all().item()
        assert e.last_lightmap_ms()[0] > 0
    finally:
        e.close()


# ---- 2. the engine form
def test_engine_form_equals_engine_less_form():
    import torch
    _, (tris, uvs) = special()
    s = lms.uv_scene(tris, uvs, n_meshes=2)
    e = _engine(s)
    try:
        st0 = e.stats()
        for (w, h), mesh, flip in (((64, 64), None, False), ((65, 63), 1, True), ((7, 5), 0, False), ((1, 1), None, True)):
            want = engine.lightmap_surfels_device(tris, uvs, w, h, mesh=mesh, flip=flip, device=0)
            surf = torch.full((w * h, 8), 7.0, dtype=torch.float32, device="cuda")
            own = torch.full((w * h,), 7, dtype=torch.int32, device="cuda")
            rs, ro = e.lightmap_surfels(w, h, mesh=mesh, flip=flip, out=(surf, own))
            assert rs is surf and ro is own
            got = surf.cpu().numpy().view(abi.SURFEL).reshape(-1), own.cpu().numpy().view(np.uint32)
            assert_surfels_equal(got, want, ("engine", w, h, mesh, flip))
            assert e.last_query_kernel_name() == "k_lm_surfels" and e.last_query_ms() > 0
            sm, rm = e.last_lightmap_ms()
            assert 0 < sm <= e.last_query_ms() and rm == 0
            assert_surfels_equal(e.lightmap_surfels(w, h, mesh=mesh, flip=flip), want, ("engine, numpy", w, h))
            e.lightmap_surfels(w, h, mesh=mesh, flip=flip, out=(surf, None))   # owners left out
            assert np.array_equal(_u32(surf.cpu().numpy()), _u32(want[0]).reshape(-1, 8))
        # a triangle the walks skip owns nothing: a uniforms-only update keeps the caller's shorter count in force
        for count in (len(tris) - 2, 1, 0):
            u = s.uniforms.copy()
            u["bvh_triangle_count"] = count
            e.update(RenderConfig(uniforms=Change.update(u)))
            got = e.lightmap_surfels(64, 64)
            assert_surfels_equal(got, lightmap.surfels(tris, uvs, 64, 64, tri_count=count), ("count", count))
            assert (got[1][got[1] != NO] < count).all() and ((got[1] != NO).any() == (count > 0))
        assert e.stats() == st0, "lightmap queries moved rb_get_stats"
    finally:
        e.close()


# ---- 3. the resolve
def chart_sums(w, h, seed=2):
    """sums with charts, gaps and w = 0 texels inside the charts"""
    rng = np.random.default_rng(seed)
    s = np.zeros(w * h, dtype=abi.RADIANCE)
    s["sum"] = rng.uniform(0, 50, (w * h, 3)).astype(f32)
    weight = rng.integers(1, 17, w * h).astype(f32)
    ys, xs = np.divmod(np.arange(w * h), w)
    weight[((xs // 5 + ys // 4) % 3 == 0) & (w * h > 1)] = 0     # the gutters between charts
    weight[rng.uniform(size=w * h) < 0.05] = 0                  # holes inside charts
    if w * h > 1:
        weight[0] = 3
    s["weight"] = weight
    return s


@pytest.mark.parametrize("width,height", [(1, 1), (1, 9), (9, 1), (65, 63)])
def test_resolve_equals_the_model(width, height):
    s = chart_sums(width, height)
    assert width * height == 1 or ((s["weight"] == 0).any() and (s["weight"] > 0).any())
    for dilate in (0, 1, 2, 64):
        got = engine.lightmap_resolve(s, width, height, dilate, device=0)
        want = lightmap.resolve(s, width, height, dilate)
        bad = np.argwhere((_u32(got) != _u32(want)).any(-1))
        assert len(bad) == 0, (width, height, dilate, len(bad), bad[:5])
    empty = np.zeros(width * height, dtype=abi.RADIANCE)
    assert (_u32(engine.lightmap_resolve(empty, width, height, 64, device=0)) == 0).all()


# ---- 4. the bake
BAKE_SCENES = {"cube": lms.cube_scene, "mesh578": lms.mesh578}


@pytest.fixture(scope="module", params=list(BAKE_SCENES))
def baked(request):
    """an engine per scene, shared by the bake tests; the surfels of both atlases from the engine-less form"""
    s = BAKE_SCENES[request.param]()
    e = _engine(s)
    surf = {(w, h): engine.lightmap_surfels_device(s.bvh_triangles, s.uvs, w, h, device=0) for w, h in ((16, 16), (33, 31))}
    yield request.param, s, e, surf
    e.close()


def test_bake_equals_its_stages(baked):
    import torch
    name, s, e, surf = baked
    st0 = e.stats()
    lit = 0
    for (w, h), (sf, own) in surf.items():
        assert (own != NO).any() and ((name, w) != ("mesh578", 33) or (own == NO).any()), (name, w, h)
        for samples, first_sample in ((1, 0), (5, 0), (5, 7), (1, 7)):
            sums = np.zeros(w * h, dtype=abi.RADIANCE)
            rgba = e.bake_lightmap(w, h, samples, first_sample=first_sample, dilate=2, sums=sums)
            assert e.last_query_kernel_name().startswith("k_cam") and e.last_query_ms() > 0
            sm, rm = e.last_lightmap_ms()
            assert sm > 0 and rm > 0 and sm + rm <= e.last_query_ms()
            want = e.trace_hemisphere(sf["pos"], sf["normal"], samples, first_sample)
            where = (name, w, h, samples, first_sample)
            assert np.array_equal(_u32(sums), _u32(want)), where
            assert (sums["weight"] == np.where(own != NO, samples, 0)).all(), where
            assert rgba.shape == (h, w, 4) and np.array_equal(_u32(rgba), _u32(engine.lightmap_resolve(sums, w, h, 2, device=0))), where
            lit += int((sums["sum"] != 0).any(1).sum())
            # the device form on torch tensors
            d_rgba = torch.full((w * h, 4), 7.0, dtype=torch.float32, device="cuda")
            d_sums = torch.full((w * h, 4), 7.0, dtype=torch.float32, device="cuda")
            assert e.bake_lightmap(w, h, samples, first_sample=first_sample, dilate=2, out=d_rgba, sums=d_sums) is d_rgba
            assert np.array_equal(_u32(d_rgba.cpu().numpy()), _u32(rgba).reshape(-1, 4)) and np.array_equal(_u32(d_sums.cpu().numpy()), _u32(sums).reshape(-1, 4)), where
            # either output alone, and the other dilate counts
            assert np.array_equal(_u32(e.bake_lightmap(w, h, samples, first_sample=first_sample, dilate=0)), _u32(lightmap.resolve(sums, w, h, 0)))
            only = torch.full((w * h, 4), 7.0, dtype=torch.float32, device="cuda")
            assert e.bake_lightmap(w, h, samples, first_sample=first_sample, dilate=1, sums=only) is only
            assert np.array_equal(_u32(only.cpu().numpy()), _u32(sums).reshape(-1, 4))
    assert lit > 0, "no texel of the scene carried any light"
    assert e.stats() == st0, "lightmap bakes moved rb_get_stats"


def test_two_calls_accumulated_equal_one(baked):
    """the ordered sum of samples 0 .. 5 is the sum of samples 0 .. 4 plus sample 5: one more float32 addition per component"""
    name, s, e, surf = baked
    w, h = 33, 31
    a, b, one = (np.zeros(w * h, dtype=abi.RADIANCE) for _ in range(3))
    e.bake_lightmap(w, h, 5, first_sample=3, sums=a)
    e.bake_lightmap(w, h, 1, first_sample=8, sums=b)
    rgba = e.bake_lightmap(w, h, 6, first_sample=3, sums=one)
    acc = np.zeros(w * h, dtype=abi.RADIANCE)
    acc["sum"], acc["weight"] = (a["sum"] + b["sum"]).astype(f32), (a["weight"] + b["weight"]).astype(f32)
    assert np.array_equal(_u32(acc), _u32(one)), name
    assert np.array_equal(_u32(engine.lightmap_resolve(acc, w, h, 2, device=0)), _u32(rgba))
    assert np.array_equal(_u32(bake.lightmap(e, w, h, 6, first_sample=3)), _u32(rgba))


def test_a_bake_between_iterator_frames():
    s = lms.cube_scene().with_params(spp=4)
    rc = RenderConfig.from_scene(s)

    def frames(query):
        e = Engine.new(rc, device=0)
        it = e.frame_iterator(rc)
        out, answers = [], []
        while it.has_next():
            out.append(it.next().pixels.copy())
            if query:
                kernel = e.last_kernel_name()
                answers.append(e.bake_lightmap(16, 16, 3))
                assert e.last_kernel_name() == kernel
        acc, st = e.read_accumulation(), e.stats()
        e.close()
        return out, acc, st, answers
    plain, acc0, st0, _ = frames(False)
    asked, acc1, st1, answers = frames(True)
    assert len(plain) == len(asked) == 4
    for a, b in zip(plain, asked):
        assert np.array_equal(a, b)
    assert np.array_equal(_u32(acc0), _u32(acc1))
    assert all(st0[k] == st1[k] for k in st0 if not k.endswith("_ms")), (st0, st1)
    for m in answers[1:]:
        assert np.array_equal(_u32(m), _u32(answers[0]))
    assert (answers[0][..., 3] == 1).any()


def test_refusals_leave_the_engine_rendering_the_golden_frame():
    import torch
    from renderbaby_amd._lib import load
    lib = load()
    s = scenes.cornell(32, 32, 2, 4)
    rc = RenderConfig.from_scene(s)
    e = Engine.new(rc, device=0)
    try:
        e.update(rc)
        h = e._h
        base = _params()   # 4 x 3
        rgba, sums = np.full(48, 7, dtype=f32), np.full(12, 7, dtype=abi.RADIANCE)
        d_rgba = torch.full((12, 4), 7.0, dtype=torch.float32, device="cuda")
        d_sums = torch.full((12, 4), 7.0, dtype=torch.float32, device="cuda")
        d_surf = torch.full((12, 8), 7.0, dtype=torch.float32, device="cuda")
        d_own = torch.full((12,), 7, dtype=torch.int32, device="cuda")
        calls = [lambda p, fs=0, n=2: lib.rb_bake_lightmap(h, p, fs, n, rgba.ctypes.data, sums.ctypes.data),
                 lambda p, fs=0, n=2: lib.rb_bake_lightmap_device(h, p, fs, n, d_rgba.data_ptr(), d_sums.data_ptr()),
                 lambda p, fs=0, n=2: lib.rb_lightmap_surfels_device(h, p, d_surf.data_ptr(), d_own.data_ptr())]
        for k, call in enumerate(calls):
            for name, fields in REFUSALS:
                assert call(_params(**fields).ctypes.data) == INVALID_OPTIONS, (k, name)
                assert lib.rb_last_error(h)
            assert call(None) == NULL_ARGUMENT
            if k < 2:   # the limits on the samples are rb_trace_hemisphere's
                for fs, n in ((0, 0), (0, 65537), (0xFFFFFFFF, 1), (0xFFFFFFFE, 2)):
                    assert call(base.ctypes.data, fs, n) == INVALID_OPTIONS, (k, fs, n)
                assert call(_params(width=16384, height=16384).ctypes.data, 0, 8) == INVALID_OPTIONS   # 2^28 texels x 8 samples
        bp = base.ctypes.data
        assert lib.rb_bake_lightmap(h, bp, 0, 2, None, None) == NULL_ARGUMENT and lib.rb_bake_lightmap_device(h, bp, 0, 2, None, None) == NULL_ARGUMENT
        assert lib.rb_lightmap_surfels_device(h, bp, None, d_own.data_ptr()) == NULL_ARGUMENT
        # the device forms' buffers: a host pointer, a misaligned one, an allocation that ends before width * height records
        assert lib.rb_bake_lightmap_device(h, bp, 0, 2, rgba.ctypes.data, None) == INVALID_OPTIONS
        assert lib.rb_bake_lightmap_device(h, bp, 0, 2, d_rgba.data_ptr(), sums.ctypes.data) == INVALID_OPTIONS
        assert lib.rb_bake_lightmap_device(h, bp, 0, 2, d_rgba.data_ptr() + 4, None) == INVALID_OPTIONS
        large = _params(width=2048, height=2048).ctypes.data   # (beyond the block the tensors' allocator carved them from)
        assert lib.rb_bake_lightmap_device(h, large, 0, 2, d_rgba.data_ptr(), None) == INVALID_OPTIONS
        assert lib.rb_bake_lightmap_device(h, large, 0, 2, None, d_sums.data_ptr()) == INVALID_OPTIONS
        assert lib.rb_lightmap_surfels_device(h, bp, rgba.ctypes.data, None) == INVALID_OPTIONS
        assert lib.rb_lightmap_surfels_device(h, bp, d_surf.data_ptr() + 8, None) == INVALID_OPTIONS
        assert lib.rb_lightmap_surfels_device(h, bp, d_surf.data_ptr(), d_own.data_ptr() + 2) == INVALID_OPTIONS
        assert lib.rb_lightmap_surfels_device(h, large, d_surf.data_ptr(), None) == INVALID_OPTIONS
        lib.rb_sync(h)
        assert (rgba == 7).all() and (_u32(sums) == f32(7).view(np.uint32)).all()
        assert all((t == 7).all().item() for t in (d_rgba, d_sums, d_surf, d_own))
        # Cornell carries no uvs: every corner is (0, height), no triangle has uv area, and the map is RB_OK and all empty
        got = e.bake_lightmap(4, 3, 2, sums=sums)
        assert (_u32(got) == 0).all() and (_u32(sums) == 0).all()
        assert np.array_equal(e.render(rc).pixels, _oracle.render(s)[2])
    finally:
        e.close()
    cold = Engine.new(rc, device=0)   # no update yet: not ready, and still a refusal first
    try:
        out = np.zeros(48, dtype=f32)
        assert lib.rb_bake_lightmap(cold._h, base.ctypes.data, 0, 2, out.ctypes.data, None) not in (0, INVALID_OPTIONS)
        assert lib.rb_bake_lightmap(cold._h, base.ctypes.data, 0, 0, out.ctypes.data, None) == INVALID_OPTIONS
        assert np.array_equal(cold.render(rc).pixels, _oracle.render(s)[2])
    finally:
        cold.close()
    # an engine without triangles
    bare = _engine(scenes.sky_only())
    try:
        assert (_u32(bare.bake_lightmap(9, 5, 2)) == 0).all()
        sf, own = bare.lightmap_surfels(9, 5)
        assert (own == NO).all() and (_u32(sf) == 0).all()
    finally:
        bare.close()


def test_sharded_engine_and_multi_device_handle():
    s = lms.cube_scene()
    e = _engine(s)
    want = e.bake_lightmap(16, 16, 2, first_sample=7)
    e.close()
    for kw in (dict(shard_rank=1, shard_count=3, stripe_rows=8), dict(devices=[0, 0], gather_peer_copy=True)):
        p = _engine(s, **kw)
        try:
            assert np.array_equal(_u32(p.bake_lightmap(16, 16, 2, first_sample=7)), _u32(want)), kw
            assert p.last_query_ms() > 0 and p.last_lightmap_ms()[0] > 0
        finally:
            p.close()


# ---- 5. the point of it
def test_a_baked_map_is_the_texture_the_engine_then_shades_with():
    """The cube example under its sky: its textured -z face owns the whole atlas (the +z face has the same uvs and the higher
    indices); the cube carries no uvs on its top.  Bake with the normals turned outwards, hand the map back as the skin texture,
    and a ray at the centre of a texel's surfel returns the albedo the texel's baked value encodes."""
    w = h = 32
    s = lms.cube_scene()
    e = _engine(s)
    try:
        rgba = bake.lightmap(e, w, h, 64, flip=True, dilate=2)
        sf, own = e.lightmap_surfels(w, h, flip=True)
        assert (own < 2).all(), "the first face's two triangles own the atlas"
        assert (rgba[..., 3] == 1).all() and (rgba[..., :3] > 0).all(), "every texel sees the sky"
        # no empty texel beside a baked one after two passes (here: no empty texel at all)
        empty = rgba[..., 3] == 0
        baked_ = np.pad(rgba[..., 3] == 1, 1)
        near = np.zeros_like(empty)
        for dx, dy in lightmap.NEIGHBOURS:
            near |= baked_[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
        assert not (empty & near).any()
        tex = bake.lightmap_texture(rgba)
        assert tex.shape == (h, w) and tex.dtype == np.uint32
        e.update(RenderConfig(uniforms=Change.update(s.uniforms), textures=Change.update([(w, h, tex.reshape(-1))])))
        n = sf["normal"]
        hits, surf = e.cast_rays((sf["pos"] + f32(0.5) * n).astype(f32), -n, surfaces=True)
        print("triangles hit:", np.unique(hits["prim"], return_counts=True), "t:", hits["t"].min(), hits["t"].max())
        # The 32 centres on the face's diagonal lie on the edge its two triangles share: there the walk's own triangle test may
        # take either triangle, or neither and go on to the +z face, which carries the same uvs.  Everywhere else the ray meets
        # the texel's owner; the albedo below is asked of all 1024.
        assert (hits["kind"] == abi.HIT_TRIANGLE).all() and (hits["mesh"] == 0).all()
        off_diagonal = np.arange(w * h) % w + np.arange(w * h) // w != w - 1   # the edge runs from (0, 32) to (32, 0) in texels
        assert (hits["prim"][off_diagonal] == own[off_diagonal]).all() and (np.abs(hits["t"][off_diagonal] - 0.5) < 1e-3).all()
        assert (surf["flags"] & abi.SURFACE_USE_TEXTURE).all() and (surf["texture_index"] == 0).all()
        enc = lambda c: np.clip(c.astype(np.float64), 0, 1) ** (1 / 2.2)   # noqa: E731
        err = np.abs(enc(surf["albedo"]) - enc(rgba[..., :3].reshape(-1, 3)))
        print("largest encoding error:", err.max(), "of", 1 / 255)
        assert err.max() <= 1 / 255
        assert len(np.unique(tex)) > 8, "the map is not one flat colour"
    finally:
        e.close()
