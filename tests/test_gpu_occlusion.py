"""Any-hit occlusion queries (rb_occluded) and the device forms (rb_occluded_device / rb_cast_rays_device); DESIGN.md section 12.
Every comparison is exact and no ray is left out.

The yardstick is the identity with the closest-hit query, which tests/test_gpu_query.py pins to the oracle bit for bit: with
RB_MASK_ALL, out[i] == OCCLUDED exactly when rb_cast_rays(...)[i].t < tmax[i].  It is asked at the sharpest tmax there is --
the hit's own t (VISIBLE: the comparison is strict) and the next float above it (OCCLUDED) -- so half of the hitting rays lie
on each side of the answer by one ulp.  One check goes to the oracle without rb_cast_rays in between.
"""
import ctypes as C

import numpy as np
import pytest

from renderbaby_amd import Engine, RenderConfig, abi, aov, scenes
from tests import _oracle
from tests.conftest import has_gpu
from tests.test_gpu_query import (_coincident_triangles, _copy, _engine, _identical_spheres, _normalize, _with_uniforms, id_scene,
                                  oracle_emissive, pixel_centre_rays, plane_rays, random_rays, FAR_LIGHT, SKY_ID)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

f32 = np.float32
VIS, OCC, INV = abi.OCCL_VISIBLE, abi.OCCL_OCCLUDED, abi.OCCL_INVALID
KERNELS = ("k_occl", "k_occl_bvh", "k_occl_chunk")


def identity_cases(hits, seed=5):
    """the four (tmax, expected bytes) of the identity for the closest-hit records `hits`"""
    t, kind = hits["t"].astype(f32), hits["kind"]
    hit, invalid = (kind != abi.HIT_NONE) & (kind != abi.HIT_INVALID), kind == abi.HIT_INVALID
    rnd = (np.random.default_rng(seed).random(len(t)).astype(f32) * f32(2.0) * np.minimum(t, f32(1e19))).astype(f32)

    def expect(occluded):
        return np.where(invalid, INV, np.where(occluded, OCC, VIS)).astype(np.uint8)
    return [("t", t, expect(np.zeros(len(t), bool))),
            ("t+", np.nextafter(t, f32(np.inf)), expect(hit)),
            ("random", rnd, expect(hit & (t < np.minimum(rnd, f32(1e20))))),
            ("null", None, expect(hit))]


def check_identity(e, O, D, label, tally=None):
    """rb_occluded against rb_cast_rays of the same engine on the rays (O, D); returns the answers of the four cases.
    `tally`: [rays, rays that hit something] of the scene, counted up."""
    O, D = np.ascontiguousarray(O, f32).reshape(-1, 3), np.ascontiguousarray(D, f32).reshape(-1, 3)
    hits = e.cast_rays(O, D)
    hit = (hits["kind"] != abi.HIT_NONE) & (hits["kind"] != abi.HIT_INVALID)
    print(f"{label}: {len(O)} rays, {hit.mean():.3f} hit")
    if tally is not None:
        tally[0] += len(O)
        tally[1] += int(hit.sum())
    got = []
    for name, tmax, want in identity_cases(hits):
        out = e.occluded(O, D, tmax)
        assert e.last_query_kernel_name() in KERNELS
        bad = np.nonzero(out != want)[0]
        assert len(bad) == 0, (label, name, len(bad), bad[:5], out[bad[:5]], want[bad[:5]], hits[bad[:5]])
        got.append(out)
    return got


def ray_sets(scene, n_random=1500):
    """the ray sets of test_gpu_query.py: pixel centres, the same scaled by 3 and 2^-20, random rays (axis-parallel, zero and
    non-finite directions among them), rays in the plane of a triangle"""
    O, D = pixel_centre_rays(scene)
    O, D = O.reshape(-1, 3), D.reshape(-1, 3)
    sets = [("pixels", O, D), ("pixels x3", O, (D * f32(3.0)).astype(f32)), ("pixels x2^-20", O, (D * f32(2.0 ** -20)).astype(f32))]
    sets.append(("random",) + random_rays(scene, n_random, 11))
    if len(scene.bvh_triangles):
        sets.append(("in-plane",) + plane_rays(scene)[:2])
    return sets


def check_scene(scene, n_random=1500, mutate=None, **kw):
    e = _engine(scene, **kw)
    try:
        if mutate is not None:
            scene = mutate(e, scene)
        st0 = e.stats()
        tally = [0, 0]
        for name, O, D in ray_sets(scene, n_random):
            check_identity(e, O, D, f"{scene.name} {name}", tally)
        assert tally[1] * 4 >= tally[0], ("fewer than a quarter of the scene's rays hit something", tally)
        assert e.stats() == st0, "queries moved rb_get_stats"
        return e.last_query_kernel_name()
    finally:
        e.close()


# ---- 1. the identity
@pytest.mark.parametrize("color_hash", [0, 1])
def test_identity_feature_scene(color_hash):
    assert check_scene(scenes.feature_scene(width=48, height=32, color_hash=color_hash)) in KERNELS


def test_identity_cornell_with_the_phantom_light():
    s = scenes.cornell(48, 36, 1, 4)
    assert len(s.lights) == 0
    assert check_scene(s) == "k_occl"


@pytest.mark.parametrize("kw", [dict(sphere_tree="device"), dict(sphere_tree="host"), dict(no_sphere_bvh=True)])
def test_identity_identical_spheres(kw):
    assert check_scene(_identical_spheres(), n_random=600, **kw) == ("k_occl_bvh" if "sphere_tree" in kw else "k_occl")


@pytest.mark.parametrize("kw,kernel", [(dict(), "k_occl_chunk"), (dict(reference_walk=True), "k_occl_bvh")])
def test_identity_coincident_triangles(kw, kernel):
    assert check_scene(_coincident_triangles(), n_random=1200, **kw) == kernel


def test_identity_kept_sphere_count():
    s = scenes.feature_scene(width=32, height=24)
    check_scene(s, n_random=600, mutate=_with_uniforms(spheres_count=2))


@pytest.mark.parametrize("kw", [dict(), dict(reference_walk=True)])
def test_identity_kept_triangle_and_node_counts(kw):
    s = scenes.mesh_scene(12, 12, 40, 30, 1, 4, seed=3)
    nt, nn = len(s.bvh_triangles), len(s.bvh_nodes)
    check_scene(s, n_random=500, mutate=_with_uniforms(bvh_triangle_count=nt // 2), **kw)
    check_scene(s, n_random=500, mutate=_with_uniforms(bvh_node_count=nn - 2, bvh_triangle_count=nt - 7), **kw)


def test_identity_full_size_scenes_and_every_walk_agrees():
    """C3 and the lamp fixture at their BASELINE frame sizes: the chunked walk, the reference walk, the own-tree flag, the
    host-built chunk tree and the engine-built tree each satisfy the identity against their own closest-hit records and give
    the same bytes; 20 000 spheres with both tree builders and with the scan."""
    from renderbaby_amd import refscenes
    for s in (scenes.mesh_c3().with_params(spp=1), refscenes.ref_lamp(spp=1)):
        assert s.width * s.height >= 1920 * 1080
        D = aov.pixel_centre_dirs(s.uniforms).reshape(-1, 3)
        O = np.tile(np.asarray(s.uniforms["camera"]["pos"][0], f32), (len(D), 1))
        ref = None
        walks = [(dict(), True, "k_occl_chunk"), (dict(reference_walk=True), True, "k_occl_bvh"), (dict(host_bvh=True), True, "k_occl_bvh"),
                 (dict(chunk_tree="host"), True, "k_occl_chunk"), (dict(build_tree="device"), False, "k_occl_chunk")]
        for kw, with_tree, kernel in walks:
            e = _engine(s, with_tree=with_tree, **kw)
            tally = [0, 0]
            got = check_identity(e, O, D, f"{s.name} {kw}", tally)
            assert tally[1] * 4 >= tally[0], (s.name, tally)
            assert e.last_query_kernel_name() == kernel, (kw, e.last_query_kernel_name())
            e.close()
            if ref is None:
                ref = got
            for a, b in zip(got, ref):   # (every walk reports the same t: the tmax of the four cases are the same values)
                assert np.array_equal(a, b), (s.name, kw)
    s = scenes.spheres_scene(n=20_000, width=112, height=112, spp=1, max_depth=4, extent=30.0)
    O, D = pixel_centre_rays(s)
    ref = None
    for kw in (dict(sphere_tree="device"), dict(sphere_tree="host"), dict(no_sphere_bvh=True)):
        e = _engine(s, **kw)
        tally = [0, 0]
        got = check_identity(e, O, D, f"{s.name} {kw}", tally)
        assert tally[1] * 4 >= tally[0], (s.name, tally)
        e.close()
        if ref is None:
            ref = got
        for a, b in zip(got, ref):
            assert np.array_equal(a, b), kw


# ---- 2. the oracle, without rb_cast_rays in between
def test_against_the_oracle_walk():
    """rbo_trace_ray with max_depth = 1 on the emissive-tagged copy names the winner of the oracle's own closest-hit search;
    rbo_intersect_* on that primitive gives its t; the byte must be t < tmax."""
    s = scenes.feature_scene(width=48, height=32)
    ids = id_scene(s, per_triangle=True)
    e = _engine(s)
    try:
        O, D = pixel_centre_rays(s)
        O, D = O.reshape(-1, 3), D.reshape(-1, 3)
        Or, Dr = random_rays(s, 1200, 17)
        Dn = _normalize(Dr)
        ok = np.isfinite(Or).all(1) & np.isfinite(Dn).all(1) & (Dn != 0).any(1)
        O, D = np.concatenate([O, Or[ok]]), np.concatenate([D, Dn[ok]])
        same = np.all(_normalize(D).view(np.uint32) == D.view(np.uint32), axis=1)   # the device normalises: rays it leaves as they are
        n_pix, n_rnd = 48 * 32, int(ok.sum())
        print(f"oracle check: {n_pix} pixel + {n_rnd} of 1200 random rays are valid; normalize() leaves {int(same[:n_pix].sum())} + {int(same[n_pix:].sum())} as they are")
        # (re-normalising an f32 unit vector moves a component by an ulp at most, and often none: neither part may thin out)
        assert n_rnd >= 1000 and same[:n_pix].sum() * 4 >= n_pix and same[n_pix:].sum() * 4 >= n_rnd, "the filter emptied a part of the ray set"
        O, D = O[same], D[same]
        em = oracle_emissive(ids, O, D)
        t = np.full(len(O), 1e20, f32)
        gh = float(s.uniforms["ground_height"][0])
        for i in range(len(O)):
            k = em[i]
            if tuple(k) == SKY_ID:
                continue
            if k[0] == 0:
                t[i] = _oracle.isect_ground(O[i], D[i], gh)
            elif int(k[0]) == abi.HIT_TRIANGLE:
                tri = s.bvh_triangles[int(k[1]) - 1]
                t[i] = _oracle.isect_triangle(O[i], D[i], tri["v0"], tri["v1"], tri["v2"])[0]
            else:
                p = (s.spheres if int(k[0]) == abi.HIT_SPHERE else s.lights)[int(k[1]) - 1]
                t[i] = _oracle.isect_sphere(O[i], D[i], p["center"], float(p["radius"]))
        hit = t < f32(1e20)
        assert hit.mean() >= 0.25 and len(O) > 1500
        rnd = (np.random.default_rng(3).random(len(t)).astype(f32) * f32(2.0) * np.minimum(t, f32(1e19))).astype(f32)
        for tmax, occluded in ((t, np.zeros(len(t), bool)), (np.nextafter(t, f32(np.inf)), hit), (rnd, hit & (t < rnd)), (None, hit)):
            out = e.occluded(O, D, tmax)
            assert np.array_equal(out, np.where(occluded, OCC, VIS).astype(np.uint8))
    finally:
        e.close()


# ---- 2b. the chunked walk's acceptance threshold, against the oracle's triangle test
_NEAR = {}


def _near_surface_rays():
    """129 rays that start 0.0015 from a triangle of a 578-triangle mesh (15 caller nodes, some 40 chunks of 16) and point at
    it: at its centroid, or at the middle of one of its edges, which it shares with a neighbour; every eighth points away.  Per
    ray the oracle's own t (rbo_intersect_triangle) of every triangle the ray comes near; computed once."""
    if _NEAR:
        return _NEAR["s"], _NEAR["O"], _NEAR["D"], _NEAR["T"]
    s = scenes.mesh_scene(12, 12, 40, 30, 1, 4, seed=3)
    tr = s.bvh_triangles
    v0, v1, v2 = (tr[k].astype(np.float64) for k in ("v0", "v1", "v2"))
    nrm = np.cross(v1 - v0, v2 - v0)
    area = np.linalg.norm(nrm, axis=1)
    O, D = [], []
    for j, k in enumerate(np.nonzero(area > 1e-4)[0]):
        n_ = nrm[k] / area[k]
        aim = (v0[k] + v1[k] + v2[k]) / 3.0 if j % 2 == 0 else (v1[k] + v2[k]) / 2.0
        away = j % 8 == 7
        o, d = (aim + 0.0015 * n_).astype(f32), (n_ if away else -n_).astype(f32)
        # rays the device leaves as they are (it normalises), and whose oracle t of the aimed triangle is well inside (0.001, 0.002)
        if not np.array_equal(_normalize(d).view(np.uint32), d.view(np.uint32)):
            continue
        t = _oracle.isect_triangle(o, d, tr[k]["v0"], tr[k]["v1"], tr[k]["v2"])[0]
        if away or j % 2 == 1 or 0.0012 < t < 0.0018:
            O.append(o)
            D.append(d)
        if len(O) == 129:
            break
    assert len(O) == 129
    O, D = np.array(O, f32), np.array(D, f32)
    # the oracle's t of every triangle whose plane the ray meets anywhere near the triangle (float64 prefilter, generous)
    T = []
    for o, d in zip(O.astype(np.float64), D.astype(np.float64)):
        den = nrm @ d
        with np.errstate(divide="ignore", invalid="ignore"):
            tt = np.einsum("ij,ij->i", nrm, v0 - o) / den
        p = o + tt[:, None] * d
        r = np.maximum(np.linalg.norm(v1 - v0, axis=1), np.linalg.norm(v2 - v0, axis=1))
        near = np.isfinite(tt) & (np.linalg.norm(p - v0, axis=1) <= 1.5 * r + 1e-3)
        T.append(np.array([_oracle.isect_triangle(o.astype(f32), d.astype(f32), tr[k]["v0"], tr[k]["v1"], tr[k]["v2"])[0]
                           for k in np.nonzero(near | (den == 0.0))[0]], f32))
    _NEAR.update(s=s, O=O, D=D, T=T)
    return s, O, D, T


@pytest.mark.parametrize("n", [1, 63, 65, 129])
def test_chunk_walk_accepts_hits_just_past_the_threshold(n):
    """k_occl_chunk with waves that start with lanes that never walk (1, 63, 65 and 129 rays): a hit at t = 0.0015 is a hit (the
    reference accepts t > 0.001), with tmax = 0.0019 so that nothing farther along the ray answers for it, and with no bound."""
    s, O, D, T = _near_surface_rays()
    O, D, T = O[:n], D[:n], T[:n]
    e = _engine(s)
    try:
        for bound in (f32(0.0019), None):
            tm = f32(1e20) if bound is None else bound
            want = np.array([OCC if np.any((t > f32(0.001)) & (t < tm)) else VIS for t in T], np.uint8)
            out = e.occluded(O, D, None if bound is None else np.full(n, bound, f32))
            assert e.last_query_kernel_name() == "k_occl_chunk"
            assert np.array_equal(out, want), (bound, np.nonzero(out != want)[0][:5])
            if bound is not None and n >= 63:
                assert (want == OCC).sum() * 3 >= n and (want == VIS).any()   # (the rays aimed at centroids hit by construction)
    finally:
        e.close()


# ---- 3. masks
def test_masks():
    s = scenes.feature_scene(width=48, height=32)
    empty = scenes.sky_only()

    def variant(mask):
        """the scene without the categories that `mask` leaves out; the lights cannot be removed (an empty buffer holds the
        phantom light): they become one light too far away to be hit, and the test asserts that none is"""
        v = _copy(s)
        if not mask & abi.MASK_LIGHTS:
            v = _copy(v, lights=FAR_LIGHT.copy())
        if not mask & abi.MASK_GROUND:
            v.uniforms["ground_enabled"] = 0
        if not mask & abi.MASK_SPHERES:
            v = _copy(v, spheres=np.zeros(0, dtype=abi.SPHERE))
            v.uniforms["spheres_count"] = 0
        if not mask & abi.MASK_TRIANGLES:
            v = _copy(v, meshes=empty.meshes, bvh_nodes=empty.bvh_nodes, bvh_indices=empty.bvh_indices, bvh_triangles=empty.bvh_triangles,
                      uvs=empty.uvs)
            v.uniforms["bvh_node_count"] = 0
            v.uniforms["bvh_triangle_count"] = 0
        return v
    sets = ray_sets(s, 1500)
    O, D = np.concatenate([x[1] for x in sets]), np.concatenate([x[2] for x in sets])
    full = _engine(s)
    try:
        tmax = (np.random.default_rng(9).random(len(O)).astype(f32) * f32(12.0)).astype(f32)
        for mask in (abi.MASK_GROUND, abi.MASK_TRIANGLES, abi.MASK_SPHERES, abi.MASK_LIGHTS, abi.MASK_GROUND | abi.MASK_SPHERES,
                     abi.MASK_TRIANGLES | abi.MASK_LIGHTS):
            ev = _engine(variant(mask))
            try:
                if not mask & abi.MASK_LIGHTS:
                    assert not (ev.cast_rays(O, D)["kind"] == abi.HIT_LIGHT).any(), mask
                for tm in (None, tmax):
                    got = full.occluded(O, D, tm, mask)
                    assert np.array_equal(got, ev.occluded(O, D, tm)), (mask, tm is None)
                    assert (got == OCC).any() and (got == VIS).any(), mask
            finally:
                ev.close()
        out = full.occluded(O, D, None, 0)
        valid = full.cast_rays(O, D)["kind"] != abi.HIT_INVALID
        assert (out[valid] == VIS).all() and (out[~valid] == INV).all() and (~valid).sum() >= 3
        with pytest.raises(Exception) as ei:
            full.occluded(O, D, None, 16)
        assert ei.value.code == 18
    finally:
        full.close()


# ---- 4. edge values
def test_edge_values_of_tmax_and_invalid_rays():
    s = scenes.feature_scene(width=16, height=8)
    e = _engine(s)
    try:
        o = np.asarray(s.uniforms["camera"]["pos"][0], f32)
        down = np.array([0, -1, 0], f32)   # the ground at t = 2 (or a sphere before it)
        t0 = e.cast_rays(o[None], down[None])[0]["t"]
        assert f32(0.001) < t0 < f32(100)
        near = np.nextafter(f32(0.001), f32(np.inf))
        tm = np.array([np.nan, np.inf, -np.inf, -1, 0, 0.001, near, 1e20, t0, np.nextafter(t0, f32(np.inf))], f32)
        want = [INV, OCC, VIS, VIS, VIS, VIS, VIS, OCC, VIS, OCC]
        out = e.occluded(np.tile(o, (len(tm), 1)), np.tile(down, (len(tm), 1)), tm)
        assert out.tolist() == want
        # invalid rays, whatever their tmax
        bad = np.array([[0, 0, 0], [np.nan, 0, 1], [1e25, -3e24, 2e20], [np.inf, 0, 0]], f32)
        for tmv in (None, np.full(4, 5.0, f32), np.full(4, np.nan, f32), np.full(4, -1.0, f32)):
            assert (e.occluded(np.tile(o, (4, 1)), bad, tmv) == INV).all()
        assert (e.occluded(np.full((1, 3), np.nan, f32), down[None]) == INV).all()
    finally:
        e.close()


def test_counts_pieces_and_page_locked_outputs():
    from renderbaby_amd._lib import load
    lib = load()
    s = scenes.mesh_scene(12, 12, 40, 30, 1, 4, seed=3)
    e = _engine(s)
    n = (1 << 22) + 77   # two pieces
    p = lib.rb_host_alloc(n)
    assert p
    try:
        rng = np.random.default_rng(2)
        O = np.tile(np.asarray(s.uniforms["camera"]["pos"][0], f32), (n, 1))
        D = rng.normal(size=(n, 3)).astype(f32)
        D[:, 2] = -np.abs(D[:, 2]) - f32(1.0)
        hits = e.cast_rays(O, D)
        hit = hits["kind"] != abi.HIT_NONE
        assert hit.mean() > 0.1
        tmax = np.where(np.arange(n) % 2 == 0, hits["t"], np.nextafter(hits["t"], f32(np.inf))).astype(f32)
        want = np.where(hit & (np.arange(n) % 2 == 1), OCC, VIS).astype(np.uint8)
        out = e.occluded(O, D, tmax)
        assert np.array_equal(out, want)
        pinned = np.ctypeslib.as_array((C.c_uint8 * n).from_address(p))
        pinned[:] = 77
        assert e.occluded(O, D, tmax, out=pinned) is pinned and np.array_equal(pinned, want)
        for m in (0, 1, 63, 64, 65):
            for lo in (0, (1 << 22) - 30, n - m):
                assert np.array_equal(e.occluded(O[lo:lo + m], D[lo:lo + m], tmax[lo:lo + m]), want[lo:lo + m]), (m, lo)
        rays, o1 = (abi.Ray * 1)(), (C.c_uint8 * 1)()
        assert lib.rb_occluded(e._h, None, None, 0, abi.MASK_ALL, None) == 0
        assert lib.rb_occluded(e._h, None, None, 1, abi.MASK_ALL, o1) == 15
        assert lib.rb_occluded(e._h, rays, None, 1, abi.MASK_ALL, None) == 15
        assert lib.rb_occluded(e._h, rays, None, (1 << 31) - 63, abi.MASK_ALL, o1) == 18
    finally:
        e.close()
        lib.rb_host_free(p)


# ---- 5. the device forms
def _device_forms(e, s, lib, n_random=3000):
    import torch
    sets = ray_sets(s, n_random) if s.width * s.height <= 4096 else []
    if sets:
        O, D = np.concatenate([x[1] for x in sets]), np.concatenate([x[2] for x in sets])
    else:
        D = aov.pixel_centre_dirs(s.uniforms).reshape(-1, 3)
        O = np.tile(np.asarray(s.uniforms["camera"]["pos"][0], f32), (len(D), 1))
    hits, surf = e.cast_rays(O, D, surfaces=True)
    tmax = np.where(np.arange(len(O)) % 2 == 0, hits["t"], np.nextafter(hits["t"], f32(np.inf))).astype(f32)
    dev = torch.device("cuda", 0)
    tO, tD, tT = torch.from_numpy(O).to(dev), torch.from_numpy(D).to(dev), torch.from_numpy(tmax).to(dev)
    dh, ds = e.cast_rays(tO, tD, surfaces=True)
    assert dh.is_cuda and ds.is_cuda and dh.shape == (len(O), 12)
    assert e.last_query_kernel_name().startswith("k_query") and e.last_query_ms() > 0
    assert np.array_equal(dh.cpu().numpy().view(np.uint32).reshape(-1), hits.view(np.uint32).reshape(-1))
    assert np.array_equal(ds.cpu().numpy().view(np.uint32).reshape(-1), surf.view(np.uint32).reshape(-1))
    assert np.array_equal(e.cast_rays(tO, tD).cpu().numpy().view(np.uint32).reshape(-1), hits.view(np.uint32).reshape(-1))
    for tm_h, tm_d in ((tmax, tT), (None, None)):
        for mask in (abi.MASK_ALL, abi.MASK_TRIANGLES | abi.MASK_GROUND):
            got = e.occluded(tO, tD, tm_d, mask)
            assert got.is_cuda and got.dtype == torch.uint8
            assert e.last_query_kernel_name() in KERNELS and e.last_query_ms() > 0
            assert np.array_equal(got.cpu().numpy(), e.occluded(O, D, tm_h, mask))
    return tO, tD


def test_device_forms_equal_the_host_forms():
    import torch
    from renderbaby_amd._lib import load
    lib = load()
    for s in (scenes.feature_scene(width=48, height=32), scenes.mesh_c3().with_params(spp=1)):
        e = _engine(s)
        try:
            tO, tD = _device_forms(e, s, lib)
            if s.width * s.height > 4096:
                continue
            # refusals: a host pointer, a misaligned pointer, a wrong dtype, a tensor that is not contiguous
            rays = e._ray_records(tO, tD)
            n = len(rays)
            out = torch.empty(n + 16, dtype=torch.uint8, device=rays.device)
            host_rays, host_out = np.zeros(n, dtype=abi.RAY), np.zeros(n, np.uint8)
            hits = torch.empty((n, 12), dtype=torch.float32, device=rays.device)
            assert lib.rb_occluded_device(e._h, host_rays.ctypes.data, None, n, abi.MASK_ALL, out.data_ptr()) == 18
            assert lib.rb_occluded_device(e._h, rays.data_ptr(), None, n, abi.MASK_ALL, host_out.ctypes.data) == 18
            assert lib.rb_occluded_device(e._h, rays.data_ptr() + 4, None, n - 1, abi.MASK_ALL, out.data_ptr()) == 18
            assert lib.rb_occluded_device(e._h, rays.data_ptr(), None, n, 16, out.data_ptr()) == 18
            assert lib.rb_occluded_device(e._h, rays.data_ptr(), None, n, abi.MASK_ALL, out.data_ptr() + 3) == 0   # bytes need no alignment
            assert lib.rb_sync(e._h) == 0
            assert np.array_equal(out[3:3 + n].cpu().numpy(), e.occluded(tO, tD).cpu().numpy())
            assert lib.rb_cast_rays_device(e._h, host_rays.ctypes.data, n, hits.data_ptr(), None) == 18
            assert lib.rb_cast_rays_device(e._h, rays.data_ptr(), n - 1, hits.data_ptr() + 8, None) == 18
            assert lib.rb_cast_rays_device(e._h, rays.data_ptr(), n, hits.data_ptr(), hits.data_ptr() + 4) == 18
            assert lib.rb_cast_rays_device(e._h, None, 1, hits.data_ptr(), None) == 15
            assert lib.rb_cast_rays_device(e._h, None, 0, None, None) == 0 and lib.rb_occluded_device(e._h, None, None, 0, 0, None) == 0
            for bad in (lambda: e.occluded(tO.double(), tD.double()), lambda: e.occluded(tO.cpu(), tD.cpu(), torch.ones(n)),
                        lambda: e.occluded_records(rays.t().contiguous().t()), lambda: e.occluded_records(rays, out=torch.empty(n, device=rays.device)),
                        lambda: e.cast_ray_records(rays, hits_out=np.empty(n, dtype=abi.HIT)),
                        lambda: e.cast_ray_records(np.zeros(n, abi.RAY), hits_out=np.empty(n - 1, abi.HIT)),
                        lambda: e.cast_ray_records(np.zeros(n, abi.RAY), hits_out=np.empty(n, abi.RADIANCE))):
                with pytest.raises(ValueError):
                    bad()
        finally:
            e.close()


def test_device_forms_on_an_engine_of_the_current_device():
    """device = -1: the engine takes the device that is current at creation, and so do the tensors it accepts"""
    import torch
    from renderbaby_amd._lib import load
    s = scenes.feature_scene(width=40, height=36)
    rc = RenderConfig.from_scene(s)
    e = Engine.new(rc)   # device=-1
    try:
        assert e.query_device == torch.cuda.current_device() == 0
        e.update(rc)
        _device_forms(e, s, load(), n_random=800)
    finally:
        e.close()


def test_device_forms_on_a_sharded_engine_and_a_multi_device_handle():
    from renderbaby_amd._lib import load
    s = scenes.feature_scene(width=40, height=36)
    for kw in (dict(shard_rank=1, shard_count=3, stripe_rows=8), dict(devices=[0, 0], gather_peer_copy=True)):
        e = _engine(s, **kw)
        try:
            _device_forms(e, s, load(), n_random=800)
        finally:
            e.close()


# ---- 6. non-interference
def test_an_occlusion_query_between_iterator_frames_changes_nothing():
    import torch
    s = scenes.feature_scene(width=48, height=32, spp=4)
    rc = RenderConfig.from_scene(s)
    O, D = pixel_centre_rays(s)
    O, D = O.reshape(-1, 3), D.reshape(-1, 3)

    def frames(query):
        e = Engine.new(rc, device=0)
        it = e.frame_iterator(rc)
        out = []
        while it.has_next():
            out.append(it.next().pixels.copy())
            if query:
                kernel = e.last_kernel_name()
                assert (e.occluded(O, D) != INV).all()
                e.occluded(torch.from_numpy(O).cuda(), torch.from_numpy(D).cuda(), torch.full((len(O),), 3.0, device="cuda"))
                assert e.last_query_kernel_name() in KERNELS
                assert e.last_kernel_name() == kernel   # rb_last_kernel_name is the render's
        st = e.stats()
        e.close()
        return out, st
    plain, st0 = frames(False)
    asked, st1 = frames(True)
    assert len(plain) == len(asked) == 4
    for a, b in zip(plain, asked):
        assert np.array_equal(a, b)
    timed = {k for k in st0 if k.endswith("_ms") or k.endswith("_s") or "time" in k}
    print("stats compared:", sorted(set(st0) - timed), "left out as times:", sorted(timed))
    assert set(st0) == set(st1) and len(set(st0) - timed) >= 3
    for k in set(st0) - timed:   # every counter rb_get_stats reports; only measured times may differ between two runs
        assert st0[k] == st1[k], k


# ---- 7. ambient occlusion
def test_ambient_occlusion_of_open_ground_and_of_a_closed_cube():
    ground = scenes.sky_only(width=48, height=32)
    ground.uniforms["ground_enabled"] = 1
    ground.uniforms["ground_height"] = 0.0
    ground.uniforms["camera"]["dir"] = (0, -0.5, -1)
    e = _engine(ground)
    try:
        hits = e.render_hits()
        on_ground = hits["kind"] == abi.HIT_GROUND
        assert on_ground.sum() > 48 * 32 // 4
        ao = aov.ambient_occlusion(e, hits, n_dirs=16, radius=5.0)
        assert ao.shape == hits.shape and ao.dtype == np.float32 and (ao == f32(1.0)).all()
    finally:
        e.close()
    c = 3.0   # the cube [-3, 3]^3 about the camera, two triangles per face
    q = scenes._quad
    faces = [q((-c, -c, -c), (c, -c, -c), (c, c, -c), (-c, c, -c)), q((-c, -c, c), (c, -c, c), (c, c, c), (-c, c, c)),
             q((-c, -c, -c), (-c, -c, c), (-c, c, c), (-c, c, -c)), q((c, -c, -c), (c, -c, c), (c, c, c), (c, c, -c)),
             q((-c, -c, -c), (c, -c, -c), (c, -c, c), (-c, -c, c)), q((-c, c, -c), (c, c, -c), (c, c, c), (-c, c, c))]
    u = scenes.make_uniforms(48, 32, 1, 4, cam_pos=(0.3, 0.2, 0.1), cam_dir=(0.2, -0.1, -1.0), ground_enabled=0, sky=(0.5, 0.7, 1.0))
    cube = scenes._finish("cube", u, np.zeros(0, dtype=abi.SPHERE), np.zeros(0, dtype=abi.POINT_LIGHT),
                          [(scenes.material(), [t for f in faces for t in f])])
    e = _engine(cube)
    try:
        hits = e.render_hits()
        assert (hits["kind"] == abi.HIT_TRIANGLE).all()
        ao = aov.ambient_occlusion(e, hits, n_dirs=16, radius=float(2 * c * np.sqrt(3.0)) + 1.0)
        assert (ao == f32(0.0)).all(), (ao != 0).sum()
        assert aov.ao_u8(ao).shape == hits.shape + (4,)
    finally:
        e.close()
