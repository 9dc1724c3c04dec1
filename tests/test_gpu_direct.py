"""Direct light at surface points (rb_scene_emitters / rb_light_rays / rb_direct_light and their device forms; DESIGN.md section
21), bit for bit on uint32 views:

  the table     = the numpy model renderbaby_amd/direct.py, and each record's emission what rb_cast_rays reports for its primitive;
  the generator = the model: origin, direction and pad words of every record, every bound, every contribution;
  the sums      = direct.fold of the model's contributions under rb_occluded's bytes on the generator's own records and bounds
                  (rb_occluded is held to the oracle in tests/test_gpu_occlusion.py), once per walk;
  the forms and the pieces give the same answers, a call has a query's side effects: none, and the first call after an update
  sees the new scene.  The estimator itself is held to the path tracer: rb_trace_hemisphere at max_depth = 1.
"""
import ctypes as C

import numpy as np
import pytest

from renderbaby_amd import Change, Engine, RenderConfig, abi, bake, direct, engine, hemisphere, scenes
from tests import _oracle
from tests.conftest import has_gpu
from tests.test_direct_abi import INVALID_OPTIONS, MASK_REFUSALS, NULL_ARGUMENT, REFUSALS, _params
from tests.test_direct_model import SAMPLES, compare_estimators, floor_points, lit_cornell, seeds_drawing
from tests.test_gpu_hemisphere import _mesh_beside_spheres, model_surfels, scene_surfels
from tests.test_gpu_query import _copy, _engine
from tests.test_gpu_radiance import _mesh, _u32, given_seeds

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

f32, u32 = np.float32, np.uint32
PIECE = abi.HEMI_PIECE_ITEMS
NO_LIGHTS = abi.MASK_ALL & ~abi.MASK_LIGHTS
M = 130   # two blocks of 64 surfels and a part


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def lamps():
    """more than 64 spheres, so the engine walks its sphere tree, a few of them emissive"""
    s = scenes.spheres_scene(n=300, width=40, height=40, spp=1, max_depth=4, extent=5.0)
    sp = s.spheres.copy()
    for k in (7, 150, 299):
        sp["material"]["emissive"][k] = (30.0, 20.0 + k, 10.0)
    return scenes.Scene(s.uniforms, sp, s.lights, s.meshes, s.bvh_nodes, s.bvh_indices, s.bvh_triangles, s.uvs, name="lamps")


def long_table():
    """20 003 candidates, five blocks of the table's 32-bit scan (4096 flags a block on gfx950: 256 threads of 16 items,
    rocPRIM's default_scan_config_base): the 1 % of emissive spheres the scene draws for itself, emission set on the spheres 0, 1,
    4095, 4096, 4097, 9999 and 19999 -- the ends of the list and either side of the first block edge --, and after the spheres
    three lights of which the middle one is dark"""
    s = scenes.spheres_scene(n=20000, width=24, height=16, spp=1, max_depth=4, extent=40.0)
    sp = s.spheres.copy()
    for k in (0, 1, 4095, 4096, 4097, 9999, 19999):
        sp["material"]["emissive"][k] = (3.0 + k, 2.0, 1.0)
    lights = np.zeros(3, dtype=abi.POINT_LIGHT)
    lights["center"], lights["radius"] = [(-30.0, 40.0, 0.0), (0.0, 45.0, 5.0), (30.0, 40.0, -5.0)], (1.0, 2.0, 0.5)
    lights["material"]["emissive"] = [(50.0, 40.0, 30.0), (0.0, 0.0, 0.0), (10.0, 20.0, 30.0)]
    return scenes.Scene(s.uniforms, sp, lights, s.meshes, s.bvh_nodes, s.bvh_indices, s.bvh_triangles, s.uvs, name="long table")


def mixed_surfels(e, scene):
    """130 hit points of the scene with model_surfels' special ones -- the invalid ones among them -- mixed in"""
    pts, nrm = scene_surfels(e, scene, M)
    bad_p, bad_n = model_surfels(M)
    mixed = np.arange(M) % 3 == 1
    pts[mixed], nrm[mixed] = bad_p[mixed], bad_n[mixed]
    return pts, nrm


# ---- 1. the table
TABLE_SCENES = {"feature": lambda: scenes.feature_scene(width=24, height=16), "feature, colour hash": lambda: scenes.feature_scene(width=24, height=16, color_hash=1),
                "cornell": lambda: scenes.cornell(32, 32, 1, 4), "no emitter": scenes.sky_only, "mesh": _mesh, "lamps": lamps, "long table": long_table}


@pytest.mark.parametrize("name", list(TABLE_SCENES))
def test_table_equals_the_model_in_both_forms(name):
    import torch
    s = TABLE_SCENES[name]()
    want = direct.scene_emitters(s)
    e = _engine(s)
    try:
        st0 = e.stats()
        # the call that builds reports its kernel time; once the table stands a call reports 0
        count = C.c_size_t(99)
        assert e._lib.rb_scene_emitters(e._h, None, 0, C.byref(count)) == 0 and count.value == len(want)
        assert e.last_query_kernel_name() == "k_emit_scatter" and e.last_query_ms() > 0
        assert e._lib.rb_scene_emitters(e._h, None, 0, C.byref(count)) == 0 and count.value == len(want) and e.last_query_ms() == 0
        got = e.scene_emitters()
        assert e.last_query_kernel_name() == "k_emit_scatter" and e.last_query_ms() == 0
        assert got.dtype == abi.EMITTER and len(got) == len(want) and np.array_equal(_bytes(got), _bytes(want)), (name, got, want)
        assert (len(want) == 0) == (name == "no emitter")
        assert np.array_equal(_bytes(e.scene_emitters()), _bytes(want))   # the table stands: the same again
        lib, n = e._lib, len(want)
        for cap in sorted({0, 1, max(n - 1, 0), n, n + 3}):
            # host form: min(count, capacity) records, the count always the total, nothing behind them touched
            buf = np.zeros(cap + 1, dtype=abi.EMITTER)
            buf.view(u32)[:] = 0x07070707
            count = C.c_size_t(99)
            assert lib.rb_scene_emitters(e._h, buf.ctypes.data if cap else None, cap, C.byref(count)) == 0 and count.value == n, (name, cap)
            k = min(cap, n)
            assert np.array_equal(_bytes(buf[:k]), _bytes(want[:k])) and (buf[k:].view(u32) == 0x07070707).all(), (name, cap)
            # device form
            t = torch.full((cap + 1, 16), 7.0, dtype=torch.float32, device="cuda")
            d_got, d_count = e.scene_emitters(out=t[:cap]) if cap else (t[:0], None)
            if cap:
                assert d_count == n and np.array_equal(_bytes(d_got.cpu().numpy()[:k]), _bytes(want[:k])) and (t[k:] == 7).all().item(), (name, cap)
        cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        assert lib.rb_scene_emitters_device(e._h, None, 0, cnt.data_ptr()) == 0 and lib.rb_sync(e._h) == 0 and int(cnt.item()) == n
        assert e.stats() == st0, "the table moved rb_get_stats"
    finally:
        e.close()


@pytest.mark.parametrize("name", ["feature", "cornell", "lamps"])
def test_emission_of_a_record_is_what_cast_rays_reports(name):
    s = TABLE_SCENES[name]()
    e = _engine(s)
    try:
        t = e.scene_emitters()
        assert len(t) >= 2
        tri = t["kind"] == abi.HIT_TRIANGLE
        n = np.cross(t["b"].astype(np.float64), t["c"].astype(np.float64))
        with np.errstate(all="ignore"):
            n = np.where(tri[:, None], n / np.linalg.norm(n, axis=1)[:, None], (0.0, 1.0, 0.0))
        centre = np.where(tri[:, None], t["a"] + (t["b"] + t["c"]) / f32(3.0), t["a"])
        gap = np.where(tri, 0.004, t["b"][:, 0] + 0.004)   # just off the primitive: nothing lies between
        org = (centre + n * gap[:, None]).astype(f32)
        hits, surf = e.cast_rays(org, (-n).astype(f32), surfaces=True)
        assert np.array_equal(hits["kind"], t["kind"]) and np.array_equal(hits["prim"], t["prim"]), (hits["kind"], hits["prim"], t["kind"], t["prim"])
        assert np.array_equal(_u32(surf["emissive"]), _u32(t["emissive"]))
    finally:
        e.close()


# ---- 2. the generator against the model
def tables():
    """the feature scene's table, one record of it, none, and one with bad records mixed in (they are dark and still count)"""
    e = direct.scene_emitters(scenes.feature_scene())
    spoilt = np.concatenate([e, e, e])
    spoilt["a"][5, 1], spoilt["b"][6, 0], spoilt["c"][7, 2], spoilt["emissive"][8, 0] = np.nan, np.inf, -np.inf, np.nan
    spoilt["area"][9], spoilt["area"][10], spoilt["area"][11], spoilt["kind"][12], spoilt["kind"][13] = 0.0, -1.0, np.inf, 1, 0xFFFFFFFF
    return {"scene": e, "one": e[2:3], "none": e[:0], "spoilt": spoilt}


@pytest.mark.parametrize("with_seeds", [False, True], ids=["index", "seeds"])
@pytest.mark.parametrize("which", ["scene", "one", "none", "spoilt"])
def test_generator_equals_the_model(which, with_seeds):
    table = tables()[which]
    pts, nrm = model_surfels(M)
    pts[0::3] = (pts[0::3] * f32(0.3)).astype(f32) + f32([0, -1, -2])   # near the scene: most items are lit
    nrm[0::3] = (0.1, 1.0, 0.05)
    ids = given_seeds(M) if with_seeds else None
    if with_seeds:   # the edge draw: u0 == 1.0f for sample 7 of surfel 0 and sample 8 of surfel 3
        ids[0], ids[3] = seeds_drawing(0xFFFFFFFF, 7, 0), seeds_drawing(0xFFFFFF80, 7, 1)
    n_dark = n_lit = n_invalid = 0
    for samples, first_sample, offset, shorten in ((3, 0, 1e-3, 1e-3), (4, 7, 0.0, 0.0), (5, 7, 1e-3, 0.5)):
        rays, tmax, contrib = engine.light_rays(table, pts, nrm, samples, first_sample, seeds=ids, offset=offset, shorten=shorten, device=0)
        o, d, t, c = direct.rays(table, hemisphere.surfels(pts, nrm), first_sample, samples, seeds=ids, offset=offset, shorten=shorten)
        where = (which, with_seeds, samples, first_sample)
        assert rays.shape == (M * samples,) and tmax.shape == (M * samples,) and contrib.shape == (M * samples, 4), where
        for what, got, want in (("origin", rays["origin"], o), ("dir", rays["dir"], d), ("tmax", tmax[:, None], t[:, None]), ("contrib", contrib, c)):
            bad = np.nonzero((_u32(got) != _u32(want)).any(1))[0]
            assert len(bad) == 0, (where, what, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
        assert (_u32(rays["_pad0"]) == 0).all() and (_u32(rays["_pad1"]) == 0).all(), where
        n_lit += int((t > 0).sum())
        n_dark += int(((t == 0) & (c[:, 3] == 1)).sum())
        n_invalid += int((c[:, 3] == 0).sum())
        if with_seeds and first_sample == 7 and len(table):
            u0 = direct.draws(M, 7, samples, seeds=ids)["u0"]
            assert u0[0] == 1.0 and u0[3 * samples + 1] == 1.0
    assert n_invalid > 0 and n_dark > 0 and (n_lit > 0) == (which != "none")


# ---- 3. the sums, once per walk
WALKS = {"feature": (lambda: scenes.feature_scene(width=24, height=16), dict(), "k_occl"),
         "mesh chunk": (_mesh, dict(), "k_occl_chunk"), "mesh bvh": (_mesh, dict(reference_walk=True), "k_occl_bvh"),
         "lamps": (lamps, dict(), "k_occl_bvh"), "mesh + spheres": (_mesh_beside_spheres, dict(), "k_occl_chunk")}


def model_sums(e, table, pts, nrm, samples, first_sample, ids, mask, offset=1e-3, shorten=1e-3):
    """direct.fold of the model's contributions under rb_occluded's bytes on the generator's own records and bounds"""
    rays, tmax, _ = engine.light_rays(table, pts, nrm, samples, first_sample, seeds=ids, offset=offset, shorten=shorten, device=0)
    contrib = direct.rays(table, hemisphere.surfels(pts, nrm), first_sample, samples, seeds=ids, offset=offset, shorten=shorten)[3]
    occ = e.occluded_records(rays, tmax, mask)
    return direct.fold(contrib, occ, samples), occ, tmax


@pytest.mark.parametrize("name", list(WALKS))
def test_sums_equal_the_fold_of_the_model(name):
    make, kw, kernel = WALKS[name]
    s = make()
    table = direct.scene_emitters(s)
    assert len(table) > 0
    e = _engine(s, **kw)
    try:
        pts, nrm = mixed_surfels(e, s)
        st0, lit, shadowed = e.stats(), 0, 0
        for samples, first_sample, with_seeds, mask in ((3, 0, False, abi.MASK_ALL), (4, 7, True, abi.MASK_ALL), (5, 7, False, NO_LIGHTS), (4, 0, True, 0)):
            ids = given_seeds(M) if with_seeds else None
            got = e.direct_light(pts, nrm, samples, first_sample=first_sample, seeds=ids, mask=mask)
            assert e.last_query_kernel_name() == kernel, e.last_query_kernel_name()
            assert e.last_query_ms() > 0 and 0 < e.last_camera_rays_ms() <= e.last_query_ms()
            want, occ, tmax = model_sums(e, table, pts, nrm, samples, first_sample, ids, mask)
            where = (name, samples, first_sample, with_seeds, mask)
            bad = np.nonzero((_u32(got).reshape(-1, 4) != _u32(want).reshape(-1, 4)).any(1))[0]
            assert got.dtype == abi.RADIANCE and len(bad) == 0, (where, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
            gone = (occ == abi.OCCL_INVALID).reshape(M, samples).all(1)
            assert gone.sum() >= 3 and not _u32(got[gone]).any() and (got["weight"][~gone] == samples).all(), where
            # the caller's table, equal to the scene's, gives the bits of NULL
            assert np.array_equal(_u32(e.direct_light(pts, nrm, samples, emitters=table, first_sample=first_sample, seeds=ids, mask=mask)), _u32(got)), where
            lit += int((got["sum"] != 0).any(1).sum())
            if mask == abi.MASK_ALL:
                shadowed += int(((occ == abi.OCCL_OCCLUDED) & (tmax > 0)).sum())
            if mask == 0:
                assert not (occ == abi.OCCL_OCCLUDED).any()
        assert lit > 0 and shadowed > 0, "the scene lit nothing, or shadowed nothing"
        # one light gets a map of its own, and an empty table lights nothing
        one = e.direct_light(pts, nrm, 4, emitters=table[-1:])
        assert np.array_equal(_u32(one), _u32(model_sums(e, table[-1:], pts, nrm, 4, 0, None, abi.MASK_ALL)[0]))
        none = e.direct_light(pts, nrm, 4, emitters=table[:0])
        assert not _u32(none["sum"]).any() and np.array_equal(none["weight"], one["weight"])
        assert e.stats() == st0, "direct-light queries moved rb_get_stats"
    finally:
        e.close()


# ---- 4. forms and pieces
def test_device_forms_and_a_forced_launch_shape_equal_the_host_forms():
    import torch
    s = _mesh()
    table = direct.scene_emitters(s)
    e = _engine(s)
    try:
        pts, nrm = mixed_surfels(e, s)
        ids = given_seeds(M)
        tp, tn = torch.from_numpy(pts).cuda(), torch.from_numpy(nrm).cuda()
        tids = torch.from_numpy(ids.view(np.int32)).cuda()
        ttab = torch.from_numpy(table.view(f32).reshape(-1, 16)).cuda()
        for sid, tsid in ((None, None), (ids, tids)):
            rad = e.direct_light(pts, nrm, 5, first_sample=7, seeds=sid)
            d_rad = e.direct_light(tp, tn, 5, first_sample=7, seeds=tsid)
            assert e.last_query_kernel_name() == "k_occl_chunk" and e.last_query_ms() > 0 and e.last_camera_rays_ms() > 0
            assert d_rad.shape == (M, 4) and d_rad.is_cuda and np.array_equal(_u32(d_rad.cpu().numpy()), _u32(rad).reshape(-1, 4))
            d_own = e.direct_light(tp, tn, 5, emitters=ttab, first_sample=7, seeds=tsid)
            assert np.array_equal(_u32(d_own.cpu().numpy()), _u32(rad).reshape(-1, 4))
            d_up = e.direct_light(tp, tn, 5, emitters=table, first_sample=7, seeds=tsid)   # a numpy table beside tensors is uploaded
            assert np.array_equal(_u32(d_up.cpu().numpy()), _u32(rad).reshape(-1, 4))
        assert (rad["sum"] != 0).any(1).sum() > 20
        # out= : an array or a tensor to fill
        filled = np.zeros(M, dtype=abi.RADIANCE)
        assert e.direct_light(pts, nrm, 5, first_sample=7, seeds=ids, out=filled) is filled and np.array_equal(_u32(filled), _u32(rad))
        out = torch.full((M, 4), -1.0, dtype=torch.float32, device="cuda")
        assert e.direct_light(tp, tn, 5, first_sample=7, seeds=tids, out=out) is out and np.array_equal(_u32(out.cpu().numpy()), _u32(rad).reshape(-1, 4))
        # sub-ranges with their ids equal the whole call's records
        for first, n in ((70, 60), (127, 2), (64, 64), (0, 1), (129, 1)):
            sl = slice(first, first + n)
            assert np.array_equal(_u32(e.direct_light(pts[sl], nrm[sl], 5, first_sample=7, seeds=ids[sl])), _u32(rad[sl])), (first, n)
        assert len(e.direct_light(pts[:0], nrm[:0], 5)) == 0
        # fewer than 64 surfels go in linear order instead of a padded block: one surfel at many samples, 63, and 64 beside them
        for first, n, samples in ((0, 1, 300), (3, 2, 129), (60, 63, 7), (60, 64, 7)):
            sl = slice(first, first + n)
            got = e.direct_light(pts[sl], nrm[sl], samples, first_sample=2, seeds=ids[sl])
            assert np.array_equal(_u32(got), _u32(model_sums(e, table, pts[sl], nrm[sl], samples, 2, ids[sl], abi.MASK_ALL)[0])), (first, n, samples)
            d_got = e.direct_light(tp[sl], tn[sl], samples, first_sample=2, seeds=tids[sl])
            assert np.array_equal(_u32(d_got.cpu().numpy()), _u32(got).reshape(-1, 4)), (first, n, samples)
        # bake.direct_irradiance on tensors stays on the device and equals the host form's mean
        mean = bake.direct_irradiance(e, pts, nrm, 5, first_sample=7, seeds=ids)
        d_mean = bake.direct_irradiance(e, tp, tn, 5, first_sample=7, seeds=tids)
        assert mean.shape == (M, 3) and d_mean.is_cuda and np.allclose(d_mean.cpu().numpy(), mean, rtol=1e-6, atol=0)   # (torch divides there)
        assert np.array_equal(_u32(mean), _u32(np.where(rad["weight"][:, None] > 0, rad["sum"] / np.maximum(rad["weight"], 1)[:, None], 0).astype(f32)))
        # the launch shape: reservations of 64 items on a grid of one block per CU
        o = _engine(s, queue_batch=64, blocks_per_cu=1)
        try:
            assert np.array_equal(_u32(o.direct_light(pts, nrm, 5, first_sample=7, seeds=ids)), _u32(rad))
        finally:
            o.close()
        for bad in (dict(out=np.zeros(M, f32)), dict(out=out[:5]), dict(out=out[:, :3]), dict(samples=-1), dict(seeds=ids[:5]),
                    dict(emitters=ttab)):   # (a tensor table beside numpy points)
            with pytest.raises(ValueError):
                e.direct_light(pts, nrm, **dict(dict(samples=1), **bad))
        with pytest.raises(ValueError):
            e.direct_light(tp, tn, 1, emitters=ttab[:, :8])
    finally:
        e.close()


def test_a_call_across_a_piece_boundary():
    """RB_HEMI_PIECE_ITEMS + 77 * samples items at samples = 64 on the feature scene: two pieces.  Every surfel against two
    calls split at the piece boundary (seeds carry the indices on); the last 77 surfels and the 32 before the boundary against
    the fold of the model; both against the device form's answers, whose two pieces go through the same loop on the caller's
    buffers."""
    import torch
    samples = 64
    b = PIECE // samples
    n = b + 77
    s = scenes.feature_scene(width=24, height=16)
    table = direct.scene_emitters(s)
    e = _engine(s)
    try:
        p0, n0 = scene_surfels(e, s, 200)
        idx = np.arange(n) % 200
        pts, nrm = np.ascontiguousarray(p0[idx]), np.ascontiguousarray(n0[idx])
        ids = np.arange(n, dtype=np.uint32)
        one = e.direct_light(pts, nrm, samples, first_sample=7)
        assert e.last_query_kernel_name() == "k_occl" and e.last_query_ms() > 0
        two = np.concatenate([e.direct_light(pts[:b], nrm[:b], samples, first_sample=7),
                              e.direct_light(pts[b:], nrm[b:], samples, first_sample=7, seeds=ids[b:])])
        assert np.array_equal(_u32(one), _u32(two))
        assert (one["weight"] == samples).all() and (one["sum"] != 0).any(1).sum() > 1000
        assert not np.array_equal(_u32(one[:200]), _u32(one[200:400]))   # the same surfels under other ids
        tail = slice(b - 32, n)
        want = model_sums(e, table, pts[tail], nrm[tail], samples, 7, ids[tail], abi.MASK_ALL)[0]
        assert np.array_equal(_u32(one[tail]), _u32(want))
        d_pts, d_nrm = (torch.from_numpy(a).to(f"cuda:{e.query_device}") for a in (pts, nrm))
        dev = e.direct_light(d_pts, d_nrm, samples, first_sample=7)
        assert e.last_camera_rays_ms() > 0   # both pieces' event pairs were recorded and are read
        assert np.array_equal(_u32(dev.cpu().numpy()), _u32(one).reshape(n, 4))
    finally:
        e.close()


# ---- 5. the estimator against the path tracer, on the device
def test_estimator_against_trace_hemisphere():
    """The criterion of tests/test_direct_model.py with rb_trace_hemisphere as the other side: 16 floor points of a Cornell copy
    with max_depth = 1 and a black sky, 4096 samples each -- one surfel per sample, so that the per-sample values come back."""
    s = lit_cornell()
    pts, nrm = floor_points()
    e = _engine(s)
    try:
        rep_p, rep_n = np.repeat(pts, SAMPLES, axis=0), np.repeat(nrm, SAMPLES, axis=0)
        hemi = e.trace_hemisphere(rep_p, rep_n, 1)
        dirc = e.direct_light(rep_p, rep_n, 1)
        assert (hemi["weight"] == 1).all() and (dirc["weight"] == 1).all()
        mh, md, se = compare_estimators(hemi["sum"], dirc["sum"], "cornell floor, device")
        for factor in (1 / 2.0, np.pi, 5.5 ** 2):   # a dropped N, 1 / pi or 1 / d^2
            assert abs(mh - md * factor) > 5.0 * se
        # and summed on the device, sample by sample
        rad = e.direct_light(pts, nrm, SAMPLES)
        assert np.isclose((rad["sum"].astype(np.float64) / SAMPLES).mean(), md, rtol=0.02)
    finally:
        e.close()


# ---- 6. after an update
def test_the_first_call_after_an_update_sees_the_new_scene():
    s = scenes.feature_scene(width=24, height=16)
    e = _engine(s)
    try:
        pts, nrm = mixed_surfels(e, s)

        def check(scene, what):
            table = direct.scene_emitters(scene)
            got = e.direct_light(pts, nrm, 4, first_sample=3)   # the sums first: they must not be the old table's
            assert np.array_equal(_bytes(e.scene_emitters()), _bytes(table)), what
            want = model_sums(e, table, pts, nrm, 4, 3, None, abi.MASK_ALL)[0]
            assert np.array_equal(_u32(got), _u32(want)), what
            return got
        base = check(s, "as created")
        # a mesh material's emission: the quad goes dark, the red wall glows
        meshes = s.meshes.copy()
        meshes["material"]["emissive"][1] = 0
        meshes["material"]["emissive"][2] = (3.0, 0.5, 0.25)
        s1 = _copy(s, meshes=meshes)
        e.update(RenderConfig(uniforms=Change.update(s.uniforms), meshes=Change.update(meshes)))   # (every update carries the uniforms)
        assert [int(p) for p in direct.scene_emitters(s1)["prim"]] == [4, 5, 4, 0, 1]
        after = check(s1, "meshes updated")
        assert not np.array_equal(_u32(after), _u32(base))
        # the lights gone: Change::Delete of the lights is refused as the reference refuses it (the table stands), so they are
        # updated to an empty array, which leaves the phantom light
        with pytest.raises(Exception):
            e.update(RenderConfig(uniforms=Change.update(s.uniforms), lights=Change.delete()))
        assert np.array_equal(_bytes(e.scene_emitters()), _bytes(direct.scene_emitters(s1)))
        s2 = _copy(s1, lights=np.zeros(0, dtype=abi.POINT_LIGHT))
        e.update(RenderConfig(uniforms=Change.update(s.uniforms), lights=Change.update(s2.lights)))
        assert len(direct.scene_emitters(s2)) == 3
        check(s2, "lights emptied")
        # the spheres shortened: the emissive one is gone
        s3 = _copy(s2, spheres=s.spheres[:4].copy())
        s3.uniforms["spheres_count"] = 4
        e.update(RenderConfig(uniforms=Change.update(s.uniforms), spheres=Change.update(s.spheres[:4].copy())))
        assert [int(k) for k in direct.scene_emitters(s3)["kind"]] == [abi.HIT_TRIANGLE] * 2
        check(s3, "spheres shortened")
        # uniforms that keep a smaller triangle count: the second glowing triangle is behind it
        u = s3.uniforms.copy()
        u["bvh_triangle_count"] = 5
        e.update(RenderConfig(uniforms=Change.update(u)))
        table = direct.scene_emitters(s3, triangle_count=5)
        assert [int(p) for p in table["prim"]] == [4] and np.array_equal(_bytes(e.scene_emitters()), _bytes(table))
        # a refused update leaves the table standing
        with pytest.raises(Exception):
            e.update(RenderConfig(uniforms=Change.update(u), meshes=Change.delete()))
        assert np.array_equal(_bytes(e.scene_emitters()), _bytes(table))
    finally:
        e.close()


# ---- 7. side effects, refusals, sharding
def test_a_direct_light_query_between_iterator_frames():
    s = scenes.feature_scene(width=48, height=32, spp=4)
    rc = RenderConfig.from_scene(s)
    small = scenes.feature_scene(width=24, height=16)
    probe = _engine(small)
    pts, nrm = scene_surfels(probe, small)
    probe.close()

    def frames(query):
        e = Engine.new(rc, device=0)
        it = e.frame_iterator(rc)
        out, answers = [], []
        while it.has_next():
            out.append(it.next().pixels.copy())
            if query:
                kernel = e.last_kernel_name()
                answers.append((e.direct_light(pts, nrm, 3), e.scene_emitters()))
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
    for rad, tab in answers[1:]:
        assert np.array_equal(_u32(rad), _u32(answers[0][0])) and np.array_equal(_bytes(tab), _bytes(answers[0][1]))
    assert (answers[0][0]["sum"] != 0).any()


def test_refusals_leave_the_engine_rendering_the_golden_frame():
    import torch
    from renderbaby_amd._lib import load
    lib = load()
    s = scenes.cornell(32, 32, 2, 4)
    rc = RenderConfig.from_scene(s)
    e = Engine.new(rc, device=0)
    pts = np.array([(0.1 * i, 0.25, -3.0) for i in range(4)], f32)
    nrm = np.tile(f32([0, 1, 0]), (4, 1))
    surf = hemisphere.surfels(pts, nrm)
    tab = direct.scene_emitters(s)
    try:
        e.update(rc)
        h = e._h
        base = _params()
        before = e.direct_light(pts, nrm, 2)
        assert (before["sum"] != 0).any()
        d_surf = torch.from_numpy(surf.view(f32).reshape(-1, 8)).cuda()
        d_tab = torch.from_numpy(tab.view(f32).reshape(-1, 16)).cuda()
        out = np.full(64, 7, dtype=abi.RADIANCE)
        d_out = torch.full((64, 4), 7, dtype=torch.float32, device="cuda")
        for fn, tp, sp, o in ((lib.rb_direct_light, tab.ctypes.data, surf.ctypes.data, out.ctypes.data),
                              (lib.rb_direct_light_device, d_tab.data_ptr(), d_surf.data_ptr(), d_out.data_ptr())):
            for name, kw in REFUSALS:
                args = dict(n=4, first_sample=0, samples=2, params=base, n_emit=2)
                args.update(kw)
                assert fn(h, tp, args["n_emit"], sp, None, args["n"], args["params"].ctypes.data, args["first_sample"], args["samples"], o) == INVALID_OPTIONS, name
                assert lib.rb_last_error(h)
                if "n_emit" not in kw:   # ... and with the scene's own table
                    assert fn(h, None, 0, sp, None, args["n"], args["params"].ctypes.data, args["first_sample"], args["samples"], o) == INVALID_OPTIONS, name
            for name, fields in MASK_REFUSALS:
                assert fn(h, tp, 2, sp, None, 4, _params(**fields).ctypes.data, 0, 2, o) == INVALID_OPTIONS, name
            assert fn(h, None, 1 << 40, sp, None, 4, base.ctypes.data, 0, 2, o) == 0   # n_emit is not looked at beside a NULL table
            assert lib.rb_sync(h) == 0
            out[:], d_out[:] = 7, 7
            assert fn(h, tp, 2, None, None, 4, base.ctypes.data, 0, 2, o) == NULL_ARGUMENT and fn(h, tp, 2, sp, None, 4, None, 0, 2, o) == NULL_ARGUMENT
            assert fn(h, tp, 2, sp, None, 4, base.ctypes.data, 0, 2, None) == NULL_ARGUMENT
            assert fn(h, None, 0, None, None, 0, base.ctypes.data, 0, 2, None) == 0 and fn(h, None, 0, None, None, 0, None, 0, 2, None) == 0   # n == 0
        lib.rb_sync(h)
        assert (out.view(np.uint32) == np.float32(7).view(np.uint32)).all() and (d_out == 7).all().item()
        # the device form's buffers: a host pointer, a misaligned one, an allocation that ends before its elements
        dev, bp = lib.rb_direct_light_device, base.ctypes.data
        assert dev(h, None, 0, surf.ctypes.data, None, 4, bp, 0, 2, d_out.data_ptr()) == INVALID_OPTIONS
        assert dev(h, None, 0, d_surf.data_ptr(), None, 4, bp, 0, 2, out.ctypes.data) == INVALID_OPTIONS
        assert dev(h, tab.ctypes.data, 2, d_surf.data_ptr(), None, 4, bp, 0, 2, d_out.data_ptr()) == INVALID_OPTIONS
        assert dev(h, d_tab.data_ptr() + 4, 1, d_surf.data_ptr(), None, 4, bp, 0, 2, d_out.data_ptr()) == INVALID_OPTIONS
        assert dev(h, d_tab.data_ptr(), 1 << 20, d_surf.data_ptr(), None, 4, bp, 0, 2, d_out.data_ptr()) == INVALID_OPTIONS
        assert dev(h, None, 0, d_surf.data_ptr() + 4, None, 3, bp, 0, 2, d_out.data_ptr()) == INVALID_OPTIONS
        assert dev(h, None, 0, d_surf.data_ptr(), None, 4, bp, 0, 2, d_out.data_ptr() + 4) == INVALID_OPTIONS
        assert dev(h, None, 0, d_surf.data_ptr(), None, 1 << 20, bp, 0, 1, d_out.data_ptr()) == INVALID_OPTIONS
        assert dev(h, None, 0, d_surf.data_ptr(), d_out.data_ptr() + 2, 4, bp, 0, 2, d_out.data_ptr()) == INVALID_OPTIONS   # d_seeds
        cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        count = C.c_size_t(0)
        assert lib.rb_scene_emitters(h, None, 0, None) == NULL_ARGUMENT and lib.rb_scene_emitters(h, None, 2, C.byref(count)) == NULL_ARGUMENT
        assert lib.rb_scene_emitters_device(h, d_tab.data_ptr(), 2, None) == NULL_ARGUMENT
        assert lib.rb_scene_emitters_device(h, tab.ctypes.data, 2, cnt.data_ptr()) == INVALID_OPTIONS
        assert lib.rb_scene_emitters_device(h, d_tab.data_ptr(), 1 << 20, cnt.data_ptr()) == INVALID_OPTIONS
        assert lib.rb_scene_emitters_device(h, d_tab.data_ptr() + 8, 1, cnt.data_ptr()) == INVALID_OPTIONS
        assert lib.rb_scene_emitters_device(h, d_tab.data_ptr(), 2, cnt.data_ptr() + 2) == INVALID_OPTIONS
        assert (d_out == 7).all().item() and int(cnt.item()) == 0
        assert dev(h, None, 0, d_surf.data_ptr(), None, 4, bp, 0, 2, d_out.data_ptr()) == 0 and lib.rb_sync(h) == 0
        assert np.array_equal(_u32(d_out.cpu().numpy()[:4]), _u32(before).reshape(4, -1)) and (d_out[4:] == 7).all().item()
        assert np.array_equal(_u32(e.direct_light(pts, nrm, 2)), _u32(before))
        assert np.array_equal(e.render(rc).pixels, _oracle.render(s)[2])
    finally:
        e.close()
    cold = Engine.new(rc, device=0)   # no update yet: not ready, and still a refusal first
    try:
        out = np.zeros(4, dtype=abi.RADIANCE)
        count = C.c_size_t(0)
        assert lib.rb_direct_light(cold._h, None, 0, surf.ctypes.data, None, 4, base.ctypes.data, 0, 2, out.ctypes.data) not in (0, INVALID_OPTIONS)
        assert lib.rb_direct_light(cold._h, tab.ctypes.data, 2, surf.ctypes.data, None, 4, base.ctypes.data, 0, 2, out.ctypes.data) not in (0, INVALID_OPTIONS)
        assert lib.rb_direct_light(cold._h, None, 0, surf.ctypes.data, None, 4, base.ctypes.data, 0, 0, out.ctypes.data) == INVALID_OPTIONS
        assert lib.rb_scene_emitters(cold._h, None, 0, C.byref(count)) not in (0, INVALID_OPTIONS)
        assert np.array_equal(cold.render(rc).pixels, _oracle.render(s)[2])
    finally:
        cold.close()


def test_sharded_engine_and_multi_device_handle():
    """both forms on a sharded engine (a surfel sees the whole scene) and on a multi-device handle on one device"""
    import torch
    s = scenes.feature_scene(width=24, height=16)
    e = _engine(s)
    pts, nrm = scene_surfels(e, s)
    want, table = e.direct_light(pts, nrm, 2, first_sample=7), e.scene_emitters()
    e.close()
    tp, tn = torch.from_numpy(pts).cuda(), torch.from_numpy(nrm).cuda()
    for kw in (dict(shard_rank=1, shard_count=3, stripe_rows=8), dict(devices=[0, 0], gather_peer_copy=True)):
        p = _engine(s, **kw)
        try:
            assert np.array_equal(_u32(p.direct_light(pts, nrm, 2, first_sample=7)), _u32(want)), kw
            assert np.array_equal(_bytes(p.scene_emitters()), _bytes(table)), kw
            dev = p.direct_light(tp, tn, 2, first_sample=7)
            assert np.array_equal(_u32(dev.cpu().numpy()), _u32(want).reshape(-1, 4)), kw
            assert p.last_query_kernel_name() == "k_occl" and p.last_query_ms() > 0
        finally:
            p.close()


# ---- 8. the layers above
def test_lightmap_direct_is_the_three_stages():
    s = scenes.feature_scene(width=24, height=16)
    e = _engine(s)
    try:
        w, h, samples = 24, 16, 4
        got = bake.lightmap_direct(e, w, h, samples, first_sample=2, dilate=1)
        surf, own = e.lightmap_surfels(w, h)
        sums = e.direct_light(surf, None, samples, first_sample=2)
        assert got.shape == (h, w, 4) and np.array_equal(_u32(got), _u32(engine.lightmap_resolve(sums, w, h, dilate=1, device=0)))
        covered = own != abi.LIGHTMAP_NO_OWNER
        assert covered.any() and (got[..., 3].reshape(-1)[covered] == 1).all() and (got[..., :3] > 0).any()
    finally:
        e.close()
