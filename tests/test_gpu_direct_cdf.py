"""Direct light with a weighted pick (rb_emitter_cdf / rb_scene_emitter_cdf / rb_light_rays_cdf / rb_direct_light_cdf and their
device forms), bit for bit on uint32 views:

  the table by power = direct.emitter_cdf, from one record to past one block of the scan, and the scene's own in both forms;
  the generator      = direct.rays(cdf=...): by power, by a caller's table, and the ramp j + 1, which is rb_light_rays;
  the sums           = direct.fold of the model's contributions under rb_occluded's bytes on the model's records, once per walk,
                       and for tables no host form accepts -- decreasing, total 0, total above 2^24 -- through the device form;
  the forms and the pieces give the same answers, a refused call has done nothing, and rb_direct_light's own sums on the same
  engine do not move.
"""
import ctypes as C

import numpy as np
import pytest

from renderbaby_amd import Change, Engine, RenderConfig, abi, bake, direct, engine, hemisphere, scenes
from tests import _oracle
from tests.conftest import has_gpu
from tests.test_direct_abi import INVALID_OPTIONS, MASK_REFUSALS, NULL_ARGUMENT, REFUSALS, _params
from tests.test_direct_cdf_abi import BAD_TABLES
from tests.test_direct_cdf_model import TOP, table as power_table
from tests.test_direct_model import seeds_drawing
from tests.test_gpu_direct import M, NO_LIGHTS, PIECE, WALKS, _bytes, long_table, mixed_surfels, tables
from tests.test_gpu_hemisphere import model_surfels, scene_surfels
from tests.test_gpu_query import _copy, _engine
from tests.test_gpu_radiance import _mesh, _u32, given_seeds

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

f32, u32 = np.float32, np.uint32


def same_rows(got, want, where):
    g, w = _u32(got).reshape(len(got), -1), _u32(want).reshape(len(want), -1)
    bad = np.nonzero((g != w).any(1))[0]
    assert g.shape == w.shape and len(bad) == 0, (where, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])


# ---- 1. the table by power
@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 4097])
def test_emitter_cdf_equals_the_model(n):
    rng = np.random.default_rng(100 + n)
    e = power_table(n, rng)
    for k in (0, 4095, 4096, n - 1):   # unweighable at the ends and on either side of the scan's first block edge
        if k < n and n > 1:
            e["area"][k] = (0.0, np.nan, -1.0, np.inf)[k % 4]
    if n > 2:
        e["emissive"][n // 2], e["area"][n // 2] = (3e38, 1, 1), 10.0   # a power that overflows: clamped, the top of the table
    want = direct.emitter_cdf(e)
    got = engine.emitter_cdf(e, device=0)
    assert got.dtype == u32 and np.array_equal(got, want), (n, np.nonzero(got != want)[0][:5])
    assert int(want[-1]) <= TOP and (n <= 2 or int(want[-1]) > 0)
    # narrow powers: the quantised weights are not all the floor of 1
    e = power_table(n, rng, -2.0, 2.0)
    want = direct.emitter_cdf(e)
    assert np.array_equal(engine.emitter_cdf(e, device=0), want) and int(want[-1]) >= direct.cdf_scale(n)
    # no power anywhere: zeros
    e["emissive"] = 0
    assert not engine.emitter_cdf(e, device=0).any()
    assert len(engine.emitter_cdf(e[:0], device=0)) == 0


CDF_SCENES = {"feature": lambda: scenes.feature_scene(width=24, height=16), "cornell": lambda: scenes.cornell(32, 32, 1, 4), "long table": long_table,
              "no emitter": scenes.sky_only}


@pytest.mark.parametrize("name", list(CDF_SCENES))
def test_scene_cdf_equals_the_model_in_both_forms(name):
    import torch
    s = CDF_SCENES[name]()
    table = direct.scene_emitters(s)
    want = direct.emitter_cdf(table)
    n = len(want)
    e = _engine(s)
    try:
        st0 = e.stats()
        lib = e._lib
        # neither the emitter table nor the uniform pick makes the weights: the first call that asks for them does, and reports
        # its kernel time; once they stand a call reports 0
        assert len(e.scene_emitters()) == n
        pts, nrm = (scene_surfels(e, s, 8) if n else (np.zeros((8, 3), f32), np.tile(f32([0, 1, 0]), (8, 1))))
        uniform = e.direct_light(pts, nrm, 2)
        count = C.c_size_t(99)
        assert lib.rb_scene_emitter_cdf(e._h, None, 0, C.byref(count)) == 0 and count.value == n
        assert e.last_query_kernel_name() == "k_emit_quant" and (e.last_query_ms() > 0 or n == 0)
        assert lib.rb_scene_emitter_cdf(e._h, None, 0, C.byref(count)) == 0 and count.value == n and e.last_query_ms() == 0
        got = e.scene_emitter_cdf()
        assert got.dtype == u32 and np.array_equal(got, want) and e.last_query_ms() == 0, (name, got[:8], want[:8])
        for cap in sorted({0, 1, max(n - 1, 0), n, n + 3}):
            buf = np.full(cap + 1, 0x07070707, dtype=u32)
            count = C.c_size_t(99)
            assert lib.rb_scene_emitter_cdf(e._h, buf.ctypes.data if cap else None, cap, C.byref(count)) == 0 and count.value == n, (name, cap)
            k = min(cap, n)
            assert np.array_equal(buf[:k], want[:k]) and (buf[k:] == 0x07070707).all(), (name, cap)
            if cap:
                t = torch.full((cap + 1,), 7, dtype=torch.int32, device="cuda")
                d_got, d_count = e.scene_emitter_cdf(out=t[:cap])
                assert d_count == n and np.array_equal(d_got.cpu().numpy().view(u32)[:k], want[:k]) and (t[k:] == 7).all().item(), (name, cap)
        cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        assert lib.rb_scene_emitter_cdf_device(e._h, None, 0, cnt.data_ptr()) == 0 and lib.rb_sync(e._h) == 0 and int(cnt.item()) == n
        # the scene's weights are the caller's by power, and the uniform pick has not moved
        if n:
            by_scene = e.direct_light(pts, nrm, 3, pick="power")
            same_rows(e.direct_light(pts, nrm, 3, emitters=table, pick="power"), by_scene, name)
            same_rows(e.direct_light(pts, nrm, 3, emitters=table, pick=want), by_scene, name)
        same_rows(e.direct_light(pts, nrm, 2), uniform, name)
        assert e.stats() == st0, "the table moved rb_get_stats"
    finally:
        e.close()


def test_the_scene_cdf_follows_an_update():
    s = scenes.feature_scene(width=24, height=16)
    e = _engine(s)
    try:
        pts, nrm = scene_surfels(e, s, 40)
        before = e.scene_emitter_cdf()
        assert np.array_equal(before, direct.emitter_cdf(direct.scene_emitters(s)))
        lights = s.lights.copy()
        lights["material"]["emissive"][0] = (lights["material"]["emissive"][0] * f32(9.0)).astype(f32)
        s1 = _copy(s, lights=lights)
        e.update(RenderConfig(uniforms=Change.update(s.uniforms), lights=Change.update(lights)))
        table = direct.scene_emitters(s1)
        want = direct.emitter_cdf(table)
        assert not np.array_equal(want, before)
        got = e.direct_light(pts, nrm, 4, first_sample=3, pick="power")   # the sums first: they must not be the old weights'
        same_rows(got, model_sums(e, table, want, pts, nrm, 4, 3, None, abi.MASK_ALL), "after the update")
        assert e.last_query_ms() > 0
        assert np.array_equal(e.scene_emitter_cdf(), want) and e.last_query_ms() == 0   # ... and that call made them
        with pytest.raises(Exception):   # a refused update leaves them standing
            e.update(RenderConfig(uniforms=Change.update(s.uniforms), meshes=Change.delete()))
        assert np.array_equal(e.scene_emitter_cdf(), want) and e.last_query_ms() == 0
    finally:
        e.close()


# ---- 2. the generator against the model
def caller_tables(table):
    """pick tables of a caller's for `table`: by power, the ramp, weights of the caller's own with zero steps in them"""
    n = len(table)
    own = np.cumsum((np.arange(n) * 7 + 3) % 5 * 1000, dtype=np.uint64).astype(u32)
    if n and own[-1] == 0:
        own[-1] = 5
    return {"power": direct.emitter_cdf(table), "ramp": np.arange(1, n + 1, dtype=u32), "own": own}


@pytest.mark.parametrize("which", ["scene", "one", "none", "spoilt"])
def test_generator_equals_the_model(which):
    table = tables()[which]
    pts, nrm = model_surfels(M)
    pts[0::3] = (pts[0::3] * f32(0.3)).astype(f32) + f32([0, -1, -2])   # near the scene: most items are lit
    nrm[0::3] = (0.1, 1.0, 0.05)
    ids = given_seeds(M)
    ids[0], ids[3] = seeds_drawing(0xFFFFFFFF, 7, 0), seeds_drawing(0xFFFFFF80, 7, 1)   # u0 == 1.0f
    surf = hemisphere.surfels(pts, nrm)
    n_lit = n_dark = 0
    for name, cdf in caller_tables(table).items():
        for samples, first_sample, offset, shorten, sid in ((3, 0, 1e-3, 1e-3, None), (5, 7, 0.0, 0.5, ids)):
            where = (which, name, samples)
            kw = dict(seeds=sid, offset=offset, shorten=shorten)
            rays, tmax, contrib = engine.light_rays(table, pts, nrm, samples, first_sample, device=0, cdf=cdf, **kw)
            o, d, t, c = direct.rays(table, surf, first_sample, samples, cdf=cdf, **kw)
            for what, got, want in (("origin", rays["origin"], o), ("dir", rays["dir"], d), ("tmax", tmax[:, None], t[:, None]), ("contrib", contrib, c)):
                same_rows(got, want, (where, what))
            assert (_u32(rays["_pad0"]) == 0).all() and (_u32(rays["_pad1"]) == 0).all(), where
            n_lit += int((t > 0).sum())
            n_dark += int(((t == 0) & (c[:, 3] == 1)).sum())
            plain = engine.light_rays(table, pts, nrm, samples, first_sample, device=0, **kw)
            if name == "ramp":   # the identity, on the device too
                for got, want in zip((rays, tmax, contrib), plain):
                    assert np.array_equal(_bytes(got), _bytes(want)), where
            if name == "power":   # NULL is the table by power
                for got, want in zip(engine.light_rays(table, pts, nrm, samples, first_sample, device=0, cdf="power", **kw), (rays, tmax, contrib)):
                    assert np.array_equal(_bytes(got), _bytes(want)), where
    assert n_dark > 0 and (n_lit > 0) == (which != "none")


def test_equal_powers_are_the_uniform_pick_on_the_device():
    table = tables()["scene"].copy()
    table["area"], table["emissive"] = 2.0, (3, 1, 2)
    pts, nrm = model_surfels(M)
    pts[0::3] = (pts[0::3] * f32(0.3)).astype(f32) + f32([0, -1, -2])
    got = engine.light_rays(table, pts, nrm, 6, 1, device=0, cdf="power")
    for a, b in zip(got, engine.light_rays(table, pts, nrm, 6, 1, device=0)):
        assert np.array_equal(_bytes(a), _bytes(b))
    assert (got[1] > 0).any()


# ---- 3. the sums, once per walk
def model_sums(e, table, cdf, pts, nrm, samples, first_sample, ids, mask, offset=1e-3, shorten=1e-3):
    """direct.fold of the model's contributions under rb_occluded's bytes on the model's own records and bounds"""
    o, d, tmax, contrib = direct.rays(table, hemisphere.surfels(pts, nrm), first_sample, samples, seeds=ids, offset=offset, shorten=shorten, cdf=cdf)
    rays = np.zeros(len(o), dtype=abi.RAY)
    rays["origin"], rays["dir"] = o, d
    return direct.fold(contrib, e.occluded_records(rays, tmax, mask), samples)


@pytest.mark.parametrize("name", ["feature", "mesh chunk", "mesh bvh", "lamps"])
def test_sums_equal_the_fold_of_the_model(name):
    make, kw, kernel = WALKS[name]
    s = make()
    table = direct.scene_emitters(s)
    cdf = direct.emitter_cdf(table)
    assert len(table) > 0 and int(cdf[-1]) > 0
    e = _engine(s, **kw)
    try:
        pts, nrm = mixed_surfels(e, s)
        uniform = e.direct_light(pts, nrm, 4, first_sample=7)
        st0, lit = e.stats(), 0
        for samples, first_sample, with_seeds, mask in ((3, 0, False, abi.MASK_ALL), (4, 7, True, abi.MASK_ALL), (5, 7, False, NO_LIGHTS)):
            ids = given_seeds(M) if with_seeds else None
            where = (name, samples, first_sample, with_seeds, mask)
            got = e.direct_light(pts, nrm, samples, first_sample=first_sample, seeds=ids, mask=mask, pick="power")   # NULL emitters
            assert e.last_query_kernel_name() == kernel, e.last_query_kernel_name()
            assert e.last_query_ms() > 0 and 0 < e.last_camera_rays_ms() <= e.last_query_ms()
            same_rows(got, model_sums(e, table, cdf, pts, nrm, samples, first_sample, ids, mask), where)
            assert got.dtype == abi.RADIANCE
            # a caller's table equal to the scene's: its power, and its weights given
            same_rows(e.direct_light(pts, nrm, samples, emitters=table, first_sample=first_sample, seeds=ids, mask=mask, pick="power"), got, where)
            same_rows(e.direct_light(pts, nrm, samples, emitters=table, first_sample=first_sample, seeds=ids, mask=mask, pick=cdf), got, where)
            lit += int((got["sum"] != 0).any(1).sum())
        assert lit > 0
        # a caller's weights: a group switched off, one boosted
        own = caller_tables(table)["own"]
        same_rows(e.direct_light(pts, nrm, 4, emitters=table, pick=own), model_sums(e, table, own, pts, nrm, 4, 0, None, abi.MASK_ALL), (name, "own"))
        # the ramp is the uniform pick, and rb_direct_light's own sums have not moved
        ramp = np.arange(1, len(table) + 1, dtype=u32)
        same_rows(e.direct_light(pts, nrm, 4, emitters=table, first_sample=7, pick=ramp), uniform, (name, "ramp"))
        same_rows(e.direct_light(pts, nrm, 4, first_sample=7), uniform, (name, "uniform after"))
        none = e.direct_light(pts, nrm, 4, emitters=table[:0], pick="power")
        assert not _u32(none["sum"]).any() and np.array_equal(none["weight"], uniform["weight"])
        assert e.stats() == st0, "direct-light queries moved rb_get_stats"
    finally:
        e.close()


GARBAGE = {"decreasing": lambda n: np.arange(n, 0, -1, dtype=u32) * u32(3), "total 0": lambda n: np.zeros(n, u32),
           "total above 2^24": lambda n: np.concatenate([np.arange(1, n, dtype=u32), [TOP + 1]]).astype(u32),
           "all equal": lambda n: np.full(n, 6, u32), "wrapping": lambda n: np.concatenate([[0xFFFFFFFF], np.arange(1, n, dtype=u32)]).astype(u32),
           "a dip": lambda n: np.where(np.arange(n) == 1, 0, np.arange(1, n + 1) * 5).astype(u32)}


def test_malformed_tables_through_the_device_form():
    """No host form takes these; the device form cannot look and does not: section 23.1 defines the result, and the search
    stays inside the table by construction."""
    import torch
    for make in (lambda: scenes.feature_scene(width=24, height=16), long_table):
        s = make()
        table = direct.scene_emitters(s)
        n = len(table)
        e = _engine(s)
        try:
            pts, nrm = scene_surfels(e, s, 70)
            tp, tn = torch.from_numpy(pts).cuda(), torch.from_numpy(nrm).cuda()
            ttab = torch.from_numpy(table.view(f32).reshape(-1, 16)).cuda()
            for name, f in GARBAGE.items():
                cdf = f(n)
                assert len(cdf) == n
                if (np.diff(cdf.astype(np.int64)) < 0).any() or int(cdf[-1]) > TOP:
                    with pytest.raises(Exception):
                        e.direct_light(pts, nrm, 5, emitters=table, pick=cdf)   # the host form refuses it
                got = e.direct_light(tp, tn, 5, emitters=ttab, pick=torch.from_numpy(cdf.view(np.int32)).cuda())
                want = model_sums(e, table, cdf, pts, nrm, 5, 0, None, abi.MASK_ALL)
                same_rows(got.cpu().numpy(), want.view(f32).reshape(-1, 4), (s.name, name))
                if name in ("total 0", "total above 2^24"):
                    assert not _u32(want["sum"]).any() and (want["weight"] == 5).all()
        finally:
            e.close()


# ---- 4. forms and pieces
def test_device_forms_and_a_forced_launch_shape_equal_the_host_forms():
    import torch
    s = _mesh()
    table = direct.scene_emitters(s)
    cdf = direct.emitter_cdf(table)
    own = caller_tables(table)["own"]
    e = _engine(s)
    try:
        pts, nrm = mixed_surfels(e, s)
        ids = given_seeds(M)
        tp, tn = torch.from_numpy(pts).cuda(), torch.from_numpy(nrm).cuda()
        tids = torch.from_numpy(ids.view(np.int32)).cuda()
        ttab = torch.from_numpy(table.view(f32).reshape(-1, 16)).cuda()
        town = torch.from_numpy(own.view(np.int32)).cuda()
        rad = e.direct_light(pts, nrm, 5, first_sample=7, seeds=ids, pick="power")
        mine = e.direct_light(pts, nrm, 5, emitters=table, first_sample=7, seeds=ids, pick=own)
        assert (rad["sum"] != 0).any(1).sum() > 20 and not np.array_equal(_u32(rad), _u32(mine))
        d_rad = e.direct_light(tp, tn, 5, first_sample=7, seeds=tids, pick="power")
        assert e.last_query_kernel_name() == "k_occl_chunk" and e.last_query_ms() > 0 and e.last_camera_rays_ms() > 0
        assert d_rad.shape == (M, 4) and d_rad.is_cuda
        same_rows(d_rad.cpu().numpy(), rad.view(f32).reshape(-1, 4), "device, the scene's")
        same_rows(e.direct_light(tp, tn, 5, emitters=ttab, first_sample=7, seeds=tids, pick="power").cpu().numpy(), rad.view(f32).reshape(-1, 4), "device, by power")
        same_rows(e.direct_light(tp, tn, 5, emitters=ttab, first_sample=7, seeds=tids, pick=town).cpu().numpy(), mine.view(f32).reshape(-1, 4), "device, own")
        # a numpy table of weights beside tensors is uploaded
        same_rows(e.direct_light(tp, tn, 5, emitters=table, first_sample=7, seeds=tids, pick=own).cpu().numpy(), mine.view(f32).reshape(-1, 4), "uploaded")
        # fewer than 64 surfels go in linear order: one surfel at many samples, 63, and 64 beside them
        for first, n, samples in ((0, 1, 300), (60, 63, 7), (60, 64, 7)):
            sl = slice(first, first + n)
            got = e.direct_light(pts[sl], nrm[sl], samples, first_sample=2, seeds=ids[sl], pick="power")
            same_rows(got, model_sums(e, table, cdf, pts[sl], nrm[sl], samples, 2, ids[sl], abi.MASK_ALL), (first, n, samples))
            d_got = e.direct_light(tp[sl], tn[sl], samples, first_sample=2, seeds=tids[sl], pick="power")
            same_rows(d_got.cpu().numpy(), got.view(f32).reshape(-1, 4), (first, n, samples))
        assert len(e.direct_light(pts[:0], nrm[:0], 5, pick="power")) == 0
        # bake passes the pick through
        mean = bake.direct_irradiance(e, pts, nrm, 5, first_sample=7, seeds=ids, pick="power")
        assert np.array_equal(_u32(mean), _u32(np.where(rad["weight"][:, None] > 0, rad["sum"] / np.maximum(rad["weight"], 1)[:, None], 0).astype(f32)))
        # the launch shape: reservations of 64 items on a grid of one block per CU
        o = _engine(s, queue_batch=64, blocks_per_cu=1)
        try:
            same_rows(o.direct_light(pts, nrm, 5, first_sample=7, seeds=ids, pick="power"), rad, "forced shape")
        finally:
            o.close()
        for bad in (dict(pick=town), dict(pick=own[:-1], emitters=table), dict(pick="brightest")):
            with pytest.raises(ValueError):
                e.direct_light(pts, nrm, 1, **bad)
    finally:
        e.close()


def test_a_call_across_a_piece_boundary():
    """RB_HEMI_PIECE_ITEMS + 77 * samples items at samples = 64 on the feature scene: two pieces, which share the one table of
    weights.  The whole call against two calls split at the boundary, the surfels around the boundary against the fold of the
    model, both against the device form."""
    import torch
    samples = 64
    b = PIECE // samples
    n = b + 77
    s = scenes.feature_scene(width=24, height=16)
    table = direct.scene_emitters(s)
    cdf = direct.emitter_cdf(table)
    e = _engine(s)
    try:
        p0, n0 = scene_surfels(e, s, 200)
        idx = np.arange(n) % 200
        pts, nrm = np.ascontiguousarray(p0[idx]), np.ascontiguousarray(n0[idx])
        ids = np.arange(n, dtype=np.uint32)
        one = e.direct_light(pts, nrm, samples, first_sample=7, pick="power")
        assert e.last_query_kernel_name() == "k_occl" and e.last_query_ms() > 0
        two = np.concatenate([e.direct_light(pts[:b], nrm[:b], samples, first_sample=7, pick="power"),
                              e.direct_light(pts[b:], nrm[b:], samples, first_sample=7, seeds=ids[b:], pick="power")])
        same_rows(one, two, "split")
        assert (one["weight"] == samples).all() and (one["sum"] != 0).any(1).sum() > 1000
        tail = slice(b - 32, n)
        same_rows(one[tail], model_sums(e, table, cdf, pts[tail], nrm[tail], samples, 7, ids[tail], abi.MASK_ALL), "tail")
        d_pts, d_nrm = (torch.from_numpy(a).to(f"cuda:{e.query_device}") for a in (pts, nrm))
        dev = e.direct_light(d_pts, d_nrm, samples, first_sample=7, emitters=table, pick="power")   # weights made for the call, queued
        assert e.last_camera_rays_ms() > 0
        same_rows(dev.cpu().numpy(), one.view(f32).reshape(n, 4), "device")
    finally:
        e.close()


def test_sharded_engine_and_multi_device_handle():
    import torch
    s = scenes.feature_scene(width=24, height=16)
    e = _engine(s)
    pts, nrm = scene_surfels(e, s)
    want, cdf = e.direct_light(pts, nrm, 2, first_sample=7, pick="power"), e.scene_emitter_cdf()
    e.close()
    tp, tn = torch.from_numpy(pts).cuda(), torch.from_numpy(nrm).cuda()
    for kw in (dict(shard_rank=1, shard_count=3, stripe_rows=8), dict(devices=[0, 0], gather_peer_copy=True)):
        p = _engine(s, **kw)
        try:
            same_rows(p.direct_light(pts, nrm, 2, first_sample=7, pick="power"), want, kw)
            assert np.array_equal(p.scene_emitter_cdf(), cdf), kw
            same_rows(p.direct_light(tp, tn, 2, first_sample=7, pick="power").cpu().numpy(), want.view(f32).reshape(-1, 4), kw)
            assert p.last_query_kernel_name() == "k_occl" and p.last_query_ms() > 0
        finally:
            p.close()


# ---- 5. refusals
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
    cdf = direct.emitter_cdf(tab)
    assert len(tab) == 2
    try:
        e.update(rc)
        h = e._h
        base = _params()
        uniform = e.direct_light(pts, nrm, 2)
        before = e.direct_light(pts, nrm, 2, pick="power")
        assert (before["sum"] != 0).any()
        d_surf = torch.from_numpy(surf.view(f32).reshape(-1, 8)).cuda()
        d_tab = torch.from_numpy(tab.view(f32).reshape(-1, 16)).cuda()
        d_cdf = torch.from_numpy(cdf.view(np.int32)).cuda()
        out = np.full(64, 7, dtype=abi.RADIANCE)
        d_out = torch.full((64, 4), 7, dtype=torch.float32, device="cuda")
        for fn, tp, cp, sp, o in ((lib.rb_direct_light_cdf, tab.ctypes.data, cdf.ctypes.data, surf.ctypes.data, out.ctypes.data),
                                  (lib.rb_direct_light_cdf_device, d_tab.data_ptr(), d_cdf.data_ptr(), d_surf.data_ptr(), d_out.data_ptr())):
            for name, kw in REFUSALS:
                args = dict(n=4, first_sample=0, samples=2, params=base, n_emit=2)
                args.update(kw)
                tail = (sp, None, args["n"], args["params"].ctypes.data, args["first_sample"], args["samples"], o)
                assert fn(h, tp, cp, args["n_emit"], *tail) == INVALID_OPTIONS, name
                assert fn(h, tp, None, args["n_emit"], *tail) == INVALID_OPTIONS, name
                assert lib.rb_last_error(h)
                if "n_emit" not in kw:   # ... and with the scene's own table
                    assert fn(h, None, None, 0, *tail) == INVALID_OPTIONS, name
            for name, fields in MASK_REFUSALS:
                assert fn(h, tp, cp, 2, sp, None, 4, _params(**fields).ctypes.data, 0, 2, o) == INVALID_OPTIONS, name
            # a table of weights without a table of emitters
            assert fn(h, None, cp, 2, sp, None, 4, base.ctypes.data, 0, 2, o) == INVALID_OPTIONS
            assert fn(h, None, cp, 0, None, None, 0, base.ctypes.data, 0, 2, None) == INVALID_OPTIONS   # in an empty call too
            assert fn(h, tp, cp, 2, None, None, 4, base.ctypes.data, 0, 2, o) == NULL_ARGUMENT and fn(h, tp, cp, 2, sp, None, 4, None, 0, 2, o) == NULL_ARGUMENT
            assert fn(h, tp, cp, 2, sp, None, 4, base.ctypes.data, 0, 2, None) == NULL_ARGUMENT
            assert fn(h, None, None, 0, None, None, 0, base.ctypes.data, 0, 2, None) == 0 and fn(h, None, None, 0, None, None, 0, None, 0, 2, None) == 0
        # the host form looks at a caller's weights
        for name, bad in BAD_TABLES:
            assert lib.rb_direct_light_cdf(h, tab.ctypes.data, bad.ctypes.data, 2, surf.ctypes.data, None, 4, base.ctypes.data, 0, 2, out.ctypes.data) == INVALID_OPTIONS, name
        lib.rb_sync(h)
        assert (out.view(np.uint32) == np.float32(7).view(np.uint32)).all() and (d_out == 7).all().item()
        # the device form's buffers: d_cdf in host memory, misaligned, in an allocation that ends before its entries
        dev, bp = lib.rb_direct_light_cdf_device, base.ctypes.data
        good = (d_surf.data_ptr(), None, 4, bp, 0, 2, d_out.data_ptr())
        assert dev(h, d_tab.data_ptr(), cdf.ctypes.data, 2, *good) == INVALID_OPTIONS
        assert dev(h, d_tab.data_ptr(), d_cdf.data_ptr() + 2, 1, *good) == INVALID_OPTIONS
        assert dev(h, d_tab.data_ptr(), d_surf.data_ptr(), 1 << 20, *good) == INVALID_OPTIONS
        assert dev(h, tab.ctypes.data, d_cdf.data_ptr(), 2, *good) == INVALID_OPTIONS
        assert dev(h, None, None, 0, surf.ctypes.data, None, 4, bp, 0, 2, d_out.data_ptr()) == INVALID_OPTIONS
        assert dev(h, None, None, 0, d_surf.data_ptr(), None, 4, bp, 0, 2, out.ctypes.data) == INVALID_OPTIONS
        cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        count = C.c_size_t(0)
        assert lib.rb_scene_emitter_cdf(h, None, 0, None) == NULL_ARGUMENT and lib.rb_scene_emitter_cdf(h, None, 2, C.byref(count)) == NULL_ARGUMENT
        assert lib.rb_scene_emitter_cdf_device(h, d_cdf.data_ptr(), 2, None) == NULL_ARGUMENT
        assert lib.rb_scene_emitter_cdf_device(h, cdf.ctypes.data, 2, cnt.data_ptr()) == INVALID_OPTIONS
        assert lib.rb_scene_emitter_cdf_device(h, d_cdf.data_ptr(), 1 << 20, cnt.data_ptr()) == INVALID_OPTIONS
        assert lib.rb_scene_emitter_cdf_device(h, d_cdf.data_ptr() + 2, 1, cnt.data_ptr()) == INVALID_OPTIONS
        assert lib.rb_scene_emitter_cdf_device(h, d_cdf.data_ptr(), 2, cnt.data_ptr() + 2) == INVALID_OPTIONS
        assert (d_out == 7).all().item() and int(cnt.item()) == 0
        assert dev(h, None, None, 0, *good) == 0 and lib.rb_sync(h) == 0
        same_rows(d_out.cpu().numpy()[:4], before.view(f32).reshape(4, -1), "after the refusals")
        assert (d_out[4:] == 7).all().item()
        same_rows(e.direct_light(pts, nrm, 2, pick="power"), before, "host, after the refusals")
        same_rows(e.direct_light(pts, nrm, 2), uniform, "the uniform pick")
        assert np.array_equal(e.render(rc).pixels, _oracle.render(s)[2])
    finally:
        e.close()
    cold = Engine.new(rc, device=0)   # no update yet: not ready, and still a refusal first
    try:
        out = np.zeros(4, dtype=abi.RADIANCE)
        count = C.c_size_t(0)
        for tp, cp in ((None, None), (tab.ctypes.data, None), (tab.ctypes.data, cdf.ctypes.data)):
            assert lib.rb_direct_light_cdf(cold._h, tp, cp, 2, surf.ctypes.data, None, 4, base.ctypes.data, 0, 2, out.ctypes.data) not in (0, INVALID_OPTIONS)
        assert lib.rb_direct_light_cdf(cold._h, None, None, 0, surf.ctypes.data, None, 4, base.ctypes.data, 0, 0, out.ctypes.data) == INVALID_OPTIONS
        assert lib.rb_scene_emitter_cdf(cold._h, None, 0, C.byref(count)) not in (0, INVALID_OPTIONS)
        assert np.array_equal(cold.render(rc).pixels, _oracle.render(s)[2])
    finally:
        cold.close()


# ---- 6. the layer above
def test_lightmap_direct_passes_the_pick_through():
    s = scenes.feature_scene(width=24, height=16)
    e = _engine(s)
    try:
        w, h, samples = 24, 16, 4
        got = bake.lightmap_direct(e, w, h, samples, first_sample=2, dilate=1, pick="power")
        surf, own = e.lightmap_surfels(w, h)
        sums = e.direct_light(surf, None, samples, first_sample=2, pick="power")
        assert got.shape == (h, w, 4) and np.array_equal(_u32(got), _u32(engine.lightmap_resolve(sums, w, h, dilate=1, device=0)))
        assert not np.array_equal(_u32(got), _u32(bake.lightmap_direct(e, w, h, samples, first_sample=2, dilate=1)))
    finally:
        e.close()
