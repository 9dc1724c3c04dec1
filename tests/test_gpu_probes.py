"""Irradiance probes made on the device (rb_probe_rays / rb_bake_probes / rb_bake_probes_device), bit for
bit on uint32 views:

  the generator  = the numpy model renderbaby_amd/probes.py: origin, direction, seed and pad words of every record;
  the projection = probes.project over the unmodified oracle's rbo_trace_ray(scene, o, d, seed) of the very records
                   rb_probe_rays returned, all 28 words of every probe, for every k_cam kernel;
  the forms and the pieces give the same answers, and a call has a query's side effects: none;
  and the coefficients mean what section 18 says: a uniform sky comes back as its colour, a lamp pulls band 1 towards it.
"""

import numpy as np
import pytest

from renderbaby_amd import Engine, RenderConfig, abi, bake, engine, probes, scenes
from tests import _oracle
from tests.conftest import has_gpu
from tests.test_gpu_camera import oracle_sums
from tests.test_gpu_hemisphere import _mesh_beside_spheres, scene_surfels
from tests.test_gpu_query import FAR_LIGHT, _engine
from tests.test_gpu_radiance import _mesh, _u32, given_seeds
from tests.test_probe_abi import INVALID_OPTIONS, NULL_ARGUMENT, REFUSALS

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

f32 = np.float32
PIECE = abi.PROBE_PIECE_ITEMS
AXES = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], f32)
INVALID = [(np.inf, 0, 0), (0, np.nan, 0), (1, 2, -np.inf)]


def words(sh):
    """(n, 28) uint32 of abi.SH9 records or of an (n, 28) float32 array"""
    return _u32(np.ascontiguousarray(sh).view(f32).reshape(-1, 28))


def model_probes(m, seed=4):
    """m positions for the generator: random ones, then from the front an Inf, a NaN and a -Inf component (invalid probes)
    and 3e38 (valid: the origin takes no offset); position 0 keeps a valid one"""
    rng = np.random.default_rng(seed)
    pos = (rng.normal(size=(m, 3)) * 3.0).astype(f32)
    for j, p in enumerate(INVALID + [(3e38, 3e38, 3e38), (-0.0, 0.0, 1e-30)]):
        i = 1 + 3 * j   # spread over the first block of 64 where m allows it
        if i < m:
            pos[i] = p
    return pos


def scene_probes(e, scene, m=130):
    """the first m hit points of render_hits pushed 0.05 along their normals (turned towards the camera): free space"""
    pts, nrm = scene_surfels(e, scene, m)
    return np.ascontiguousarray((pts + f32(0.05) * nrm).astype(f32))


def oracle_sh(scene, rays, seeds, samples):
    """abi.SH9[n] from the records of rb_probe_rays: rbo_trace_ray per valid record (an invalid one: {0, 0, 0, 0}, max_depth 0:
    {0, 0, 0, 1}), folded by the model in sample order"""
    per = oracle_sums(scene, rays, seeds, 1)
    col = np.concatenate([per["sum"], per["weight"][:, None]], axis=1).astype(f32)
    return probes.project(rays["dir"], col, samples)


# ---- 1. the generator against the model
@pytest.mark.parametrize("with_seeds", [False, True], ids=["index", "seeds"])
def test_generator_equals_the_model(with_seeds):
    n_invalid = 0
    for m in (1, 63, 65, 130):
        pos = model_probes(m)
        ids = given_seeds(m) if (with_seeds and m >= 7) else (np.arange(m, dtype=np.uint32) * np.uint32(2654435761) if with_seeds else None)
        ranges = [(0, m)] + ([(70, 60), (127, 2), (64, 64)] if m == 130 else [])   # 70 .. 129: starts and ends inside a block of 64
        for first, n in ranges:
            for samples, first_sample in ((1, 0), (2, 7), (5, 7)):
                sl = slice(first, first + n)
                sid = None if ids is None else ids[sl]
                rays, seeds = engine.probe_rays_device(pos[sl], samples, first_sample, seeds=sid, device=0)
                o, d, s = probes.rays(pos[sl], first_sample, samples, seeds=sid)
                where = (with_seeds, m, first, n, samples, first_sample)
                assert rays.shape == (n * samples,) and seeds.shape == (n * samples,), where
                assert np.array_equal(seeds, s), where
                assert np.array_equal(_u32(rays["origin"]), _u32(o)), where
                bad = np.nonzero((_u32(rays["dir"]) != _u32(d)).any(1))[0]
                assert len(bad) == 0, (where, bad[:5], rays["dir"][bad[:5]], d[bad[:5]])
                assert (_u32(rays["_pad0"]) == 0).all() and (_u32(rays["_pad1"]) == 0).all(), where
                n_invalid += int((_u32(rays["dir"]) == 0).all(1).sum())
                if ids is None and first > 0:   # seeds = NULL names a probe by its index in the CALL
                    whole = probes.rays(pos, first_sample, samples)[2]
                    assert not np.array_equal(s, whole[first * samples:(first + n) * samples])
    assert n_invalid > 0, "no invalid probe was mixed in"


def test_generator_without_seeds_out_keeps_the_seed_in_the_record():
    from renderbaby_amd._lib import load
    pos = model_probes(65)
    rec = probes.records(pos)
    rays = np.zeros(65 * 3, dtype=abi.RAY)
    assert load().rb_probe_rays(0, rec.ctypes.data, None, 65, 7, 3, rays.ctypes.data, None) == 0
    o, d, s = probes.rays(pos, 7, 3)
    assert np.array_equal(_u32(rays["_pad0"]), s) and (_u32(rays["_pad1"]) == 0).all()
    assert np.array_equal(_u32(rays["origin"]), _u32(o)) and np.array_equal(_u32(rays["dir"]), _u32(d))


# ---- 2. the projection against the model over the oracle's colours
def check_bake(scene, kernel, **kw):
    e = _engine(scene, **kw)
    try:
        pos = scene_probes(e, scene)
        st0, band1, band2 = e.stats(), 0, 0
        for samples, first_sample, ids in ((5, 7, None), (1, 0, given_seeds(len(pos)))):
            got = e.bake_probes(pos, samples, first_sample, seeds=ids)
            assert e.last_query_kernel_name() == kernel, e.last_query_kernel_name()
            assert e.last_query_ms() > 0 and 0 < e.last_camera_rays_ms() <= e.last_query_ms()
            assert 0 < e.last_probe_project_ms() <= e.last_query_ms()
            rays, seeds = engine.probe_rays_device(pos, samples, first_sample, seeds=ids, device=0)
            want = oracle_sh(scene, rays, seeds, samples)
            bad = np.nonzero((words(got) != words(want)).any(1))[0]
            assert got.dtype == abi.SH9 and len(bad) == 0, (scene.name, kernel, samples, len(bad), bad[:3], got[bad[:3]], want[bad[:3]])
            assert (got["weight"] == samples).all()
            band1 += int((got["sum"][:, 1:4] != 0).sum())
            band2 += int((got["sum"][:, 4:9] != 0).sum())
        assert band1 > 0 and band2 > 0, "no probe of the scene carried any directional light"
        assert e.stats() == st0, "probe bakes moved rb_get_stats"
    finally:
        e.close()


@pytest.mark.parametrize("color_hash", [0, 1])
def test_feature_scene(color_hash):
    check_bake(scenes.feature_scene(width=24, height=16, color_hash=color_hash), "k_cam")


@pytest.mark.parametrize("kw,kernel", [(dict(), "k_cam_chunk"), (dict(reference_walk=True), "k_cam_bvh")])
def test_multi_node_mesh(kw, kernel):
    s = _mesh()
    assert len(s.bvh_triangles) == 578
    check_bake(s, kernel, **kw)


def test_mesh_beside_a_sphere_tree():
    check_bake(_mesh_beside_spheres(), "k_cam_chunk")


# ---- 3. depth 0 and 1, invalid probes mixed in
def test_depth_zero_and_one_and_invalid_probes():
    s = scenes.feature_scene(width=24, height=16)
    for depth in (0, 1):
        sd = s.with_params(max_depth=depth)
        e = _engine(sd)
        try:
            pos = scene_probes(e, sd)
            for j in range(1, 130, 3):
                pos[j] = INVALID[(j // 3) % 3]
            got = e.bake_probes(pos, 3)
            rays, seeds = engine.probe_rays_device(pos, 3, device=0)
            want = oracle_sh(sd, rays, seeds, 3)
            assert np.array_equal(words(got), words(want))
            gone = (rays["dir"] == 0).all(1).reshape(130, 3).all(1)
            assert gone.sum() == 43 and (words(got[gone]) == 0).all() and (got["weight"][~gone] == 3).all()   # 28 words of +0
            if depth == 0:
                assert (_u32(got["sum"]) == 0).all()
            else:
                assert (got["sum"][~gone][:, 0] != 0).any(1).sum() > 20   # the winner's emission, the sky for a miss
        finally:
            e.close()


# ---- 4. forms and launch shapes
def test_device_forms_and_a_forced_launch_shape_equal_the_host_forms():
    import torch
    s = _mesh()
    e = _engine(s)
    try:
        pos = scene_probes(e, s)
        pos[1::9] = INVALID[0]
        ids = given_seeds(130)
        tp = torch.from_numpy(pos).cuda()
        tids = torch.from_numpy(ids.view(np.int32)).cuda()
        for sid, tsid in ((None, None), (ids, tids)):
            sh = e.bake_probes(pos, 5, 7, seeds=sid)
            d_sh = e.bake_probes(tp, 5, 7, seeds=tsid)
            assert e.last_query_kernel_name() == "k_cam_chunk" and e.last_query_ms() > 0
            assert d_sh.shape == (130, 28) and d_sh.is_cuda and d_sh.dtype == torch.float32
            assert np.array_equal(words(d_sh.cpu().numpy()), words(sh))
        # out= : an array or a tensor to fill
        filled = np.zeros(130, dtype=abi.SH9)
        assert e.bake_probes(pos, 5, 7, seeds=ids, out=filled) is filled and np.array_equal(words(filled), words(sh))
        out = torch.full((130, 28), -1.0, dtype=torch.float32, device="cuda")
        assert e.bake_probes(tp, 5, 7, seeds=tids, out=out) is out and np.array_equal(words(out.cpu().numpy()), words(sh))
        # sub-ranges with their ids equal the whole call's records
        for first, n in ((70, 60), (127, 2), (64, 64), (0, 1), (129, 1)):
            sl = slice(first, first + n)
            assert np.array_equal(words(e.bake_probes(pos[sl], 5, 7, seeds=ids[sl])), words(sh[sl])), (first, n)
        assert len(e.bake_probes(pos[:0], 5)) == 0
        # accumulating over calls with first_sample is the caller's: the halves are what a call of their samples gives
        a, b = e.bake_probes(pos, 2, 7, seeds=ids), e.bake_probes(pos, 3, 9, seeds=ids)
        assert np.array_equal(a["weight"] + b["weight"], sh["weight"])
        # bake.probes: the coefficients of the same sums
        L = bake.probes(e, pos, 5, first_sample=7, seeds=ids)
        assert L.shape == (130, 9, 3) and np.array_equal(L, probes.radiance_coefficients(sh))
        assert np.array_equal(bake.probes(e, tp, 5, first_sample=7, seeds=tids), L)
        # the launch shape: reservations of 64 items on a grid of one block per CU
        o = _engine(s, queue_batch=64, blocks_per_cu=1)
        try:
            assert np.array_equal(words(o.bake_probes(pos, 5, 7, seeds=ids)), words(sh))
        finally:
            o.close()
        for bad in (dict(out=np.zeros(130, f32)), dict(out=out[:5]), dict(out=out[:, :3]), dict(samples=-1), dict(seeds=ids[:5])):
            with pytest.raises(ValueError):
                e.bake_probes(pos, **dict(dict(samples=1), **bad))
    finally:
        e.close()


def test_both_projection_shapes_give_the_same_words(monkeypatch):
    """RB_PROBE_SHAPE chooses between one wave per 64 probes and three waves with three coefficients each"""
    s = scenes.feature_scene(width=24, height=16)
    e = _engine(s)
    try:
        pos = scene_probes(e, s)
        pos[4] = INVALID[1]
        got = {}
        for shape in ("plain", "split"):
            monkeypatch.setenv("RB_PROBE_SHAPE", shape)
            got[shape] = [e.bake_probes(pos[:n], samples, 7) for n, samples in ((130, 11), (1, 1), (64, 8), (65, 16))]
        monkeypatch.delenv("RB_PROBE_SHAPE")
        for a, b in zip(got["plain"], got["split"]):
            assert np.array_equal(words(a), words(b))
        rays, seeds = engine.probe_rays_device(pos, 11, 7, device=0)
        assert np.array_equal(words(got["split"][0]), words(oracle_sh(s, rays, seeds, 11)))
    finally:
        e.close()


# ---- 5. pieces
def test_a_call_across_a_piece_boundary():
    """RB_PROBE_PIECE_ITEMS + 77 * samples items at samples = 64 on the feature scene: two pieces.  Every probe against two
    calls split at the piece boundary (seeds carry the indices on); the last 77 probes and the 32 before the boundary against
    the oracle; every probe against the device form's answer, whose two pieces go through the same loop on the caller's buffers."""
    import torch
    samples = 64
    b = PIECE // samples
    n = b + 77
    s = scenes.feature_scene(width=24, height=16)
    e = _engine(s)
    try:
        p0 = scene_probes(e, s, 200)
        pos = np.ascontiguousarray(p0[np.arange(n) % 200])
        ids = np.arange(n, dtype=np.uint32)
        one = e.bake_probes(pos, samples, 7)
        assert e.last_query_kernel_name() == "k_cam" and e.last_query_ms() > 0
        two = np.concatenate([e.bake_probes(pos[:b], samples, 7), e.bake_probes(pos[b:], samples, 7, seeds=ids[b:])])
        assert np.array_equal(words(one), words(two))
        assert (one["weight"] == samples).all() and (one["sum"][:, 0] != 0).any(1).sum() > 1000
        assert not np.array_equal(words(one[:200]), words(one[200:400]))   # the same probes under other ids
        tail = slice(b - 32, n)
        rays, seeds = engine.probe_rays_device(pos[tail], samples, 7, seeds=ids[tail], device=0)
        assert np.array_equal(words(one[tail]), words(oracle_sh(s, rays, seeds, samples)))
        dev = e.bake_probes(torch.from_numpy(pos).to(f"cuda:{e.query_device}"), samples, 7)
        assert e.last_camera_rays_ms() > 0 and e.last_probe_project_ms() > 0   # both pieces' event pairs were recorded and are read
        assert np.array_equal(words(dev.cpu().numpy()), words(one))
    finally:
        e.close()


# ---- 6. side effects, refusals, shards
def test_a_probe_bake_between_iterator_frames():
    s = scenes.feature_scene(width=48, height=32, spp=4)
    rc = RenderConfig.from_scene(s)
    small = scenes.feature_scene(width=24, height=16)
    first = _engine(small)
    pos = scene_probes(first, small)
    first.close()

    def frames(query):
        e = Engine.new(rc, device=0)
        it = e.frame_iterator(rc)
        out, answers = [], []
        while it.has_next():
            out.append(it.next().pixels.copy())
            if query:
                kernel = e.last_kernel_name()
                answers.append(e.bake_probes(pos, 3))
                assert e.last_kernel_name() == kernel and e.last_query_kernel_name() == "k_cam"
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
    for sh in answers[1:]:
        assert np.array_equal(words(sh), words(answers[0]))


def test_refusals_leave_the_engine_rendering_the_golden_frame():
    import torch
    from renderbaby_amd._lib import load
    lib = load()
    s = scenes.cornell(32, 32, 2, 4)
    rc = RenderConfig.from_scene(s)
    e = Engine.new(rc, device=0)
    pos = np.array([(0.0, 0.1 * i + 0.2, 0.0) for i in range(4)], f32)
    rec = probes.records(pos)
    try:
        e.update(rc)
        h = e._h
        before = e.bake_probes(pos, 2)
        d_rec = torch.from_numpy(rec.view(f32).reshape(-1, 4)).cuda()
        out = np.full(64, 7, dtype=abi.SH9)
        d_out = torch.full((64, 28), 7, dtype=torch.float32, device="cuda")
        for fn, pp, o in ((lib.rb_bake_probes, rec.ctypes.data, out.ctypes.data), (lib.rb_bake_probes_device, d_rec.data_ptr(), d_out.data_ptr())):
            for name, kw in REFUSALS:
                args = dict(n=4, first_sample=0, samples=2)
                args.update(kw)
                assert fn(h, pp, None, args["n"], args["first_sample"], args["samples"], o) == INVALID_OPTIONS, name
                assert lib.rb_last_error(h)
            assert fn(h, None, None, 4, 0, 2, o) == NULL_ARGUMENT and fn(h, pp, None, 4, 0, 2, None) == NULL_ARGUMENT
            assert fn(h, None, None, 0, 0, 2, None) == 0   # n == 0
        lib.rb_sync(h)
        assert (out.view(f32) == 7).all() and (d_out == 7).all().item()
        # the device form's buffers: a host pointer, a misaligned one, an allocation that ends before n elements
        dev_fn = lib.rb_bake_probes_device
        assert dev_fn(h, rec.ctypes.data, None, 4, 0, 2, d_out.data_ptr()) == INVALID_OPTIONS
        assert dev_fn(h, d_rec.data_ptr(), None, 4, 0, 2, out.ctypes.data) == INVALID_OPTIONS
        assert dev_fn(h, d_rec.data_ptr() + 4, None, 3, 0, 2, d_out.data_ptr()) == INVALID_OPTIONS
        assert dev_fn(h, d_rec.data_ptr(), None, 4, 0, 2, d_out.data_ptr() + 4) == INVALID_OPTIONS
        assert dev_fn(h, d_rec.data_ptr(), None, 1 << 20, 0, 1, d_out.data_ptr()) == INVALID_OPTIONS
        assert dev_fn(h, d_rec.data_ptr(), d_out.data_ptr() + 2, 4, 0, 2, d_out.data_ptr()) == INVALID_OPTIONS   # d_seeds
        assert (d_out == 7).all().item()
        assert dev_fn(h, d_rec.data_ptr(), None, 4, 0, 2, d_out.data_ptr()) == 0 and lib.rb_sync(h) == 0
        assert np.array_equal(words(d_out.cpu().numpy()[:4]), words(before)) and (d_out[4:] == 7).all().item()
        assert np.array_equal(words(e.bake_probes(pos, 2)), words(before))
        assert np.array_equal(e.render(rc).pixels, _oracle.render(s)[2])
    finally:
        e.close()
    cold = Engine.new(rc, device=0)   # no update yet: not ready, and still a refusal first
    try:
        out = np.zeros(4, dtype=abi.SH9)
        assert lib.rb_bake_probes(cold._h, rec.ctypes.data, None, 4, 0, 2, out.ctypes.data) not in (0, INVALID_OPTIONS)
        assert lib.rb_bake_probes(cold._h, rec.ctypes.data, None, 4, 0, 0, out.ctypes.data) == INVALID_OPTIONS
        assert np.array_equal(cold.render(rc).pixels, _oracle.render(s)[2])
    finally:
        cold.close()


def test_sharded_engine_and_multi_device_handle():
    """both forms on a sharded engine (a probe sees the whole scene) and on a multi-device handle on one device"""
    import torch
    s = scenes.feature_scene(width=24, height=16)
    e = _engine(s)
    pos = scene_probes(e, s)
    want = e.bake_probes(pos, 2, 7)
    e.close()
    tp = torch.from_numpy(pos).cuda()
    for kw in (dict(shard_rank=1, shard_count=3, stripe_rows=8), dict(devices=[0, 0], gather_peer_copy=True)):
        p = _engine(s, **kw)
        try:
            assert np.array_equal(words(p.bake_probes(pos, 2, 7)), words(want)), kw
            dev = p.bake_probes(tp, 2, 7)
            assert np.array_equal(words(dev.cpu().numpy()), words(want)), kw
            assert p.last_query_kernel_name() == "k_cam" and p.last_query_ms() > 0 and p.last_probe_project_ms() > 0
        finally:
            p.close()


# ---- 7, 8. the point of it
def test_a_uniform_sky_comes_back_as_its_colour():
    """no geometry, ground off, sky colour c, 4096 samples: irradiance / pi is within 6 x 1.283 c / sqrt(4096) of c for the six
    axis normals (the l = 1 and l = 2 estimators' variances, 4 pi c^2 / samples per coefficient, folded with A_l / pi and
    sum_m Y_lm(n)^2)"""
    c = np.array([0.5, 0.7, 1.0], f32)
    s = scenes.sky_only(sky=tuple(c))
    samples = 4096
    e = _engine(s)
    try:
        pos = np.array([(0, 0, 0), (3, -2, 5), (-40, 7, 0.5)], f32)
        sh = e.bake_probes(pos, samples)
        assert (sh["weight"] == samples).all()
        got = probes.irradiance(sh, AXES) / np.pi
        bound = 6.0 * 1.283 * c.astype(np.float64) / np.sqrt(samples)
        print("irradiance / pi:", got, "bound:", bound)
        assert (np.abs(got - c.astype(np.float64)) <= bound).all(), (got, bound)
        # every sample carries the sky: the ordered sum of c * Y0 from the model
        _, d, _ = probes.rays(pos, 0, samples)
        assert np.array_equal(words(sh), words(probes.project(d, np.tile(c, (len(d), 1)), samples)))
    finally:
        e.close()


def test_a_lamp_pulls_band_one_towards_it():
    """one emissive sphere at +x of the probe under a black sky: the band-1 vector (L3, L1, L2) of every channel has a positive
    dot product with +x, and L0 > 0"""
    u = scenes.make_uniforms(16, 16, 1, 4, cam_pos=(0, 0, 8), cam_dir=(0, 0, -1), ground_enabled=0, sky=(0, 0, 0))
    sp = np.zeros(1, dtype=abi.SPHERE)
    sp[0]["center"], sp[0]["radius"], sp[0]["material"] = (3.0, 0.0, 0.0), 1.0, scenes.material(diffuse=(0, 0, 0), emissive=(4.0, 3.0, 2.0))
    s = scenes._finish("lamp", u, sp, FAR_LIGHT.copy(), [])
    e = _engine(s)
    try:
        L = bake.probes(e, np.zeros((1, 3), f32), 1024)[0]
        print("L0:", L[0], "band 1 (x, y, z):", L[3], L[1], L[2])
        assert (L[0] > 0).all()
        assert ((np.stack([L[3], L[1], L[2]], axis=0) * np.array([1.0, 0.0, 0.0])[:, None]).sum(0) > 0).all()
        assert (np.abs(L[3]) > 3 * np.abs(L[1])).all() and (np.abs(L[3]) > 3 * np.abs(L[2])).all()   # and it points nowhere else
    finally:
        e.close()
