"""Camera rays made on the device (rb_camera_rays / rb_trace_camera / rb_trace_camera_device), bit for bit
on uint32 views:

  the generator = the numpy model renderbaby_amd/camera.py, for every kind, with and without jitter and a lens;
  the trace     = the ordered float32 sum of the unmodified oracle's rbo_trace_ray(scene, o, d, seed) over the very records
                  rb_camera_rays returned, no pixel left out, for every k_cam kernel;
  the forms, the pieces and the regions give the same answers, and a call has a query's side effects: none.
"""
import ctypes as C

import numpy as np
import pytest

from renderbaby_amd import Engine, RenderConfig, abi, bake, camera, engine, scenes
from tests import _oracle
from tests.conftest import has_gpu
from tests.test_camera_abi import INVALID_OPTIONS, NULL_ARGUMENT, REFUSALS
from tests.test_gpu_query import FAR_LIGHT, _copy, _engine, _identical_spheres
from tests.test_gpu_radiance import _mesh, _u32

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

f32 = np.float32
PIECE = abi.CAMERA_PIECE_ITEMS
POSE = dict(pos=(0.3, 1.5, 4.0), dir=(0.2, -0.3, -1.0), up=(0.1, 1.0, 0.0))
KINDS = {"pinhole": ("perspective", dict(fov_deg=50.0)), "lens": ("perspective", dict(fov_deg=50.0, aperture=0.5, focus_distance=3.0)),
         "ortho": ("ortho", dict(ortho_width=4.0)), "equirect": ("equirect", {})}


# ---- 1. the generator against the model
@pytest.mark.parametrize("jitter", [True, False], ids=["jitter", "centre"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_generator_equals_the_model(kind, jitter):
    k, kw = KINDS[kind]
    for w, h in ((1, 1), (63, 1), (65, 3), (7, 5)):
        cam = camera.make(k, w, h, jitter=jitter, **POSE, **kw)
        regions = [(0, w * h)] + ([(70, 60), (127, 2), (64, 64)] if w * h > 130 else [])   # 70 .. 129: starts and ends inside a block of 64
        for first, n in regions:
            for samples, first_sample in ((1, 0), (2, 7), (5, 0), (5, 7)):
                rays, seeds = engine.camera_rays_device(cam, samples, first_sample, region=(first, n), device=0)
                o, d, s = camera.rays(cam, np.arange(first, first + n), first_sample, samples)
                where = (kind, jitter, w, h, first, n, samples, first_sample)
                assert rays.shape == (n * samples,) and seeds.shape == (n * samples,), where
                assert np.array_equal(seeds, s), where
                assert np.array_equal(_u32(rays["origin"]), _u32(o)), where
                bad = np.nonzero((_u32(rays["dir"]) != _u32(d)).any(1))[0]
                assert len(bad) == 0, (where, bad[:5], rays["dir"][bad[:5]], d[bad[:5]])
                assert (_u32(rays["_pad0"]) == 0).all() and (_u32(rays["_pad1"]) == 0).all(), where
                assert (d != 0).any(1).all(), where   # (these cameras have no invalid ray)


def test_generator_marks_invalid_rays_as_the_model_does():
    """pos with an Inf: every origin is non-finite, every direction 0 0 0, for each kind; an ortho window so far from the
    origin that only a part of its origins overflows"""
    for k, kw in KINDS.values():
        cam = camera.make(k, 7, 5, **dict(POSE, pos=(np.inf, 1.0, 2.0)), **kw)
        rays, seeds = engine.camera_rays_device(cam, 2, device=0)
        o, d, s = camera.rays(cam, np.arange(35), 0, 2)
        assert np.array_equal(_u32(rays["origin"]), _u32(o)) and np.array_equal(seeds, s)
        assert (rays["dir"] == 0).all() and (d == 0).all()
    cam = camera.make("ortho", 7, 5, pos=(3.3e38, 0, 0), dir=(0, 0, -1), ortho_width=1e38)
    rays, _ = engine.camera_rays_device(cam, 2, device=0)
    o, d, _ = camera.rays(cam, np.arange(35), 0, 2)
    assert np.array_equal(_u32(rays["origin"]), _u32(o)) and np.array_equal(_u32(rays["dir"]), _u32(d))
    gone = (rays["dir"] == 0).all(1)
    assert 0 < gone.sum() < len(gone) and np.array_equal(gone, ~np.isfinite(o).all(1))


# ---- 2. the trace against the oracle on the generated rays
def oracle_sums(scene, rays, seeds, samples, counts_kept=0):
    """abi.RADIANCE[n] from the records of rb_camera_rays: rbo_trace_ray per valid record, summed in sample order from +0"""
    os_, L = _oracle.OracleScene(scene, 1, counts_kept), _oracle.lib()
    n = len(rays) // samples
    out = np.zeros(n, dtype=abi.RADIANCE)
    rgb, st = np.zeros(3, f32), _oracle.Stats()
    walked = int(scene.uniforms["max_depth"][0]) > 0
    for i in range(n):
        acc, w = np.zeros(3, f32), f32(0)
        for k in range(samples):
            r = rays[i * samples + k]
            if not (r["dir"] != 0).any():
                continue
            w = f32(w + f32(1))
            if walked:
                o, d = np.ascontiguousarray(r["origin"]), np.ascontiguousarray(r["dir"])
                L.rbo_trace_ray(C.byref(os_.c), o.ctypes.data, d.ctypes.data, int(seeds[i * samples + k]), rgb.ctypes.data, C.byref(st))
                assert np.isfinite(rgb).all(), (i, k, rgb)
                acc = (acc + rgb).astype(f32)
        out[i]["sum"], out[i]["weight"] = acc, w
    return out


def scene_camera(scene, w, h, **kw):
    """a thin-lens camera where the scene's own camera stands: the number of lens draws differs from item to item"""
    c = scene.uniforms["camera"][0]
    args = dict(fov_deg=50.0, aperture=0.3, focus_distance=4.0)
    args.update(kw)
    return camera.make("perspective", w, h, c["pos"], dir=c["dir"], **args)


def check_trace(scene, kernel, sizes=((65, 3), (7, 5)), e=None, **kw):
    own = e is None
    e = _engine(scene, **kw) if own else e
    try:
        st0, lit = e.stats(), 0
        for (w, h), (samples, first_sample) in zip(sizes, ((5, 7), (1, 0))):
            cam = scene_camera(scene, w, h)
            got = e.trace_camera(cam, samples, first_sample)
            assert e.last_query_kernel_name() == kernel, e.last_query_kernel_name()
            assert e.last_query_ms() > 0
            rays, seeds = engine.camera_rays_device(cam, samples, first_sample, device=0)
            want = oracle_sums(scene, rays, seeds, samples)
            bad = np.nonzero((_u32(got).reshape(-1, 4) != _u32(want).reshape(-1, 4)).any(1))[0]
            assert len(bad) == 0, (scene.name, kernel, w, h, samples, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
            assert (got["weight"] == samples).all()
            lit += int((want["sum"] != 0).any(1).sum())
        assert lit > 0, "no pixel of the scene carried any light"
        assert e.stats() == st0, "camera queries moved rb_get_stats"
    finally:
        if own:
            e.close()


@pytest.mark.parametrize("color_hash", [0, 1])
def test_feature_scene(color_hash):
    check_trace(scenes.feature_scene(width=24, height=16, color_hash=color_hash), "k_cam")


@pytest.mark.parametrize("kw,kernel", [(dict(), "k_cam_chunk"), (dict(reference_walk=True), "k_cam_bvh")])
def test_multi_node_mesh(kw, kernel):
    s = _mesh()
    assert len(s.bvh_triangles) == 578
    check_trace(s, kernel, **kw)


def test_identical_spheres():
    check_trace(_identical_spheres().with_params(width=24, height=24), "k_cam_bvh")


def test_mesh_beside_a_sphere_tree():
    m = _mesh()
    b = scenes.spheres_scene(n=150, width=32, height=20, spp=1, max_depth=4, extent=5.0)
    sp = b.spheres.copy()
    sp["center"][:, 1] += f32(1.0)
    s = _copy(m, spheres=sp)
    s.uniforms["spheres_count"] = len(sp)
    check_trace(s, "k_cam_chunk")


def test_other_kinds_through_the_trace():
    """ortho and equirect (jittered) and the pinhole without jitter through k_cam, against the oracle on their records"""
    s = scenes.feature_scene(width=24, height=16)
    c = s.uniforms["camera"][0]
    e = _engine(s)
    try:
        for k, kw in (("ortho", dict(ortho_width=6.0)), ("equirect", {}), ("perspective", dict(jitter=False))):
            cam = camera.make(k, 33, 5, c["pos"], dir=c["dir"], **kw)
            got = e.trace_camera(cam, 3, 7)
            rays, seeds = engine.camera_rays_device(cam, 3, 7, device=0)
            assert np.array_equal(_u32(got), _u32(oracle_sums(s, rays, seeds, 3))), k
            assert (got["sum"] != 0).any(1).sum() > 20
    finally:
        e.close()


def test_a_camera_whose_rays_are_not_finite_weighs_nothing():
    s = scenes.feature_scene(width=24, height=16)
    e = _engine(s)
    try:
        cam = camera.make("equirect", 65, 3, (0.0, np.inf, 0.0))
        got = e.trace_camera(cam, 5)
        assert (_u32(got) == 0).all()   # {+0, +0, +0, +0}
        # some of an ortho camera's origins overflow: those samples weigh 0, the pixel's other samples count
        cam = camera.make("ortho", 7, 5, pos=(3.3e38, 0, 0), dir=(0, 0, -1), ortho_width=1e38)
        got = e.trace_camera(cam, 5)
        rays, seeds = engine.camera_rays_device(cam, 5, device=0)
        want = oracle_sums(s, rays, seeds, 5)
        assert np.array_equal(_u32(got), _u32(want))
        assert len(set(want["weight"].tolist())) > 2 and want["weight"].min() == 0 and want["weight"].max() == 5
    finally:
        e.close()


def test_depth_zero_and_one():
    s = scenes.feature_scene(width=24, height=16)
    for depth in (0, 1):
        sd = s.with_params(max_depth=depth)
        e = _engine(sd)
        try:
            cam = scene_camera(sd, 65, 3)
            got = e.trace_camera(cam, 3)
            rays, seeds = engine.camera_rays_device(cam, 3, device=0)
            assert np.array_equal(_u32(got), _u32(oracle_sums(sd, rays, seeds, 3)))
            assert (got["weight"] == 3).all()
            if depth == 0:
                assert (_u32(got["sum"]) == 0).all()
            else:
                assert (got["sum"] != 0).any(1).sum() > 20   # the winner's emission, the sky for a miss
            bad = camera.make("equirect", 7, 5, (np.nan, 0.0, 0.0))
            assert (_u32(e.trace_camera(bad, 3)) == 0).all()   # invalid at any depth: weight 0
        finally:
            e.close()


# ---- 3. forms, regions, pieces
def test_device_form_and_regions_equal_the_whole_host_call():
    import torch
    s = _mesh()
    cam = scene_camera(s, 65, 3)
    e = _engine(s)
    try:
        whole = e.trace_camera(cam, 5, 7)
        out = torch.full((195, 4), -1.0, dtype=torch.float32, device="cuda")
        assert e.trace_camera(cam, 5, 7, out=out) is out
        assert e.last_query_kernel_name() == "k_cam_chunk" and e.last_query_ms() > 0
        assert np.array_equal(_u32(out.cpu().numpy()), _u32(whole).reshape(-1, 4))
        for first, n in ((0, 1), (70, 60), (64, 64), (194, 1), (1, 194), (195, 0), (0, 0)):
            part = e.trace_camera(cam, 5, 7, region=(first, n))
            assert np.array_equal(_u32(part), _u32(whole[first:first + n])), (first, n)
            dpart = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
            e.trace_camera(cam, 5, 7, region=(first, n), out=dpart)
            assert np.array_equal(_u32(dpart.cpu().numpy()), _u32(whole[first:first + n]).reshape(-1, 4)), (first, n)
        filled = np.zeros(60, dtype=abi.RADIANCE)
        assert e.trace_camera(cam, 5, 7, region=(70, 60), out=filled) is filled and np.array_equal(_u32(filled), _u32(whole[70:130]))
        # first_sample continues the stream: samples 7 .. 11 are samples 7 .. 8 and then 9 .. 11, up to the order of the adds
        a, b = e.trace_camera(cam, 2, 7), e.trace_camera(cam, 3, 9)
        assert np.allclose(a["sum"] + b["sum"], whole["sum"], rtol=1e-5, atol=1e-6) and not np.array_equal(a["sum"], b["sum"])
        # the launch shape: reservations of 64 items on a grid of one block per CU
        o = _engine(s, queue_batch=64, blocks_per_cu=1)
        try:
            assert np.array_equal(_u32(o.trace_camera(cam, 5, 7)), _u32(whole))
        finally:
            o.close()
        for bad in (dict(out=np.zeros(195, f32)), dict(out=out[:5]), dict(out=out[:, :3]), dict(region=(-1, 4)), dict(samples=-1)):
            with pytest.raises(ValueError):
                e.trace_camera(cam, **dict(dict(samples=1), **bad))
    finally:
        e.close()


def test_a_call_across_a_piece_boundary():
    """RB_CAMERA_PIECE_ITEMS + 77 * samples items on the Cornell scene at max_depth = 2: two pieces.  Every pixel against two
    calls split at the piece boundary; the last 77 pixels and the 64 around the boundary against the oracle; every pixel against
    the device form's answer, whose two pieces go through the same loop on the caller's buffer."""
    import torch
    samples = 4
    b = PIECE // samples
    n = b + 77
    s = scenes.cornell(32, 32, 1, 2)
    cam = scene_camera(s, 2048, 1025, focus_distance=30.0)
    assert n * samples == PIECE + 77 * samples and n <= 2048 * 1025
    e = _engine(s)
    try:
        one = e.trace_camera(cam, samples, 7, region=(0, n))
        assert e.last_query_kernel_name() == "k_cam" and e.last_query_ms() > 0
        two = np.concatenate([e.trace_camera(cam, samples, 7, region=(0, b)), e.trace_camera(cam, samples, 7, region=(b, 77))])
        assert np.array_equal(_u32(one), _u32(two))
        assert (one["weight"] == samples).all() and (one["sum"] != 0).any(1).sum() > 1000
        rays, seeds = engine.camera_rays_device(cam, samples, 7, region=(b - 32, 32 + 77), device=0)
        want = oracle_sums(s, rays, seeds, samples)
        assert np.array_equal(_u32(one[b - 32:]), _u32(want))
        dev = e.trace_camera(cam, samples, 7, region=(0, n), out=torch.empty((n, 4), dtype=torch.float32, device=f"cuda:{e.query_device}"))
        assert e.last_camera_rays_ms() > 0   # both pieces' event pairs were recorded and are read
        assert np.array_equal(_u32(dev.cpu().numpy()), _u32(one).reshape(n, 4))
    finally:
        e.close()


# ---- 4. side effects and refusals
def test_a_camera_query_between_iterator_frames():
    s = scenes.feature_scene(width=48, height=32, spp=4)
    rc = RenderConfig.from_scene(s)
    cam = scene_camera(s, 65, 3)

    def frames(query):
        e = Engine.new(rc, device=0)
        it = e.frame_iterator(rc)
        out, answers = [], []
        while it.has_next():
            out.append(it.next().pixels.copy())
            if query:
                kernel = e.last_kernel_name()
                answers.append(e.trace_camera(cam, 3))
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
    for a in answers[1:]:
        assert np.array_equal(_u32(a), _u32(answers[0]))


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
        base = np.ascontiguousarray(camera.make("perspective", 8, 4, (0, 1, 3), aperture=0.2, focus_distance=2.0)).reshape(1)
        out = np.full(64, 7, dtype=abi.RADIANCE)
        d_out = torch.full((64, 4), 7.0, dtype=torch.float32, device="cuda")
        before = e.trace_camera(base[0], 2)
        for fn, o in ((lib.rb_trace_camera, out.ctypes.data), (lib.rb_trace_camera_device, d_out.data_ptr())):
            for name, make in REFUSALS:
                cam, kw = make(base)
                args = dict(first_pixel=0, n=4, first_sample=0, samples=2)
                args.update(kw)
                assert fn(h, cam.ctypes.data, args["first_pixel"], args["n"], args["first_sample"], args["samples"], o) == INVALID_OPTIONS, name
                assert lib.rb_last_error(h)
            assert fn(h, None, 0, 4, 0, 2, o) == NULL_ARGUMENT and fn(h, base.ctypes.data, 0, 4, 0, 2, None) == NULL_ARGUMENT
            assert fn(h, None, 0, 0, 0, 2, None) == 0 and fn(h, base.ctypes.data, 32, 0, 0, 2, None) == 0   # n_pixels == 0
        lib.rb_sync(h)
        assert (out["weight"] == 7).all() and (d_out == 7).all().item()
        dev, cp = lib.rb_trace_camera_device, base.ctypes.data
        assert dev(h, cp, 0, 4, 0, 2, out.ctypes.data) == INVALID_OPTIONS            # a host pointer
        assert dev(h, cp, 0, 4, 0, 2, d_out.data_ptr() + 4) == INVALID_OPTIONS       # misaligned
        big = np.ascontiguousarray(camera.make("perspective", 4096, 4096, (0, 1, 3))).reshape(1)
        assert dev(h, big.ctypes.data, 0, 1 << 24, 0, 1, d_out.data_ptr()) == INVALID_OPTIONS   # the allocation ends before n pixels
        assert dev(h, cp, 0, 32, 0, 2, d_out.data_ptr()) == 0 and lib.rb_sync(h) == 0
        assert np.array_equal(_u32(d_out.cpu().numpy()[:32]), _u32(before).reshape(-1, 4)) and (d_out[32:] == 7).all().item()
        assert np.array_equal(_u32(e.trace_camera(base[0], 2)), _u32(before))
        assert np.array_equal(e.render(rc).pixels, _oracle.render(s)[2])
    finally:
        e.close()
    cold = Engine.new(rc, device=0)   # no update yet: not ready, and still a refusal first
    try:
        assert lib.rb_trace_camera(cold._h, base.ctypes.data, 0, 4, 0, 2, out.ctypes.data) not in (0, INVALID_OPTIONS)
        assert lib.rb_trace_camera(cold._h, base.ctypes.data, 0, 4, 0, 0, out.ctypes.data) == INVALID_OPTIONS
        assert np.array_equal(cold.render(rc).pixels, _oracle.render(s)[2])
    finally:
        cold.close()


def test_sharded_engine_and_multi_device_handle():
    """both forms on a sharded engine (the camera sees the whole scene) and on a multi-device handle on one device"""
    import torch
    s = scenes.feature_scene(width=24, height=16)
    cam = scene_camera(s, 65, 3)
    e = _engine(s)
    want = e.trace_camera(cam, 2, 7)
    e.close()
    for kw in (dict(shard_rank=1, shard_count=3, stripe_rows=8), dict(devices=[0, 0], gather_peer_copy=True)):
        p = _engine(s, **kw)
        try:
            assert np.array_equal(_u32(p.trace_camera(cam, 2, 7)), _u32(want)), kw
            dev = p.trace_camera(cam, 2, 7, out=torch.zeros((195, 4), dtype=torch.float32, device="cuda"))
            assert np.array_equal(_u32(dev.cpu().numpy()), _u32(want).reshape(-1, 4)), kw
            assert p.last_query_kernel_name() == "k_cam" and p.last_query_ms() > 0
        finally:
            p.close()


# ---- 5. the point of it
def test_a_thin_lens_blurs_what_is_off_its_focal_plane():
    """A thin-lens camera above the checkerboard ground, looking down at it, focused on the ground point of the image's centre
    (the distance ALONG FORWARD of the centre column's middle hits, from rb_cast_rays).  The 64 samples of a pixel are 64
    rays from 64 lens points; for the centre pixel, on the focal plane, they meet on the ground within a pixel's footprint; for
    pixels of the centre column near the top and the bottom of the image, off the plane, they land many footprints apart.
    bake.camera_rays has one lens point per pixel and cannot show either."""
    u = scenes.make_uniforms(16, 16, 1, 4, cam_pos=(0, 3, 5), cam_dir=(0, -0.5, -1), ground_enabled=1, ground_height=0.0,
                             checkerboard_enabled=1, sky=(0.5, 0.7, 1.0))
    s = scenes._finish("ground", u, np.zeros(0, dtype=abi.SPHERE), FAR_LIGHT.copy(), [])
    w = h = 65
    pose = dict(pos=(0.0, 3.0, 5.0), dir=(0.0, -0.5, -1.0), fov_deg=40.0)
    e = _engine(s)
    try:
        pin = camera.make("perspective", w, h, jitter=False, **pose)
        o, d, _ = camera.rays(pin, np.arange(w * h), 0, 1)
        hits = e.cast_rays(o, d)
        assert (hits["kind"] == abi.HIT_GROUND).all()
        ground = (o + hits["t"][:, None] * d).reshape(h, w, 3)            # the pinhole image's ground points
        depth = (hits["t"] * (d @ pin["forward"])).reshape(h, w)          # their distance along forward
        mid, col = h // 2, w // 2
        focus = float(depth[mid - 1:mid + 2, col].mean())                 # the focal plane through the centre pixel's ground point
        foot = lambda r: float(max(np.linalg.norm(ground[r, col] - ground[r + dr, col + dc]) for dr in (-1, 1) for dc in (-1, 1)))
        lens = camera.make("perspective", w, h, jitter=False, aperture=1.0, focus_distance=focus, **pose)

        def spread(row):
            rays, seeds = engine.camera_rays_device(lens, 64, region=(row * w + col, 1), device=0)
            assert len(np.unique(_u32(rays["origin"]), axis=0)) == 64 and len(np.unique(seeds)) == 64   # 64 lens points
            hit = e.cast_ray_records(rays)
            assert (hit["kind"] == abi.HIT_GROUND).all()
            pts = rays["origin"] + hit["t"][:, None] * rays["dir"]
            return float(np.linalg.norm(pts - ground[row, col], axis=1).max())
        on, top, bottom = spread(mid), spread(2), spread(h - 3)
        print(f"focus {focus:.3f}; spread / footprint: centre {on / foot(mid):.4f}, top {top / foot(2):.2f}, bottom {bottom / foot(h - 3):.2f}")
        assert on <= foot(mid)
        assert top > foot(2) and bottom > foot(h - 3)
        # and the image: bake.render_camera is Engine.trace_camera through bake.tone_map
        img = bake.render_camera(e, lens, 64)
        assert img.shape == (h, w, 4) and img.dtype == np.uint8 and (img[..., 3] == 255).all()
        assert np.array_equal(img, bake.tone_map(e.trace_camera(lens, 64).reshape(h, w)))
        assert len(np.unique(img[..., :3].reshape(-1, 3), axis=0)) > 20
    finally:
        e.close()
