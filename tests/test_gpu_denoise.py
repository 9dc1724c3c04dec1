"""The edge-avoiding a-trous denoiser on the device (rb_denoise*) against its numpy model
(renderbaby_amd/denoise.py).  Every comparison with the model is exact: the bits of the linear vec4 and the bytes of the RGBA8.
"""
import ctypes as C

import numpy as np
import pytest

from renderbaby_amd import Change, Engine, RenderConfig, RenderError, abi, denoise, engine, scenes
from tests.conftest import has_gpu
from tests.test_gpu_query import _copy, _engine

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

f32 = np.float32
INVALID_OPTIONS, NULL_ARGUMENT, NOT_INITIALIZED = 18, 15, 17


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def synthetic(h, w, seed, islands=True, non_finite=True):
    """colour and guides of a made-up frame: three surfaces (every filterable class) meeting at edges, normals that vary
    within a surface, positions on tilted planes, textured albedo (some of it below the floor), class 0 islands and non-finite
    pixels in both kinds of place"""
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[0:h, 0:w]
    g = np.zeros((h, w), dtype=abi.GUIDE)
    region = ((xx * 3) // max(w, 1) + (yy * 2) // max(h, 1)) % 3
    g["cls"] = np.array([abi.HIT_GROUND, abi.HIT_TRIANGLE, abi.HIT_SPHERE], np.uint32)[region]
    base = np.array([[0, 1, 0], [0, 0, 1], [0.6, 0, 0.8]], f32)[region]
    n = base + rng.normal(0, 0.05, (h, w, 3)).astype(f32)
    g["normal"] = (n / np.sqrt((n * n).sum(-1, keepdims=True), dtype=f32)).astype(f32)
    g["t"] = (f32(4.0) + f32(0.01) * xx + f32(0.02) * yy + region).astype(f32)
    g["pos"] = np.stack([f32(0.02) * xx, f32(0.03) * region + f32(0.0005) * rng.random((h, w)), f32(-0.02) * yy], -1).astype(f32)
    g["albedo"] = (rng.random((h, w, 3)) ** 3).astype(f32)   # (a good share below the default floor of 0.01)
    signal = np.array([[0.9, 0.5, 0.2], [0.1, 0.4, 0.8], [2.5, 2.0, 0.3]], f32)[region]
    c = (signal * g["albedo"] + rng.gamma(0.5, 0.4, (h, w, 3))).astype(f32)
    if islands and h * w >= 12:
        isl = rng.random((h, w)) < 0.06
        g["cls"][isl] = 0
        g["cls"][h // 2, w // 3:w // 3 + 3] = 0
    if non_finite and h * w >= 12:
        k = max(1, h * w // 40)
        py, px = rng.integers(0, h, k), rng.integers(0, w, k)
        c[py, px, rng.integers(0, 3, k)] = np.array([np.nan, np.inf, -np.inf], f32)[rng.integers(0, 3, k)]
    return c, g


def check_core(h, w, seed, **kw):
    c, g = synthetic(h, w, seed)
    p = denoise.params(**kw)
    want_lin, want_img = denoise.filter(c, g, p, rgba=True)
    lin, img = engine.denoise_buffers(c, g, p, device=0)
    bad = np.nonzero((bits(lin) != bits(want_lin)).any(-1))
    assert len(bad[0]) == 0, (h, w, kw, len(bad[0]), bad[0][:4], bad[1][:4], lin[bad][:4], want_lin[bad][:4])
    assert np.array_equal(img, want_img), (h, w, kw)
    return lin, c, g


# ---- 1. the core against the model
@pytest.mark.parametrize("h,w", [(1, 1), (1, 37), (41, 1), (5, 3), (33, 67), (70, 130)])
@pytest.mark.parametrize("iterations", [0, 1, 5, 8])
@pytest.mark.parametrize("sigma_color", [0.0, 2.0])
def test_core_equals_the_model_at_every_size(h, w, iterations, sigma_color):
    """sizes that are no multiple of any tile (64 x 4, 16 x 16), down to one pixel; with 8 iterations the last steps (64, 128)
    are beyond the width of every frame here; the colour term off and on"""
    lin, c, g = check_core(h, w, 100 + h * w, iterations=iterations, sigma_color=sigma_color)
    passed = (g["cls"] == 0) | ~np.isfinite(c).all(-1)
    assert np.array_equal(bits(lin[..., :3])[passed], bits(c)[passed])   # class 0 and non-finite pixels: bit-identical


@pytest.mark.parametrize("kw", [dict(sigma_color=4.0), dict(sigma_color=-1.0), dict(sigma_color=0.3), dict(normal_power_log2=0),
                                dict(normal_power_log2=10), dict(sigma_depth=0.5), dict(sigma_depth=1e-4), dict(albedo_floor=0.25),
                                dict(iterations=6, sigma_color=1.0)])
def test_core_equals_the_model_for_each_parameter(kw):
    check_core(45, 83, 7, **kw)


@pytest.mark.parametrize("variant", ["plain", "lds"])
def test_both_iteration_kernels_equal_the_model(variant, monkeypatch):
    """the LDS-staged kernel of steps 1 and 2 and the plain one compute the same bits (RB_DENOISE_VARIANT is the measurement
    switch of tools/denoise_rate.py)"""
    monkeypatch.setenv("RB_DENOISE_VARIANT", variant)
    for h, w in ((1, 1), (19, 50), (64, 64), (35, 17)):
        check_core(h, w, 31 + h, iterations=3)
        check_core(h, w, 77 + h, iterations=2, sigma_color=1.5)


def test_core_refuses_bad_parameters():
    c, g = synthetic(4, 4, 1)
    for kw in (dict(iterations=9), dict(normal_power_log2=11), dict(sigma_depth=0.0), dict(sigma_depth=np.nan), dict(sigma_color=np.inf),
               dict(albedo_floor=0.0), dict(albedo_floor=-np.inf), dict(flags=1), dict(_reserved=(0, 1))):
        p = denoise.default_params()
        for k, v in kw.items():
            p[k] = v
        with pytest.raises(RenderError) as ei:
            engine.denoise_buffers(c, g, p, device=0)
        assert ei.value.code == INVALID_OPTIONS, kw


# ---- 2. the engine path
def mesh_small():
    return scenes.mesh_scene(24, 24, 96, 64, 4, 4, seed=3)


def many_spheres():
    return scenes.spheres_scene(n=300, width=80, height=60, spp=4, max_depth=4, extent=10.0)


ENGINE_CASES = [("cornell", lambda: scenes.cornell(96, 72, 4, 4), dict()),
                ("feature", lambda: scenes.feature_scene(width=96, height=64, spp=4), dict()),
                ("mesh-chunk", mesh_small, dict()),
                ("mesh-reference", mesh_small, dict(reference_walk=True)),
                ("spheres", many_spheres, dict())]


def engine_frames(make, kw, p):
    """(model linear, model rgba, engine linear, engine rgba, device linear, device rgba, guides) of one rendered scene"""
    import torch
    s = make()
    rc = RenderConfig.from_scene(s)
    e = Engine.new(rc, device=0, **kw)
    try:
        frame = e.render(rc)
        acc = e.read_accumulation()
        g = e.denoise_guides()
        img = e.denoise(p)
        lin = e.denoise(p, linear=True)
        d_img = torch.empty((s.height, s.width, 4), dtype=torch.uint8, device="cuda:0")
        d_lin = torch.empty((s.height, s.width, 4), dtype=torch.float32, device="cuda:0")
        assert e.denoise(p, out=d_img) is d_img and e.denoise(p, linear=True, out=d_lin) is d_lin
        want_lin, want_img = denoise.filter(denoise.mean_radiance(acc), g, p, rgba=True)
        return want_lin, want_img, lin, img, d_lin.cpu().numpy(), d_img.cpu().numpy(), g, frame, s
    finally:
        e.close()


@pytest.mark.parametrize("name,make,kw", ENGINE_CASES, ids=[c[0] for c in ENGINE_CASES])
def test_engine_denoise_equals_the_model(name, make, kw):
    for p in (denoise.default_params(), denoise.params(iterations=5, sigma_color=4.0, normal_power_log2=5)):
        want_lin, want_img, lin, img, d_lin, d_img, g, _, _ = engine_frames(make, kw, p)
        assert (g["cls"] != 0).mean() > 0.3, "the scene must have something to filter"
        assert np.array_equal(bits(lin), bits(want_lin)), name
        assert np.array_equal(img, want_img), name
        assert np.array_equal(bits(d_lin), bits(lin)) and np.array_equal(d_img, img), "host and device forms differ"


def test_every_walk_gives_the_same_frame():
    p = denoise.default_params()
    a = engine_frames(mesh_small, dict(), p)
    b = engine_frames(mesh_small, dict(reference_walk=True), p)
    assert np.array_equal(bits(a[2]), bits(b[2])) and np.array_equal(a[3], b[3])
    assert np.array_equal(a[6].view(np.uint32), b[6].view(np.uint32)), "the guides differ between the walks"


@pytest.mark.parametrize("name,make,kw", ENGINE_CASES, ids=[c[0] for c in ENGINE_CASES])
def test_guides_against_the_records(name, make, kw):
    s = make()
    e = _engine(s, **kw)
    try:
        hits, surf = e.render_hits(surfaces=True)
        g = e.denoise_guides()
    finally:
        e.close()
    assert np.array_equal(bits(g["normal"]), bits(hits["normal"])) and np.array_equal(bits(g["t"]), bits(hits["t"]))
    assert np.array_equal(bits(g["albedo"]), bits(surf["albedo"]))
    k = hits["kind"]
    filterable = np.isin(k, (abi.HIT_GROUND, abi.HIT_TRIANGLE, abi.HIT_SPHERE)) & ~(surf["emissive"] > 0).any(-1)
    assert np.array_equal(g["cls"], np.where(filterable, k, 0))
    hit = (k != abi.HIT_NONE) & (k != abi.HIT_INVALID)
    assert hit.mean() > 0.3
    cam = np.asarray(s.uniforms["camera"]["pos"], np.float64).reshape(3)
    dist = np.sqrt(((g["pos"][hit].astype(np.float64) - cam) ** 2).sum(-1))
    t = hits["t"][hit].astype(np.float64)
    err = np.abs(dist - t) / t
    print(f"{name}: | |pos - camera| - t | / t at most {err.max():.3g}")
    assert (err <= 1e-5).all()
    # the public restatement agrees with the engine's buffer: exactly in everything but pos, there to rounding
    m = denoise.guides_from_records(s.uniforms, hits, surf)
    for f in ("normal", "t", "albedo", "cls"):
        assert np.array_equal(bits(m[f]), bits(g[f])), f
    assert (np.abs(m["pos"][hit].astype(np.float64) - g["pos"][hit]).max(-1) <= 1e-5 * t).all()


def test_zero_iterations_is_the_renders_own_frame():
    for make, kw in ((lambda: scenes.cornell(64, 48, 4, 4), dict()), (mesh_small, dict())):
        s = make()
        rc = RenderConfig.from_scene(s)
        e = Engine.new(rc, device=0, **kw)
        try:
            e.update(rc)
            frame = e.render_current().pixels
            assert np.array_equal(e.denoise(denoise.params(iterations=0)), frame)
            lin = e.denoise(denoise.params(iterations=0), linear=True)
            assert np.array_equal(bits(lin[..., :3]), bits(denoise.mean_radiance(e.read_accumulation())))
        finally:
            e.close()


# ---- 3. the contract
def test_a_denoise_leaves_the_render_alone():
    s = scenes.feature_scene(width=64, height=48, spp=4)
    rc = RenderConfig.from_scene(s)
    e = Engine.new(rc, device=0)
    try:
        frame = e.render(rc).pixels.copy()
        acc, st, kernel = e.read_accumulation(), e.stats(), e.last_kernel_name()
        e.denoise()
        e.denoise(linear=True)
        e.denoise_guides()
        assert e.stats() == st and e.last_kernel_name() == kernel
        assert np.array_equal(bits(e.read_accumulation()), bits(acc)) and np.array_equal(e.read_rgba(), frame)
        assert np.array_equal(e.render_current().pixels, frame), "the engine renders afterwards, and the same"
    finally:
        e.close()


def test_a_denoise_between_iterator_frames_keeps_the_pass_run_ahead():
    s = scenes.feature_scene(width=48, height=32, spp=4)
    rc = RenderConfig.from_scene(s)

    def frames(ask):
        e = Engine.new(rc, device=0)
        it = e.frame_iterator(rc)
        out, filtered = [], []
        while it.has_next():
            out.append(it.next().pixels.copy())
            if ask:
                kernel = e.last_kernel_name()
                filtered.append(e.denoise(linear=True))
                want = denoise.filter(denoise.mean_radiance(e.read_accumulation()), e.denoise_guides())
                assert np.array_equal(bits(filtered[-1]), bits(want)), "the filter read another accumulation than the committed one"
                assert e.last_kernel_name() == kernel
        st = e.stats()
        e.close()
        return out, st
    plain, st0 = frames(False)
    asked, st1 = frames(True)
    assert len(plain) == len(asked) == 4
    for a, b in zip(plain, asked):
        assert np.array_equal(a, b)
    for k in ("segments", "paths", "launches"):   # the run-ahead pass was kept, not traced again; a denoise counts nothing
        assert st0[k] == st1[k], k


def test_guides_follow_accepted_updates_only():
    s = scenes.feature_scene(width=48, height=32, spp=2)
    rc = RenderConfig.from_scene(s)
    e = Engine.new(rc, device=0)
    try:
        e.render(rc)
        g0 = e.denoise_guides()
        before = e.denoise(linear=True)
        bad = s.bvh_nodes.copy()
        bad["left"][0] = 0   # a cycle: refused by validation
        bad["right"][0] = 0
        bad["primitive_count"][0] = 0
        with pytest.raises(RenderError):
            e.update(RenderConfig(bvh_nodes=Change.create(bad)))
        assert np.array_equal(e.denoise_guides().view(np.uint32), g0.view(np.uint32)), "a refused update touched the guides"
        assert np.array_equal(bits(e.denoise(linear=True)), bits(before))
        assert e.last_denoise_ms()[1] == 0.0, "the guides were built again after a refused update"
        moved = _copy(s)
        moved.uniforms["camera"]["pos"][0][0] += f32(0.75)
        e.update(RenderConfig(uniforms=Change.update(moved.uniforms)))
        g1 = e.denoise_guides()
        assert not np.array_equal(g1["pos"], g0["pos"])
        fresh = _engine(moved)
        try:
            assert np.array_equal(fresh.denoise_guides().view(np.uint32), g1.view(np.uint32))
        finally:
            fresh.close()
    finally:
        e.close()


def _code(fn):
    with pytest.raises(RenderError) as ei:
        fn()
    return ei.value.code


def test_refusals():
    import torch
    s = scenes.feature_scene(width=32, height=24, spp=1)
    rc = RenderConfig.from_scene(s)
    sharded = Engine.new(rc, device=0, shard_rank=0, shard_count=2)
    multi = Engine.new(rc, devices=[0, 0], gather_peer_copy=True)
    cold = Engine.new(rc, device=0)
    e = Engine.new(rc, device=0)
    try:
        sharded.render(rc)
        multi.render(rc)
        for x in (sharded, multi):
            assert _code(x.denoise) == INVALID_OPTIONS
            assert _code(x.denoise_guides) == INVALID_OPTIONS
        buf = np.empty((24, 32, 4), np.uint8)
        p0 = np.ascontiguousarray(denoise.default_params()).reshape(1)
        assert cold._lib.rb_denoise(cold._h, p0.ctypes.data, buf.ctypes.data, None) == NOT_INITIALIZED
        assert cold._lib.rb_render(cold._h, buf.ctypes.data) == NOT_INITIALIZED   # what a render before the first update gives
        frame = e.render(rc).pixels.copy()
        for kw in (dict(iterations=9), dict(normal_power_log2=11), dict(sigma_depth=-1.0), dict(sigma_color=np.nan), dict(albedo_floor=0.0),
                   dict(flags=2)):
            assert _code(lambda: e.denoise(denoise.params(**kw))) == INVALID_OPTIONS, kw
        p = np.ascontiguousarray(denoise.default_params()).reshape(1)
        lib, h = e._lib, e._h
        host = np.empty((24, 32, 4), np.uint8)
        assert lib.rb_denoise_device(h, p.ctypes.data, host.ctypes.data, None) == INVALID_OPTIONS   # a host pointer
        assert lib.rb_denoise_device(h, p.ctypes.data, None, host.ctypes.data) == INVALID_OPTIONS
        d_lin = torch.empty(24 * 32 * 4 + 4, dtype=torch.float32, device="cuda:0")
        assert lib.rb_denoise_device(h, p.ctypes.data, None, d_lin.data_ptr() + 4) == INVALID_OPTIONS   # not 16-byte aligned
        assert lib.rb_denoise_device(h, p.ctypes.data, None, d_lin.data_ptr()) == 0 and lib.rb_sync(h) == 0
        assert np.array_equal(bits(d_lin[:24 * 32 * 4].cpu().numpy().reshape(24, 32, 4)), bits(e.denoise(linear=True)))
        assert lib.rb_denoise(h, p.ctypes.data, None, None) == NULL_ARGUMENT
        assert lib.rb_denoise_device(h, p.ctypes.data, None, None) == NULL_ARGUMENT
        assert lib.rb_denoise(h, None, host.ctypes.data, None) == NULL_ARGUMENT
        assert lib.rb_denoise_guides(h, None) == NULL_ARGUMENT
        # the engine denoises and renders afterwards
        assert e.denoise().shape == (24, 32, 4)
        assert np.array_equal(e.render_current().pixels, frame)
    finally:
        for x in (sharded, multi, cold, e):
            x.close()


def test_page_locked_destinations():
    from renderbaby_amd.engine import PinnedFrame
    s = scenes.cornell(64, 48, 2, 4)
    rc = RenderConfig.from_scene(s)
    e = Engine.new(rc, device=0)
    pin = PinnedFrame(64, 48)
    try:
        e.render(rc)
        want = e.denoise()
        got = e.denoise(out=pin.array)
        assert got is pin.array and np.array_equal(got, want)
    finally:
        pin.free()
        e.close()


# ---- 4. quality
def tone_mse(lin, ref):
    a, b = lin[..., :3].astype(np.float64), ref[..., :3].astype(np.float64)
    return float((((a / (a + 1)) - (b / (b + 1))) ** 2).mean())


QUALITY = [("cornell", lambda spp: scenes.cornell(256, 256, spp, 4)), ("mesh", lambda spp: scenes.mesh_scene(48, 48, 256, 256, spp, 4, seed=3))]


@pytest.mark.parametrize("name,make", QUALITY, ids=[q[0] for q in QUALITY])
def test_denoised_4spp_is_closer_to_the_converged_render_than_raw_4spp(name, make):
    """256 x 256, depth 4: mean squared error of x / (x + 1) against the same engine's 1024-spp render, default parameters.
    The condition is `denoised < raw`; the measured errors and their ratio are recorded in DESIGN.md section 13 and
    profiles/r09_denoise_rate.txt."""
    out = {}
    for spp in (1024, 4):
        rc = RenderConfig.from_scene(make(spp))
        e = Engine.new(rc, device=0)
        try:
            e.render(rc)
            out[spp] = e.denoise(denoise.params(iterations=0), linear=True)   # the mean radiance, mirrored
            if spp == 4:
                den = e.denoise(linear=True)
        finally:
            e.close()
    ref, raw = out[1024], out[4]
    m_raw, m_den = tone_mse(raw, ref), tone_mse(den, ref)
    print(f"quality {name}: raw 4 spp {m_raw:.6g}, denoised {m_den:.6g}, ratio {m_den / m_raw:.4f}")
    assert m_den < m_raw
