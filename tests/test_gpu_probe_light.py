"""Light points from a baked probe grid on the device (rb_probe_coefficients / rb_light_points and their device forms; DESIGN.md
section 19), bit for bit on uint32 views:

  both stages = the numpy model renderbaby_amd/probes.py (coefficients, light) on grids of 1 .. 125 probes, for points inside
                and outside the grid, on cell faces, at probes, invalid ones, with invalid probes among their corners;
  the forms, the pieces and the two launch shapes give the same answers, and a call has a query's side effects: none;
  end to end a baked grid lights points as the model says, and under a uniform sky as the float64 irradiance of section 18 says.
"""
import numpy as np
import pytest

from renderbaby_amd import Engine, RenderConfig, abi, aov, bake, engine, probes, scenes
from tests import _oracle
from tests.conftest import has_gpu
from tests.test_gpu_hemisphere import scene_surfels
from tests.test_gpu_query import _engine
from tests.test_probe_light_abi import GRID_REFUSALS, INVALID_OPTIONS, LIMIT, NULL_ARGUMENT, _grid
from tests.test_probe_light_model import lit_words, random_sums, u32

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

f32, f64 = np.float32, np.float64
GRIDS = [(1, 1, 1), (2, 1, 3), (3, 4, 2), (5, 5, 5)]
SIZES = [1, 63, 65, 130]
BOX = ((-1.0, -2.0, 0.0), (2.0, 2.0, 1.0))


def sh_words(sh):
    return u32(np.ascontiguousarray(sh).view(f32).reshape(-1, 28))


def dark_probes(counts):
    """the record indices of the probes of the topmost cell (every corner that exists) and of probe 0: the invalid ones"""
    nx, ny, nz = counts
    top = [range(max(c - 2, 0), c) for c in counts]
    cell = [(iz * ny + iy) * nx + ix for iz in top[2] for iy in top[1] for ix in top[0]]
    return sorted(set(cell) | {0}) if nx * ny * nz > 1 else []


def grid_case(counts, seed=5):
    """(grid, sums, coefficients by the model): random sums, the probes of ``dark_probes`` invalid in four ways"""
    rng = np.random.default_rng(seed + sum(counts))
    n = counts[0] * counts[1] * counts[2]
    grid = probes.grid_params(*BOX, counts)
    sh = random_sums(n, rng)
    for k, i in enumerate(dark_probes(counts)):
        sh["weight"][i] = (0.0, np.nan, -3.0, np.inf)[k % 4]
    return grid, sh, probes.coefficients(sh)


def mixed_points(grid, m, seed=11):
    """m points and normals, point i of kind i % 7: 0 inside the grid, 1 outside it, 2 on a cell face, 3 exactly at a probe,
    4 invalid, 5 in the cell of probe 0 (an invalid probe among its corners), 6 in the topmost cell (all corners invalid)"""
    rng = np.random.default_rng(seed)
    org, step, cnt = grid["origin"].astype(f64), grid["step"].astype(f64), grid["counts"].astype(f64)
    span = np.maximum(cnt - 1.0, 0.0) * step
    pos = (org + rng.uniform(0.0, 1.0, (m, 3)) * span).astype(f32)
    nrm = rng.normal(size=(m, 3)).astype(f32) * f32(3.0)
    for i in range(m):
        kind = i % 7
        if kind == 1:
            a = rng.integers(3)
            pos[i, a] = f32(org[a] - rng.uniform(0.1, 9.0) * step[a]) if rng.integers(2) else f32(org[a] + span[a] + rng.uniform(0.1, 9.0) * step[a])
        elif kind == 2:
            a = rng.integers(3)
            pos[i, a] = f32(org[a] + rng.integers(0, int(cnt[a])) * step[a])
        elif kind == 3:
            pos[i] = (org + np.array([rng.integers(0, int(c)) for c in cnt]) * step).astype(f32)
        elif kind == 4:
            bad = [(np.inf, 0), (np.nan, 0), (0, np.nan), (0, -np.inf)][(i // 7) % 4]
            pos[i, 1] += f32(bad[0])
            nrm[i, 2] += f32(bad[1])
            if (i // 7) % 5 == 4:
                nrm[i] = 0
        elif kind == 5:
            pos[i] = (org + rng.uniform(0.05, 0.95, 3) * step * (cnt > 1)).astype(f32)
        elif kind == 6:
            pos[i] = (org + span - rng.uniform(0.05, 0.95, 3) * step * (cnt > 1)).astype(f32)
    return pos, nrm


def assert_lit_equal(got, want, where):
    assert got.dtype == abi.LIT and got.shape == want.shape, where
    bad = np.nonzero((lit_words(got) != lit_words(want)).any(1))[0]
    assert len(bad) == 0, (where, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])


# ---- 1. both stages against the model
@pytest.mark.parametrize("counts", GRIDS, ids=["x".join(map(str, g)) for g in GRIDS])
def test_both_stages_equal_the_model(counts):
    grid, sh, co = grid_case(counts)
    got_co = engine.probe_coefficients(sh, device=0)
    assert got_co.dtype == abi.SH9 and np.array_equal(sh_words(got_co), sh_words(co)), counts
    dark = dark_probes(counts)
    assert (sh_words(got_co[dark]) == 0).all() and (got_co["weight"][[i for i in range(len(sh)) if i not in dark]] == 1.0).all()
    seen = dict(unlit=0, partial=0, full=0, invalid=0)
    for m in SIZES:
        pos, nrm = mixed_points(grid, m, seed=11 + m)
        want = probes.light(grid, co, pos, nrm)
        assert_lit_equal(engine.light_points(grid, got_co, pos, nrm, device=0), want, (counts, m))
        valid = np.isfinite(pos).all(1) & np.isfinite(nrm).all(1) & (nrm != 0).any(1)
        seen["invalid"] += int((~valid).sum())
        seen["unlit"] += int((valid & (want["weight"] == 0)).sum())
        seen["partial"] += int(((want["weight"] > 0) & (want["weight"] < 0.99)).sum())
        seen["full"] += int((want["weight"] >= 0.99).sum())
    print(counts, seen)
    assert seen["invalid"] > 0 and seen["full"] > 0
    if len(dark):
        assert seen["unlit"] > 0 and seen["partial"] > 0
    else:   # one probe: again with that probe invalid, and nothing is lit
        dead = sh.copy()
        dead["weight"] = 0
        pos, nrm = mixed_points(grid, 65)
        out = engine.light_points(grid, engine.probe_coefficients(dead, device=0), pos, nrm, device=0)
        assert (lit_words(out) == 0).all()


# ---- 2. the forms
def test_engine_forms_equal_the_engineless_forms_for_numpy_and_torch(monkeypatch):
    import torch
    counts = (3, 4, 2)
    grid, sh, co = grid_case(counts)
    pos, nrm = mixed_points(grid, 130)
    want = probes.light(grid, co, pos, nrm)
    e = _engine(scenes.feature_scene(width=24, height=16))
    try:
        st0 = e.stats()
        # numpy in, numpy out
        got_co = e.probe_coefficients(sh)
        assert e.last_query_kernel_name() == "k_probe_coeffs" and e.last_query_ms() > 0
        assert got_co.dtype == abi.SH9 and np.array_equal(sh_words(got_co), sh_words(co))
        assert_lit_equal(e.light_points(grid, got_co, pos, nrm), want, "numpy")
        assert e.last_query_kernel_name() == "k_probe_light" and e.last_query_ms() > 0
        surf = np.zeros(130, dtype=abi.SURFEL)
        surf["pos"], surf["normal"] = pos, nrm
        assert_lit_equal(e.light_points(grid, got_co, surf), want, "surfel records")
        assert_lit_equal(engine.light_points(grid, co, surf, device=0), want, "engine-less surfel records")
        # tensors in, tensors out, nothing copied; the coefficients in place
        t_sh = torch.from_numpy(sh.view(f32).reshape(-1, 28).copy()).cuda()
        t_co = e.probe_coefficients(t_sh)
        assert t_co.shape == (24, 28) and t_co.is_cuda and t_co is not t_sh and np.array_equal(sh_words(t_co.cpu().numpy()), sh_words(co))
        assert np.array_equal(sh_words(t_sh.cpu().numpy()), sh_words(sh))   # the input stands
        assert e.probe_coefficients(t_sh, out=t_sh) is t_sh and np.array_equal(sh_words(t_sh.cpu().numpy()), sh_words(co))
        t_surf = torch.from_numpy(surf.view(f32).reshape(-1, 8).copy()).cuda()
        t_lit = e.light_points(grid, t_sh, t_surf)
        assert t_lit.shape == (130, 4) and t_lit.is_cuda and t_lit.dtype == torch.float32
        assert_lit_equal(t_lit.cpu().numpy().view(abi.LIT).reshape(-1), want, "torch")
        t_out = torch.full((130, 4), -1.0, dtype=torch.float32, device="cuda")
        assert e.light_points(grid, t_sh, torch.from_numpy(pos).cuda(), torch.from_numpy(nrm).cuda(), out=t_out) is t_out
        assert_lit_equal(t_out.cpu().numpy().view(abi.LIT).reshape(-1), want, "torch points and normals")
        assert len(e.light_points(grid, got_co, pos[:0], nrm[:0])) == 0 and len(e.probe_coefficients(sh[:0])) == 0
        # the other launch shape
        monkeypatch.setenv("RB_LIGHT_SHAPE", "wide")
        assert_lit_equal(e.light_points(grid, got_co, pos, nrm), want, "wide")
        assert e.last_query_kernel_name() == "k_probe_light_wide"
        assert_lit_equal(engine.light_points(grid, co, pos, nrm, device=0), want, "engine-less wide")
        monkeypatch.setenv("RB_LIGHT_SHAPE", "pairs")
        assert_lit_equal(e.light_points(grid, got_co, pos, nrm), want, "pairs")
        assert e.last_query_kernel_name() == "k_probe_light"
        monkeypatch.delenv("RB_LIGHT_SHAPE")
        assert e.stats() == st0, "lighting points moved rb_get_stats"
        for bad in (dict(coeffs=co[:5]), dict(out=t_out[:5]), dict(out=np.zeros(130, abi.LIT))):
            with pytest.raises(ValueError):
                e.light_points(grid, **dict(dict(coeffs=got_co, points=pos, normals=nrm), **bad))
    finally:
        e.close()


# ---- 3. pieces
def test_points_across_piece_boundaries(monkeypatch):
    grid, sh, co = grid_case((5, 5, 5))
    pos, nrm = mixed_points(grid, 130 + 128)
    want = probes.light(grid, co, pos, nrm)
    one = engine.light_points(grid, co, pos, nrm, device=0)
    monkeypatch.setenv("RB_LIGHT_PIECE_POINTS", "128")   # three pieces: 128, 128, 2
    cut = engine.light_points(grid, co, pos, nrm, device=0)
    monkeypatch.delenv("RB_LIGHT_PIECE_POINTS")
    assert_lit_equal(one, want, "one piece")
    assert_lit_equal(cut, one, "three pieces")


# ---- 4. side effects, refusals, shards
def test_refusals_leave_the_engine_rendering_the_golden_frame():
    import torch
    from renderbaby_amd._lib import load
    lib = load()
    s = scenes.cornell(32, 32, 2, 4)
    rc = RenderConfig.from_scene(s)
    grid, sh, co = grid_case((2, 1, 3))
    g = np.asarray(grid).reshape(1)
    pos, nrm = mixed_points(grid, 4, seed=3)
    surf = np.zeros(4, dtype=abi.SURFEL)
    surf["pos"], surf["normal"] = pos, nrm
    want = probes.light(grid, co, pos, nrm)
    e = Engine.new(rc, device=0)
    try:
        e.update(rc)
        h, st0 = e._h, e.stats()
        d_co = torch.from_numpy(co.view(f32).reshape(-1, 28).copy()).cuda()
        d_pts = torch.from_numpy(surf.view(f32).reshape(-1, 8).copy()).cuda()
        d_out = torch.full((64, 4), 7, dtype=torch.float32, device="cuda")
        d_sh = torch.full((64, 28), 7, dtype=torch.float32, device="cuda")
        lp, pc = lib.rb_light_points_device, lib.rb_probe_coefficients_device
        for name, kw in GRID_REFUSALS:
            assert lp(h, _grid(**kw).ctypes.data, d_co.data_ptr(), d_pts.data_ptr(), 4, d_out.data_ptr()) == INVALID_OPTIONS, name
            assert lib.rb_last_error(h)
        assert lp(h, g.ctypes.data, d_co.data_ptr(), d_pts.data_ptr(), LIMIT + 1, d_out.data_ptr()) == INVALID_OPTIONS
        assert lp(h, None, d_co.data_ptr(), d_pts.data_ptr(), 4, d_out.data_ptr()) == NULL_ARGUMENT
        assert lp(h, g.ctypes.data, None, d_pts.data_ptr(), 4, d_out.data_ptr()) == NULL_ARGUMENT
        assert lp(h, g.ctypes.data, d_co.data_ptr(), None, 4, d_out.data_ptr()) == NULL_ARGUMENT
        assert lp(h, g.ctypes.data, d_co.data_ptr(), d_pts.data_ptr(), 4, None) == NULL_ARGUMENT
        assert lp(h, g.ctypes.data, None, None, 0, None) == 0 and pc(h, None, 0, None) == 0
        assert pc(h, d_sh.data_ptr(), LIMIT + 1, d_sh.data_ptr()) == INVALID_OPTIONS
        assert pc(h, None, 4, d_sh.data_ptr()) == NULL_ARGUMENT and pc(h, d_sh.data_ptr(), 4, None) == NULL_ARGUMENT
        # the device forms' buffers: host pointers, misaligned ones, allocations that end early
        assert lp(h, g.ctypes.data, co.ctypes.data, d_pts.data_ptr(), 4, d_out.data_ptr()) == INVALID_OPTIONS
        assert lp(h, g.ctypes.data, d_co.data_ptr(), surf.ctypes.data, 4, d_out.data_ptr()) == INVALID_OPTIONS
        assert lp(h, g.ctypes.data, d_co.data_ptr(), d_pts.data_ptr(), 4, want.ctypes.data) == INVALID_OPTIONS
        assert lp(h, g.ctypes.data, d_sh.data_ptr() + 4, d_pts.data_ptr(), 4, d_out.data_ptr()) == INVALID_OPTIONS
        assert lp(h, g.ctypes.data, d_co.data_ptr(), d_pts.data_ptr() + 8, 3, d_out.data_ptr()) == INVALID_OPTIONS
        assert lp(h, g.ctypes.data, d_co.data_ptr(), d_pts.data_ptr(), 4, d_out.data_ptr() + 4) == INVALID_OPTIONS
        assert lp(h, g.ctypes.data, d_co.data_ptr(), d_pts.data_ptr(), 1 << 20, d_out.data_ptr()) == INVALID_OPTIONS   # 32 MiB of surfels
        big = _grid(counts=(1 << 10, 1 << 10, 1))   # 2^20 records asked of a buffer of six
        assert lp(h, big.ctypes.data, d_co.data_ptr(), d_pts.data_ptr(), 4, d_out.data_ptr()) == INVALID_OPTIONS
        assert pc(h, sh.ctypes.data, 6, d_sh.data_ptr()) == INVALID_OPTIONS and pc(h, d_sh.data_ptr(), 6, sh.ctypes.data) == INVALID_OPTIONS
        assert pc(h, d_sh.data_ptr() + 8, 6, d_sh.data_ptr()) == INVALID_OPTIONS and pc(h, d_sh.data_ptr(), 1 << 20, d_sh.data_ptr()) == INVALID_OPTIONS
        lib.rb_sync(h)
        assert (d_out == 7).all().item() and (d_sh == 7).all().item()
        # and the call that is in order
        assert lp(h, g.ctypes.data, d_co.data_ptr(), d_pts.data_ptr(), 4, d_out.data_ptr()) == 0 and lib.rb_sync(h) == 0
        assert_lit_equal(d_out.cpu().numpy()[:4].copy().view(abi.LIT).reshape(-1), want, "after the refusals")
        assert (d_out[4:] == 7).all().item()
        assert e.stats() == st0, "refusals or a call moved rb_get_stats"
        assert np.array_equal(e.render(rc).pixels, _oracle.render(s)[2])
    finally:
        e.close()
    cold = Engine.new(rc, device=0)   # no update yet: every engine entry point asks for a scene, an empty call too -- and refuses first
    try:
        assert lib.rb_light_points_device(cold._h, g.ctypes.data, None, None, 0, None) not in (0, INVALID_OPTIONS, NULL_ARGUMENT)
        assert lib.rb_probe_coefficients_device(cold._h, None, 0, None) not in (0, INVALID_OPTIONS, NULL_ARGUMENT)
        assert lib.rb_light_points_device(cold._h, _grid(flags=1).ctypes.data, None, None, 0, None) == INVALID_OPTIONS
        assert np.array_equal(cold.render(rc).pixels, _oracle.render(s)[2])
    finally:
        cold.close()


def test_a_call_between_iterator_frames():
    s = scenes.feature_scene(width=48, height=32, spp=4)
    rc = RenderConfig.from_scene(s)
    grid, sh, co = grid_case((3, 4, 2))
    pos, nrm = mixed_points(grid, 130)
    want = probes.light(grid, co, pos, nrm)

    def frames(query):
        e = Engine.new(rc, device=0)
        it = e.frame_iterator(rc)
        out = []
        while it.has_next():
            out.append(it.next().pixels.copy())
            if query:
                kernel = e.last_kernel_name()
                assert_lit_equal(e.light_points(grid, e.probe_coefficients(sh), pos, nrm), want, len(out))
                assert e.last_kernel_name() == kernel and e.last_query_kernel_name() == "k_probe_light"
        acc, st = e.read_accumulation(), e.stats()
        e.close()
        return out, acc, st
    plain, acc0, st0 = frames(False)
    asked, acc1, st1 = frames(True)
    assert len(plain) == len(asked) == 4
    for a, b in zip(plain, asked):
        assert np.array_equal(a, b)
    assert np.array_equal(u32(acc0), u32(acc1))
    assert all(st0[k] == st1[k] for k in st0 if not k.endswith("_ms")), (st0, st1)


def test_sharded_engine_and_multi_device_handle():
    import torch
    s = scenes.feature_scene(width=24, height=16)
    grid, sh, co = grid_case((3, 4, 2))
    pos, nrm = mixed_points(grid, 130)
    want = probes.light(grid, co, pos, nrm)
    t_sh = torch.from_numpy(sh.view(f32).reshape(-1, 28).copy()).cuda()
    for kw in (dict(shard_rank=1, shard_count=3, stripe_rows=8), dict(devices=[0, 0], gather_peer_copy=True)):
        p = _engine(s, **kw)
        try:
            got_co = p.probe_coefficients(sh)
            assert np.array_equal(sh_words(got_co), sh_words(co)), kw
            assert_lit_equal(p.light_points(grid, got_co, pos, nrm), want, kw)
            t_lit = p.light_points(grid, p.probe_coefficients(t_sh), torch.from_numpy(pos).cuda(), torch.from_numpy(nrm).cuda())
            assert_lit_equal(t_lit.cpu().numpy().view(abi.LIT).reshape(-1), want, kw)
            assert p.last_query_kernel_name() == "k_probe_light" and p.last_query_ms() > 0
        finally:
            p.close()


# ---- 5. end to end
def test_a_baked_grid_lights_points_as_the_model_says():
    """no Monte-Carlo tolerance: the device's own rb_bake_probes output through both stages on the device and through the model"""
    s = scenes.feature_scene(width=24, height=16)
    e = _engine(s)
    try:
        pts, nrm = scene_surfels(e, s)
        lo, hi = pts.min(0) - f32(0.5), pts.max(0) + f32(0.5)
        sh = e.bake_probes(probes.grid(lo, hi, (2, 2, 2)), 64)
        grid = probes.grid_params(lo, hi, (2, 2, 2))
        assert (sh["weight"] > 0).all()
        co = engine.probe_coefficients(sh, device=0)
        assert np.array_equal(sh_words(co), sh_words(probes.coefficients(sh)))
        lit = engine.light_points(grid, co, pts, nrm, device=0)
        assert_lit_equal(lit, probes.light(grid, probes.coefficients(sh), pts, nrm), "feature scene")
        assert (lit["weight"] > 0.99).all() and (lit["value"] > 0).any(1).sum() > 100 and np.isfinite(lit["value"]).all()
        g2, c2 = bake.probe_grid(e, lo, hi, (2, 2, 2), 64)
        assert np.array_equal(u32(np.asarray(g2).reshape(1).view(f32)), u32(np.asarray(grid).reshape(1).view(f32)))
        assert np.array_equal(sh_words(c2), sh_words(co))
    finally:
        e.close()


def test_under_a_uniform_sky_the_blend_is_section_18s_irradiance():
    """against the float64 blend of probes.irradiance(...) / pi over the same records: 1e-5 x the size of the terms"""
    c = np.array([0.5, 0.7, 1.0], f32)
    s = scenes.sky_only(sky=tuple(c))
    e = _engine(s)
    try:
        lo, hi = (-2.0, -1.0, -3.0), (2.0, 3.0, 1.0)
        sh = e.bake_probes(probes.grid(lo, hi, (2, 2, 2)), 256)
        grid = probes.grid_params(lo, hi, (2, 2, 2))
        co = e.probe_coefficients(sh)
        pos, nrm = mixed_points(grid, 130)
        keep = np.isfinite(pos).all(1) & np.isfinite(nrm).all(1) & (nrm != 0).any(1)
        pos, nrm = pos[keep], nrm[keep]
        lit = e.light_points(grid, co, pos, nrm)
        table = probes.irradiance(sh, probes._unit(nrm)) / np.pi   # (probe, point, channel)
        want, W, size = probes.blend64(grid, co, pos, nrm, corner_values=lambda idx, n: table[idx, np.arange(len(idx))])
        err = np.abs(lit["value"].astype(f64) - np.maximum(want, 0.0))
        print("max error / size:", (err / size).max(), "value range:", lit["value"].min(), lit["value"].max())
        assert (W > 0.999).all() and (err <= 1e-5 * size).all()
        assert (np.abs(lit["value"].astype(f64) - c.astype(f64)) < 0.5).all()   # and it is the sky's colour, to the noise of 256 samples
    finally:
        e.close()


def test_probe_lit_preview():
    s = scenes.feature_scene(width=32, height=20)
    e = _engine(s)
    try:
        hits, surf = e.render_hits(surfaces=True)
        grid, co = bake.probe_grid(e, (-6.0, 0.1, -12.0), (6.0, 6.0, 2.0), (3, 2, 3), 32)
        img = aov.probe_lit(e, grid, co, hits, surf)
        assert img.shape == (20, 32, 3) and img.dtype == f32 and np.isfinite(img).all() and (img >= 0).all()
        emits = (surf["emissive"] > 0).any(-1) | (hits["kind"] == abi.HIT_LIGHT) | (hits["kind"] == abi.HIT_NONE)
        assert emits.any() and (~emits).any()
        assert np.array_equal(u32(img[emits]), u32(surf["emissive"][emits]))
        lit = ~emits & (hits["kind"] != abi.HIT_INVALID)
        assert (img[lit] > 0).any()
        assert aov.color_map(img).shape == (20, 32, 3)
    finally:
        e.close()
