"""The baked-probe kernels (k_probe_coeffs, k_probe_light, k_probe_light_wide, k_probe_moments, k_probe_light_vis; csrc/
rb_probe_light.hip, rb_probe_depth.hip, rb_probe_visibility.hip, rb_device_probe.hpp) at degenerate inputs, where
tests/test_gpu_probe_light.py and tests/test_gpu_probe_visibility.py stop: whatever a caller's baker, loader or accumulation
loop may leave in the records -- NaN, infinities, subnormals, negative and huge words in every field --, normals at and round the
guards of the fast square root and division, texel boundaries walked an ulp at a time, points as far out as a float reaches,
and sums that overflow on the way through bake, moments and blend.  DESIGN.md section 20.6 has the tables.

The reference is the numpy model (renderbaby_amd/probes.py), itself held to the scalar transcription of the definition
(tests/_probe_scalar.py) on these very cases by tests/test_probe_edges_model.py.  All comparisons are on uint32 views through the
engine-less forms with device = 0.  The blend (rb_lit) is compared with no exception at all: that the model's words hold no
NaN is asserted first.  Stage 1, the moments and the bakes are compared under the one rule sections 19.1 and 20.1 state: where
the model's word is a NaN the device's must be a NaN, of any sign and payload; every other word is equal in every bit.  Every
section prints how many NaN words it compared.  No input is left out of a comparison but the far points of section f in the
visible blend, which section 20.1 puts outside the contract.
"""
import numpy as np
import pytest

from renderbaby_amd import abi, engine, probes, scenes
from renderbaby_amd._lib import load
from tests import _probe_edge_cases as C
from tests.conftest import has_gpu
from tests.test_gpu_query import _engine

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

f32, f64 = np.float32, np.float64
SHAPES = ("pairs", "wide")
LIVE = 16


def held(got, want, width, where, nan_rule=False):
    bad, nans = C.mismatches(got, want, width, nan_rule)
    assert len(bad) == 0, (where, len(bad), "rows differ", bad[:5], np.ascontiguousarray(got).view(f32).reshape(-1, width)[bad[:3]],
                           np.ascontiguousarray(want).view(f32).reshape(-1, width)[bad[:3]])
    return nans


def no_nan(lit, where):
    assert not np.isnan(np.ascontiguousarray(lit).view(f32)).any(), (where, "the model's rb_lit holds a NaN")


def changed(a, b):
    return int((C.words(a, 4) != C.words(b, 4)).any(1).sum())


def plain_blend(grid, co, pos, nrm, want, where, monkeypatch):
    """rb_light_points under both launch shapes against ``want``, every bit"""
    no_nan(want, where)
    for shape in SHAPES:
        monkeypatch.setenv("RB_LIGHT_SHAPE", shape)
        got = engine.light_points(grid, co, pos, nrm, device=0)
        held(got, want, 4, (where, shape))
    monkeypatch.delenv("RB_LIGHT_SHAPE")
    return got


def visible_blend(grid, co, mm, pos, nrm, kw, where, keep=None):
    want = probes.light_visible(grid, co, mm, pos, nrm, probes.visibility_params(**kw))
    got = engine.light_points_visible(grid, co, mm, pos, nrm, device=0, **kw)
    if keep is None:
        no_nan(want, where)
        held(got, want, 4, (where, kw))
    else:
        no_nan(want[keep], where)
        held(got[keep], want[keep], 4, (where, kw))
    return got, want


# ---- a. stage 1
def test_stage_1_on_every_pair_of_specials():
    sh = C.stage1_records()
    want = probes.coefficients(sh)
    nans = held(engine.probe_coefficients(sh, device=0), want, 28, "stage 1", nan_rule=True)
    same = sh.copy()
    assert load().rb_probe_coefficients(0, same.ctypes.data, len(same), same.ctypes.data) == 0   # out = in
    held(same, want, 28, "stage 1 in place", nan_rule=True)
    print("stage 1:", nans, "NaN words of", want.view(f32).size, "compared under the NaN rule")
    assert nans > 0


# ---- b. normals
NORMALS = C.normal_cases()


@pytest.mark.parametrize("name", list(NORMALS))
def test_normals(name, monkeypatch):
    grid, co = C.valid_grid()
    nrm = NORMALS[name]
    pos = C.positions_inside(grid, len(nrm), seed=3)
    plain_blend(grid, co, pos, nrm, probes.light(grid, co, pos, nrm), name, monkeypatch)


@pytest.mark.parametrize("k", C.SCALES)
def test_a_scaled_normal_gives_the_same_bits(k, monkeypatch):
    """light_points(nrm 2^k) == light_points(nrm), the device against itself: the pair straddles the guards of sqrt_exact and
    div3_exact, so the fast paths and the compiler's are held to each other.  The normals are ``lattice_normals``, for which
    the definition is invariant at every k; arbitrary components are too at every k but -70, where their squares are rounded as
    subnormals (the model itself moves 254 of 256 points): those are held to the model there, as in section b."""
    for lattice in (True, False):
        grid, co, pos, nrm, big = C.scaled_pair(k, lattice)
        for shape in SHAPES:
            monkeypatch.setenv("RB_LIGHT_SHAPE", shape)
            base, got = engine.light_points(grid, co, pos, nrm, device=0), engine.light_points(grid, co, pos, big, device=0)
            assert (base["weight"] > 0).all()
            if lattice or k != -70:
                held(got, base, 4, ("scaled by 2^%d" % k, "lattice" if lattice else "arbitrary", shape))
            held(got, probes.light(grid, co, pos, big), 4, ("scaled by 2^%d against the model" % k, shape))


# ---- c. coefficient records, one hazard to a grid
@pytest.fixture(scope="module")
def live_engine():
    e = _engine(scenes.feature_scene(width=24, height=16))
    yield e
    e.close()


@pytest.mark.parametrize("hazard", list(C.record_hazards()))
@pytest.mark.parametrize("m", [65, 256])
def test_one_hazard_in_one_record(hazard, m, monkeypatch):
    grid, pos, nrm, _, at_neighbour = C.record_points(m)
    base = C.record_base()
    co = base.copy()
    C.record_hazards()[hazard](co)
    clean, want = probes.light(grid, base, pos, nrm), probes.light(grid, co, pos, nrm)
    assert changed(want, clean) >= LIVE, (hazard, "the case is not live")
    got = plain_blend(grid, co, pos, nrm, want, hazard, monkeypatch)
    if hazard not in C.SHOWS_AT_A_NEIGHBOUR:
        assert changed(got[at_neighbour], clean[at_neighbour]) == 0, "a record showed at a neighbouring probe"
    # the same through section 20's kernel with both weights off, and with the wrap weight alone
    visible_blend(grid, co, None, pos, nrm, dict(wrap=False, depth=False), hazard)
    visible_blend(grid, co, None, pos, nrm, dict(depth=False), hazard)


def test_the_engine_forms_on_tensors(live_engine, monkeypatch):
    """every hazard of section c, and three of section d, through rb_light_points_device and rb_light_points_visible_device"""
    import torch
    e = live_engine
    grid, pos, nrm, _, _ = C.record_points(256)
    t_pos, t_nrm = torch.from_numpy(pos).cuda(), torch.from_numpy(nrm).cuda()
    for hazard, plant in C.record_hazards().items():
        co = C.record_base()
        plant(co)
        want = probes.light(grid, co, pos, nrm)
        t_co = torch.from_numpy(co.view(f32).reshape(-1, 28).copy()).cuda()
        for shape in SHAPES:
            monkeypatch.setenv("RB_LIGHT_SHAPE", shape)
            got = e.light_points(grid, t_co, t_pos, t_nrm)
            assert e.last_query_kernel_name() == ("k_probe_light_wide" if shape == "wide" else "k_probe_light")
            held(got.cpu().numpy().view(abi.LIT).reshape(-1), want, 4, (hazard, shape, "torch"))
    monkeypatch.delenv("RB_LIGHT_SHAPE")
    grid, co, pos, nrm = C.moment_points(65)
    t_co = torch.from_numpy(co.view(f32).reshape(-1, 28).copy()).cuda()
    t_pos, t_nrm = torch.from_numpy(pos).cuda(), torch.from_numpy(nrm).cuda()
    for hazard in ("mean qnan", "mean2 0.0", "valid -0.0"):
        mm = C.benign_moments(8)
        C.moment_hazards()[hazard](mm, slice(None))
        t_mm = torch.from_numpy(mm.view(f32).reshape(-1, 256).copy()).cuda()
        for kw in C.SETTINGS[:3]:
            want = probes.light_visible(grid, co, mm, pos, nrm, probes.visibility_params(**kw))
            got = e.light_points_visible(grid, t_co, t_mm, t_pos, t_nrm, **kw)
            held(got.cpu().numpy().view(abi.LIT).reshape(-1), want, 4, (hazard, kw, "torch"))
        t_out, t_share = e.probe_moments(t_mm)
        want_mom, want_share = probes.moments(mm)
        held(t_out.cpu().numpy(), want_mom, 256, (hazard, "moments of moments, torch"), nan_rule=True)
        held(t_share.cpu().numpy(), want_share, 1, (hazard, "share, torch"), nan_rule=True)


# ---- d. moments, one hazard to a map
_clean = {}


def clean_blend(k):
    if k not in _clean:
        grid, co, pos, nrm = C.moment_points(65)
        _clean[k] = probes.light_visible(grid, co, C.benign_moments(8), pos, nrm, probes.visibility_params(**C.SETTINGS[k]))
    return _clean[k]


@pytest.mark.parametrize("scope", ["one probe", "all probes"])
@pytest.mark.parametrize("hazard", list(C.moment_hazards()))
def test_one_hazard_in_the_maps(hazard, scope):
    grid, co, pos, nrm = C.moment_points(65)
    mm = C.benign_moments(8)
    C.moment_hazards()[hazard](mm, slice(C.MOMENT_PROBE, C.MOMENT_PROBE + 1) if scope == "one probe" else slice(None))
    for k, kw in enumerate(C.SETTINGS):
        got, want = visible_blend(grid, co, mm, pos, nrm, kw, (hazard, scope))
        n = changed(want, clean_blend(k))
        if hazard in C.NOT_SHOWN or C.setting_hides_the_maps(kw):
            assert n == 0 and changed(got, clean_blend(k)) == 0, (hazard, scope, kw, n, "showed, and the definition says it must not")
        else:
            assert n >= LIVE, (hazard, scope, kw, n, "the case is not live")


@pytest.mark.parametrize("kw", C.EXTRA_SETTINGS, ids=[f"{k}={C.name_of(v)}" for kw in C.EXTRA_SETTINGS for k, v in kw.items()])
def test_the_floor_and_the_bias_at_their_edges(kw):
    grid, co, pos, nrm = C.points_near_probes(65) if "min_visibility" in kw else C.moment_points(65)
    hidden = C.benign_moments(8)
    C.moment_hazards()["mean2 == mean mean"](hidden, slice(None))
    far = C.overflowing(grid, pos, nrm, kw.get("normal_bias", 0.0))
    assert not far.any(), "no difference of positions overflows: every point is in contract"
    for name, mm in (("benign", C.benign_moments(8)), ("variance 0", hidden), ("shut", C.shut_moments(8))):
        got, want = visible_blend(grid, co, mm, pos, nrm, kw, name)
    if "min_visibility" in kw:
        assert (want["weight"] > 0).sum() >= LIVE, "the floor lit nothing: the case is not live"
    elif abs(float(kw["normal_bias"])) > 1:
        assert (want["weight"] == 0).sum() >= LIVE


# ---- e. the texel
@pytest.mark.parametrize("origin", [(0.0, 0.0, 0.0), (3.0, -5.0, 7.0)], ids=["origin 0", "origin 3 -5 7"])
@pytest.mark.parametrize("log2_scale", [0, 20, -20])
def test_the_texel_a_point_reads(origin, log2_scale):
    """a 1 x 1 x 1 grid, the wrap off, a floor of 0; texel T carries mean 0, valid 1 and its own mean2, so W = (mean2[T] / (mean2[T]
    + r r))^3 names the texel that was read (tests/test_probe_edges_model.py proves it does, and that all the boundaries occur)"""
    scale = 2.0 ** log2_scale
    grid, co = C.texel_grid(origin)
    walk, labels = C.texel_vectors()
    vec = np.concatenate([walk * f32(scale), np.zeros((1, 3), f32), probes.oct_centres() * f32(scale)]).astype(f32)
    pos = (np.asarray(origin, f32) + vec).astype(f32)
    nrm = np.tile(np.array([(0.0, 0.0, 1.0)], f32), (len(pos), 1))
    got, want = visible_blend(grid, co, C.texel_map(scale), pos, nrm, dict(wrap=False, min_visibility=0.0), ("texel", origin, log2_scale))
    if origin == (0.0, 0.0, 0.0):   # from the model: every walk falls on both sides of its boundary, and the centres reach all 64
        T = probes.oct_texel(vec[:len(walk)])
        C.boundaries_straddled(labels, T % 8, T // 8, vec[:len(walk), 2] < 0)
        assert set(probes.oct_texel(vec[-64:]).tolist()) == set(range(64))


# ---- f. far and clamped points
@pytest.mark.parametrize("counts", [(1, 1, 1), (2, 2, 2), (2, 1, 3)], ids=["1x1x1", "2x2x2", "2x1x3"])
def test_far_points(counts, monkeypatch):
    grid, co = C.valid_grid(counts)
    pos, nrm, far = C.far_points(grid, 256)
    want = probes.light(grid, co, pos, nrm)
    assert far.sum() == 128 and (want["weight"][far] > 0).all()
    plain_blend(grid, co, pos, nrm, want, ("far", counts), monkeypatch)   # the clamp is in contract: every word
    mm = C.benign_moments(len(co))
    for kw in C.SETTINGS:   # one call holds both kinds; RB_OK, or the binding raises
        got, model = visible_blend(grid, co, mm, pos, nrm, kw, ("far, visible", counts), keep=~far)
        bad, _ = C.mismatches(got[far], model[far], 4, nan_rule=True)
        print(counts, kw, ":", int(far.sum()) - len(bad), "of", int(far.sum()), "far points equal the model (outside the contract: not asserted)")


# ---- g. k_probe_moments
SUMS = C.moment_sums()


@pytest.mark.parametrize("name", list(SUMS))
def test_moments(name):
    sums = SUMS[name]
    want, want_share = probes.moments(sums)
    got, share = engine.probe_moments(sums, device=0)
    nans = held(got, want, 256, name, nan_rule=True)
    nans += held(share, want_share, 1, (name, "share"), nan_rule=True)
    lib = load()
    for ask in (True, False):
        same, sh = sums.copy(), np.full(len(sums), 7, f32)
        assert lib.rb_probe_moments(0, same.ctypes.data, len(same), same.ctypes.data, sh.ctypes.data if ask else None) == 0   # in place
        held(same, want, 256, (name, "in place", ask), nan_rule=True)
        apart = np.zeros_like(sums)
        assert lib.rb_probe_moments(0, sums.ctypes.data, len(sums), apart.ctypes.data, sh.ctypes.data if ask else None) == 0
        held(apart, want, 256, (name, "out of place", ask), nan_rule=True)
        if ask:
            held(sh, want_share, 1, (name, "share"), nan_rule=True)
        else:
            assert (sh == 7).all()
    print(name, ":", nans, "NaN words compared under the NaN rule")


# ---- h. the chain: sums that overflow through bake, moments and blend
@pytest.mark.parametrize("samples", [65, 130])
@pytest.mark.parametrize("reach", [1e19, 1e20, 3e38])
def test_the_depth_chain_at_distances_whose_squares_overflow(reach, samples, monkeypatch):
    """under a bare sky every ray misses with t = 1e20f: r = min(t, max_distance), r r and then sum_r2 overflow to inf"""
    from tests.test_gpu_probe_visibility import assert_depth_equal, model_depth
    e = _engine(scenes.sky_only())
    try:
        grid = np.zeros(1, dtype=abi.PROBE_GRID)[0]
        grid["origin"], grid["step"], grid["counts"] = (-0.5, 0.25, 1.0), (1.0, 1.0, 1.0), (2, 1, 1)
        ppos = np.array([(-0.5, 0.25, 1.0), (0.5, 0.25, 1.0)], f32)
        want_sums, hits = model_depth(e, ppos, samples, 0, None, reach)
        assert (hits["t"] == f32(1e20)).all()
        for shape in ("lds", "readlane"):
            monkeypatch.setenv("RB_DEPTH_SHAPE", shape)
            sums = e.bake_probe_depth(ppos, samples, reach)
            assert_depth_equal(sums, want_sums, (reach, samples, shape))
        monkeypatch.delenv("RB_DEPTH_SHAPE")
        assert np.isinf(want_sums["texel"][:, :, 1]).any(), "no sum of r r overflowed"
        want_mom, want_share = probes.moments(sums)
        mom, share = engine.probe_moments(sums, device=0)
        nans = held(mom, want_mom, 256, "moments", nan_rule=True) + held(share, want_share, 1, "share", nan_rule=True)
        assert np.isinf(want_mom["texel"][:, :, 1]).any()
        # points in the cell, and points beyond the mean: as far out as the misses, and further
        co = C.record_base()[:2]
        rng = np.random.default_rng(97)
        pos = (ppos[0] + rng.uniform(0.02, 0.98, (65, 3)) * (1.0, 0.0, 0.0)).astype(f32)
        out = rng.normal(size=(32, 3))
        pos[1::2] += (out / np.sqrt((out * out).sum(1))[:, None] * 3e20).astype(f32)   # r r overflows: r = inf
        nrm = C.generic_normals(65, seed=101)
        floor = 0.125
        for kw in (dict(min_visibility=floor), dict(min_visibility=floor, wrap=False), dict()):
            got, want = visible_blend(grid, co, mom, pos, nrm, kw, ("chain", reach, samples))
        beyond = np.zeros(65, bool)
        beyond[1::2] = True
        kw = dict(min_visibility=floor, wrap=False)
        plain = probes.light(grid, co, pos, nrm)
        vis = probes.light_visible(grid, co, mom, pos, nrm, probes.visibility_params(**kw))
        assert (plain["weight"][beyond] > 0).all()
        if reach < 1e20:   # mean = 1e19, mean mean finite: var is 0 or inf, den = inf, ch = 0 or inf / inf -- vis is the floor either way
            # (the clamp leaves a far point one corner, the probe on its side; a texel without a sample is open)
            side = (pos[beyond, 0] > 0).astype(int)
            assert (np.abs(pos[beyond, 0]) > 1e18).all() and (plain["weight"][beyond] == 1).all()
            sampled = mom["texel"][side, probes.oct_texel((pos[beyond] - ppos[side]).astype(f32)), 2] == 1
            assert np.array_equal(vis["weight"][beyond], np.where(sampled, f32(floor), f32(1.0))) and sampled.sum() >= 8
        else:             # mean = 1e20: mean mean = inf = mean2, var = |inf - inf| is a NaN, so is den, den > 0 fails: ch = 1, open
            held(vis[beyond], plain[beyond], 4, "var a NaN: ch = 1")
        held(vis[~beyond], plain[~beyond], 4, "not beyond the mean: open")
        print("chain", reach, samples, ":", nans, "NaN words compared under the NaN rule")
    finally:
        e.close()


@pytest.mark.parametrize("shape", ["plain", "split"])
def test_the_projection_of_colours_whose_sums_overflow(shape, monkeypatch):
    """rb_update takes a sky colour of 3e38 (the boundary checks no colour): every ray misses and returns it, colour x Yj is
    finite, the ordered sums overflow to +-inf (and stay there: a finite term of the other sign makes no NaN).  k_sh_project and
    k_sh_project_split against probes.project over the device's own traced colours of the very records, under the NaN rule."""
    s = scenes.sky_only(sky=(3e38, 2e38, 1e38))
    e = _engine(s)
    try:
        rng = np.random.default_rng(103)
        pos = rng.normal(size=(65, 3)).astype(f32)
        nans = 0
        for samples in (16, 65):
            rays, seeds = engine.probe_rays_device(pos, samples, 0, device=0)
            col = e.trace_ray_records(rays, seeds)
            assert np.array_equal(col["sum"], np.tile(np.array([(3e38, 2e38, 1e38)], f32), (len(rays), 1))) and (col["weight"] == 1).all()
            want = probes.project(rays["dir"], np.concatenate([col["sum"], col["weight"][:, None]], axis=1), samples)
            monkeypatch.setenv("RB_PROBE_SHAPE", shape)
            got = e.bake_probes(pos, samples)
            monkeypatch.delenv("RB_PROBE_SHAPE")
            nans += held(got, want, 28, (shape, samples), nan_rule=True)
            assert np.isinf(want["sum"]).any()
        print("projection,", shape, ":", nans, "NaN words compared under the NaN rule")
    finally:
        e.close()
