"""The numpy model of the baked-probe consumers (renderbaby_amd/probes.py: coefficients, light, moments, light_visible) held to
the scalar transcription of DESIGN.md sections 19.1 and 20.1 (tests/_probe_scalar.py) on every degenerate input of
tests/_probe_edge_cases.py, on uint32 views, without a device.  This is the plain reference tests/test_gpu_probe_edges.py then
holds the device to: a vectorised select that evaluates a branch the definition never takes, and differs, is found here.

It also asserts, from the model alone, that every case is live: a hazard planted singly changes at least 16 points' outputs,
unless the definition says it must not show, and then the outputs are equal.  DESIGN.md section 20.6 has the tables.
"""
import numpy as np
import pytest

from renderbaby_amd import probes
from tests import _probe_edge_cases as C
from tests import _probe_scalar as S

f32, f64 = np.float32, np.float64
LIVE = 16


def same(model, scalar, width, where, nan_rule=False):
    bad, nans = C.mismatches(model, scalar, width, nan_rule)
    assert len(bad) == 0, (where, len(bad), bad[:5], np.asarray(model).view(f32).reshape(-1, width)[bad[:3]], np.asarray(scalar).reshape(-1, width)[bad[:3]])
    return nans


def no_nan(lit, where):
    assert not np.isnan(np.ascontiguousarray(lit).view(f32)).any(), (where, "the model's rb_lit holds a NaN: the blend could not be compared bit for bit")


def changed(a, b):
    return int((C.words(a, 4) != C.words(b, 4)).any(1).sum())


# ---- a. stage 1
def test_stage_1_on_every_pair_of_specials():
    sh = C.stage1_records()
    co = probes.coefficients(sh)
    nans = same(co, S.coefficients(sh.view(f32)), 28, "stage 1", nan_rule=True)
    print("stage 1:", nans, "NaN words of", co.view(f32).size)
    v = co.view(f32).reshape(22, 22, 28)
    sums, w = C.SPECIALS[:, None], C.SPECIALS[None, :]
    valid = (w > 0) & (w < np.inf)
    with np.errstate(all="ignore"):
        assert (np.isinf(v[:, :, 0]) & np.isfinite(sums) & valid & (w >= 1)).any(), "no sum * K_j overflowed"
        sub = (np.abs(v[:, :, 0]) > 0) & (np.abs(v[:, :, 0]) < C.FLT_MIN)
    assert (sub & valid).any(), "no quotient landed in the subnormal range"
    assert (v[:, 2:4, 27] == 1).all() and (v[:, :2, 27] == 0).all(), "a subnormal weight is a valid one, a zero is not"
    assert (C.words(co, 28)[~np.broadcast_to(valid, (22, 22)).reshape(-1)] == 0).all()


# ---- b. normals
NORMALS = C.normal_cases()


@pytest.mark.parametrize("name", list(NORMALS))
def test_normals(name):
    grid, co = C.valid_grid()
    nrm = NORMALS[name]
    pos = C.positions_inside(grid, len(nrm), seed=3)
    want = probes.light(grid, co, pos, nrm)
    no_nan(want, name)
    same(want, S.light(grid, co.view(f32), pos, nrm), 4, name)
    w = C.words(want, 4)
    with np.errstate(all="ignore"):
        len2 = ((nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]).astype(f32) + nrm[:, 2] * nrm[:, 2]).astype(f32)
    if name.startswith("len2 overflows"):
        assert np.isfinite(nrm).all() and np.isinf(len2).all() and (w == 0).all(), "finite components, len2 not finite: invalid, all-zero bits"
    elif name.startswith("len2 == 0"):
        assert (len2 == 0).all() and (nrm != 0).any(1).all()
    elif name == "len2 subnormal":
        assert ((len2 > 0) & (len2 < C.FLT_MIN)).all() and (want["weight"] > 0).all()
    elif name.startswith("guard"):
        assert np.isfinite(len2).all() and (want["weight"] > 0).all()   # (2^60 squared is 2^120: every one of them is lit)
    else:
        ok = np.isfinite(nrm).all(1) & (nrm != 0).any(1) & np.isfinite(len2)
        assert ok.sum() > 1000 and (w[~ok] == 0).all() and (want["weight"][ok] > 0).all()


@pytest.mark.parametrize("k", C.SCALES)
def test_a_scaled_normal_in_the_model(k):
    """The definition is invariant under nrm 2^k wherever no square of a component is rounded as a subnormal: for the lattice
    normals at every k (``_probe_edge_cases.lattice_normals`` has the argument), for arbitrary components at every k but -70,
    where what the definition says is what the model and the scalar transcription compute, and they agree."""
    for lattice in (True, False):
        grid, co, pos, nrm, big = C.scaled_pair(k, lattice)
        base, got = probes.light(grid, co, pos, nrm), probes.light(grid, co, pos, big)
        same(got, S.light(grid, co.view(f32), pos, big), 4, (k, lattice))
        n = changed(got, base)
        print("k =", k, "lattice" if lattice else "arbitrary", ":", n, "of 256 points differ from the unscaled normal's in the model")
        assert n == 0 or (k == -70 and not lattice), (k, lattice, n)
        assert (base["weight"] > 0).all()


# ---- c. coefficient records, one hazard to a grid
@pytest.mark.parametrize("hazard", list(C.record_hazards()))
@pytest.mark.parametrize("m", [65, 256])
def test_one_hazard_in_one_record(hazard, m):
    grid, pos, nrm, at_hazard, at_neighbour = C.record_points(m)
    base = C.record_base()
    co = base.copy()
    C.record_hazards()[hazard](co)
    clean, want = probes.light(grid, base, pos, nrm), probes.light(grid, co, pos, nrm)
    no_nan(want, hazard)
    same(want, S.light(grid, co.view(f32), pos, nrm), 4, hazard)
    assert changed(want, clean) >= LIVE, (hazard, changed(want, clean))
    assert at_neighbour.sum() == 14
    if hazard in C.SHOWS_AT_A_NEIGHBOUR:   # w_c = 0 * inf or 0 * NaN is a NaN, not 0: the corner is taken, W is a NaN and the point unlit
        assert (C.words(want[at_neighbour], 4) == 0).all() and (clean["weight"][at_neighbour] == 1).all()
    else:
        assert changed(want[at_neighbour], clean[at_neighbour]) == 0, "a record showed at a neighbouring probe: skipped entirely"
    if hazard == "weight -1.0":
        assert (C.words(want[:2], 4) == 0).all() and want["weight"][2] == 0.5, "W below 0, exactly 0 and above 0 along the edge"
        assert (C.words(want[at_hazard], 4) == 0).all()
    if hazard in ("weight -0.0", "weight qnan"):   # -0: the corner is skipped, and it is the only one; NaN: W > 0 fails
        assert (C.words(want[at_hazard], 4) == 0).all()
    if hazard == "weight inf":   # W = inf passes W > 0; E / W = inf / inf, a NaN, which max(., 0) turns into 0
        assert (C.words(want[at_hazard], 4)[:, :3] == 0).all() and np.isposinf(want["weight"][at_hazard]).all()


# ---- d. moments, one hazard to a map
def vis_model(grid, co, mm, pos, nrm, kw):
    return probes.light_visible(grid, co, mm, pos, nrm, probes.visibility_params(**kw))


def vis_scalar(grid, co, mm, pos, nrm, kw):
    return S.light(grid, co.view(f32), pos, nrm, (mm.view(f32), probes.visibility_params(**kw)))


_clean = {}


def clean_blend(m, k):
    if (m, k) not in _clean:
        grid, co, pos, nrm = C.moment_points(m)
        _clean[m, k] = vis_model(grid, co, C.benign_moments(8), pos, nrm, C.SETTINGS[k])
    return _clean[m, k]


@pytest.mark.parametrize("scope", ["one probe", "all probes"])
@pytest.mark.parametrize("hazard", list(C.moment_hazards()))
def test_one_hazard_in_the_maps(hazard, scope):
    m = 65
    grid, co, pos, nrm = C.moment_points(m)
    mm = C.benign_moments(8)
    C.moment_hazards()[hazard](mm, slice(C.MOMENT_PROBE, C.MOMENT_PROBE + 1) if scope == "one probe" else slice(None))
    for k, kw in enumerate(C.SETTINGS):
        want = vis_model(grid, co, mm, pos, nrm, kw)
        no_nan(want, (hazard, scope, kw))
        same(want, vis_scalar(grid, co, mm, pos, nrm, kw), 4, (hazard, scope, kw))
        n = changed(want, clean_blend(m, k))
        if hazard in C.NOT_SHOWN or C.setting_hides_the_maps(kw):
            assert n == 0, (hazard, scope, kw, n, "showed, and the definition says it must not")
        else:
            assert n >= LIVE, (hazard, scope, kw, n)


@pytest.mark.parametrize("kw", C.EXTRA_SETTINGS, ids=[f"{k}={C.name_of(v)}" for kw in C.EXTRA_SETTINGS for k, v in kw.items()])
def test_the_floor_and_the_bias_at_their_edges(kw):
    grid, co, pos, nrm = C.points_near_probes(65) if "min_visibility" in kw else C.moment_points(65)
    hidden = C.benign_moments(8)
    C.moment_hazards()["mean2 == mean mean"](hidden, slice(None))   # variance 0: beyond the mean vis is 0, and the floor decides
    for name, mm in (("benign", C.benign_moments(8)), ("variance 0", hidden), ("shut", C.shut_moments(8))):
        want = vis_model(grid, co, mm, pos, nrm, kw)
        no_nan(want, (name, kw))
        far = C.overflowing(grid, pos, nrm, kw.get("normal_bias", 0.0))
        assert not far.any(), "|n| <= 1: pos + n * bias stays finite for every bias the boundary accepts"
        same(want, vis_scalar(grid, co, mm, pos, nrm, kw), 4, (name, kw))
    if "min_visibility" in kw:   # every corner of ``shut`` has vis = 0: the floor is every weight's last factor
        assert (C.words(vis_model(grid, co, C.shut_moments(8), pos, nrm, {}), 4) == 0).all(), "a floor of 0 leaves nothing lit"
        assert (want["weight"] > 0).sum() >= LIVE, "the floor lit nothing"
        assert changed(want, vis_model(grid, co, C.shut_moments(8), pos, nrm, dict(min_visibility=1.0))) >= LIVE
        if kw["min_visibility"] < 1e-40:   # (tl wb) 2^-149 is 2^-149 or 0: W counts the corners that kept a weight
            assert set(np.unique(want["weight"] / C.SUB_MIN)) <= set(range(9)) and (want["weight"] == 0).any()
    elif abs(float(kw["normal_bias"])) > 1:   # the point is moved out of every probe's reach: r = inf or huge, vis = 0
        assert (want["weight"] == 0).sum() >= LIVE


# ---- e. the texel
@pytest.mark.parametrize("origin", [(0.0, 0.0, 0.0), (3.0, -5.0, 7.0)], ids=["origin 0", "origin 3 -5 7"])
@pytest.mark.parametrize("log2_scale", [0, 20, -20])
def test_the_texel_a_point_reads(origin, log2_scale):
    """W = 1 * vis = (mean2[T] / (mean2[T] + r r))^3 names the texel T that was read"""
    scale = 2.0 ** log2_scale
    grid, co = C.texel_grid(origin)
    mm = C.texel_map(scale)
    walk, labels = C.texel_vectors()
    vec = np.concatenate([walk * f32(scale), np.zeros((1, 3), f32), probes.oct_centres() * f32(scale)]).astype(f32)
    pos =(np.asarray(origin, f32) + vec).astype(f32)
    nrm = np.tile(np.array([(0.0, 0.0, 1.0)], f32), (len(pos), 1))
    kw = dict(wrap=False, min_visibility=0.0)
    want = vis_model(grid, co, mm, pos, nrm, kw)
    no_nan(want, "texel")
    same(want, vis_scalar(grid, co, mm, pos, nrm, kw), 4, ("texel", origin, log2_scale))
    # the expected texel from the model's own v = pos - P (position rounding moves it), by the scalar transcription
    v = (pos - np.asarray(origin, f32)).astype(f32)
    seen = set()
    axes = np.zeros((len(v), 3), int)   # per vector (tx, ty, lower half) by the scalar transcription
    var = mm["texel"][0, :, 1]
    with np.errstate(all="ignore"):
        for i, vi in enumerate(v):
            if not vi.any():
                assert want["weight"][i] == 1, "r == 0: open"
                continue
            axes[i] = S.texel_axes(vi)
            r = f32(np.sqrt(S.dot3(vi, vi)))
            ch = (var / (var + f32(r * r)).astype(f32)).astype(f32)   # the bound each of the 64 texels would give
            every = ((ch * ch).astype(f32) * ch).astype(f32)
            T = axes[i, 1] * 8 + axes[i, 0]
            assert want["weight"][i] == every[T] and (every == every[T]).sum() == 1, (i, vi, T, "the weight does not name the texel")
            seen.add(T)
    if origin == (0.0, 0.0, 0.0):   # v is the intended vector: every walk falls on both sides of its boundary, in its half
        C.boundaries_straddled(labels, axes[:len(walk), 0], axes[:len(walk), 1], axes[:len(walk), 2])
        assert seen == set(range(64)), "all 64 texels"
        hand = {tuple(h): probes.oct_texel([h])[0] for h in C.HAND_WRITTEN}
        assert hand[(1, 0, 0)] % 8 == 7 and hand[(3, 0, 0)] % 8 == 7, "px = 1 into column 7"
        assert hand[(0.1, 0.1, -0.0)] == hand[(0.1, 0.1, 0.0)] != hand[(0.1, 0.1, -0.8)]


# ---- f. far and clamped points
@pytest.mark.parametrize("counts", [(1, 1, 1), (2, 2, 2), (2, 1, 3)], ids=["1x1x1", "2x2x2", "2x1x3"])
def test_far_points(counts):
    grid, co = C.valid_grid(counts)
    n = len(co)
    pos, nrm, far = C.far_points(grid, 256)
    want = probes.light(grid, co, pos, nrm)
    no_nan(want, "far")
    same(want, S.light(grid, co.view(f32), pos, nrm), 4, ("far", counts))
    assert far.sum() == 128 and (want["weight"][far] > 0).all(), "the clamp is in contract: a far point takes the nearest cell's edge"
    mm = C.benign_moments(n)
    for kw in C.SETTINGS:
        vis = vis_model(grid, co, mm, pos, nrm, kw)
        sc = vis_scalar(grid, co, mm, pos, nrm, kw)
        same(vis[~far], sc[~far], 4, ("far, visible, the points in contract", counts, kw))
        bad, _ = C.mismatches(vis[far], sc[far], 4, nan_rule=True)
        print(counts, kw, "far points:", len(bad), "of", int(far.sum()), "differ between the model and the scalar transcription")


# ---- g. the moments
SUMS = C.moment_sums()


@pytest.mark.parametrize("name", list(SUMS))
def test_moments(name):
    sums = SUMS[name]
    mom, share = probes.moments(sums)
    s_mom, s_share = S.moments(sums.view(f32))
    nans = same(mom, s_mom, 256, name, nan_rule=True)
    nans += same(share, s_share, 1, name + ", share", nan_rule=True)
    print(name, ":", nans, "NaN words")
    cnt = sums["texel"][:, :, 2]
    valid = (cnt > 0) & np.isfinite(cnt)
    assert (C.words(mom, 256).reshape(-1, 64, 4)[~valid] == 0).all() and (mom["texel"][:, :, 2][valid] == 1).all()
    if name.startswith("ordered sums"):
        assert list(C.words(share, 1)[:3, 0]) == [0, 0, 0], "C == 0: the share is +0 whatever B is; C == inf: 0 / inf"
        assert np.isnan(share[3])
    if name == "back above count":
        assert (mom["texel"][:, :, 3][valid] > 1).all() and (share > 1).all()
