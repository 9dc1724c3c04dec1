"""Conservativeness of the triangle sift's pass 1 ("The triangle sift"), on the numpy model of it
(renderbaby_amd/tri_filter_model.py) against the float32 triangle test of tools/margin_check.py: no hit that test ACCEPTS may be
missing from a candidate mask.  Zero, not few.  CPU only.

 * that tool's grazing-heavy generator, three regimes, 1.2 M rays, each pair (triangle, ray) with a group and a region of its own;
   the same again 16 times as large (a power of two: the f32 edges scale exactly), where the triangles are beyond the range the
   determinant-floor cap is claimed for, as C2's walls are;
 * a miniature of tools/margin_search.py's climb, aimed at (pass 1 rejects and the reference accepts): the slack of the three
   compares is driven down over accepted hits;
 * origins on a triangle's own plane and on its edges;
 * direction components that are tiny normal floats or subnormals, whose reciprocals are finite and enormous or infinite: the
   products of a slab value would overflow one by one, so such a lane must take every slot;
 * the Cornell box's table: rays from inside the box, from the camera and from under the light quad's 0.01 gap;
 * every ray family of tests/_edge_scenes.py against that scene's table, and tests/_root_box_cases.py's origins and directions
   (+-0, subnormal, infinite and NaN components; faces, edges and corners of the box) against the Cornell table;
 * the tables of tests/_tri_filter_cases.py's named scenes -- groups of 1 to 4, open groups between closed ones, dead slots, a
   list that starts at slot 7, scenes far from the origin, 2^-10 and 2^10 as large -- under the rays aimed at their triangles' edges
   and vertices on grazing rays, and two random families.  The conditions that keep the aimed family from being empty are checked
   here, by the reference test alone.

The constants pass 1 rests on are pinned as tests/test_margin_bound.py pins the chunked walk's."""
import os

import numpy as np
import pytest

from renderbaby_amd import scenes
from renderbaby_amd import tri_filter_model as M
from tests import _edge_scenes, _root_box_cases
from tests import _tri_filter_cases as T
from tests._tri_filter_cases import MC, F32, ROOT, _tool, _prepared, _scene_table, _hold, _unit, tiny_component_rays


def _pairs_keep(o, d, v0, e1, e2):
    """every pair's own group and region (the triangle's box and the ray's origin) -> (accepted, keep, closed, detail)"""
    grp = M.make_group(np.stack(v0)[None], np.stack(e1)[None], np.stack(e2)[None])
    oo = np.stack(o).astype(np.float64)
    reg = M.make_region(grp, oo, oo)
    keep, det = M.pass1(grp, reg, o, d, detail=True)
    ok, _, _ = MC.mt32(o, d, v0, e1, e2)
    return ok, keep, grp["closed"], det


# ------------------------------------------------------------------------------- the constants ---
def test_constants_are_the_sources():
    src = open(os.path.join(ROOT, "renderbaby_amd", "csrc", "rb_tri_filter.hpp")).read()
    for k, v in (("kSiftKS", "24.0f"), ("kSiftKP", "12.0f"), ("kSiftKT", "11.0f"), ("kSiftKD", "16.0f")):
        assert f"{k} = {v} * 5.9604645e-8f * 1.01f" in src, k
    assert "constexpr double kSiftSlabUlps = 8.0;" in src and "kSiftEdgeMax = 1e9, kSiftSpMax = 1e12;" in src
    assert "constexpr double kSiftAlphaMax = 1e-3;" in src and "constexpr double kSiftBoxGrow = 1.05;" in src
    assert (M.KS, M.KP, M.KT, M.KD) == tuple(F32(c) * F32(5.9604645e-8) * F32(1.01) for c in (24.0, 12.0, 11.0, 16.0))
    dev = open(os.path.join(ROOT, "renderbaby_amd", "csrc", "rb_device_intersect.hpp")).read()
    assert "constexpr float kSiftFMax = 1.5e5f;" in dev and "0.001f - __builtin_fmaf(kt, f, kd)" in dev
    assert dev.count("p.sift_rmax, 5)") == 3 and "r.rmax = static_cast<float>(1e38 / reach);" in src   # the bound the certification's overflow line assumes
    kern = open(os.path.join(ROOT, "renderbaby_amd", "csrc", "rb_kernels.hip")).read()
    assert "kSiftFMax == kChunkFMax && kSiftKS == kChunkKS && kSiftKP == kChunkKP && kSiftKT == kChunkKT && kSiftKD == kChunkKD" in kern


def test_the_sift_s_own_inequalities_are_certified():
    # tools/margin_certify.py, the sift's section: Sp per launch, the fma-form slab values on an approximate reciprocal, the
    # compare against 0.001 - dt, the cone's dot product and the reciprocal in f -- comparisons between rationals, with the
    # constants the sources and the model carry
    mcert = _tool("margin_certify")
    assert len(mcert.sift_checks) == 9
    for name, need, has in mcert.sift_checks:
        assert need <= has, (name, float(need), float(has))
    assert mcert.SLAB_ULPS == M.SLAB_ULPS == 8.0 and mcert.e_rcp == 2 * mcert.u


# --------------------------------------------------------------------------- the generator's rays ---
@pytest.mark.parametrize("scale", [1.0, 16.0])
@pytest.mark.parametrize("regime", ["floor", "grazing", "steep"])
def test_generator(regime, scale):
    rng = np.random.default_rng([20241004, ["floor", "grazing", "steep"].index(regime), int(scale)])
    n = 200_000
    o, d, v0, e1, e2, _, _ = MC.batch(rng, n, regime)
    s = F32(scale)
    o, v0, e1, e2 = (tuple(c * s for c in a) for a in (o, v0, e1, e2))
    ok, keep, closed, _ = _pairs_keep(o, d, v0, e1, e2)
    print(f"{regime} x{scale:g}: {int(ok.sum())} accepted of {n}, {int((~keep).sum())} rejected by pass 1, {int(closed.sum())} closed groups")
    assert closed.mean() > 0.9
    assert ok.sum() > n // 100, "the generator no longer hits"
    assert not (ok & ~keep).any(), ("accepted hits missing from the mask", int((ok & ~keep).sum()))
    if regime == "steep":
        # not a measure of quality, a guard against a pass 1 that keeps everything: the generator aims at barycentrics in
        # [-0.3, 1.3]^2, so 1 - 1 / 2.56 = 61 % of the rays pass outside the edges' parallelogram; a fifth of the misses is far below that
        assert (~keep[~ok]).mean() > 0.2, "pass 1 rejects next to nothing: the test says little"


# ------------------------------------------------------------------------------------ the climb ---
def test_climb_towards_a_rejected_accepted_hit():
    rng = np.random.default_rng(20241005)
    n = 30_000
    parts = [MC.batch(rng, n, r) for r in ("floor", "grazing", "steep")]
    o, d, v0, e1, e2 = (tuple(np.concatenate([p[k][i] for p in parts]) for i in range(3)) for k in range(5))

    def slack(o, d):
        ok, keep, closed, det = _pairs_keep(o, d, v0, e1, e2)
        with np.errstate(all="ignore"):
            s = np.fmin(det["tf"] - det["tn"], det["tf"] - det["thr"]) / (np.abs(det["tf"]) + np.abs(det["tn"]) + F32(1e-30))
        return ok, keep, np.where(ok & closed & np.isfinite(s), s, np.inf)

    ok, keep, best = slack(o, d)
    assert not (ok & ~keep).any()
    for it in range(40):
        step = 10.0 ** rng.uniform(-7.5, -2.5, len(best))
        o2 = tuple((c.astype(np.float64) * (1.0 + step * rng.normal(size=len(best)))).astype(F32) for c in o)
        d2 = tuple((c.astype(np.float64) + step * rng.normal(size=len(best))).astype(F32) for c in d)
        ln = np.sqrt(MC.dot32(d2, d2))
        d2 = tuple(c / ln for c in d2)
        ok2, keep2, s2 = slack(o2, d2)
        assert not (ok2 & ~keep2).any(), ("round", it, int((ok2 & ~keep2).sum()))
        better = s2 < best
        o = tuple(np.where(better, a, b) for a, b in zip(o2, o))
        d = tuple(np.where(better, a, b) for a, b in zip(d2, d))
        best = np.where(better, s2, best)
    print("smallest relative slack of an accepted hit after the climb:", float(best.min()))
    assert best.min() > 0.0


# ------------------------------------------------------------ origins on the plane and on the edges ---
@pytest.mark.parametrize("where", ["plane", "edge"])
def test_origins_on_the_triangle(where):
    rng = np.random.default_rng([7, where == "edge"])
    n = 200_000
    _, _, v0, e1, e2, _, _ = MC.batch(rng, n, "steep")
    a, b = rng.uniform(-0.2, 1.2, n), rng.uniform(-0.2, 1.2, n)
    if where == "edge":
        k = rng.integers(0, 3, n)
        a, b = np.where(k == 0, 0.0, a), np.where(k == 1, 0.0, np.where(k == 2, 1.0 - a, b))
    o = tuple((v0[i].astype(np.float64) + a * e1[i] + b * e2[i]).astype(F32) for i in range(3))
    d = rng.normal(size=(3, n))
    flat = rng.random(n) < 0.5       # half of the directions nearly in the plane
    nrm = np.cross(np.stack(e1).T.astype(np.float64), np.stack(e2).T.astype(np.float64)).T
    nrm /= np.maximum(np.linalg.norm(nrm, axis=0), 1e-300)
    d = np.where(flat, d - nrm * (d * nrm).sum(0) * (1.0 - 10.0 ** rng.uniform(-8, -1, n)), d)
    d = tuple((d[i] / np.linalg.norm(d, axis=0)).astype(F32) for i in range(3))
    ok, keep, closed, _ = _pairs_keep(o, d, v0, e1, e2)
    print(f"{where}: {int(ok.sum())} accepted, {int((~keep).sum())} rejected by pass 1")
    assert not (ok & ~keep).any()


# ------------------------------------------------------------------------------------- scenes ---
def test_direction_components_that_are_tiny_normal_floats():
    # 1 / d_k is finite and enormous: c r or o r overflows on its own where their difference does not.  Such a lane must take
    # every slot (sift_rmax), not an infinity for a slab value.  The rays a review found first, then the sweep.
    tb = _scene_table(scenes.cornell(64, 48, 4, 8))
    o = np.array([[0, 5, -3], [0, 5, -3], [0.5, 5.5, -3]], F32)
    d = np.array([[1, 1.2e-38, 0], [1, -1.2e-38, 0], [0, 1.2e-38, -1]], F32)
    cand, acc = _hold(tb, o, d, "the three rays")
    assert acc.sum() == 3 and acc[9, 0] and acc[9, 1] and acc[5, 2]
    o, d = tiny_component_rays()
    cand, acc = _hold(tb, o, d, "tiny components, as drawn")
    assert acc.sum() > len(o) // 4, "the sweep no longer hits"
    _hold(tb, o, _unit(d), "tiny components, normalised")


def test_cornell_table():
    scene = scenes.cornell(64, 48, 4, 8)
    tb = _scene_table(scene)
    groups = tb[0]
    assert [c for _, c, _ in groups] == [2] * 6 and all(g["closed"][0] for _, _, g in groups), "six planar quads"
    rng = np.random.default_rng(11)
    b, n = scenes.BOX, 60_000
    lo, hi = np.array([b["x0"], b["y0"], b["z0"]]), np.array([b["x1"], b["y1"], b["z1"]])
    inside = (lo + rng.random((n, 3)) * (hi - lo)).astype(F32)
    cand, acc = _hold(tb, inside, _unit(rng.normal(size=(n, 3))), "inside the box")
    assert cand.sum(0).mean() < 4.0, "the box test no longer sifts the Cornell box"
    cam = np.tile(np.array([0, 3, 5], F32), (n, 1))
    _hold(tb, cam, _unit(np.column_stack([rng.uniform(-0.6, 0.6, n), rng.uniform(-0.6, 0.6, n), -np.ones(n)])), "from the camera")
    # from the walls themselves (a bounce's origin: on a wall's plane, within rounding), every direction
    on = inside.copy()
    axis, side = rng.integers(0, 3, n), rng.integers(0, 2, n)
    on[np.arange(n), axis] = np.where(side == 0, lo[axis], hi[axis]).astype(F32)
    cand, _ = _hold(tb, on, _unit(rng.normal(size=(n, 3))), "from the walls")
    # under the light quad, 0.01 below the ceiling: upward rays through the gap, and rays that start inside it
    under = np.column_stack([rng.uniform(-1.2, 1.2, n), rng.uniform(0.3, 5.7399, n), rng.uniform(-4.2, -1.8, n)]).astype(F32)
    up = _unit(np.column_stack([rng.normal(size=n) * 0.3, np.abs(rng.normal(size=n)) + 0.05, rng.normal(size=n) * 0.3]))
    cand, acc = _hold(tb, under, up, "under the light")
    assert acc[10:12].any(), "no ray hits the light quad"
    gap = under.copy()
    gap[:, 1] = rng.uniform(5.74, 5.75, n).astype(F32)
    _hold(tb, gap, _unit(rng.normal(size=(n, 3))), "inside the gap")


@pytest.mark.parametrize("name", sorted(_root_box_cases.BOXES))
def test_root_box_families(name):
    o, d, _, _ = _root_box_cases.cases(name)
    tb = _scene_table(scenes.cornell(64, 48, 4, 8))
    _hold(tb, o, d, f"{name}, as drawn")          # directions with +-0, subnormal, infinite and NaN components, not normalised
    _hold(tb, o, _unit(d), f"{name}, normalised")


def test_edge_scene_families():
    scene = _edge_scenes.texture_edges_scene()
    v0, e1, e2 = _prepared(scene)
    fams = [("aimed", _edge_scenes.aimed_rays(scene)[:2]), ("threshold", _edge_scenes.threshold_rays(scene)[:2]),
            ("far ground", _edge_scenes.far_ground_rays())]
    for first in range(0, len(v0), M.MAX_SLOTS):      # the wall's triangles in lists a node could hold
        sl = slice(first, first + M.MAX_SLOTS)
        sub = scenes.Scene(scene.uniforms, scene.spheres, scene.lights, scene.meshes, scene.bvh_nodes, scene.bvh_indices[sl],
                           scene.bvh_triangles, scene.uvs, scene.textures, scene.name)
        for what, (o, d) in fams:
            cand, acc = _hold(_scene_table(sub, o), np.asarray(o, F32), _unit(d), f"{what}, slots {first}..")
            if what == "aimed":
                # along -z exactly, two reciprocals are infinite and their axes say nothing (inf - inf): every quad of the wall
                # stays.  A hair off the axis the same rays are sifted.
                assert acc.any() and cand.all()
                cand, acc = _hold(_scene_table(sub, o), np.asarray(o, F32), _unit(np.asarray(d, F32) + F32([1e-3, 2e-3, 0])), "aimed, tilted")
                assert acc.any() and cand.sum(0).mean() < 0.25 * cand.shape[0], "the wall's quads are not sifted"


# ------------------------------------------------------------------------- the named tables ---
def test_every_group_size_occurs_and_every_table_sifts():
    sizes, blocks = set(), {}
    for name in T.tables():
        (groups, reg, tri), (first, end) = T.table_of(name)
        assert sum(c for _, c, _ in groups) == end - first == len(tri[0])
        closed = [c for _, c, g in groups if g["closed"][0]]
        assert int(tri[3].sum()) >= M.MIN_LIVE and closed and bool(reg["on"][0]), (name, "the model says this list does not sift")
        sizes |= set(closed)
        blocks[name] = (end - first + 31) // 32
    assert sizes == {1, 2, 3, 4}, sizes
    assert [blocks[n] for n in T.SOUPS] == [2, 2, 4, 4]
    groups, _, tri = T.table_of("mixed")[0]
    kinds = [bool(g["closed"][0]) for _, _, g in groups]
    assert kinds[0] and kinds[-1] and not all(kinds[1:-1]) and int((~tri[3]).sum()) == 1, "open groups between closed ones, one dead slot"
    (_, _, tri), (first, end) = T.table_of("offset")
    assert (first, end) == (7, 47) and int((~tri[3]).sum()) == 3


@pytest.mark.parametrize("name", T.tables())
def test_named_tables(name):
    tb, _ = T.table_of(name)
    _, reg, tri = tb
    rng = np.random.default_rng([36, T.tables().index(name)])
    o, d, slot, outside = T.aimed_rays(tri, reg, rng)
    assert len(o) <= T.MAX_AIMED and tri[3][slot].all()
    lo, hi = reg["lo"][:, 0], reg["hi"][:, 0]
    assert ((o > lo) & (o < hi)).all(), "an aimed origin outside the region"
    accepts, refuses, outside_share = T.aimed_census(tri, o, d, slot, outside)
    print(f"{name}: {len(o)} aimed rays; of the (ray, aimed slot) pairs the reference accepts {accepts:.1%}, refuses {refuses:.1%}; "
          f"{outside_share:.2%} of the accepted have P outside the exact triangle")
    assert accepts >= 0.10 and refuses >= 0.10 and outside_share >= 0.01, (name, accepts, refuses, outside_share)
    cand, _ = _hold(tb, o, d, f"{name}, aimed")
    assert not cand.all(), "pass 1 rejects nothing of the aimed rays"
    cand, acc = _hold(tb, *T.region_rays(reg, 20_000, rng), f"{name}, inside the region")
    assert acc.any() and cand.mean() < 0.5, "the box test no longer sifts this table"
    _hold(tb, *T.surface_rays(tri, 20_000, rng), f"{name}, from the triangles")
    _hold(tb, *T.edge_rays(tri, reg, 10_000, rng), f"{name}, along the edges")


def test_rays_along_the_edges_of_bent_groups_see_the_sign_of_s():
    # what tests/test_gpu_tri_filter.py's comparison of the device's masks with the model's rests on for `lb = |d . n| - s`: on
    # the bent table a model with the sign turned gives other masks in a large share of the bits of this family (on planar
    # groups, s = 2e-6, in a few of a million), so a kernel with that sign cannot stay within 1 % of the model there
    import types
    src = open(M.__file__).read()
    assert src.count('lb = np.abs(y) - grp["s"]') == 1
    turned = types.ModuleType("tri_filter_model_turned")
    exec(compile(src.replace('lb = np.abs(y) - grp["s"]', 'lb = np.abs(y) + grp["s"]'), turned.__name__, "exec"), turned.__dict__)
    (groups, reg, tri), _ = T.table_of("bent")
    assert [c for _, c, _ in groups] == [2] * 6 and all(8e-4 < float(g["s"][0]) < 1e-3 for _, _, g in groups)
    o, d = T.edge_rays(tri, reg, 10_000, np.random.default_rng(36))
    ot, dt = np.ascontiguousarray(o.T), np.ascontiguousarray(d.T)
    share = float((M.candidate_mask(groups, reg, ot, dt) != turned.candidate_mask(groups, reg, ot, dt)).mean())
    print(f"bent, along the edges: {len(o)} rays, the sign of s turned changes {share:.1%} of the bits")
    assert len(o) > 4000 and share > 0.10
