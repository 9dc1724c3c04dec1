"""tests/_tree_model.py on the host builders (rb_debug_own_tree -> fast_bvh_build, rb_debug_sphere_tree -> sphere_bvh_build):
their trees hold every invariant on every input that tests/test_gpu_tree_invariants.py gives the device builders, and the
checker rejects, with the reason meant, each single corruption of a read-back that passed.  No GPU."""
import numpy as np
import pytest

from renderbaby_amd import bvh
from tests import _tree_cases as K
from tests import _tree_model as M


def own_verdict(t, case, report=None, **changed):
    tris, _, idx, tri_count = K.mesh_case(case)
    a = {**t, **changed}
    return M.check_own_tree(a["nodes"], a["slots"], a["slot_meta"], a["root"], a["depth"], a["bmin"], a["bmax"], tris, idx, tri_count, report)


def sphere_verdict(t, spheres, **changed):
    a = {**t, **changed}
    return M.check_sphere_tree(a["nodes"], a["leaf"], a["ids"], a["root"], a["depth"], spheres)


@pytest.mark.parametrize("case", K.MESH_CASES)
def test_host_own_tree_holds_the_invariants(case):
    tris, nodes, idx, _ = K.mesh_case(case)
    t = bvh.debug_own_tree(tris, nodes, idx)
    assert t is not None
    report = {}
    assert own_verdict(t, case, report) is None
    print(f"{case}: depth {t['depth']}, need {report['need']}, excess {report['excess']}")


@pytest.mark.parametrize("layout,n", K.SPHERE_CASES)
def test_host_sphere_tree_holds_the_invariants(layout, n):
    s = K.sphere_case(layout, n)
    t = bvh.debug_sphere_tree(s)
    assert t is not None and sphere_verdict(t, s) is None      # (the axis rule included: sphere_bvh_build states the same rule)


def test_fa_is_never_below_its_bound_where_f32_underflows():
    """Edges of 1e-25: F_k = L^2 / 1e-6 is about 1e-44, where f32 is subnormal and a conversion to nearest lands below it (7
    steps of 2^-149 for 7.14); of 1e-30: about 1e-54, which converts to 0.  The builders step up there."""
    tris, nodes, idx, _ = K.mesh_case("count_1024")
    tris = tris.copy()
    for k, e in ((0, 1e-25), (1, 1e-30)):
        tris["v0"][k], tris["v1"][k], tris["v2"][k] = (0, 0, 0), (e, 0, 0), (0, e, 0)
    nodes, idx = bvh.build_canonical(tris)
    t = bvh.debug_own_tree(tris, nodes, idx)
    assert M.check_own_tree(t["nodes"], t["slots"], t["slot_meta"], t["root"], t["depth"], t["bmin"], t["bmax"], tris, idx, len(tris)) is None
    n = t["nodes"]
    fa = np.concatenate([n["left_fa"], n["right_fa"]])
    assert (fa > 0).all()                                       # no child's bound is 0 while a triangle below has an edge


# ------------------------------------------------------------------------ mutants ---
@pytest.fixture(scope="module")
def own():
    """a passing read-back with finite and infinite FA words: the soup with collinear triangles"""
    tris, nodes, idx, _ = K.mesh_case("degenerate")
    t = bvh.debug_own_tree(tris, nodes, idx)
    assert own_verdict(t, "degenerate") is None
    return t


@pytest.fixture(scope="module")
def balls():
    s = K.sphere_case("random", 1025)
    t = bvh.debug_sphere_tree(s)
    assert sphere_verdict(t, s) is None
    return t, s


def _reachable(t):
    order, why = M._walk(t["root"], len(t["nodes"]), lambda i: (t["nodes"]["left"][i], t["nodes"]["right"][i]), lambda r: bool(int(r) & M.LEAF))
    assert why is None
    return order


def _step(x, up):
    return np.nextafter(np.float32(x), np.float32(np.inf if up else -np.inf))


def _patched(t, i, **fields):
    nodes = t["nodes"].copy()
    for k, v in fields.items():
        nodes[k][i] = v
    return nodes


def test_mutant_own_box_one_ulp_inwards(own):
    n = own["nodes"]
    for i in _reachable(own)[:5]:
        lo, hi = n["lmin"][i].copy(), n["rmax"][i].copy()
        lo[1], hi[2] = _step(lo[1], True), _step(hi[2], False)
        assert "box" in own_verdict(own, "degenerate", nodes=_patched(own, i, lmin=lo))
        assert "box" in own_verdict(own, "degenerate", nodes=_patched(own, i, rmax=hi))


def test_mutant_fa_one_ulp_lower(own):
    n = own["nodes"]
    picked = [i for i in _reachable(own) if np.isfinite(n["left_fa"][i]) and n["left_fa"][i] > 0][:8]
    assert picked
    for i in picked:
        why = own_verdict(own, "degenerate", nodes=_patched(own, i, left_fa=_step(n["left_fa"][i], False)))
        assert why and "FA" in why and "below" in why, why


def test_mutant_fa_finite_where_inf_is_due(own):
    n = own["nodes"]
    picked = [i for i in _reachable(own) if np.isinf(n["right_fa"][i])][:4]
    assert picked
    for i in picked:
        for v in (1.5e5, 3.0e38):
            assert "finite where +inf is due" in own_verdict(own, "degenerate", nodes=_patched(own, i, right_fa=np.float32(v)))


def test_mutant_two_slots_equal(own):
    slots = own["slots"].copy()
    slots[7] = slots[300]
    assert "twice" in own_verdict(own, "degenerate", slots=slots)


def _leaf_holding(t, pos):
    """(node, field) of the leaf reference that holds position `pos`"""
    n = t["nodes"]
    for i in _reachable(t):
        for f in ("left", "right"):
            r = int(n[f][i])
            if r & M.LEAF and (r & 0x0FFFFFFF) <= pos < (r & 0x0FFFFFFF) + ((r >> 28) & 7) + 1:
                return i, f
    raise AssertionError(pos)


def test_mutant_slot_dropped_with_the_leaf_shortened(own):
    """the second triangle of a two-triangle leaf leaves `slots`; the leaf is shortened and every later leaf moved up, so the
    tree is sound in itself and only the comparison with the valid slots can tell"""
    nodes = own["nodes"].copy()
    i, f = next((i, f) for i in _reachable(own) for f in ("left", "right") if int(nodes[f][i]) >> 28 == 0x9)
    gone = (int(nodes[f][i]) & 0x0FFFFFFF) + 1
    nodes[f][i] = int(nodes[f][i]) & ~(1 << 28)
    for g in ("left", "right"):
        later = ((nodes[g] & M.LEAF) != 0) & ((nodes[g] & 0x0FFFFFFF) > gone)
        nodes[g][later] -= 1
    why = own_verdict(own, "degenerate", slots=np.delete(own["slots"], gone), nodes=nodes)
    assert "1 missing" in why, why


def test_mutant_leaf_overlaps_its_neighbour(own):
    i, f = _leaf_holding(own, 500)
    r = int(own["nodes"][f][i])
    assert "overlaps its neighbour" in own_verdict(own, "degenerate", nodes=_patched(own, i, **{f: r - 1}))


def test_mutant_node_referenced_twice(own, balls):
    n = own["nodes"]
    i = next(i for i in _reachable(own) if not int(n["left"][i]) & M.LEAF)
    assert "referenced twice" in own_verdict(own, "degenerate", nodes=_patched(own, i, right=n["left"][i]))
    t, s = balls
    ref = t["nodes"]["ref"][t["root"]].copy()
    assert not int(ref[0]) & M.LEAF
    ref[3] = ref[0]
    assert "referenced twice" in sphere_verdict(t, s, nodes=_patched(t, t["root"], ref=ref))


def test_mutant_depth_reduced(own, balls):
    """The sphere tree's depth is an equality: one less is rejected.  The own tree's builders all report two more than the walk can
    need (printed by the tests above), so one less than reported still covers the stack and is no defect; what is rejected is a
    depth one below the need."""
    report = {}
    assert own_verdict(own, "degenerate", report) is None and report["excess"] == 2
    assert own_verdict(own, "degenerate", depth=report["need"]) is None
    assert "does not cover" in own_verdict(own, "degenerate", depth=report["need"] - 1)
    t, s = balls
    assert "is not 3 x" in sphere_verdict(t, s, depth=t["depth"] - 1)
    assert "is not 3 x" in sphere_verdict(t, s, depth=t["depth"] - 3)


def test_mutant_mesh_bounds_shrunk(own):
    for key, a, up in (("bmin", 0, True), ("bmax", 2, False)):
        b = own[key].copy()
        b[a] = _step(b[a], up)
        assert "mesh bounds" in own_verdict(own, "degenerate", **{key: b})


def test_mutant_sphere_box_one_ulp_inwards(balls):
    t, s = balls
    for i in range(min(4, len(t["nodes"]))):
        for k in (0, 2):
            h = t["nodes"]["hy"][i].copy()
            h[k] = _step(h[k], False)
            why = sphere_verdict(t, s, nodes=_patched(t, i, hy=h))
            assert why and f"node {i} child {k} axis 1" in why, why
    # far enough inwards to leave a sphere outside: the containment itself
    h = t["nodes"]["hx"][0].copy()
    h[0] *= np.float32(0.999)
    assert "does not contain" in sphere_verdict(t, s, nodes=_patched(t, 0, hx=h))
    h = t["nodes"]["hx"][0].copy()
    h[0] *= np.float32(1.01)
    assert "loose" in sphere_verdict(t, s, nodes=_patched(t, 0, hx=h))


def test_mutant_ids_swapped_without_the_leaf_records(balls):
    t, s = balls
    ids = t["ids"].copy()
    ids[[3, 700]] = ids[[700, 3]]
    assert "leaf record 3 " in sphere_verdict(t, s, ids=ids)
    ids = t["ids"].copy()
    ids[5] = ids[6]
    assert "permutation" in sphere_verdict(t, s, ids=ids)


def test_mutant_sphere_leaf_of_17(balls):
    """A leaf reference has four bits for count - 1: the builders' own formula for 17 spheres carries into the leaf bit and reads
    as one sphere, so the seventeenth (taken from the neighbour) and fifteen more are in no leaf: the tiling names it."""
    t, s = balls
    nodes = t["nodes"]
    for i in range(len(nodes)):
        ref = nodes["ref"][i].copy()
        full = [k for k in range(3) if int(ref[k]) != M.NONE and int(ref[k]) & M.LEAF and (int(ref[k]) >> 27) & 0xF == 15
                and int(ref[k + 1]) != M.NONE and int(ref[k + 1]) & M.LEAF]
        if full:
            k = full[0]
            first, nxt = int(ref[k]) & 0x07FFFFFF, int(ref[k + 1])
            ref[k] = (0x80000000 | ((17 - 1) << 27) | first) & 0xFFFFFFFF
            ref[k + 1] = 0x80000000 | ((((nxt >> 27) & 0xF) - 1) << 27) | ((nxt & 0x07FFFFFF) + 1)
            why = sphere_verdict(t, s, nodes=_patched(t, i, ref=ref))
            assert why and "leaves a gap" in why, why
            return
    raise AssertionError("no leaf of 16 spheres beside another leaf in this tree")


def test_mutant_axes_name_the_wrong_axis(balls):
    t, s = balls
    axes = int(t["nodes"]["axes"][t["root"]])
    for wrong in (axes ^ 1 if (axes & 3) != 2 else axes ^ 2, (axes & ~0xC) | ((((axes >> 2) & 3) + 1) % 3) << 2):
        why = sphere_verdict(t, s, nodes=_patched(t, t["root"], axes=wrong))
        assert why and "names axis" in why, why
    # without the axis rule the split order itself tells: the centres are not ordered along another axis
    a = dict(t, nodes=_patched(t, t["root"], axes=(axes & ~3) | ((axes & 3) + 1) % 3))
    why = M.check_sphere_tree(a["nodes"], a["leaf"], a["ids"], a["root"], a["depth"], s, axis_rule=False)
    assert why and "split order" in why, why
