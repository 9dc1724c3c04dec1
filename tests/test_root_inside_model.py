"""The rule by which k_trace goes past the root box's slab test (rb_device_intersect.hpp, RB_ROOT_INSIDE),
held against the slab test itself in numpy float32 (tests/_root_box_cases.py: isect_aabb as it is written, on the correctly
rounded 1 / d): wherever the rule says "known", the slab test says true.  About 10^5 seeded rays and the hand-made ones: origins
one ulp inside and outside of every face and exactly on it, on edges and at corners; direction components +-0, subnormal,
2^-100, +-inf, NaN and ordinary; the Cornell box, a box flat in one axis, extents of 2^60 and a box with an infinite bound.
No GPU: tests/test_gpu_root_inside.py runs the same cases through the device's own arithmetic."""
import numpy as np
import pytest

from tests import _root_box_cases as rb

F = np.float32


@pytest.fixture(scope="module")
def table():
    out = {}
    for name in rb.BOXES:
        o, d, bmin, bmax = rb.cases(name)
        out[name] = (o, d, bmin, bmax, rb.slab(o, d, bmin, bmax), rb.known(o, d, bmin, bmax))
    return out


@pytest.mark.parametrize("name", sorted(rb.BOXES))
def test_known_implies_the_slab_test(table, name):
    o, d, bmin, bmax, slab, known = table[name]
    bad = np.flatnonzero(known & ~slab)
    print(name, len(o), "rays,", int(known.sum()), "known,", int(slab.sum()), "pass the slab test")
    assert bad.size == 0, (name, o[bad[:4]], d[bad[:4]])


def test_the_cases_reach_what_they_are_for(table):
    total = sum(len(t[0]) for t in table.values())
    left = sum(int((~t[5]).sum()) for t in table.values())
    print(total, "rays,", left, "left to the slab test:", round(100.0 * left / total, 1), "%")
    assert 95_000 <= total <= 120_000
    assert left <= 0.6 * total                       # the rule answers at least 40 % of what is generated
    assert not table["flat"][5].any() and not table["open"][5].any()   # nothing strictly inside; an infinite bound
    for name in ("cornell", "huge"):
        o, d, bmin, bmax, slab, known = table[name]
        # every face from both sides and on it: one ulp inside, exactly on, one ulp outside, with and without a NaN
        for c in range(3):
            for b, inward in ((bmin[c], F(np.inf)), (bmax[c], F(-np.inf))):
                for v in (np.nextafter(b, inward), b, np.nextafter(b, -inward)):
                    assert (o[:, c] == v).sum() >= 50, (name, c, v)
        on_faces = ((o == bmin) | (o == bmax)).sum(axis=1)
        assert (on_faces == 2).sum() >= 100 and (on_faces == 3).sum() >= 12, name      # edges, corners
        assert (known & np.any(np.isinf(d), axis=1)).any() and (known & np.any(d == 0, axis=1)).any()
        assert (known & np.any(np.abs(d) == rb.SUB, axis=1)).any()
        nan = np.any(np.isnan(d), axis=1)
        assert nan.sum() >= 1000 and not known[nan].any()
        inside = np.all((o > bmin) & (o < bmax), axis=1)
        assert (inside & nan & ~slab).any(), name    # a direction of three NaNs inside the box fails the slab test
        assert (~known & slab).any() and (~known & ~slab).any(), name


def test_hand_made_rays():
    bmin, bmax = (np.array(b, F) for b in rb.BOXES["cornell"])
    mid = (bmin + bmax) / F(2.0)
    o = np.array([mid, mid, mid, [bmax[0], mid[1], mid[2]], np.nextafter(bmax, F(-np.inf)), np.nextafter(bmin, F(np.inf)), [0, 3, 5], mid], F)
    d = np.array([[0, 0, 0], [np.inf, -np.inf, 0.0], [np.nan, 0, 1], [1, 0, 0], [rb.SUB, 1, -1], [-1, -1, -1], [0, 0, -1], [np.nan] * 3], F)
    # the centre with a zero and with an infinite direction; one NaN component (fminf / fmaxf drop that axis: the test still
    # passes, the rule does not claim it); on a face, leaving; one ulp inside two corners; the camera of C2; three NaNs
    assert rb.known(o, d, bmin, bmax).tolist() == [True, True, False, False, True, True, False, False]
    assert rb.slab(o, d, bmin, bmax).tolist() == [True, True, True, True, True, True, True, False]
