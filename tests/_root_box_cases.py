"""The root box of the single-node walk in numpy float32: the slab test as isect_aabb writes it (rb_device_intersect.hpp) on the
correctly rounded 1 / d, the rule by which k_trace goes past it (origin strictly inside a finite box, no NaN in the direction),
and the cases both tests of it share -- tests/test_root_inside_model.py on the CPU, tests/test_gpu_root_inside.py against the
device's own arithmetic (rb_debug_root_box).  Everything is seeded; nothing here needs a GPU."""
import numpy as np

from renderbaby_amd import scenes

F = np.float32
INF, NAN = F(np.inf), F(np.nan)
SUB = F(2.0 ** -140)   # a subnormal: its reciprocal overflows to infinity


def slab(o, d, bmin, bmax):
    """isect_aabb(o, 1 / d, bmin, bmax) for n rays (o, d: [n, 3] float32).  fminf / fmaxf hand back the other operand for a
    NaN (np.fmin / np.fmax); the last compare is false for one."""
    o, d = np.asarray(o, F), np.asarray(d, F)
    with np.errstate(all="ignore"):
        inv = F(1.0) / d
        t0 = (np.asarray(bmin, F) - o) * inv
        t1 = (np.asarray(bmax, F) - o) * inv
        lo, hi = np.fmin(t0, t1), np.fmax(t0, t1)
        tmin = np.fmax(np.fmax(lo[:, 0], lo[:, 1]), lo[:, 2])
        tmax = np.fmin(np.fmin(hi[:, 0], hi[:, 1]), hi[:, 2])
        return tmax >= np.fmax(tmin, F(0.0))


def known(o, d, bmin, bmax):
    """the rule: True where the slab test's answer is known to be true without running it"""
    o, d, bmin, bmax = np.asarray(o, F), np.asarray(d, F), np.asarray(bmin, F), np.asarray(bmax, F)
    with np.errstate(invalid="ignore"):
        inside = np.all((o > bmin) & (o < bmax), axis=1)
    return inside & ~np.any(np.isnan(d), axis=1) & bool(np.all(np.isfinite(bmin)) and np.all(np.isfinite(bmax)))


_B = scenes.BOX
BOXES = {
    "cornell": ((_B["x0"], _B["y0"], _B["z0"]), (_B["x1"], _B["y1"], _B["z1"])),
    "huge": ((-2.0 ** 60, -2.0 ** 60, -2.0 ** 60), (2.0 ** 60, 2.0 ** 60, 2.0 ** 60)),
    "flat": ((-1.0, 2.0, -1.0), (1.0, 2.0, 1.0)),             # nothing is strictly inside
    "open": ((-1.0, -np.inf, -1.0), (1.0, 3.0, 1.0)),         # an infinite bound: the rule must not apply
}
COUNTS = {"cornell": 46000, "huge": 46000, "flat": 4000, "open": 4000}


def _directions(rng, n):
    special = np.array([0.0, -0.0, SUB, -SUB, 2.0 ** -100, -2.0 ** -100, INF, -INF, NAN], F)
    d = rng.uniform(-1.0, 1.0, (n, 3)).astype(F)
    pick = rng.random((n, 3)) < 0.3
    d[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
    return d


def _interior(rng, n, bmin, bmax):
    """origins drawn inside the box (a flat or open axis: around its finite bound)"""
    lo = np.where(np.isfinite(bmin), bmin, F(-8.0)).astype(np.float64)
    hi = np.where(np.isfinite(bmax), bmax, F(8.0)).astype(np.float64)
    return (lo + rng.random((n, 3)) * (hi - lo)).astype(F)


def cases(name):
    """(o, d, bmin, bmax) of box `name`: 70 % of the origins drawn inside, the rest with one, two or three components (faces,
    edges, corners) put one ulp inside a bound, exactly on it or one ulp outside; a third of the direction components special
    (+-0, subnormal, 2^-100, +-inf, NaN); the hand-made rays in front."""
    bmin, bmax = (np.array(b, F) for b in BOXES[name])
    n = COUNTS[name]
    rng = np.random.default_rng([0x29, sorted(BOXES).index(name)])
    o = _interior(rng, n, bmin, bmax)
    d = _directions(rng, n)
    on = np.flatnonzero(rng.random(n) < 0.3)
    for i in on:
        for c in rng.permutation(3)[: rng.integers(1, 4)]:
            b, other = (bmin[c], bmax[c]) if rng.random() < 0.5 else (bmax[c], bmin[c])
            if not np.isfinite(b):
                continue
            out = -INF if (other > b or (other == b and b == bmin[c] and rng.random() < 0.5)) else INF   # away from the other bound
            o[i, c] = (np.nextafter(b, -out), b, np.nextafter(b, out))[rng.integers(0, 3)]
    mid = ((bmin.astype(np.float64) + bmax) / 2).astype(F)
    mid = np.where(np.isfinite(mid), mid, F(0.0))
    hand_d = np.array([[0, 0, 0], [-0.0, 0, -0.0], [1, 0, 0], [NAN, 1, 0], [0, NAN, 0], [0, 1, NAN], [INF, -INF, 0], [INF, INF, INF],
                       [SUB, -SUB, SUB], [2.0 ** -100, 1, -1], [0.3, -0.5, 0.8], [-INF, 0, SUB], [NAN, NAN, NAN]], F)
    hand_o = np.tile(mid, (len(hand_d), 1))
    corner = np.tile(bmin, (len(hand_d), 1))
    face = np.tile(mid, (len(hand_d), 1))
    face[:, 2] = bmax[2]                      # exactly on the plane z = bmax.z, every hand-made direction
    o = np.concatenate([hand_o, np.where(np.isfinite(corner), corner, F(0.0)), face, o])
    d = np.concatenate([hand_d, hand_d, hand_d, d])
    return o, d, bmin, bmax
