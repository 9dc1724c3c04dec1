"""normalize_trim (rb_device_math.hpp), the normalize of k_trace and k_trace_direct, on the device against the compiler's
v / sqrt(dot(v, v)) with its correctly rounded / and sqrt (rb_debug_normalize_sites): every component of every result bit for
bit, a NaN equal to a NaN.  Zero differences are expected.

The general form (the sphere normal, the scatter's operand, the new direction):
 * 2^20 seeded vectors whose exponents are drawn over the whole binary32 range, half of them with the three exponents close
   together (so that no single component decides L), half independently;
 * every triple, both signs, of a set of special values: each bound the guards use (2^-100 and 2^-30 for a numerator, 2^-60 and
   2^60 for L and so 2^-30 and 2^30 for a lone component, 2^59 and 2^-60 for the denominator) with the floats one ulp below and
   above it, 0 (one, two and three zero components, either sign), subnormals, values whose squares overflow or underflow L, an
   infinity and a NaN (in each position);
 * vectors searched for on the host whose root, or whose L, has an all-ones significand or all ones in its low 16 bits (the
   guards of the reciprocal), none of their components zero.
The unit-vector form (the rejection loop's accepted point):
 * every point with coordinates from {0, +-2^-24, +-2^-23, +-1/2, +-(1 - 2^-24)} that the loop can accept (0 < L < 1);
 * the first try of the loop from 2^20 consecutive seeds, wherever it is accepted."""
import itertools

import numpy as np
import pytest

from renderbaby_amd import _lib

pytestmark = pytest.mark.gpu
f32 = np.float32


def _f(bits):
    return np.asarray(bits, np.uint32).view(f32)


def _b(x):
    return np.asarray(x, f32).view(np.uint32)


def _len2(v):
    """dot(v, v) as the device computes it: (xx + yy) + zz in float32"""
    with np.errstate(all="ignore"):
        return (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]


def _seeded(n, rng):
    sign = rng.integers(0, 2, (n, 3), dtype=np.uint32) << np.uint32(31)
    mant = rng.integers(0, 1 << 23, (n, 3), dtype=np.uint32)
    expo = rng.integers(0, 256, (n, 3), dtype=np.int64)
    near = np.arange(n) < n // 2
    base = rng.integers(0, 256, n, dtype=np.int64)
    close = np.clip(base[:, None] + rng.integers(-3, 4, (n, 3)), 0, 255)
    expo = np.where(near[:, None], close, expo).astype(np.uint32)
    return _f(sign | (expo << np.uint32(23)) | mant)


def _specials():
    vals = []
    for e in (-100, -60, -30, -24, 29, 30, 59, 60, 100):
        b = int(_b(2.0 ** e))
        vals += [b - 1, b, b + 1]
    vals += [int(_b(x)) for x in (0.0, 1.0, 3.0, 2.0 ** 64, 1.5 * 2.0 ** 127, 2.0 ** -70, 2.0 ** -75)]
    vals += [0x00000001, 0x007FFFFF, 0x00400000]          # subnormals: the least, the greatest, 2^-127
    vals += [0x7F800000, 0x7FC00000, 0x7F800001]          # infinity, a quiet NaN, a signalling one
    one = np.array(vals, np.uint32)
    both = np.concatenate([one, one | np.uint32(0x80000000)])
    return _f(np.array(list(itertools.product(both, repeat=3)), np.uint32))


def _ones_in_root_or_L(rng):
    """vectors without a zero component whose sqrt(L), or whose L, ends in 16 or in 23 one bits: random directions scaled to a
    target length, the first component then walked ulp by ulp until the float32 result lands on the target"""
    out, found = [], {"root16": 0, "root23": 0, "L16": 0, "L23": 0}
    for e in (-20, -1, 0, 1, 7, 20):
        for mant in (0x7FFFFF, 0x12FFFF, 0x00FFFF, 0x7EFFFF):
            target = float(_f((127 + e) << 23 | mant))
            u = rng.normal(size=(96, 3))
            u /= np.linalg.norm(u, axis=1)[:, None]
            for of_root in (True, False):
                length = target if of_root else np.sqrt(target)
                v = (u * length).astype(f32)
                steps = np.arange(-48, 49, dtype=np.int64)
                cand = np.repeat(v[:, None, :], len(steps), axis=1)
                cand[:, :, 0] = _f((_b(v[:, 0]).astype(np.int64)[:, None] + steps).astype(np.uint32))
                cand = cand.reshape(-1, 3)
                L = _len2(cand)
                got = np.sqrt(L) if of_root else L
                low = _b(got) & np.uint32(0xFFFF)
                hit = (low == 0xFFFF) & (np.abs(cand).min(axis=1) > 0)
                out.append(cand[hit])
                m23 = (_b(got[hit]) & np.uint32(0x7FFFFF)) == 0x7FFFFF
                found[("root" if of_root else "L") + "16"] += int(hit.sum())
                found[("root" if of_root else "L") + "23"] += int(m23.sum())
    return np.concatenate(out), found


def _unit_points():
    g = 2.0 ** -24
    coords = np.array([0.0, g, -g, 2 * g, -2 * g, 0.5, -0.5, 1.0 - g, -(1.0 - g)], f32)
    pts = np.array(list(itertools.product(coords, repeat=3)), f32)
    L = _len2(pts)
    return pts[(L > 0) & (L < 1)]


@pytest.fixture(scope="module")
def inputs():
    rng = np.random.default_rng(20270127)
    seeded, special = _seeded(1 << 20, rng), _specials()
    ones, found = _ones_in_root_or_L(rng)
    print("seeded", len(seeded), "special", len(special), "all-ones cases", found)
    assert min(found.values()) > 0, found
    return np.concatenate([seeded, special, ones]).astype(f32), _unit_points()


def test_inputs_hold_the_cases(inputs):
    general, unit = inputs
    L = _len2(general)
    zeros = (general == 0).sum(axis=1)
    assert all((zeros == k).any() for k in (0, 1, 2, 3))
    assert np.isinf(L).any() and np.isnan(L).any() and ((L == 0) & (zeros < 3)).any()
    sub = (np.abs(general) > 0) & (np.abs(general) < f32(2.0 ** -126))
    assert sub.any(axis=0).all()
    for pos in range(3):
        assert np.isinf(general[:, pos]).any() and np.isnan(general[:, pos]).any()
    # both sides of each guard, among vectors with nothing else to send them the slow way
    fast_L = (L >= f32(2.0 ** -60)) & (L < f32(2.0 ** 60))
    small = np.abs(general).min(axis=1)
    assert (fast_L & (small >= f32(2.0 ** -30))).sum() > 1000 and (fast_L & (small < f32(2.0 ** -30)) & (small > 0)).sum() > 1000
    assert (~fast_L & np.isfinite(L) & (small >= f32(2.0 ** -30))).sum() > 1000
    assert len(unit) > 300 and (unit == 0).any() and (np.abs(unit) == f32(2.0 ** -24)).any() and (np.abs(unit) == f32(1 - 2.0 ** -24)).any()


def test_normalize_sites_match_the_compiler_s_quotient(inputs):
    general, unit = inputs
    xyz = np.ascontiguousarray(np.concatenate([general, unit]), dtype=f32)
    out = np.zeros(16, np.uint32)
    n_seeds = 1 << 20
    assert _lib.load().rb_debug_normalize_sites(xyz.ctypes.data, len(general), len(unit), 0x9E3779B9, n_seeds, out.ctypes.data) == 0
    print("differing: general", out[0], "unit points", out[1], "unit seeds", out[2], "; accepted tries", out[3], "of", n_seeds)
    detail = dict(index=int(out[4]) - 1, v=[hex(int(x)) for x in out[5:8]], got=[hex(int(x)) for x in out[8:11]], want=[hex(int(x)) for x in out[11:14]])
    assert out[0] == 0 and out[1] == 0 and out[2] == 0, detail
    assert 0.45 * n_seeds < out[3] < 0.60 * n_seeds   # the unit ball fills pi / 6 of the cube
