"""The range arguments behind normalize_trim (rb_device_math.hpp), without a GPU.  The constants are read from the header as it
spells them, so a changed bound is checked, not the one this file remembers.

 * one range test: the correctly rounded root of every L that sqrt_exact's fast path accepts is a denominator that div3_exact's
   guard accepts, so the guard's range test is redundant after the root's.
 * the numerators by magnitude: with every |component| at or above normalize_trim's bound, L is at or above the root's lower
   bound (so only `L < upper` is tested), and the bound is no lower than the one div3_exact asks of a numerator.
 * the unit-vector form: every coordinate rnd_pm1 can return is 0 or a multiple of 2^-24 with magnitude in [2^-24, 1]; the
   point (0, 0, 0) cannot be drawn; an accepted point's L and root are in the fast ranges.
 * div_newton's obligation -- operands, q0 and the remainder clear of the subnormal range, the remainder exact -- modelled in
   exact rational arithmetic at the corners of those ranges, with the quotient it returns compared with the rounded one."""
import os
import re
from fractions import Fraction

import numpy as np

from tests.test_rnd_fused import one_rounding, pcg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
MIN_NORMAL = Fraction(1, 2 ** 126)


def _header():
    return open(os.path.join(ROOT, "renderbaby_amd/csrc/rb_device_math.hpp")).read()


def _body(name):
    """the text of the function `name` (up to the first line that closes it in column 0)"""
    text = _header()
    m = re.search(rf"^(?:template <[^>]*>\n)?DEV \w+ {name}\([^;\n]*\) \{{\n.*?^}}", text, re.M | re.S)
    assert m, name
    return m.group(0)


def _bits(x):
    return int(np.array(x, f32).view(np.uint32))


def _float(bits):
    return np.array(bits, np.uint32).view(f32)[()]


def _bit_range(body, var):
    """(low, high) bit patterns, high exclusive, of the test `(var - 0xLOW) < 0xSPAN`"""
    m = re.search(rf"\({var} - 0x([0-9A-Fa-f]+)u\) < 0x([0-9A-Fa-f]+)u", body)
    assert m, (var, body[:80])
    lo = int(m.group(1), 16)
    return lo, lo + int(m.group(2), 16)


def _hexfloat(body, pattern):
    m = re.search(pattern, body)
    assert m, pattern
    return f32(float.fromhex(m.group(1)))


def constants():
    c = {}
    c["root"] = _bit_range(_body("sqrt_exact"), r"__float_as_uint\(x\)")
    c["den"] = _bit_range(_body("div3_exact"), "xb")
    m = re.search(r">= \(0x([0-9A-Fa-f]+)u << 1\) - 2u", _body("div3_exact"))
    c["num"] = _float(int(m.group(1), 16))
    trim = _body("normalize_trim")
    c["trim_root_plain"] = _bit_range(trim, r"__float_as_uint\(L\)")
    c["trim_den_plain"] = _bit_range(trim, "xb")
    c["trim_upper"] = _hexfloat(trim, r"L < (0x1p[-+]?\d+)f")
    c["trim_num"] = _hexfloat(trim, r"fabsf\(a\.z\)\) >= (0x1p[-+]?\d+)f")
    return c


def test_the_header_spells_the_ranges_this_file_expects():
    c = constants()
    print({k: (tuple(hex(x) for x in v) if isinstance(v, tuple) else float(v)) for k, v in c.items()})
    assert c["root"] == (_bits(2.0 ** -60), _bits(2.0 ** 60))
    assert c["den"] == (_bits(2.0 ** -60), _bits(2.0 ** 59))
    assert c["num"] == f32(2.0 ** -100)
    # with its knobs off normalize_trim tests what sqrt_exact and div3_exact test
    assert c["trim_root_plain"] == c["root"] and c["trim_den_plain"] == c["den"]


def test_root_of_the_fast_range_is_a_denominator_of_the_fast_range():
    c = constants()
    (lo, hi), (dlo, dhi) = c["root"], c["den"]
    ends = np.array([lo, lo + 1, hi - 2, hi - 1], np.uint32).view(f32)
    roots = np.sqrt(ends)   # numpy's float32 square root is correctly rounded, and monotonic: the ends bound every root
    print("L in", [float(x) for x in ends[[0, 3]]], "-> root in", [float(x) for x in roots[[0, 3]]],
          "; the guard takes", [float(_float(dlo)), float(_float(dhi))])
    assert roots[0] == f32(2.0 ** -30) and roots[3] <= f32(2.0 ** 30)
    rb = roots.view(np.uint32)
    assert (rb >= dlo).all() and (rb < dhi).all()
    assert (np.diff(rb.astype(np.int64)) >= 0).all()


def test_numerator_bound_implies_the_lower_bound_of_L():
    c = constants()
    t, (lo, hi) = c["trim_num"], c["root"]
    assert t >= c["num"]                       # what passes here would have passed div3_exact's numerator test
    assert c["trim_upper"] == _float(hi)       # `L < upper` is the upper half of the root's range test
    sq = t * t                                 # the smallest square of a component that passes; exact (a power of two)
    assert Fraction(float(sq)) == Fraction(float(t)) ** 2
    L = (sq + sq) + sq                         # the smallest L: every sum rounds monotonically, so no L is below it
    assert _bits(sq) >= lo and _bits(L) >= lo
    # one ulp below the bound the implication is not needed: such a component fails the test
    below = _float(_bits(t) - 1)
    assert below < t


# ------------------------------------------------------------------------------------------------ the unit-vector form
def test_every_coordinate_is_zero_or_on_the_grid():
    lo, hi = _bits(1.0), _bits(4294967296.0)
    step, zeros, smallest, largest = 1 << 24, [], f32(1.0), f32(0.0)
    for b0 in range(lo, hi + 1, step):
        c = np.arange(b0, min(b0 + step, hi + 1), dtype=np.uint32).view(f32)
        x = one_rounding(c)
        scaled = x.astype(f64) * f64(2.0 ** 24)
        assert (scaled == np.rint(scaled)).all()            # a multiple of 2^-24
        mag = np.abs(x)
        zeros += [float(v) for v in c[mag == 0]]
        nz = mag[mag != 0]
        smallest, largest = min(smallest, nz.min()), max(largest, nz.max())
    assert one_rounding(np.zeros(1, f32))[0] == f32(-1.0)   # c = 0, the one value outside [1, 2^32]
    print("zero at c =", zeros, "; non-zero magnitudes in", [float(smallest), float(largest)])
    assert zeros == [2.0 ** 31]
    assert smallest == f32(2.0 ** -24) and largest == f32(1.0)


def test_the_origin_cannot_be_drawn():
    # a coordinate is 0 only for c = (float)seed = 2^31: the seeds that round to it
    window = [s for s in range(2 ** 31 - 512, 2 ** 31 + 512) if f32(s) == f32(2.0 ** 31)]
    assert window[0] == 2 ** 31 - 64 and window[-1] == 2 ** 31 + 128
    # (0, 0, 0) needs pcg to map a seed of the window into the window, twice in a row; it never does once
    followers = [s for s in window if pcg(s) in set(window)]
    assert followers == []


def test_accepted_points_are_inside_the_fast_ranges():
    c = constants()
    (lo, hi), (dlo, dhi) = c["root"], c["den"]
    g = f32(2.0 ** -24)
    least = (g * g + f32(0)) + f32(0)                # one coordinate at the grid's first step, two zeros
    most = _float(_bits(1.0) - 1)                    # accepted means L < 1
    assert least == f32(2.0 ** -48)
    assert lo <= _bits(least) and _bits(most) < hi
    roots = np.sqrt(np.array([least, most], f32))
    print("L in", [float(least), float(most)], "-> root in", [float(r) for r in roots])
    assert roots[0] == g and roots[1] < f32(1.0)
    assert dlo <= _bits(roots[0]) and _bits(roots[1]) < dhi


# ------------------------------------------------------------------------------------------------ div_newton, a model
def _rn(fr):
    """a Fraction rounded to the nearest float32, ties to even (through the exact double where the value fits, which every
    value here does: products and sums of two or three float32)"""
    d = float(fr)
    assert Fraction(d) == fr
    return f32(d)


def div_newton_model(a, b):
    """-> the quotient div_newton returns for float32 a, b with y = RN(1 / b), and its intermediate values as Fractions"""
    A, B = Fraction(float(a)), Fraction(float(b))
    y = f32(1.0) / b                                  # rcp_newton is the correctly rounded reciprocal where it is used
    Y = Fraction(float(y))
    q0 = _rn(A * Y)
    r = A - B * Fraction(float(q0))                   # the fused multiply-add's argument, before its rounding
    q = f32(float(Fraction(float(q0)) + r * Y))       # one rounding of the exact sum (a double holds it to far below half an ulp)
    return q, y, q0, r


def _corner_pairs():
    def around(x):
        b = _bits(x)
        return [_float(b), _float(b + 1), _float(b - 1)]

    ones = lambda e: _float(_bits(2.0 ** e) - 2)      # the largest significand the guard lets through, below 2^e
    unit_den = [f32(2.0 ** -24), _float(_bits(2.0 ** -24) + 1), ones(-23), f32(0.5), ones(0), _float(_bits(1.0) - 3)]
    unit_num = [f32(2.0 ** -24), f32(3 * 2.0 ** -24), f32(0.5), _float(_bits(1.0) - 1)]
    pairs = [(a, b, "unit") for b in unit_den for a in unit_num if a <= b * f32(1.0000002)]
    t = constants()["trim_num"]
    gen_den = [f32(2.0 ** -30) * f32(1.7320508), ones(-29), f32(1.0), ones(30), f32(2.0 ** 30)]
    gen_num = around(t)[:2] + [f32(1.0), ones(1), ones(30), f32(2.0 ** 30)]
    pairs += [(a, b, "general") for b in gen_den for a in gen_num if a <= b * f32(1.0000002)]
    return pairs


def test_div_newton_stays_clear_of_the_subnormal_range_at_the_corners():
    pairs = _corner_pairs()
    assert len([p for p in pairs if p[2] == "unit"]) >= 12 and len([p for p in pairs if p[2] == "general"]) >= 12
    for a, b, what in pairs:
        for sign in (f32(1.0), f32(-1.0)):
            q, y, q0, r = div_newton_model(sign * a, b)
            for name, v in (("a", a), ("b", b), ("y", y), ("q0", q0), ("q", q)):
                assert abs(Fraction(float(v))) >= MIN_NORMAL and np.isfinite(v), (what, float(a), float(b), name)
            assert r == 0 or abs(r) >= MIN_NORMAL, (what, float(a), float(b), r)
            assert Fraction(float(f32(float(r)))) == r, "the remainder is a float32: the fused multiply-add returns it exactly"
            assert _bits(q) == _bits((sign * a) / b), (what, float(a), float(b))
            assert np.signbit(q) == np.signbit(sign), "a non-zero quotient has its sign without a copysign"
