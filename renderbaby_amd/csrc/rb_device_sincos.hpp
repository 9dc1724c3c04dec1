// rb_device_sincos.hpp -- sincos_turn, the fixed polynomial sine and cosine of the device's ray generators (rb_camera.hip,
// rb_hemisphere.hip).  Its includer keeps floating-point contraction off.
#pragma once
#include "rb_device_math.hpp"

#pragma clang fp contract(off)

namespace rb {
namespace {

// sin and cos of pi * s for s in [-1, 1] (section 15.3): q = the nearest quarter turn, r = s - q / 2 exactly, x = r * (float)pi
// with |x| <= pi / 4, the two Taylor polynomials in Horner form -- one multiply, then one add per step --, the result by the
// quadrant q mod 4.  Within 2^-22 of the true values; the coefficients are the binary64 quotients rounded to binary32.
struct SinCos {
    float s, c;
};
DEV SinCos sincos_turn(float s) {
    const float q = __builtin_rintf(2.0f * s);
    const float r = s - 0.5f * q;
    const float x = r * 3.14159274101257324f;
    const float x2 = x * x;
    float ps = (float)(1.0 / 362880.0);
    ps = ps * x2 + (float)(-1.0 / 5040.0);
    ps = ps * x2 + (float)(1.0 / 120.0);
    ps = ps * x2 + (float)(-1.0 / 6.0);
    ps = ps * x2 + 1.0f;
    const float sn = x * ps;
    float pc = (float)(1.0 / 40320.0);
    pc = pc * x2 + (float)(-1.0 / 720.0);
    pc = pc * x2 + (float)(1.0 / 24.0);
    pc = pc * x2 + (float)(-1.0 / 2.0);
    pc = pc * x2 + 1.0f;
    const uint32_t quad = (uint32_t)(int)q & 3u;
    SinCos o;
    o.s = quad == 0u ? sn : quad == 1u ? pc : quad == 2u ? -sn : -pc;
    o.c = quad == 0u ? pc : quad == 1u ? -sn : quad == 2u ? -pc : sn;
    return o;
}

}  // namespace
}  // namespace rb
