// rb_device_sh.hpp -- the nine real spherical harmonics of bands 0-2 as the device's probe stages share them (rb_probe.hip's
// projection, rb_probe_light.hip's lighting).  Its includer keeps floating-point contraction off.
#pragma once
#include "rb_device_math.hpp"

#pragma clang fp contract(off)

namespace rb {
namespace {

struct ShBasis {
    float y[9];
};
// the basis of the direction as given: one operation per step, section 18.1's grouping
DEV ShBasis sh_basis(float x, float y, float z) {
    ShBasis b;
    b.y[0] = 0.282094792f;
    b.y[1] = 0.488602512f * y;
    b.y[2] = 0.488602512f * z;
    b.y[3] = 0.488602512f * x;
    b.y[4] = 1.09254843f * (x * y);
    b.y[5] = 1.09254843f * (y * z);
    b.y[6] = 0.315391565f * (3.0f * (z * z) - 1.0f);
    b.y[7] = 1.09254843f * (x * z);
    b.y[8] = 0.546274215f * (x * x - y * y);
    return b;
}

}  // namespace
}  // namespace rb
