// rb_device_centre.hpp -- the pixel-centre ray of the first-hit buffers, shared by the query kernels (rb_query.hip) and the
// denoiser's guide pack (rb_denoise.hip): both must normalise the same direction bit for bit.
#pragma once
#include "rb_device_math.hpp"

#pragma clang fp contract(off)

namespace rb {
namespace {

// shader.wgsl:693-709 for the pixel CENTRE: start_path_hashed's arithmetic with both offsets 0.0f
DEV f3 centre_ray_dir(const Cam& c, uint32_t x, uint32_t y) {
    const float ax = (float)x + 0.0f, ay = (float)y + 0.0f;
    float qx, qy;
    if (c.fast_wh) {
        qx = __builtin_copysignf(div_newton(ax, c.wm1, c.inv_wm1), ax);
        qy = __builtin_copysignf(div_newton(ay, c.hm1, c.inv_hm1), ay);
    } else {
        qx = ax / c.wm1;
        qy = ay / c.hm1;
    }
    const float u = ((qx * 2.0f) - 1.0f) * c.aspect;
    const float v = 1.0f - qy * 2.0f;
    return normalize(((c.fov * u) * ld3(c.right) + (c.fov * v) * ld3(c.up)) + ld3(c.fwd));
}

}  // namespace
}  // namespace rb
