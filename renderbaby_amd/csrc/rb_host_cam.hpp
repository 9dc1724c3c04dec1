// rb_host_cam.hpp -- the render camera's per-launch invariants (shader.wgsl:690,702-708) in the shader's operation order, worked
// out on the host: single IEEE binary32 operations, no contraction, correctly rounded / and sqrt (the Makefile's NUMERICS hold
// for host code too).  Host only.  The one source of these steps: host_cam (rb_kernels.hip) fills a launch's Cam from them,
// rb_view_from_camera (rb_queries.cpp) the rb_view of the temporal reprojection.
#pragma once
#include <cstdint>

#include "../../include/rb_abi.h"

#pragma clang fp contract(off)

namespace rb {

struct CamBasis {
    float aspect;
    float fwd[3], right[3], up[3];
    float fov, wm1, hm1;
};

inline CamBasis host_cam_basis(const rb_camera& cam, uint32_t width, uint32_t height) {
    struct V { float x, y, z; };
    auto cross = [](V a, V b) { return V{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; };
    auto normalize = [](V a) {
        const float len = __builtin_sqrtf((a.x * a.x + a.y * a.y) + a.z * a.z);
        return V{a.x / len, a.y / len, a.z / len};
    };
    CamBasis c{};
    c.aspect = (float)width / (float)height;
    const V fwd = normalize(V{cam.dir[0], cam.dir[1], cam.dir[2]});
    const V right = normalize(cross(V{0.0f, 1.0f, 0.0f}, fwd));
    const V up = cross(fwd, right);
    c.fwd[0] = fwd.x, c.fwd[1] = fwd.y, c.fwd[2] = fwd.z;
    c.right[0] = right.x, c.right[1] = right.y, c.right[2] = right.z;
    c.up[0] = up.x, c.up[1] = up.y, c.up[2] = up.z;
    c.fov = cam.pane_width / (2.0f * cam.pane_distance * c.aspect);
    c.wm1 = (float)(width - 1u);
    c.hm1 = (float)(height - 1u);
    return c;
}

}  // namespace rb
