// rb_probe_visibility.hip -- light points from a baked probe grid without leaks (rb_light_points_visible; DESIGN.md section 20,
// the normative definition): rb_light_points' blend with every corner's weight times a wrapped cosine of the point's normal
// towards the probe and the Chebyshev bound of the point's distance against the probe's depth moments (rb_probe_depth.hip).
// Same numerics contract as rb_kernels.hip: every step one binary32 operation in the order written, no FMA contraction,
// correctly rounded / and sqrt, so that renderbaby_amd/probes.py (light_visible) equals this file bit for bit.
#include "rb_device_probe.hpp"

#pragma clang fp contract(off)

namespace rb {
namespace {

// =================================================== k_probe_light_vis ====
// probe_light_body (rb_device_probe.hpp) in k_probe_light's shape, the corners in groups of two: beside a group's 2 x 7 record
// loads its two texel loads, whose addresses need no record.
__global__ void __launch_bounds__(256) k_probe_light_vis(const ProbeLightArgs a, const ProbeVisArgs va) { probe_light_body<2, true>(a, va); }

}  // namespace

// out[i] = the lit value of points[i], i < a.m, as launch_probe_light, with the visibility weights of `prm` from the grid's
// moment maps (nullptr under RB_VIS_NO_DEPTH: not read).  The caller has checked the grid and prm.  Returns a hipError_t.
int launch_probe_light_vis(const ProbeLightArgs& a, const rb_probe_depth* moments, const rb_light_visibility& prm, void* stream_) {
    if (a.m == 0u) return 0;
    if (a.coeffs == nullptr || a.points == nullptr || a.out == nullptr) return (int)hipErrorInvalidValue;
    if (moments == nullptr && (prm.flags & RB_VIS_NO_DEPTH) == 0u) return (int)hipErrorInvalidValue;
    if (a.grid.counts[0] == 0u || a.grid.counts[1] == 0u || a.grid.counts[2] == 0u) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_probe_light_vis, dim3((a.m + 255u) / 256u), dim3(256), 0, static_cast<hipStream_t>(stream_), a, ProbeVisArgs{moments, prm});
    return (int)hipGetLastError();
}

}  // namespace rb
