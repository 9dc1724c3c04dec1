// rb_device_probe.hpp -- what the kernels over a baked probe grid share (rb_probe_light.hip, rb_probe_visibility.hip,
// rb_probe_depth.hip; DESIGN.md sections 19 and 20): a coefficient record in registers, one axis of a point's cell, the texel of
// a vector in a probe's octahedral map, and the blend of the eight probes round a point with or without the visibility weights.
// Its includer keeps floating-point contraction off.
#pragma once
#include "rb_device_sh.hpp"

#pragma clang fp contract(off)

namespace rb {
namespace {

constexpr int kShQuads = sizeof(rb_sh9) / 16;   // a record is seven 16-byte loads

struct ShRecord {
    float v[kShQuads * 4];   // sum[j][ch] at j * 3 + ch, the weight at 27
};
DEV ShRecord load_record(const rb_sh9* recs, size_t idx) {
    const v4f* const q = reinterpret_cast<const v4f*>(recs) + idx * kShQuads;
    ShRecord r;
#pragma unroll
    for (int k = 0; k < kShQuads; k++) {
        const v4f x = q[k];
        r.v[k * 4 + 0] = x.x;
        r.v[k * 4 + 1] = x.y;
        r.v[k * 4 + 2] = x.z;
        r.v[k * 4 + 3] = x.w;
    }
    return r;
}

// One axis of the cell: the lower probe's index i0 and the point's share t of the way to the upper one.  max(f, 0.0f) is
// f > 0.0f ? f : 0.0f and min(f, top) is f < top ? f : top (section 19: a NaN cannot arrive here, -0 becomes +0).
struct CellAxis {
    uint32_t i0;
    float t;
};
DEV CellAxis cell_axis(float p, float origin, float step, uint32_t count) {
    float f = (p - origin) / step;
    f = f > 0.0f ? f : 0.0f;
    const float top = (float)(count - 1u);
    f = f < top ? f : top;
    CellAxis a;
    a.i0 = min((uint32_t)__builtin_floorf(f), count >= 2u ? count - 2u : 0u);   // f <= 2^31: the conversion is exact
    a.t = f - (float)a.i0;
    return a;
}

// Section 20.1: the texel of a vector, of any length, in the 8 x 8 octahedral map, ty * 8 + tx.  The zero vector is the
// caller's to catch; whatever comes in -- a NaN of 0 / 0 included -- the result is at most 63, so it may index a map: the
// clamp is made on the float (a NaN becomes 0), where floor and the conversion agree and nothing is out of the conversion's range.
DEV uint32_t oct_axis(float p) { return (uint32_t)__builtin_fminf(__builtin_fmaxf((p * 0.5f + 0.5f) * 8.0f, 0.0f), 7.0f); }
DEV uint32_t oct_texel(float vx, float vy, float vz) {
    const float s = (__builtin_fabsf(vx) + __builtin_fabsf(vy)) + __builtin_fabsf(vz);
    float px = vx / s, py = vy / s;
    if (vz < 0.0f) {   // (-0.0f stays in the upper half)
        const float fx = (1.0f - __builtin_fabsf(py)) * (px >= 0.0f ? 1.0f : -1.0f);
        const float fy = (1.0f - __builtin_fabsf(px)) * (py >= 0.0f ? 1.0f : -1.0f);
        px = fx;
        py = fy;
    }
    return oct_axis(py) * 8u + oct_axis(px);
}

// what k_probe_light_vis takes beside ProbeLightArgs (VIS == false: not read)
struct ProbeVisArgs {
    const rb_probe_depth* moments;   // nx ny nz maps, the records' order; not read under RB_VIS_NO_DEPTH
    rb_light_visibility prm;
};

// lane = point.  The corners in the definition's order, GROUP of them at a time: a group's record indices and geometric weights,
// its loads, then its arithmetic; a corner's dot products fold into three sums, so what lives across corners is E, W, the
// basis and the cell.  A corner that the definition skips is loaded all the same (a corner that does not exist: the record of
// its d = 0 neighbour, which is inside the grid) and dropped by a select, so no value of it reaches the result and the loads of
// several corners can be in flight.
// VIS (section 20.3): every corner's weight times the wrapped cosine towards the probe and the Chebyshev bound of the probe's
// depth moments.  Neither the texel of a corner nor the two factors that need no record wait for a load: the texel's address
// comes from the point and the probe's position, so its 16-byte load goes out with the group's record loads.
template <int GROUP, bool VIS>
DEV void probe_light_body(const ProbeLightArgs& a, const ProbeVisArgs& va) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.m) return;
    const v4f p0 = reinterpret_cast<const v4f*>(a.points)[(size_t)i * 2u], p1 = reinterpret_cast<const v4f*>(a.points)[(size_t)i * 2u + 1u];
    const f3 pos = mk(p0.x, p0.y, p0.z), nrm = mk(p1.x, p1.y, p1.z);
    v4f* const out = reinterpret_cast<v4f*>(a.out) + i;
    const v4f nothing = {0.0f, 0.0f, 0.0f, 0.0f};
    const float len2 = dot(nrm, nrm);
    if (!(finite3(pos) && finite3(nrm) && !zero3(nrm) && (__float_as_uint(len2) & 0x7F800000u) != 0x7F800000u)) {
        *out = nothing;
        return;
    }
    const f3 n = div3_exact(nrm, sqrt_exact(len2));
    const ShBasis b = sh_basis(n.x, n.y, n.z);

    const rb_probe_grid& g = a.grid;
    const CellAxis ax = cell_axis(pos.x, g.origin[0], g.step[0], g.counts[0]);
    const CellAxis ay = cell_axis(pos.y, g.origin[1], g.step[1], g.counts[1]);
    const CellAxis az = cell_axis(pos.z, g.origin[2], g.step[2], g.counts[2]);
    const bool two_x = g.counts[0] >= 2u, two_y = g.counts[1] >= 2u, two_z = g.counts[2] >= 2u;
    const uint32_t base = (az.i0 * g.counts[1] + ay.i0) * g.counts[0] + ax.i0;   // < nx ny nz <= 2^31 - 64
    const uint32_t sx = two_x ? 1u : 0u, sy = two_y ? g.counts[0] : 0u, sz = two_z ? g.counts[0] * g.counts[1] : 0u;
    const float ux = 1.0f - ax.t, uy = 1.0f - ay.t, uz = 1.0f - az.t;
    const bool wrap = VIS && (va.prm.flags & RB_VIS_NO_WRAP) == 0u, depth = VIS && (va.prm.flags & RB_VIS_NO_DEPTH) == 0u;   // wave-uniform
    const f3 biased = VIS ? pos + va.prm.normal_bias * n : pos;

    float E[3] = {0.0f, 0.0f, 0.0f}, W = 0.0f;
#pragma unroll 1
    for (int c0 = 0; c0 < 8; c0 += GROUP) {   // (GROUP == 8: one trip, and the corner numbers are constants)
        uint32_t idx[GROUP];
        float wg[GROUP], wb[GROUP], dist[GROUP];
        bool exists[GROUP];
        v4f tex[GROUP];
#pragma unroll
        for (int k = 0; k < GROUP; k++) {
            const int c = c0 + k;
            const bool dx = (c & 1) != 0, dy = (c & 2) != 0, dz = (c & 4) != 0;
            idx[k] = base + (dx ? sx : 0u) + (dy ? sy : 0u) + (dz ? sz : 0u);
            wg[k] = ((dx ? ax.t : ux) * (dy ? ay.t : uy)) * (dz ? az.t : uz);
            exists[k] = (!dx || two_x) && (!dy || two_y) && (!dz || two_z);
            if constexpr (VIS) {
                const f3 P = mk(g.origin[0] + (float)(ax.i0 + (dx ? 1u : 0u)) * g.step[0], g.origin[1] + (float)(ay.i0 + (dy ? 1u : 0u)) * g.step[1],
                                g.origin[2] + (float)(az.i0 + (dz ? 1u : 0u)) * g.step[2]);
                const f3 q = P - pos, v = biased - P;
                const float l = sqrt_exact(dot(q, q));
                const float cw = l > 0.0f ? dot(q, n) / l : 1.0f;
                const float h = (cw + 1.0f) * 0.5f;
                wb[k] = wrap ? h * h + 0.2f : 1.0f;
                dist[k] = sqrt_exact(dot(v, v));
                // (v == 0, or a corner that does not exist: some texel of a map inside the grid, dropped below)
                if (depth) tex[k] = reinterpret_cast<const v4f*>(va.moments)[(size_t)idx[k] * 64u + oct_texel(v.x, v.y, v.z)];
            }
        }
        ShRecord r[GROUP];
#pragma unroll
        for (int k = 0; k < GROUP; k++) r[k] = load_record(a.coeffs, idx[k]);
#pragma unroll
        for (int k = 0; k < GROUP; k++) {
            float w = wg[k] * r[k].v[27];
            bool skip = !exists[k] || w == 0.0f;
            if constexpr (VIS) {
                float vis = 1.0f;
                if (depth) {
                    const float mean = tex[k].x, mean2 = tex[k].y;
                    const float var = __builtin_fabsf(mean2 - mean * mean), dl = dist[k] - mean;
                    const float den = var + dl * dl;
                    const float ch = den > 0.0f ? var / den : 1.0f;
                    const bool open = dist[k] == 0.0f || tex[k].z == 0.0f || !(dist[k] > mean);
                    vis = open ? 1.0f : (ch * ch) * ch;
                }
                vis = vis > va.prm.min_visibility ? vis : va.prm.min_visibility;
                w = (w * wb[k]) * vis;
                skip = skip || w == 0.0f;
            }
            float e[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int j = 0; j < 9; j++) {
#pragma unroll
                for (int ch = 0; ch < 3; ch++) e[ch] = e[ch] + r[k].v[j * 3 + ch] * b.y[j];
            }
#pragma unroll
            for (int ch = 0; ch < 3; ch++) E[ch] = skip ? E[ch] : E[ch] + w * e[ch];
            W = skip ? W : W + w;
        }
    }

    if (W > 0.0f) {
        const float r = E[0] / W, gr = E[1] / W, bl = E[2] / W;
        const v4f lit = {r > 0.0f ? r : 0.0f, gr > 0.0f ? gr : 0.0f, bl > 0.0f ? bl : 0.0f, W};
        *out = lit;
    } else {
        *out = nothing;
    }
}

}  // namespace
}  // namespace rb
