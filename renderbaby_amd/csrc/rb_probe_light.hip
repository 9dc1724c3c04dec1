// rb_probe_light.hip -- light points from a baked probe grid on the device (rb_probe_coefficients, rb_light_points; DESIGN.md
// section 19, the normative definition): the SH9 sums of rb_bake_probes scaled to irradiance-over-pi coefficients, and the blend
// of the eight probes round a point of a regular grid, each probe's coefficients dotted with the basis of the point's normal.
// Same numerics contract as rb_kernels.hip: every step one binary32 operation in the order written, no FMA contraction,
// correctly rounded / and sqrt, so that renderbaby_amd/probes.py (coefficients, light) equals this file bit for bit.
#include <cstdlib>

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

// ====================================================== k_probe_coeffs ====
// lane = probe.  The lane holds its whole record before it writes, so `out` may be `sums`.
__global__ void __launch_bounds__(256) k_probe_coeffs(const rb_sh9* sums, uint32_t n, rb_sh9* out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    ShRecord r = load_record(sums, i);
    const float w = r.v[27];
    const bool valid = w > 0.0f && w < __builtin_inff();   // finite and greater than 0; a NaN fails both
#pragma unroll
    for (int j = 0; j < 9; j++) {
        const float k = j == 0 ? 12.566371f : j < 4 ? 8.37758f : 3.1415927f;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) r.v[j * 3 + ch] = valid ? (r.v[j * 3 + ch] * k) / w : 0.0f;
    }
    r.v[27] = valid ? 1.0f : 0.0f;
    v4f* const q = reinterpret_cast<v4f*>(out) + (size_t)i * kShQuads;
#pragma unroll
    for (int k = 0; k < kShQuads; k++) {
        const v4f x = {r.v[k * 4 + 0], r.v[k * 4 + 1], r.v[k * 4 + 2], r.v[k * 4 + 3]};
        q[k] = x;
    }
}

// ======================================================= k_probe_light ====
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

// lane = point.  The corners in the definition's order, GROUP of them at a time: a group's record indices and geometric weights,
// its loads, then its arithmetic; a corner's dot products fold into three sums, so what lives across corners is E, W, the
// basis and the cell.  A corner that the
// definition skips is loaded all the same (a corner that does not exist: the record of its d = 0 neighbour, which is inside
// the grid) and dropped by a select, so no value of it reaches the result and the loads of several corners can be in flight.
template <int GROUP>
DEV void probe_light_body(const ProbeLightArgs& a) {
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

    float E[3] = {0.0f, 0.0f, 0.0f}, W = 0.0f;
#pragma unroll 1
    for (int c0 = 0; c0 < 8; c0 += GROUP) {   // (GROUP == 8: one trip, and the corner numbers are constants)
        uint32_t idx[GROUP];
        float wg[GROUP];
        bool exists[GROUP];
#pragma unroll
        for (int k = 0; k < GROUP; k++) {
            const int c = c0 + k;
            const bool dx = (c & 1) != 0, dy = (c & 2) != 0, dz = (c & 4) != 0;
            idx[k] = base + (dx ? sx : 0u) + (dy ? sy : 0u) + (dz ? sz : 0u);
            wg[k] = ((dx ? ax.t : ux) * (dy ? ay.t : uy)) * (dz ? az.t : uz);
            exists[k] = (!dx || two_x) && (!dy || two_y) && (!dz || two_z);
        }
        ShRecord r[GROUP];
#pragma unroll
        for (int k = 0; k < GROUP; k++) r[k] = load_record(a.coeffs, idx[k]);
#pragma unroll
        for (int k = 0; k < GROUP; k++) {
            const float w = wg[k] * r[k].v[27];
            const bool skip = !exists[k] || w == 0.0f;
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

// The two shapes differ in how many corners' loads the compiler may keep in flight, that is in the registers a lane holds
// against the waves that share a SIMD: "pairs" -- the corners in groups of two, the two records that lie side by side in
// memory, 82 registers, five waves --, "wide" -- all eight corners' 56 loads issued before the first use, 243 registers, two
// waves (section 19.4 has the measurement that chose).
__global__ void __launch_bounds__(256) k_probe_light(const ProbeLightArgs a) { probe_light_body<2>(a); }
__global__ void __launch_bounds__(256) k_probe_light_wide(const ProbeLightArgs a) { probe_light_body<8>(a); }

}  // namespace

// out[i] = the coefficients of sums[i], i < n, queued on `stream`; out may be sums.  Returns a hipError_t.
int launch_probe_coeffs(const rb_sh9* sums, uint32_t n, rb_sh9* out, void* stream_) {
    if (n == 0u) return 0;
    if (sums == nullptr || out == nullptr) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_probe_coeffs, dim3((n + 255u) / 256u), dim3(256), 0, static_cast<hipStream_t>(stream_), sums, n, out);
    return (int)hipGetLastError();
}

// out[i] = the lit value of points[i], i < a.m, from the grid's coefficient records, queued on `stream`.  The caller has
// checked the grid (counts >= 1, their product <= 2^31 - 64: every record index fits 32 bits).  `shape`: kLightShape* or 0 =
// the default, or RB_LIGHT_SHAPE in the environment; *kernel_name, if asked for, names the kernel.  Returns a hipError_t.
int launch_probe_light(const ProbeLightArgs& a, uint32_t shape, void* stream_, const char** kernel_name) {
    if (a.m == 0u) return 0;
    if (a.coeffs == nullptr || a.points == nullptr || a.out == nullptr) return (int)hipErrorInvalidValue;
    if (a.grid.counts[0] == 0u || a.grid.counts[1] == 0u || a.grid.counts[2] == 0u) return (int)hipErrorInvalidValue;
    if (shape == 0u) {
        const char* env = std::getenv("RB_LIGHT_SHAPE");   // measurements: "pairs" | "wide"
        shape = env && env[0] == 'w' ? kLightShapeWide : env && env[0] == 'p' ? kLightShapePairs : kLightShapeDefault;
    }
    const dim3 blocks((a.m + 255u) / 256u);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (shape == kLightShapeWide) hipLaunchKernelGGL(k_probe_light_wide, blocks, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(k_probe_light, blocks, dim3(256), 0, stream, a);
    if (kernel_name) *kernel_name = shape == kLightShapeWide ? "k_probe_light_wide" : "k_probe_light";
    return (int)hipGetLastError();
}

}  // namespace rb
