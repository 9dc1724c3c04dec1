// rb_probe_light.hip -- light points from a baked probe grid on the device (rb_probe_coefficients, rb_light_points; DESIGN.md
// section 19, the normative definition): the SH9 sums of rb_bake_probes scaled to irradiance-over-pi coefficients, and the blend
// of the eight probes round a point of a regular grid, each probe's coefficients dotted with the basis of the point's normal.
// Same numerics contract as rb_kernels.hip: every step one binary32 operation in the order written, no FMA contraction,
// correctly rounded / and sqrt, so that renderbaby_amd/probes.py (coefficients, light) equals this file bit for bit.
#include <cstdlib>

#include "rb_device_probe.hpp"

#pragma clang fp contract(off)

namespace rb {
namespace {

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
// probe_light_body (rb_device_probe.hpp) without the visibility weights.
// The two shapes differ in how many corners' loads the compiler may keep in flight, that is in the registers a lane holds
// against the waves that share a SIMD: "pairs" -- the corners in groups of two, the two records that lie side by side in
// memory, 82 registers, five waves --, "wide" -- all eight corners' 56 loads issued before the first use, 243 registers, two
// waves (section 19.4 has the measurement that chose).
__global__ void __launch_bounds__(256) k_probe_light(const ProbeLightArgs a) { probe_light_body<2, false>(a, ProbeVisArgs{}); }
__global__ void __launch_bounds__(256) k_probe_light_wide(const ProbeLightArgs a) { probe_light_body<8, false>(a, ProbeVisArgs{}); }

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
