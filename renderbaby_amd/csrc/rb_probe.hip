// rb_probe.hip -- irradiance probes made on the device (rb_probe_rays, rb_bake_probes; DESIGN.md section 18, the normative
// definition): the uniform-sphere ray of every (probe, sample) item from the item's own random stream -- two draws, sincos_turn
// for the azimuth, z uniform in [-1, 1], world axes --, and the projection of a piece's traced colours onto the nine real
// spherical harmonics of bands 0-2 of each item's own direction.  The generator runs before the kernels that walk the records
// (k_cam*, rb_radiance.hip), as k_hemi_rays does (section 16); the projection runs behind them on the colour scratch k_rad_sum
// reads.  Same numerics contract as rb_kernels.hip: every step one binary32 operation in the order written, no FMA contraction,
// correctly rounded / and sqrt, so that renderbaby_amd/probes.py equals this file bit for bit.
#include <cstdlib>

#include "rb_device_sh.hpp"
#include "rb_device_sincos.hpp"

#pragma clang fp contract(off)

namespace rb {
namespace {

// ======================================================== k_probe_rays ====
// lane = item, in k_hemi_rays' two orders.  Item order (the trace's scratch): item = (block * samples + sample) * 64 +
// probe-in-block, block = 64 consecutive probes of the piece.  Linear order (rb_probe_rays): item = probe-in-piece * samples +
// sample.  The record is k_cam_rays': {origin, seed after the two draws}, {direction, 0}, or the seed beside it.
__global__ void __launch_bounds__(256) k_probe_rays(const ProbeGenArgs g) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const GenItem it = gen_item(t, g.samples, g.linear);
    const uint32_t pr = it.idx, smp = it.smp;
    if (pr >= g.n) return;   // the padding of the last block, and the lanes behind the last item

    const v4f p0 = reinterpret_cast<const v4f*>(g.probes)[pr];
    const f3 pos = mk(p0.x, p0.y, p0.z);

    const uint32_t sid = g.ids != nullptr ? g.ids[pr] : g.id_base + pr;
    uint32_t seed = pcg(sid + pcg(g.first_sample + smp));
    const float u1 = rnd(seed), u2 = rnd(seed);
    const SinCos az = sincos_turn(u1 * 2.0f - 1.0f);
    const float z = 1.0f - (u2 + u2);
    const float r = sqrt_exact(1.0f - z * z);   // |z| <= 1: the radicand is >= 0
    f3 d = normalize(mk(r * az.c, r * az.s, z));

    // rb_cast_rays' rule; an invalid item keeps the probe's position as it was given beside a zero direction
    if (!(finite3(pos) && finite3(d) && !zero3(d))) d = mk(0, 0, 0);

    store_record(g.recs, g.seeds, t, pos, d, seed);
}

// ======================================================== k_sh_project ====
// Shaped like k_rad_sum: a block of 64 probes per wavefront, lane = probe, so a sample row is a contiguous 1 KiB of colours and
// 2 KiB of records.  k_sh_project: one wave per block of probes folds all nine coefficients (27 sums and the weight).
// k_sh_project_split: three waves per block of probes, wave g folds coefficients 3g .. 3g + 2 and the last one the weight --
// three times the waves for reading the rows three times (section 18.4 has the measurement that chose).  Every sum starts at
// +0 and takes its samples in ascending order, one multiply and one add each, whichever wave holds it.
// The basis is sh_basis (rb_device_sh.hpp) of the direction AS STORED in the record.
// the sums of coefficients J0 .. J0 + COEFS - 1 of block `blk`'s probes on the calling wave; the weight goes with coefficient 8
template <int J0, int COEFS>
DEV void sh_project_body(const float* __restrict__ colors, const rb_ray* __restrict__ recs, uint32_t n, uint32_t S, rb_sh9* __restrict__ out,
                         uint32_t blk, uint32_t lane) {
    const uint32_t probe = blk * 64u + lane;
    if (probe >= n) return;
    const size_t row0 = ((size_t)blk * S) * 64u + lane;
    const nt_f4* __restrict__ c = reinterpret_cast<const nt_f4*>(colors) + row0;
    const nt_f4* __restrict__ d = reinterpret_cast<const nt_f4*>(recs) + row0 * 2u + 1u;
    float acc[COEFS][3];
#pragma unroll
    for (int j = 0; j < COEFS; j++) acc[j][0] = acc[j][1] = acc[j][2] = 0.0f;
    float w = 0.0f;
    auto fold = [&](const nt_f4 v, const nt_f4 dir) {
        const ShBasis b = sh_basis(dir.x, dir.y, dir.z);   // (the terms this wave does not fold are dead code)
#pragma unroll
        for (int j = 0; j < COEFS; j++) {
            const float yj = b.y[J0 + j];
            acc[j][0] = acc[j][0] + v.x * yj;
            acc[j][1] = acc[j][1] + v.y * yj;
            acc[j][2] = acc[j][2] + v.z * yj;
        }
        w = w + v.w;
    };
    uint32_t s = 0;
    for (; s + 8u <= S; s += 8u) {
        nt_f4 v[8], dir[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            v[k] = __builtin_nontemporal_load(&c[(size_t)(s + k) * 64u]);
            dir[k] = __builtin_nontemporal_load(&d[(size_t)(s + k) * 128u]);
        }
#pragma unroll
        for (int k = 0; k < 8; k++) fold(v[k], dir[k]);
    }
    for (; s < S; s++) fold(__builtin_nontemporal_load(&c[(size_t)s * 64u]), __builtin_nontemporal_load(&d[(size_t)s * 128u]));

    float* const o = reinterpret_cast<float*>(out + probe) + J0 * 3;
#pragma unroll
    for (int j = 0; j < COEFS; j++) {
        o[j * 3 + 0] = acc[j][0];
        o[j * 3 + 1] = acc[j][1];
        o[j * 3 + 2] = acc[j][2];
    }
    if (J0 + COEFS == 9) o[COEFS * 3] = w;
}

__global__ void __launch_bounds__(256) k_sh_project(const float* __restrict__ colors, const rb_ray* __restrict__ recs, uint32_t n, uint32_t S,
                                                    rb_sh9* __restrict__ out) {
    sh_project_body<0, 9>(colors, recs, n, S, out, blockIdx.x * 4u + (threadIdx.x >> 6), threadIdx.x & 63u);
}

__global__ void __launch_bounds__(192) k_sh_project_split(const float* __restrict__ colors, const rb_ray* __restrict__ recs, uint32_t n, uint32_t S,
                                                          rb_sh9* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    switch (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) {   // wave-uniform
        case 0: sh_project_body<0, 3>(colors, recs, n, S, out, blockIdx.x, lane); break;
        case 1: sh_project_body<3, 3>(colors, recs, n, S, out, blockIdx.x, lane); break;
        default: sh_project_body<6, 3>(colors, recs, n, S, out, blockIdx.x, lane); break;
    }
}

}  // namespace

// One piece: every record of it, queued on `stream`; nothing is waited for.  Item order: g.n probes, rounded up to whole blocks
// of 64 (the records of the padding are not written, neither the trace kernels nor the projection read them); linear order:
// g.n probes' g.n * samples items.
int launch_probe_rays(const ProbeGenArgs& g, void* stream_) {
    if (g.n == 0u) return 0;
    if (g.probes == nullptr || g.recs == nullptr || g.samples == 0u) return (int)hipErrorInvalidValue;
    if (g.linear == 0u && g.seeds != nullptr) return (int)hipErrorInvalidValue;
    const uint64_t lanes = gen_lanes(g.n, g.samples, g.linear);
    if (lanes == 0u) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_probe_rays, dim3((uint32_t)((lanes + 255u) / 256u)), dim3(256), 0, static_cast<hipStream_t>(stream_), g);
    return (int)hipGetLastError();
}

// out[i] = the ordered sums of probe i < n of the piece, from the colour scratch launch_radiance filled ([block of 64][sample][64])
// and the piece's records in item order.  `shape`: kProbeShape* or 0 = the default, or RB_PROBE_SHAPE in the environment.
int launch_sh_project(const float* colors, const rb_ray* recs, uint32_t n, uint32_t samples, rb_sh9* out, uint32_t shape, void* stream_) {
    if (n == 0u) return 0;
    if (colors == nullptr || recs == nullptr || out == nullptr || samples == 0u) return (int)hipErrorInvalidValue;
    if (shape == 0u) {
        const char* env = std::getenv("RB_PROBE_SHAPE");   // measurements: "plain" | "split"
        shape = env && env[0] == 's' ? kProbeShapeSplit : env && env[0] == 'p' ? kProbeShapePlain : kProbeShapeDefault;
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const uint32_t blocks64 = (n + 63u) / 64u;
    if (shape == kProbeShapeSplit) hipLaunchKernelGGL(k_sh_project_split, dim3(blocks64), dim3(192), 0, stream, colors, recs, n, samples, out);
    else hipLaunchKernelGGL(k_sh_project, dim3((blocks64 + 3u) / 4u), dim3(256), 0, stream, colors, recs, n, samples, out);
    return (int)hipGetLastError();
}

}  // namespace rb
