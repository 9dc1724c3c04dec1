// rb_hemisphere.hip -- hemisphere rays made on the device (rb_hemisphere_rays, rb_trace_hemisphere, rb_openness_hemisphere;
// DESIGN.md section 16, the normative definition): the cosine-weighted ray of every (surfel, sample) item from the item's own
// random stream -- two draws, sincos_turn for the azimuth, the branch-free tangent frame of Duff et al. 2017 --, and the count
// of the any-hit bytes of a surfel's samples.  One full-width pass, one lane per item, before the kernels that walk the records
// (k_cam*, rb_radiance.hip; k_occl*, rb_query.hip), as k_cam_rays is (section 15.4).  Same numerics contract as rb_kernels.hip:
// every step one binary32 operation in the order written, no FMA contraction, correctly rounded / and sqrt, so that
// renderbaby_amd/hemisphere.py equals this file bit for bit.
#include "rb_device_sincos.hpp"

#pragma clang fp contract(off)

namespace rb {
namespace {

// ========================================================= k_hemi_rays ====
// lane = item.  Item order (the trace's scratch): item = (block * samples + sample) * 64 + surfel-in-block, block = 64
// consecutive surfels of the piece -- the order the k_cam kernels hand items out in, so a wave's 64 records are one contiguous
// 2 KiB and its 64 surfels another.  Linear order (rb_hemisphere_rays, openness): item = surfel-in-piece * samples + sample.
// Every lane makes its surfel's frame itself (section 16.4: the lanes of a wave are 64 different surfels in item order, so
// sharing it would take LDS and a barrier across the block's waves to save a division, a square root and two dozen multiplies
// beside 64 B of record traffic per item).
__global__ void __launch_bounds__(256) k_hemi_rays(const HemiGenArgs g) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const GenItem it = gen_item(t, g.samples, g.linear);
    const uint32_t sf = it.idx, smp = it.smp;
    if (sf >= g.n) return;   // the padding of the last block, and the lanes behind the last item

    const v4f* const sp = reinterpret_cast<const v4f*>(g.surfels) + (size_t)sf * 2u;
    const v4f s0 = sp[0], s1 = sp[1];
    const f3 pos = mk(s0.x, s0.y, s0.z);
    const f3 nrm = normalize(mk(s1.x, s1.y, s1.z));
    bool ok = finite3(pos) && finite3(nrm) && !zero3(nrm);

    const uint32_t sid = g.ids != nullptr ? g.ids[sf] : g.id_base + sf;
    uint32_t seed = pcg(sid + pcg(g.first_sample + smp));
    const float u1 = rnd(seed), u2 = rnd(seed);
    const SinCos az = sincos_turn(u1 * 2.0f - 1.0f);
    const float r = sqrt_exact(u2), z = sqrt_exact(1.0f - u2);

    // Duff et al. 2017, "Building an Orthonormal Basis, Revisited": |sg + nrm.z| >= 1
    const float sg = __builtin_copysignf(1.0f, nrm.z);
    const float a = -1.0f / (sg + nrm.z);
    const float b = (nrm.x * nrm.y) * a;
    const f3 t1 = mk(1.0f + (sg * (nrm.x * nrm.x)) * a, sg * b, (-sg) * nrm.x);
    const f3 t2 = mk(b, sg + (nrm.y * nrm.y) * a, -nrm.y);
    f3 d = normalize(((r * az.c) * t1 + (r * az.s) * t2) + z * nrm);

    const float reach = sqrt_exact((pos.x * pos.x + pos.y * pos.y) + pos.z * pos.z);
    f3 o = pos + (g.offset * fmaxf(1.0f, reach)) * nrm;
    // rb_cast_rays' rule.  An invalid item is marked by a zero direction and keeps the surfel's position as it was given: a
    // NaN made here has no defined sign or payload and stays out of the record.
    ok = ok && finite3(o) && finite3(d) && !zero3(d);
    if (!ok) {
        o = pos;
        d = mk(0, 0, 0);
    }

    store_record(g.recs, g.seeds, t, o, d, seed);
    if (g.tmax != nullptr) g.tmax[t] = g.radius;
}

// ========================================================= k_hemi_count ====
// lane = surfel: the any-hit bytes of its `samples` items (linear order) -> {open, valid}.  A count, so nothing depends on the
// order or the launch shape.  Rows whose length is a multiple of 4 are read a word at a time (the scratch is 256-byte aligned).
__global__ void __launch_bounds__(256) k_hemi_count(const uint8_t* __restrict__ occl, uint32_t n, uint32_t samples, rb_openness* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint8_t* const row = occl + (size_t)i * samples;
    uint32_t open = 0u, valid = 0u;
    if ((samples & 3u) == 0u) {
        const uint32_t* const w = reinterpret_cast<const uint32_t*>(row);
        for (uint32_t k = 0; k < samples / 4u; k++) {
            const uint32_t x = w[k];
            for (uint32_t j = 0; j < 32u; j += 8u) {
                const uint32_t v = (x >> j) & 255u;
                open += v == (uint32_t)RB_OCCL_VISIBLE ? 1u : 0u;
                valid += v != (uint32_t)RB_OCCL_INVALID ? 1u : 0u;
            }
        }
    } else {
        for (uint32_t k = 0; k < samples; k++) {
            const uint32_t v = row[k];
            open += v == (uint32_t)RB_OCCL_VISIBLE ? 1u : 0u;
            valid += v != (uint32_t)RB_OCCL_INVALID ? 1u : 0u;
        }
    }
    const uint2 res = {open, valid};
    reinterpret_cast<uint2*>(out)[i] = res;
}

}  // namespace

// One piece: every record of it, queued on `stream`; nothing is waited for.  Item order: g.n surfels, rounded up to whole
// blocks of 64 (the records of the padding are not written, the trace kernels do not read them); linear order: g.n surfels'
// g.n * samples items.
int launch_hemisphere_rays(const HemiGenArgs& g, void* stream_) {
    if (g.n == 0u) return 0;
    if (g.surfels == nullptr || g.recs == nullptr || g.samples == 0u) return (int)hipErrorInvalidValue;
    if (g.linear == 0u && (g.seeds != nullptr || g.tmax != nullptr)) return (int)hipErrorInvalidValue;
    const uint64_t lanes = gen_lanes(g.n, g.samples, g.linear);
    if (lanes == 0u) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_hemi_rays, dim3((uint32_t)((lanes + 255u) / 256u)), dim3(256), 0, static_cast<hipStream_t>(stream_), g);
    return (int)hipGetLastError();
}

// out[i] = {open, valid} of the result bytes occl[i * samples .. (i + 1) * samples), i < n
int launch_hemisphere_count(const uint8_t* occl, uint32_t n, uint32_t samples, rb_openness* out, void* stream_) {
    if (n == 0u) return 0;
    if (occl == nullptr || out == nullptr || samples == 0u) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_hemi_count, dim3((n + 255u) / 256u), dim3(256), 0, static_cast<hipStream_t>(stream_), occl, n, samples, out);
    return (int)hipGetLastError();
}

}  // namespace rb
