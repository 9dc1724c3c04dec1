// rb_probe_depth.hip -- the depth moments of irradiance probes made on the device (rb_bake_probe_depth, rb_probe_moments;
// DESIGN.md section 20, the normative definition): the first-hit distances of a probe's rays folded into its 8 x 8 octahedral
// map -- per texel the sums of r and r r, the samples and those that met a back face --, and the division that turns the sums
// into the moments the blend reads (rb_probe_visibility.hip).  The projection runs behind the kernels that answer the records
// (k_query*, rb_query.hip) over the generator's LINEAR order, in which one probe's records and hits are contiguous.  Same
// numerics contract as rb_kernels.hip: every step one binary32 operation in the order written, no FMA contraction, correctly
// rounded / and sqrt, so that renderbaby_amd/probes.py (depth_project, moments) equals this file bit for bit.
#include <cstdlib>

#include "rb_device_probe.hpp"

#pragma clang fp contract(off)

namespace rb {
namespace {

constexpr uint32_t kNoTexel = 64u;   // the texel of a sample that adds nothing: no lane's

// ====================================================== k_depth_project ====
// One wave per probe, lane = texel, the probe's samples in rows of 64.  Of a row each lane first takes ITS OWN sample -- the
// direction quad of the record, the first and the third quad of the hit, coalesced -- to the sample's texel and terms; then the
// row is folded in ascending sample order: at step j the lane that is sample j's texel, and no other, adds sample j's terms.
// Every sum so takes its samples in the definition's order whatever the fold's shape: LDS == true parks the row's terms in
// LDS, where all lanes read entry j at one address (a broadcast); LDS == false reads lane j's four words across into scalar
// registers (v_readlane).  The next row's loads are issued ahead of the current row's fold.
struct DepthRaw {
    v4f dir, h0, h2;   // {d, 0}; {t, kind, prim, mesh}; {normal, -}
};
DEV DepthRaw load_raw(const v4f* recs, const v4f* hits, size_t first, uint32_t k, uint32_t S) {
    DepthRaw r;
    r.dir = r.h0 = r.h2 = v4f{0.0f, 0.0f, 0.0f, 0.0f};   // a lane behind the probe's last sample: a zero direction, skipped
    if (k < S) {
        r.dir = __builtin_nontemporal_load(&recs[(first + k) * 2u + 1u]);
        r.h0 = __builtin_nontemporal_load(&hits[(first + k) * 3u]);
        r.h2 = __builtin_nontemporal_load(&hits[(first + k) * 3u + 2u]);
    }
    return r;
}

// {texel as bits, r, r r, back} of one sample
DEV v4f depth_term(const DepthRaw& s, float max_distance) {
    const f3 d = mk(s.dir.x, s.dir.y, s.dir.z);
    const uint32_t kind = __float_as_uint(s.h0.y);
    const bool skipped = zero3(d) || kind == 0xFFFFFFFFu /* RB_HIT_INVALID */;
    const uint32_t T = skipped ? kNoTexel : oct_texel(d.x, d.y, d.z);
    const float r = s.h0.x < max_distance ? s.h0.x : max_distance;
    const bool surface = kind == 2u /* RB_HIT_TRIANGLE */ || kind == 3u /* RB_HIT_SPHERE */;
    const float back = surface && dot(mk(s.h2.x, s.h2.y, s.h2.z), d) > 0.0f ? 1.0f : 0.0f;   // (sum + 0.0f leaves a sum's bits)
    return v4f{__uint_as_float(T), r, r * r, back};
}

template <bool LDS>
__global__ void __launch_bounds__(256) k_depth_project(const rb_ray* __restrict__ recs_, const rb_hit* __restrict__ hits_, uint32_t n, uint32_t S,
                                                       float max_distance, rb_probe_depth* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t probe = blockIdx.x * 4u + wave;
    if (probe >= n) return;   // (the whole wave; the waves of a block never wait for each other)
    v4f* row = nullptr;
    if constexpr (LDS) {
        __shared__ v4f park[4][64];
        row = park[wave];
    }
    const v4f* const recs = reinterpret_cast<const v4f*>(recs_);
    const v4f* const hits = reinterpret_cast<const v4f*>(hits_);
    const size_t first = (size_t)probe * S;   // n S <= 2^22 items: every index below fits

    float sum_r = 0.0f, sum_r2 = 0.0f, count = 0.0f, back = 0.0f;
    DepthRaw cur = load_raw(recs, hits, first, lane, S);
    for (uint32_t row0 = 0; row0 < S; row0 += 64u) {
        DepthRaw nxt = cur;
        if (S - row0 > 64u) nxt = load_raw(recs, hits, first, row0 + 64u + lane, S);
        const v4f mine = depth_term(cur, max_distance);
        const uint32_t rows = S - row0 < 64u ? S - row0 : 64u;
        if constexpr (LDS) {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();   // the row before has been read
            row[lane] = mine;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        const auto step = [&](uint32_t j) {   // j is wave-uniform
            v4f t;
            if constexpr (LDS) {
                t = row[j];
            } else {
                t = v4f{__int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine.x), (int)j)),
                        __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine.y), (int)j)),
                        __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine.z), (int)j)),
                        __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine.w), (int)j))};
            }
            const bool hit = __float_as_uint(t.x) == lane;
            sum_r = hit ? sum_r + t.y : sum_r;
            sum_r2 = hit ? sum_r2 + t.z : sum_r2;
            count = hit ? count + 1.0f : count;
            back = hit ? back + t.w : back;
        };
        if (rows == 64u) {
#pragma unroll 8
            for (uint32_t j = 0; j < 64u; j++) step(j);
        } else {   // the last row, or the only one
#pragma unroll 1
            for (uint32_t j = 0; j < rows; j++) step(j);
        }
        cur = nxt;
    }
    reinterpret_cast<v4f*>(out)[(size_t)probe * 64u + lane] = v4f{sum_r, sum_r2, count, back};   // the map: one 1-KiB store
}

// ====================================================== k_probe_moments ====
// One wave per probe, lane = texel.  The lane holds its texel before it writes, so `out` may be `sums`.  B and C take the
// texels in ascending order: 64 steps of two cross-lane reads and two adds, beside a kernel that moves 2 KiB per wave.
__global__ void __launch_bounds__(256) k_probe_moments(const rb_probe_depth* sums, uint32_t n, rb_probe_depth* out, float* share) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t probe = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (probe >= n) return;
    const v4f x = reinterpret_cast<const v4f*>(sums)[(size_t)probe * 64u + lane];
    const bool valid = x.z > 0.0f && x.z < __builtin_inff();   // finite and greater than 0; a NaN fails both
    const v4f zero = {0.0f, 0.0f, 0.0f, 0.0f}, m = {x.x / x.z, x.y / x.z, 1.0f, x.w / x.z};
    if (share != nullptr) {
        float B = 0.0f, C = 0.0f;
#pragma unroll 8
        for (int j = 0; j < 64; j++) {   // (all 64 at once would park 128 words in scalar registers and spill them)
            B = B + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x.w), j));
            C = C + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x.z), j));
        }
        if (lane == 0u) share[probe] = C == 0.0f ? 0.0f : B / C;
    }
    reinterpret_cast<v4f*>(out)[(size_t)probe * 64u + lane] = valid ? m : zero;
}

}  // namespace

// out[i] = the ordered sums of probe i < n of the piece, from the piece's records in linear order and the hits launch_query
// left for them (record and hit i * samples + k: sample k of probe i), queued on `stream`.  Returns a hipError_t.
int launch_depth_project(const rb_ray* recs, const rb_hit* hits, uint32_t n, uint32_t samples, float max_distance, rb_probe_depth* out,
                         uint32_t shape, void* stream_) {
    if (n == 0u) return 0;
    if (recs == nullptr || hits == nullptr || out == nullptr || samples == 0u) return (int)hipErrorInvalidValue;
    if (shape == 0u) {
        const char* env = std::getenv("RB_DEPTH_SHAPE");   // measurements: "lds" | "readlane"
        shape = env && env[0] == 'l' ? kDepthShapeLds : env && env[0] == 'r' ? kDepthShapeReadlane : kDepthShapeDefault;
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const dim3 blocks((n + 3u) / 4u);
    if (shape == kDepthShapeLds) hipLaunchKernelGGL(k_depth_project<true>, blocks, dim3(256), 0, stream, recs, hits, n, samples, max_distance, out);
    else hipLaunchKernelGGL(k_depth_project<false>, blocks, dim3(256), 0, stream, recs, hits, n, samples, max_distance, out);
    return (int)hipGetLastError();
}

// out[i] = the moments of sums[i], i < n, and share[i] (unless nullptr) its back-face share, queued on `stream`; out may be sums
int launch_probe_moments(const rb_probe_depth* sums, uint32_t n, rb_probe_depth* out, float* share, void* stream_) {
    if (n == 0u) return 0;
    if (sums == nullptr || out == nullptr) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_probe_moments, dim3((n + 3u) / 4u), dim3(256), 0, static_cast<hipStream_t>(stream_), sums, n, out, share);
    return (int)hipGetLastError();
}

}  // namespace rb
