// rb_debug.hip -- the kernels that render nothing: the exhaustive device checks of the exact-arithmetic helpers (rcp_newton,
// rcp_det, rnd_pm1, div_newton, normalize_trim), the triangle trip of k_trace against accept_slot, the device math the parity tests ask for, and
// the two measurement kernels (k_salu_mix, k_l1_gather) -- each with its launch and its C entry point, so that the hot-path
// translation unit (rb_kernels.hip) holds the render kernels alone.  They need nothing of the engine.
//
// Same numerics contract as rb_kernels.hip (same flags, same pragma): the checks compare with the arithmetic the render
// kernels are compiled to.
#include <algorithm>

#include "rb_device_shade.hpp"

#pragma clang fp contract(off)

namespace rb {
namespace {

// Exhaustive check of rcp_newton against the compiler's correctly rounded 1/b: every one of the
// 2^23 significands at biased exponent `expo`, both signs.  mismatch[0] counts differing results
// among rcp_safe inputs; mismatch[1..] records up to 15 offending bit patterns.
__global__ void k_rcp_exhaustive(uint32_t expo, uint32_t* mismatch) {
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= (1u << 23)) return;
    for (uint32_t sign = 0; sign < 2; sign++) {
        const uint32_t bits = (sign << 31) | ((expo & 0xFFu) << 23) | m;
        const float b = __uint_as_float(bits);
        float want, got;
        if (expo & 0x100u) {  // mode 1: sqrt (positive operands only)
            if (sign) continue;
            want = sqrtf(b);
            got = sqrt_exact(b);
        } else {
            if (!rcp_safe(b)) continue;
            want = 1.0f / b;
            got = rcp_newton(b);
        }
        if (__float_as_uint(want) != __float_as_uint(got)) {
            const uint32_t k = atomicAdd(&mismatch[0], 1u);
            if (k < 15u) mismatch[1u + k] = bits;
        }
    }
}

// Exhaustive check of rcp_det, guard and both of its ways, against the compiler's correctly rounded 1/b: every one of the
// 2^23 significands at biased exponent `expo`, both signs.  A NaN equals a NaN.  mismatch[0] counts differing results;
// mismatch[1..] records up to 15 offending bit patterns.
__global__ void k_rcp_det_exhaustive(uint32_t expo, uint32_t* mismatch) {
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= (1u << 23)) return;
    for (uint32_t sign = 0; sign < 2; sign++) {
        const uint32_t bits = (sign << 31) | ((expo & 0xFFu) << 23) | m;
        const float b = __uint_as_float(bits);
        const float want = 1.0f / b, got = rcp_det(b);
        if (__float_as_uint(want) != __float_as_uint(got) && !(want != want && got != got)) {
            const uint32_t k = atomicAdd(&mismatch[0], 1u);
            if (k < 15u) mismatch[1u + k] = bits;
        }
    }
}

// normalize_trim, both forms (rb_device_math.hpp: what k_trace and k_trace_direct normalize with), against the compiler's
// v / sqrt(dot(v, v)) with its correctly rounded / and sqrt.  Lanes [0, n): the general form on the caller's vectors.  Lanes
// [n, n + n_unit): the rejection loop's form on the caller's points, which must be ones the loop can accept.  Lanes behind
// them: the same form on the first try of random_unit_vector from seed0 + k, where that try is accepted.  A NaN equals a NaN.
// out[0..2] = differing vectors in the three ranges, out[3] = accepted tries, out[4] = 1 + the lane of one differing vector,
// out[5..7] = its components, out[8..10] = the form's result, out[11..13] = the compiler's.
DEV bool same_or_both_nan(float a, float b) { return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b); }
__global__ void k_normalize_sites(const float* __restrict__ xyz, uint32_t n, uint32_t n_unit, uint32_t seed0, uint32_t n_seeds, uint32_t* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n + n_unit + n_seeds) return;
    f3 v;
    uint32_t range = 0u;
    if (i < n + n_unit) {
        v = mk(xyz[3u * i], xyz[3u * i + 1u], xyz[3u * i + 2u]);
        range = i < n ? 0u : 1u;
    } else {
        uint32_t s = seed0 + (i - n - n_unit);
        const float x = rnd_pm1(s), y = rnd_pm1(s), z = rnd_pm1(s);
        v = mk(x, y, z);
        if (!(dot(v, v) < 1.0f)) return;
        atomicAdd(&out[3], 1u);
        range = 2u;
    }
    const f3 got = range == 0u ? normalize_trim<false>(v) : normalize_trim<true>(v);
    const float len = sqrtf(dot(v, v));
    const f3 want = mk(v.x / len, v.y / len, v.z / len);
    if (!(same_or_both_nan(got.x, want.x) && same_or_both_nan(got.y, want.y) && same_or_both_nan(got.z, want.z))) {
        if (atomicAdd(&out[range], 1u) == 0u && atomicExch(&out[4], i + 1u) == 0u) {
            out[5] = __float_as_uint(v.x), out[6] = __float_as_uint(v.y), out[7] = __float_as_uint(v.z);
            out[8] = __float_as_uint(got.x), out[9] = __float_as_uint(got.y), out[10] = __float_as_uint(got.z);
            out[11] = __float_as_uint(want.x), out[12] = __float_as_uint(want.y), out[13] = __float_as_uint(want.z);
        }
    }
}

// The triangle trip of k_trace (intersect_bvh<.., TRIP = true>: accept_trip; a build with RB_TRIP_ASM = 0 compares accept_slot<true>
// with itself) against the form every other caller keeps, accept_slot<true>, on the same (ray, triangle, incoming hit):
// {t, u, v, slot} afterwards, bit for bit.  The record is wave-uniform as in the walk (it reaches the trip in scalar registers),
// so a wave is one triangle and 64 rays.  Waves [0, n_waves) draw both from `seed`: rays aimed at and around the triangle, with
// scales that reach the determinant's guards now and then, and an incoming hit.t of 1e20 or near the triangle.  The waves
// behind them are the constructed cases, one per wave (trip_case), each lane one of four incoming hits -- 1e20, 0.5, the case's
// own t and the float above it -- with lanes 8..15 of every 16 switched off on entry, which must leave their hit as it came.
// mismatch[0] counts differing triples; mismatch[1] is the index of one and mismatch[2..] its 16 input and 8 output words.
// The root box of the single-node walk (rb_device_intersect.hpp, RB_ROOT_INSIDE): for n rays {o, d} and one box, the slab test as
// the walk runs it -- isect_aabb on rcp_exact's reciprocals -- and the rule that lets k_trace go past it, root_inside with
// box_finite.  out[i] = (slab test true ? 1 : 0) | (rule says "known" ? 2 : 0).  The box is a kernel argument: wave-uniform, as
// the node is in the walk.
__global__ void __launch_bounds__(256) k_root_box(const float* rays, uint32_t n, f3 bmin, f3 bmax, uint32_t* out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const f3 o = mk(rays[i * 6u], rays[i * 6u + 1u], rays[i * 6u + 2u]), d = mk(rays[i * 6u + 3u], rays[i * 6u + 4u], rays[i * 6u + 5u]);
    const bool slab = isect_aabb(o, mk(rcp_exact(d.x), rcp_exact(d.y), rcp_exact(d.z)), bmin, bmax);
    const bool known = root_inside(o, d, bmin, bmax) && box_finite(bmin, bmax);
    out[i] = (slab ? 1u : 0u) | (known ? 2u : 0u);
}

constexpr uint32_t kTripCases = 44u;
DEV void trip_case(uint32_t k, f3& o, f3& d, f3& v0, f3& e1, f3& e2) {
    // d = +z, e1 = (0, A, 0), e2 = (1, 0, 0), v0 = 0: every product with a zero is exact, so det = A, and with A = 1 the ray
    // from o has u = o.y, v = o.x, t = -o.z exactly
    o = mk(0.25f, 0.25f, -1.0f);
    d = mk(0.0f, 0.0f, 1.0f);
    v0 = mk(0.0f, 0.0f, 0.0f);
    e1 = mk(0.0f, 1.0f, 0.0f);
    e2 = mk(1.0f, 0.0f, 0.0f);
    const uint32_t eps = 0x358637BDu, big = 0x71800000u, one = 0x3F800000u, tmin = 0x3A83126Fu;   // 1e-6f, 2^100, 1, 0.001f
    const float nan = __uint_as_float(0x7FC00000u), inf = __uint_as_float(0x7F800000u);
    switch (k) {
        case 0: case 1: case 2: e1.y = __uint_as_float(eps - 1u + k); break;                  // |det| below, at, above 1e-6
        case 3: case 4: case 5: e1.y = -__uint_as_float(eps - 1u + (k - 3u)); break;
        case 6: case 7: case 8: e1.y = __uint_as_float(big - 1u + (k - 6u)); break;           // |det| below, at, above 2^100
        case 9: e1.y = -0x1p100f; break;
        case 10: e1.y = 0x1p120f; break;
        case 11: e1.y = __uint_as_float(0x3F80FFFFu); break;                                  // low 16 bits all ones
        case 12: e1.y = __uint_as_float(0xC123FFFFu); break;
        case 13: e1.y = __uint_as_float(0x3FFFFFFFu); break;                                  // the one significand rcp_tri excludes
        case 14: o.y = 0.0f; break;                                                           // u = 0, -0, 1, the floats around them
        case 15: o.y = -0.0f; break;
        case 16: o.y = -0x1p-149f; break;
        case 17: o.y = 1.0f; o.x = 0.0f; break;
        case 18: o.y = __uint_as_float(one + 1u); o.x = 0.0f; break;
        case 19: o.x = 0.0f; break;                                                           // v = 0, -0, below 0
        case 20: o.x = -0.0f; break;
        case 21: o.x = -0x1p-149f; break;
        case 22: o.x = 0.75f; break;                                                          // u + v = 1 and the float above
        case 23: o.x = 0.75f; o.y = __uint_as_float(0x3E800001u); break;
        case 24: o.z = -__uint_as_float(tmin); break;                                         // t = 0.001 and around, 0, below 0
        case 25: o.z = -__uint_as_float(tmin + 1u); break;
        case 26: o.z = -__uint_as_float(tmin - 1u); break;
        case 27: o.z = 0.0f; break;
        case 28: o.z = 1.0f; break;
        case 29: o.x = nan; break;                                                            // a NaN and an infinity in o and in d
        case 30: o.y = nan; break;
        case 31: o.z = nan; break;
        case 32: d.x = nan; break;
        case 33: d.y = nan; break;
        case 34: d.z = nan; break;
        case 35: o.x = inf; break;
        case 36: o.y = -inf; break;
        case 37: o.z = -inf; break;
        case 38: d.x = inf; break;
        case 39: d.y = -inf; break;
        case 40: d.z = inf; break;
        case 41: e1.y = 0.0f; break;                                                          // det = 0, a NaN and an infinite edge
        case 42: e1.y = nan; break;
        default: e2.x = inf; break;
    }
}
DEV float trip_unit(uint32_t& s) {   // [-1, 1)
    s = pcg(s);
    return (float)(int32_t)s * 0x1p-31f;
}
// FLAT (rb_debug_triangle_trip_flat): the flat kernels' trip, accept_trip<.., UV = false>, whose {t, slot} must be accept_slot<true>'s.
// VREC (rb_debug_triangle_trip_vec): the trip of the sift's pass 2, which takes the record and the slot in vector registers -- the
// same triples, handed over per lane.
template <bool FLAT, bool VREC>
DEV void trip_sweep(uint32_t n_waves, uint32_t seed, uint32_t* mismatch) {
    const uint32_t wave = (blockIdx.x * 256u + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (wave >= n_waves + kTripCases) return;
    f3 o, d, v0, e1, e2;
    float hit_t = 1e20f;
    bool on = true;
    if (wave < n_waves) {
        uint32_t sw = pcg(seed ^ (wave * 0x9E3779B9u)), sl = pcg(sw + lane * 0x85EBCA6Bu + 1u);
        const uint32_t kind = pcg(sw) & 15u;   // 0: tiny triangle (|det| around 1e-6), 1: huge (|det| >= 2^100), else ordinary
        const float scale = kind == 0u ? 0x1p-10f : kind == 1u ? 0x1p52f : 1.0f;
        v0 = mk(trip_unit(sw), trip_unit(sw), trip_unit(sw));
        e1 = scale * mk(trip_unit(sw), trip_unit(sw), trip_unit(sw));
        e2 = scale * mk(trip_unit(sw), trip_unit(sw), trip_unit(sw));
        o = 2.0f * mk(trip_unit(sl), trip_unit(sl), trip_unit(sl));
        const float a = 0.7f * trip_unit(sl) + 0.5f, b = 0.7f * trip_unit(sl) + 0.5f;        // in and around the triangle
        const f3 to = (v0 + a * e1 + b * e2) - o;
        d = __builtin_amdgcn_rsqf(dot(to, to) + 1e-30f) * to;
        const uint32_t r = pcg(sl);
        if (r & 1u) hit_t = 2.0f * (float)(r >> 8) * 0x1p-24f;
        on = (r & 6u) != 0u;   // a quarter of the lanes are off on entry
    } else {
        trip_case(wave - n_waves, o, d, v0, e1, e2);
        on = (lane & 8u) == 0u;
    }
    // the record as the walk hands it over: wave-uniform, in scalar registers
    auto uni = [](float x) { return __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(x))); };
    const v4f ra = {uni(v0.x), uni(v0.y), uni(v0.z), 0.0f}, rb_ = {uni(e1.x), uni(e1.y), uni(e1.z), 0.0f},
              rc = {uni(e2.x), uni(e2.y), uni(e2.z), 1.0f};
    const uint32_t slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)(wave + 1u));
    v4f va = {v0.x, v0.y, v0.z, 0.0f}, vb = {e1.x, e1.y, e1.z, 0.0f}, vc = {e2.x, e2.y, e2.z, 1.0f};
    uint32_t vslot = wave + 1u;
    if constexpr (VREC) asm volatile("" : "+v"(va.x), "+v"(va.y), "+v"(va.z), "+v"(vb.x), "+v"(vb.y), "+v"(vb.z), "+v"(vc.x), "+v"(vc.y), "+v"(vc.z), "+v"(vslot));
    if (wave >= n_waves) {
        TriHit own;
        own.t = 1e20f, own.u = 0.0f, own.v = 0.0f, own.slot = 0u, own.hit = false;
        accept_slot<true>(ra, rb_, rc, slot, o, d, own);
        const uint32_t v = lane & 3u;
        hit_t = v == 0u ? 1e20f : v == 1u ? 0.5f : v == 2u ? own.t : __uint_as_float(__float_as_uint(own.t) + 1u);
    }
    TriHit want, got;
    want.t = hit_t, want.u = -2.0f, want.v = -3.0f, want.slot = 0xABCDu, want.hit = false;
    got = want;
    float big = 0x1p100f;
    if constexpr (RB_TRIP_BLOCK) asm("s_mov_b32 %0, 0x71800000" : "=s"(big));
    if (on) {
        accept_slot<true>(ra, rb_, rc, slot, o, d, want);
        if constexpr (FLAT && RB_TRIP_BLOCK) {
            TriHitT<false> flat;
            flat.t = got.t, flat.slot = got.slot, flat.hit = false;
            if constexpr (VREC) accept_trip<RB_TRIP_ASM - 1, false, true>(va, vb, vc, vslot, o, d, big, flat);
            else accept_trip<RB_TRIP_ASM - 1, false>(ra, rb_, rc, slot, o, d, big, flat);
            got.t = flat.t, got.slot = flat.slot, got.u = want.u, got.v = want.v;   // no u, v to compare
        } else if constexpr (RB_TRIP_BLOCK && VREC) accept_trip<RB_TRIP_ASM - 1, true, true>(va, vb, vc, vslot, o, d, big, got);
        else if constexpr (RB_TRIP_BLOCK) accept_trip<RB_TRIP_ASM - 1>(ra, rb_, rc, slot, o, d, big, got);
        else accept_slot<true>(ra, rb_, rc, slot, o, d, got);
    }
    if (__float_as_uint(want.t) != __float_as_uint(got.t) || __float_as_uint(want.u) != __float_as_uint(got.u) ||
        __float_as_uint(want.v) != __float_as_uint(got.v) || want.slot != got.slot) {
        if (atomicAdd(&mismatch[0], 1u) == 0u) {
            mismatch[1] = wave * 64u + lane;
            const float in[16] = {o.x, o.y, o.z, d.x, d.y, d.z, ra.x, ra.y, ra.z, rb_.x, rb_.y, rb_.z, rc.x, rc.y, rc.z, hit_t};
            for (int k = 0; k < 16; k++) mismatch[2 + k] = __float_as_uint(in[k]);
            mismatch[18] = __float_as_uint(got.t), mismatch[19] = __float_as_uint(got.u), mismatch[20] = __float_as_uint(got.v);
            mismatch[21] = got.slot;
            mismatch[22] = __float_as_uint(want.t), mismatch[23] = __float_as_uint(want.u), mismatch[24] = __float_as_uint(want.v);
            mismatch[25] = want.slot;
        }
    }
}

template <bool FLAT>
__global__ void __launch_bounds__(256) k_triangle_trip(uint32_t n_waves, uint32_t seed, uint32_t* mismatch) {
    trip_sweep<FLAT, false>(n_waves, seed, mismatch);
}
template <bool FLAT>
__global__ void __launch_bounds__(256) k_triangle_trip_vec(uint32_t n_waves, uint32_t seed, uint32_t* mismatch) {
    trip_sweep<FLAT, true>(n_waves, seed, mismatch);
}

// Pass 1 of the triangle sift on the caller's rays (rb_debug_tri_filter): sift_ray and sift_block as k_trace_sift runs them, over
// the list [first, end) of the node and the table and region in p.  out[4 i + b] = ray i's candidate bits of block b.
__global__ void __launch_bounds__(256) k_tri_filter(const KParams p, const float* rays, uint32_t n, uint32_t first, uint32_t end, uint32_t* out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const f3 o = mk(rays[i * 6u], rays[i * 6u + 1u], rays[i * 6u + 2u]), d = mk(rays[i * 6u + 3u], rays[i * 6u + 4u], rays[i * 6u + 5u]);
    const SiftRay r = sift_ray(p, o, d);
    uint32_t ends = p.sift_block_ends, g0 = 0u, b = 0u;
    for (uint32_t base = first; base < end && b < 4u; base += 32u, ends >>= 8, b++) {
        const uint32_t g1 = ends & 0xFFu;
        out[i * 4u + b] = sift_block(p, r, d, g0, g1, (end - base < 32u) ? end - base : 32u);
        g0 = g1;
    }
    for (; b < 4u; b++) out[i * 4u + b] = 0u;   // blocks the list does not have
}

// What the scalar unit sustains next to the vector units (rb_measure_salu_mix, tools/salu_mix.py):
// every wave runs a loop of 64 independent v_fma_f32 in their two-operand encoding, v_fmac_f32 (16 registers, four rounds), with SALU scalar adds spread among each 16 of
// them -- four registers, so neighbours are independent -- and, with BRANCH, one s_cbranch_execz per 16 that is never taken
// (exec is never empty in a wave that runs).  The loop's own three scalar instructions come on top of the 4 * SALU.
// stamp[0..1]: the shader clock and the 100 MHz clock over the first wave's loop, for the clock the run had.
template <int SALU, bool BRANCH>
__global__ void __launch_bounds__(256, 8) k_salu_mix(uint32_t rounds, float c, float* sink, unsigned long long* stamp) {
    float v[16];
#pragma unroll
    for (int k = 0; k < 16; k++) v[k] = (float)(threadIdx.x + k) * 0x1p-20f;
    const float c2 = c * 0x1p-20f;   // an accumulator gains c * c2 a time: nothing overflows
    uint32_t s0 = rounds, s1 = rounds + 1u, s2 = rounds + 2u, s3 = rounds + 3u;
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
#define RB_MIX_F(k) "v_fmac_f32_e32 %" #k ", %[c], %[c2]\n\t"
#define RB_MIX_S(j) "s_add_u32 %[s" #j "], %[s" #j "], 1\n\t"
    // four vector instructions with 0 .. 4 scalar adds among them
#define RB_MIX_Q0(a, b, c, d) RB_MIX_F(a) RB_MIX_F(b) RB_MIX_F(c) RB_MIX_F(d)
#define RB_MIX_Q1(a, b, c, d) RB_MIX_F(a) RB_MIX_F(b) RB_MIX_S(0) RB_MIX_F(c) RB_MIX_F(d)
#define RB_MIX_Q2(a, b, c, d) RB_MIX_F(a) RB_MIX_S(0) RB_MIX_F(b) RB_MIX_F(c) RB_MIX_S(1) RB_MIX_F(d)
#define RB_MIX_Q3(a, b, c, d) RB_MIX_F(a) RB_MIX_S(0) RB_MIX_F(b) RB_MIX_S(1) RB_MIX_F(c) RB_MIX_S(2) RB_MIX_F(d)
#define RB_MIX_Q4(a, b, c, d) RB_MIX_F(a) RB_MIX_S(0) RB_MIX_F(b) RB_MIX_S(1) RB_MIX_F(c) RB_MIX_S(2) RB_MIX_F(d) RB_MIX_S(3)
#define RB_MIX_BR "s_cbranch_execz .Lmix_out_%=\n\t"
#define RB_MIX_GROUP(Q, BR) Q(0, 1, 2, 3) Q(4, 5, 6, 7) Q(8, 9, 10, 11) Q(12, 13, 14, 15) BR
#define RB_MIX_ASM(Q, BR)                                                                                                 \
    asm volatile(RB_MIX_GROUP(Q, BR) RB_MIX_GROUP(Q, BR) RB_MIX_GROUP(Q, BR) RB_MIX_GROUP(Q, BR) ".Lmix_out_%=:"          \
                 : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]), "+v"(v[8]), \
                   "+v"(v[9]), "+v"(v[10]), "+v"(v[11]), "+v"(v[12]), "+v"(v[13]), "+v"(v[14]), "+v"(v[15]), [s0] "+s"(s0), \
                   [s1] "+s"(s1), [s2] "+s"(s2), [s3] "+s"(s3)                                                            \
                 : [c] "v"(c), [c2] "v"(c2)                                                                                             \
                 : "scc")
    for (uint32_t r = rounds; r != 0u; r--) {
        if constexpr (BRANCH) {
            if constexpr (SALU == 0) RB_MIX_ASM(RB_MIX_Q0, RB_MIX_BR);
            else if constexpr (SALU == 4) RB_MIX_ASM(RB_MIX_Q1, RB_MIX_BR);
            else if constexpr (SALU == 8) RB_MIX_ASM(RB_MIX_Q2, RB_MIX_BR);
            else if constexpr (SALU == 12) RB_MIX_ASM(RB_MIX_Q3, RB_MIX_BR);
            else RB_MIX_ASM(RB_MIX_Q4, RB_MIX_BR);
        } else {
            if constexpr (SALU == 0) RB_MIX_ASM(RB_MIX_Q0, "");
            else if constexpr (SALU == 4) RB_MIX_ASM(RB_MIX_Q1, "");
            else if constexpr (SALU == 8) RB_MIX_ASM(RB_MIX_Q2, "");
            else if constexpr (SALU == 12) RB_MIX_ASM(RB_MIX_Q3, "");
            else RB_MIX_ASM(RB_MIX_Q4, "");
        }
    }
#undef RB_MIX_F
#undef RB_MIX_S
#undef RB_MIX_Q0
#undef RB_MIX_Q1
#undef RB_MIX_Q2
#undef RB_MIX_Q3
#undef RB_MIX_Q4
#undef RB_MIX_BR
#undef RB_MIX_GROUP
#undef RB_MIX_ASM
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    float acc = (float)(s0 ^ s1 ^ s2 ^ s3);
#pragma unroll
    for (int k = 0; k < 16; k++) acc += v[k];
    if (acc == 12345.678f) sink[0] = acc;   // keeps the loop's values alive
    if (blockIdx.x == 0u && threadIdx.x == 0u) {
        stamp[0] = t1 - t0;
        stamp[1] = r1 - r0;
    }
}

// Exhaustive check of rnd_pm1 against `rnd(seed) * 2.0f - 1.0f` (the shader's three roundings): all 2^32 seeds, 256 per
// thread of a 2^16 x 256 grid.  pcg is a bijection, so every word the conversion can meet is met.  mismatch[0] counts the
// seeds whose value or whose seed afterwards differs; mismatch[1..] records up to 15 of them.
__global__ void __launch_bounds__(256) k_rnd_pm1_exhaustive(uint32_t* mismatch) {
    const uint32_t first = blockIdx.x * 256u + threadIdx.x;   // < 2^24
    uint32_t bad = 0u, first_bad = 0u;
    for (uint32_t k = 0; k < 256u; k++) {
        const uint32_t seed = first + (k << 24);
        uint32_t sa = seed, sb = seed;
        const float want = rnd(sa) * 2.0f - 1.0f;
        const float got = rnd_pm1(sb);
        if (__float_as_uint(want) != __float_as_uint(got) || sa != sb) {
            if (bad == 0u) first_bad = seed;
            bad++;
        }
    }
    if (bad != 0u) {
        const uint32_t n = atomicAdd(&mismatch[0], bad);
        if (n < 15u) mismatch[1u + n] = first_bad;
    }
}

// Exhaustive check of div_newton: thread = one denominator significand (biased exponent eb),
// loop over `a_count` numerator significands starting at a_begin (biased exponent ea).
__global__ void k_div_exhaustive(uint32_t b_begin, uint32_t ea, uint32_t eb, uint32_t a_begin, uint32_t a_count,
                                 unsigned long long* mismatch) {
    const uint32_t mb = b_begin + blockIdx.x * blockDim.x + threadIdx.x;
    if (mb >= (1u << 23)) return;
    const float b = __uint_as_float((eb << 23) | mb);
    if (!div_safe_den(b)) return;
    const float y = rcp_newton(b);
    unsigned long long bad = 0;
    uint32_t first_bad = 0;
    for (uint32_t i = 0; i < a_count; i++) {
        const float a = __uint_as_float((ea << 23) | ((a_begin + i) & 0x7FFFFFu));
        const float want = a / b;
        const float got = div_newton(a, b, y);
        if (__float_as_uint(want) != __float_as_uint(got)) {
            if (bad == 0) first_bad = __float_as_uint(a);
            bad++;
        }
    }
    if (bad) {
        const unsigned long long k = atomicAdd(&mismatch[0], bad);
        if (k < 7ull) {
            mismatch[1 + 2 * k] = first_bad;
            mismatch[2 + 2 * k] = __float_as_uint(b);
        }
    }
}

// Ceiling of the L1 / texture-address path, measured where the bench runs: every lane gathers 16 bytes from its own
// pseudo-random 128-byte line of a table that fits in L2 (the access pattern of a lane-per-ray tree walk), eight
// or sixteen independent loads in flight per lane.  A wave instruction then costs 64 L1 accesses (rocprofv3 counts
// TCP_TOTAL_CACHE_ACCESSES = 1.000 per lane load on it: profiles/r03_l1_ceiling.txt); accesses per second = the number
// the mesh kernels' TCP_TOTAL_CACHE_ACCESSES rate is compared with (bench.py, roofline.l1).
template <int INFLIGHT>
__global__ void __launch_bounds__(256) k_l1_gather(const float4* __restrict__ table, uint32_t lines_mask, uint32_t rounds, float4* sink) {
    // per-lane line sequence: an odd stride through the table (every line visited, no two lanes of a wave on one line
    // while the table has >= 64 lines), piece = lane & 7; one multiply-add per load keeps the address arithmetic out of the way
    const uint32_t lane_id = blockIdx.x * 256u + threadIdx.x;
    uint32_t line = lane_id * 2654435761u;
    const uint32_t step = (lane_id * 40503u) | 1u;
    const uint32_t piece = lane_id & 7u;
    float4 acc = make_float4(0, 0, 0, 0);
    for (uint32_t r = 0; r < rounds; r++) {
        float4 v[INFLIGHT];
#pragma unroll
        for (int k = 0; k < INFLIGHT; k++) {
            line += step;
            v[k] = table[(size_t)(line & lines_mask) * 8u + piece];
        }
#pragma unroll
        for (int k = 0; k < INFLIGHT; k++) acc.x += v[k].x, acc.y += v[k].y, acc.z += v[k].z, acc.w += v[k].w;
    }
    if (acc.x == 12345.678f) sink[0] = acc;   // never true for the zero-filled table: keeps the loads alive
}

// Exposes the device's /, sqrt, normalize and u32->f32 to the parity tests.
__global__ void k_debug_math(const float* a, const float* b, float* out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = a[i], y = b[i];
    out[i] = x / y;
    out[n + i] = sqrtf(fabsf(x));
    const f3 v = normalize(mk(x, y, x * y));
    out[2 * n + i] = v.x;
    out[3 * n + i] = v.y;
    out[4 * n + i] = v.z;
    out[5 * n + i] = (float)__float_as_uint(x) / 4294967296.0f;
    out[6 * n + i] = fminf(fmaxf(x, y), x * 0.0f);
    out[7 * n + i] = dot(mk(x, y, x), mk(y, y, x));
}

// The device round trip of a test hook: `bytes` of zeroed device memory, the launch, a wait, and the first out_bytes copied
// out.  One allocation, so nothing is left behind when it fails.
template <class T, class Launch>
int round_trip(T* out, size_t out_bytes, size_t bytes, Launch&& launch) {
    T* d = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&d), bytes) != hipSuccess) return RB_ERR_DEVICE;
    (void)hipMemset(d, 0, bytes);
    launch(d);
    const hipError_t rc = hipGetLastError(), st = hipDeviceSynchronize();
    (void)hipMemcpy(out, d, out_bytes, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    return (rc != hipSuccess || st != hipSuccess) ? RB_ERR_DEVICE : RB_OK;
}

// out[0] = shader clocks per vector instruction and SIMD (8 waves on each), out[1] = the shader clock in GHz the first wave saw,
// out[2] = the launch's milliseconds; the better of two launches.  scalar_per_16 in {0, 4, 8, 12, 16}.  false on failure.
bool measure_salu_mix(uint32_t scalar_per_16, bool branch, uint32_t rounds, double out[3]) {
    float* sink = nullptr;
    unsigned long long* stamp = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&sink), 16) != hipSuccess) return false;
    if (hipMalloc(reinterpret_cast<void**>(&stamp), 16) != hipSuccess) { (void)hipFree(sink); return false; }
    hipEvent_t t0, t1;
    (void)hipEventCreate(&t0);
    (void)hipEventCreate(&t1);
    const uint32_t blocks = device_cu_count_cached() * 8u;   // 4 waves a block: 8 waves on every SIMD
    float best = 0.0f;
    unsigned long long st[2] = {0, 0};
    bool ok = true;
    for (int rep = 0; rep < 3 && ok; rep++) {   // the first launch warms up
        (void)hipEventRecord(t0, nullptr);
#define RB_MIX_LAUNCH(S)                                                                                                         \
    if (branch) hipLaunchKernelGGL((k_salu_mix<S, true>), dim3(blocks), dim3(256), 0, nullptr, rounds, 0.5f, sink, stamp);      \
    else hipLaunchKernelGGL((k_salu_mix<S, false>), dim3(blocks), dim3(256), 0, nullptr, rounds, 0.5f, sink, stamp)
        switch (scalar_per_16) {
            case 0u: RB_MIX_LAUNCH(0); break;
            case 4u: RB_MIX_LAUNCH(4); break;
            case 8u: RB_MIX_LAUNCH(8); break;
            case 12u: RB_MIX_LAUNCH(12); break;
            case 16u: RB_MIX_LAUNCH(16); break;
            default: ok = false; break;
        }
#undef RB_MIX_LAUNCH
        (void)hipEventRecord(t1, nullptr);
        if (!ok || hipGetLastError() != hipSuccess || hipEventSynchronize(t1) != hipSuccess) { ok = false; break; }
        float ms = 0.0f;
        (void)hipEventElapsedTime(&ms, t0, t1);
        if (rep > 0 && ms > 0.0f && (best == 0.0f || ms < best)) {
            best = ms;
            (void)hipMemcpy(st, stamp, 16, hipMemcpyDeviceToHost);
        }
    }
    (void)hipEventDestroy(t0);
    (void)hipEventDestroy(t1);
    (void)hipFree(sink);
    (void)hipFree(stamp);
    if (!ok || best <= 0.0f || st[1] == 0ull) return false;
    const double ghz = (double)st[0] / (double)st[1] * 0.1;   // the second counter runs at 100 MHz
    out[0] = (best * 1e-3) * (ghz * 1e9) / ((double)rounds * 64.0 * 8.0);
    out[1] = ghz;
    out[2] = best;
    return true;
}

// -> lane accesses per second (0 on failure): the best of a few shapes (8 or 16 loads in flight per lane, 4 or 8 waves
// per SIMD); table_bytes is rounded down to a power of two >= 8 KiB
double measure_l1_gather(size_t table_bytes, uint32_t rounds) {
    size_t lines = 64;
    while (lines * 2 * 128 <= table_bytes) lines *= 2;
    float4 *table = nullptr, *sink = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&table), lines * 128) != hipSuccess) return 0.0;
    if (hipMalloc(reinterpret_cast<void**>(&sink), 16) != hipSuccess) { (void)hipFree(table); return 0.0; }
    (void)hipMemset(table, 0, lines * 128);
    hipEvent_t t0, t1;
    (void)hipEventCreate(&t0);
    (void)hipEventCreate(&t1);
    double best = 0.0;
    for (int shape = 0; shape < 4; shape++) {
        const uint32_t inflight = (shape & 1) ? 16u : 8u, blocks = device_cu_count_cached() * ((shape & 2) ? 8u : 4u);
        for (int rep = 0; rep < 2; rep++) {
            (void)hipEventRecord(t0, nullptr);
            if (inflight == 16u) hipLaunchKernelGGL(k_l1_gather<16>, dim3(blocks), dim3(256), 0, nullptr, table, (uint32_t)(lines - 1), rounds, sink);
            else hipLaunchKernelGGL(k_l1_gather<8>, dim3(blocks), dim3(256), 0, nullptr, table, (uint32_t)(lines - 1), rounds, sink);
            (void)hipEventRecord(t1, nullptr);
            if (hipEventSynchronize(t1) != hipSuccess) break;
            float ms = 0.0f;
            (void)hipEventElapsedTime(&ms, t0, t1);
            if (ms > 0.0f) best = std::max(best, (double)blocks * 256.0 * rounds * inflight / (ms * 1e-3));
        }
    }
    (void)hipEventDestroy(t0);
    (void)hipEventDestroy(t1);
    (void)hipFree(table);
    (void)hipFree(sink);
    return best;
}
}  // namespace

// rb_debug_tri_filter's device half (rb_runtime.cpp has the engine): n rays of six floats each, four mask words per ray out
int debug_tri_filter(const KParams& p, const float* rays, uint32_t n, uint32_t first, uint32_t end, uint32_t* out) {
    const size_t out_bytes = (size_t)n * 16u, in_bytes = (size_t)n * 24u;   // one buffer: the result words, then the rays
    return round_trip(out, out_bytes, out_bytes + in_bytes, [&](uint32_t* d) {
        float* dr = reinterpret_cast<float*>(d + (size_t)n * 4u);
        (void)hipMemcpy(dr, rays, in_bytes, hipMemcpyHostToDevice);
        hipLaunchKernelGGL(k_tri_filter, dim3((n + 255u) / 256u), dim3(256), 0, nullptr, p, dr, n, first, end, d);
    });
}
}  // namespace rb

extern "C" {

// Test hook: exhaustive device check of the fast reciprocal (all 2^23 significands, both signs)
// at one biased exponent.  out16[0] = number of mismatches, out16[1..15] = offending bit patterns.
int rb_debug_rcp_exhaustive(uint32_t biased_exponent, uint32_t* out16) {
    if (!out16) return RB_ERR_NULL_ARGUMENT;
    return rb::round_trip(out16, 64, 64, [&](uint32_t* d) {
        hipLaunchKernelGGL(rb::k_rcp_exhaustive, dim3((1u << 23) / 256), dim3(256), 0, nullptr, biased_exponent, d);
    });
}

// Test hook: the same sweep for rcp_det, the reciprocal of the single-node walk's triangle test, guard included: every
// significand and both signs at one biased exponent against `1.0f / x`, bit patterns compared (a NaN equals a NaN).
int rb_debug_rcp_det_exhaustive(uint32_t biased_exponent, uint32_t* out16) {
    if (!out16) return RB_ERR_NULL_ARGUMENT;
    if (biased_exponent > 255u) return RB_ERR_INVALID_OPTIONS;
    return rb::round_trip(out16, 64, 64, [&](uint32_t* d) {
        hipLaunchKernelGGL(rb::k_rcp_det_exhaustive, dim3((1u << 23) / 256), dim3(256), 0, nullptr, biased_exponent, d);
    });
}

// Test hook: the triangle trip of k_trace / k_trace_direct against the form the other kernels keep (accept_slot<true>) on n
// seeded (ray, triangle, incoming hit) triples and the constructed edge cases behind them (k_triangle_trip).
// out32[0] = number of triples whose {t, u, v, slot} differ in any bit, out32[1] = the index of one, out32[2..17] its
// o, d, v0, edge1, edge2 and incoming hit.t, out32[18..21] the trip's {t, u, v, slot}, out32[22..25] accept_slot's.
int rb_debug_triangle_trip(uint32_t n, uint32_t seed, uint32_t* out32) {
    if (!out32) return RB_ERR_NULL_ARGUMENT;
    if (n > (1u << 26)) return RB_ERR_INVALID_OPTIONS;
    return rb::round_trip(out32, 128, 128, [&](uint32_t* d) {
        const uint32_t n_waves = (n + 63u) / 64u, waves = n_waves + rb::kTripCases;
        hipLaunchKernelGGL(rb::k_triangle_trip<false>, dim3((waves + 3u) / 4u), dim3(256), 0, nullptr, n_waves, seed, d);
    });
}

// Test hook: the same sweep for the trip of k_trace_flat / k_trace_flat_direct, which carries {t, slot}: those two words against
// accept_slot<true>'s.  out32 as above (the u, v words repeat accept_slot's).
int rb_debug_triangle_trip_flat(uint32_t n, uint32_t seed, uint32_t* out32) {
    if (!out32) return RB_ERR_NULL_ARGUMENT;
    if (n > (1u << 26)) return RB_ERR_INVALID_OPTIONS;
    return rb::round_trip(out32, 128, 128, [&](uint32_t* d) {
        const uint32_t n_waves = (n + 63u) / 64u, waves = n_waves + rb::kTripCases;
        hipLaunchKernelGGL(rb::k_triangle_trip<true>, dim3((waves + 3u) / 4u), dim3(256), 0, nullptr, n_waves, seed, d);
    });
}

// Test hook: the same sweep for the trip of the sift's pass 2 (k_trace_sift), which takes the record in vector registers; `uv`
// nonzero: the form that carries u, v.  out32 as above.
int rb_debug_triangle_trip_vec(uint32_t n, uint32_t seed, uint32_t uv, uint32_t* out32) {
    if (!out32) return RB_ERR_NULL_ARGUMENT;
    if (n > (1u << 26)) return RB_ERR_INVALID_OPTIONS;
    return rb::round_trip(out32, 128, 128, [&](uint32_t* d) {
        const uint32_t n_waves = (n + 63u) / 64u, waves = n_waves + rb::kTripCases;
        if (uv) hipLaunchKernelGGL(rb::k_triangle_trip_vec<false>, dim3((waves + 3u) / 4u), dim3(256), 0, nullptr, n_waves, seed, d);
        else hipLaunchKernelGGL(rb::k_triangle_trip_vec<true>, dim3((waves + 3u) / 4u), dim3(256), 0, nullptr, n_waves, seed, d);
    });
}

// Test hook: the root box of the single-node walk on the caller's n rays (six floats each: o, d) and box (bmin, bmax): the slab
// test on the walk's own reciprocals and the rule k_trace skips it by (k_root_box).  out[i] = slab | known << 1.
int rb_debug_root_box(const float* rays, uint32_t n, const float* box6, uint32_t* out) {
    if (!rays || !box6 || !out) return RB_ERR_NULL_ARGUMENT;
    if (n == 0u) return RB_OK;
    if (n > (1u << 24)) return RB_ERR_INVALID_OPTIONS;
    const size_t out_bytes = (size_t)n * 4u, in_bytes = (size_t)n * 24u;   // one buffer: the n result words, then the rays
    const rb::f3 bmin = {box6[0], box6[1], box6[2]}, bmax = {box6[3], box6[4], box6[5]};
    return rb::round_trip(out, out_bytes, out_bytes + in_bytes, [&](uint32_t* d) {
        float* dr = reinterpret_cast<float*>(d + n);
        (void)hipMemcpy(dr, rays, in_bytes, hipMemcpyHostToDevice);
        hipLaunchKernelGGL(rb::k_root_box, dim3((n + 255u) / 256u), dim3(256), 0, nullptr, dr, n, bmin, bmax, d);
    });
}

// Test hook: the normalize of k_trace / k_trace_direct (normalize_trim, general and unit-vector form) against the compiler's
// v / sqrt(dot(v, v)) on the caller's vectors and on the accepted first tries of n_seeds seeds (k_normalize_sites).
int rb_debug_normalize_sites(const float* xyz, uint32_t n, uint32_t n_unit, uint32_t seed0, uint32_t n_seeds, uint32_t* out16) {
    if (!out16 || (!xyz && n + n_unit != 0u)) return RB_ERR_NULL_ARGUMENT;
    if (n > (1u << 26) || n_unit > (1u << 26) || n_seeds > (1u << 26)) return RB_ERR_INVALID_OPTIONS;
    const size_t total = (size_t)n + n_unit + n_seeds, in_bytes = ((size_t)n + n_unit) * 12u;
    if (total == 0u) {
        std::fill(out16, out16 + 16, 0u);
        return RB_OK;
    }
    return rb::round_trip(out16, 64, 64 + in_bytes, [&](uint32_t* d) {   // one buffer: the 16 result words, then the vectors
        float* dv = reinterpret_cast<float*>(d + 16);
        if (in_bytes) (void)hipMemcpy(dv, xyz, in_bytes, hipMemcpyHostToDevice);
        hipLaunchKernelGGL(rb::k_normalize_sites, dim3((uint32_t)((total + 255u) / 256u)), dim3(256), 0, nullptr, dv, n, n_unit, seed0, n_seeds, d);
    });
}

// Measurement aid (tools/salu_mix.py): what a vector instruction costs with scalar ones among them (k_salu_mix).
int rb_measure_salu_mix(int32_t device, uint32_t scalar_per_16, uint32_t branch, double* out3) {
    if (!out3) return RB_ERR_NULL_ARGUMENT;
    if (scalar_per_16 > 16u || (scalar_per_16 & 3u) != 0u) return RB_ERR_INVALID_OPTIONS;
    int before = -1;
    if (device >= 0 && (hipGetDevice(&before) != hipSuccess || hipSetDevice(device) != hipSuccess)) return RB_ERR_DEVICE;
    const bool ok = rb::measure_salu_mix(scalar_per_16, branch != 0u, 4096u, out3);
    if (before >= 0) (void)hipSetDevice(before);   // the caller's device is current again
    return ok ? RB_OK : RB_ERR_DEVICE;
}

// Test hook: device check of the one-rounding form of `rnd(seed) * 2 - 1` (rnd_pm1) against the three-operation form on all
// 2^32 seeds.  out16[0] = number of differing seeds, out16[1..15] = some of them.
int rb_debug_rnd_pm1_exhaustive(uint32_t* out16) {
    if (!out16) return RB_ERR_NULL_ARGUMENT;
    return rb::round_trip(out16, 64, 64, [&](uint32_t* d) {
        hipLaunchKernelGGL(rb::k_rnd_pm1_exhaustive, dim3(1u << 16), dim3(256), 0, nullptr, d);
    });
}

// Test hook: device check of the fast exact division over denominators [b_begin, b_begin+b_count)
// x numerators [a_begin, a_begin+a_count) (significands; biased exponents ea / eb).
// out16[0] = mismatch count, then up to 7 (a, b) bit-pattern pairs.
int rb_debug_div_exhaustive(uint32_t b_begin, uint32_t b_count, uint32_t ea, uint32_t eb, uint32_t a_begin,
                            uint32_t a_count, unsigned long long* out16) {
    if (!out16) return RB_ERR_NULL_ARGUMENT;
    return rb::round_trip(out16, 128, 128, [&](unsigned long long* d) {
        hipLaunchKernelGGL(rb::k_div_exhaustive, dim3((b_count + 255) / 256), dim3(256), 0, nullptr, b_begin, ea, eb, a_begin, a_count, d);
    });
}

int rb_measure_l1_gather(int32_t device, uint64_t table_bytes, double* accesses_per_s) {
    if (!accesses_per_s) return RB_ERR_NULL_ARGUMENT;
    if (device >= 0 && hipSetDevice(device) != hipSuccess) return RB_ERR_DEVICE;
    *accesses_per_s = rb::measure_l1_gather(table_bytes ? static_cast<size_t>(table_bytes) : (2u << 20), 512u);
    return *accesses_per_s > 0.0 ? RB_OK : RB_ERR_DEVICE;
}

// Debug hook for tests/test_gpu_parity.py: device /, sqrt, normalize, u32->f32, min/max, dot.
int rb_debug_math(const float* a, const float* b, float* out8n, uint32_t n) {
    if (!a || !b || !out8n) return RB_ERR_NULL_ARGUMENT;
    if (n == 0) return RB_OK;
    const size_t n4 = static_cast<size_t>(n) * 4;   // one buffer: the 8 n results, then a, then b
    return rb::round_trip(out8n, 8 * n4, 10 * n4, [&](float* d) {
        float *da = d + 8 * static_cast<size_t>(n), *db = da + n;
        (void)hipMemcpy(da, a, n4, hipMemcpyHostToDevice);
        (void)hipMemcpy(db, b, n4, hipMemcpyHostToDevice);
        hipLaunchKernelGGL(rb::k_debug_math, dim3((n + 255) / 256), dim3(256), 0, nullptr, da, db, d, n);
    });
}

}  // extern "C"
