// rb_device_math.hpp -- vec3, IEEE-exact fast reciprocal / division / sqrt, conversions, PCG RNG, colour output.
// Part of the single device translation unit rb_kernels.hip (numerics contract: see there).
#pragma once
#include "rb_device_common.hpp"

#pragma clang fp contract(off)

namespace rb {
namespace {

// ------------------------------------------------------------------ vec3 --
struct f3 {
    float x, y, z;
};
DEV f3 mk(float x, float y, float z) { return f3{x, y, z}; }
DEV f3 ld3(const float* p) { return f3{p[0], p[1], p[2]}; }
DEV f3 operator+(f3 a, f3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
DEV f3 operator-(f3 a, f3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
DEV f3 operator*(f3 a, f3 b) { return mk(a.x * b.x, a.y * b.y, a.z * b.z); }
DEV f3 operator*(float s, f3 a) { return mk(s * a.x, s * a.y, s * a.z); }
DEV f3 divs(f3 a, float s) { return mk(a.x / s, a.y / s, a.z / s); }
DEV float dot(f3 a, f3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
DEV f3 cross(f3 a, f3 b) { return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
DEV f3 div3_exact(f3 a, float b);
DEV float sqrt_exact(float x);
DEV f3 normalize(f3 a) { return div3_exact(a, sqrt_exact(dot(a, a))); }
// no component is an infinity or a NaN (rb_cast_rays' rule for a ray's origin and direction); every component is +-0
DEV bool finite3(f3 a) {
    const uint32_t m = 0x7F800000u;
    return (__float_as_uint(a.x) & m) != m && (__float_as_uint(a.y) & m) != m && (__float_as_uint(a.z) & m) != m;
}
DEV bool zero3(f3 a) { return a.x == 0.0f && a.y == 0.0f && a.z == 0.0f; }

// ---- IEEE-exact 1/b in 3-5 instructions instead of the 12-instruction a/b expansion.
// v_rcp_f32 is accurate to 1 ulp; one (RB_RCP_STEPS=1) or two Newton steps with FMA give the
// correctly rounded reciprocal for every significand except a few (e.g. all ones), which is a
// property of the significand alone as long as b and 1/b are normal.  Lanes outside
// [2^-100, 2^100] or with a significand the exhaustive device check (rb_debug_rcp_exhaustive,
// tests/test_gpu_parity.py::test_fast_reciprocal_is_exhaustively_exact) has not cleared fall back
// to the compiler's division, so the result is `1.0f / b` bit for bit in every case.
#ifndef RB_RCP_STEPS
#define RB_RCP_STEPS 1
#endif
#ifndef RB_FAST_RCP
#define RB_FAST_RCP 1
#endif
DEV float rcp_newton(float b) {
    float r = __builtin_amdgcn_rcpf(b);
    float e = __builtin_fmaf(-b, r, 1.0f);
    r = __builtin_fmaf(e, r, r);
#if RB_RCP_STEPS >= 2
    e = __builtin_fmaf(-b, r, 1.0f);
    r = __builtin_fmaf(e, r, r);
#endif
    return r;
}
DEV bool rcp_safe(float b) {
    const uint32_t x = __float_as_uint(b) & 0x7FFFFFFFu;
    // 2^-100 <= |b| < 2^100 and significand not all ones
    return (x - 0x0D800000u) < 0x64000000u && (x & 0x007FFFFFu) != 0x007FFFFFu;
}
DEV float rcp_exact(float b) {
#if RB_FAST_RCP
    if (rcp_safe(b)) return rcp_newton(b);
#endif
    return 1.0f / b;
}

// ---- IEEE-exact a/b from the exact reciprocal: q0 = RN(a*y), r = a - b*q0 (exact in an FMA),
// q = RN(q0 + r*y) with y = RN(1/b).  Whether q is the correctly rounded quotient depends only on
// the two significands while a, b, a/b and r stay clear of the subnormal range; the device check
// rb_debug_div_exhaustive walked ALL 2^23 x 2^23 significand pairs with zero mismatches
// (profiles/r01_div_exhaustive_2p46.log; sampled again by the test suite).  Used where one
// denominator serves three numerators (normalize), so the range checks amortise; anything
// outside the checked ranges takes the compiler's division, so results never change.
#ifndef RB_FAST_DIV
#define RB_FAST_DIV 1
#endif
DEV float div_newton(float a, float b, float y) {
    const float q0 = a * y;
    const float r = __builtin_fmaf(-b, q0, a);
    return __builtin_fmaf(r, y, q0);
}
// b in [2^-60, 2^60), significand not all ones
DEV bool div_safe_den(float b) {
    const uint32_t x = __float_as_uint(b) & 0x7FFFFFFFu;
    return (x - 0x21800000u) < 0x3C000000u && (x & 0x007FFFFFu) != 0x007FFFFFu;
}
// v / len for len = sqrt(dot(v, v)) (normalize).  len < 2^59 bounds every |component| below 2^60
// (anything larger would have made len infinite); a non-zero component must be >= 2^-100 in
// magnitude so that q0 and the exact remainder stay representable.  A zero numerator keeps its
// sign through the final copysign, which is also the sign of every non-zero quotient (len > 0).
DEV f3 div3_exact(f3 a, float b) {
#if RB_FAST_DIV
    // (x << 1) - 2 wraps a zero to 0xFFFFFFFE, so the unsigned minimum flags only 0 < |x| < 2^-100
    const uint32_t tx = (__float_as_uint(a.x) << 1) - 2u, ty = (__float_as_uint(a.y) << 1) - 2u,
                   tz = (__float_as_uint(a.z) << 1) - 2u;
    const bool num_ok = min(min(tx, ty), tz) >= (0x0D800000u << 1) - 2u;
    const uint32_t xb = __float_as_uint(b);  // b >= 0: sign bit clear unless -0 / NaN payloads
    const bool den_ok = (xb - 0x21800000u) < 0x3B800000u && (xb & 0x007FFFFFu) != 0x007FFFFFu;  // [2^-60, 2^59)
    if (num_ok && den_ok) {
        const float y = rcp_newton(b);
        const float qx = div_newton(a.x, b, y), qy = div_newton(a.y, b, y), qz = div_newton(a.z, b, y);
        return mk(__builtin_copysignf(qx, a.x), __builtin_copysignf(qy, a.y), __builtin_copysignf(qz, a.z));
    }
#endif
    return mk(a.x / b, a.y / b, a.z / b);
}
// ---- IEEE-exact sqrt without the subnormal / zero / infinity handling of the compiler's
// expansion: v_sqrt_f32 (1 ulp), then pick among s-1ulp, s, s+1ulp by the sign of the exact
// residuals x - s_lo*s and x - s_hi*s (the same selection the compiler emits).  Valid for
// x in [2^-60, 2^60); checked for all 2^23 significands at an even and an odd exponent by
// rb_debug_rcp_exhaustive (mode 1).  Everything else takes sqrtf.
#ifndef RB_FAST_SQRT
#define RB_FAST_SQRT 1
#endif
DEV float sqrt_newton(float x) {
    const float s = __builtin_amdgcn_sqrtf(x);
    const float s_lo = __uint_as_float(__float_as_uint(s) - 1u);
    const float s_hi = __uint_as_float(__float_as_uint(s) + 1u);
    const float r_lo = __builtin_fmaf(-s_lo, s, x);
    const float r_hi = __builtin_fmaf(-s_hi, s, x);
    float out = (r_lo <= 0.0f) ? s_lo : s;
    out = (r_hi > 0.0f) ? s_hi : out;
    return out;
}
DEV float sqrt_exact(float x) {
#if RB_FAST_SQRT
    if ((__float_as_uint(x) - 0x21800000u) < 0x3C000000u) return sqrt_newton(x);  // positive, [2^-60, 2^60)
#endif
    return sqrtf(x);
}

// ---- normalize for the kernels of single-node trees (k_trace and k_trace_direct with MULTI = false):
// normalize() bit for bit, with the guards of its two fast paths joined.  Each arm has a knob for the A/B builds of
// profiles/r27_c2_bench_ab.txt; with all three at 0 it carries the guards normalize() has.
//
// RB_NORM_ONE_RANGE -- one range test.  sqrt_exact's fast path takes L = dot(v, v) in [2^-60, 2^60) (bits 0x21800000 up to
//   0x5D800000).  The correctly rounded root of such an L lies in [2^-30, 2^30]: the square root is monotonic and 2^-30 and 2^30
//   are floats, so rounding cannot cross them.  div3_exact asks its denominator to lie in [2^-60, 2^59) (bits 0x21800000 up to
//   0x5D000000), which holds all of [2^-30, 2^30]: after the root's fast path the denominator's range test cannot fail and is
//   dropped.  What is left of that guard is the significand test of the reciprocal (all ones: not cleared by the exhaustive check).
// RB_NORM_MIN3_ABS -- the numerators by magnitude.  div3_exact lets a zero numerator through its fast path, which costs a shift
//   per component in front of the unsigned minimum and a copysign per quotient behind the division (a -0 comes out of
//   div_newton as +0).  Here the test is on min(|x|, |y|, |z|) as floats: a zero component fails it and takes the compiler's
//   division, which gives the same value, and a quotient of non-zero operands has its sign from the multiply, so the three
//   copysigns go as well.  The bound is 2^-30 where div3_exact needs 2^-100: with every |component| >= 2^-30 each square is at
//   least 2^-60 and so is L (rounding is monotonic), which makes the lower half of L's range test redundant; the upper half is
//   one float compare, L < 2^60.  A component in (0, 2^-30) now takes the compiler's path, same value.  A NaN component can pass
//   the minimum (the minimum of a NaN and a number is the number) but makes L a NaN, and an infinity makes L an infinity or a
//   NaN: neither is below 2^60.
// RB_NORM_UNIT -- the rejection loop's vector (UNIT = true) needs no range test.  A coordinate is RN(c * 2^-31 - 1) with
//   c = (float)seed in [0, 2^32]: a float in [-1, 1], and every float there is a multiple of 2^-24 or 0 -- c * 2^-31 - 1 reaches
//   no further down than that grid, since c * 2^-31 is a multiple of 2^-24 from c = 2^30 on, where the difference is exact, and
//   below it the difference is in [-1, -1/2], where floats are 2^-24 apart; so it is 0, or its magnitude is in [2^-24, 1].  An accepted point has
//   L = (xx + yy) + zz < 1 with every term 0 or >= 2^-48, all of them multiples of 2^-48 below 1: the sums are exact or round
//   on a coarser grid, and L is 0 -- only for the point (0, 0, 0) -- or in [2^-48, 1), inside the root's fast range.  (0, 0, 0)
//   needs three consecutive outputs of pcg that convert to c = 2^31, the seeds 2^31 - 64 .. 2^31 + 128; no seed in that window
//   is followed by another one (tests/test_normalize_ranges.py walks them), so L = 0 is never accepted.  s = RN(sqrt(L)) is in
//   [2^-24, 1).  div_newton's obligation is that operands, q0 and the remainder stay clear of the subnormal range: a numerator
//   is 0 (q0 = r = 0 exactly; the copysign, kept at this site, restores a -0) or in [2^-24, 1); y = RN(1 / s) in (1, 2^24];
//   q0 = RN(a * y) in [2^-24, 2^24]; r = a - s * q0 is a multiple of ulp(s) * ulp(q0) >= 2^-47 * 2^-47 = 2^-94, exact in the
//   fused multiply-add, zero or at least 2^-94 in magnitude; the quotient is within an ulp of q0.  Every input meets it.
#ifndef RB_NORM_ONE_RANGE
#define RB_NORM_ONE_RANGE 1
#endif
#ifndef RB_NORM_MIN3_ABS
#define RB_NORM_MIN3_ABS 1
#endif
#ifndef RB_NORM_UNIT
#define RB_NORM_UNIT 1
#endif
template <bool UNIT = false>
DEV f3 normalize_trim(f3 a) {
#if RB_FAST_DIV && RB_FAST_SQRT
    constexpr bool unit = UNIT && RB_NORM_UNIT != 0;
    const float L = dot(a, a);
    bool ok = true;   // L in the root's fast range, the numerators in the division's
    if constexpr (!unit) {
        if constexpr (RB_NORM_MIN3_ABS != 0) {
            ok = L < 0x1p60f && fminf(fminf(fabsf(a.x), fabsf(a.y)), fabsf(a.z)) >= 0x1p-30f;
        } else {
            ok = (__float_as_uint(L) - 0x21800000u) < 0x3C000000u;
            const uint32_t tx = (__float_as_uint(a.x) << 1) - 2u, ty = (__float_as_uint(a.y) << 1) - 2u, tz = (__float_as_uint(a.z) << 1) - 2u;
            ok = ok && min(min(tx, ty), tz) >= (0x0D800000u << 1) - 2u;
        }
    }
    float b;
    if (ok) b = sqrt_newton(L);
    else b = sqrtf(L);
    const uint32_t xb = __float_as_uint(b);
    bool fast = ok && (xb & 0x007FFFFFu) != 0x007FFFFFu;
    if constexpr (!unit && RB_NORM_ONE_RANGE == 0) fast = fast && (xb - 0x21800000u) < 0x3B800000u;
    if (fast) {
        const float y = rcp_newton(b);
        const float qx = div_newton(a.x, b, y), qy = div_newton(a.y, b, y), qz = div_newton(a.z, b, y);
        if constexpr (!unit && RB_NORM_MIN3_ABS != 0) return mk(qx, qy, qz);
        else return mk(__builtin_copysignf(qx, a.x), __builtin_copysignf(qy, a.y), __builtin_copysignf(qz, a.z));
    }
    return mk(a.x / b, a.y / b, a.z / b);
#else
    return normalize(a);
#endif
}
// TRIM selects it at compile time: the kernels that do not ask for it keep normalize() and the code they have.
template <bool TRIM, bool UNIT = false>
DEV f3 normalize_for(f3 a) {
    if constexpr (TRIM) return normalize_trim<UNIT>(a);
    else return normalize(a);
}

// 1/a for the triangle test: the reference rejects |a| < 1e-6 first (its reciprocal is never used),
// so only the upper range and the significand need checking.
DEV float rcp_tri(float a) {
#if RB_FAST_RCP
    const uint32_t x = __float_as_uint(a) & 0x7FFFFFFFu;
    if (x < 0x71800000u && (x & 0x007FFFFFu) != 0x007FFFFFu) return rcp_newton(a);
#endif
    return 1.0f / a;
}

// rcp_tri for the single-node walk's triangle loop (accept_slot), where its guard is issued for every lane of every trip: the
// same two ways to the same bits, chosen by two compares without a mask.  |a| < 2^100 as a float compare (the abs is an
// operand modifier; a NaN fails it and takes the division), and the low half of the bits not all ones as a 16-bit compare:
// that sends one significand in 65 536 to `1.0f / a` where rcp_tri sends one in 2^23, which is the value either way.  The
// 16-bit compare is written as the plain VOPC instruction on the register's low half: for `(uint16_t)bits != 0xFFFF` the
// compiler picks the SDWA form of the 32-bit compare, which measured slower than the two masks it replaces
// (profiles/r20_c2_bench_ab.txt).  Both lane masks are joined by the scalar unit and handed back as the branch's condition,
// so the exec mask is split once.  Checked against `1.0f / a` by rb_debug_rcp_det_exhaustive.
#ifndef RB_RCP_DET
#define RB_RCP_DET 1   // 0: accept_slot calls rcp_tri, for the A/B builds of profiles/r20_c2_bench_ab.txt
#endif
DEV float rcp_det(float a) {
#if RB_FAST_RCP && RB_RCP_DET
    uint64_t ones;
    asm("v_cmp_eq_u16_e64 %0, -1, %1" : "=s"(ones) : "v"(__float_as_uint(a)));
    const uint64_t large = __builtin_amdgcn_fcmpf(__builtin_fabsf(a), 0x1p100f, 11 /* FCMP_UGE: !(|a| < 2^100) */);
    if (__builtin_amdgcn_inverse_ballot_w64(large | ones)) return 1.0f / a;
    return rcp_newton(a);
#else
    return rcp_tri(a);
#endif
}

// WGSL u32(f32) / i32(f32): truncate + saturate, NaN -> 0
DEV uint32_t f2u(float f) {
    if (!(f > 0.0f)) return 0u;
    if (f >= 4294967296.0f) return 0xFFFFFFFFu;
    return (uint32_t)f;
}
DEV int32_t f2i(float f) {
    if (f != f) return 0;
    if (f >= 2147483648.0f) return 2147483647;
    if (f <= -2147483648.0f) return (int32_t)(-2147483647 - 1);
    return (int32_t)f;
}

// ------------------------------------------------------------------- RNG --
// shader.wgsl:417-421
DEV uint32_t pcg(uint32_t seed) {
    uint32_t state = seed * 747796405u + 2891336453u;
    uint32_t word = ((state >> ((state >> 28u) + 4u)) ^ state) * 277803737u;
    return (word >> 22u) ^ word;
}
// shader.wgsl:423-426
DEV float rnd(uint32_t& seed) {
    seed = pcg(seed);
    return (float)seed / 4294967296.0f;
}
// rnd(seed) * 2.0f - 1.0f in one rounding: with c = (float)seed that expression is RN(RN(RN(c * 2^-32) * 2) - 1); both scalings
// are exact (c is 0 or >= 1: nothing comes near the subnormal range), so it equals RN(c * 2^-31 - 1), one fma.  Checked for every
// float value c can take (tests/test_rnd_fused.py) and for all 2^32 seeds on the device (rb_debug_rnd_pm1_exhaustive).
DEV float rnd_pm1(uint32_t& seed) {
    seed = pcg(seed);
    return __builtin_fmaf((float)seed, 0x1p-31f, -1.0f);
}
// shader.wgsl:429-446.  The wave loops until its slowest lane has a vector.  A lane that has its vector does not sit the
// remaining rounds out: it goes on trying from the seed it is left with.  A rejected try has no effect but three hashes of the
// seed, so those may be run early; at the first accepted one the lane puts the seed back to where that try began and stops
// ("parks"), so the first try of its next call is the accepting one.  Every path draws the vectors it always drew; the wave
// runs fewer rounds (the model is tools/unit_vector_rounds.py).  PARK = false is the function as it was,
// three roundings per coordinate included, for a kernel whose register allocation must not move (k_trace_fast<true>).
#ifndef RB_PARK_SEED
#define RB_PARK_SEED 1   // 0: the plain loop around the fused try, for A/B builds (profiles/r15_c2_bench_ab.txt)
#endif
// TRIM: the accepted point goes through normalize_trim<true> (above), which needs none of normalize()'s range tests for it.
template <bool PARK = true, bool TRIM = false>
DEV f3 random_unit_vector(uint32_t& seed) {
    if constexpr (!PARK) {
        f3 p;
        for (;;) {
            const float px = rnd(seed) * 2.0f - 1.0f;
            const float py = rnd(seed) * 2.0f - 1.0f;
            const float pz = rnd(seed) * 2.0f - 1.0f;
            p = mk(px, py, pz);
            if (dot(p, p) < 1.0f) break;
        }
        return normalize(p);
    } else if constexpr (RB_PARK_SEED == 0) {
        float x, y, z;
        do {
            x = rnd_pm1(seed), y = rnd_pm1(seed), z = rnd_pm1(seed);
        } while (!(dot(mk(x, y, z), mk(x, y, z)) < 1.0f));
        return normalize(mk(x, y, z));
    } else {
        // The first try, which every lane is owed: nothing to select, nobody to park.  After it the two predicates are kept
        // one bit per lane in scalar register pairs -- who is still owed a vector, whose try landed inside the sphere -- so
        // that a round costs the vector unit the try and four selects (three coordinates and the seed) and nothing else.
        uint32_t s = seed;
        float x = rnd_pm1(s), y = rnd_pm1(s), z = rnd_pm1(s);
        uint64_t owed = __builtin_amdgcn_ballot_w64(!(dot(mk(x, y, z), mk(x, y, z)) < 1.0f));
        while (owed != 0ull) {
            uint32_t t = s;
            const float qx = rnd_pm1(t), qy = rnd_pm1(t), qz = rnd_pm1(t);
            const uint64_t inside = __builtin_amdgcn_ballot_w64(dot(mk(qx, qy, qz), mk(qx, qy, qz)) < 1.0f);
            const bool take = __builtin_amdgcn_inverse_ballot_w64(inside & owed);
            const bool park = __builtin_amdgcn_inverse_ballot_w64(inside & ~owed);
            x = take ? qx : x;
            y = take ? qy : y;
            z = take ? qz : z;
            s = park ? s : t;   // a parked lane stays in front of its accepting try, whatever rounds follow
            owed &= ~inside;
        }
        seed = s;
        return normalize_for<TRIM, true>(mk(x, y, z));
    }
}

// --------------------------------------------------------- colour output --
DEV float linear_to_gamma(float c) { return (c > 0.0f) ? sqrtf(c) : 0.0f; }  // :137-142
DEV uint32_t color_map(f3 c) {                                                // :144-151
    uint32_t r = f2u(linear_to_gamma(c.x) * 255.999f);
    uint32_t g = f2u(linear_to_gamma(c.y) * 255.999f);
    uint32_t b = f2u(linear_to_gamma(c.z) * 255.999f);
    return (255u << 24) | (b << 16) | (g << 8) | r;
}
DEV f3 hash_to_color(uint32_t n) {  // :394-400
    uint32_t h = n * 2654435761u;
    return mk((float)(h % 41u) / 40.0f, (float)(h % 29u) / 28.0f, (float)(h % 19u) / 18.0f);
}

}  // namespace
}  // namespace rb
