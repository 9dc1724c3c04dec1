// rb_device_intersect.hpp -- textures, primitive intersection tests, work counters, BVH walks (reference order, fast tree, sphere tree).
// Part of the single device translation unit rb_kernels.hip (numerics contract: see there).
#pragma once
#include "rb_device_math.hpp"

#pragma clang fp contract(off)

namespace rb {
namespace {

// -------------------------------------------------------------- textures --
// shader.wgsl:153-191.  pow(c, 2.2) over the 256 possible channel values is a
// host-computed table (same libm as the oracle), so textured hits stay bit-exact.
// TEXEL = false (the flat kernels, k_trace_flat / k_trace_flat_direct; DESIGN.md section 4, "Scenes that carry no u, v"): the
// launch has established that no material a segment can sample carries an index >= 0, so the texel way is not compiled and
// the index is not looked at.
template <bool TEXEL = true>
DEV f3 sample_texture(const KParams& p, int32_t index, float uvx, float uvy) {
    if (!TEXEL || index < 0) {
        if (p.u.checkerboard_enabled > 0u) {
            int32_t u2 = f2i(floorf(uvx * 10.0f));
            int32_t v2 = f2i(floorf(uvy * 10.0f));
            int32_t sum = (int32_t)((uint32_t)u2 + (uint32_t)v2);
            return (sum % 2 == 0) ? ld3(p.u.checkerboard_color_1) : ld3(p.u.checkerboard_color_2);
        }
        return mk(1.0f, 1.0f, 1.0f);
    }
    if ((uint32_t)index >= p.n_tex) return mk(0.0f, 0.0f, 0.0f);
    const v4u iw = ((cu4p)p.tex_info)[index];
    rb_texture_info info;
    info.offset = iw.x;
    info.width = iw.y;
    info.height = iw.z;
    float u = uvx - floorf(uvx);
    float v = uvy - floorf(uvy);
    uint32_t x = min(f2u(u * (float)info.width), info.width - 1u);
    uint32_t y = min(f2u((1.0f - v) * (float)info.height), info.height - 1u);
    const uint32_t pixel = cptr(p.tex_data)[info.offset + y * info.width + x];
    const RB_CONST float* lut = cptr(p.srgb_lut);
    return mk(lut[pixel & 255u], lut[(pixel >> 8) & 255u], lut[(pixel >> 16) & 255u]);
}

// ---------------------------------------------------------- intersection --
// shader.wgsl:193-215 / :217-239
DEV float isect_sphere(f3 o, f3 d, float a, f3 center, float radius) {
    f3 oc = o - center;
    float half_b = dot(oc, d);
    float c = dot(oc, oc) - radius * radius;
    float disc = half_b * half_b - a * c;
    if (disc < 0.0f) return -1.0f;
    float sqrtd = sqrtf(disc);
    float root = (-half_b - sqrtd) / a;
    if (root <= 0.001f) {
        root = (-half_b + sqrtd) / a;
        if (root <= 0.001f) return -1.0f;
    }
    return root;
}

// shader.wgsl:248-280 with edge1/edge2 supplied (v1 - v0, v2 - v0).  (A branch-free form that evaluates
// everything and folds the four early returns into one predicate was measured slower on gfx950, 34.8 vs
// 33.5 ms on C2-short: the early-outs do skip whole-wave work.  tools/ablate/rb_forks.patch.)
DEV float isect_triangle(f3 o, f3 d, f3 v0, f3 edge1, f3 edge2, float& uo, float& vo) {
    const f3 h = cross(d, edge2);
    const float a = dot(edge1, h);
    if (fabsf(a) < 1e-6f) return -1.0f;
    const float f = rcp_tri(a);
    const f3 s = o - v0;
    const float u = f * dot(s, h);
    if (u < 0.0f || u > 1.0f) return -1.0f;
    const f3 q = cross(s, edge1);
    const float v = f * dot(d, q);
    if (v < 0.0f || u + v > 1.0f) return -1.0f;
    const float t = f * dot(edge2, q);
    if (t > 0.0f) {
        uo = u;
        vo = v;
        return t;
    }
    return -1.0f;
}

// shader.wgsl:664-671 with inv_dir = 1/dir hoisted per ray (pure function of dir)
DEV bool isect_aabb(f3 o, f3 inv, f3 bmin, f3 bmax) {
    f3 t0 = (bmin - o) * inv;
    f3 t1 = (bmax - o) * inv;
    float tmin = fmaxf(fmaxf(fminf(t0.x, t1.x), fminf(t0.y, t1.y)), fminf(t0.z, t1.z));
    float tmax = fminf(fminf(fmaxf(t0.x, t1.x), fmaxf(t0.y, t1.y)), fmaxf(t0.z, t1.z));
    return tmax >= fmaxf(tmin, 0.0f);
}

// The root box of the single-node walk without its slab test (k_trace / k_trace_direct; DESIGN.md section 4, "The root box
// where a ray starts inside it").  RB_ROOT_INSIDE = 0 gives the slab test in every segment, as before r29.
#ifndef RB_ROOT_INSIDE
#define RB_ROOT_INSIDE 1
#endif
// The rule: an origin strictly inside [bmin, bmax] in all three components and a direction without a NaN component make
// isect_aabb(o, 1 / d, bmin, bmax) true, if the box's six bounds are finite (box_finite; they are wave-uniform, so that part is
// scalar work).  Every compare is ordered: a NaN anywhere says "not known".  v_cmp_o takes two components at a time.
// The bounds must be wave-uniform.
// (the largest of the six magnitudes' bit patterns, as integers: written with float compares it becomes six vector compares)
DEV bool box_finite(f3 bmin, f3 bmax) {
    const uint32_t m = 0x7FFFFFFFu;
    // (... and the empty asm statements keep each maximum a scalar one: three at a time they are matched to v_max3_u32)
    uint32_t a = max(__float_as_uint(bmin.x) & m, __float_as_uint(bmin.y) & m);
    asm("" : "+s"(a));
    a = max(a, __float_as_uint(bmin.z) & m);
    asm("" : "+s"(a));
    a = max(a, __float_as_uint(bmax.x) & m);
    asm("" : "+s"(a));
    a = max(a, __float_as_uint(bmax.y) & m);
    asm("" : "+s"(a));
    a = max(a, __float_as_uint(bmax.z) & m);
    asm("" : "+s"(a));
    return a < 0x7F800000u;
}
// root_inside_mask: the wave's lanes for which the per-lane part holds, as a lane mask (0 for a lane that is off).  The compares
// are asked for as masks so that they are joined with scalar instructions and tested as one word: as bools, the compiler turns
// the joined bool back into a 0 / 1 register and compares that once more.  2 = ordered >, 4 = ordered <, 7 = ordered.
DEV uint64_t root_inside_mask(f3 o, f3 d, f3 bmin, f3 bmax) {
    return __builtin_amdgcn_fcmpf(o.x, bmin.x, 2) & __builtin_amdgcn_fcmpf(o.x, bmax.x, 4) & __builtin_amdgcn_fcmpf(o.y, bmin.y, 2) &
           __builtin_amdgcn_fcmpf(o.y, bmax.y, 4) & __builtin_amdgcn_fcmpf(o.z, bmin.z, 2) & __builtin_amdgcn_fcmpf(o.z, bmax.z, 4) &
           __builtin_amdgcn_fcmpf(d.x, d.y, 7) & __builtin_amdgcn_fcmpf(d.z, d.z, 7);
}
DEV bool root_inside(f3 o, f3 d, f3 bmin, f3 bmax) { return ((root_inside_mask(o, d, bmin, bmax) >> __lane_id()) & 1ull) != 0ull; }
// What a lane knows about its ray and the root box before the segment starts: nothing, or the slab test's answer that
// ColorRing::stage_row worked out for the primary ray it was handed in this iteration's refill.
constexpr uint32_t kBoxUnknown = 0u, kBoxMiss = 1u, kBoxHit = 2u;

// shader.wgsl:402-414
DEV float isect_ground(f3 o, f3 d, float ground_height) {
    if (fabsf(d.y) < 1e-6f) return -1.0f;
    float t = (ground_height - o.y) / d.y;
    return (t > 0.0f) ? t : -1.0f;
}

// ------------------------------------------------------------ statistics --
template <bool STATS>
struct Tally {
    uint32_t segments = 0, paths = 0;
    unsigned long long nodes = 0, tris = 0, spheres = 0, lights = 0, mesh_hits = 0;
};
template <>
struct Tally<false> {
    uint32_t segments = 0, paths = 0;
};

DEV unsigned long long wave_sum(unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
template <bool STATS>
DEV void flush_tally(const Tally<STATS>& t, unsigned long long* counters) {
    unsigned long long seg = wave_sum((unsigned long long)t.segments);
    unsigned long long pth = wave_sum((unsigned long long)t.paths);
    const bool lead = (__lane_id() == 0);
    if (lead) {
        atomicAdd(&counters[C_SEGMENTS], seg);
        atomicAdd(&counters[C_PATHS], pth);
    }
    if constexpr (STATS) {
        unsigned long long a = wave_sum(t.nodes), b = wave_sum(t.tris), c = wave_sum(t.spheres),
                           d = wave_sum(t.lights), e = wave_sum(t.mesh_hits);
        if (lead) {
            atomicAdd(&counters[C_NODES], a);
            atomicAdd(&counters[C_TRIS], b);
            atomicAdd(&counters[C_SPHERES], c);
            atomicAdd(&counters[C_LIGHTS], d);
            atomicAdd(&counters[C_MESH_HITS], e);
        }
    }
}

// -------------------------------------------------------- BVH traversal --
// UV = false: the winner without its barycentrics, for the flat kernels, whose scenes never read them (tri_uv is their only reader)
template <bool UV>
struct TriHitT {
    float t, u, v;
    uint32_t slot;  // position in bvh_indices (prepared-triangle index)
    bool hit;
};
template <>
struct TriHitT<false> {
    float t;
    uint32_t slot;
    bool hit;
};
using TriHit = TriHitT<true>;

// shader.wgsl:282-392.  Same visit order (left pushed first, right popped first),
// same strict `t > 0.001 && t < hit.t` acceptance, so the winner is the same
// triangle.  Shading data of shader.wgsl:350-372 depends only on the final
// winner and is produced afterwards (tri_shade).  `stack` is this lane's column
// of an LDS array [kStackDepth][blockDim]; the host has verified that the tree
// fits (rb_bvh.cpp).
template <bool UV>   // (false: never run -- the flat kernels have no multi-node walk -- but intersect_bvh's text below them is compiled)
DEV void test_slot(const v4f a, const v4f b, const v4f c, uint32_t slot, f3 o, f3 d, TriHitT<UV>& h) {
    float u, v;
    const float t = isect_triangle(o, d, mk(a.x, a.y, a.z), mk(b.x, b.y, b.z), mk(c.x, c.y, c.z), u, v);
    if (t > 0.001f && t < h.t) {
        h.hit = true;
        h.t = t;
        if constexpr (UV) {
            h.u = u;
            h.v = v;
        }
        h.slot = slot;
    }
}

// test_slot for the wave-uniform triangle list of the single-node walk (intersect_bvh): isect_triangle's operations on the
// same operands in the same order and test_slot's acceptance (|a| >= 1e-6, 0 <= u <= 1, v >= 0, u + v <= 1, t > 0,
// t > 0.001, t < h.t, all as written there, so a NaN takes the same way), but the hit is taken where t is computed:
// no -1 is handed back through the four early-outs to be compared with 0.001 and h.t once more.  hit.hit is left alone:
// carried through the loop it is a lane mask in two scalar registers that every join of the early-outs merges again;
// the caller sets it once from hit.t, which leaves its initial 1e20 exactly when a triangle is accepted (t < hit.t).
// DET: 1/det through rcp_det's two-compare guard (the kernels of single-node trees); false keeps rcp_tri, same bits, so that
// the register allocation of the multi-node kernels, which carry this loop too, does not move.
template <bool DET = false>
DEV void accept_slot(const v4f a, const v4f b, const v4f c, uint32_t slot, f3 o, f3 d, TriHit& hit) {
    const f3 v0 = mk(a.x, a.y, a.z), edge1 = mk(b.x, b.y, b.z), edge2 = mk(c.x, c.y, c.z);
    const f3 h = cross(d, edge2);
    const float det = dot(edge1, h);
    if (!(fabsf(det) < 1e-6f)) {
        const float f = DET ? rcp_det(det) : rcp_tri(det);
        const f3 s = o - v0;
        const float u = f * dot(s, h);
        if (!(u < 0.0f || u > 1.0f)) {
            const f3 q = cross(s, edge1);
            const float v = f * dot(d, q);
            if (!(v < 0.0f || u + v > 1.0f)) {
                const float t = f * dot(edge2, q);
                if (t > 0.0f && t > 0.001f && t < hit.t) {
                    hit.t = t;
                    hit.u = u;
                    hit.v = v;
                    hit.slot = slot;
                }
            }
        }
    }
}

// The triangle trip of k_trace / k_trace_direct on single-node trees (intersect_bvh<.., MULTI = false, TRIP = true>; DESIGN.md
// section 4, "The triangle trip's flow by hand", and section 9, r25).  Knobs, each 0 for the A/B builds of
// profiles/r25_c2_bench_ab.txt:
#ifndef RB_TRIP_PLAIN
#define RB_TRIP_PLAIN 1   // the record loaded at the top of its own trip into the registers the arithmetic reads, one latch; 0: the double buffer
#endif
#ifndef RB_TRIP_ASM
#define RB_TRIP_ASM 3     // accept_trip below: 1 without a skip, 2 with one skip after the u test, 3 with another after the v test; 0: accept_slot as the compiler lays it out
#endif
// accept_trip writes out rcp_det's fast form; a build that switches that form off (the A/B knobs of earlier rounds) gets accept_slot back
#define RB_TRIP_BLOCK (RB_TRIP_ASM != 0 && RB_FAST_RCP && RB_RCP_DET)

// accept_slot<true> with the exec flow laid out by hand.  The vector instructions are the ones the compiler emits for
// accept_slot<true> -- the same operations on the same operands in the same order, the operand order of every commutative
// add and multiply included -- so t, u, v are the same bits.  What differs is the flow between them.  The compiler nests four
// early-outs: each joins two compares in a scalar pair, saves the mask, narrows it, tests it, and all four are restored one after
// the other at the same point.  Here the mask on entry is kept in one scalar pair and every early-out narrows exec with v_cmpx,
// which writes the compare's lanes -- 0 for a lane that is off -- into exec.  A compound test is two of them in a row:
// narrowing by one and then by the other leaves exactly the lanes that pass both, which is the conjunction the source writes
// (!(u < 0 || u > 1) is !(u < 0) && !(u > 1)).  The compares are the compiler's: nlt / ngt where the source negates a `<` / `>`
// (true for a NaN, so a NaN goes on as it does in accept_slot), lt where it does not (false for a NaN).  `t > 0.0f` has no
// instruction, as in the compiler's code: `t > 0.001f` is an ordered compare too, false for a NaN like `t > 0.0f`, and every
// other t above 0.001 is above 0.  A lane outside rcp_det's guard takes the division under one more mask, put back before u is
// formed.  The accepted hit's four moves run under the last mask, and one move restores the entry mask: exec leaves the block
// as it entered it, whichever lanes were on, none included (every instruction between is a vector one, which an empty mask
// turns into nothing, or touches only the block's own scalar temporaries).
// SKIP: 1 = one branch over the rest of the trip when no lane passes the u test, 2 = another one after the v test.  big: 2^100 (the caller holds it in a scalar register).
// UV = false: the accepted hit moves slot and t only (TriHitT<false>); every other instruction is the same in both forms.
// VREC = true (pass 2 of the triangle sift, sift_triangles below): the record and the slot are per-lane values in vector registers.
// The instruction text is the same, so t (and u, v) are the same bits for the same triangle and ray.
template <int SKIP, bool UV = true, bool VREC = false>
DEV void accept_trip(const v4f a, const v4f b, const v4f c, uint32_t slot, f3 o, f3 d, float big, TriHitT<UV>& hit) {
    float r8, r10, r11, r12, r13, r14, r15, r16, r17;
    uint64_t entry, keep, m, ds;
#define RB_TRIP_HEAD                                                                                                     \
    "s_mov_b64 %[entry], exec\n\t"                                                                                       \
    "v_mul_f32_e32 %[r8], %[cz], %[dy]\n\t"                                                                              \
    "v_mul_f32_e32 %[r10], %[cy], %[dz]\n\t"                                                                             \
    "v_sub_f32_e32 %[r10], %[r8], %[r10]\n\t"                                                                            \
    "v_mul_f32_e32 %[r8], %[cx], %[dz]\n\t"                                                                              \
    "v_mul_f32_e32 %[r11], %[cz], %[dx]\n\t"                                                                             \
    "v_sub_f32_e32 %[r11], %[r8], %[r11]\n\t"                                                                            \
    "v_mul_f32_e32 %[r8], %[cy], %[dx]\n\t"                                                                              \
    "v_mul_f32_e32 %[r12], %[cx], %[dy]\n\t"                                                                             \
    "v_sub_f32_e32 %[r12], %[r8], %[r12]\n\t"                                                                            \
    "v_mul_f32_e32 %[r8], %[bx], %[r10]\n\t"                                                                             \
    "v_mul_f32_e32 %[r13], %[by], %[r11]\n\t"                                                                            \
    "v_add_f32_e32 %[r8], %[r8], %[r13]\n\t"                                                                             \
    "v_mul_f32_e32 %[r13], %[bz], %[r12]\n\t"                                                                            \
    "v_add_f32_e32 %[r13], %[r13], %[r8]\n\t"                                                                            \
    "v_cmpx_nlt_f32_e64 vcc, |%[r13]|, %[eps]\n\t"           /* !(|det| < 1e-6) */                                       \
    "v_cmp_eq_u16_e64 %[m], -1, %[r13]\n\t"                  /* rcp_det's guard: low half all ones, */                   \
    "v_cmp_nlt_f32_e64 vcc, |%[r13]|, %[big]\n\t"            /* or !(|det| < 2^100) */                                   \
    "v_rcp_f32_e32 %[r8], %[r13]\n\t"                                                                                    \
    "s_or_b64 %[m], vcc, %[m]\n\t"                                                                                       \
    "v_fma_f32 %[r14], -%[r13], %[r8], 1.0\n\t"                                                                          \
    "v_fmac_f32_e32 %[r8], %[r14], %[r8]\n\t"                                                                            \
    "s_and_saveexec_b64 %[keep], %[m]\n\t"                                                                               \
    "s_cbranch_execz .Ltrip_rcp_%=\n\t"                                                                                  \
    "v_div_scale_f32 %[r8], %[ds], %[r13], %[r13], 1.0\n\t"  /* 1.0f / det as the compiler expands it */                 \
    "v_rcp_f32_e32 %[r14], %[r8]\n\t"                                                                                    \
    "v_div_scale_f32 %[r15], vcc, 1.0, %[r13], 1.0\n\t"                                                                  \
    "v_fma_f32 %[r16], -%[r8], %[r14], 1.0\n\t"                                                                          \
    "v_fmac_f32_e32 %[r14], %[r16], %[r14]\n\t"                                                                          \
    "v_mul_f32_e32 %[r16], %[r15], %[r14]\n\t"                                                                           \
    "v_fma_f32 %[r17], -%[r8], %[r16], %[r15]\n\t"                                                                       \
    "v_fmac_f32_e32 %[r16], %[r17], %[r14]\n\t"                                                                          \
    "v_fma_f32 %[r8], -%[r8], %[r16], %[r15]\n\t"                                                                        \
    "v_div_fmas_f32 %[r8], %[r8], %[r14], %[r16]\n\t"                                                                    \
    "v_div_fixup_f32 %[r8], %[r8], %[r13], 1.0\n"                                                                        \
    ".Ltrip_rcp_%=:\n\t"                                                                                                 \
    "s_mov_b64 exec, %[keep]\n\t"                                                                                        \
    "v_subrev_f32_e32 %[r13], %[ax], %[ox]\n\t"                                                                          \
    "v_subrev_f32_e32 %[r14], %[ay], %[oy]\n\t"                                                                          \
    "v_subrev_f32_e32 %[r15], %[az], %[oz]\n\t"                                                                          \
    "v_mul_f32_e32 %[r10], %[r13], %[r10]\n\t"                                                                           \
    "v_mul_f32_e32 %[r11], %[r14], %[r11]\n\t"                                                                           \
    "v_add_f32_e32 %[r10], %[r10], %[r11]\n\t"                                                                           \
    "v_mul_f32_e32 %[r11], %[r15], %[r12]\n\t"                                                                           \
    "v_add_f32_e32 %[r10], %[r11], %[r10]\n\t"                                                                           \
    "v_mul_f32_e32 %[r10], %[r10], %[r8]\n\t"                /* u */                                                     \
    "v_cmpx_ngt_f32_e32 vcc, 0, %[r10]\n\t"                  /* !(u < 0) */                                              \
    "v_cmpx_nlt_f32_e32 vcc, 1.0, %[r10]\n\t"                /* !(u > 1) */
#define RB_TRIP_TAIL                                                                                                     \
    "v_mul_f32_e32 %[r11], %[bz], %[r14]\n\t"                                                                            \
    "v_mul_f32_e32 %[r12], %[by], %[r15]\n\t"                                                                            \
    "v_sub_f32_e32 %[r12], %[r11], %[r12]\n\t"                                                                           \
    "v_mul_f32_e32 %[r11], %[bx], %[r15]\n\t"                                                                            \
    "v_mul_f32_e32 %[r15], %[bz], %[r13]\n\t"                                                                            \
    "v_sub_f32_e32 %[r15], %[r11], %[r15]\n\t"                                                                           \
    "v_mul_f32_e32 %[r11], %[by], %[r13]\n\t"                                                                            \
    "v_mul_f32_e32 %[r13], %[bx], %[r14]\n\t"                                                                            \
    "v_sub_f32_e32 %[r13], %[r11], %[r13]\n\t"                                                                           \
    "v_mul_f32_e32 %[r11], %[dx], %[r12]\n\t"                                                                            \
    "v_mul_f32_e32 %[r14], %[dy], %[r15]\n\t"                                                                            \
    "v_add_f32_e32 %[r11], %[r11], %[r14]\n\t"                                                                           \
    "v_mul_f32_e32 %[r14], %[dz], %[r13]\n\t"                                                                            \
    "v_add_f32_e32 %[r11], %[r14], %[r11]\n\t"                                                                           \
    "v_mul_f32_e32 %[r11], %[r11], %[r8]\n\t"                /* v */                                                     \
    "v_add_f32_e32 %[r14], %[r10], %[r11]\n\t"                                                                           \
    "v_cmpx_ngt_f32_e32 vcc, 0, %[r11]\n\t"                  /* !(v < 0) */                                              \
    "v_cmpx_nlt_f32_e32 vcc, 1.0, %[r14]\n\t"                /* !(u + v > 1) */
#define RB_TRIP_LAST                                                                                                     \
    "v_mul_f32_e32 %[r12], %[cx], %[r12]\n\t"                                                                            \
    "v_mul_f32_e32 %[r14], %[cy], %[r15]\n\t"                                                                            \
    "v_add_f32_e32 %[r12], %[r12], %[r14]\n\t"                                                                           \
    "v_mul_f32_e32 %[r13], %[cz], %[r13]\n\t"                                                                            \
    "v_add_f32_e32 %[r12], %[r13], %[r12]\n\t"                                                                           \
    "v_mul_f32_e32 %[r8], %[r12], %[r8]\n\t"                 /* t */                                                     \
    "v_cmpx_lt_f32_e32 vcc, %[tmin], %[r8]\n\t"              /* t > 0.001 */                                             \
    "v_cmpx_lt_f32_e32 vcc, %[r8], %[ht]\n\t"                /* t < hit.t */                                             \
    "v_mov_b32_e32 %[hs], %[slot]\n\t"
#define RB_TRIP_MOVES_UV                                                                                                 \
    "v_mov_b32_e32 %[hv], %[r11]\n\t"                                                                                    \
    "v_mov_b32_e32 %[ht], %[r8]\n\t"                                                                                     \
    "v_mov_b32_e32 %[hu], %[r10]\n"
#define RB_TRIP_MOVES_T                                                                                                  \
    "v_mov_b32_e32 %[ht], %[r8]\n"
#define RB_TRIP_OUT_UV [ht] "+v"(hit.t), [hu] "+v"(hit.u), [hv] "+v"(hit.v), [hs] "+v"(hit.slot)
#define RB_TRIP_OUT_T [ht] "+v"(hit.t), [hs] "+v"(hit.slot)
#define RB_TRIP_TEMPS                                                                                                    \
    [r8] "=&v"(r8), [r10] "=&v"(r10),                                                                                     \
      [r11] "=&v"(r11), [r12] "=&v"(r12), [r13] "=&v"(r13), [r14] "=&v"(r14), [r15] "=&v"(r15), [r16] "=&v"(r16),         \
      [r17] "=&v"(r17), [entry] "=&s"(entry), [keep] "=&s"(keep), [m] "=&s"(m), [ds] "=&s"(ds)
#define RB_TRIP_IN(K)                                                                                                    \
    [ax] K(a.x), [ay] K(a.y), [az] K(a.z), [bx] K(b.x), [by] K(b.y), [bz] K(b.z), [cx] K(c.x),                            \
      [cy] K(c.y), [cz] K(c.z), [slot] K(slot), [ox] "v"(o.x), [oy] "v"(o.y), [oz] "v"(o.z), [dx] "v"(d.x),               \
      [dy] "v"(d.y), [dz] "v"(d.z), [eps] "s"(1e-6f)
#define RB_TRIP_CLOBBERS "vcc", "scc"   /* s_or_b64 and s_and_saveexec_b64 write scc */
#define RB_TRIP_OPS_UV(K) : RB_TRIP_OUT_UV, RB_TRIP_TEMPS : RB_TRIP_IN(K), [big] "s"(big), [tmin] "s"(0.001f) : RB_TRIP_CLOBBERS
#define RB_TRIP_OPS_T(K) : RB_TRIP_OUT_T, RB_TRIP_TEMPS : RB_TRIP_IN(K), [big] "s"(big), [tmin] "s"(0.001f) : RB_TRIP_CLOBBERS
#define RB_TRIP_SKIP "s_cbranch_execz .Ltrip_end_%=\n\t"
    // one statement per form: the same blocks in the same order, with the moves' variant put in
#define RB_TRIP_EMIT(MOVES, OPS)                                                                                         \
    if constexpr (SKIP == 2) {                                                                                           \
        asm volatile(RB_TRIP_HEAD RB_TRIP_SKIP RB_TRIP_TAIL RB_TRIP_SKIP RB_TRIP_LAST MOVES ".Ltrip_end_%=:\n\t"         \
                     "s_mov_b64 exec, %[entry]" OPS);                                                                    \
    } else if constexpr (SKIP == 1) {                                                                                    \
        asm volatile(RB_TRIP_HEAD RB_TRIP_SKIP RB_TRIP_TAIL RB_TRIP_LAST MOVES ".Ltrip_end_%=:\n\t"                      \
                     "s_mov_b64 exec, %[entry]" OPS);                                                                    \
    } else {                                                                                                             \
        asm volatile(RB_TRIP_HEAD RB_TRIP_TAIL RB_TRIP_LAST MOVES "\ts_mov_b64 exec, %[entry]" OPS);                     \
    }
    if constexpr (UV && VREC) {
        RB_TRIP_EMIT(RB_TRIP_MOVES_UV, RB_TRIP_OPS_UV("v"))
    } else if constexpr (UV) {
        RB_TRIP_EMIT(RB_TRIP_MOVES_UV, RB_TRIP_OPS_UV("s"))
    } else if constexpr (VREC) {
        RB_TRIP_EMIT(RB_TRIP_MOVES_T, RB_TRIP_OPS_T("v"))
    } else {
        RB_TRIP_EMIT(RB_TRIP_MOVES_T, RB_TRIP_OPS_T("s"))
    }
#undef RB_TRIP_EMIT
#undef RB_TRIP_SKIP
#undef RB_TRIP_HEAD
#undef RB_TRIP_MOVES_UV
#undef RB_TRIP_MOVES_T
#undef RB_TRIP_OUT_UV
#undef RB_TRIP_OUT_T
#undef RB_TRIP_TEMPS
#undef RB_TRIP_IN
#undef RB_TRIP_CLOBBERS
#undef RB_TRIP_OPS_UV
#undef RB_TRIP_OPS_T
#undef RB_TRIP_TAIL
#undef RB_TRIP_LAST
}

// (One triangle per step.  r01-r02 tested two per step with packed f32 math: on gfx950 a packed f32 instruction issues at
// half the rate of a plain one (MI355X_MICROARCH.md), so the pairing bought no throughput and paid for the register
// pairs -- 4.9 % slower on C2, profiles/r03_noslp.txt.  That arm lives in tools/ablate/rb_forks.patch.)

// Walk of the library's own tree over the same triangles (rb_bvh.cpp / rb_build.hip; RB_FLAG_FAST_BVH -- r02's default
// for large meshes, since r03 the chunked walk of rb_kernels.hip is the default): nearer child first, subtrees
// skipped when missed or entered beyond the best t.  It reproduces the reference walk's winner
// (shader.wgsl:282-392) bit for bit -- DESIGN.md section 4 has the full argument:
//  * candidates are evaluated with the reference's isect_triangle, so t, u, v are the same bits;
//  * equal t resolves by the triangle's rank in the reference's visit order;
//  * the reference only tests a triangle if every node from the root to its leaf passes intersect_aabb: an
//    improving candidate is accepted only after that chain has been re-checked with the reference's own slab
//    arithmetic on the reference's boxes;
//  * no triangle the reference would report as hit is ever lost to culling.  The reference's f32
//    Moller-Trumbore can report a hit some distance from its triangle; that distance is bounded as long as the
//    ray is not nearly parallel to the triangle's plane.  Hits are therefore split by c0 = kFastGrazeCos:
//      (A) |cos(ray, normal)| >= c0: a subtree of the library's tree is skipped only if the ray misses its box
//          inflated by a margin that covers every such hit below it (entry());
//      (B) |cos| < c0 (the ray is within ~1.7 degrees of the triangle's plane; no useful bound exists): found by a
//          second pass over the REFERENCE tree with the reference's own slab tests, entering only nodes whose
//          normal cone admits such a triangle, and testing only the triangles of a leaf that are (gnode_step / gleaf_step).
//    Both passes offer their candidates to the same closest-hit rule, so the reference's winner is always among them.
// The walk is a resumable object so that the same steps serve the per-segment kernels (intersect_bvh_fast
// below: run to completion) and the stepped kernel (k_trace_fast: lanes that finish are shaded and refilled
// while the others keep walking).
//
// (A) in numbers.  For the ray (o, d), |d| = 1 +- 4 ulp, and a triangle k with L = max(|e1|, |e2|), N = |e1 x e2|,
// s = o - v0, a = d . (e2 x e1) = N cos(d, n_k) and the reference's computed determinant a^ (a hit is accepted only
// if |a^| >= 1e-6), the point X = o + t^ d of an ACCEPTED hit satisfies (u = 2^-24, first order, every rounding of
// shader.wgsl:248-280 in the no-FMA f32 arithmetic of the contract)
//     dist_inf(X, box(triangle k)) <= 26 u (|s| + L) L^2 / |a_k|  +  7.5 u (|s| + 2 L)
// (r03's sharper sum, second order included: (21.4 |s| + 9.1 L) u L^2 / |a_k|, of which 11.2 |s| + 4.6 L across the ray and
// 10.2 |s| + 4.6 L along it -- k_trace_chunk uses the two parts separately, this walk keeps the round figure)
// as long as 5.42 u L^2 / |a^| <= 0.05.  With |cos| >= c0: L^2 / |a_k| <= (max_k L_k^2 / N_k) / c0, a per-child
// constant FA (stored in the node's pad words with the 0.95 that bounds |a^| >= 0.95 |a|; +inf = always enter,
// beyond 1.5e5 where no bound is claimed or for a triangle with N = 0); |s| + 2 L <= Sp = (distance from o to the
// child box's farthest corner) + 2 (sum of its extents); plus 10 u Sp for the rounding of the slab test itself:
//     margin = Sp (27 u FA + 20 u),
// and X is inside the box so inflated, entered no later than t^: the slab test with that margin and the cull
// `entry > best t` are safe.
// Can a triangle whose normal lies in `cone` = {c cos(alpha), tan(alpha)} (every unit normal below is within alpha of
// +-c) have |cos(d, n)| < c0?  |cos(d, n)| >= cos(alpha) (x - tan(alpha) sqrt(1 - x^2)) with x = |d . c|.  y = x cos(alpha)
// is known to 6e-7, k2 - y^2 to 4e-6 k2; all zeros = no cone = always possible; tan(alpha) = -1 = nothing below = never.
// cone_cos_bound: that lower bound of |cos(d, n)| over the cone (<= 0, or NaN, when it says nothing).
DEV float cone_cos_bound(f3 d, v4f cone) {
    const float y = fabsf(__builtin_fmaf(d.z, cone.z, __builtin_fmaf(d.y, cone.y, d.x * cone.x)));
    const float k2 = __builtin_fmaf(cone.z, cone.z, __builtin_fmaf(cone.y, cone.y, cone.x * cone.x));
    const float root = 1.000001f * __builtin_amdgcn_sqrtf(fmaxf(__builtin_fmaf(-y, y, k2), 0.0f) + 4e-6f * k2);
    return __builtin_fmaf(-cone.w, root, y - 1e-6f);
}
DEV bool cone_admits_grazing(f3 d, v4f cone) {
    if (cone.w < 0.0f) return false;
    return !(cone_cos_bound(d, cone) >= kFastGrazeCos);
}
constexpr float kFastKF = 27.0f * 5.9604645e-8f * 1.01f;
constexpr float kFastKS = 20.0f * 5.9604645e-8f * 1.01f;
template <bool STATS>
struct FastWalk {
    f3 o, d, inv;
    float m_ref;        // shrink of a reference leaf box for the chain shortcut (reference_would_test)
    TriHit h;
    uint32_t best_rank;
    uint32_t cur;       // current child reference (leaf: bit 31); second pass: reference node, or bit 31 | next slot of a leaf
    uint32_t gend;      // second pass: end of the leaf being scanned
    bool graze;         // false: the culled walk of the library's tree (A); true: the second pass over the reference tree (B)
    int sp;

    DEV void begin(const KParams& p, f3 o_, f3 d_) {
        o = o_;
        d = d_;
        h.hit = false;
        h.t = 1e20f;
        h.u = 0.0f;
        h.v = 0.0f;
        h.slot = 0u;
        best_rank = 0xFFFFFFFFu;
        inv = mk(rcp_exact(d.x), rcp_exact(d.y), rcp_exact(d.z));
        // farthest the ray origin can be from any point of the mesh: the rounding error of a slab test on any of
        // the reference's boxes is below 8 ulp of that
        const f3 fb0 = ld3(p.fast_bmin), fb1 = ld3(p.fast_bmax);
        const float sx_ = fmaxf(fabsf(o.x - fb0.x), fabsf(o.x - fb1.x)), sy_ = fmaxf(fabsf(o.y - fb0.y), fabsf(o.y - fb1.y)),
                    sz_ = fmaxf(fabsf(o.z - fb0.z), fabsf(o.z - fb1.z));
        m_ref = 1e-6f * sqrtf(sx_ * sx_ + sy_ * sy_ + sz_ * sz_) + 1e-30f;
        cur = p.fast_root;
        gend = 0u;
        graze = false;
        sp = 0;
    }
    DEV bool at_leaf() const { return (cur & 0x80000000u) != 0u; }
    // which step this lane needs next: 0 node / 1 leaf of the library's tree, 2 node / 3 leaf chunk of the second pass
    DEV uint32_t kind() const { return (graze ? 2u : 0u) | (cur >> 31); }

    // Entries beyond the LDS stack (trees deeper than kStackDepth: only device-built ones, the host
    // builder limits its depth) spill to this lane's column of a global scratch array.
    // (volatile on the spill side keeps the compiler from merging the two accesses into one through a
    // generic pointer, which would turn every LDS stack access into a flat_load / flat_store)
    DEV static volatile uint32_t* spill(const KParams& p, int at) {
        return p.stack_overflow + ((size_t)(uint32_t)(at - (int)kStackDepth) * (gridDim.x * blockDim.x) + blockIdx.x * blockDim.x + threadIdx.x);
    }
    DEV static void push(const KParams& p, uint32_t* stack, uint32_t stride, int at, uint32_t v) {
        if (__builtin_expect(at < (int)kStackDepth, 1)) stack[at * stride] = v;
        else *spill(p, at) = v;
    }
    DEV static uint32_t peek(const KParams& p, const uint32_t* stack, uint32_t stride, int at) {
        uint32_t v;
        if (__builtin_expect(at < (int)kStackDepth, 1)) v = stack[at * stride];
        else v = *spill(p, at);
        return v;
    }
    // next pending subtree; when the library's tree is done the second pass starts at the reference root;
    // false when both are complete
    DEV bool pop(const KParams& p, const uint32_t* stack, uint32_t stride) {
        if (sp == 0) {
            if (graze || p.fast_skip_second_pass != 0u) return false;
            graze = true;
            cur = 0u;
            return true;
        }
        sp--;
        cur = peek(p, stack, stride, sp);
        return true;
    }

    // visit the child unless the ray misses its inflated box or enters it beyond the best t (comparisons are
    // written so that a NaN means "visit").  This arithmetic only steers the walk: fused operations and the
    // hardware's approximate sqrt / rcp are fine as long as every rounding is on the safe side.
    DEV bool entry(v4f lo, v4f hi, float fa, float& tn) const {
        const f3 a = mk(lo.x, lo.y, lo.z) - o, b = mk(hi.x, hi.y, hi.z) - o;
        const float fx = fmaxf(fabsf(a.x), fabsf(b.x)), fy = fmaxf(fabsf(a.y), fabsf(b.y)), fz = fmaxf(fabsf(a.z), fabsf(b.z));
        // Sp >= |o - v0| + 2 L for every triangle below: farthest corner (v_sqrt_f32 is within 1 ulp) + box extents
        const float sp_ = 1.001f * __builtin_amdgcn_sqrtf(__builtin_fmaf(fx, fx, __builtin_fmaf(fy, fy, fz * fz))) +
                          2.0f * (((b.x - a.x) + (b.y - a.y)) + (b.z - a.z));
        const float mm = (fa <= 1.5e5f) ? sp_ * __builtin_fmaf(kFastKF, fa, kFastKS) : 1e30f;   // NaN -> 1e30
        const f3 t0 = mk(a.x - mm, a.y - mm, a.z - mm) * inv;
        const f3 t1 = mk(b.x + mm, b.y + mm, b.z + mm) * inv;
        tn = fmaxf(fmaxf(fminf(t0.x, t1.x), fminf(t0.y, t1.y)), fminf(t0.z, t1.z));
        const float tf = fminf(fminf(fmaxf(t0.x, t1.x), fmaxf(t0.y, t1.y)), fmaxf(t0.z, t1.z));
        return !(tf < fmaxf(tn, 0.0f)) && !(tn > h.t);
    }

    // (B): can a triangle with |cos(d, n)| < c0 lie below a reference node?  cone = {c cos(alpha), tan(alpha)},
    // every unit normal below is within alpha of +-c, so |cos(d, n)| >= cos(alpha) (x - tan(alpha) sqrt(1 - x^2)) with
    // x = |d . c|.  y = x cos(alpha) is known to 6e-7, k2 - y^2 to 4e-6 k2; all zeros = no cone = always possible;
    // tan(alpha) = -1 = no large triangle below = never.
    DEV bool graze_possible(v4f cone) const { return cone_admits_grazing(d, cone); }
    // The second pass: the reference's own walk (shader.wgsl:309-389: same nodes, same slab arithmetic, so a leaf
    // is reached exactly when the reference tests its triangles), restricted to nodes that can hold a class-(B)
    // triangle, and in a leaf to the triangles that are class (B) for this ray (the prepared unit normal is the
    // reference's f32 normalize(cross(e1, e2))).  Candidates go through the reference's intersect_triangle and the
    // closest-hit rule of leaf_step; the visit order does not matter because equal t resolves by reference rank.
    // Resumable like the first pass: one reference node per gnode_step, up to kGrazeChunk triangles per gleaf_step,
    // on the same (by now empty) stack.
    static constexpr uint32_t kGrazeChunk = 16u;
    DEV bool gnode_step(const KParams& p, uint32_t* stack, uint32_t stride, Tally<STATS>& tl) {
        const cf4p gn = (cf4p)p.gnodes + (size_t)cur * 4u;
        const v4f cone = gn[2];
        if (graze_possible(cone)) {
            const v4f n0 = gn[0], n1 = gn[1];
            if constexpr (STATS) tl.nodes++;
            if (isect_aabb(o, inv, mk(n0.x, n0.y, n0.z), mk(n1.x, n1.y, n1.z))) {
                const v4f n3 = gn[3];   // first, count (the leaf's large triangles in gslots), cap, is_leaf
                // A near-degenerate hit of a triangle below is reported no farther than margin(cap) from this box
                // (entry(): the same bound with L^2 / |a^| <= L^2 / 1e-6), so it cannot beat the best t if the ray
                // enters the inflated box beyond it.
                float tn;
                if (entry(n0, n1, n3.z, tn)) {
                    const uint32_t node_count = p.u.bvh_node_count;
                    if (__float_as_uint(n3.w) != 0u) {   // leaf
                        const uint32_t first = __float_as_uint(n3.x), count = __float_as_uint(n3.y);
                        if (count > 0u) {
                            cur = 0x80000000u | first;
                            gend = first + count;
                            return true;
                        }
                    } else {
                        const uint32_t l = __float_as_uint(n0.w), r = __float_as_uint(n1.w);
                        const bool hl = l < node_count, hr = r < node_count;   // guards :376-387
                        if (hl && hr) {
                            stack[sp * stride] = r;
                            sp++;
                            cur = l;
                            return true;
                        }
                        if (hl || hr) {
                            cur = hl ? l : r;
                            return true;
                        }
                    }
                }
            }
        }
        return pop(p, stack, stride);
    }
    DEV bool gleaf_step(const KParams& p, uint32_t* stack, uint32_t stride, Tally<STATS>& tl) {
        const cf4p ptris = (cf4p)p.ptris;
        const RB_CONST uint32_t* meta = cptr(p.slot_meta);
        const RB_CONST uint32_t* gslots = cptr(p.gslots);
        uint32_t j = cur & 0x7FFFFFFFu;
        const uint32_t stop = (j + kGrazeChunk < gend) ? j + kGrazeChunk : gend;
        for (; j < stop; j++) {
            const uint32_t slot = gslots[j];
            const v4f nr = ptris[slot * 4u + 3u];
            // prepared normal vs true normal: the f32 cross product is off by <= 2.42 u L^2, i.e. the direction by
            // <= 2.5 u q + 3 u <= 6.5e-4 rad for every triangle (A) has a finite margin for (q <= 4275); a
            // triangle beyond that (or without a normal: NaN here) has FA = +inf and is never culled by (A)
            if (!(fabsf(__builtin_fmaf(d.z, nr.z, __builtin_fmaf(d.y, nr.y, d.x * nr.x))) < kFastGrazeCos * 1.03f)) continue;
            const v4f a = ptris[slot * 4u], b = ptris[slot * 4u + 1u], c = ptris[slot * 4u + 2u];
            if (__float_as_uint(c.w) == 0u) continue;  // guard :336
            if constexpr (STATS) tl.tris++;
            float u, v;
            const float t = isect_triangle(o, d, mk(a.x, a.y, a.z), mk(b.x, b.y, b.z), mk(c.x, c.y, c.z), u, v);
            if (t > 0.001f && !(t > h.t)) {
                const uint32_t rank = meta[slot * 2u + 1u] & ~kSlotLarge;
                if (t < h.t || rank < best_rank) {
                    h.hit = true;
                    h.t = t;
                    h.u = u;
                    h.v = v;
                    h.slot = slot;
                    best_rank = rank;
                    if constexpr (STATS) tl.mesh_hits++;
                }
            }
        }
        if (j < gend) {
            cur = 0x80000000u | j;
            return true;
        }
        return pop(p, stack, stride);
    }
    // one step of whatever kind this lane needs; false when the walk is complete
    DEV bool step(const KParams& p, uint32_t* stack, uint32_t stride, Tally<STATS>& tl) {
        switch (kind()) {
            case 0u: return node_step(p, stack, stride, tl);
            case 1u: return leaf_step(p, stack, stride, tl);
            case 2u: return gnode_step(p, stack, stride, tl);
            default: return gleaf_step(p, stack, stride, tl);
        }
    }

    // cur is an internal node: descend into the nearer child that is hit, remember the other.
    // Returns false when the walk is complete.
    DEV bool node_step(const KParams& p, uint32_t* stack, uint32_t stride, Tally<STATS>& tl) {
        const cf4p nodes = (cf4p)p.fast_nodes;
        const v4f l0 = nodes[cur * 4u], l1 = nodes[cur * 4u + 1u], r0 = nodes[cur * 4u + 2u], r1 = nodes[cur * 4u + 3u];
        if constexpr (STATS) tl.nodes++;
        const uint32_t lref = __float_as_uint(l0.w), rref = __float_as_uint(l1.w);
        float tl_, tr_;
        const bool hl = entry(l0, l1, r0.w, tl_), hr = entry(r0, r1, r1.w, tr_);
        if (hl && hr) {
            const bool left_first = !(tr_ < tl_);
            push(p, stack, stride, sp, left_first ? rref : lref);
            sp++;
            cur = left_first ? lref : rref;
            return true;
        }
        if (hl) {
            cur = lref;
            return true;
        }
        if (hr) {
            cur = rref;
            return true;
        }
        return pop(p, stack, stride);
    }

    DEV bool reference_would_test(const KParams& p, uint32_t leaf_node, Tally<STATS>& tl) const {
        const cf4p rnodes = (cf4p)p.nodes;
        const RB_CONST uint32_t* parent = cptr(p.ref_parent);
        const float m = m_ref;
        // Shortcut: if the ray passes through the reference LEAF's box shrunk by m on every side (m = 1e-6 of
        // the farthest the origin can be from the mesh: twice the rounding error of this slab test plus that of
        // the reference's), it passes through the interior of every ancestor's box with room to spare, so each of
        // the reference's slab tests succeeds; only a ray that merely grazes the leaf box needs the exact walk
        // up the chain.
        {
            const v4f n0 = rnodes[leaf_node * 3u], n1 = rnodes[leaf_node * 3u + 1u];
            if constexpr (STATS) tl.nodes++;
            const bool thick = (n1.x - n0.x >= 2.0f * m) && (n1.y - n0.y >= 2.0f * m) && (n1.z - n0.z >= 2.0f * m);
            const f3 t0 = (mk(n0.x + m, n0.y + m, n0.z + m) - o) * inv;
            const f3 t1 = (mk(n1.x - m, n1.y - m, n1.z - m) - o) * inv;
            const float tn = fmaxf(fmaxf(fminf(t0.x, t1.x), fminf(t0.y, t1.y)), fminf(t0.z, t1.z));
            const float tf = fminf(fminf(fmaxf(t0.x, t1.x), fmaxf(t0.y, t1.y)), fmaxf(t0.z, t1.z));
            const bool finite = (t0.x == t0.x) && (t0.y == t0.y) && (t0.z == t0.z) && (t1.x == t1.x) && (t1.y == t1.y) &&
                                (t1.z == t1.z);
            if (thick && finite && tf >= fmaxf(tn, 0.0f)) return true;
        }
        uint32_t n = leaf_node;
        for (;;) {
            const v4f n0 = rnodes[n * 3u], n1 = rnodes[n * 3u + 1u];
            if constexpr (STATS) tl.nodes++;
            if (!isect_aabb(o, inv, mk(n0.x, n0.y, n0.z), mk(n1.x, n1.y, n1.z))) return false;
            if (n == 0u) return true;
            n = parent[n];
        }
    }

    // cur is a leaf (1 or 2 triangles): test them, then take the next pending subtree.
    // Returns false when the walk is complete.
    DEV bool leaf_step(const KParams& p, uint32_t* stack, uint32_t stride, Tally<STATS>& tl) {
        const cf4p ftris = (cf4p)p.fast_tris;
        const RB_CONST uint32_t* fslots = cptr(p.fast_slots);
        const RB_CONST uint32_t* meta = cptr(p.slot_meta);
        const uint32_t first = cur & 0x0FFFFFFFu, count = ((cur >> 28) & 3u) + 1u;
        for (uint32_t j = first; j < first + count; j++) {
            const v4f a = ftris[j * 4u], b = ftris[j * 4u + 1u], c = ftris[j * 4u + 2u];
            if constexpr (STATS) tl.tris++;
            float u, v;
            const float t = isect_triangle(o, d, mk(a.x, a.y, a.z), mk(b.x, b.y, b.z), mk(c.x, c.y, c.z), u, v);
            if (t > 0.001f && !(t > h.t)) {
                const uint32_t slot = fslots[j];
                const uint32_t leaf_node = meta[slot * 2u], rank = meta[slot * 2u + 1u] & ~kSlotLarge;
                if ((t < h.t || rank < best_rank) && reference_would_test(p, leaf_node, tl)) {
                    h.hit = true;
                    h.t = t;
                    h.u = u;
                    h.v = v;
                    h.slot = slot;
                    best_rank = rank;
                    if constexpr (STATS) tl.mesh_hits++;
                }
            }
        }
        return pop(p, stack, stride);
    }
};

// The triangle sift of a single-node tree (k_trace_sift; DESIGN.md section 4, "The triangle sift"): the list's triangles in the
// two-pass form the sphere scan has (segment_spheres).  Pass 1, full width, wave-uniform records: one conservative box test per
// GROUP of neighbouring triangles (rb_tri_filter.hpp) leaves a candidate bit per slot.  It is the conservative half of chunk_child
// (rb_device_chunk.hpp) at a leaf: a hit the reference's f32 test ACCEPTS has its exact plane point within mm of the triangle's
// box and its reported t within dt of that point's parameter (section 4.1, E1-E7), mm = Sp (KP f + KS), dt = Sp (KT f + KD), f the
// bound of |e1| |e2| / |a^| for this ray's own |cos| (the group's cone), Sp >= |o - v0| + L / 2.  Sp is one constant per launch,
// folded into p.sift_k*: it holds for every origin inside p.sift_lo..hi, which a lane checks once per segment; a lane outside
// takes every slot.  Every compare is written so that a NaN means "candidate".  Pass 2, per lane, ascending slots: the lane's own
// candidates through accept_trip with the record in vector registers -- same instructions, same bits; the strict t < hit.t in
// ascending order keeps the reference's winner.
constexpr float kSiftFMax = 1.5e5f;   // kChunkFMax (rb_kernels.hip checks)
// what pass 1 holds of a ray for the whole list
struct SiftRay {
    f3 inv, oi;    // approximate reciprocals of d, and o * inv: their error and the slab values' rounding are inside sift_ks (sift_region)
    bool inside;   // the origin is inside the region Sp was made for, and no reciprocal is beyond sift_rmax (or a NaN)
};
DEV SiftRay sift_ray(const KParams& p, f3 o, f3 d) {
    SiftRay r;
    r.inv = mk(__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y), __builtin_amdgcn_rcpf(d.z));
    r.oi = mk(o.x * r.inv.x, o.y * r.inv.y, o.z * r.inv.z);
    const f3 lo = ld3(p.sift_lo), hi = ld3(p.sift_hi);
    r.inside = ((__builtin_amdgcn_fcmpf(o.x, lo.x, 2) & __builtin_amdgcn_fcmpf(o.x, hi.x, 4) & __builtin_amdgcn_fcmpf(o.y, lo.y, 2) &
                 __builtin_amdgcn_fcmpf(o.y, hi.y, 4) & __builtin_amdgcn_fcmpf(o.z, lo.z, 2) & __builtin_amdgcn_fcmpf(o.z, hi.z, 4) &
                 // the slab values are sums of separately rounded products, c r - o r -+ (h + mm) |r|: a reciprocal so large that one of
                 // them overflows (a direction component that is a tiny normal float, or 0) would leave an infinity where the exact
                 // value is finite.  Below sift_rmax none can (sift_region); a lane beyond it takes every slot.  5: ordered <=
                 __builtin_amdgcn_fcmpf(fabsf(r.inv.x), p.sift_rmax, 5) & __builtin_amdgcn_fcmpf(fabsf(r.inv.y), p.sift_rmax, 5) &
                 __builtin_amdgcn_fcmpf(fabsf(r.inv.z), p.sift_rmax, 5)) >>
                __lane_id()) & 1ull;   // ordered compares: a NaN origin, a NaN or infinite reciprocal are outside
    return r;
}
// Pass 1 over one block of the list: its n <= 32 slots are covered by groups [g0, g1) (wave-uniform); slot base + k ends at bit k.
DEV uint32_t sift_block(const KParams& p, const SiftRay& r, f3 d, uint32_t g0, uint32_t g1, uint32_t n) {
    const float kp = p.sift_kp, ks = p.sift_ks, kt = p.sift_kt, kd = p.sift_kd;
    const cf4p groups = (cf4p)p.sift_groups;
    const f3 inv = r.inv, oi = r.oi;
    uint32_t cand = 0u;
    for (uint32_t g = g1; g != g0; g--) {   // last group first
        const cf4p rec = groups + (size_t)(g - 1u) * 4u;
        const v4f r0 = rec[0], r1 = rec[1], r2 = rec[2];
        const uint32_t count = __float_as_uint(rec[3].y);
        const float y = __builtin_fmaf(d.z, r2.z, __builtin_fmaf(d.y, r2.y, d.x * r2.x));
        const float lb = fabsf(y) - r2.w;
        const float fl = r0.w * __builtin_amdgcn_rcpf(lb);
        const float f = (lb > 1e-6f && fl < r1.w) ? fl : r1.w;   // NaN -> the cap
        const float mm = __builtin_fmaf(kp, f, ks), thr = 0.001f - __builtin_fmaf(kt, f, kd);
        const float tcx = __builtin_fmaf(r0.x, inv.x, -oi.x), tcy = __builtin_fmaf(r0.y, inv.y, -oi.y), tcz = __builtin_fmaf(r0.z, inv.z, -oi.z);
        const float hx = r1.x + mm, hy = r1.y + mm, hz = r1.z + mm;
        const float ix = fabsf(inv.x), iy = fabsf(inv.y), iz = fabsf(inv.z);
        const float tn = fmaxf(fmaxf(__builtin_fmaf(-hx, ix, tcx), __builtin_fmaf(-hy, iy, tcy)), __builtin_fmaf(-hz, iz, tcz));
        const float tf = fminf(fminf(__builtin_fmaf(hx, ix, tcx), __builtin_fmaf(hy, iy, tcy)), __builtin_fmaf(hz, iz, tcz));
        // keep = (!(tf < tn) && !(tf < thr)) || !(f <= kSiftFMax), as lane masks joined by scalar instructions (11: unordered >=,
        // 10: unordered >): written with bools the compiler branches round the second and third compare
        const uint64_t keep = (__builtin_amdgcn_fcmpf(tf, tn, 11) & __builtin_amdgcn_fcmpf(tf, thr, 11)) | __builtin_amdgcn_fcmpf(f, kSiftFMax, 10);
        uint32_t ones;
        asm("v_cndmask_b32_e64 %0, 0, -1, %1" : "=v"(ones) : "s"(keep));
        cand = __builtin_amdgcn_alignbit(cand, ones, 32u - count);   // `count` copies of the bit shifted in
    }
    if (!r.inside) cand = 0xFFFFFFFFu;
    return cand & (0xFFFFFFFFu >> (32u - n));
}
template <bool UV>
DEV void sift_triangles(const KParams& p, f3 o, f3 d, uint32_t first, uint32_t end, float big, TriHitT<UV>& h) {
    const SiftRay r = sift_ray(p, o, d);
    const cf4p ptris = (cf4p)p.ptris;
    uint32_t ends = p.sift_block_ends, g0 = 0u;
    for (uint32_t base = first; base < end; base += 32u, ends >>= 8) {
        const uint32_t g1 = ends & 0xFFu;
        uint32_t cand = sift_block(p, r, d, g0, g1, (end - base < 32u) ? end - base : 32u);
        g0 = g1;
        const cf4p block = ptris + (size_t)base * 4u;
        while (cand != 0u) {
            const uint32_t k = (uint32_t)__ffs((int)cand) - 1u;
            cand &= cand - 1u;
            const cf4p rec = block + __umul24(k, 4u);
            v4f a = rec[0], b = rec[1], c = rec[2];
            uint32_t live = __float_as_uint(c.w);
            asm volatile("" : "+v"(a.x), "+v"(b.x), "+v"(live));   // all three parts asked for before `live` is looked at: one wait
            if (live != 0u) accept_trip<RB_TRIP_ASM - 1, UV, true>(a, b, c, base + k, o, d, big, h);   // guard :336
        }
    }
}

template <bool STATS>
DEV TriHit intersect_bvh_fast(const KParams& p, f3 o, f3 d, uint32_t* stack, uint32_t stride, Tally<STATS>& tl) {
    FastWalk<STATS> w;
    w.begin(p, o, d);
    while (w.step(p, stack, stride, tl)) {
    }
    return w.h;
}

// MULTI = false: the caller only ever sees trees of at most one node (k_trace, the Cornell kernel): the walks of
// multi-node trees are left out of its code altogether -- inlined there they cost the hot loop registers (their
// live ranges pushed 73 VGPRs of k_trace into scratch: 74 B of HBM traffic per segment, -10 %).
// TRIP (with MULTI = false; k_trace and k_trace_direct only): the triangle loop in the form the RB_TRIP_* knobs above choose.
// Every other caller of the single-node walk keeps the double-buffered loop and accept_slot as they were.
// box (TRIP only): kBoxUnknown, or the staged answer of the root box's slab test for this lane's ray.
// UV (the flat kernels pass false; they need TRIP and the hand-laid trip): accept_trip's.
// SIFT (k_trace_sift: TRIP, the hand-laid trip, no STATS): the list through sift_triangles.
template <bool STATS, bool MULTI = true, bool TRIP = false, bool UV = true, bool SIFT = false>
DEV TriHitT<UV> intersect_bvh(const KParams& p, f3 o, f3 d, uint32_t* stack, uint32_t stride, Tally<STATS>& tl, uint32_t box = kBoxUnknown) {
    static_assert(UV || (TRIP && !MULTI && RB_TRIP_BLOCK && RB_TRIP_PLAIN != 0), "the flat forms exist for the hand-laid trip only");
    static_assert(!SIFT || (TRIP && !MULTI && !STATS && RB_TRIP_BLOCK), "the sift is written around the hand-laid trip; counting builds keep the plain loop");
    TriHitT<UV> h;
    h.hit = false;
    h.t = 1e20f;
    if constexpr (UV) {
        h.u = 0.0f;
        h.v = 0.0f;
    }
    h.slot = 0u;
    const uint32_t node_count = p.u.bvh_node_count;
    if (node_count == 0u) return h;
    if constexpr (MULTI) {
        if (p.fast_nodes != nullptr) return intersect_bvh_fast<STATS>(p, o, d, stack, stride, tl);
    }
    constexpr bool skip_box = TRIP && !MULTI && RB_ROOT_INSIDE != 0;
    // (the TRIP instantiations make the reciprocals where the root box still needs them, below)
    const f3 inv = skip_box ? d : mk(rcp_exact(d.x), rcp_exact(d.y), rcp_exact(d.z));
    const cf4p nodes = (cf4p)p.nodes;
    const cf4p ptris = (cf4p)p.ptris;  // 4 x float4 per triangle

    if (node_count == 1u) {
        // Single-node tree (the Cornell box): no stack; the node and its triangles are
        // wave-uniform, so they are fetched with scalar loads and every lane that is
        // inside the box walks the same primitive list.  Same tests, same order.  The record of
        // the next triangle (the last one again at the end of the list: the address stays inside
        // the table) is requested at the top of a trip, before the current one is tested, into
        // scalar registers of its own, and is only waited for when the trip is over.
        const v4f n0 = nodes[0], n1 = nodes[1];
        const v4u n2 = ((cu4p)p.nodes)[2];
        if constexpr (STATS) tl.nodes++;
        const uint32_t first = n2.z, count = n2.w;
        const uint32_t end = (first + count < p.index_len) ? first + count : p.index_len;  // guard :331
        auto in_box = [&]() {
            const f3 b0 = mk(n0.x, n0.y, n0.z), b1 = mk(n1.x, n1.y, n1.z);
            if constexpr (skip_box) {
                // A lane has its answer if its primary's was staged or if it starts strictly inside the box.  One scalar
                // branch takes a wave whose active lanes all have theirs past the three reciprocals and the slab arithmetic;
                // any other wave runs them as before, all lanes, and uses what they say (the same bits where both exist).
                const uint64_t unknown = __builtin_amdgcn_uicmp(box, kBoxUnknown, 32) & ~root_inside_mask(o, d, b0, b1);   // 32: ==
                if (__builtin_expect(unknown == 0ull && box_finite(b0, b1), 1)) return box != kBoxMiss;
                return isect_aabb(o, mk(rcp_exact(d.x), rcp_exact(d.y), rcp_exact(d.z)), b0, b1);
            } else {
                return isect_aabb(o, inv, b0, b1);
            }
        };
        if (first < end && in_box()) {
            constexpr bool trip = TRIP && !MULTI;
            float big = 0x1p100f;
            if constexpr (trip && RB_TRIP_BLOCK) asm("s_mov_b32 %0, 0x71800000" : "=s"(big));   // not re-made in every trip
            auto test = [&](const v4f a, const v4f b, const v4f c, uint32_t slot) {
                if constexpr (STATS) tl.tris++;
                const float before = h.t;
                if constexpr (trip && RB_TRIP_BLOCK) accept_trip<RB_TRIP_ASM - 1, UV>(a, b, c, slot, o, d, big, h);
                else accept_slot<!MULTI>(a, b, c, slot, o, d, h);
                if constexpr (STATS) tl.mesh_hits += (h.t != before) ? 1u : 0u;
            };
            if constexpr (SIFT) {
                sift_triangles<UV>(p, o, d, first, end, big, h);
            } else if constexpr (trip && RB_TRIP_PLAIN != 0) {
                // The record is requested at the top of its own trip, into the registers the arithmetic reads, and waited for
                // there: no second register set, no copies, no clamped address of a next record, and one compare at the bottom.
                // (Eight waves per SIMD cover the scalar load: profiles/r25_c2_bench_ab.txt.)
                // The empty asm statements pin what the compiler would otherwise move into the trip: the whole record is asked
                // for in the header block (it would fetch a and b only once c.w has said `live`, a second wait), and the guard's
                // 2^100 sits in a register set once per segment.
                cf4p rec = ptris + (size_t)first * 4u;
                for (uint32_t slot = first; slot != end; slot++, rec += 4) {
                    v4f a = rec[0], b = rec[1], c = rec[2];
                    uint32_t live = __float_as_uint(c.w);
                    asm volatile("" : "+s"(a.x), "+s"(b.x), "+s"(live));
                    if (live != 0u) test(a, b, c, slot);  // guard :336
                }
            } else {
                const uint32_t last = end - 1u;
                cf4p rec = ptris + (size_t)first * 4u;
                v4f a = rec[0], b = rec[1], c = rec[2];
                bool live = __float_as_uint(c.w) != 0u;  // guard :336
                for (uint32_t slot = first;; slot++) {
                    if (slot < last) rec += 4;
                    const v4f na = rec[0], nb = rec[1], nc = rec[2];
                    if (live) test(a, b, c, slot);
                    if (slot == last) break;
                    a = na;
                    b = nb;
                    c = nc;
                    live = __float_as_uint(nc.w) != 0u;
                }
            }
            h.hit = h.t < 1e20f;
        }
        return h;
    }
    if constexpr (!MULTI) return h;

    int sp = 0;
    stack[0] = 0u;
    sp = 1;
    while (sp > 0) {
        sp--;
        const uint32_t node_idx = stack[sp * stride];
        if (node_idx >= node_count) continue;
        const v4f n0 = nodes[node_idx * 3u], n1 = nodes[node_idx * 3u + 1u];
        const v4u n2 = ((cu4p)p.nodes)[node_idx * 3u + 2u];
        if constexpr (STATS) tl.nodes++;
        if (!isect_aabb(o, inv, mk(n0.x, n0.y, n0.z), mk(n1.x, n1.y, n1.z))) continue;
        const uint32_t left = n2.x, right = n2.y, first = n2.z, count = n2.w;
        if (count > 0u) {
            for (uint32_t i = 0; i < count; i++) {
                const uint32_t slot = first + i;
                if (slot >= p.index_len) continue;
                const v4f a = ptris[slot * 4u], b = ptris[slot * 4u + 1u], c = ptris[slot * 4u + 2u];
                if (__float_as_uint(c.w) == 0u) continue;  // guard :336
                if constexpr (STATS) tl.tris++;
                const float before = h.t;
                test_slot(a, b, c, slot, o, d, h);
                if constexpr (STATS) tl.mesh_hits += (h.t != before) ? 1u : 0u;
            }
        } else {
            if (left < node_count) {
                stack[sp * stride] = left;
                sp++;
            }
            if (right < node_count) {
                stack[sp * stride] = right;
                sp++;
            }
        }
    }
    return h;
}

DEV float uv_at(const KParams& p, uint32_t i) { return (i < p.n_uvs) ? cptr(p.uvs)[i] : 0.0f; }

// shader.wgsl:353-361
DEV void tri_uv(const KParams& p, const TriHit& h, float& uvx, float& uvy) {
    const v4u s0 = ((cu4p)p.pshade)[h.slot];
    const uint32_t i0 = s0.x, i1 = s0.y, i2 = s0.z;  // v0_index, v1_index, v2_index
    const float w = 1.0f - h.u - h.v;
    const float uv0x = uv_at(p, i0 * 2u), uv0y = uv_at(p, i0 * 2u + 1u);
    const float uv1x = uv_at(p, i1 * 2u), uv1y = uv_at(p, i1 * 2u + 1u);
    const float uv2x = uv_at(p, i2 * 2u), uv2y = uv_at(p, i2 * 2u + 1u);
    uvx = (w * uv0x + h.u * uv1x) + h.v * uv2x;
    uvy = (w * uv0y + h.u * uv1y) + h.v * uv2y;
}

}  // namespace
}  // namespace rb
