// rb_device_chunk.hpp -- the chunked walk's per-ray pieces: the child test with its culling margins and
// the node step.  Shared by the render kernel (rb_kernels.hip, k_trace_chunk) and the query kernel (rb_query.hip, k_query_chunk),
// which schedule them differently around the same pooled leaf phase.
#pragma once
#include "rb_device_shade.hpp"

#pragma clang fp contract(off)

namespace rb {
namespace {

// when a wave of the chunked walk switches between its node phase and its pooled leaf phase
#ifndef RB_CHUNK_NODE_LANES
#define RB_CHUNK_NODE_LANES 32   // keep stepping nodes while this many lanes are at one ...
#endif
#ifndef RB_CHUNK_NODE_STEPS
#define RB_CHUNK_NODE_STEPS 8    // ... but at most this many steps per outer iteration (r04: 8 instead of 5, + 1..2 %)
#endif
#ifndef RB_CHUNK_LEAF_LANES
#define RB_CHUNK_LEAF_LANES 8    // test chunks once this many lanes wait at one (or nobody is at a node)
#endif

typedef __attribute__((address_space(3))) v4f lds_v4f;
typedef __attribute__((address_space(3))) uint32_t lds_u32;

// This lane's column of the block's traversal stacks (rb_internal.hpp, kStackEntryBytes): entry k at column[k * block].
template <class Entry>
DEV Entry* stack_column(Entry* s_stack, uint32_t tid) {
    static_assert(sizeof(Entry) == kStackEntryBytes, "the traversal stacks are columns of 4-byte entries shared by every walk of a kernel");
    return &s_stack[tid];
}

// Settled experiments, each measured in r03 (profiles/r03_chunk_steps.txt) and kept as tools/ablate/rb_forks.patch, not here:
// the margin as one box inflation instead of its two parts (C3 - 9 %), Sp by the largest component (- 3 %), the fixed c0
// instead of the ray's own cone bound (- 1..2 %), no chunks put aside (- 3..8 %), no prefetch of the next round (- 2 %).
// of the hit's error (21.4 |s| + 9.1 L) u L^2 / |a|, (11.2 |s| + 4.6 L) is how far the exact plane
// point Q* = o + t* d can be from the triangle's box -- that part inflates the box --, (10.2 |s| + 4.6 L) is |t^ - t*|, which
// only moves the hit along the ray.  4 u of kChunkKS are for the slab arithmetic done on the uninflated box (chunk_child).
// The stored bounds are of G / |a^| with G = |e1| |e2| where r02 had L^2 (E7's leading terms carry |e1| |e2|); the proviso of the
// bounds, 5.42 u L^2 / |a^| <= 0.05, is the host's business where it can be (rb_bvh.cpp pack_fac) and this test elsewhere.
// The five constants are written out in rb_kernels.hip, where tools/margin_certify.py certified them and
// tests/test_margin_bound.py reads them; that file defines RB_CHUNK_MARGINS_DEFINED and this header checks that they are the
// values below, which every other translation unit takes from here.
struct ChunkMargins {
    static constexpr float FMax = 1.5e5f;
    static constexpr float KS = 24.0f * 5.9604645e-8f * 1.01f;
    static constexpr float KP = 12.0f * 5.9604645e-8f * 1.01f;   // across
    static constexpr float KT = 11.0f * 5.9604645e-8f * 1.01f;   // along
    static constexpr float KD = 16.0f * 5.9604645e-8f * 1.01f;   // along, the relative part: 4 u t^ (t^ |d| <= |s| + 2.1 L), |d| = 1 +- 4 u, in units of Sp
};
#ifdef RB_CHUNK_MARGINS_DEFINED
static_assert(kChunkFMax == ChunkMargins::FMax && kChunkKS == ChunkMargins::KS && kChunkKP == ChunkMargins::KP &&
              kChunkKT == ChunkMargins::KT && kChunkKD == ChunkMargins::KD, "rb_kernels.hip's margin constants are not this header's");
#else
constexpr float kChunkFMax = ChunkMargins::FMax, kChunkKS = ChunkMargins::KS, kChunkKP = ChunkMargins::KP, kChunkKT = ChunkMargins::KT,
                kChunkKD = ChunkMargins::KD;
#endif
constexpr uint32_t kChunkWaveLds = 64u * 32u + 64u * 8u + 128u * 4u;  // per wave: ray records, best keys, unit table
constexpr unsigned long long kChunkNoHit = 0x60AD78EC00000000ull;     // (bits of 1e20f) << 32: shader.wgsl:283-290
typedef __attribute__((address_space(3))) unsigned long long lds_u64;

// max(|a|, |b|) in one instruction (fmaxf(fabsf(a), fabsf(b)) compiles to three: each operand is quietened first)
DEV float max_abs(float a, float b) {
    float r;
    asm("v_max_f32 %0, |%1|, |%2|" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// One child slot of a ChunkNode: enter it?  `order` = where the ray enters the box as stored (nearer child first).
// The slab values are the reference's (shader.wgsl:664-671 on the box as stored); the inflated box is derived from
// them per axis -- a box grown by mm enters mm |1 / d| earlier and leaves as much later -- so one set of operations
// serves the exact test and the conservative one.  NaN (0 * inf) always means "enter".
DEV bool chunk_child(v4f lo, v4f hi, uint32_t fac, v4f cone, bool exact, f3 o, f3 d, f3 inv, float best_t, float& order) {
    const f3 a = mk(lo.x, lo.y, lo.z) - o, b = mk(hi.x, hi.y, hi.z) - o;
    const f3 t0 = a * inv, t1 = b * inv;
    const float nx = fminf(t0.x, t1.x), ny = fminf(t0.y, t1.y), nz = fminf(t0.z, t1.z);
    const float fx = fmaxf(t0.x, t1.x), fy = fmaxf(t0.y, t1.y), fz = fmaxf(t0.z, t1.z);
    const float tmin = fmaxf(fmaxf(nx, ny), nz), tmax = fminf(fminf(fx, fy), fz);
    if (exact && !(tmax >= fmaxf(tmin, 0.0f))) return false;   // the reference does not enter this node
    // the bound of L^2 / |a^| this ray needs below the child
    // |a| = N |cos(d, n)| >= N lb for every triangle below, lb = the cone's lower bound of |cos| for THIS ray: the bound
    // (L^2 / N) / (0.95 lb) -- the stored one, made for |cos| >= c0, times c0 / lb -- up to the determinant floor,
    // which holds whatever the angle (all zeros = no cone: lb <= 0; tan = -1 = nothing below: the floor of nothing)
    const float lb = cone_cos_bound(d, cone);
    const float cap = __uint_as_float(fac & 0xFFFF0000u);
    const float fl = __uint_as_float(fac << 16) * (kFastGrazeCos * 1.00001f) * __builtin_amdgcn_rcpf(lb);
    const float f = (lb > 1e-6f && fl < cap) ? fl : cap;   // NaN -> cap
    // Sp >= |o - v0| + L / 2 for every triangle below (E7's L terms are less than half its |s| terms): farthest corner
    // (v_sqrt_f32 is within 1 ulp) + half the box's extents
    const float mx = max_abs(a.x, b.x), my = max_abs(a.y, b.y), mz = max_abs(a.z, b.z);
    const float sp_ = 1.001f * __builtin_amdgcn_sqrtf(__builtin_fmaf(mx, mx, __builtin_fmaf(my, my, mz * mz))) +
                      0.5f * (((b.x - a.x) + (b.y - a.y)) + (b.z - a.z));
    const float ix = fabsf(inv.x), iy = fabsf(inv.y), iz = fabsf(inv.z);
    // Q* = o + t* d, the exact plane point of an accepted hit, lies on the ray within mm of the triangle's box, so the ray's
    // line passes the box inflated by mm at parameters [tn, tf] that hold t*; what is reported, t^, is within dt of t*, has to
    // be positive and, for the winner, no larger than the best t so far
    const bool fin = f <= kChunkFMax;                                        // NaN -> always enter
    const float mm = fin ? sp_ * __builtin_fmaf(kChunkKP, f, kChunkKS) : 1e30f;
    const float dt = fin ? sp_ * __builtin_fmaf(kChunkKT, f, kChunkKD) : 1e30f;
    const float tn = fmaxf(fmaxf(__builtin_fmaf(-mm, ix, nx), __builtin_fmaf(-mm, iy, ny)), __builtin_fmaf(-mm, iz, nz));
    const float tf = fminf(fminf(__builtin_fmaf(mm, ix, fx), __builtin_fmaf(mm, iy, fy)), __builtin_fmaf(mm, iz, fz));
    // nearer child first by where the ray enters the box AS STORED, not the inflated one: a wide margin makes tn early for
    // every child that has one and says little about which child the ray meets first (r04: C3 - 17 % triangle tests, - 9 %
    // child tests, + 14 % segments/s; C5 + 6 %; any order is correct)
    order = tmin;
    return !(tf < tn) && !(tf < -dt) && !(tn - dt > best_t);
}

// cur is an internal node: descend into the nearer child that is entered, remember the other.  False when the walk is complete.
template <bool STATS>
DEV bool chunk_node_step(const KParams& p, uint32_t* stack, uint32_t stride, f3 o, f3 d, f3 inv, float best_t, uint32_t& cur,
                         int& sp, Tally<STATS>& tl) {
    const bool exact = (cur & kChunkExact) != 0u;
    const cf4p q = (cf4p)p.chunk_nodes + (size_t)(cur & 0x3FFFFFFFu) * 6u;
    const v4f l0 = q[0], l1 = q[1], r0 = q[2], r1 = q[3], lc = q[4], rc = q[5];
    const uint32_t lref = __float_as_uint(l0.w), rref = __float_as_uint(l1.w);
    float kl = 0.0f, kr = 0.0f;
    if constexpr (STATS) tl.nodes += (lref != kChunkNone ? 1u : 0u) + (rref != kChunkNone ? 1u : 0u);
    const bool vl = lref != kChunkNone && chunk_child(l0, l1, __float_as_uint(r0.w), lc, exact, o, d, inv, best_t, kl);
    const bool vr = rref != kChunkNone && chunk_child(r0, r1, __float_as_uint(r1.w), rc, exact, o, d, inv, best_t, kr);
    if (vl && vr) {
        // (the entry distance is not kept with the reference: dropping put-aside subtrees at the pop when a nearer hit
        // has turned up meanwhile was measured -- 8-byte stack entries -- and removes 0.3 % of the box tests)
        const bool left_first = !(kr < kl);
        stack[sp * stride] = left_first ? rref : lref;
        sp++;
        cur = left_first ? lref : rref;
        return true;
    }
    if (vl || vr) {
        cur = vl ? lref : rref;
        return true;
    }
    if (sp == 0) return false;
    sp--;
    cur = stack[sp * stride];
    return true;
}

}  // namespace
}  // namespace rb
