// rb_device_chunk.hpp -- the chunked walk, defined once for every kernel that runs it: the child test with
// its culling margins and the node step, and around them the wave's phases -- the wave's corner of LDS (chunk_lds), a lane's walk
// state (ChunkLane, chunk_set_aside), the root box (chunk_begin), the node phase (chunk_node_phase), the pooled leaf phase
// (chunk_leaf_phase), the step after a round (chunk_leaf_retire) and the winner's record (chunk_winner).  k_rad_chunk /
// k_cam_chunk (rb_radiance.hip), k_query_chunk and k_occl_chunk (rb_query.hip) run these phases and keep what differs between
// them: where a lane's ray comes from, when the wave refills and finishes, and what a finished walk is worth.  k_trace_chunk
// (rb_kernels.hip) uses chunk_node_step alone and keeps its own copy of the phases (DESIGN.md section 4.2 says why): a fix to the
// phases here belongs there too.
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

// ---------------------------------------------------------------- the wave's phases around the node step ----
// Two shapes of work alternate inside one wavefront: lane = RAY at the nodes, lane = TRIANGLE for the pooled chunks.

// This wave's corner of LDS behind the block's traversal stacks (kChunkWaveLds bytes)
struct ChunkLds {
    lds_v4f* rayrec;   // [64][2]: {o, chunk put aside}, {d, chunk stood at}
    lds_u64* best;     // [64]: (t bits) << 32 | rank
    lds_u32* units;    // [128]: ray lane (| 64: its second chunk) of every pooled (ray, chunk) pair
};
DEV ChunkLds chunk_lds(uint32_t* s_stack, uint32_t stack_depth, uint32_t block, uint32_t tid) {
    unsigned char* const wl = reinterpret_cast<unsigned char*>(s_stack + stack_depth * block) + (tid >> 6) * kChunkWaveLds;
    return {(lds_v4f*)wl, (lds_u64*)(wl + 64u * 32u), (lds_u32*)(wl + 64u * 40u)};
}

// A lane's walk.  The phases act on the lanes whose state is kChunkWalk and set kChunkDone where a lane has nothing left; every
// other value is the kernel's own (a lane without a ray, or one whose segment has yet to begin).  The phases take the lane by
// value and return it, chunk_set_aside takes it by reference, and the state is a word, not a flag: each of these decides what
// the compiler makes of the node loop (profiles/r34_chunk_walk_shared.txt has the forms that were tried and what each cost).
constexpr uint32_t kChunkWalk = 2u, kChunkDone = 3u;
struct ChunkLane {
    uint32_t cur;             // the node or chunk the lane stands at (kChunkNone: nothing else left to walk)
    uint32_t pend;            // the chunk this lane has put aside
    int sp;                   // entries on its stack column
    unsigned long long key;   // (t bits) << 32 | rank of the best hit so far; what its entry of `best` starts a round with
    uint32_t state;           // kChunkWalk, kChunkDone or a value of the kernel's own
};

// A lane whose walk arrives at a chunk while it holds none aside keeps the chunk for the next leaf phase and goes on with the
// subtree it had put aside, so it takes part in twice as many node passes between two waits (the best t it culls with is then
// one chunk behind: never wrong, rarely wasteful -- few chunk visits hit)
DEV void chunk_set_aside(ChunkLane& L, uint32_t* stack, uint32_t stride) {
    if (L.state == kChunkWalk && L.cur != kChunkNone && (L.cur & kChunkLeaf) != 0u && L.pend == kChunkNone) {
        L.pend = L.cur;
        if (L.sp == 0) {
            L.cur = kChunkNone;
        } else {
            L.sp--;
            L.cur = stack[L.sp * stride];
        }
    }
}

// Start of a walk: the root's own box (shader.wgsl:283-315; inv = rcp_exact of d's components), then its two children.
// The lane walks if its ray meets that box.
template <bool STATS>
DEV ChunkLane chunk_begin(const KParams& fp, f3 o, f3 inv, ChunkLane L, Tally<STATS>& tl) {
    const cf4p rn = (cf4p)fp.nodes;
    const v4f n0 = rn[0], n1 = rn[1];
    if constexpr (STATS) tl.nodes++;
    if (isect_aabb(o, inv, mk(n0.x, n0.y, n0.z), mk(n1.x, n1.y, n1.z))) {
        L.cur = fp.chunk_root;
        L.state = kChunkWalk;
    } else {
        L.state = kChunkDone;
    }
    return L;
}

// Tree: a few node steps while enough lanes are at a node.  `bound`: the t a child is culled against -- the t of the lane's key
// in the closest-hit kernels, tmax in the any-hit one.
template <bool STATS>
DEV ChunkLane chunk_node_phase(const KParams& p, uint32_t* stack, uint32_t stride, f3 o, f3 d, f3 inv, float bound, ChunkLane L,
                               Tally<STATS>& tl) {
#pragma unroll 1
    for (int it = 0; it < RB_CHUNK_NODE_STEPS; ++it) {
        const bool at_node = L.state == kChunkWalk && L.cur != kChunkNone && (L.cur & kChunkLeaf) == 0u;
        const uint32_t n = (uint32_t)__popcll(__ballot(at_node));
        if (n == 0u || (it > 0 && n < (uint32_t)RB_CHUNK_NODE_LANES)) break;
        if (at_node) {
            if (!chunk_node_step<STATS>(p, stack, stride, o, d, inv, bound, L.cur, L.sp, tl)) {
                if (L.pend != kChunkNone) L.cur = kChunkNone;   // nothing left to walk, one chunk still to be tested
                else L.state = kChunkDone;
            }
            chunk_set_aside(L, stack, stride);
        }
    }
    return L;
}

// One round of the leaf phase = 64 / kChunkTris pairs: this lane's pair, its ray record and its triangle's three pieces
struct ChunkRound {
    v4f r0, r1, a, b, c;
    uint32_t rl;
    bool valid;
};
DEV ChunkRound chunk_fetch(cf4p ca, cf4p cb, cf4p cc, const ChunkLds& w, uint32_t lane, uint32_t g0, uint32_t n_units) {
    ChunkRound r;
    const uint32_t g = g0 + lane / kChunkTris;
    const bool ok = g < n_units;
    const uint32_t e = w.units[ok ? g : 0u];   // (entry 0 exists: n_units != 0)
    r.rl = e & 63u;
    r.r0 = w.rayrec[r.rl * 2u];
    r.r1 = w.rayrec[r.rl * 2u + 1u];
    const uint32_t ref = __float_as_uint((e & 64u) ? r.r1.w : r.r0.w), first = ref & 0x03FFFFFFu, cnt = ((ref >> 26) & 31u) + 1u;
    const uint32_t j = lane & (kChunkTris - 1u);
    r.valid = ok && j < cnt;
    const uint32_t pos = first + (j < cnt ? j : 0u);   // (position `first` exists: a chunk holds at least one triangle)
    r.a = ca[pos];
    r.b = cb[pos];
    r.c = cc[pos];
    return r;
}

// Leaves: pool the (ray, chunk) pairs of the lanes that hold a chunk, kChunkTris lanes per pair -- one triangle per lane, records
// read as consecutive 16-byte pieces of three arrays, the ray fetched from LDS, the reference's intersect_triangle unchanged --
// and a hit goes to its ray's entry of `best` with one LDS atomic min.  When the wave has run its rounds, a lane that took part
// -- it waited at a chunk (lf) or held one aside -- calls after(lf): its entry of `best` is then the key after those rounds.
// after(lf) does what the kernel makes of that key and must end in chunk_leaf_retire(L, lf, ...).  (Why a callable and not a
// returned flag: profiles/r34_chunk_walk_shared.txt.)
// AHEAD: the next round's ray records and triangle pieces are requested before this round's are tested (the render and radiance
// kernels).  RANK: the key's low word is the triangle's rank in the reference's visit order, so that the minimum is the
// reference's strict `t < closest` in visit order; without it the word stays zero (any hit: the bound is the ray lane's, which
// compares after the round).
template <bool AHEAD, bool RANK, bool STATS, class After>
DEV void chunk_leaf_phase(const KParams& p, const ChunkLds& w, uint32_t lane, f3 o, f3 d, const ChunkLane L, Tally<STATS>& tl, After after) {
    const bool lf = L.state == kChunkWalk && L.cur != kChunkNone && (L.cur & kChunkLeaf) != 0u;   // waits at a chunk
    const bool lp = L.state == kChunkWalk && L.pend != kChunkNone;                                // holds one aside
    const unsigned long long m = __ballot(lf), mp = __ballot(lp);
    const uint32_t n_pend = (uint32_t)__popcll(mp), n_units = n_pend + (uint32_t)__popcll(m);
    const uint32_t n_node = (uint32_t)__popcll(__ballot(L.state == kChunkWalk && L.cur != kChunkNone && !lf));
    if (!(n_units != 0u && (n_units >= (uint32_t)RB_CHUNK_LEAF_LANES || n_node == 0u))) return;
    const unsigned long long below = (1ull << lane) - 1ull;
    if (lp) w.units[(uint32_t)__popcll(mp & below)] = lane;
    if (lf) w.units[n_pend + (uint32_t)__popcll(m & below)] = lane | 64u;
    if (lf || lp) {
        const v4f r0 = {o.x, o.y, o.z, __uint_as_float(L.pend)}, r1 = {d.x, d.y, d.z, __uint_as_float(L.cur)};
        w.rayrec[lane * 2u] = r0;
        w.rayrec[lane * 2u + 1u] = r1;
        w.best[lane] = L.key;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const cf4p ca = (cf4p)p.chunk_a, cb = (cf4p)p.chunk_b, cc = (cf4p)p.chunk_c;
    constexpr uint32_t kPairsPerRound = 64u / kChunkTris;
    ChunkRound nx;
    if constexpr (AHEAD) nx = chunk_fetch(ca, cb, cc, w, lane, 0u, n_units);
#pragma unroll 1
    for (uint32_t g0 = 0; g0 < n_units; g0 += kPairsPerRound) {
        ChunkRound r;
        if constexpr (AHEAD) {
            r = nx;
            if (g0 + kPairsPerRound < n_units) nx = chunk_fetch(ca, cb, cc, w, lane, g0 + kPairsPerRound, n_units);
        } else {
            r = chunk_fetch(ca, cb, cc, w, lane, g0, n_units);
        }
        if constexpr (STATS) tl.tris += r.valid ? 1u : 0u;
        float u, v;
        const float t = isect_triangle(mk(r.r0.x, r.r0.y, r.r0.z), mk(r.r1.x, r.r1.y, r.r1.z), mk(r.a.x, r.a.y, r.a.z),
                                       mk(r.b.x, r.b.y, r.b.z), mk(r.c.x, r.c.y, r.c.z), u, v);
        if (r.valid && t > 0.001f) {
            unsigned long long k = (unsigned long long)__float_as_uint(t) << 32;
            if constexpr (RANK) k |= __float_as_uint(r.a.w);
            __hip_atomic_fetch_min(&w.best[r.rl], k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            if constexpr (STATS) tl.mesh_hits++;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lf || lp) after(lf);
}

// After a round, for a lane that took part (lf || lp): the chunk the lane stood at is done (lf), or there was nothing left to
// walk -- pop, or the walk is complete.
DEV ChunkLane chunk_leaf_retire(ChunkLane L, bool lf, uint32_t* stack, uint32_t stride) {
    L.pend = kChunkNone;
    if (L.state == kChunkWalk && (lf || L.cur == kChunkNone)) {
        if (L.sp == 0) {
            L.state = kChunkDone;
        } else {
            L.sp--;
            L.cur = stack[L.sp * stride];
        }
    }
    chunk_set_aside(L, stack, stride);
    return L;
}

// A complete walk's hit: (t, u, v) of the winner again from its prepared record, the same operations on the same values
DEV TriHit chunk_winner(const KParams& fp, f3 o, f3 d, unsigned long long key) {
    TriHit th;
    th.hit = key != kChunkNoHit;
    th.t = 1e20f;
    th.u = th.v = 0.0f;
    th.slot = 0u;
    if (th.hit) {
        th.slot = cptr(fp.chunk_rank_slot)[(uint32_t)key];
        const cf4p tp = (cf4p)fp.ptris + (size_t)th.slot * 4u;
        const v4f a = tp[0], b = tp[1], c = tp[2];
        th.t = isect_triangle(o, d, mk(a.x, a.y, a.z), mk(b.x, b.y, b.z), mk(c.x, c.y, c.z), th.u, th.v);
    }
    return th;
}

}  // namespace
}  // namespace rb
